"""The footprint helper (tests/footprint.py) without a GPU: it reports what it should, its masks
match what the oracle's reference functions write, and every device entry of the ctypes table
has a row in tests/test_gpu_footprint.py or a stated reason not to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import footprint as fp
from conftest import ROOT, load_package


# ------------------------------------------------------------------ 1. the helper can fail
def _two(carve):
    """the same carve on both fills: [(arena, buffers)] * 2"""
    out = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill, capacity=1 << 20)
        out.append((ar, carve(ar)))
    return out


def _check(runs, masks, entry):
    """entry(host bytes, buffers) plays the device entry on a copy of each arena"""
    afters = []
    for ar, bufs in runs:
        after = ar.bytes().copy()
        entry(after, bufs)
        afters.append(after)
    (a1, b1), (a2, _) = runs
    fp.check_arena(a1, afters[0], a2, afters[1], {b.name: m for b, m in zip(b1, masks)})


def _carve(ar):
    return [ar.list("out", (5, 3), np.int32), ar.plane("dst", 2, 16, 16, np.uint16)]


def _good(host, bufs):
    lst, pl = bufs
    lst.data(host)[...] = np.arange(15).reshape(5, 3)
    pl.picture(host)[...] = 7


def test_standin_passes():
    runs = _two(_carve)
    lst, pl = runs[0][1]
    _check(runs, [lst.mask(), fp.hpel_mask(pl)], _good)


def _poke(where):
    def entry(host, bufs):
        _good(host, bufs)
        lst, pl = bufs
        g = pl.guard_rows
        if where == "list_end":
            lst.np(host)[lst.guard + lst.n] = 1
        elif where == "row_below":
            pl.np(host)[1, g + pl.rows, 40] = 1
        elif where == "slack":
            pl.np(host)[0, g + 5, pl.width + 64] = 1
        elif where == "gap":
            pl.np(host)[0, pl.frame_rows - 1, 3] = 1
        elif where == "list_before":
            lst.np(host)[lst.guard - 1] = 1
    return entry


@pytest.mark.parametrize("where,coords", [
    ("list_end", "(5, 0)"), ("list_before", "(-1, 2)"), ("row_below", "(1, 48, 8)"), ("slack", "(0, -27, 48)"),
    ("gap", "(0, 66, -29)")])
def test_standin_overrun_is_named(where, coords):
    runs = _two(_carve)
    lst, pl = runs[0][1]
    with pytest.raises(AssertionError, match="outside the footprint") as e:
        _check(runs, [lst.mask(), fp.hpel_mask(pl)], _poke(where))
    assert coords in str(e.value), str(e.value)
    assert ("out:" if where.startswith("list") else "dst:") in str(e.value)


def test_standin_unwritten_is_named():
    def entry(host, bufs):
        _good(host, bufs)
        bufs[1].picture(host)[1, 3, 9] = fp.fill_value(np.uint16, host[0])     # left as the arena had it
        bufs[0].data(host)[4, 1] = fp.fill_value(np.int32, host[0])
    runs = _two(_carve)
    lst, pl = runs[0][1]
    with pytest.raises(AssertionError, match="not written") as e:
        _check(runs, [lst.mask(), fp.hpel_mask(pl)], entry)
    assert "(4, 1)" in str(e.value)
    with pytest.raises(AssertionError, match="not written") as e:
        _check(runs, [lst.mask(), fp.hpel_mask(pl)],
               lambda h, b: (_good(h, b), entry(h, b), b[0].data(h).__setitem__((4, 1), 1)))
    assert "(1, -29, -23)" in str(e.value)


def test_standin_input_must_come_back():
    """a buffer that is no output is an input: writing it is reported as well"""
    def carve(ar):
        return [ar.list("in", 8, np.int16, np.arange(8)), ar.list("out", 8, np.int16)]

    def entry(host, bufs):
        bufs[1].data(host)[...] = 3
        bufs[0].data(host)[2] = 99
    runs = _two(carve)
    with pytest.raises(AssertionError, match=r"in: 1 element.*\(2, 0\)"):
        _check(runs, [runs[0][1][0].none(), runs[0][1][1].mask()], entry)


def test_shrunk_mask_fails():
    """one row less in the mask than the entry writes: reported at that row"""
    runs = _two(_carve)
    lst, pl = runs[0][1]
    m = fp.hpel_mask(pl)
    m[:, pl.guard_rows + pl.rows - 1] = False
    with pytest.raises(AssertionError, match=r"outside the footprint.*\(0, 47, -32\)"):
        _check(runs, [lst.mask(), m], _good)


def test_alignment_and_geometry():
    ar = fp.Arena(fp.FILLS[0], capacity=1 << 20)
    a = ar.list("a", (3, 4), np.int32)
    p = ar.plane("p", 2, 48, 16, np.uint8)
    q = ar.plane("q", 2, 48, 16, np.uint8, extra=4)
    assert a.start % 4096 == 0 and (a.start + a.guard * 4) % 16 == 0
    assert p.stride == fp.plane_stride(48) + 64 and q.stride == p.stride + 4
    assert p.frame_stride == (16 + 64 + 32 + 3) * p.stride != (16 + 64) * p.stride
    assert (p.start + p.origin) % 16 == 0 and p.stride % 16 == 0
    assert (q.start + q.origin) % 16 == 0 and q.stride % 16 == 4          # rows only dword-aligned
    t = fp.Arena(fp.FILLS[0], fp.TIGHT, capacity=1 << 20).plane("p", 2, 48, 16, np.uint8)
    assert t.stride == fp.plane_stride(48) and t.frame_stride == 80 * t.stride and t.origin == 32 * t.stride + 32


# ------------------------------------------------------------------ 2. the masks match the oracle
def _oracle_runs(carve, call):
    """carve(arena) -> buffers; call(host, buffers) runs the oracle into the arena.  Returns
    (buffers of run 1, after1, after2) after checking every byte outside the buffers."""
    res = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill, capacity=4 << 20)
        bufs = carve(ar)
        before = ar.bytes().copy()
        call(ar.host, bufs)
        res.append((ar, bufs, before, ar.bytes().copy()))
    return res


def _exact(res, name, mask, extra=None):
    """the oracle's writes into buffer `name` are exactly `mask` (plus `extra`, scratch rows the
    mask function lists), and both runs agree inside the mask"""
    (a1, b1, _, h1), (_, _, _, h2) = res
    buf = {b.name: b for b in b1}[name]
    w = fp.written(buf.np(h1), buf.np(h2), buf)
    if extra is not None:
        w &= ~extra
    over, under = w & ~mask, mask & ~w
    assert not over.any(), (name, "oracle writes outside the mask", [buf.coords(i) for i in np.argwhere(over)[:4]])
    assert not under.any(), (name, "mask elements the oracle leaves", [buf.coords(i) for i in np.argwhere(under)[:4]])
    agree = (buf.np(h1) == buf.np(h2)) | ~mask
    assert agree.all(), (name, "depends on guard bytes", [buf.coords(i) for i in np.argwhere(~agree)[:4]])


def _inputs_kept(res, names):
    for ar, bufs, before, after in res:
        for b in bufs:
            if b.name in names:
                assert np.array_equal(b.np(before), b.np(after)), b.name


def _pix(rs, bd, shape):
    return rs.integers(0, 1 << bd, shape).astype(np.uint8 if bd == 8 else np.uint16)


def _a(buf, host, off=0):
    """address of element `off` of a buffer's region"""
    return C.c_void_p(host.ctypes.data + buf.start + int(off) * buf.dtype.itemsize)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("W,H", [(16, 16), (48, 32)])
def test_oracle_hpel_mask(oracle, bd, extra, W, H):
    rs = np.random.default_rng(W + bd)
    pdt = oracle.pixel_dtype(bd)
    src = _pix(rs, bd, (2, H + 64, W + 64))

    def carve(ar):
        return [ar.plane("src", 2, W, H, pdt, src, extra=extra)] + \
               [ar.plane(n, 2, W, H, pdt, extra=extra) for n in "hvc"]

    def call(host, bufs):
        s = bufs[0]
        for f in range(2):
            o = s.origin + f * s.frame_stride
            oracle.fn(bd, "frame_filter")(_a(s, host, o), *[_a(b, host, o) for b in bufs[1:]], s.stride, W, H)
    res = _oracle_runs(carve, call)
    for n in "hvc":
        buf = {b.name: b for b in res[0][1]}[n]
        _exact(res, n, fp.hpel_mask(buf))
    _inputs_kept(res, {"src"})


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("W,H", [(48, 34), (48, 32), (72, 40), (136, 18)])
def test_oracle_lowres_mask(oracle, bd, W, H):
    rs = np.random.default_rng(W + bd)
    pdt = oracle.pixel_dtype(bd)
    src = _pix(rs, bd, (2, H + 64, W + 64))

    def carve(ar):
        return [ar.plane("src", 2, W, H, pdt, src)] + [ar.plane("l%d" % k, 2, W // 2, H // 2, pdt) for k in range(4)]

    def call(host, bufs):
        s, d = bufs[0], bufs[1]
        for f in range(2):
            ptrs = (C.c_void_p * 4)(*[_a(b, host, b.origin + f * b.frame_stride).value for b in bufs[1:]])
            oracle.fn(bd, "frame_init_lowres")(_a(s, host, s.origin + f * s.frame_stride), s.stride, W, H, ptrs,
                                               d.stride)
    res = _oracle_runs(carve, call)
    for b in res[0][1][1:]:
        _exact(res, b.name, fp.lowres_mask(b))
    _inputs_kept(res, {"src"})


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("width", [8, 9, 24, 25, 1032])
def test_oracle_weight_scale_mask(oracle, bd, width):
    """the plane holds the width x 3 region at its top-left padding pixel, as the lookahead calls it"""
    rs = np.random.default_rng(width)
    pdt = oracle.pixel_dtype(bd)
    px = 32 if width > 64 else 0
    W, H = fp.weight_scale_cols(width) - 2 * px, 3        # the strips read src as far as they write dst
    pic = _pix(rs, bd, (2, H, W + 2 * px))

    def carve(ar):
        kw = dict(pad_x=px, pad_y=0, stride=fp.plane_stride(width, 0) + 64)
        return [ar.plane("src", 2, W, H, pdt, pic, **kw),
                ar.plane("dst", 2, W, H, pdt, **kw)]

    for scale, denom, offset in ((40, 5, -6), (1, 0, 3)):
        def call(host, bufs):
            s, d = bufs
            for f in range(2):
                o = s.origin - px + f * s.frame_stride
                oracle.fn(bd, "weight_scale_plane")(_a(d, host, o), d.stride, _a(s, host, o), s.stride, width, H, scale,
                                                    denom, offset)
        res = _oracle_runs(carve, call)
        _exact(res, "dst", fp.weight_scale_mask(res[0][1][1], -px, 0, width, H))
        _inputs_kept(res, {"src"})
    assert [fp.weight_scale_cols(w) for w in (8, 9, 24, 25, 1032)] == [8, 16, 24, 32, 1032]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("sub8x8", [0, 1])
@pytest.mark.parametrize("lines,padh,W", [(16, 32, 48), (48, 64, 48), (16, 32, 100)])
def test_oracle_integral_mask(oracle, bd, sub8x8, lines, padh, W):
    rs = np.random.default_rng(lines + bd)
    pdt = oracle.pixel_dtype(bd)

    def carve(ar):
        s = ar.plane("src", 2, W, lines, pdt, pad_x=padh)
        s.np(ar.host)[:, s.guard_rows:s.guard_rows + s.rows] = _pix(np.random.default_rng(lines), bd,
                                                                    (2, s.rows, s.stride))      # whole rows
        return [s, ar.plane("sum", 2, W, lines, np.uint16, pad_x=padh, stride=s.stride,
                            rows=(lines + 64) * (2 if sub8x8 else 1))]

    def call(host, bufs):
        s, d = bufs
        for f in range(2):
            oracle.fn(bd, "frame_integral")(_a(s, host, s.origin + f * s.frame_stride), s.stride, lines, padh, sub8x8,
                                            _a(d, host, d.origin + f * d.frame_stride))
    res = _oracle_runs(carve, call)
    mask, scratch = fp.integral_masks(res[0][1][1], lines, padh, sub8x8)
    _exact(res, "sum", mask, extra=scratch)
    _inputs_kept(res, {"src"})


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("transform", [4, 8])
@pytest.mark.parametrize("mbw,mbh", [(1, 1), (17, 3)])
def test_oracle_recon_mask(oracle, bd, transform, mbw, mbh):
    rs = np.random.default_rng(mbw + bd)
    pdt, cdt = oracle.pixel_dtype(bd), oracle.coef_dtype(bd)
    W, H = 16 * mbw, 16 * mbh
    n = mbw * mbh
    dq4, dq8 = oracle.cqm_dequant([[16] * 16] * 4 + [[16] * 64] * 4)
    dmf = np.ascontiguousarray(dq8[1] if transform == 8 else dq4[1])

    coefs, qps, pic = rs.integers(-40, 40, (2 * n, 256)), rs.integers(10, 40, 2 * n), _pix(rs, bd, (2, H + 64, W + 64))

    def carve(ar):
        return [ar.list("dct", (2 * n, 256), cdt, coefs), ar.list("qp", 2 * n, np.int32, qps),
                ar.plane("pred", 2, W, H, pdt, pic), ar.plane("recon", 2, W, H, pdt)]

    def call(host, bufs):
        d, q, p, r = bufs
        for f in range(2):
            oracle.fn(bd, "mb_dequant_idct_add")(transform, _a(d, host, d.guard + f * n * 256), mbw, mbh,
                                                 C.c_void_p(dmf.ctypes.data), _a(q, host, q.guard + f * n),
                                                 _a(p, host, p.origin + f * p.frame_stride), p.stride,
                                                 _a(r, host, r.origin + f * r.frame_stride), r.stride)
    res = _oracle_runs(carve, call)
    _exact(res, "recon", fp.recon_mask(res[0][1][3], mbw, mbh))
    _inputs_kept(res, {"dct", "qp", "pred"})


@pytest.mark.parametrize("bd", [8, 10])
def test_oracle_block_list_masks(oracle, bd):
    """add_idct_list and zigzag_sub: the destination blocks, the n outputs, nothing past item n - 1"""
    rs = np.random.default_rng(bd)
    pdt, cdt = oracle.pixel_dtype(bd), oracle.coef_dtype(bd)
    stride, rows, n = 96, 40, 65
    for kind in range(7):
        w, sz = oracle.IDCT_W[kind], oracle.IDCT_IN[kind]
        cells = [(y, x) for y in range(0, rows - w + 1, w) for x in range(0, stride - w + 1, w)]
        n = min(65, len(cells))
        offs = np.array([cells[i][0] * stride + cells[i][1] for i in rs.permutation(len(cells))[:n]], np.int64)
        plane =_pix(rs, bd, stride * rows)
        coefs = rs.integers(-300, 300, (n + 16, sz))
        res = []
        for fill in fp.FILLS:
            ar = fp.Arena(fill, capacity=1 << 20)
            d = ar.list("dst", stride * rows, pdt, plane)
            o = ar.list("off", n + 16, np.int64, np.concatenate([offs, np.full(16, 1 << 40)]))   # items past n: unread
            c = ar.list("dct", (n + 16, sz), cdt, coefs)
            after = ar.bytes().copy()
            oracle.fn(bd, "add_idct_list")(kind, _a(d, after, d.guard), stride, _a(o, after, o.guard),
                                           _a(c, after, c.guard), n)
            res.append((ar, after))
        # in place: outside the blocks the plane keeps its pixels; "dct is not modified"
        fp.check_arena(res[0][0], res[0][1], res[1][0], res[1][1],
                       {"dst": fp.blocks_mask(res[0][0].bufs[0], offs, w, w, stride)})
    n = 65
    for kind in (0, 1, 2):
        w = 8 if kind == 2 else 4
        cells = [(y, x) for y in range(0, rows - w + 1, w) for x in range(0, stride - w + 1, w)]
        n = min(65, len(cells))
        do = np.array([cells[i][0] * stride + cells[i][1] for i in rs.permutation(len(cells))[:n]], np.int64)
        so = rs.integers(0, stride * (rows - 8) - 8, n).astype(np.int64)
        res = []
        for fill in fp.FILLS:
            ar = fp.Arena(fill, capacity=1 << 20)
            src = ar.list("src", stride * rows, pdt, _pix(np.random.default_rng(3), bd, stride * rows))
            dst = ar.list("dst", stride * rows, pdt, _pix(np.random.default_rng(4), bd, stride * rows))
            level = ar.list("level", (n + 16, w * w), cdt)
            dc = ar.list("dc", n + 16, cdt)
            after = ar.bytes().copy()
            base = after.ctypes.data

            def at(b, i=0):
                return C.c_void_p(int(base + b.start + (b.guard + int(i)) * b.dtype.itemsize))
            for i in range(n):
                oracle.fn(bd, "zigzag_sub_s")(kind, 0, at(level, i * w * w), at(src, so[i]), stride, at(dst, do[i]),
                                              stride, at(dc, i))
            res.append((ar, after))
        a1 = res[0][0]
        masks = {"dst": fp.blocks_mask(a1.bufs[1], do, w, w, stride), "level": a1.bufs[2].items(n)}
        if kind == 1:
            masks["dc"] = a1.bufs[3].items(n)         # "dc[i] (4x4ac only)"
        fp.check_arena(a1, res[0][1], res[1][0], res[1][1], masks)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("rng", [4, 8])
@pytest.mark.parametrize("mbw,mbh", [(1, 1), (3, 1), (5, 2)])
def test_oracle_table_masks(oracle, bd, rng, mbw, mbh):
    """me_search_full, me_search_full8, me_search_centred: the oracle fills its whole table (which
    has no padding entries: the exception table_mask lists) and `origin`, and nothing after"""
    rs = np.random.default_rng(bd + rng)
    pdt, sdt = oracle.pixel_dtype(bd), oracle.sad_dtype(bd)
    W, H, w = 16 * mbw, 16 * mbh, 2 * rng + 1
    n = mbw * mbh
    pw = (2 * rng + (6 if bd == 8 else 4) + 3) // 4 * 4
    centre = np.stack([rs.integers(-40, 40, n), rs.integers(-40, 40, n)], 1).astype(np.int16)
    centre[0] = (-60, -60)
    centre[-1] = (60, 60)
    res = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill, capacity=4 << 20)
        r2 = np.random.default_rng(1)
        fenc = ar.plane("fenc", 1, W, H, pdt, _pix(r2, bd, (1, H + 64, W + 64)))
        ref = ar.plane("ref", 1, W, H, pdt, _pix(r2, bd, (1, H + 64, W + 64)))
        cen = ar.list("centre", (n, 2), np.int16, centre)
        t16 = ar.list("table", (n, w, w), sdt)
        t8 = ar.list("table8", (n, 4, w, w), np.uint16)
        tc = ar.list("tablec", (n, w, pw), sdt)
        org = ar.list("origin", (n, 2), np.int16)
        after = ar.bytes().copy()
        base = after.ctypes.data

        def at(b, off):
            return C.c_void_p(base + b.start + int(off) * b.dtype.itemsize)
        common = (at(fenc, fenc.origin), fenc.stride, at(ref, ref.origin), ref.stride, mbw, mbh, rng)
        oracle.fn(bd, "me_search_full")(*common, at(t16, t16.guard))
        oracle.fn(bd, "me_search_full8")(*common, at(t8, t8.guard))
        oracle.fn(bd, "me_search_centred")(*common, at(cen, cen.guard), at(tc, tc.guard), at(org, org.guard))
        res.append((ar, after))
    a1 = res[0][0]
    fp.check_arena(a1, res[0][1], res[1][0], res[1][1],
                   {b.name: fp.table_mask(b) for b in a1.bufs if b.name in ("table", "table8", "tablec", "origin")})


# ------------------------------------------------------------------ 3. the entry list is complete
def _stream_entries():
    """every entry of the ctypes tables whose prototype ends in `void *stream`"""
    x = load_package()
    protos = {}
    for header, pat in (("x264hip.h", r"\bint\s+x264hip_(?:##BD##_)?(\w+)\(([^;]*?)\);"),
                        ("x264hip_mbtree.h", r"\bint\s+x264hip_mbtree_(\w+)\(([^;]*?)\);"),
                        ("x264hip_mc.h", r"\bint\s+x264hip_(?:8|10)_(\w+?)\s*\(([^;]*?)\);")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for name, params in re.findall(pat, text, re.S):
            protos.setdefault((header, name), params)
    out = []
    for name in x._PER_DEPTH:
        if "void *stream" in protos.get(("x264hip.h", name), ""):         # (the void initialisers: no stream)
            out.append(name)
    for name in x._PLAIN:
        if "void *stream" in protos.get(("x264hip.h", name), ""):
            out.append(name)
    for name in x._MC:
        assert "void *stream" in protos[("x264hip_mc.h", name)]
        out.append(name)
    for name in x._MBTREE:
        assert "void *stream" in protos[("x264hip_mbtree.h", name)]
        out.append("mbtree_" + name)
    return out


def test_every_stream_entry_has_a_row_or_a_reason():
    import test_gpu_footprint as g
    entries = _stream_entries()
    assert len(entries) > 60 and "hpel_filter" in entries and "mbtree_finish" in entries and "upload_planes" in entries
    covered = {e for row in g.ROWS for e in row.entries}
    reasons = dict(g.EXCLUDED)
    assert not covered & set(reasons), sorted(covered & set(reasons))
    missing = [e for e in entries if e not in covered and e not in reasons]
    assert not missing, "device entries with no footprint row and no stated reason: %s" % missing
    stale = [e for e in list(covered) + list(reasons) if e not in entries]
    assert not stale, "rows or reasons for entries the ctypes table does not have: %s" % stale
    assert all(isinstance(r, str) and len(r) > 10 and "\n" not in r for r in reasons.values())
