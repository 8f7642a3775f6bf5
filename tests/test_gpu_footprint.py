"""Write and read footprints of the device entries (tests/footprint.py has the method).

One row per entry in ROWS.  For every case of a row, at 8 and 10 bit:

a. write footprint -- the call runs on two arenas filled with 0xA5 / 0x5A; outside the masks
   (taken from include/x264hip.h) nothing changes, inputs included, and inside them the two runs
   agree.  Then the wrapper runs once more with its own tight allocation, and the in-mask values
   equal that call's result.
b. oracle equality -- the plane writers also equal the oracle inside the mask, stride-slack
   variant included.
c. read independence -- the inputs hold data only where the header lets the entry read (the
   picture and its 32-pixel padding, items [0, n)); a third run replaces every other byte of the
   arena (guard rows, stride slack, the inter-frame gap, items past n, list guards) by noise and
   must give the outputs of the first bit for bit.  (The two fills of (a) already differ there.)
d. variants -- (a) again under the switches that change the row's store or strip code.

Planes come in two strides where the row is about row alignment (the `extra` of its cases):
plane_stride(W) + 64, which keeps the 16-byte alignment of the streaming kernels, and 4 pixels
more (rows only dword-aligned: the fallback kernels).  The second is left out where the ABI
forbids it, and the row says so: upload_plane / upload_planes want strides that are multiples of
16; frame_integral's row is the whole stride, whose column-per-lane kernel X264HIP_INTEGRAL_VARIANT
selects instead.  Every other plane has the stride slack, the guard rows and the inter-frame gap.
"""
import types

import numpy as np
import pytest

import footprint as fp

pytestmark = pytest.mark.gpu

ROWS = []
# entries that take a stream and have no row here, with the reason
EXCLUDED = {
    "mb_mc": "has its own footprint test, test_gpu_mbmc.py::test_untouched_pixels_and_strides",
    "lowres_inter_cost": "shares lowres_inter_cost_ex's launcher; the _ex form is tested",
    "lowres_bidir_cost": "shares lowres_bidir_cost_ex's launcher; the _ex form is tested",
    "forward_ref": "a hipMemcpyPeerAsync of `bytes` bytes between two devices; no kernel of the library",
    "upload": "flat copy of `bytes` bytes; test_gpu_runtime.py::test_upload_from_pinned checks both ends of it",
    "stream_destroy": "takes a stream to release, no device buffer",
    "lowres_status": "waits for the stream and reports; no device buffer of the caller's",
}

STREAM_VARIANTS = [("X264HIP_STREAM_NT", 0), ("X264HIP_STREAM_NT", 1), ("X264HIP_STREAM_XCD", 1),
                   ("X264HIP_STREAM_XCD", 2)]
ME_VARIANTS = [("X264HIP_ME_XCD", 0), ("X264HIP_ME_XCD", 1)]


def pdt(bd):
    return np.uint8 if bd == 8 else np.uint16


def cdt(bd):
    return np.int16 if bd == 8 else np.int32


def udt(bd):
    return np.uint16 if bd == 8 else np.uint32


def sdt(bd):
    return np.uint16 if bd == 8 else np.uint32


def pix(seed, bd, shape):
    return np.random.default_rng(seed).integers(0, 1 << bd, shape).astype(pdt(bd))


class Row:
    """name: the id; entries: the ABI entries (without x264hip_{8,10}_) the row covers;
    cases: list of (id, dict); setup(ar, bd, **case) -> namespace of buffers (carved identically
    on every arena); call(hip, c, dev, tight) -> None, or with tight the wrapper's own outputs
    {buffer name: tensor}; masks(c) -> {buffer name: mask} (+ optional maybe(c));
    oracle(orc, c, host) -> {buffer name: expected whole region} or None; variants: switches."""

    def __init__(self, name, entries, cases, setup, call, masks, oracle=None, variants=(), maybe=None,
                 variant_case=None):
        self.name, self.entries, self.cases, self.setup, self.call, self.masks = name, entries, cases, setup, call, masks
        self.oracle, self.variants, self.maybe = oracle, list(variants), maybe
        self.variant_case = variant_case or (lambda bd, case: True)
        ROWS.append(self)


def pytest_generate_tests(metafunc):
    if "row" in metafunc.fixturenames:          # (runs once the whole module, ROWS included, is imported)
        metafunc.parametrize("row,case,bd,var", _params())


def _params():
    out = []
    for row in ROWS:
        for cid, case in row.cases:
            for bd in (8, 10):
                for var in [None] + row.variants:
                    if var is not None and not row.variant_case(bd, case):
                        continue
                    vid = "" if var is None else "-%s=%d" % (var[0].replace("X264HIP_", ""), var[1])
                    out.append(pytest.param(row, case, bd, var, id="%s-%s-%d%s" % (row.name, cid, bd, vid)))
    return out


def _run(hip, row, bd, case, ar, noise=None):
    """carve and fill `ar`, run the row's call on its bytes on the device; (ctx, bytes after)"""
    import torch
    c = row.setup(ar, bd, **case)
    if noise is not None:
        keep = np.zeros(ar.used, bool)
        for b in ar.bufs:
            keep[b.start:b.start + b.nbytes] = np.repeat(b.readable.ravel(), b.dtype.itemsize)
        junk = np.random.default_rng(noise).integers(0, 256, ar.used, dtype=np.uint8)
        ar.bytes()[~keep] = junk[~keep]
    dev = ar.device()
    try:
        row.call(hip, c, dev, False)
        torch.cuda.synchronize()
        return c, dev.cpu().numpy()
    except RuntimeError as e:
        if "illegal memory access" in str(e) or "hipError" in str(e):
            pytest.exit("GPU fault in %s: %s" % (row.name, e), returncode=3)    # nothing more runs on this device
        raise


def test_footprint(hip, oracle, row, case, bd, var):
    import torch
    if var is not None:
        hip.set_variant(*var)
    a1, a2 = fp.Arena(fp.FILLS[0]), fp.Arena(fp.FILLS[1])
    c1, after1 = _run(hip, row, bd, case, a1)
    c2, after2 = _run(hip, row, bd, case, a2)
    masks = row.masks(c1)
    fp.check_arena(a1, after1, a2, after2, masks, row.maybe(c1) if row.maybe else None)
    by_name = {b.name: b for b in a1.bufs}
    maybe = row.maybe(c1) if row.maybe else {}

    def inside(name, region):
        m = masks[name] & ~maybe[name] if name in maybe else masks[name]
        return region[m]
    # a. the wrapper's own tight allocation gives the same in-mask values
    at = fp.Arena(fp.FILLS[0], fp.TIGHT)
    ct = row.setup(at, bd, **case)
    dev = at.device()
    own = row.call(hip, ct, dev, True)
    torch.cuda.synchronize()
    tmasks, tmaybe = row.masks(ct), (row.maybe(ct) if row.maybe else {})
    tb = {b.name: b for b in at.bufs}
    for name, t in (own or {}).items():
        got = t.contiguous().cpu().numpy().view(tb[name].dtype).ravel()
        got = np.concatenate([got, np.zeros(tb[name].np(at.bytes()).size - got.size, got.dtype)]).reshape(tb[name].shape)
        m = tmasks[name] & ~tmaybe[name] if name in tmaybe else tmasks[name]
        want = inside(name, by_name[name].np(after1))
        assert np.array_equal(got[m], want), (name, "differs from the wrapper's own allocation")
    # b. the oracle, inside the mask
    if row.oracle is not None and var is None:
        for name, want in row.oracle(oracle, c1, a1.bytes()).items():
            want, where = want if isinstance(want, tuple) else (want, masks[name])
            got = by_name[name].np(after1)
            bad = (got != want) & masks[name] & where
            assert not bad.any(), (name, "differs from the oracle", [by_name[name].coords(i)
                                                                      for i in np.argwhere(bad)[:4]])
    # c. read independence
    if var is None:
        a3 = fp.Arena(fp.FILLS[0])
        _, after3 = _run(hip, row, bd, case, a3, noise=7)
        for name in masks:
            b = by_name[name]
            bad = (b.np(after3) != b.np(after1)) & masks[name]
            if name in maybe:
                bad &= ~maybe[name]
            assert not bad.any(), (name, "depends on bytes outside what the entry may read",
                                   [b.coords(i) for i in np.argwhere(bad)[:4]])


def T(buf, dev):
    """the payload of a list / the whole region of a plane as a tensor"""
    return buf.dt(dev) if isinstance(buf, fp.ListBuf) else buf.t(dev)


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ------------------------------------------------------------------ hpel_filter
def _hpel_setup(ar, bd, W, H, extra):
    src = ar.plane("src", 2, W, H, pdt(bd), pix(W + H, bd, (2, H + 64, W + 64)), extra=extra)
    return _ns(W=W, H=H, bd=bd, src=src, outs=[ar.plane(n, 2, W, H, pdt(bd), extra=extra) for n in "hvc"])


def _hpel_call(hip, c, dev, tight):
    outs = hip.hpel_filter(c.src.t(dev), c.src.origin, c.src.stride, c.W, c.H,
                           outs=None if tight else [o.t(dev) for o in c.outs])
    return dict(zip("hvc", outs)) if tight else None


def _hpel_oracle(orc, c, host):
    out = {}
    s = c.src.np(host)
    res = [orc.frame_filter(c.bd, s[f].ravel().copy(), c.src.origin, c.src.stride, c.W, c.H) for f in range(2)]
    for k, o in enumerate(c.outs):
        out[o.name] = np.stack([res[f][k].reshape(s[f].shape) for f in range(2)])
    return out


Row("hpel_filter", ("hpel_filter",),
    # W 976: (np - 1) % 64 == 0, the stream kernel; 992: strip7's second wave holds two pieces; 16, 48:
    # ragged 64-wide tiles of the fused kernel; H 16 / 32: (H + 16) / 12 ragged and exact
    [("%dx%d%s" % (W, H, "+4" if e else ""), dict(W=W, H=H, extra=e))
     for W in (16, 48, 976, 992) for H in (16, 32) for e in (0, 4)],
    _hpel_setup, _hpel_call, lambda c: {o.name: fp.hpel_mask(o) for o in c.outs}, _hpel_oracle,
    # (the switches act on the streaming kernels only: 8 bit, 16-byte aligned rows)
    variants=STREAM_VARIANTS, variant_case=lambda bd, case: bd == 8 and not case["extra"])


# ------------------------------------------------------------------ frame_init_lowres
def _lowres_setup(ar, bd, W, H, extra):
    src = ar.plane("src", 2, W, H, pdt(bd), pix(W * H, bd, (2, H + 64, W + 64)), extra=extra)
    return _ns(W=W, H=H, bd=bd, src=src,
               outs=[ar.plane("l%d" % k, 2, W // 2, H // 2, pdt(bd), extra=extra) for k in range(4)])


def _lowres_call(hip, c, dev, tight):
    if tight:
        outs, _ = hip.frame_init_lowres(c.src.t(dev), c.src.origin, c.src.stride, c.W, c.H)
        return {"l%d" % k: o for k, o in enumerate(outs)}
    hip.frame_init_lowres(c.src.t(dev), c.src.origin, c.src.stride, c.W, c.H, outs=[o.t(dev) for o in c.outs],
                          lowres_stride=c.outs[0].stride, out_origin=c.outs[0].origin)


def _lowres_oracle(orc, c, host):
    s = c.src.np(host)
    o0 = c.outs[0]
    out = {o.name: np.zeros(o.shape, o.dtype) for o in c.outs}
    for f in range(2):
        want = orc.frame_init_lowres(c.bd, s[f].ravel(), c.src.origin, c.src.stride, c.W, c.H, o0.stride)
        for k, o in enumerate(c.outs):
            g = o.guard_rows
            out[o.name][f, g:g + o.rows] = want[k]
    return out


Row("frame_init_lowres", ("frame_init_lowres",),
    # odd hl (34 -> 17, 18 -> 9): the two-rows-per-wave tail; 72 and 136 wide: the dword kernel at 8 bit.
    # The ABI wants dst_stride a multiple of 4 bytes: the +4 stride keeps that.
    [("%dx%d%s" % (W, H, "+4" if e else ""), dict(W=W, H=H, extra=e))
     for W, H in ((48, 34), (48, 32), (72, 40), (136, 18)) for e in (0, 4)],
    _lowres_setup, _lowres_call, lambda c: {o.name: fp.lowres_mask(o) for o in c.outs}, _lowres_oracle,
    # (the switches act on lowres_rows_kernel only: 8 bit, 16-byte aligned rows, a width of whole MBs)
    variants=STREAM_VARIANTS, variant_case=lambda bd, case: bd == 8 and not case["extra"] and case["W"] % 16 == 0)


# ------------------------------------------------------------------ weight_scale_plane
def _wsp_setup(ar, bd, width, weight, extra):
    cols = fp.weight_scale_cols(width)            # the strips read src as far as they write dst
    kw = dict(pad_x=0, pad_y=0, stride=(None if ar.geom is fp.TIGHT else fp.plane_stride(cols, 0) + 64 + extra))
    src = ar.plane("src", 2, cols, 3, pdt(bd), pix(width, bd, (2, 3, cols)), **kw)
    return _ns(bd=bd, width=width, weight=weight, src=src, dst=ar.plane("dst", 2, cols, 3, pdt(bd), **kw))


def _wsp_call(hip, c, dev, tight):
    # the C entry itself: the wrapper serves whole padded lowres planes only (width + 64 columns)
    s, d = c.src.t(dev), c.dst.t(dev)
    es = s.element_size()
    f = getattr(hip.lib(), "x264hip_%d_weight_scale_plane" % c.bd)
    hip._rc(f(d.data_ptr() + c.dst.origin * es, c.dst.stride, c.dst.frame_stride, s.data_ptr() + c.src.origin * es,
              c.src.stride, c.src.frame_stride, c.width, 3, 2, *c.weight, hip._stream()), "weight_scale_plane")
    return {"dst": d} if tight else None


def _wsp_oracle(orc, c, host):
    want = c.dst.np(host).copy()
    s = c.src.np(host)
    for f in range(2):
        flat = want[f].reshape(-1)
        orc.weight_scale_plane(c.bd, s[f].ravel(), c.src.origin, c.src.stride, c.width, 3, *c.weight, dst=flat)
    return {"dst": want}


Row("weight_scale_plane", ("weight_scale_plane",),
    # widths 8, 9, 24, 25: both branches of the strip rounding; 1032: the second 1024-column block
    [("w%d-%s%s" % (w, "a" if wt[0] == 40 else "b", "+4" if e else ""), dict(width=w, weight=wt, extra=e))
     for w in (8, 9, 24, 25, 1032) for wt in ((40, 5, -6), (1, 0, 3)) for e in (0, 4)],
    _wsp_setup, _wsp_call, lambda c: {"dst": fp.weight_scale_mask(c.dst, 0, 0, c.width, 3)}, _wsp_oracle)


# ------------------------------------------------------------------ frame_integral
def _integral_setup(ar, bd, lines, padh, sub8x8, W):
    # (one stride on every arena: the integral of a row is a function of the whole stride)
    src = ar.plane("src", 2, W, lines, pdt(bd), pad_x=padh, stride=fp.plane_stride(W, padh) + 64)
    g = src.guard_rows
    src.np(ar.host)[:, g:g + src.rows] = pix(lines + W, bd, (2, src.rows, src.stride))   # the row is the whole stride
    src.readable[:, g:g + src.rows] = True
    out = ar.plane("sum", 2, W, lines, np.uint16, pad_x=padh, stride=src.stride,
                   rows=(lines + 64) * (2 if sub8x8 else 1))
    return _ns(bd=bd, lines=lines, padh=padh, sub8x8=sub8x8, src=src, out=out)


def _integral_call(hip, c, dev, tight):
    out = hip.frame_integral(c.src.t(dev), c.src.origin, c.src.stride, c.lines, c.padh, c.sub8x8,
                             out=None if tight else c.out.t(dev), out_origin=None if tight else c.out.origin)
    return {"sum": out} if tight else None


def _integral_oracle(orc, c, host):
    s = c.src.np(host)
    want = np.zeros(c.out.shape, np.uint16)
    g = c.out.guard_rows
    for f in range(2):
        want[f, g:g + c.out.rows] = orc.frame_integral(c.bd, s[f].ravel(), c.src.origin, c.src.stride, c.lines,
                                                       c.padh, int(c.sub8x8))
    return {"sum": want}


Row("frame_integral", ("frame_integral",),
    # W 48: stride 192 or 256; W 100: stride - padh - 8 off a wave (and a dword) boundary of columns
    [("l%d-p%d-s%d-w%d" % (ln, ph, s8, W), dict(lines=ln, padh=ph, sub8x8=s8, W=W))
     for ln, ph in ((16, 32), (48, 64)) for s8 in (0, 1) for W in (48, 100)],
    _integral_setup, _integral_call, lambda c: {"sum": fp.integral_masks(c.out, c.lines, c.padh, c.sub8x8)[0]},
    _integral_oracle, variants=[("X264HIP_INTEGRAL_VARIANT", 1)])


# ------------------------------------------------------------------ mb_dct_quant / mb_dequant_idct_add
def _quant_tables(hip, bd, transform):
    import checkasm_bufs as cb
    q4m, q4b, q8m, q8b = hip.cqm_init(bd, cb.cqm_lists(0, bd))
    dq4, dq8 = hip.cqm_dequant(cb.cqm_lists(0, bd))
    qp = 20 + 6 * (bd - 8)
    return ((q4m[1, qp], q4b[1, qp], dq4[1]) if transform == 4 else (q8m[1, qp], q8b[1, qp], dq8[1]))


def _dq_setup(ar, bd, mbw, mbh, transform, dx):
    import conftest
    hip = conftest.load_package()
    W, H = 16 * mbw, 16 * mbh
    n = 2 * mbw * mbh
    mf, bias, _ = _quant_tables(hip, bd, transform)
    rs = np.random.default_rng(mbw * 7 + dx)
    ref = pix(mbw + mbh, bd, (2, H + 64, W + 64 + 64))
    fenc = np.clip(ref.astype(np.int32) + rs.integers(-6, 7, ref.shape), 0, (1 << bd) - 1).astype(pdt(bd))
    return _ns(bd=bd, mbw=mbw, mbh=mbh, transform=transform, dx=dx, n=n,
               fenc=ar.plane("fenc", 2, W + 64, H, pdt(bd), fenc), pred=ar.plane("pred", 2, W + 64, H, pdt(bd), ref),
               mf=ar.list("mf", mf.size, udt(bd), mf), bias=ar.list("bias", bias.size, udt(bd), bias),
               dct=ar.list("dct", (n + 16, 256), cdt(bd)), nz=ar.list("nz", n + 16, np.int32))


def _dq_call(hip, c, dev, tight):
    dct, nz = hip.mb_dct_quant(c.transform, c.fenc.t(dev), c.fenc.origin + c.dx, c.fenc.stride, c.pred.t(dev),
                               c.pred.origin + c.pred.stride + 5, c.pred.stride, c.mbw, c.mbh, 2, T(c.mf, dev),
                               T(c.bias, dev), dct=None if tight else T(c.dct, dev), nz=None if tight else T(c.nz, dev))
    return {"dct": dct, "nz": nz} if tight else None


def _dq_masks(c):
    return {"dct": c.dct.items(c.n), "nz": c.nz.items(c.n)}


Row("mb_dct_quant", ("mb_dct_quant",),
    # 1, 15, 17, 20 MBs: below a 16-MB strip, just before, just past and ragged; dx moves the strips'
    # sector shift as test_mb_dct_quant_strip_alignment does
    [("%dx%d-t%d-dx%d" % (w, h, t, dx), dict(mbw=w, mbh=h, transform=t, dx=dx))
     for w in (1, 15, 17, 20) for h in (1, 3) for t in (4, 8) for dx in (0, 16, 48)],
    _dq_setup, _dq_call, _dq_masks, variants=STREAM_VARIANTS)


def _rec_setup(ar, bd, mbw, mbh, transform, extra):
    import conftest
    hip = conftest.load_package()
    W, H = 16 * mbw, 16 * mbh
    n = 2 * mbw * mbh
    rs = np.random.default_rng(mbw * 3 + transform)
    coefs = rs.integers(-30, 31, (n, 256)) * (rs.random((n, 256)) < 0.3)
    _, _, dmf = _quant_tables(hip, bd, transform)
    dct = ar.list("dct", (n + 16, 256), cdt(bd), valid=n)
    dct.data(ar.host)[:n] = coefs
    qp = ar.list("qp", n + 16, np.int32, valid=n)
    qp.data(ar.host)[:n] = rs.integers(10, 40 + 6 * (bd - 8), n)
    return _ns(bd=bd, mbw=mbw, mbh=mbh, transform=transform, n=n, dct=dct, qp=qp,
               dmf=ar.list("dmf", dmf.size, np.int32, dmf),
               pred=ar.plane("pred", 2, W, H, pdt(bd), pix(mbw, bd, (2, H + 64, W + 64)), extra=extra),
               recon=ar.plane("recon", 2, W, H, pdt(bd), extra=extra))


def _rec_call(hip, c, dev, tight):
    import torch
    recon = torch.zeros_like(c.pred.t(dev)) if tight else c.recon.t(dev)
    hip.mb_dequant_idct_add(c.transform, T(c.dct, dev), c.mbw, c.mbh, 2, T(c.dmf, dev), T(c.qp, dev), c.pred.t(dev),
                            c.pred.origin, c.pred.stride, recon, c.recon.origin, c.recon.stride)
    return {"recon": recon} if tight else None


def _rec_oracle(orc, c, host):
    want = np.zeros(c.recon.shape, c.recon.dtype)
    nm = c.mbw * c.mbh
    p = c.pred.np(host)
    for f in range(2):
        flat = want[f].reshape(-1)
        orc.mb_dequant_idct_add(c.bd, c.transform, c.dct.data(host)[f * nm:(f + 1) * nm], c.mbw, c.mbh,
                                c.dmf.data(host), c.qp.data(host)[f * nm:(f + 1) * nm], p[f].ravel(), c.pred.origin,
                                c.pred.stride, flat, c.recon.origin, c.recon.stride)
    return {"recon": want}


Row("mb_dequant_idct_add", ("mb_dequant_idct_add",),
    [("%dx%d-t%d%s" % (w, h, t, "+4" if e else ""), dict(mbw=w, mbh=h, transform=t, extra=e))
     for w in (1, 15, 17, 20) for h in (1, 3) for t in (4, 8) for e in (0, 4)],
    _rec_setup, _rec_call, lambda c: {"recon": fp.recon_mask(c.recon, c.mbw, c.mbh)}, _rec_oracle)


# ------------------------------------------------------------------ search tables
def _tab_setup(ar, bd, mbw, mbh, rng, kind, shift=0):
    W, H = 16 * mbw, 16 * mbh
    n = 2 * mbw * mbh
    ref = pix(mbw * mbh + rng, bd, (2, H + 64, W + 64))
    fenc = np.roll(ref, (1, -2), (1, 2))
    w = 2 * rng + 1
    c = _ns(bd=bd, mbw=mbw, mbh=mbh, rng=rng, kind=kind, n=n, shift=shift,
            fenc=ar.plane("fenc", 2, W, H, pdt(bd), fenc), ref=ar.plane("ref", 2, W, H, pdt(bd), ref))
    pitch = (w + 3) // 4 * 4
    if kind == "full":
        c.table = ar.list("table", (n, w, pitch), sdt(bd))
    elif kind == "full8":
        c.table = ar.list("table", (n, 4, w, pitch), np.uint16)
    else:
        # centres that clamp at each frame edge, and some that do not
        rs = np.random.default_rng(n)
        cen = np.stack([rs.integers(-12, 13, n), rs.integers(-12, 13, n)], 1)
        cen[0] = (-70, -70)
        cen[-1] = (70, 70)
        if n > 2:
            cen[1] = (70, -70)
            cen[-2] = (-70, 70)
        c.centre = ar.list("centre", (n + 16, 2), np.int16, valid=n)
        c.centre.data(ar.host)[:n] = cen
        pw = (2 * rng + (6 if bd == 8 else 4) + 3) // 4 * 4
        c.table = ar.list("table", (n, w, pw), sdt(bd))
        c.origin = ar.list("origin", (n, 2), np.int16)
    return c


def _tab_call(hip, c, dev, tight):
    a = (c.fenc.t(dev), c.fenc.origin + c.shift, c.fenc.stride, c.ref.t(dev), c.ref.origin, c.ref.stride, c.mbw, c.mbh, 2, c.rng)
    tab = None if tight else T(c.table, dev)
    if c.kind == "full":
        t = hip.me_search_full(*a, table=tab)
        return {"table": t} if tight else None
    if c.kind == "full8":
        t = hip.me_search_full8(*a, table8=tab)
        return {"table": t} if tight else None
    t, o = hip.me_search_centred(*a, T(c.centre, dev)[:c.n], table=tab, origin=None if tight else T(c.origin, dev))
    return {"table": t, "origin": o} if tight else None


def _tab_masks(c):
    m = {"table": fp.table_mask(c.table)}
    if c.kind == "centred":
        m["origin"] = c.origin.mask()
    return m


def _tab_oracle(orc, c, host):
    """the SAD entries [0, 2*range] of every row are the oracle's; the padding entries the header
    describes are held to the tight call's only (me_search_centred: the whole row is SADs)"""
    f_, r_ = c.fenc.np(host), c.ref.np(host)
    w = 2 * c.rng + 1
    nm = c.mbw * c.mbh
    pay = np.zeros(c.table.pshape, c.table.dtype)
    sad = np.zeros(c.table.pshape, bool)
    org = np.zeros((c.n, 2), np.int16)
    for f in range(2):
        a = (c.bd, f_[f].ravel(), c.fenc.origin + c.shift, c.fenc.stride, r_[f].ravel(), c.ref.origin, c.ref.stride, c.mbw,
             c.mbh, c.rng)
        sl = slice(f * nm, (f + 1) * nm)
        if c.kind == "full":
            pay[sl, :, :w] = orc.me_search_full(*a).reshape(nm, w, w)
            sad[sl, :, :w] = True
        elif c.kind == "full8":
            pay[sl, :, :, :w] = orc.me_search_full8(*a).reshape(nm, 4, w, w)
            sad[sl, :, :, :w] = True
        else:
            t, o = orc.me_search_centred(*a, c.centre.data(host)[sl])
            pay[sl] = t.reshape(nm, w, -1)
            sad[sl] = True
            org[sl] = o
    want = c.table.np(host).copy()
    want[c.table.guard:c.table.guard + c.table.n] = pay.ravel()
    out = {"table": (want, c.table.mask(sad))}
    if c.kind == "centred":
        wo = c.origin.np(host).copy()
        wo[c.origin.guard:c.origin.guard + c.origin.n] = org.ravel()
        out["origin"] = wo
    return out


def _tab_row(kind, entry):
    # grids 1x1, 3x1, 5x2 and every range the ABI takes; the footprint is the whole table, padding
    # entries included, and nothing after the last macroblock's last row
    return Row(entry, (entry,),
               [("%dx%d-r%d" % (w, h, r), dict(mbw=w, mbh=h, rng=r, kind=kind))
                for w, h in ((1, 1), (3, 1), (5, 2)) for r in (4, 8, 16, 24)] +
               # fenc one pixel off a dword: the column-per-lane kernel for unaligned planes
               ([] if kind == "full8" else [("3x1-r%d-odd" % r, dict(mbw=3, mbh=1, rng=r, kind=kind, shift=1))
                                            for r in (4, 16)]),
               _tab_setup, _tab_call, _tab_masks, _tab_oracle, variants=ME_VARIANTS)


_tab_row("full", "me_search_full")
_tab_row("full8", "me_search_full8")
_tab_row("centred", "me_search_centred")


# ------------------------------------------------------------------ list entries
NS = (1, 63, 65, 257)          # one item; one short of a wave, one past it; past a 256-thread block
TAIL = 16                      # items after n in buffers the entry operates on in place, or reads


def _offs(ar, name, n, offs):
    """n offsets the entry may read, then TAIL items of fill it may not"""
    b = ar.list(name, n + TAIL, np.int64, valid=n)
    b.data(ar.host)[:n] = offs
    return b


def _vals(ar, name, n, dtype, vals, fields=None):
    shape = (n + TAIL,) if fields is None else (n + TAIL, fields)
    b = ar.list(name, shape, dtype, valid=n)
    b.data(ar.host)[:n] = np.asarray(vals).reshape(b.data(ar.host)[:n].shape)
    return b


PL_STRIDE, PL_ROWS = 96, 80


# the plane of the block writers (add_idct, zigzag_sub): 17 x 17 = 289 cells of 16x16, so 257 destination
# blocks of any kind never overlap
BIG_STRIDE, BIG_ROWS = 272, 272


def _flat_plane(ar, name, bd, seed, stride=PL_STRIDE, rows=PL_ROWS):
    return ar.list(name, stride * rows, pdt(bd), pix(seed, bd, stride * rows))


def _block_offs(seed, n, bw, bh, margin=0):
    """top-left offsets of n blocks inside the flat plane (`margin` pixels free above and left)"""
    rs = np.random.default_rng(seed)
    x = rs.integers(margin, PL_STRIDE - bw + 1, n)
    y = rs.integers(margin, PL_ROWS - bh + 1, n)
    return (y * PL_STRIDE + x).astype(np.int64)


def _cells(seed, n, w):
    """offsets of n distinct w x w cells of the big plane's w-grid (never overlapping), shuffled"""
    cells = [(y, x) for y in range(0, BIG_ROWS - w + 1, w) for x in range(0, BIG_STRIDE - w + 1, w)]
    pick = np.random.default_rng(seed).permutation(len(cells))[:n]
    assert len(pick) == n, "plane too small"
    return np.array([cells[i][0] * BIG_STRIDE + cells[i][1] for i in pick], np.int64)


def _list_cases(extra):
    return [("n%d-%s" % (n, "-".join("%s%s" % (k[0], v) for k, v in e.items())), dict(n=n, **e))
            for n in NS for e in extra]


def _simple_row(name, entry, extra, setup, call, outs, variants=(), maybe=None):
    """outs(c) -> {buffer name: number of items written} for plain [n, ...] outputs"""
    return Row(name, (entry,), _list_cases(extra), setup, call,
               lambda c: {k: (c.__dict__[k].items(v) if isinstance(v, int) else v) for k, v in outs(c).items()},
               variants=variants, maybe=maybe)


# pixel_cmp_batch: "scores[i] = op( fenc + fenc_off[i], fenc_stride, ref + ref_off[i], ref_stride )"
def _cmp_setup(ar, bd, n, op, i_pixel):
    import x264hip
    bw, bh = x264hip.PIXEL_SIZES[i_pixel]
    return _ns(bd=bd, n=n, op=op, i_pixel=i_pixel, fenc=_flat_plane(ar, "fenc", bd, 1), ref=_flat_plane(ar, "ref", bd, 2),
               fo=_offs(ar, "fo", n, _block_offs(n, n, bw, bh)), ro=_offs(ar, "ro", n, _block_offs(n + 1, n, bw, bh)),
               scores=ar.list("scores", n, np.int32))


def _cmp_call(hip, c, dev, tight):
    r = hip.pixel_cmp_batch(c.op, c.i_pixel, T(c.fenc, dev), PL_STRIDE, T(c.ref, dev), PL_STRIDE, T(c.fo, dev)[:c.n],
                            T(c.ro, dev)[:c.n], scores=None if tight else T(c.scores, dev))
    return {"scores": r} if tight else None


_simple_row("pixel_cmp", "pixel_cmp_batch", [dict(op=0, i_pixel=0), dict(op=1, i_pixel=3), dict(op=2, i_pixel=6),
                                             dict(op=3, i_pixel=0)],
            _cmp_setup, _cmp_call, lambda c: {"scores": c.n})


# pixel_stat_batch: "out[i] = the reference entry on pix1 + off1[i] (and pix2 + off2[i] ...)"
def _stat_setup(ar, bd, n, op, i_pixel, height):
    return _ns(bd=bd, n=n, op=op, i_pixel=i_pixel, height=height, p1=_flat_plane(ar, "p1", bd, 3),
               p2=_flat_plane(ar, "p2", bd, 4), o1=_offs(ar, "o1", n, _block_offs(n + 2, n, 16, 32)),
               o2=_offs(ar, "o2", n, _block_offs(n + 3, n, 16, 32)), out=ar.list("out", n, np.int64))


def _stat_call(hip, c, dev, tight):
    r = hip.pixel_stat_batch(c.op, c.i_pixel, T(c.p1, dev), PL_STRIDE, T(c.o1, dev)[:c.n], T(c.p2, dev), PL_STRIDE,
                             T(c.o2, dev)[:c.n], c.height, out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


_simple_row("pixel_stat", "pixel_stat_batch",
            [dict(op=0, i_pixel=0, height=0), dict(op=1, i_pixel=3, height=0), dict(op=2, i_pixel=0, height=0),
             dict(op=3, i_pixel=0, height=9), dict(op=4, i_pixel=3, height=32)],
            _stat_setup, _stat_call, lambda c: {"out": c.n})


# var2_batch: "out[3i] = return value, out[3i+1..2] = ssd[0..1]"
def _var2_setup(ar, bd, n, i_pixel):
    return _ns(bd=bd, n=n, i_pixel=i_pixel, fenc=_flat_plane(ar, "fenc", bd, 5), fdec=_flat_plane(ar, "fdec", bd, 6),
               fo=_offs(ar, "fo", n, _block_offs(n, n, 8 + 40, 16)), do=_offs(ar, "do", n, _block_offs(n + 1, n, 8 + 24, 16)),
               out=ar.list("out", (n, 3), np.int32))


def _var2_call(hip, c, dev, tight):
    r = hip.var2_batch(c.i_pixel, T(c.fenc, dev), PL_STRIDE, 40, T(c.fdec, dev), PL_STRIDE, 24, T(c.fo, dev)[:c.n],
                       T(c.do, dev)[:c.n], out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


_simple_row("var2", "var2_batch", [dict(i_pixel=2), dict(i_pixel=3)], _var2_setup, _var2_call, lambda c: {"out": c.n})


# ads_batch: "writes the passing candidate indices in order to mvs[i*mvs_pitch ..] and their count to
# nmv[i]": nmv[i] entries of row i, the rest of the row untouched
ADS_PITCH, ADS_DELTA = 72, 256


def _ads_setup(ar, bd, n, i_pixel):
    import oracle_lib as orc
    rs = np.random.default_rng(n + i_pixel)
    sums = rs.integers(0, 1 << (bd + 6), 4096).astype(np.uint16)
    cost = rs.integers(0, 1 << 10, 512).astype(np.uint16)
    width = rs.integers(0, ADS_PITCH + 1, n).astype(np.int32)
    width[0] = 64 if n > 1 else ADS_PITCH
    so = rs.integers(0, 4096 - ADS_DELTA - ADS_PITCH - 16, n).astype(np.int64)
    co = rs.integers(0, 512 - ADS_PITCH, n).astype(np.int64)
    dc = rs.integers(0, 1 << (bd + 6), (n, 4)).astype(np.int32)
    thresh = rs.integers(0, 2 << (bd + 6), n).astype(np.int32)
    ns = {0: 4, 1: 2, 3: 1}[i_pixel]
    count = [len(orc.ads(bd, ns, dc[k], sums, so[k], ADS_DELTA, cost, co[k], int(width[k]), int(thresh[k])))
             for k in range(n)]
    return _ns(bd=bd, n=n, i_pixel=i_pixel, count=count, dc=_vals(ar, "dc", n, np.int32, dc, 4),
               sums=ar.list("sums", 4096, np.int16, sums), so=_offs(ar, "so", n, so),
               cost=ar.list("cost", 512, np.int16, cost), co=_offs(ar, "co", n, co),
               width=_vals(ar, "width", n, np.int32, width), thresh=_vals(ar, "thresh", n, np.int32, thresh),
               mvs=ar.list("mvs", (n, ADS_PITCH), np.int16), nmv=ar.list("nmv", n, np.int32))


def _ads_call(hip, c, dev, tight):
    n = c.n
    r = hip.ads_batch(c.bd, c.i_pixel, T(c.dc, dev)[:n], T(c.sums, dev), ADS_DELTA, T(c.so, dev)[:n], T(c.cost, dev),
                      T(c.co, dev)[:n], T(c.width, dev)[:n], T(c.thresh, dev)[:n], mvs_pitch=ADS_PITCH,
                      outs=None if tight else (T(c.mvs, dev), T(c.nmv, dev)))
    return {"mvs": r[0], "nmv": r[1]} if tight else None


def _ads_masks(c):
    pm = np.zeros((c.n, ADS_PITCH), bool)
    for k, cnt in enumerate(c.count):
        pm[k, :cnt] = True
    return {"mvs": c.mvs.mask(pm), "nmv": c.nmv.mask()}


Row("ads", ("ads_batch",), _list_cases([dict(i_pixel=0), dict(i_pixel=1), dict(i_pixel=3)]), _ads_setup, _ads_call,
    _ads_masks)


# intra_cmp_x3_batch: "scores[3i..3i+2] = the reference's res[3] ... this entry does not write fdec"
def _intra_setup(ar, bd, n, kind, op):
    import x264hip
    w, h = x264hip.INTRA_SIZES[kind]
    do = _block_offs(n + 5, n, 36, 1) if kind == 4 else _block_offs(n + 5, n, w, h, margin=1)
    return _ns(bd=bd, n=n, kind=kind, op=op, fenc=_flat_plane(ar, "fenc", bd, 7), fdec=_flat_plane(ar, "fdec", bd, 8),
               fo=_offs(ar, "fo", n, _block_offs(n + 4, n, w, h)), do=_offs(ar, "do", n, do),
               out=ar.list("out", (n, 3), np.int32))


def _intra_call(hip, c, dev, tight):
    r = hip.intra_cmp_x3_batch(c.kind, c.op, T(c.fenc, dev), PL_STRIDE, T(c.fdec, dev), PL_STRIDE, T(c.fo, dev)[:c.n],
                               T(c.do, dev)[:c.n], out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


_simple_row("intra_cmp_x3", "intra_cmp_x3_batch",
            [dict(kind=0, op=0), dict(kind=1, op=2), dict(kind=2, op=0), dict(kind=3, op=2), dict(kind=4, op=3)],
            _intra_setup, _intra_call, lambda c: {"out": c.n})


# subpel_cmp_batch / subpel_qpel9_batch: "scores[i] = op( fenc + fenc_off[i], fenc_stride, get_ref(qx, qy) )",
# "scores[9i + 3(dy+1) + (dx+1)]"
SP_W, SP_H = 48, 32


def _subpel_setup(ar, bd, n, op, i_pixel, nine):
    import oracle_lib as orc
    import x264hip
    bw, bh = x264hip.PIXEL_SIZES[i_pixel]
    f = ar.plane("fpel", 1, SP_W, SP_H, pdt(bd), pix(9, bd, (1, SP_H + 64, SP_W + 64)))
    flat = f.np(ar.host)[0].ravel().copy()
    hv = orc.frame_filter(bd, flat, f.origin, f.stride, SP_W, SP_H)
    planes = [f]
    for name, a in zip("hvc", hv):
        p = ar.plane(name, 1, SP_W, SP_H, pdt(bd), a.reshape(f.shape[1:])[None, f.guard_rows:f.guard_rows + f.rows,
                                                                           :SP_W + 64])
        planes.append(p)
    rs = np.random.default_rng(n + op)
    bx, by = rs.integers(0, SP_W - bw + 1, n), rs.integers(0, SP_H - bh + 1, n)
    # the candidate block, one more pixel for qpel9's neighbours and the interpolation's +1 stay in the padding
    mvx, mvy = rs.integers(-4 * 28, 4 * 28, n), rs.integers(-4 * 28, 4 * 28, n)
    qxy = np.stack([4 * bx + mvx, 4 * by + mvy], 1).astype(np.int32)
    qxy[:, 0] = np.clip(qxy[:, 0], -4 * 30, 4 * (SP_W + 30 - bw))
    qxy[:, 1] = np.clip(qxy[:, 1], -4 * 30, 4 * (SP_H + 30 - bh))
    return _ns(bd=bd, n=n, op=op, i_pixel=i_pixel, nine=nine, planes=planes, fenc=_flat_plane(ar, "fenc", bd, 10),
               fo=_offs(ar, "fo", n, _block_offs(n + 6, n, bw, bh)), qxy=_vals(ar, "qxy", n, np.int32, qxy, 2),
               scores=ar.list("scores", (n, 9) if nine else (n,), np.int32))


def _subpel_call(hip, c, dev, tight):
    fn = hip.subpel_qpel9_batch if c.nine else hip.subpel_cmp_batch
    p0 = c.planes[0]
    r = fn(c.op, c.i_pixel, T(c.fenc, dev), PL_STRIDE, [p.t(dev) for p in c.planes], p0.origin, p0.stride,
           T(c.fo, dev)[:c.n], T(c.qxy, dev)[:c.n], scores=None if tight else T(c.scores, dev))
    return {"scores": r} if tight else None


_simple_row("subpel_cmp", "subpel_cmp_batch", [dict(op=0, i_pixel=0, nine=0), dict(op=2, i_pixel=3, nine=0),
                                               dict(op=2, i_pixel=6, nine=0)],
            _subpel_setup, _subpel_call, lambda c: {"scores": c.n})
_simple_row("subpel_qpel9", "subpel_qpel9_batch", [dict(op=0, i_pixel=0, nine=1), dict(op=2, i_pixel=3, nine=1)],
            _subpel_setup, _subpel_call, lambda c: {"scores": c.n})


# sub_dct_batch: "dct holds n consecutive outputs of the selected entry's size"
def _subdct_setup(ar, bd, n, kind):
    import x264hip
    w, h = [(4, 4), (8, 8), (16, 16), (8, 8), (8, 16), (8, 8), (16, 16)][kind]
    return _ns(bd=bd, n=n, kind=kind, fenc=_flat_plane(ar, "fenc", bd, 11), fdec=_flat_plane(ar, "fdec", bd, 12),
               fo=_offs(ar, "fo", n, _block_offs(n + 7, n, w, h)), do=_offs(ar, "do", n, _block_offs(n + 8, n, w, h)),
               out=ar.list("out", (n, x264hip.DCT_OUT_SIZE[kind]), cdt(bd)))


def _subdct_call(hip, c, dev, tight):
    r = hip.sub_dct_batch(c.kind, T(c.fenc, dev), PL_STRIDE, T(c.fdec, dev), PL_STRIDE, T(c.fo, dev)[:c.n],
                          T(c.do, dev)[:c.n], out=None if tight else T(c.out, dev).view(-1))
    return {"out": r} if tight else None


_simple_row("sub_dct", "sub_dct_batch", [dict(kind=k) for k in range(7)], _subdct_setup, _subdct_call,
            lambda c: {"out": c.n})


# add_idct_batch: "n calls of the add*_idct* entry `kind` on dst + dst_off[i] (stride dst_stride) ...
# dct is not modified": the destination blocks and nothing else of the plane
IDCT_W = [4, 8, 16, 8, 16, 8, 16]
IDCT_IN = [16, 64, 256, 4, 16, 64, 256]


def _addidct_setup(ar, bd, n, kind):
    rs = np.random.default_rng(n + kind)
    offs = _cells(n + kind, n, IDCT_W[kind])
    return _ns(bd=bd, n=n, kind=kind, offs=offs, dst=_flat_plane(ar, "dst", bd, 13, BIG_STRIDE, BIG_ROWS),
               do=_offs(ar, "do", n, offs),
               dct=_vals(ar, "dct", n, cdt(bd), rs.integers(-200, 201, (n, IDCT_IN[kind])), IDCT_IN[kind]))


def _addidct_call(hip, c, dev, tight):
    hip.add_idct_batch(c.kind, T(c.dst, dev), BIG_STRIDE, T(c.do, dev)[:c.n], T(c.dct, dev)[:c.n])
    return {"dst": T(c.dst, dev)} if tight else None


def _addidct_oracle(orc, c, host):
    want = c.dst.np(host).copy()
    want[c.dst.guard:c.dst.guard + c.dst.n] = orc.add_idct_list(c.bd, c.kind, c.dst.data(host), BIG_STRIDE, c.offs,
                                                                c.dct.data(host)[:c.n])
    return {"dst": want}


Row("add_idct", ("add_idct_batch",), _list_cases([dict(kind=k) for k in range(7)]), _addidct_setup, _addidct_call,
    lambda c: {"dst": fp.blocks_mask(c.dst, c.offs, IDCT_W[c.kind], IDCT_W[c.kind], BIG_STRIDE)}, _addidct_oracle)


# in-place coefficient entries: items [0, n) of the operated-on buffer, never n .. n + 16
def _coefs(seed, n, size, lim=300):
    rs = np.random.default_rng(seed)
    return rs.integers(-lim, lim + 1, (n, size))


def _dequant_setup(ar, bd, n, kind):
    import x264hip
    size = 64 if kind == 1 else 16
    dq4, dq8 = x264hip.cqm_dequant([[16] * 16] * 4 + [[16] * 64] * 4)
    mf = dq8[1] if kind == 1 else dq4[1]
    return _ns(bd=bd, n=n, kind=kind, dct=_vals(ar, "dct", n, cdt(bd), _coefs(n, n, size), size),
               mf=ar.list("mf", mf.size, np.int32, mf),
               qp=_vals(ar, "qp", n, np.int32, np.random.default_rng(n).integers(0, 52 + 6 * (bd - 8), n)))


def _dequant_call(hip, c, dev, tight):
    hip.dequant_batch(c.kind, T(c.dct, dev)[:c.n], T(c.mf, dev), T(c.qp, dev)[:c.n])
    return {"dct": T(c.dct, dev)} if tight else None


_simple_row("dequant", "dequant_batch", [dict(kind=k) for k in range(3)], _dequant_setup, _dequant_call,
            lambda c: {"dct": c.n})


# quant_batch / quant_dc_batch: "in-place quantisation of n blocks ... nz[i] = the entry's return value"
def _quant_setup(ar, bd, n, kind):
    import x264hip
    size = 64 if kind in (0, 2) else 4 if kind == 4 else 16
    q4m, q4b, q8m, q8b = x264hip.cqm_init(bd, [[16] * 16] * 4 + [[16] * 64] * 4)
    qp = 20 + 6 * (bd - 8)
    mf, bias = (q8m[1, qp], q8b[1, qp]) if kind == 0 else (q4m[1, qp], q4b[1, qp])
    return _ns(bd=bd, n=n, kind=kind, dct=_vals(ar, "dct", n, cdt(bd), _coefs(n + 1, n, size, 2000), size),
               mf=ar.list("mf", mf.size, udt(bd), mf), bias=ar.list("bias", bias.size, udt(bd), bias),
               nz=ar.list("nz", n, np.int32))


def _quant_call(hip, c, dev, tight):
    nz = None if tight else T(c.nz, dev)
    if c.kind >= 3:
        r = hip.quant_dc_batch(c.kind, T(c.dct, dev)[:c.n], int(c.mf.data_host[0]) >> 1, int(c.bias.data_host[0]) << 1, nz=nz)
    else:
        r = hip.quant_batch(c.kind, T(c.dct, dev)[:c.n], T(c.mf, dev), T(c.bias, dev), nz=nz)
    return {"dct": T(c.dct, dev), "nz": r} if tight else None


def _quant_setup2(ar, bd, n, kind):
    c = _quant_setup(ar, bd, n, kind)
    c.mf.data_host, c.bias.data_host = c.mf.data(ar.host).copy(), c.bias.data(ar.host).copy()
    return c


_simple_row("quant", "quant_batch", [dict(kind=k) for k in range(3)], _quant_setup2, _quant_call,
            lambda c: {"dct": c.n, "nz": c.n})
_simple_row("quant_dc", "quant_dc_batch", [dict(kind=3), dict(kind=4)], _quant_setup2, _quant_call,
            lambda c: {"dct": c.n, "nz": c.n})


# dc_batch: "in-place DC transforms: DC_4x4 on n arrays d[16]; DC_2x4 on n pairs (dct[8] out,
# dct4x4[8][16] in/out)"; of dct4x4 the reference (dct2x4dc, dct.c:109-143) writes the eight DC coefficients
def _dc_setup(ar, bd, n, kind):
    c = _ns(bd=bd, n=n, kind=kind)
    if kind == 1:
        c.dct = ar.list("dct", (n + TAIL, 8), cdt(bd))
        c.dct4x4 = _vals(ar, "dct4x4", n, cdt(bd), _coefs(n + 2, n, 128), 128)
    else:
        c.dct = _vals(ar, "dct", n, cdt(bd), _coefs(n + 3, n, 16, 2000), 16)
    return c


def _dc_call(hip, c, dev, tight):
    if c.kind == 1:
        hip.dc_batch(1, T(c.dct, dev)[:c.n], T(c.dct4x4, dev)[:c.n], n=c.n)
        return {"dct": T(c.dct, dev), "dct4x4": T(c.dct4x4, dev)} if tight else None
    hip.dc_batch(c.kind, T(c.dct, dev)[:c.n])
    return {"dct": T(c.dct, dev)} if tight else None


def _dc_masks(c):
    m = {"dct": c.dct.items(c.n)}
    if c.kind == 1:
        pm = np.zeros(c.dct4x4.pshape, bool)
        pm[:c.n, ::16] = True
        m["dct4x4"] = c.dct4x4.mask(pm)
    return m


Row("dc", ("dc_batch",), _list_cases([dict(kind=0), dict(kind=1), dict(kind=2)]), _dc_setup, _dc_call, _dc_masks)


# idct_dequant_2x4_batch: "dconly = 0: writes dct4x4[8][16] per call, 128 coefs apart" -- of them the
# reference (idct_dequant_2x4_dc, quant.c) stores the eight DC coefficients and leaves dct[8] alone --
# "or _dconly (dconly = 1: in place on dct[8])"
def _idq_setup(ar, bd, n, dconly):
    import x264hip
    dq4, _ = x264hip.cqm_dequant([[16] * 16] * 4 + [[16] * 64] * 4)
    c = _ns(bd=bd, n=n, dconly=dconly, dct=_vals(ar, "dct", n, cdt(bd), _coefs(n + 4, n, 8), 8),
            mf=ar.list("mf", 96, np.int32, dq4[3]),
            qp=_vals(ar, "qp", n, np.int32, np.random.default_rng(n + 1).integers(0, 52, n)))
    c.dct4x4 = None if dconly else ar.list("dct4x4", (n + TAIL, 128), cdt(bd))
    return c


def _idq_call(hip, c, dev, tight):
    hip.idct_dequant_2x4_batch(c.dconly, T(c.dct, dev)[:c.n], T(c.mf, dev), T(c.qp, dev)[:c.n],
                               dct4x4=None if c.dconly else T(c.dct4x4, dev)[:c.n])
    if not tight:
        return None
    return {"dct": T(c.dct, dev)} if c.dconly else {"dct4x4": T(c.dct4x4, dev)}


def _idq_masks(c):
    if c.dconly:
        return {"dct": c.dct.items(c.n)}
    pm = np.zeros(c.dct4x4.pshape, bool)
    pm[:c.n, ::16] = True
    return {"dct4x4": c.dct4x4.mask(pm)}


Row("idct_dequant_2x4", ("idct_dequant_2x4_batch",), _list_cases([dict(dconly=0), dict(dconly=1)]), _idq_setup,
    _idq_call, _idq_masks)


# optimize_chroma_dc_batch: "in place, dequant_mf[i] per call, nz[i] = return value"
def _optc_setup(ar, bd, n, c422):
    rs = np.random.default_rng(n + c422)
    nc = 8 if c422 else 4
    d = rs.integers(-6, 7, (n, nc)) * (rs.integers(0, 3, (n, nc)) > 0)
    return _ns(bd=bd, n=n, c422=c422, dct=_vals(ar, "dct", n, cdt(bd), d, nc),
               mf=_vals(ar, "mf", n, np.int32, (16 * rs.integers(10, 19, n)) << rs.integers(0, 5, n)),
               nz=ar.list("nz", n, np.int32))


def _optc_call(hip, c, dev, tight):
    r = hip.optimize_chroma_dc_batch(c.c422, T(c.dct, dev)[:c.n], T(c.mf, dev)[:c.n], nz=None if tight else T(c.nz, dev))
    return {"dct": T(c.dct, dev), "nz": r} if tight else None


_simple_row("optimize_chroma_dc", "optimize_chroma_dc_batch", [dict(c422=0), dict(c422=1)], _optc_setup, _optc_call,
            lambda c: {"dct": c.n, "nz": c.n})


# denoise_dct_batch: "n consecutive blocks of `size` coefficients sharing sum[size] (accumulated) and offset[size]"
def _denoise_setup(ar, bd, n, size):
    rs = np.random.default_rng(n + size)
    return _ns(bd=bd, n=n, size=size, dct=_vals(ar, "dct", n, cdt(bd), _coefs(n + 5, n, size), size),
               sums=ar.list("sums", size, np.int32, rs.integers(0, 1000, size)),
               offset=ar.list("offset", size, udt(bd), rs.integers(0, 60, size)))


def _denoise_call(hip, c, dev, tight):
    hip.denoise_dct_batch(T(c.dct, dev)[:c.n], c.size, T(c.sums, dev), T(c.offset, dev), n=c.n)
    return {"dct": T(c.dct, dev), "sums": T(c.sums, dev)} if tight else None


_simple_row("denoise_dct", "denoise_dct_batch", [dict(size=16), dict(size=64)], _denoise_setup, _denoise_call,
            lambda c: {"dct": c.n, "sums": c.sums.mask()})


# coef_stat_batch: "decimate_score / coeff_last of n blocks `pitch` coefs apart" -> out[n]
def _sparse(seed, n, size=64):
    rs = np.random.default_rng(seed)
    c = np.where(rs.random((n, size)) < 0.2, rs.integers(1, 4, (n, size)) * np.where(rs.random((n, size)) < 0.5, -1, 1), 0)
    c[:, 1] = 1                      # no all-zero block (coeff_level_run's precondition), DECIMATE15 included
    return c


def _cstat_setup(ar, bd, n, kind):
    return _ns(bd=bd, n=n, kind=kind, dct=_vals(ar, "dct", n, cdt(bd), _sparse(n + kind, n), 64),
               out=ar.list("out", n, np.int32))


def _cstat_call(hip, c, dev, tight):
    r = hip.coef_stat_batch(c.kind, T(c.dct, dev), 64, c.n, out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


_simple_row("coef_stat", "coef_stat_batch", [dict(kind=k) for k in range(8)], _cstat_setup, _cstat_call,
            lambda c: {"out": c.n})


# coeff_level_run_batch: "last[i], mask[i], count[i] (the return value) and level[18*i ..]": of row i the
# count[i] levels the reference stores (quant.c coeff_level_run); the rest of the row keeps its bytes
def _clr_setup(ar, bd, n, num):
    d = _sparse(n + num, n)
    return _ns(bd=bd, n=n, num=num, count=(d[:, :num] != 0).sum(1), dct=_vals(ar, "dct", n, cdt(bd), d, 64),
               last=ar.list("last", n, np.int32), mask=ar.list("mask", n, np.int32), count_=ar.list("count", n, np.int32),
               level=ar.list("level", (n, 18), cdt(bd)))


def _clr_call(hip, c, dev, tight):
    r = hip.coeff_level_run_batch(c.num, T(c.dct, dev), 64, c.n,
                                  outs=None if tight else tuple(T(b, dev) for b in (c.last, c.mask, c.count_, c.level)))
    return dict(zip(("last", "mask", "count", "level"), r)) if tight else None


def _clr_masks(c):
    pm = np.arange(18)[None, :] < np.asarray(c.count)[:, None]
    return {"last": c.last.mask(), "mask": c.mask.mask(), "count": c.count_.mask(), "level": c.level.mask(pm)}


Row("coeff_level_run", ("coeff_level_run_batch",), _list_cases([dict(num=k) for k in (4, 8, 15, 16)]), _clr_setup,
    _clr_call, _clr_masks)


# zigzag_scan_batch: "zigzag_scan_4x4 (size 4) / 8x8 (size 8), frame or field order, n blocks" -> level[n][size*size]
def _zscan_setup(ar, bd, n, size, field):
    return _ns(bd=bd, n=n, size=size, field=field,
               dct=_vals(ar, "dct", n, cdt(bd), _coefs(n + 6, n, size * size, 999), size * size),
               level=ar.list("level", (n, size * size), cdt(bd)))


def _zscan_call(hip, c, dev, tight):
    r = hip.zigzag_scan_batch(c.size, c.field, T(c.dct, dev)[:c.n], level=None if tight else T(c.level, dev), n=c.n)
    return {"level": r} if tight else None


_simple_row("zigzag_scan", "zigzag_scan_batch", [dict(size=4, field=0), dict(size=8, field=1)], _zscan_setup,
            _zscan_call, lambda c: {"level": c.n})


# zigzag_sub_batch: "level (16 or 64 per call), dc[i] (4x4ac only), nz[i]; dst block is overwritten with the src block"
def _zsub_setup(ar, bd, n, kind, field):
    w = 8 if kind == 2 else 4
    offs = _cells(n + kind, n, w)
    return _ns(bd=bd, n=n, kind=kind, field=field, offs=offs, w=w, src=_flat_plane(ar, "src", bd, 14),
               dst=_flat_plane(ar, "dst", bd, 15, BIG_STRIDE, BIG_ROWS), so=_offs(ar, "so", n, _block_offs(n + 9, n, w, w)),
               do=_offs(ar, "do", n, offs), level=ar.list("level", (n, w * w), cdt(bd)), dc=ar.list("dc", n, cdt(bd)),
               nz=ar.list("nz", n, np.int32))


def _zsub_call(hip, c, dev, tight):
    r = hip.zigzag_sub_batch(c.kind, c.field, T(c.src, dev), PL_STRIDE, T(c.dst, dev), BIG_STRIDE, T(c.so, dev)[:c.n],
                             T(c.do, dev)[:c.n], outs=None if tight else (T(c.level, dev), T(c.dc, dev), T(c.nz, dev)))
    if not tight:
        return None
    out = {"level": r[0], "nz": r[2], "dst": T(c.dst, dev)}
    if c.kind == 1:
        out["dc"] = r[1]
    return out


def _zsub_masks(c):
    m = {"level": c.level.mask(), "nz": c.nz.mask(), "dst": fp.blocks_mask(c.dst, c.offs, c.w, c.w, BIG_STRIDE)}
    if c.kind == 1:
        m["dc"] = c.dc.mask()
    return m


def _zsub_oracle(orc, c, host):
    dst = c.dst.data(host).copy()
    src, so = c.src.data(host), c.so.data(host)
    level, nz, dc = np.zeros(c.level.pshape, c.level.dtype), np.zeros(c.n, np.int32), np.zeros(c.n, c.dc.dtype)
    for i in range(c.n):
        nz[i], level[i], dc[i], dst = orc.zigzag_sub(c.bd, c.kind, c.field, src, so[i], PL_STRIDE, dst, c.offs[i], BIG_STRIDE)
    out = {}
    for b, a in ((c.dst, dst), (c.level, level), (c.nz, nz)) + (((c.dc, dc),) if c.kind == 1 else ()):
        want = b.np(host).copy()
        want[b.guard:b.guard + b.n] = a.ravel()
        out[b.name] = want
    return out


Row("zigzag_sub", ("zigzag_sub_batch",), _list_cases([dict(kind=0, field=0), dict(kind=1, field=1), dict(kind=2, field=0)]),
    _zsub_setup, _zsub_call, _zsub_masks, _zsub_oracle)


# zigzag_interleave_batch: "n blocks (64 coefs in/out, 16 nnz bytes per call)"; of the 16 nnz bytes the
# reference (zigzag_interleave_8x8_cavlc, dct.c) stores nnz[0], [1], [8], [9]
def _zint_setup(ar, bd, n):
    return _ns(bd=bd, n=n, src=_vals(ar, "src", n, cdt(bd), _sparse(n, n), 64), dst=ar.list("dst", (n, 64), cdt(bd)),
               nnz=ar.list("nnz", (n, 16), np.uint8))


def _zint_call(hip, c, dev, tight):
    r = hip.zigzag_interleave_batch(T(c.src, dev)[:c.n], outs=None if tight else (T(c.dst, dev), T(c.nnz, dev)), n=c.n)
    return {"dst": r[0], "nnz": r[1]} if tight else None


def _zint_masks(c):
    pm = np.zeros((c.n, 16), bool)
    pm[:, [0, 1, 8, 9]] = True
    return {"dst": c.dst.mask(), "nnz": c.nnz.mask(pm)}


Row("zigzag_interleave", ("zigzag_interleave_batch",), _list_cases([dict()]), _zint_setup, _zint_call, _zint_masks)


# ------------------------------------------------------------------ motion search and refinement
ME_W, ME_H = 48, 32
GRIDS = ((1, 1), (3, 1), (5, 2))


def _smooth(seed, bd, shape):
    """textured frames a search can follow: low-passed noise over the whole padded picture"""
    rs = np.random.default_rng(seed)
    a = rs.random(shape)
    for ax in (-1, -2):
        a = (a + np.roll(a, 1, ax) + np.roll(a, 2, ax) + np.roll(a, 3, ax)) / 4
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * ((1 << bd) - 1)).astype(pdt(bd))


def _me_content(ar, bd, nf, W, H, seed, hpel=True, prefix=""):
    """fenc = the reference moved by (3, 2) plus noise; the reference's F (and H, V, C) planes"""
    import oracle_lib as orc
    ref = _smooth(seed, bd, (nf, H + 64, W + 64))
    noise = np.random.default_rng(seed + 1).integers(-2, 3, ref.shape)
    fenc = np.clip(np.roll(ref, (2, 3), (1, 2)).astype(np.int32) + noise, 0, (1 << bd) - 1).astype(pdt(bd))
    fe = ar.plane(prefix + "fenc", nf, W, H, pdt(bd), fenc)
    F = ar.plane(prefix + "F", nf, W, H, pdt(bd), ref)
    planes = [F]
    if hpel:
        g = F.guard_rows
        hv = [orc.frame_filter(bd, F.np(ar.host)[f].ravel().copy(), F.origin, F.stride, W, H) for f in range(nf)]
        for k, name in enumerate("HVC"):
            data = np.stack([hv[f][k].reshape(F.shape[1:])[g:g + F.rows, :W + 64] for f in range(nf)])
            planes.append(ar.plane(prefix + name, nf, W, H, pdt(bd), data))
    return fe, planes


def _cost_table(ar, span=8192):
    import refine_cases as rc
    cm, c0 = rc.cost_mv(span=span)
    return ar.list("cost_mv", cm.size, np.int16, cm), c0


def _esa_par(seed, mbw, mbh, nf, me_range):
    """test_me_search_esa_fused's parameters: predictor centres, clipped windows, unbeatable predictors"""
    rs = np.random.default_rng(seed)
    nmb = mbw * mbh
    n = nf * nmb
    par = np.zeros((n, 8), np.int16)
    par[:, 0], par[:, 1] = rs.integers(-12, 13, n), rs.integers(-12, 13, n)
    par[:, 2], par[:, 3] = rs.integers(-64, 65, n), rs.integers(-64, 65, n)
    mb = np.arange(n) % nmb
    mbx, mby = mb % mbw, mb // mbw
    tight = rs.integers(0, me_range + 1, (n, 4)) * (rs.random((n, 4)) < 0.3)
    par[:, 4] = np.minimum(-16 * mbx - 24 + tight[:, 0], par[:, 0])
    par[:, 5] = np.minimum(-16 * mby - 24 + tight[:, 1], par[:, 1])
    par[:, 6] = np.maximum(16 * (mbw - 1 - mbx) + 20 - tight[:, 2], par[:, 0])
    par[:, 7] = np.maximum(16 * (mbh - 1 - mby) + 24 - tight[:, 3], par[:, 1])
    init = rs.integers(0, 20000, n).astype(np.int32)
    init[::7] = 0
    return par, init


def _grid_cases(extra):
    return [("%dx%d-%s" % (w, h, "-".join("%s%s" % (k[0], v) for k, v in e.items())), dict(mbw=w, mbh=h, **e))
            for w, h in GRIDS for e in extra]


# me_esa_argmin / me_esa_argmin_at: "out[3*i] = {cost, mx, my} ... n = #MBs"; table rows past MB n - 1 unread
def _argmin_setup(ar, bd, mbw, mbh, rng, me_range, at):
    import oracle_lib as orc
    W, H = 16 * mbw, 16 * mbh
    n = 2 * mbw * mbh
    fe, (F,) = _me_content(ar, bd, 2, W, H, rng + mbw, hpel=False)
    par, init = _esa_par(rng + at, mbw, mbh, 2, me_range)
    w = 2 * rng + 1
    tabs, orgs = [], []
    for f in range(2):
        a = (bd, fe.np(ar.host)[f].ravel(), fe.origin, fe.stride, F.np(ar.host)[f].ravel(), F.origin, F.stride, mbw, mbh,
             rng)
        sl = slice(f * mbw * mbh, (f + 1) * mbw * mbh)
        if at:
            t, o = orc.me_search_centred(*a, par[sl, :2])
            orgs.append(o)
            tabs.append(t.reshape(mbw * mbh, w, -1))
        else:
            par[sl, 0:2] = np.clip(par[sl, 0:2], -(rng - me_range), rng - me_range) if rng > me_range else 0
            par[sl, 4] = np.maximum(par[sl, 4], -rng)
            par[sl, 5] = np.maximum(par[sl, 5], -rng)
            par[sl, 6] = np.maximum(np.minimum(par[sl, 6], rng - 3), par[sl, 4])
            par[sl, 7] = np.maximum(np.minimum(par[sl, 7], rng), par[sl, 5])
            t = np.zeros((mbw * mbh, w, (w + 3) // 4 * 4), sdt(bd))
            t[:, :, :w] = orc.me_search_full(*a).reshape(mbw * mbh, w, w)
            tabs.append(t)
    tab = np.concatenate(tabs)
    cm, c0 = _cost_table(ar)
    c = _ns(bd=bd, n=n, rng=rng, me_range=me_range, at=at, c0=c0, cm=cm,
            table=_vals(ar, "table", n, sdt(bd), tab, tab[0].size), par=_vals(ar, "par", n, np.int16, par, 8),
            init=_vals(ar, "init", n, np.int32, init), out=ar.list("out", (n, 3), np.int32))
    c.origin = _vals(ar, "origin", n, np.int16, np.concatenate(orgs), 2) if at else None
    return c


def _argmin_call(hip, c, dev, tight):
    n = c.n
    r = hip.me_esa_argmin(T(c.table, dev)[:n], c.rng, c.me_range, T(c.par, dev)[:n], T(c.init, dev)[:n],
                          (T(c.cm, dev), c.c0), out=None if tight else T(c.out, dev),
                          origin=T(c.origin, dev)[:n] if c.at else None)
    return {"out": r} if tight else None


Row("me_esa_argmin", ("me_esa_argmin",), _grid_cases([dict(rng=16, me_range=16, at=0), dict(rng=8, me_range=4, at=0),
                                                      dict(rng=24, me_range=16, at=0)]),
    _argmin_setup, _argmin_call, lambda c: {"out": c.out.mask()})
Row("me_esa_argmin_at", ("me_esa_argmin_at",), _grid_cases([dict(rng=16, me_range=16, at=1), dict(rng=8, me_range=8, at=1),
                                                            dict(rng=24, me_range=24, at=1), dict(rng=4, me_range=4, at=1)]),
    _argmin_setup, _argmin_call, lambda c: {"out": c.out.mask()})


# me_search_esa: "out[3*i] = { cost, mx, my }"
def _esa_setup(ar, bd, mbw, mbh, rng, me_range):
    n = 2 * mbw * mbh
    fe, (F,) = _me_content(ar, bd, 2, 16 * mbw, 16 * mbh, rng + mbh, hpel=False)
    par, init = _esa_par(rng + 3, mbw, mbh, 2, me_range)
    cm, c0 = _cost_table(ar)
    return _ns(bd=bd, n=n, mbw=mbw, mbh=mbh, rng=rng, me_range=me_range, fenc=fe, ref=F, cm=cm, c0=c0,
               par=_vals(ar, "par", n, np.int16, par, 8), init=_vals(ar, "init", n, np.int32, init),
               out=ar.list("out", (n, 3), np.int32))


def _esa_call(hip, c, dev, tight):
    r = hip.me_search_esa(c.fenc.t(dev), c.fenc.origin, c.fenc.stride, c.ref.t(dev), c.ref.origin, c.ref.stride, c.mbw,
                          c.mbh, 2, c.rng, c.me_range, T(c.par, dev)[:c.n], T(c.init, dev)[:c.n], (T(c.cm, dev), c.c0),
                          out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


Row("me_search_esa", ("me_search_esa",), _grid_cases([dict(rng=r, me_range=m) for r, m in ((4, 4), (8, 8), (16, 16),
                                                                                          (24, 16))]),
    _esa_setup, _esa_call, lambda c: {"out": c.out.mask()}, variants=ME_VARIANTS)


# me_search_esa8: "partition p of MB mb at index i = 8*mb + p ... out[3*i] = { cost, mx, my }"
def _esa8_setup(ar, bd, mbw, mbh, rng, me_range):
    import esa8_cases as e8
    nmb = mbw * mbh
    fe, (F,) = _me_content(ar, bd, 1, 16 * mbw, 16 * mbh, rng + 9, hpel=False)
    cen, par, init = e8.jobs(mbw, mbh, me_range, seed=rng + mbw, spread=4, frac=0.3, centre_amp=6, limit=8)
    cm, c0 = _cost_table(ar)
    return _ns(bd=bd, nmb=nmb, mbw=mbw, mbh=mbh, rng=rng, me_range=me_range, fenc=fe, ref=F, cm=cm, c0=c0,
               centre=_vals(ar, "centre", nmb, np.int16, cen, 2), par=_vals(ar, "par", 8 * nmb, np.int16, par, 8),
               init=_vals(ar, "init", 8 * nmb, np.int32, init), out=ar.list("out", (8 * nmb, 3), np.int32))


def _esa8_call(hip, c, dev, tight):
    r = hip.me_search_esa8(c.fenc.t(dev), c.fenc.origin, c.fenc.stride, c.ref.t(dev), c.ref.origin, c.ref.stride, c.mbw,
                           c.mbh, 1, c.rng, c.me_range, T(c.centre, dev)[:c.nmb], T(c.par, dev)[:8 * c.nmb],
                           T(c.init, dev)[:8 * c.nmb], (T(c.cm, dev), c.c0), out=None if tight else T(c.out, dev))
    return {"out": r} if tight else None


Row("me_search_esa8", ("me_search_esa8",), _grid_cases([dict(rng=8, me_range=8), dict(rng=16, me_range=12),
                                                        dict(rng=0, me_range=6)]),
    _esa8_setup, _esa8_call, lambda c: {"out": c.out.mask()})


# me_tesa: "out[4*i] = { cost, mx, my, number of COST_MV candidates }"
def _integral_of(ar, name, bd, F, lines, sub8x8, rows=None):
    """frame_integral's output for the plane buffer F, from the oracle; only what frame_integral writes
    may be read.  rows: the buffer's rows per frame (the 4x4 sums then start at row rows // 2)"""
    import oracle_lib as orc
    h = lines + 64
    out = ar.plane(name, F.nframes, F.width, lines, np.uint16, stride=F.stride, rows=rows or h * (2 if sub8x8 else 1))
    g = out.guard_rows
    half = (out.frame_rows // 2) if rows else h
    for f in range(F.nframes):
        buf = orc.frame_integral(bd, F.np(ar.host)[f].ravel(), F.origin, F.stride, lines, 32, int(sub8x8))
        for k in range(2 if sub8x8 else 1):
            r0 = g + k * half
            out.np(ar.host)[f, r0 + 1:r0 + lines + 56, :F.stride - 8] = buf[k * h + 1:k * h + lines + 56, :F.stride - 8]
            out.readable[f, r0 + 1:r0 + lines + 56, :F.stride - 8] = True
    return out


def _tesa_setup(ar, bd, mbw, mbh, me_range, satd):
    import tesa_cases as tc
    n = 2 * mbw * mbh
    W, H = 16 * mbw, 16 * mbh
    fe, (F,) = _me_content(ar, bd, 2, W, H, me_range + mbw, hpel=False)
    par, init = tc.params(mbw, mbh, me_range, seed=me_range + bd, nframes=2)
    cm, c0 = _cost_table(ar, span=16384)
    return _ns(bd=bd, n=n, mbw=mbw, mbh=mbh, me_range=me_range, satd=satd, fenc=fe, ref=F, cm=cm, c0=c0,
               integral=_integral_of(ar, "integral", bd, F, H, False), par=_vals(ar, "par", n, np.int16, par, 8),
               init=_vals(ar, "init", n, np.int32, init), out=ar.list("out", (n, 4), np.int32))


def _tesa_call(hip, c, dev, tight):
    r = hip.me_tesa(c.fenc.t(dev), c.fenc.origin, c.fenc.stride, c.ref.t(dev), c.ref.origin, c.ref.stride,
                    c.integral.t(dev), c.mbw, c.mbh, 2, c.me_range, T(c.par, dev)[:c.n], T(c.init, dev)[:c.n],
                    (T(c.cm, dev), c.c0), satd=c.satd, out=None if tight else T(c.out, dev),
                    integral_origin=c.integral.origin)
    return {"out": r} if tight else None


Row("me_tesa", ("me_tesa",), _grid_cases([dict(me_range=16, satd=1), dict(me_range=8, satd=0), dict(me_range=32, satd=1)]),
    # (X264HIP_TESA_VARIANT=1 forces the in-scan SADs, which me_range 32 takes anyway)
    _tesa_setup, _tesa_call, lambda c: {"out": c.out.mask()}, variants=[("X264HIP_TESA_VARIANT", 1)],
    variant_case=lambda bd, case: case["me_range"] <= 24)


# the partition-list entries: pos / par / mvc from refine_cases, search_cases and bidir_cases at 48x32
def _jobs_n(gen, n, i_pixel, seed):
    """the first n partitions of enough 48x32 frames; (arrays..., nframes)"""
    import refine_cases as rc
    per = (ME_W // 16) * (ME_H // 16) * len(rc.PARTS[i_pixel])
    nf = -(-n // per)
    return [a[:n] for a in gen(ME_W // 16, ME_H // 16, nf, i_pixel, seed)], nf


def _refine_setup(ar, bd, n, i_pixel, subme, form):
    import refine_cases as rc
    (pos, par, cost), nf = _jobs_n(rc.jobs, n, i_pixel, n + subme)
    fe, planes = _me_content(ar, bd, nf, ME_W, ME_H, n + i_pixel)
    cm, c0 = _cost_table(ar)
    c = _ns(bd=bd, n=n, i_pixel=i_pixel, subme=subme, form=form, fenc=fe, planes=planes, cm=cm, c0=c0,
            pos=_vals(ar, "pos", n, np.int32, pos, 3), par=_vals(ar, "par", n, np.int16, par, 8),
            cost=_vals(ar, "cost", n, np.int32, cost), out=ar.list("out", (n, 4), np.int32),
            nevals=ar.list("nevals", n, np.int32))
    if form == "refdupe":
        thr, rcost, c.exits = _thresholds(n)
        c.thresh = _vals(ar, "thresh", n, np.int32, thr)
        c.ref_cost = _vals(ar, "ref_cost", n, np.int32, rcost)
    return c


def _refine_call(hip, c, dev, tight):
    n, p0 = c.n, c.planes[0]
    args = (c.fenc.t(dev), c.fenc.origin, c.fenc.stride, [p.t(dev) for p in c.planes], p0.origin, p0.stride, c.i_pixel,
            c.subme, T(c.pos, dev)[:n], T(c.par, dev)[:n], T(c.cost, dev)[:n], (T(c.cm, dev), c.c0))
    kw = dict(out=None if tight else T(c.out, dev), nevals=T(c.nevals, dev))
    if c.form == "refdupe":
        r = hip.me_refine_qpel_refdupe(*args, halfpel_thresh=T(c.thresh, dev)[:n], ref_cost=T(c.ref_cost, dev)[:n],
                                       **kw)
        return {"out": r, "nevals": T(c.nevals, dev), "thresh": T(c.thresh, dev)} if tight else None
    ext = hip.refine_ext(0, 1, 0, ((40, 5, -3), None, None)) if c.form == "ex" else None
    r = hip.me_refine_subpel(*args, ext=ext, **kw)
    return {"out": r, "nevals": T(c.nevals, dev)} if tight else None


def _refine_masks(c):
    m = {"out": _out_mask(c), "nevals": c.nevals.mask()}
    if c.form == "refdupe":
        m["thresh"] = c.thresh.items(c.n)          # "read and written in place"
    return m


INT_MAX = (1 << 31) - 1


def _thresholds(n):
    """p_halfpel_thresh per item with a known exit set: refine_subpel leaves early iff
    (bcost * 7) >> 3 > *p_halfpel_thresh (encoder/me.c:934), and bcost holds two mv costs of at least
    29 each (refine_cases.cost_mv, lambda 40).  So a threshold of 0 (ref_cost 0) always exits and INT_MAX
    ("before its MB's first reference") never does.  Returns (thresh, ref_cost, exits)."""
    exits = np.arange(n) % 3 == 1
    return np.where(exits, 0, INT_MAX), np.where(exits, 0, np.arange(n) % 50), exits


def _out_mask(c):
    """me_search_ref_thresh: "When the exit fires the refine returns ... with m->cost, m->mv written and
    m->cost_mv left as it was: out[4*i+3] keeps what the caller stored there" """
    pm = np.ones((c.n, 4), bool)
    if getattr(c, "exits", None) is not None:
        pm[c.exits, 3] = False
    return c.out.mask(pm)


Row("me_refine_subpel", ("me_refine_subpel",),
    _list_cases([dict(i_pixel=0, subme=7, form="plain"), dict(i_pixel=3, subme=2, form="plain"),
                 dict(i_pixel=6, subme=9, form="plain")]), _refine_setup, _refine_call, _refine_masks)
Row("me_refine_subpel_ex", ("me_refine_subpel_ex",),
    _list_cases([dict(i_pixel=0, subme=7, form="ex"), dict(i_pixel=4, subme=4, form="ex")]), _refine_setup,
    _refine_call, _refine_masks)
Row("me_refine_qpel_refdupe", ("me_refine_qpel_refdupe",),
    _list_cases([dict(i_pixel=0, subme=7, form="refdupe"), dict(i_pixel=3, subme=4, form="refdupe")]), _refine_setup,
    _refine_call, _refine_masks)


def _search_setup(ar, bd, n, i_pixel, me_method, subme, form):
    import search_cases as sc
    (pos, par, mvc), nf = _jobs_n(sc.jobs, n, i_pixel, n + me_method)
    fe, planes = _me_content(ar, bd, nf, ME_W, ME_H, n + subme)
    cm, c0 = _cost_table(ar)
    c = _ns(bd=bd, n=n, i_pixel=i_pixel, me_method=me_method, subme=subme, form=form, fenc=fe, planes=planes, cm=cm,
            c0=c0, pos=_vals(ar, "pos", n, np.int32, pos, 3), par=_vals(ar, "par", n, np.int16, par, 12),
            mvc=_vals(ar, "mvc", n, np.int16, mvc, 28), out=ar.list("out", (n, 4), np.int32),
            nevals=ar.list("nevals", (n, 2), np.int32))
    if form != "plain":
        thr, rcost, c.exits = _thresholds(n)
        c.thresh = _vals(ar, "thresh", n, np.int32, thr)
        c.ref_cost = _vals(ar, "ref_cost", n, np.int32, rcost)
    if form == "tesa":
        F = planes[0]
        # the 8x8 sums in the first half of each frame's rows, the 4x4 sums in the second: the
        # wrapper takes the 4x4 plane at half the rows of a buffer twice the reference's
        c.integral = _integral_of(ar, "integral", bd, F, ME_H, True,
                                  rows=2 * F.frame_rows - (F.frame_rows - F.rows))
        c.scan = ar.list("scan", (n, 2), np.int32)
    return c


def _search_call(hip, c, dev, tight):
    n, p0 = c.n, c.planes[0]
    pl = [p.t(dev) for p in c.planes]
    a = (c.fenc.t(dev), c.fenc.origin, c.fenc.stride, pl[0], pl, p0.origin, p0.stride)
    b = (T(c.pos, dev)[:n], T(c.par, dev)[:n], T(c.mvc, dev)[:n], (T(c.cm, dev), c.c0))
    kw = dict(out=None if tight else T(c.out, dev), nevals=T(c.nevals, dev))
    if c.form != "plain":
        kw.update(halfpel_thresh=T(c.thresh, dev)[:n], ref_cost=T(c.ref_cost, dev)[:n])
    if c.form == "tesa":
        r = hip.me_search_ref_tesa(*a, c.integral.t(dev), c.i_pixel, c.subme, 16, *b, scan=T(c.scan, dev),
                                   integral_origin=c.integral.origin, **kw)
    else:
        r = hip.me_search_ref(*a, c.i_pixel, c.me_method, c.subme, 16, *b, **kw)
    if not tight:
        return None
    out = {"out": r, "nevals": T(c.nevals, dev)}
    if c.form != "plain":
        out["thresh"] = T(c.thresh, dev)
    if c.form == "tesa":
        out["scan"] = T(c.scan, dev)
    return out


def _search_masks(c):
    m = {"out": _out_mask(c), "nevals": c.nevals.mask()}
    if c.form != "plain":
        m["thresh"] = c.thresh.items(c.n)
    if c.form == "tesa":
        m["scan"] = c.scan.mask()
    return m


Row("me_search_ref", ("me_search_ref",),
    _list_cases([dict(i_pixel=0, me_method=1, subme=7, form="plain"), dict(i_pixel=3, me_method=2, subme=4, form="plain"),
                 dict(i_pixel=6, me_method=0, subme=1, form="plain"), dict(i_pixel=0, me_method=3, subme=2, form="plain")]),
    _search_setup, _search_call, _search_masks)
Row("me_search_ref_thresh", ("me_search_ref_thresh",),
    _list_cases([dict(i_pixel=0, me_method=1, subme=7, form="thresh"), dict(i_pixel=3, me_method=2, subme=4, form="thresh")]),
    _search_setup, _search_call, _search_masks)
Row("me_search_ref_tesa", ("me_search_ref_tesa",),
    _list_cases([dict(i_pixel=0, me_method=4, subme=7, form="tesa"), dict(i_pixel=3, me_method=4, subme=2, form="tesa"),
                 dict(i_pixel=6, me_method=4, subme=4, form="tesa")]),
    _search_setup, _search_call, _search_masks, variants=[("X264HIP_TESA_VARIANT", 1)])


# me_refine_bidir_satd: "out[4*i] = { m0 mv x, y, m1 mv x, y } ... cost (or NULL) ... nevals (or NULL)"
def _bidir_setup(ar, bd, n, i_pixel, satd):
    import bidir_cases as bc
    import refine_cases as rc
    per = 6 * len(rc.PARTS[i_pixel])
    nf = -(-n // per)
    mr = _ns(W=ME_W, H=ME_H, shifts=((3, 2), (-2, 1)))
    pos, par, wt = [np.concatenate(a) for a in zip(*[bc.jobs(mr, i_pixel, seed=n + f) for f in range(nf)])]
    pos[:, 0] = np.repeat(np.arange(nf), per)
    fe, l0 = _me_content(ar, bd, nf, ME_W, ME_H, n + 20)
    _, l1 = _me_content(ar, bd, nf, ME_W, ME_H, n + 21, prefix="b")
    cm, c0 = _cost_table(ar)
    return _ns(bd=bd, n=n, i_pixel=i_pixel, satd=satd, fenc=fe, l0=l0, l1=l1, cm=cm, c0=c0,
               pos=_vals(ar, "pos", n, np.int32, pos[:n], 3), par=_vals(ar, "par", n, np.int16, par[:n], 12),
               wt=_vals(ar, "wt", n, np.int32, wt[:n]), out=ar.list("out", (n, 4), np.int32),
               cost=ar.list("cost", n, np.int32), nevals=ar.list("nevals", n, np.int32))


def _bidir_call(hip, c, dev, tight):
    n, p0 = c.n, c.l0[0]
    r = hip.me_refine_bidir(c.fenc.t(dev), c.fenc.origin, c.fenc.stride, [p.t(dev) for p in c.l0],
                            [p.t(dev) for p in c.l1], p0.origin, p0.stride, c.i_pixel, T(c.pos, dev)[:n],
                            T(c.par, dev)[:n], T(c.wt, dev)[:n], (T(c.cm, dev), c.c0), satd=c.satd,
                            out=None if tight else T(c.out, dev), cost=T(c.cost, dev), nevals=T(c.nevals, dev))
    return {"out": r, "cost": T(c.cost, dev), "nevals": T(c.nevals, dev)} if tight else None


Row("me_refine_bidir_satd", ("me_refine_bidir_satd",),
    _list_cases([dict(i_pixel=0, satd=1), dict(i_pixel=3, satd=0), dict(i_pixel=1, satd=1)]), _bidir_setup, _bidir_call,
    lambda c: {"out": c.out.mask(), "cost": c.cost.mask(), "nevals": c.nevals.mask()})


# me_analyse_p16x16: "out[4*(f*mb_width*mb_height + mb)] = { m->cost, mvx, mvy, cost_mv } (raster); nevals ... as
# me_search_ref's"
def _p16_setup(ar, bd, mbw, mbh, me_method, subme):
    nmb = mbw * mbh
    fe, planes = _me_content(ar, bd, 2, 16 * mbw, 16 * mbh, mbw + subme)
    cm, c0 = _cost_table(ar)
    lr = np.random.default_rng(mbw).integers(-40, 40, (2, nmb, 2)).astype(np.int16)
    return _ns(bd=bd, mbw=mbw, mbh=mbh, me_method=me_method, subme=subme, fenc=fe, planes=planes, cm=cm, c0=c0,
               lowres_mv=ar.list("lowres_mv", (2, nmb, 2), np.int16, lr), out=ar.list("out", (2, nmb, 4), np.int32),
               nevals=ar.list("nevals", (2, nmb, 2), np.int32))


def _p16_call(hip, c, dev, tight):
    p0 = c.planes[0]
    pl = [p.t(dev) for p in c.planes]
    r = hip.me_analyse_p16x16(c.fenc.t(dev), c.fenc.origin, c.fenc.stride, pl[0], pl, p0.origin, p0.stride, c.mbw, c.mbh,
                              2, c.me_method, c.subme, 16, (T(c.cm, dev), c.c0), lowres_mv=T(c.lowres_mv, dev),
                              out=None if tight else T(c.out, dev), nevals=T(c.nevals, dev))
    return {"out": r, "nevals": T(c.nevals, dev)} if tight else None


Row("me_analyse_p16x16", ("me_analyse_p16x16",), _grid_cases([dict(me_method=1, subme=7), dict(me_method=2, subme=2)]),
    _p16_setup, _p16_call, lambda c: {"out": c.out.mask(), "nevals": c.nevals.mask()})


# ------------------------------------------------------------------ the lookahead
LA_SIZES = ((32, 32), (96, 16), (272, 48))


def _la_content(ar, bd, nf, W, H, seed):
    """the four lowres planes (F, H, V, C) of nf frames of one moving texture, from the oracle"""
    import oracle_lib as orc
    wl, hl = W // 2, H // 2
    base = _smooth(seed, bd, (H + 64 + 8 * nf, W + 64 + 8 * nf))
    bufs = [ar.plane("low" + k, nf, wl, hl, pdt(bd)) for k in "FHVC"]
    for f in range(nf):
        full = np.ascontiguousarray(base[3 * f:3 * f + H + 64, 2 * f:2 * f + W + 64])
        lows = orc.frame_init_lowres(bd, full.ravel(), 32 * (W + 64) + 32, W + 64, W, H, fp.plane_stride(wl))
        for b, low in zip(bufs, lows):
            b.picture(ar.host)[f] = low[:, :wl + 64]
    for b in bufs:
        g = b.guard_rows
        b.readable[:, g:g + b.rows, :wl + 64] = True
    return bufs


def _la_intra(bd, F, host, mbw, mbh, satd=True):
    import oracle_lib as orc
    return np.stack([orc.lowres_intra_cost(bd, F.np(host)[f].ravel(), F.origin, F.stride, mbw, mbh, satd)[0]
                     for f in range(F.nframes)])


def _la_cases(extra):
    return [("%dx%d-%s" % (W, H, "-".join("%s%s" % (k[0], v) for k, v in e.items())), dict(W=W, H=H, **e))
            for W, H in LA_SIZES for e in extra]


# lowres_intra_cost: "Outputs per frame f: intra_cost[f*mbw*mbh + mb], row_satd[f*mbh + y], cost_est[2f] / [2f+1]"
def _lai_setup(ar, bd, W, H, aq):
    mbw, mbh = W // 16, H // 16
    lows = _la_content(ar, bd, 2, W, H, W + aq)
    iq = np.random.default_rng(W).integers(100, 700, (2, mbw * mbh))
    return _ns(bd=bd, mbw=mbw, mbh=mbh, aq=aq, F=lows[0], iq=ar.list("iq", (2, mbw * mbh), np.int16, iq.astype(np.int16)),
               cost=ar.list("cost", (2, mbw * mbh), np.int16), rows=ar.list("rows", (2, mbh), np.int32),
               est=ar.list("est", (2, 2), np.int32))


def _lai_call(hip, c, dev, tight):
    r = hip.lowres_intra_cost(c.F.body(dev), c.F.stride, c.mbw, c.mbh, True, True, 4,
                              T(c.iq, dev) if c.aq else None,
                              outs=None if tight else (T(c.cost, dev), T(c.rows, dev), T(c.est, dev)))
    return dict(zip(("cost", "rows", "est"), r)) if tight else None


Row("lowres_intra_cost", ("lowres_intra_cost",), _la_cases([dict(aq=0), dict(aq=1)]), _lai_setup, _lai_call,
    lambda c: {"cost": c.cost.mask(), "rows": c.rows.mask(), "est": c.est.mask()})


# lowres_inter_cost_ex: "writes fenc->lowres_mvs (mvs[2*(f*mbs + mb)]), lowres_mv_costs (mv_costs), lowres_costs
# ..., row_satd[f*mbh + y] and est[3f..3f+2]"
def _lap_setup(ar, bd, W, H, weighted, n_slices):
    import oracle_lib as orc
    mbw, mbh = W // 16, H // 16
    nmb = mbw * mbh
    lows = _la_content(ar, bd, 3, W, H, W + weighted)
    F = lows[0]
    cm, c0 = orc.cost_mv_table(1, 512)
    c = _ns(bd=bd, mbw=mbw, mbh=mbh, weight=(58, 6, 3) if weighted else None, n_slices=n_slices, lows=lows, c0=c0,
            cm=ar.list("cost_mv", cm.size, np.int16, cm),
            intra=ar.list("intra", (2, nmb), np.int16, _la_intra(bd, F, ar.host, mbw, mbh)[1:]),
            mvs=ar.list("mvs", (2, nmb, 2), np.int16), mvc=ar.list("mv_costs", (2, nmb), np.int32),
            lc=ar.list("lowres_costs", (2, nmb), np.int16), rows=ar.list("row_satd", (2, mbh), np.int32),
            est=ar.list("est", (2, 3), np.int32), refw=None)
    if weighted:
        wl, hl = W // 2, H // 2
        c.refw = ar.plane("lowW", 3, wl, hl, pdt(bd))
        for f in range(3):
            flat = F.np(ar.host)[f].ravel()
            out = orc.weight_scale_plane(bd, flat, F.origin - 32 * F.stride - 32, F.stride, wl + 64, hl + 64, *c.weight)
            g = F.guard_rows
            c.refw.picture(ar.host)[f] = out.reshape(F.shape[1:])[g:g + F.rows, :wl + 64]
        c.refw.readable[:, F.guard_rows:F.guard_rows + F.rows, :wl + 64] = True
    return c


def _lap_call(hip, c, dev, tight):
    outs = None if tight else tuple(T(b, dev) for b in (c.mvs, c.mvc, c.lc, c.rows, c.est))
    r = hip.lowres_inter_cost(c.lows[0].body(dev)[1:], [p.body(dev)[:-1] for p in c.lows], c.lows[0].stride, c.mbw, c.mbh,
                              T(c.intra, dev), (T(c.cm, dev), c.c0), outs=outs,
                              ref_w=None if c.refw is None else c.refw.body(dev)[:-1], weight=c.weight,
                              n_slices=c.n_slices, check=getattr(c, "check", True))
    return dict(zip(("mvs", "mv_costs", "lowres_costs", "row_satd", "est"), r)) if tight else None


Row("lowres_inter_cost_ex", ("lowres_inter_cost_ex",),
    _la_cases([dict(weighted=0, n_slices=1), dict(weighted=1, n_slices=1), dict(weighted=0, n_slices=2),
               dict(weighted=1, n_slices=2)]),
    _lap_setup, _lap_call,
    lambda c: {b.name: b.mask() for b in (c.mvs, c.mvc, c.lc, c.rows, c.est)})


# lowres_bidir_cost_ex: "List l is searched ... when search & (1 << l) -- writing mvs_l / costs_l -- else read
# from them.  Writes lowres_costs, row_satd[f*mbh + y] and est[2f..2f+1]": the unsearched list's mvs and
# costs are inputs and come back bit for bit
def _lab_setup(ar, bd, W, H, search, n_slices):
    import oracle_lib as orc
    mbw, mbh = W // 16, H // 16
    nmb = mbw * mbh
    lows = _la_content(ar, bd, 4, W, H, W + search)
    cm, c0 = orc.cost_mv_table(1, 512)
    rs = np.random.default_rng(W + search)
    c = _ns(bd=bd, mbw=mbw, mbh=mbh, search=search, n_slices=n_slices, lows=lows, c0=c0,
            cm=ar.list("cost_mv", cm.size, np.int16, cm), lc=ar.list("lowres_costs", (2, nmb), np.int16),
            rows=ar.list("row_satd", (2, mbh), np.int32), est=ar.list("est", (2, 2), np.int32), mvs=[], costs=[])
    for l in (0, 1):
        searched = search >> l & 1
        c.mvs.append(ar.list("mvs%d" % l, (2, nmb, 2), np.int16, None if searched else rs.integers(-6, 7, (2, nmb, 2))))
        c.costs.append(ar.list("costs%d" % l, (2, nmb), np.int32, None if searched else rs.integers(50, 900, (2, nmb))))
    return c


def _lab_call(hip, c, dev, tight):
    body = [p.body(dev) for p in c.lows]
    r = hip.lowres_bidir_cost(body[0][1:3], [p[0:2] for p in body], [p[2:4] for p in body], c.lows[0].stride, c.mbw,
                              c.mbh, (T(c.cm, dev), c.c0), c.search, T(c.mvs[0], dev), T(c.costs[0], dev),
                              T(c.mvs[1], dev), T(c.costs[1], dev), dist_scale_factor=128, bipred_weight=32,
                              outs=None if tight else (T(c.lc, dev), T(c.rows, dev), T(c.est, dev)),
                              n_slices=c.n_slices, check=getattr(c, "check", True))
    if not tight:
        return None
    out = dict(zip(("lowres_costs", "row_satd", "est"), r))
    for l in (0, 1):
        if c.search >> l & 1:
            out["mvs%d" % l], out["costs%d" % l] = T(c.mvs[l], dev), T(c.costs[l], dev)
    return out


def _lab_masks(c):
    m = {b.name: b.mask() for b in (c.lc, c.rows, c.est)}
    for l in (0, 1):
        if c.search >> l & 1:
            m["mvs%d" % l], m["costs%d" % l] = c.mvs[l].mask(), c.costs[l].mask()
    return m


Row("lowres_bidir_cost_ex", ("lowres_bidir_cost_ex",),
    _la_cases([dict(search=3, n_slices=1), dict(search=1, n_slices=2), dict(search=2, n_slices=1),
               dict(search=0, n_slices=2)]), _lab_setup, _lab_call, _lab_masks)


# weight_cost_batch: "costs[i] (device uint32) = the reference's value with cands[i]"
def _wc_frames(ar, bd, kind, W, H):
    """fenc and ref planes of weightp_cases.make_pair in the arena: (fenc, refs, intra or None, mbw, mbh)"""
    import oracle_lib as orc
    import weightp_cases as wc
    cf = {0: 0, 1: 1, 3: 3}[kind]
    ref, fenc = wc.make_pair(bd, W, H, cf, (1.1, -6), ((0.9, 4), (1.2, -3)), seed=bd + kind)
    mbw, mbh = W // 16, H // 16
    if kind == 0:
        an = wc.Analysis(orc, ref, fenc, search_mvs=False)
        wl, hl = W // 2, H // 2
        f = ar.plane("fenc", 1, wl, hl, pdt(bd), an.fenc_lr[0][None, :, :wl + 64])
        refs = [ar.plane("ref%d" % k, 1, wl, hl, pdt(bd), p[None, :, :wl + 64]) for k, p in enumerate(an.ref_lr)]
        return f, refs, an, mbw, mbh
    if kind == 1:
        f = ar.plane("fenc", 1, W, H // 2, pdt(bd), fenc.nv[None, :, :W + 64])
        return f, [ar.plane("ref0", 1, W, H // 2, pdt(bd), ref.nv[None, :, :W + 64])], None, mbw, mbh
    f = ar.plane("fenc", 1, W, H, pdt(bd), fenc.u[None, :, :W + 64])
    return f, [ar.plane("ref0", 1, W, H, pdt(bd), ref.u[None, :, :W + 64])], None, mbw, mbh


def _wcb_setup(ar, bd, n, kind, with_mvs):
    import weightp_cases as wc
    f, refs, an, mbw, mbh = _wc_frames(ar, bd, kind, 64, 48)
    c = _ns(bd=bd, n=n, kind=kind, fenc=f, refs=refs, mbw=mbw, mbh=mbh, cands=wc.candidates(n + kind, n=max(n, 6))[:n],
            intra=None if an is None else ar.list("intra", mbw * mbh, np.int16, an.intra),
            mvs=ar.list("mvs", (mbw * mbh, 2), np.int16, wc.random_mvs(mbw, mbh, 5 + kind, lim=24)) if with_mvs else None,
            costs=ar.list("costs", n, np.int32))
    return c


def _wcb_call(hip, c, dev, tight):
    r = hip.weight_cost_batch(c.kind, c.fenc.t(dev), [p.t(dev) for p in c.refs], c.fenc.origin, c.fenc.stride, c.mbw, c.mbh,
                              c.cands, intra_cost=None if c.intra is None else T(c.intra, dev),
                              mvs=None if c.mvs is None else T(c.mvs, dev), lam=3, n_slices=2,
                              out=None if tight else T(c.costs, dev))
    return {"costs": r} if tight else None


Row("weight_cost_batch", ("weight_cost_batch",),
    [("n%d-k%d-m%d" % (n, k, m), dict(n=n, kind=k, with_mvs=m)) for n in (1, 63, 65, 70) for k, m in
     ((0, 0), (0, 1), (1, 1), (3, 0))], _wcb_setup, _wcb_call, lambda c: {"costs": c.costs.mask()})


# weights_analyse: "weighted_lowres ... by x264_weight_scale_plane over columns [-32, width + 32) and the rows of
# the 32-row border ... columns [-PADH_ALIGN, -32) ... keep whatever the caller's buffer held" -- plus the strip
# rounding weight_scale_plane states ("up to 7 columns past width are written too")
def _wa_setup(ar, bd, W, H):
    import oracle_lib as orc
    import weightp_cases as wc
    ref, fenc = wc.make_pair(bd, W, H, 0, (0.8, 20.0), seed=W + bd)
    an = wc.Analysis(orc, ref, fenc)
    wl, hl = W // 2, H // 2
    c = _ns(bd=bd, mbw=an.mbw, mbh=an.mbh, wl=wl, hl=hl, fstats=an.fstats, rstats=an.rstats,
            fenc=ar.plane("fenc", 1, wl, hl, pdt(bd), an.fenc_lr[0][None, :, :wl + 64]),
            refs=[ar.plane("ref%d" % k, 1, wl, hl, pdt(bd), p[None, :, :wl + 64]) for k, p in enumerate(an.ref_lr)],
            intra=ar.list("intra", an.mbw * an.mbh, np.int16, an.intra),
            mvs=ar.list("mvs", (an.mbw * an.mbh, 2), np.int16, an.mvs), out=ar.plane("weighted", 1, wl, hl, pdt(bd)))
    want, _ = orc.weights_analyse(bd, an.fenc_lr[0].ravel(), [p.ravel() for p in an.ref_lr], an.lo, an.ls, an.mbw,
                                  an.mbh, an.intra, an.fstats, an.rstats, mvs=an.mvs)
    c.found = bool(want[0][0])
    return c


def _wa_call(hip, c, dev, tight):
    import torch
    out = torch.zeros_like(c.fenc.body(dev)[0]) if tight else c.out.body(dev)[0]
    w, _ = hip.weights_analyse(c.fenc.body(dev)[0], [p.body(dev)[0] for p in c.refs], c.fenc.stride, c.mbw, c.mbh,
                               T(c.intra, dev), c.fstats, c.rstats, mvs=T(c.mvs, dev), weighted_lowres=out)
    assert bool(w[0][0]) == c.found
    return {"weighted": out[None]} if tight else None


def _wa_masks(c):
    assert c.found, "the fade of this case has a luma weight"
    return {"weighted": fp.weight_scale_mask(c.out, -32, -32, c.wl + 64, c.hl + 64)}


Row("weights_analyse", ("weights_analyse",), [("%dx%d" % s, dict(W=s[0], H=s[1])) for s in ((64, 48), (96, 32), (272, 48))],
    _wa_setup, _wa_call, _wa_masks)


# ------------------------------------------------------------------ plane statistics: small outputs, guards only;
# regions whose width and height are off a multiple of 4 and 16, so a kernel that rounds its reads up reads fill
def _region(ar, name, bd, nf, W, H, seed):
    """nf W x H regions with no padding: the pointer is the region's top-left, nothing else is readable"""
    return ar.plane(name, nf, W, H, pdt(bd), pix(seed, bd, (nf, H, W)), pad_x=0, pad_y=0)


def _ssd_setup(ar, bd, W, H, nv12):
    a, b = _region(ar, "pix1", bd, 2, W * (2 if nv12 else 1), H, W), _region(ar, "pix2", bd, 2, W * (2 if nv12 else 1), H, H)
    return _ns(bd=bd, W=W, H=H, nv12=nv12, a=a, b=b, out=ar.list("ssd", (2, 2) if nv12 else (2,), np.int64))


def _ssd_call(hip, c, dev, tight):
    fn = hip.ssd_nv12_batch if c.nv12 else hip.ssd_plane_batch
    r = fn(c.a.t(dev), c.a.origin, c.a.stride, c.b.t(dev), c.b.origin, c.b.stride, c.W, c.H, 2,
           out=None if tight else T(c.out, dev))
    return {"ssd": r} if tight else None


_SSD_SIZES = [("%dx%d" % s, dict(W=s[0], H=s[1])) for s in ((50, 19), (13, 5), (129, 33), (16, 16))]
Row("ssd_plane_batch", ("ssd_plane_batch",), [(i, dict(nv12=0, **c)) for i, c in _SSD_SIZES], _ssd_setup, _ssd_call,
    lambda c: {"ssd": c.out.mask()})
Row("ssd_nv12_batch", ("ssd_nv12_batch",), [(i, dict(nv12=1, **c)) for i, c in _SSD_SIZES], _ssd_setup, _ssd_call,
    lambda c: {"ssd": c.out.mask()})


# ssim_wxh: "*ssim (device float) ... Reads 4x4 blocks up to column 4*(width/4) - 1 and row 4*(height/4) - 1"
def _ssim_setup(ar, bd, W, H):
    w4, h4 = W // 4 * 4, H // 4 * 4
    return _ns(bd=bd, W=W, H=H, a=_region(ar, "pix1", bd, 1, w4, h4, W), b=_region(ar, "pix2", bd, 1, w4, h4, H),
               out=ar.list("ssim", 1, np.float32))


def _ssim_call(hip, c, dev, tight):
    import torch
    out = torch.empty(1, dtype=torch.float32, device="cuda") if tight else T(c.out, dev)
    hip.ssim_wxh(c.a.t(dev), c.a.origin, c.a.stride, c.b.t(dev), c.b.origin, c.b.stride, c.W, c.H, out=out, wait=False)
    return {"ssim": out} if tight else None


Row("ssim_wxh", ("ssim_wxh",), [("%dx%d" % s, dict(W=s[0], H=s[1])) for s in ((50, 19), (13, 9), (131, 34), (16, 16))],
    _ssim_setup, _ssim_call, lambda c: {"ssim": c.out.mask()})


# ssim_bands: "ssim (device float[n_frames * n_bands]) = each band's float"
def _bands_setup(ar, bd, W, H):
    import x264hip
    bands = x264hip.ssim_encoder_bands(H // 16, H)
    return _ns(bd=bd, W=W, H=H, nb=len(bands), a=ar.plane("pix1", 2, W, H, pdt(bd), pix(W, bd, (2, H + 64, W + 64))),
               b=ar.plane("pix2", 2, W, H, pdt(bd), pix(H, bd, (2, H + 64, W + 64))),
               bands=_vals(ar, "bands", len(bands), np.int32, bands, 2), out=ar.list("ssim", (2, len(bands)), np.float32))


def _bands_call(hip, c, dev, tight):
    r = hip.ssim_bands(c.a.t(dev), c.a.origin + 2, c.a.stride, c.b.t(dev), c.b.origin + 2, c.b.stride, c.W - 2,
                       T(c.bands, dev)[:c.nb], out=None if tight else T(c.out, dev))
    return {"ssim": r} if tight else None


Row("ssim_bands", ("ssim_bands",), [("%dx%d" % s, dict(W=s[0], H=s[1])) for s in ((48, 32), (80, 16), (272, 48))],
    _bands_setup, _bands_call, lambda c: {"ssim": c.out.mask()})


# frame_pixel_stats: "stats = device uint64[6]: sum[0..2] then ssd[0..2]"
def _fps_setup(ar, bd, W, H, cf):
    c = _ns(bd=bd, mbw=W // 16, mbh=H // 16, cf=cf, luma=ar.plane("luma", 1, W, H, pdt(bd), pix(W, bd, (1, H + 64, W + 64))),
            out=ar.list("stats", 6, np.int64), nv=None)
    if cf:
        c.nv = ar.plane("nv", 1, W, H // 2, pdt(bd), pix(H, bd, (1, H // 2 + 64, W + 64)))
    return c


def _fps_call(hip, c, dev, tight):
    r = hip.frame_pixel_stats(c.luma.t(dev), c.luma.origin, c.luma.stride, c.mbw, c.mbh, c.cf,
                              None if c.nv is None else c.nv.t(dev), None, 0 if c.nv is None else c.nv.origin,
                              0 if c.nv is None else c.nv.stride, out=None if tight else T(c.out, dev))
    return {"stats": r} if tight else None


Row("frame_pixel_stats", ("frame_pixel_stats",),
    [("%dx%d-cf%d" % (W, H, cf), dict(W=W, H=H, cf=cf)) for W, H in ((16, 16), (48, 32), (272, 48)) for cf in (0, 1)],
    _fps_setup, _fps_call, lambda c: {"stats": c.out.mask()})


# upload_plane / upload_planes: "the edge element ... repeated over pad_x bytes left and right, then rows 0 and
# height-1 with their pads over pad_y rows above and below": the picture and its pads.  aligned_only: "width_bytes,
# pad_x and both strides multiples of 16, both pointers 16-byte aligned" rules the +4 stride out.
_PINNED = {}


def _pinned(bd, W, H, seed):
    import torch
    key = (bd, W, H, seed)
    if key not in _PINNED:
        _PINNED[key] = torch.from_numpy(pix(seed, bd, (H, W)).view(np.int16 if bd == 10 else np.uint8)).pin_memory()
    return _PINNED[key]


def _up_setup(ar, bd, W, H, both):
    c = _ns(bd=bd, W=W, H=H, both=both, luma=ar.plane("luma", 1, W, H, pdt(bd)), nv=None)
    if both:
        c.nv = ar.plane("nv", 1, W, H // 2, pdt(bd), pad_y=16)
    return c


def _up_call(hip, c, dev, tight):
    es = 1 if c.bd == 8 else 2
    y = _pinned(c.bd, c.W, c.H, 1)
    if not c.both:
        hip.upload_plane(c.luma.t(dev), c.luma.origin, c.luma.stride, y, unit=es, pad_x=32 * es, pad_y=32)
        return {"luma": c.luma.t(dev)} if tight else None
    uv = _pinned(c.bd, c.W, c.H // 2, 2)
    hip.upload_planes([hip.plane_upload(c.luma.t(dev), c.luma.origin, c.luma.stride, y, unit=es, pad_x=32 * es, pad_y=32),
                       hip.plane_upload(c.nv.t(dev), c.nv.origin, c.nv.stride, uv, unit=2 * es, pad_x=32 * es, pad_y=16)])
    return {"luma": c.luma.t(dev), "nv": c.nv.t(dev)} if tight else None


def _up_masks(c):
    m = {"luma": c.luma.rect(-32, c.W + 32, -32, c.H + 32)}
    if c.both:
        m["nv"] = c.nv.rect(-32, c.W + 32, -16, c.H // 2 + 16)
    return m


_UP_SIZES = ((16, 2), (48, 18), (272, 48))
Row("upload_plane", ("upload_plane",), [("%dx%d" % s, dict(W=s[0], H=s[1], both=0)) for s in _UP_SIZES], _up_setup,
    _up_call, _up_masks)
Row("upload_planes", ("upload_planes",), [("%dx%d" % s, dict(W=s[0], H=s[1], both=1)) for s in _UP_SIZES], _up_setup,
    _up_call, _up_masks)


# mbtree_propagate (x264hip_mbtree.h): the destination planes ref_costs, read-modify-write, one element per MB
def _mbp_setup(ar, bd, w, h, n_steps):
    import mbtree_cases as mt
    n = w * h
    rng = np.random.default_rng(n + n_steps)
    dst = [rng.integers(0, 20000, n).astype(np.uint16) for _ in range(2)]
    c = _ns(w=w, h=h, n=n, dst=[_vals(ar, "ref_costs%d" % k, n, np.int16, d.view(np.int16)) for k, d in enumerate(dst)],
            steps=[])
    for k in range(n_steps):
        s = mt.crafted_step(rng, w, h, dst, ("mid", "none", "max")[k], (0.0013, 1 / 512, 0.19)[k], (32, 21, 21)[k],
                            referenced=k != 1)

        def put(name, a, fields=None):
            return None if a is None else _vals(ar, "%s%d" % (name, k), n, np.int16, a.view(np.int16), fields)
        c.steps.append(_ns(intra=put("intra", s.intra_cost), costs=put("costs", s.lowres_costs), invq=put("invq", s.inv_qscale),
                           pin=put("pin", s.propagate_in), mv0=put("mv0", s.mvs[0], 2), mv1=put("mv1", s.mvs[1], 2),
                           fps=s.fps_factor, weight=s.bipred_weight))
    return c


def _mbp_call(hip, c, dev, tight):
    n = c.n

    def t(b):
        return None if b is None else T(b, dev)[:n]
    steps = [hip.mbtree_step(t(s.intra), t(s.costs), t(s.mv0), t(c.dst[0]), s.fps, t(s.mv1), t(c.dst[1]), t(s.invq),
                             t(s.pin), s.weight) for s in c.steps]
    hip.mbtree_propagate(steps, c.w, c.h)
    return {b.name: T(b, dev) for b in c.dst} if tight else None


_MB_GRIDS = ((1, 1), (3, 2), (17, 1))
Row("mbtree_propagate", ("mbtree_propagate",),
    [("%dx%d-s%d" % (w, h, k), dict(w=w, h=h, n_steps=k)) for w, h in _MB_GRIDS for k in (1, 3)], _mbp_setup, _mbp_call,
    lambda c: {b.name: b.items(c.n) for b in c.dst})


# mbtree_finish: "qp_offset ... elements whose scaled intra cost is 0 are not written"
def _mbf_setup(ar, bd, w, h, aq):
    n = w * h
    rng = np.random.default_rng(n + aq)
    intra = np.where(rng.random(n) < 0.3, rng.integers(1, 40, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    invq = np.where(rng.random(n) < 0.4, rng.integers(1, 4, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    ic = (intra.astype(np.int64) * (invq if aq else 256) + 128) >> 8
    return _ns(n=n, aq=aq, written=ic != 0, intra=_vals(ar, "intra", n, np.int16, intra.view(np.int16)),
               invq=_vals(ar, "invq", n, np.int16, invq.view(np.int16)),
               prop=_vals(ar, "prop", n, np.int16, rng.integers(0, 32768, n).astype(np.int16)),
               qp_aq=_vals(ar, "qp_aq", n, np.float32, rng.uniform(-3, 3, n).astype(np.float32)),
               qp=ar.list("qp_offset", n, np.float32))


def _mbf_call(hip, c, dev, tight):
    n = c.n
    hip.mbtree_finish(T(c.intra, dev)[:n], T(c.prop, dev)[:n], T(c.qp_aq, dev)[:n], 5 if c.aq else 512, 0.3, 2.0,
                      inv_qscale=T(c.invq, dev)[:n] if c.aq else None, qp_offset=T(c.qp, dev))
    return {"qp_offset": T(c.qp, dev)} if tight else None


Row("mbtree_finish", ("mbtree_finish",),
    [("%dx%d-aq%d" % (w, h, a), dict(w=w, h=h, aq=a)) for w, h in _MB_GRIDS + ((33, 9),) for a in (0, 1)], _mbf_setup,
    _mbf_call, lambda c: {"qp_offset": c.qp.mask(c.written)})
