"""GPU parity: the deblocking filter and its strengths (x264hip_*_deblock_frames,
x264hip_deblock_strength, include/x264hip_deblock.h; reference common/deblock.c:277-606)
bit-exact against tests/deblock_cases.py's numpy restatement, which tests/test_cpu_deblock.py
holds to hand-worked vectors and to conditions on these very inputs (the filter changes >= 25 %
of the luma pixels, and filtering in another order gives another picture).

Every plane sits inside a larger buffer of a sentinel value (8 rows above and below, 16 columns
left and right, so frame strides are larger than the plane), and the sentinel is checked after
every call.  The sizes are the smallest that reach each hazard: 5x4 MBs have left, top and
top-right neighbours and an interior MB; 1x1 .. 2x2 the first and last diagonals and diagonals
of one MB; 24x14 MBs x 2 frames diagonals of more than one workgroup."""
import types

import numpy as np
import pytest
import torch

import deblock_cases as dc
import footprint as fp
import stream_cases as sc

pytestmark = pytest.mark.gpu

GY, GX, SENTINEL = 8, 16, 7


def _t(a, bd):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if bd == 10 else a).cuda()


def _n(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


def _embed(a):
    nf, h, w = a.shape
    buf = np.full((nf, h + 2 * GY, w + 2 * GX), SENTINEL, a.dtype)
    buf[:, GY:GY + h, GX:GX + w] = a
    return buf


def _crop(buf, like):
    nf, h, w = like.shape
    out = buf[:, GY:GY + h, GX:GX + w]
    rest = buf.copy()
    rest[:, GY:GY + h, GX:GX + w] = SENTINEL
    assert (rest == SENTINEL).all(), "pixels outside the picture were written"
    return out


def _gpu(hip, c):
    """deblock_frames on the inputs c: (luma, [chroma planes]) as the checker returns them"""
    bd = c.bd
    luma = _t(_embed(c.luma), bd)
    planes = [_t(_embed(p), bd) for p in c.chroma]
    stride = c.luma.shape[2] + 2 * GX
    chroma = None
    if c.cf:
        cs = c.chroma[0].shape[2] + 2 * GX
        chroma = (c.cf, planes, GY * cs + GX, cs)
    hip.deblock_frames(luma, GY * stride + GX, stride, c.mbw, c.mbh, torch.from_numpy(c.qp.copy()).cuda(),
                       torch.from_numpy(c.mb_flags.copy()).cuda(), torch.from_numpy(c.bs.copy()).cuda(), chroma=chroma,
                       alpha_c0_offset=c.alpha_c0_offset, beta_offset=c.beta_offset,
                       chroma_qp_index_offset=c.chroma_qp_index_offset, qp_table=c.chroma_qp_table,
                       slice_table=None if c.slice_table is None else torch.from_numpy(c.slice_table.copy()).cuda())
    torch.cuda.synchronize()
    return _crop(_n(luma, bd), c.luma), [_crop(_n(p, bd), q) for p, q in zip(planes, c.chroma)]


def _same(got, want):
    assert len(got[1]) == len(want[1])
    for name, g, w in [("luma", got[0], want[0])] + [("chroma %d" % k, g, w) for k, (g, w) in enumerate(zip(got[1], want[1]))]:
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %d of %d pixels differ, first at (frame, row, col) %s: got %d, want %d" % (
            name, len(bad), w.size, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


# ------------------------------------------------------------------ 1. the picture
@pytest.mark.parametrize("key", [e[1] for e in dc.gpu_keys("frames")], ids=dc.case_id)
def test_deblock_frames(hip, key):
    _same(_gpu(hip, dc.make_case(*key)), dc.expected(key))


@pytest.mark.parametrize("key", [e[1] for e in dc.gpu_keys("low_qp")], ids=dc.case_id)
def test_low_qp_changes_nothing(hip, key):
    """qp 0..15: qp <= qp_thresh and alpha = 0 -- nothing changes, as the checker says"""
    c = dc.make_case(*key)
    want = dc.expected(key)
    assert np.array_equal(want[0], c.luma)
    _same(_gpu(hip, c), want)


@pytest.mark.parametrize("key", [e[1] for e in dc.gpu_keys("slices")], ids=dc.case_id)
def test_slices(hip, key):
    """two slices split mid-row: the edges across the split are untouched; the same call with NULL
    filters them"""
    c = dc.make_case(*key)
    with_table = _gpu(hip, c)
    _same(with_table, dc.expected(key))
    free = dc.with_(c, slice_table=None)
    without = _gpu(hip, free)
    _same(without, dc.deblock(free))
    assert not np.array_equal(with_table[0], without[0])


def test_n_zero_and_errors(hip):
    c = dc.make_case(*dc.MAIN[0])
    luma = _t(_embed(c.luma), 8)
    before = luma.clone()
    args = (torch.from_numpy(c.qp.copy()).cuda(), torch.from_numpy(c.mb_flags.copy()).cuda(),
            torch.from_numpy(c.bs.copy()).cuda())
    stride = c.luma.shape[2] + 2 * GX
    hip.deblock_frames(luma, GY * stride + GX, stride, c.mbw, c.mbh, *args, nframes=0)
    hip.deblock_frames(luma, GY * stride + GX, stride, 0, c.mbh, *args)
    torch.cuda.synchronize()
    assert torch.equal(luma, before)
    with pytest.raises(RuntimeError):
        hip.deblock_frames(luma, GY * stride + GX, stride, c.mbw, c.mbh, *args, alpha_c0_offset=13)
    with pytest.raises(RuntimeError):
        hip.deblock_frames(luma, GY * stride + GX, stride, c.mbw, c.mbh, *args, chroma=(4, [], 0, 0))
    with pytest.raises(RuntimeError):
        hip.deblock_frames(luma, GY * stride + GX, stride, -1, c.mbh, *args)
    s = dc.make_strength_case(5, 4, 2, False)
    dev = [torch.from_numpy(a.copy()).cuda() for a in (s.nz, s.mb_flags, s.mv[0], s.ref[0])]
    with pytest.raises(RuntimeError):
        hip.deblock_strength(*dev, s.mbw, s.mbh, s.nf, mvy_limit=0)
    bs = torch.full((s.nf * 20, 2, 4, 4), 9, dtype=torch.uint8, device="cuda")
    hip.deblock_strength(*dev, s.mbw, s.mbh, 0, bs=bs)
    torch.cuda.synchronize()
    assert (bs == 9).all()


# ------------------------------------------------------------------ 2. the strengths
def _strength_gpu(hip, s, mvy_limit):
    d = lambda a: torch.from_numpy(a.copy()).cuda()
    bs = hip.deblock_strength(d(s.nz), d(s.mb_flags), d(s.mv[0]), d(s.ref[0]), s.mbw, s.mbh, s.nf,
                              mv1=d(s.mv[1]) if s.bframe else None, ref1=d(s.ref[1]) if s.bframe else None,
                              mvy_limit=mvy_limit)
    torch.cuda.synchronize()
    return bs.cpu().numpy()


@pytest.mark.parametrize("mvy_limit", [4, 2])
@pytest.mark.parametrize("bframe", [False, True], ids=["P", "B"])
@pytest.mark.parametrize("shape", dc.STRENGTH_SHAPES, ids=["5x4x2", "24x14x1"])
def test_deblock_strength(hip, shape, bframe, mvy_limit):
    assert ("strength", shape + (bframe,), mvy_limit) in dc.gpu_keys("strength")
    s = dc.make_strength_case(*shape, bframe)
    want = dc.deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf, mvy_limit)
    got = _strength_gpu(hip, s, mvy_limit)
    bad = np.argwhere(got != want)
    assert not len(bad), "%d of %d strengths differ, first at (mb, dir, edge, i) %s" % (len(bad), want.size, bad[0])
    assert set(np.unique(want)) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("entry", dc.gpu_keys("boundary"),
                         ids=lambda e: dc.case_id(e[1]) if e[0] == "frames" else "strength-%s-%d" % ("B" if e[1][3] else "P", e[2]))
def test_boundary_cases_bit_exact(hip, entry):
    """the pictures of deblock_cases.BOUNDARY -- steps across the edges that equal alpha, beta and
    (alpha >> 2) + 2 at the foot of the qp range, at both depths and in every chroma layout -- and
    the small fields of BOUNDARY_STRENGTH with vector steps of exactly the limit: a kernel that
    takes `<` for `<=` in a line filter, or `>=` for `>` in the strength rule, differs here"""
    want = dc.gpu_expected(entry)
    if entry[0] == "frames":
        _same(_gpu(hip, dc.make_case(*entry[1])), want)
    else:
        got = _strength_gpu(hip, dc.make_strength_case(*entry[1]), entry[2])
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ------------------------------------------------------------------ 3. the chain
def test_chain_residual_strength_deblock(hip):
    """mb_mc -> mb_dct_quant -> mb_dequant_idct_add -> deblock_strength -> deblock_frames at 5x4 MBs,
    8 bit: the device's nz goes into deblock_strength as it is, the search's vectors (one per 16x16
    block) are spread over the MB's 4x4 blocks on the device, and the checker, run on the GPU's
    reconstruction and nz copied back, gives the same strengths and the same picture"""
    import checkasm_bufs as cb
    import mc_cases as mcc
    import refine_cases as rc
    import search_cases as scs
    from x264hip import synth
    bd, w, h = 8, 80, 64
    mbw, mbh = w // 16, h // 16
    luma, stride, origin, nv, cs, co = synth.make_subpel_sequence(2, w, h, bd)
    planes = [luma[:1]] + [p[None] for p in mcc.nr.hpel_planes(luma[0], 32, w, h, bd)]
    dl = [_t(p, bd) for p in planes]
    fenc = _t(luma[1:], bd)
    pos, spar, mvc = scs.jobs(mbw, mbh, 1, 0, seed=13)
    cm, c0 = rc.cost_mv()
    dpos = torch.from_numpy(pos).cuda()
    out = hip.me_search_ref(fenc, origin, stride, dl[0], dl, origin, stride, 0, 1, 7, 16, dpos,
                            torch.from_numpy(spar).cuda(), torch.from_numpy(mvc).cuda(),
                            (torch.from_numpy(cm.view(np.int16)).cuda(), c0))
    lim = np.stack(mcc.mv_limits(pos[:, 1], pos[:, 2], mbw, mbh), 1).astype(np.int16)
    par = torch.zeros((len(pos), 8), dtype=torch.int16, device="cuda")
    par[:, 0:2] = out[:, 1:3].to(torch.int16)
    par[:, 4:8] = torch.from_numpy(lim).cuda()
    pred, _ = hip.mb_mc(dl, None, origin, stride, 0, dpos, par)
    q4m, q4b, _, _ = hip.cqm_init(bd, [cb.FLAT16] * 8)
    dq4, _ = hip.cqm_dequant([cb.FLAT16] * 8)
    qp = 40
    dct, nz = hip.mb_dct_quant(4, fenc, origin, stride, pred, origin, stride, mbw, mbh, 1,
                               torch.from_numpy(q4m[1, qp].copy()).cuda(), torch.from_numpy(q4b[1, qp].copy()).cuda())
    qps = torch.full((mbw * mbh,), qp, dtype=torch.int32, device="cuda")
    rec = torch.zeros_like(pred)
    hip.mb_dequant_idct_add(4, dct, mbw, mbh, 1, torch.from_numpy(dq4[1].copy()).cuda(), qps, pred, origin, stride,
                            rec, origin, stride)
    # h->mb.mv / h->mb.ref of a P frame of 16x16 partitions: the MB's vector in its sixteen blocks
    # (the jobs are the MBs in raster order), reference 0; flag bit 2 where nothing was coded
    assert np.array_equal(pos[:, 1:], np.stack(np.mgrid[0:mbh, 0:mbw][::-1], -1).reshape(-1, 2) * 16)
    mv4 = out[:, 1:3].to(torch.int16).view(1, mbh, mbw, 2).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    ref8 = torch.zeros((1, 2 * mbh, 2 * mbw), dtype=torch.int8, device="cuda")
    flags = ((nz == 0) * 4).to(torch.uint8)
    bs = hip.deblock_strength(nz, flags, mv4, ref8, mbw, mbh)
    rec_before = _n(rec, bd).copy()
    qp8 = qps.to(torch.int8)
    hip.deblock_frames(rec, origin, stride, mbw, mbh, qp8, flags, bs)
    torch.cuda.synchronize()
    nz_h, flags_h, mv_h = nz.cpu().numpy(), flags.cpu().numpy(), mv4.cpu().numpy()
    want_bs = dc.deblock_strength_py(nz_h, flags_h, [mv_h], [ref8.cpu().numpy()], mbw, mbh, 1)
    assert np.array_equal(bs.cpu().numpy(), want_bs)
    assert nz_h.any() and {0, 2} <= set(np.unique(want_bs))
    oy, ox = origin // stride, origin % stride
    c = types.SimpleNamespace(bd=bd, cf=0, mbw=mbw, mbh=mbh, nf=1, luma=rec_before[:, oy:oy + h, ox:ox + w], chroma=[],
                              qp=np.full(mbw * mbh, qp, np.int8), mb_flags=flags_h, bs=want_bs, slice_table=None,
                              alpha_c0_offset=0, beta_offset=0, chroma_qp_index_offset=0,
                              chroma_qp_table=dc.chroma_qp_table(bd))
    want = dc.deblock(c)
    got = _n(rec, bd)
    assert np.array_equal(got[:, oy:oy + h, ox:ox + w], want[0])
    # the filter acted on the reconstruction: more than 1 % of 5120 pixels is more than a dozen
    # filtered lines (a line changes at most 6 pixels), so more than one edge segment
    assert (want[0] != c.luma).mean() > 0.01
    rest, rest0 = got.copy(), rec_before.copy()
    rest[:, oy:oy + h, ox:ox + w] = rest0[:, oy:oy + h, ox:ox + w] = 0
    assert np.array_equal(rest, rest0)                                # and on nothing else


# ------------------------------------------------------------------ 4. footprint
FKEYS = [dc.key(8, 1, 5, 4, nf=2, seed=8), dc.key(10, 2, 5, 4, nf=2, seed=8), dc.key(8, 3, 3, 3, nf=2, seed=8)]


def _frames_setup(ar, bd, key=None):
    c = dc.make_case(*key)
    dt = dc.pdt(bd)
    w, h = 16 * c.mbw, 16 * c.mbh
    n = c.nf * c.mbw * c.mbh
    ns = types.SimpleNamespace(c=c, bd=bd)
    ns.luma = ar.plane("luma", c.nf, w, h, dt, c.luma, pad_x=0, pad_y=0)
    ns.chroma = [ar.plane("chroma%d" % k, c.nf, p.shape[2], p.shape[1], dt, p, pad_x=0, pad_y=0)
                 for k, p in enumerate(c.chroma)]
    ns.qp = ar.list("qp", n, np.int8, c.qp)
    ns.flags = ar.list("mb_flags", n, np.uint8, c.mb_flags)
    ns.bs = ar.list("bs", (n, 2, 4, 4), np.uint8, c.bs)
    return ns


def _frames_call(hip, ns, dev, tight):
    c = ns.c
    chroma = None
    if c.cf:
        chroma = (c.cf, [sc.T(b, dev) for b in ns.chroma], ns.chroma[0].origin, ns.chroma[0].stride)
    hip.deblock_frames(sc.T(ns.luma, dev), ns.luma.origin, ns.luma.stride, c.mbw, c.mbh, sc.T(ns.qp, dev),
                       sc.T(ns.flags, dev), sc.T(ns.bs, dev), chroma=chroma, qp_table=c.chroma_qp_table)


def _strength_setup(ar, bd, bframe=True):
    s = dc.make_strength_case(5, 4, 2, bframe)
    n = s.nf * s.mbw * s.mbh
    ns = types.SimpleNamespace(s=s, bd=bd)
    ns.nz = ar.list("nz", n, np.int32, s.nz)
    ns.flags = ar.list("mb_flags", n, np.uint8, s.mb_flags)
    ns.mv = [ar.list("mv%d" % l, m.shape, np.int16, m) for l, m in enumerate(s.mv)]
    ns.ref = [ar.list("ref%d" % l, r.shape, np.int8, r) for l, r in enumerate(s.ref)]
    ns.bs = ar.list("bs", (n, 2, 4, 4), np.uint8)
    return ns


def _strength_call(hip, ns, dev, tight):
    s = ns.s
    hip.deblock_strength(sc.T(ns.nz, dev), sc.T(ns.flags, dev), sc.T(ns.mv[0], dev), sc.T(ns.ref[0], dev), s.mbw, s.mbh,
                         s.nf, mv1=sc.T(ns.mv[1], dev) if s.bframe else None,
                         ref1=sc.T(ns.ref[1], dev) if s.bframe else None, bs=sc.T(ns.bs, dev))


def _two_fills(hip, setup, call, bd, **case):
    out = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill)
        ns = setup(ar, bd, **case)
        dev = ar.device()
        call(hip, ns, dev, False)
        torch.cuda.synchronize()
        out.append((ar, ns, dev.cpu().numpy()))
    return out


@pytest.mark.parametrize("key", FKEYS, ids=dc.case_id)
def test_frames_footprint(hip, key):
    """guard bands round every buffer, two fills: only the picture area of the planes is written,
    every other buffer comes back as it was, and the result does not depend on the bands"""
    (a1, n1, after1), (a2, n2, after2) = _two_fills(hip, _frames_setup, _frames_call, key[0], key=key)
    c = n1.c
    masks = {b.name: b.rect(0, b.width, 0, b.height) for b in [n1.luma] + n1.chroma}
    fp.check_arena(a1, after1, a2, after2, masks)
    want = dc.expected(key)
    for ar, ns, after in ((a1, n1, after1), (a2, n2, after2)):
        got = (ns.luma.picture(after), [b.picture(after) for b in ns.chroma])
        _same(got, want)
    assert c.nf == 2


@pytest.mark.parametrize("bframe", [False, True], ids=["P", "B"])
def test_strength_footprint(hip, bframe):
    (a1, n1, after1), (a2, n2, after2) = _two_fills(hip, _strength_setup, _strength_call, 8, bframe=bframe)
    fp.check_arena(a1, after1, a2, after2, {"bs": n1.bs.mask(True)})
    s = n1.s
    want = dc.deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf)
    assert np.array_equal(n1.bs.data(after1), want) and np.array_equal(n2.bs.data(after2), want)


# ------------------------------------------------------------------ 5. stream order
# rows for tests/stream_cases.py's helpers (Prepared / null_run / side_run / differing, unchanged):
# both entries on a side stream behind the delay kernel and the upload of their inputs
FRAMES_ROW = types.SimpleNamespace(name="deblock_frames", entries=("deblock_frames",),
                                   cases=[("5x4x2", {"key": None})], setup=None, call=_frames_call)
STRENGTH_ROW = types.SimpleNamespace(name="deblock_strength", entries=("deblock_strength",),
                                     cases=[("5x4x2-B", {"bframe": True})], setup=_strength_setup, call=_strength_call)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("entry", ["deblock_frames", "deblock_strength"])
def test_behind_delay(hip, entry, bd):
    if entry == "deblock_frames":
        key = dc.key(bd, 1, 5, 4, nf=2, seed=8)
        row = types.SimpleNamespace(**{**vars(FRAMES_ROW), "cases": [("5x4x2", {"key": key})], "setup": _frames_setup})
    else:
        row = STRENGTH_ROW
    p = sc.Prepared(row, bd)
    want = sc.null_run(hip, p)
    # the null-stream run is the checker's result
    if entry == "deblock_frames":
        _same((p.c.luma.picture(want), [b.picture(want) for b in p.c.chroma]), dc.expected(key))
    else:
        s = p.c.s
        assert np.array_equal(p.c.bs.data(want), dc.deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf))
    got, ended = sc.side_run(hip, p, torch.cuda.Stream())
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    assert not ended, "%s: the delay kernel in front of the call had ended when the call returned" % entry
