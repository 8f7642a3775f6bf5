"""GPU parity: batched motion compensation (x264hip_*_mb_mc, include/x264hip_mc.h; reference
common/macroblock.c:31-246, common/mc.c:49-283) bit-exact against tests/mc_cases.py's numpy
restatement (pinned to the oracle by tests/test_cpu_mc.py): every partition size and chroma format
over every luma and chroma phase with vectors into the padding and beyond the limits, explicit
weights (denom >= 1 and 0) that clip at both ends, B blocks mixing the lists with every bipred
weight, untouched pixels under a checkerboard with all strides different, mode == NULL / n == 0 /
repeatability, the search -> prediction -> residual -> reconstruction chain, and whole 1080p
frames.  8 and 10 bit; frames are 96x64, two per call, unless a test says otherwise."""
import functools
import types

import numpy as np
import pytest
import torch

import checkasm_bufs as cb
import mc_cases as mcc
import refine_cases as rc
import search_cases as sc

pytestmark = pytest.mark.gpu

W, H, NF = 96, 64, 2
NONE3 = (None, None, None)
BIWEIGHTS = np.array([32, 24, 44, -8, 72])


def _t(a, bd):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if bd == 10 else a).cuda()


def _n(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


@functools.lru_cache(maxsize=None)
def _ref(bd, cf, seed, level="mid", w=W, h=H, nf=NF):
    """a reference list's pictures, computed once and shared (never modified)"""
    return mcc.make_ref(bd, w, h, cf, nf, seed, level)


@functools.lru_cache(maxsize=None)
def _dev(bd, cf, seed, level="mid", w=W, h=H, nf=NF):
    r = _ref(bd, cf, seed, level, w, h, nf)
    return [_t(p, bd) for p in r.luma], [_t(p, bd) for p in r.chroma]


def _gapped(t, gap):
    """the same planes with `gap` unused rows between frames (another frame stride)"""
    big = torch.zeros((t.shape[0], t.shape[1] + gap, t.shape[2]), dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def _gpu(hip, bd, cf, i_pixel, k0, k1, pos, par, mode, weights, geom=(0, 0, 32, 32, 32, 32), sentinel=0, cgap=0):
    """x264hip's mb_mc into sentinel-filled planes of geometry geom = (rows_extra, stride_extra, p_oy,
    p_ox, c_oy, c_ox); k0 / k1: the _ref keys of the lists (k1 None: list 1 unused); cgap: rows
    between the reference's chroma frames.  Returns (pred, pred_c) as numpy."""
    r0 = _ref(*k0)
    l0, c0 = _dev(*k0)
    l1, c1 = _dev(*k1) if k1 is not None else (None, None)
    if cgap:
        c0, c1 = [_gapped(t, cgap) for t in c0], [_gapped(t, cgap) for t in c1]
    re, se, p_oy, p_ox, c_oy, c_ox = geom
    pred, pred_c = mcc.pred_planes(r0, sentinel, re, se)
    pt, pct = _t(pred, bd), [_t(c, bd) for c in pred_c]
    ps = pred.shape[2]
    pcs = pred_c[0].shape[2] if pred_c else 0
    chroma = (cf, c0, c1, r0.corigin, r0.cs) if cf else None
    hip.mb_mc(l0, l1, r0.origin, r0.stride, i_pixel, torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda(),
              None if mode is None else torch.from_numpy(mode).cuda(), chroma=chroma, weight=weights,
              outs=(pt, p_oy * ps + p_ox, ps, pct, c_oy * pcs + c_ox, pcs))
    return _n(pt, bd), [_n(c, bd) for c in pct]


def _want(bd, cf, i_pixel, k0, k1, pos, par, mode, weights, geom=(0, 0, 32, 32, 32, 32), sentinel=0, stats=None):
    r0 = _ref(*k0)
    r1 = _ref(*k1) if k1 is not None else None
    re, se, p_oy, p_ox, c_oy, c_ox = geom
    pred, pred_c = mcc.pred_planes(r0, sentinel, re, se)
    st = mcc.mb_mc(bd, cf, i_pixel, r0, r1, pos, par, mode, weights, pred, p_oy, p_ox, pred_c, c_oy, c_ox, stats)
    return pred, pred_c, st


def _same(got, want, tag=()):
    (gp, gc), (wp, wc_) = got, want
    bad = np.argwhere(gp != wp)
    assert not len(bad), (*tag, "luma", len(bad), bad[:4], gp[tuple(bad[0])], wp[tuple(bad[0])])
    assert len(gc) == len(wc_)
    for k, (a, b) in enumerate(zip(gc, wc_)):
        bad = np.argwhere(a != b)
        assert not len(bad), (*tag, "chroma", k, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


def _mode(lists, biw):
    return (np.asarray(lists) | (np.asarray(biw) << 8)).astype(np.int32)


# ------------------------------------------------------------------ 1. phases
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2, 3])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
def test_phases(hip, bd, cf, i_pixel):
    """list 0, every block of both frames: calls whose blocks walk through all 64 eighth-pel phases
    (so all 16 qpel phases) with random legal integer parts, then one call of vectors on and beyond
    mv_min / mv_max"""
    key = (bd, cf, 3 + bd + cf)
    pos = mcc.block_positions(W, H, NF, i_pixel)
    n = len(pos)
    zero = np.zeros((n, 2), np.int64)
    st = {}
    for rnd in range(-(-64 // n) + 1):
        edge = rnd == -(-64 // n)
        mv = mcc.edge_mvs(pos, W, H, 50 + i_pixel) if edge else mcc.phase_mvs(pos, W, H, 7 * rnd + i_pixel, base=rnd * n)
        par = mcc.make_par(pos, mv, zero, W, H)
        before = st.get("clipped", 0)
        wp, wc_, st = _want(bd, cf, i_pixel, key, None, pos, par, None, NONE3, stats=st)
        if edge:
            assert st["clipped"] > before + n // 4          # the clip changed many of these blocks' mvs
        else:
            assert st["clipped"] == before
            assert (mv < 0).any() and (mv[:, 0] > 4 * (W - pos[:, 1])).any()    # negative, and past the frame
        _same(_gpu(hip, bd, cf, i_pixel, key, None, pos, par, None, NONE3), (wp, wc_), (rnd,))
    assert st["luma_phases"] == set(range(16))
    if cf == 1:
        assert st["chroma_phases"] == set(range(64))
    elif cf == 2:                                           # mc_chroma( mvx, 2 * mvy ): dy is even
        assert st["chroma_phases"] == {(dy << 3) + dx for dy in (0, 2, 4, 6) for dx in range(8)}


# ------------------------------------------------------------------ 2. weights
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("wt", [(70, 6, -3), (2, 0, 5)])
@pytest.mark.parametrize("place", ["luma", "chroma", "all"])
def test_weights(hip, bd, wt, place):
    """mc->weight on list-0 blocks (mode == NULL and an all-list-0 mode array): on bright planes the
    unclipped values pass PIXEL_MAX, on dark ones the negative offset takes them below 0"""
    weights = {"luma": (wt, None, None), "chroma": (None, wt, wt), "all": (wt, wt, (wt[0] + 1, wt[1], -wt[2]))}[place]
    over = under = False
    for cf, i_pixel, level in ((1, 0, "bright"), (1, 6, "dark"), (2, 3, "dark"), (2, 5, "bright"), (3, 1, "bright"),
                               (3, 4, "dark")):
        key = (bd, cf, 11 + cf, level)
        pos = mcc.block_positions(W, H, NF, i_pixel)
        par = mcc.make_par(pos, mcc.phase_mvs(pos, W, H, 3 + i_pixel), np.zeros((len(pos), 2), np.int64), W, H)
        mode = None if i_pixel & 1 else _mode(np.ones(len(pos), np.int64), 32)
        wp, wc_, st = _want(bd, cf, i_pixel, key, None, pos, par, mode, weights)
        _same(_gpu(hip, bd, cf, i_pixel, key, None, pos, par, mode, weights), (wp, wc_), (cf, i_pixel, level))
        over |= st["over"]
        under |= st["under"]
        plain = _want(bd, cf, i_pixel, key, None, pos, par, mode, NONE3)
        assert (plain[0] != wp).any() == (place != "chroma")
        assert any((a != b).any() for a, b in zip(plain[1], wc_)) == (place != "luma")
    assert over
    assert under == (wt[2] < 0 or place == "all")           # only a negative offset goes below 0


# ------------------------------------------------------------------ 3. B blocks
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2, 3])
@pytest.mark.parametrize("i_pixel", [0, 3, 5])
def test_b_blocks(hip, bd, cf, i_pixel):
    """one call mixing list 0, list 1 and bipred blocks with every bipred weight on full-scale
    planes (the weighted average clips at both ends) and a weighted mc->weight, which reaches the
    list-0 blocks only"""
    k0, k1 = (bd, cf, 21, "full"), (bd, cf, 22, "full")
    pos = mcc.block_positions(W, H, NF, i_pixel)
    n = len(pos)
    mv1 = mcc.phase_mvs(pos, W, H, 5, base=9)
    mv1[::5] = mcc.edge_mvs(pos, W, H, 6)[::5]
    par = mcc.make_par(pos, mcc.phase_mvs(pos, W, H, 4), mv1, W, H)
    lists = np.arange(n) % 3 + 1
    mode = _mode(lists, BIWEIGHTS[(np.arange(n) // 3) % 5])
    weights = ((70, 6, -3), (2, 0, 5), (33, 5, 12))
    wp, wc_, st = _want(bd, cf, i_pixel, k0, k1, pos, par, mode, weights)
    assert st["over"] and st["under"] and st["clipped"] > 0
    assert all(((mode >> 8) == w).any() and (((mode >> 8) == w) & (lists == 3)).any() for w in BIWEIGHTS)
    _same(_gpu(hip, bd, cf, i_pixel, k0, k1, pos, par, mode, weights), (wp, wc_))
    # without the weight only the list-0 blocks differ (restatement), and the GPU agrees there too
    up, uc, _ = _want(bd, cf, i_pixel, k0, k1, pos, par, mode, NONE3)
    bw, bh = mcc.PIXEL_SIZES[i_pixel]
    for (f, x, y), l in zip(pos.tolist(), lists.tolist()):
        diff = (up[f, 32 + y:32 + y + bh, 32 + x:32 + x + bw] != wp[f, 32 + y:32 + y + bh, 32 + x:32 + x + bw]).any()
        assert l == 1 or not diff
    assert (up != wp).any()
    _same(_gpu(hip, bd, cf, i_pixel, k0, k1, pos, par, mode, NONE3), (up, uc))


# ------------------------------------------------------------------ 4. untouched pixels, strides
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("i_pixel", [0, 4, 6])
def test_untouched_pixels_and_strides(hip, bd, cf, i_pixel):
    """blocks on a checkerboard of the frame into sentinel-filled planes whose strides, frame strides
    and origins all differ from the reference's and from each other: every pixel no block covers
    still holds the sentinel"""
    k0, k1 = (bd, cf, 31), (bd, cf, 32)
    sentinel = 0xA5 if bd == 8 else 0x3A5
    geom, cgap = (3, 32, 5, 12, 9, 8), 7
    pos = mcc.block_positions(W, H, NF, i_pixel, checker=True)
    n = len(pos)
    par = mcc.make_par(pos, mcc.phase_mvs(pos, W, H, 8), mcc.phase_mvs(pos, W, H, 9, base=3), W, H)
    mode = _mode(np.arange(n) % 3 + 1, BIWEIGHTS[np.arange(n) % 5])
    r0 = _ref(*k0)
    wp, wc_, _ = _want(bd, cf, i_pixel, k0, k1, pos, par, mode, NONE3, geom, sentinel)
    # luma, chroma, prediction and chroma prediction: four strides and four frame strides (4:4:4's
    # chroma planes share the luma stride by definition, not the frame stride)
    strides = {r0.stride, r0.cs, wp.shape[2], wc_[0].shape[2]}
    fstrides = {r0.luma[0][0].size, r0.chroma[0][0].size + cgap * r0.cs, wp[0].size, wc_[0][0].size}
    assert len(strides) == (3 if cf == 3 else 4) and len(fstrides) == 4
    bw, bh = mcc.PIXEL_SIZES[i_pixel]
    covered = np.zeros(wp.shape, bool)
    for f, x, y in pos.tolist():
        covered[f, 5 + y:5 + y + bh, 12 + x:12 + x + bw] = True
    assert (wp[~covered] == sentinel).all() and 0.05 < covered.mean() < 0.5
    assert (wc_[0] == sentinel).mean() > 0.5
    _same(_gpu(hip, bd, cf, i_pixel, k0, k1, pos, par, mode, NONE3, geom, sentinel, cgap), (wp, wc_))


# ------------------------------------------------------------------ 5. mode == NULL, n == 0, repeatability
@pytest.mark.parametrize("bd", [8, 10])
def test_mode_null_empty_and_repeat(hip, bd):
    cf, i_pixel = 1, 3
    key = (bd, cf, 41)
    pos = mcc.block_positions(W, H, NF, i_pixel)
    par = mcc.make_par(pos, mcc.phase_mvs(pos, W, H, 2), mcc.edge_mvs(pos, W, H, 3), W, H)
    ones = _mode(np.ones(len(pos), np.int64), 44)            # the bipred weight of a list-0 block is not read
    a = _gpu(hip, bd, cf, i_pixel, key, None, pos, par, None, NONE3, sentinel=9)
    b = _gpu(hip, bd, cf, i_pixel, key, None, pos, par, ones, NONE3, sentinel=9)
    c = _gpu(hip, bd, cf, i_pixel, key, None, pos, par, ones, NONE3, sentinel=9)
    _same(a, b)
    _same(b, c)
    _same(a, _want(bd, cf, i_pixel, key, None, pos, par, None, NONE3, sentinel=9)[:2])
    e = _gpu(hip, bd, cf, i_pixel, key, None, pos[:0], par[:0], None, NONE3, sentinel=9)
    assert (e[0] == 9).all() and (e[1][0] == 9).all()
    e = _gpu(hip, bd, cf, i_pixel, key, None, pos[:0], par[:0], ones[:0], NONE3, sentinel=9)
    assert (e[0] == 9).all() and (e[1][0] == 9).all()
    # allocating form: zeroed planes shaped like the references
    r0 = _ref(*key)
    l0, c0 = _dev(*key)
    pred, pred_c = hip.mb_mc(l0, None, r0.origin, r0.stride, i_pixel, torch.from_numpy(pos).cuda(),
                             torch.from_numpy(par).cuda(), chroma=(cf, c0, None, r0.corigin, r0.cs))
    _same((_n(pred, bd), [_n(t, bd) for t in pred_c]), _want(bd, cf, i_pixel, key, None, pos, par, None, NONE3)[:2])
    with pytest.raises(RuntimeError):
        hip.mb_mc(l0, None, r0.origin, r0.stride, 7, torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda())


# ------------------------------------------------------------------ 6. search -> mc -> residual -> reconstruction
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3])
def test_chain_search_mc_residual(hip, oracle, bd, i_pixel):
    """me_search_ref (HEX, subme 7) of a quarter-pel sequence's frame 1 in frame 0, its pos and out
    into mb_mc, the prediction into mb_dct_quant and mb_dequant_idct_add: every stage equals its
    restatement on the previous stage's output"""
    from x264hip import synth
    luma, stride, origin, nv, cs, co = synth.make_subpel_sequence(2, W, H, bd)
    planes = [luma[:1]] + [p[None] for p in mcc.nr.hpel_planes(luma[0], 32, W, H, bd)]
    ref = types.SimpleNamespace(luma=planes, oy=32, ox=32, chroma=[nv[:1]], coy=co // cs, cox=co % cs, cf=1)
    dl, dn = [_t(p, bd) for p in planes], _t(nv[:1], bd)
    fenc = _t(luma[1:], bd)
    pos, spar, mvc = sc.jobs(W // 16, H // 16, 1, i_pixel, seed=5 + bd)
    cm, c0 = rc.cost_mv()
    dpos = torch.from_numpy(pos).cuda()
    out = hip.me_search_ref(fenc, origin, stride, dl[0], dl, origin, stride, i_pixel, 1, 7, 16, dpos,
                            torch.from_numpy(spar).cuda(), torch.from_numpy(mvc).cuda(),
                            (torch.from_numpy(cm.view(np.int16)).cuda(), c0))
    # par of mb_mc on the device, from the search's out: (mv, unused list 1, h->mb.mv_min / mv_max)
    lim = np.stack(mcc.mv_limits(pos[:, 1], pos[:, 2], W // 16, H // 16), 1).astype(np.int16)
    par = torch.zeros((len(pos), 8), dtype=torch.int16, device="cuda")
    par[:, 0:2] = out[:, 1:3].to(torch.int16)
    par[:, 4:8] = torch.from_numpy(lim).cuda()
    pred, pred_c = hip.mb_mc(dl, None, origin, stride, i_pixel, dpos, par, chroma=(1, [dn], None, co, cs))
    mv = out.cpu().numpy()[:, 1:3]
    assert (mv != 0).any(1).mean() > 0.5 and (mv & 3).any()           # the search found subpel motion
    wp = np.zeros_like(luma[:1])
    wc_ = [np.zeros_like(nv[:1])]
    mcc.mb_mc(bd, 1, i_pixel, ref, None, pos, par.cpu().numpy(), None, NONE3, wp, 32, 32, wc_, co // cs, co % cs)
    _same((_n(pred, bd), [_n(pred_c[0], bd)]), (wp, wc_))
    # residual and reconstruction on that prediction (flat16 lists, QP 26, inter)
    mbw, mbh = W // 16, H // 16
    q4m, q4b, _, _ = hip.cqm_init(bd, [cb.FLAT16] * 8)
    dq4, _ = hip.cqm_dequant([cb.FLAT16] * 8)
    qp = 26 + 6 * (bd - 8)
    dct, nz = hip.mb_dct_quant(4, fenc, origin, stride, pred, origin, stride, mbw, mbh, 1,
                               torch.from_numpy(q4m[1, qp].copy()).cuda(), torch.from_numpy(q4b[1, qp].copy()).cuda())
    wd, wn = oracle.mb_dct_quant(bd, 4, luma[1].ravel(), origin, stride, wp[0].ravel(), origin, stride, mbw, mbh,
                                 q4m[1, qp], q4b[1, qp])
    assert np.array_equal(dct.cpu().numpy(), wd) and np.array_equal(nz.cpu().numpy(), wn)
    qps = np.full(mbw * mbh, qp, np.int32)
    rec = torch.zeros_like(pred)
    hip.mb_dequant_idct_add(4, dct, mbw, mbh, 1, torch.from_numpy(dq4[1].copy()).cuda(), torch.from_numpy(qps).cuda(),
                            pred, origin, stride, rec, origin, stride)
    wr = np.zeros_like(wp[0]).ravel()
    oracle.mb_dequant_idct_add(bd, 4, wd, mbw, mbh, dq4[1], qps, wp[0].ravel(), origin, stride, wr, origin, stride)
    assert np.array_equal(_n(rec, bd)[0].ravel(), wr)
    # the motion-compensated prediction is what makes the residual small: far fewer coded MBs than
    # with the co-located block
    _, nz0 = oracle.mb_dct_quant(bd, 4, luma[1].ravel(), origin, stride, luma[0].ravel(), origin, stride, mbw, mbh,
                                 q4m[1, qp], q4b[1, qp])
    assert np.count_nonzero(wn) <= np.count_nonzero(nz0)


# ------------------------------------------------------------------ 7. grid size
def test_1080p_4x4_blocks(hip):
    """one 1920x1088 8-bit 4:2:0 frame of 4x4 blocks: 130 560 blocks, 2x2 chroma blocks"""
    key = (8, 1, 51, "mid", 1920, 1088, 1)
    pos = mcc.block_positions(1920, 1088, 1, 6)
    assert len(pos) == 130560
    mv = mcc.phase_mvs(pos, 1920, 1088, 12)
    mv[::7] = mcc.edge_mvs(pos, 1920, 1088, 13)[::7]
    par = mcc.make_par(pos, mv, np.zeros_like(mv), 1920, 1088)
    wp, wc_, st = _want(8, 1, 6, key, None, pos, par, None, NONE3)
    assert st["clipped"] > 1000 and len(st["chroma_phases"]) == 64
    _same(_gpu(hip, 8, 1, 6, key, None, pos, par, None, NONE3), (wp, wc_))


def test_1080p_16x16_bipred(hip):
    """one 1920x1088 8-bit 4:2:0 frame of 16x16 blocks, every block bipred"""
    k0, k1 = (8, 1, 51, "mid", 1920, 1088, 1), (8, 1, 52, "mid", 1920, 1088, 1)
    pos = mcc.block_positions(1920, 1088, 1, 0)
    n = len(pos)
    par = mcc.make_par(pos, mcc.phase_mvs(pos, 1920, 1088, 14), mcc.phase_mvs(pos, 1920, 1088, 15, base=17), 1920, 1088)
    mode = _mode(np.full(n, 3), BIWEIGHTS[np.arange(n) % 5])
    wp, wc_, _ = _want(8, 1, 0, k0, k1, pos, par, mode, NONE3)
    _same(_gpu(hip, 8, 1, 0, k0, k1, pos, par, mode, NONE3), (wp, wc_))
