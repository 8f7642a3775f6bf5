"""GPU parity on degenerate content (tests/degenerate_cases.py): the motion-search kernels against
the oracle, bit-exact in results, costs, call counts and thresholds, on constant, near-flat and
periodic planes -- where candidates cost the same and the order equal costs resolve in decides
the result: the packed (cost << 4) + code of the predictor / DIA / hexagon / square rounds, the
ESA kernels' (cost, raster index) keys, the bidir refine's j order, the threshold comparisons
across identical references -- and on full-scale planes (fenc all max against references all 0,
and the swap), where packed codes and 16-bit partial sums would overflow first; under mv-cost
lambdas 40 (only the ties symmetric about mvp stay), 1 and 0 (every SAD tie is a cost tie).
tests/test_cpu_degenerate.py pins the oracle to the Python restatements on this content, the tie
rates of these lists and their reach inside the padding.  The inputs go through the existing
GPU test files' _run helpers; a failing message names kind, lambda, size, subme, then the
helper's partition indices, got and want."""
import numpy as np
import pytest
import torch

import degenerate_cases as dg
import esa8_cases as ec
import refine_cases as rc
import tesa_cases as tc
import test_gpu_analyse as tga
import test_gpu_bidir as tgb
import test_gpu_esa8 as tge
import test_gpu_lookahead as tgl
import test_gpu_refine_chroma as tgr
import test_gpu_search as tgs
import test_gpu_tesa_search as tgt

pytestmark = pytest.mark.gpu

W, H = dg.GW, dg.GH
NONE = (None, None, None)
# the kinds of the frame-level entries: their sequences hold both of extreme's roles (fenc max on
# a zero reference in the first pair, the swap in the second)
PLANE_KINDS = ("const", "nearflat", "periodic", "extreme")


def _t(a, bd):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if bd == 10 else a).cuda()


# ---------------------------------------------------------------- me_search_ref
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("me_method", [0, 1, 2, 3])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("kind", dg.KINDS)
def test_search(hip, oracle, bd, me_method, i_pixel, kind):
    """96x64, two frame pairs per launch (the sub-8x8 sizes on corner_rows' partitions), me_range
    16, subme 1 and 7 (chroma ME), lambda 40 / 1 / 0; on const and nearflat also the
    collapsed-limit jobs (x limits one column on every third partition, y limits one row on
    every fifth)"""
    cases = dg.search_cases(kind, bd, i_pixel)
    lists = [("", dg.search_jobs(bd, i_pixel))]
    if kind in ("const", "nearflat"):
        lists.append(("collapsed", dg.search_jobs(bd, i_pixel, collapsed=True)))
    for name, jobs in lists:
        for lam in dg.LAMBDAS:
            for subme in (1, 7):
                tgs._run(hip, oracle, bd, 1, W, H, 2, i_pixel, me_method, subme, 16, 0, int(subme >= 5), 0,
                         cases=cases, jobs=jobs, cost=rc.cost_mv(lam=lam), tag=(kind, name, lam, i_pixel, subme))


def _refdupe(hip, oracle, bd, mr, jobs, i_pixel, me_method, subme, cost, tag):
    """test_gpu_search.test_refdupe on a given MultiRef: reference 0's search by the oracle, then
    me_refine_qpel_refdupe from its result with the threshold it left"""
    cf = 1
    rows, crows = mr.fenc_y.size // mr.stride, mr.fenc_c[0].size // mr.cs
    r = mr.refs[0]
    fenc = _t(mr.fenc_y.reshape(1, rows, -1), bd)
    luma = [_t(p.reshape(1, rows, -1), bd) for p in r.luma]
    ext = hip.refine_ext(1, cf, 0, NONE, fenc_chroma=[_t(mr.fenc_c[0].reshape(1, crows, -1), bd)],
                         fenc_chroma_origin=mr.co, fenc_chroma_stride=mr.cs,
                         ref_chroma=[_t(r.ref_c[0].reshape(1, crows, -1), bd)], ref_chroma_origin=mr.co,
                         ref_chroma_stride=mr.cs)
    oext = oracle.refine_ext(1, cf, 0, NONE)
    cm, c0 = cost
    cmd = torch.from_numpy(cm.view(np.int16)).cuda()
    pos, par, mvc = jobs
    n = len(pos)
    thr = np.full(n, tgs.INT_MAX, np.int32)
    rc0 = np.full(n, 40, np.int32)
    out0, _ = oracle.me_search_ref(bd, mr.fenc_y, mr.origin, mr.stride, r.luma, r.luma[0], mr.origin, mr.stride,
                                   i_pixel, me_method, subme, 16, pos[:, 1:], par, mvc, cm, c0, ext=oext,
                                   fenc_c=mr.fenc_c, fc_origin=mr.co, fcs=mr.cs, ref_c=r.ref_c, rc_origin=mr.co,
                                   rcs=mr.cs, thresh=thr, ref_cost=rc0)
    rpar = np.stack([out0[:, 1], out0[:, 2], par[:, 0] + 4, par[:, 1] - 4, par[:, 6], par[:, 7], par[:, 8], par[:, 9]],
                    1).astype(np.int16)
    init = (out0[:, 0] + rc0).astype(np.int32)
    rc1 = np.full(n, 120, np.int32)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    ne = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    hip.me_refine_qpel_refdupe(fenc, mr.origin, mr.stride, luma, mr.origin, mr.stride, i_pixel, subme,
                               torch.from_numpy(pos).cuda(), torch.from_numpy(rpar).cuda(),
                               torch.from_numpy(init).cuda(), (cmd, c0), halfpel_thresh=thr_d,
                               ref_cost=torch.from_numpy(rc1).cuda(), out=out, nevals=ne, ext=ext)
    want, wne = oracle.me_refine_qpel_refdupe(bd, mr.fenc_y, mr.origin, mr.stride, r.luma, mr.origin, mr.stride,
                                              i_pixel, subme, pos[:, 1:], rpar, init, cm, c0, thresh=thr,
                                              ref_cost=rc1, out_fill=-7, ext=oext, fenc_c=mr.fenc_c, fc_origin=mr.co,
                                              fcs=mr.cs, ref_c=r.ref_c, rc_origin=mr.co, rcs=mr.cs)
    got, ne, gthr = out.cpu().numpy(), ne.cpu().numpy(), thr_d.cpu().numpy()
    bad = np.argwhere((got != want).any(1)).ravel()
    assert not len(bad), (*tag, bad[:4], got[bad[:4]], want[bad[:4]])
    bad = np.argwhere(ne != wne).ravel()
    assert not len(bad), (*tag, bad[:4], ne[bad[:4]], wne[bad[:4]])
    bad = np.argwhere(gthr != thr).ravel()
    assert not len(bad), (*tag, bad[:4], gthr[bad[:4]], thr[bad[:4]])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("me_method", [1, 2])
@pytest.mark.parametrize("i_pixel", [0, 3])
@pytest.mark.parametrize("kind", ["const", "nearflat"])
def test_thresh_chain_and_refdupe(hip, oracle, bd, me_method, i_pixel, kind):
    """the ref = 3 chain (one launch per reference, p_halfpel_thresh chained and updated in place)
    over three identical references -- every reference reaches the same costs, so the early exit
    (bcost * 7) >> 3 > thresh and the update bcost < thresh compare a cost with itself less the
    i_ref_cost differences -- and me_refine_qpel_refdupe after reference 0; subme 7 with chroma
    ME, lambda 40 / 1 / 0"""
    mr, jobs = dg.chain_inputs(kind, bd, i_pixel)
    for lam in dg.LAMBDAS:
        cost = rc.cost_mv(lam=lam)
        tgs._chain(hip, oracle, bd, W, H, i_pixel, me_method, 7, 0, mr=mr, jobs=jobs, cost=cost,
                   tag=(kind, lam, i_pixel))
        _refdupe(hip, oracle, bd, mr, jobs[0], i_pixel, me_method, 7, cost, (kind, lam, i_pixel, "refdupe"))


# ---------------------------------------------------------------- me_refine_subpel
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2, 3])
@pytest.mark.parametrize("i_pixel", [0, 3, 6])
@pytest.mark.parametrize("kind", dg.KINDS)
def test_refine_subpel(hip, oracle, bd, cf, i_pixel, kind):
    """96x64, two frame pairs per launch, subme 2 / 7 / 9 (chroma ME from 7: 4:2:0, 4:2:2, 4:4:4),
    unweighted and FADE_WEIGHTS, lambda 40 and 0; the start costs are refine_cases.jobs' (every
    ninth 0, which no candidate beats: at lambda 0 on const / periodic the candidates tie with
    it)"""
    cases = [dg.chroma_case(kind, bd, W, H, cf, seed=bd + 17 * k, p=dg.period(i_pixel)) for k in range(2)]
    for lam in (40, 0):
        for subme, weights in ((2, NONE), (7, NONE), (9, NONE), (7, rc.FADE_WEIGHTS), (9, rc.FADE_WEIGHTS)):
            tgr._run(hip, oracle, bd, cf, W, H, 2, i_pixel, subme, 0, int(subme >= 5), weights, seed=bd + i_pixel,
                     cases=cases, cost=rc.cost_mv(lam=lam),
                     tag=(kind, lam, i_pixel, subme, "fade" if weights[0] else ""))


# ---------------------------------------------------------------- me_refine_bidir
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3])
@pytest.mark.parametrize("satd", [1, 0])
@pytest.mark.parametrize("kind", dg.KINDS)
def test_bidir(hip, oracle, bd, i_pixel, satd, kind):
    """96x64, the five bipred weights (32: the rounding average; 24 / 44 / -8: the weighted one),
    lambda 40 and 0: on const at lambda 0 the 33 candidates of a pass all cost the same, on the
    full-scale kinds every average saturates one way"""
    mr = dg.multi_ref(kind, bd, W, H, 1, seed=40 + bd + i_pixel, p=dg.period(i_pixel))
    for lam in (40, 0):
        tgb._run(hip, oracle, bd, W, H, i_pixel, satd, seed=40 + bd + i_pixel, mr=mr, cost=rc.cost_mv(lam=lam),
                 tag=(kind, lam, i_pixel, "satd" if satd else "sad"))


# ---------------------------------------------------------------- me_search_ref_tesa
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3, 6])
@pytest.mark.parametrize("kind", ["const", "periodic", "extreme", "extreme_swap"])
def test_tesa_search(hip, oracle, bd, i_pixel, kind):
    """96x64, one frame pair, corner_rows' partitions (the Python checker's time), subme 1 and 7
    (chroma ME), lambda 40 and 0, me_range 16 -- 8 for the full-scale kinds at lambda 0, where
    every candidate of the window survives the ADS and ties through both prune loops (the
    checker's second loop is quadratic in the list); nearflat is test_gpu_tesa_search.py's
    test_tesa_search_edges"""
    cases = dg.search_cases(kind, bd, i_pixel, nframes=1)
    jobs = dg.search_jobs(bd, i_pixel, nframes=1)
    for lam in (40, 0):
        me_range = 8 if lam == 0 and kind.startswith("extreme") else 16
        for subme in (1, 7):
            tgt._run(hip, oracle, bd, W, H, 1, i_pixel, subme, me_range, 0, int(subme >= 5), 0, cases=cases,
                     jobs=jobs, cost=rc.cost_mv(lam=lam), subset=i_pixel <= 3, tag=(kind, lam, i_pixel, subme))


# ---------------------------------------------------------------- me_analyse_p16x16
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(112, 80), (96, 64)])
@pytest.mark.parametrize("me_method", [1, 2])
@pytest.mark.parametrize("kind", ["const", "nearflat", "periodic"])
def test_analyse_p16x16(hip, oracle, bd, size, me_method, kind):
    """the wavefront P16x16 analysis, two frames, subme 2 and 7 (chroma ME), lambda 40 / 1 / 0: the
    neighbours carry equal mvs (median ties; duplicate predictors dropped by the !v || v == pmv
    rule of x264_predictor_clip)"""
    w, h = size
    cases = [dg.chroma_case(kind, bd, w, h, 1, seed=bd + 11 * k, p=8) for k in range(2)]
    for lam in dg.LAMBDAS:
        for subme in (2, 7):
            tga._run(hip, oracle, bd, w, h, 2, me_method, subme, 16, int(subme >= 5), 0, cases=cases,
                     cost=rc.cost_mv(lam=lam), tag=(kind, lam, subme))


# ---------------------------------------------------------------- the ESA family (frame-level entries)
def _esa_par(mbw, mbh, nf, me_range, seed):
    """test_gpu_me.test_me_search_esa_fused's partitions: predictor centres, mvps, mv_limit_fpel-like
    limits with some windows clipped, start costs with every seventh unbeatable"""
    nmb = mbw * mbh
    rs = np.random.default_rng(seed)
    par = np.zeros((nf * nmb, 8), np.int16)
    par[:, 0] = rs.integers(-12, 13, nf * nmb)
    par[:, 1] = rs.integers(-12, 13, nf * nmb)
    par[:, 2] = rs.integers(-64, 65, nf * nmb)
    par[:, 3] = rs.integers(-64, 65, nf * nmb)
    mb = np.arange(nf * nmb) % nmb
    mbx, mby = mb % mbw, mb // mbw
    tight = rs.integers(0, me_range + 1, (nf * nmb, 4)) * (rs.random((nf * nmb, 4)) < 0.3)
    par[:, 4] = np.minimum(-16 * mbx - 24 + tight[:, 0], par[:, 0])
    par[:, 5] = np.minimum(-16 * mby - 24 + tight[:, 1], par[:, 1])
    par[:, 6] = np.maximum(16 * (mbw - 1 - mbx) + 20 - tight[:, 2], par[:, 0])
    par[:, 7] = np.maximum(16 * (mbh - 1 - mby) + 24 - tight[:, 3], par[:, 1])
    init = rs.integers(0, 20000, nf * nmb).astype(np.int32)
    init[::7] = 0
    init[3::7] = 1 << 28                                      # no predictor cost: the first candidate wins
    return par, init


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("rng", [8, 16])
@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_esa_fused_and_argmin(hip, oracle, bd, rng, kind):
    """me_search_esa (fused) and me_search_centred + me_esa_argmin against the oracle's centred
    table and argmin, 96x64, two frame pairs, range = me_range 8 and 16, the entry's cost table
    and a zero table: equal costs resolve to the first candidate in raster order (me.c:627-631's
    strict <)"""
    pl, stride, origin = dg.planes(kind, 3, W, H, bd, seed=rng, p=8, refs=(0, 2))
    dev = _t(pl, bd)
    fs = pl[0].size
    mbw, mbh, nf = W // 16, H // 16, 2
    nmb = mbw * mbh
    par, init = _esa_par(mbw, mbh, nf, rng, seed=7 * rng + bd)
    par_d, init_d = torch.from_numpy(par).cuda(), torch.from_numpy(init).cuda()
    cen = torch.from_numpy(np.ascontiguousarray(par[:, :2])).cuda()
    table, org = hip.me_search_centred(dev[1:], origin, stride, dev[:-1], origin, stride, mbw, mbh, nf, rng, cen,
                                       fenc_frame_stride=fs, ref_frame_stride=fs)
    for lam in (40, 0):
        cm, c0 = ec.cost_mv(lam=lam, span=8192)
        cmd = (torch.from_numpy(cm.view(np.int16)).cuda(), c0)
        fused = hip.me_search_esa(dev[1:], origin, stride, dev[:-1], origin, stride, mbw, mbh, nf, rng, rng, par_d,
                                  init_d, cmd, fenc_frame_stride=fs, ref_frame_stride=fs).cpu().numpy()
        split = hip.me_esa_argmin(table, rng, rng, par_d, init_d, cmd, origin=org).cpu().numpy()
        for f in range(nf):
            sl = slice(f * nmb, (f + 1) * nmb)
            tab, worg = oracle.me_search_centred(bd, pl[f + 1].ravel(), origin, stride, pl[f].ravel(), origin, stride,
                                                 mbw, mbh, rng, par[sl, :2])
            want = oracle.me_esa_argmin(bd, tab.reshape(nmb, 2 * rng + 1, -1), rng, rng, par[sl], init[sl], cm, c0,
                                        origin=worg)
            for name, got in (("fused", fused[sl]), ("argmin", split[sl])):
                bad = np.argwhere((got != want).any(1)).ravel()
                assert not len(bad), (kind, lam, name, f, bad[:4], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_esa8(hip, oracle, bd, R, kind):
    """me_search_esa8, 96x64, two frame pairs, range = me_range 8 and 16, half the windows moved off
    the template (the direct pass) and all clipped by mv_limit_fpel, the entry's cost table with
    random start costs and a zero table with high ones"""
    frames = dg.planes(kind, 3, W, H, bd, seed=R, p=4, refs=(0, 2))
    for lam, init in ((40, "random"), (0, "high")):
        tge._run(hip, oracle, bd, W, H, 2, R, R, seed=R + bd, frames=frames, cost=ec.cost_mv(lam=lam),
                 tag=(kind, lam), spread=5, frac=0.5, centre_amp=6, limit=4, init=init)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("me_range,satd", [(16, True), (8, False)])
@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_me_tesa(hip, oracle, bd, me_range, satd, kind):
    """the 16x16 me_tesa kernel, 96x64, two frame pairs, me_range 16 with SATD and 8 with SAD, the
    entry's cost table and a zero table"""
    pl, stride, org = dg.planes(kind, 3, W, H, bd, seed=me_range, p=8, refs=(0, 2))
    dev = _t(pl, bd)
    mbw, mbh, nf = W // 16, H // 16, 2
    integ = hip.frame_integral(dev[:-1], org, stride, H)
    par, init = tc.params(mbw, mbh, me_range, seed=bd * 13 + me_range, nframes=nf)
    n1 = mbw * mbh
    for lam in (40, 0):
        cmv, c0 = tc.cost_mv(lam=lam)
        cmd = (torch.from_numpy(cmv.view(np.int16)).cuda(), c0)
        got = hip.me_tesa(dev[1:], org, stride, dev[:-1], org, stride, integ, mbw, mbh, nf, me_range,
                          torch.from_numpy(par).cuda(), torch.from_numpy(init).cuda(), cmd, satd=satd).cpu().numpy()
        for f in range(nf):
            f1, f0 = pl[f + 1].ravel(), pl[f].ravel()
            oi = oracle.frame_integral(bd, f0, org, stride, H, tc.PAD, False).ravel()
            want = oracle.me_tesa(bd, f1, org, stride, f0, org, oi, tc.PAD * stride + tc.PAD, stride, mbw, mbh,
                                  me_range, satd, par[f * n1:(f + 1) * n1], init[f * n1:(f + 1) * n1], cmv, c0)
            g = got[f * n1:(f + 1) * n1]
            bad = np.argwhere((g != want).any(1)).ravel()
            assert not len(bad), (kind, lam, f, bad[:4], g[bad[:4]], want[bad[:4]])


# ---------------------------------------------------------------- the lookahead's searches
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(176, 144), (64, 48)])
@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_lowres_inter(hip, oracle, bd, size, kind):
    """lowres_inter_cost on full-resolution frames of each kind (two pairs: on extreme the second
    is the swap), DIA and HEX, subme 2 and 4, SATD on and off: on the full-scale pairs the cost
    words meet LOWRES_COST_MASK's clamp"""
    w, h = size
    frames = dg.planes(kind, 3, w, h, bd, seed=5, p=8, refs=(0, 2))
    for me_method, subme, satd in ((0, 2, False), (1, 4, True), (0, 4, True), (1, 2, False)):
        tgl._case(hip, oracle, bd, w, h, 2, me_method, subme, satd, frames=frames,
                  tag=(kind, me_method, subme, satd))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(176, 144), (64, 48)])
@pytest.mark.parametrize("kind", PLANE_KINDS)
def test_lowres_bidir(hip, oracle, bd, size, kind):
    """lowres_bidir_cost on two B triplets of each kind (extreme: the B frame max between zero
    references, then the swap), both lists searched, p1's mvs as the bidir predictor, weights 32
    and 43"""
    w, h = size
    frames = dg.planes(kind, 6, w, h, bd, seed=5, p=8, refs=(0, 2, 4))
    for me_method, subme, satd, weight in ((1, 4, True, 32), (0, 2, False, 43), (0, 4, True, 43), (1, 2, False, 32)):
        tgl._bidir_case(hip, oracle, bd, w, h, 2, 3, me_method, subme, satd, 128 if weight == 32 else 85, weight,
                        frames=frames, tag=(kind, me_method, subme, satd, weight))
