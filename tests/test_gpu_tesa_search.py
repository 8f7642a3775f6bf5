"""GPU parity: x264_me_search_ref with X264_ME_TESA for every partition size
(x264hip_*_me_search_ref_tesa, reference encoder/me.c:214-318, 618-749, 774-797) against the
literal Python restatement of tests/tesa_search_cases.py (pinned to the oracle by
tests/test_cpu_tesa_search.py) followed by the oracle's refine_subpel with fpelcmp = SATD: out,
the call counts (nevals) and the scan's counts (scan) bit-exact, for every size, subme 1 / 2 / 4
/ 7 / 9, weighted references (the integral stays the unweighted plane's), chroma ME, every
me_range class, degenerate limits, skipped rows and empty lists, the multi-reference threshold
chain, and the existing 16x16 me_tesa kernel on the same inputs."""
import numpy as np
import pytest
import torch

import refine_cases as rc
import search_cases as sc
import tesa_search_cases as ts
from test_cpu_refine_chroma import _weigh

pytestmark = pytest.mark.gpu

INT_MAX = (1 << 31) - 1


def _t(a, bd):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if bd == 10 else a).cuda()


def _run(hip, oracle, bd, W, H, nframes, i_pixel, subme, me_range, fade, chroma, seed, cases=None, jobs=None,
         cost=None, subset=False, tag=()):
    """test_gpu_search._run for the TESA entry: nframes ChromaCase pairs in one launch"""
    cf = 1
    weights = rc.FADE_WEIGHTS if fade else (None, None, None)
    cases = cases or [rc.ChromaCase(bd, W, H, cf, seed=seed + 11 * k, fade=fade) for k in range(nframes)]
    c0_ = cases[0]
    rows = c0_.ref.y.shape[0]
    crows = c0_.ref.nv.shape[0]
    fws = [c.luma[0] if not fade else _weigh(c.luma[0].astype(np.int64), weights[0], bd).astype(c.luma[0].dtype)
           for c in cases]
    fenc = _t(np.stack([c.fenc_y.reshape(rows, -1) for c in cases]), bd)
    luma = [_t(np.stack([c.luma[k].reshape(rows, -1) for c in cases]), bd) for k in range(4)]
    fw = _t(np.stack([w.reshape(rows, -1) for w in fws]), bd)
    fenc_c = [_t(np.stack([c.fenc_c[0].reshape(crows, -1) for c in cases]), bd)]
    ref_c = [_t(np.stack([c.ref_c[0].reshape(crows, -1) for c in cases]), bd)]
    pos, par, mvc = jobs if jobs is not None else sc.jobs(W // 16, H // 16, nframes, i_pixel, seed=seed + subme)
    if subset:
        pos, par, mvc = ts.corner_rows(pos, par, mvc, W // 16, H // 16)
    cm, c0 = cost or rc.cost_mv()
    cmd = torch.from_numpy(cm.view(np.int16)).cuda()
    ext = hip.refine_ext(chroma, cf, 0, weights, fenc_chroma=fenc_c, fenc_chroma_origin=c0_.co,
                         fenc_chroma_stride=c0_.cs, ref_chroma=ref_c, ref_chroma_origin=c0_.co,
                         ref_chroma_stride=c0_.cs)
    # the integral of the unweighted reference (analyse.c:1243), both planes
    integ = hip.frame_integral(luma[0], c0_.origin, c0_.stride, H, sub8x8=True)
    ne = torch.full((len(pos), 2), -1, dtype=torch.int32, device="cuda")
    scan = torch.full((len(pos), 2), -1, dtype=torch.int32, device="cuda")
    got = hip.me_search_ref_tesa(fenc, c0_.origin, c0_.stride, fw, luma, c0_.origin, c0_.stride, integ, i_pixel, subme,
                                 me_range, torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda(),
                                 torch.from_numpy(mvc).cuda(), (cmd, c0), nevals=ne, scan=scan, ext=ext).cpu().numpy()
    ne, scan = ne.cpu().numpy(), scan.cpu().numpy()
    for f, c in enumerate(cases):
        sel = pos[:, 0] == f
        oi = ts.integral_planes(oracle, bd, c.luma[0], c.origin, c.stride, H)
        want, wne, wscan = ts.expected(oracle, bd, c, fws[f].ravel(), i_pixel, subme, me_range, pos[sel, 1:], par[sel],
                                       mvc[sel], cm, c0, oi, weights, chroma, cf)
        for name, g, w in (("scan", scan[sel], wscan), ("nevals", ne[sel], wne), ("out", got[sel], want)):
            bad = np.argwhere((g != w).any(1)).ravel()
            assert not len(bad), (*tag, name, f, bad[:4], g[bad[:4]], w[bad[:4]])
    return got, pos, par, mvc, scan


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("subme,fade,chroma", [(1, 0, 0), (2, 0, 0), (4, 1, 0), (7, 0, 1), (9, 1, 1)])
def test_tesa_search_small(hip, oracle, bd, i_pixel, subme, fade, chroma):
    """96x64: two frame pairs per launch for the sizes down to 8x8, one for the sub-8x8 sizes (the
    checker's time)"""
    _run(hip, oracle, bd, 96, 64, 2 if i_pixel <= 3 else 1, i_pixel, subme, 24 if subme == 9 else 16, fade, chroma,
         seed=bd + 5 * i_pixel)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3, 6])
@pytest.mark.parametrize("me_range", [4, 8, 32])
def test_tesa_search_ranges(hip, oracle, bd, i_pixel, me_range):
    """me_range 4 and 8 (limit 2 and 4: both prune loops run hard) and 32 (the window's 64 columns,
    sad_thresh 12); the 4x4 run at me_range 32 on one MB row and the corner MBs"""
    got, pos, par, mvc, scan = _run(hip, oracle, bd, 96, 64, 1, i_pixel, 2, me_range, 0, 0, seed=bd + me_range,
                                    subset=i_pixel == 6)
    assert (scan[:, 1] > me_range).any()                     # lists the prunes had to cut


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3, 5])
def test_tesa_search_edges(hip, oracle, bd, i_pixel):
    """tesa_search_cases.edge_inputs: degenerate limits, near-flat content under a high-lambda, a
    lambda-1 and a zero mv cost, a 336x48 frame (that these reach the row skip, windows of width 0
    and empty lists of scanned windows is test_cpu_tesa_search.py's
    test_edge_inputs_reach_their_paths)"""
    for cases, jobs, cost, subme, chroma, W, H in ts.edge_inputs(bd, i_pixel):
        _run(hip, oracle, bd, W, H, 1, i_pixel, subme, 16, 0, chroma, seed=bd, cases=cases, jobs=jobs, cost=cost)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("me_range", [16, 24])
def test_tesa_search_matches_me_tesa(hip, oracle, bd, me_range):
    """i_pixel 0, subme 1, the whole MB raster: the integer decision equals the existing 16x16
    kernel's (x264hip_*_me_tesa, fpelcmp = SAD) fed with the Python predictor stage's centre and
    cost"""
    W, H = 96, 64
    c = rc.ChromaCase(bd, W, H, 1, seed=21 + bd)
    rows = c.ref.y.shape[0]
    pos, par, mvc = sc.jobs(W // 16, H // 16, 1, 0, seed=bd + me_range)
    cm, c0 = rc.cost_mv()
    cmd = torch.from_numpy(cm.view(np.int16)).cuda()
    fenc = _t(c.fenc_y.reshape(1, rows, -1), bd)
    luma = [_t(p.reshape(1, rows, -1), bd) for p in c.luma]
    integ = hip.frame_integral(luma[0], c.origin, c.stride, H, sub8x8=True)
    got = hip.me_search_ref_tesa(fenc, c.origin, c.stride, luma[0], luma, c.origin, c.stride, integ, 0, 1, me_range,
                                 torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda(),
                                 torch.from_numpy(mvc).cuda(), (cmd, c0)).cpu().numpy()
    buf, i8, _ = ts.integral_planes(oracle, bd, c.luma[0], c.origin, c.stride, H)
    tpar = np.zeros((len(pos), 8), np.int16)
    init = np.zeros(len(pos), np.int32)
    pmv = np.zeros(len(pos), np.int64)
    for i in range(len(pos)):
        st = {}
        ts.search_ref_tesa_py(c.fenc_y, c.luma, c.luma[0], c.origin, c.stride, int(pos[i, 1]), int(pos[i, 2]), 0,
                              par[i], mvc[i], cm, c0, 1, me_range, buf, i8, H, bd=bd, stage=st)
        tpar[i] = (st["bmx"], st["bmy"], par[i, 0], par[i, 1], par[i, 2], par[i, 3], par[i, 4], par[i, 5])
        init[i], pmv[i] = st["bcost"], st["pmv"]
    one = hip.frame_integral(luma[0], c.origin, c.stride, H)
    old = hip.me_tesa(fenc, c.origin, c.stride, luma[0], c.origin, c.stride, one, W // 16, H // 16, 1, me_range,
                      torch.from_numpy(tpar).cuda(), torch.from_numpy(init).cuda(), (cmd, c0), satd=False).cpu().numpy()
    assert np.array_equal(got[:, 1:3], 4 * old[:, 1:3])
    same = ((old[:, 1] & 0xFFFF) | ((old[:, 2] & 0xFFFF) << 16)) == pmv        # me.c:782: the real cost
    assert np.array_equal(got[:, 0], old[:, 0] + np.where(same, got[:, 3], 0))
    assert (old[:, 1:3] != tpar[:, :2]).any()                 # the window moved some winners


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3])
def test_tesa_search_thresh_chain(hip, oracle, bd, i_pixel):
    """test_gpu_search._chain for TESA: three references of one frame, one launch each, the
    partition's p_halfpel_thresh chained through them and updated in place (me.c:931-944,
    analyse.c:1260-1314), subme 7 with chroma ME; expected = the restatement's integer stage then
    refine_fpel_satd_py with the threshold"""
    W, H, cf, subme, me_range = 96, 64, 1, 7, 16
    from test_cpu_search import _as_case
    mr = sc.MultiRef(bd, W, H, cf, seed=5 + bd)
    rows = mr.fenc_y.size // mr.stride
    crows = mr.fenc_c[0].size // mr.cs
    fenc = _t(mr.fenc_y.reshape(1, rows, -1), bd)
    fenc_c = [_t(mr.fenc_c[0].reshape(1, crows, -1), bd)]
    cm, c0 = rc.cost_mv()
    cmd = torch.from_numpy(cm.view(np.int16)).cuda()
    n = len(mr.jobs(0, i_pixel, 0)[0])
    thr = np.full(n, INT_MAX, np.int32)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    early = 0
    for k in range(3):
        r = mr.refs[k]
        luma = [_t(p.reshape(1, rows, -1), bd) for p in r.luma]
        ref_c = [_t(r.ref_c[0].reshape(1, crows, -1), bd)]
        ext = hip.refine_ext(1, cf, 0, (None, None, None), fenc_chroma=fenc_c, fenc_chroma_origin=mr.co,
                             fenc_chroma_stride=mr.cs, ref_chroma=ref_c, ref_chroma_origin=mr.co,
                             ref_chroma_stride=mr.cs)
        pos, par, mvc = mr.jobs(k, i_pixel, seed=5 + bd + 17 * k)
        rcost = np.full(n, 40 if k == 0 else 120, np.int32)
        out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        ne = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
        integ = hip.frame_integral(luma[0], mr.origin, mr.stride, H, sub8x8=True)
        hip.me_search_ref_tesa(fenc, mr.origin, mr.stride, luma[0], luma, mr.origin, mr.stride, integ, i_pixel, subme,
                               me_range, torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda(),
                               torch.from_numpy(mvc).cuda(), (cmd, c0), out=out, nevals=ne, ext=ext,
                               halfpel_thresh=thr_d, ref_cost=torch.from_numpy(rcost).cuda())
        got, ne = out.cpu().numpy(), ne.cpu().numpy()
        buf, i8, _ = ts.integral_planes(oracle, bd, r.luma[0], mr.origin, mr.stride, H)
        cc = _as_case(mr, k)
        for i in range(n):
            x, y = int(pos[i, 1]), int(pos[i, 2])
            w, nf, _ = ts.search_ref_tesa_py(mr.fenc_y, r.luma, r.luma[0], mr.origin, mr.stride, x, y, i_pixel, par[i],
                                             mvc[i], cm, c0, subme, me_range, buf, i8, H, bd=bd)
            rpar = (w[1], w[2], par[i, 0], par[i, 1], par[i, 6], par[i, 7], par[i, 8], par[i, 9])
            t = [int(thr[i])]
            w, rn = ts.refine_fpel_satd_py(cc, x, y, i_pixel, rpar, w[0], cm, c0, subme, 0, 1, (None, None, None),
                                           thresh=t, ref_cost=int(rcost[i]))
            thr[i] = t[0]
            w = tuple(-7 if v is None else v for v in w)
            early += w[3] == -7
            assert tuple(got[i]) == w, (k, i, got[i], w)
            assert tuple(ne[i]) == (nf[0] | (nf[1] << 16), rn), (k, i, ne[i], nf, hex(rn))
        assert np.array_equal(thr_d.cpu().numpy(), thr), k
    assert early > 0


def test_tesa_search_args(hip):
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = torch.zeros((2, 160, 256), dtype=torch.uint8, device="cuda")
    one = torch.zeros((2, 160, 256), dtype=torch.int16, device="cuda")          # frame_integral(sub8x8=False)'s shape
    two = torch.zeros((2, 320, 256), dtype=torch.int16, device="cuda")
    pos = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    par = torch.zeros((1, 12), dtype=torch.int16, device="cuda")
    mvc = torch.zeros((1, 14, 2), dtype=torch.int16, device="cuda")
    good = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    odd = torch.zeros(9, dtype=torch.int32, device="cuda")[1:5].view(1, 4)      # 4 bytes off the 16-byte alignment

    def call(integ, i_pixel, subme, rng, out):
        hip.me_search_ref_tesa(p, 32 * 256 + 32, 256, p, [p, p, p, p], 32 * 256 + 32, 256, integ, i_pixel, subme, rng,
                               pos, par, mvc, (t.view(torch.int16), 0), out=out)

    for integ, i_pixel, subme, rng, out in ((two, 7, 7, 16, good), (two, 0, 0, 16, good), (two, 0, 7, 3, good),
                                            (two, 0, 7, 33, good), (two, 0, 7, 16, odd), (one, 4, 7, 16, good)):
        with pytest.raises(RuntimeError):
            call(integ, i_pixel, subme, rng, out)
    call(one, 3, 1, 16, good)                                 # a single-plane integral serves i_pixel <= 3
    call(two, 4, 1, 4, good)
    torch.cuda.synchronize()
