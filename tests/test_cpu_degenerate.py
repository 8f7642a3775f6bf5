"""CPU: pins the checker and the inputs of tests/test_gpu_degenerate.py.  On the degenerate content
of tests/degenerate_cases.py (constant, near-flat, periodic and full-scale planes under mv-cost
lambdas 40 / 1 / 0) the oracle agrees with the literal Python restatements, call counts included
-- me_search_ref (DIA / HEX / UMH / ESA, subme 1 / 2 / 7, chroma ME at 7, the usual and the
collapsed-limit job lists), me_refine_subpel, the multi-reference threshold chain and
me_refine_qpel_refdupe on identical references, me_refine_bidir (SATD and SAD, weights 32 and
!= 32), the TESA restatement's ESA form, me_search_esa8 -- so either can check the HIP kernels
there; the inputs reach what they exist for (tie rates, equal SADs a period apart, the largest
cost), computed from numpy_ref and the job lists alone; and every block a schedule can reach
from the job lists' limits lies inside the padded planes.  No GPU."""
import numpy as np
import pytest

import bidir_cases as bc
import degenerate_cases as dg
import esa8_cases as ec
import numpy_ref as nr
import refine_cases as rc
import search_cases as sc
import tesa_search_cases as ts
from test_cpu_refine_chroma import refine_chroma_py
from test_cpu_search import INT_MAX, _as_case, _chain_py

W, H, CF = 48, 32, 1
MBW, MBH = W // 16, H // 16


def _jobs(i_pixel, seed, collapsed=False):
    """the frame's partitions (the sub-8x8 sizes: every fourth, the checker's time)"""
    j = ts.degenerate_jobs(MBW, MBH, i_pixel, seed) if collapsed else sc.jobs(MBW, MBH, 1, i_pixel, seed=seed)
    return tuple(a[::4] for a in j) if i_pixel >= 4 else j


def _search_vs_python(oracle, cc, bd, i_pixel, me_method, subme, me_range, jobs, cost, tag):
    pos, par, mvc = jobs
    cm, c0 = cost
    chroma = int(subme >= 5)
    none = (None, None, None)
    got, ne = oracle.me_search_ref(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.luma[0], cc.origin, cc.stride,
                                   i_pixel, me_method, subme, me_range, pos[:, 1:], par, mvc, cm, c0,
                                   ext=oracle.refine_ext(chroma, CF, 0, none), fenc_c=cc.fenc_c, fc_origin=cc.co,
                                   fcs=cc.cs, ref_c=cc.ref_c, rc_origin=cc.co, rcs=cc.cs)
    for i in range(len(pos)):
        x, y = int(pos[i, 1]), int(pos[i, 2])
        want, wn = sc.search_ref_py(cc.fenc_y, cc.luma, cc.luma[0], cc.origin, cc.stride, x, y, i_pixel, par[i],
                                    mvc[i], cm, c0, me_method, subme, me_range, bd=bd)
        assert ne[i, 0] == wn[0] | (wn[1] << 16), (tag, i, hex(ne[i, 0]), wn)
        if subme >= 2:
            rpar = (want[1], want[2], par[i, 0], par[i, 1], par[i, 6], par[i, 7], par[i, 8], par[i, 9])
            want, wrn = refine_chroma_py(cc, x, y, i_pixel, rpar, want[0], cm, c0, subme, 0, chroma, none)
            assert ne[i, 1] == wrn, (tag, i, hex(ne[i, 1]), hex(wrn))
        assert tuple(got[i]) == tuple(want), (tag, i, got[i], want)
    return got


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", dg.KINDS)
@pytest.mark.parametrize("me_method", [0, 1, 2, 3])
def test_search_oracle_vs_python(oracle, bd, kind, me_method):
    """me_search_ref on every kind x lambda 40 / 1 / 0, 16x16 / 8x8 / 4x4, subme 1 / 2 / 7 (chroma
    ME at 7); ESA at me_range 8 (the Python loops' time), the others at 16.  On const and nearflat
    also the collapsed-limit jobs (tesa_search_cases.degenerate_jobs)"""
    me_range = 8 if me_method == 3 else 16
    for i_pixel in (0, 3, 6):
        cc = dg.chroma_case(kind, bd, W, H, CF, seed=bd + i_pixel, p=dg.period(i_pixel))
        for lam in dg.LAMBDAS:
            for subme in (1, 2, 7):
                _search_vs_python(oracle, cc, bd, i_pixel, me_method, subme, me_range,
                                  _jobs(i_pixel, seed=subme + me_method), rc.cost_mv(lam=lam),
                                  (kind, lam, i_pixel, subme))
            if kind in ("const", "nearflat"):
                for subme in (1, 7):
                    _search_vs_python(oracle, cc, bd, i_pixel, me_method, subme, me_range,
                                      _jobs(i_pixel, seed=2 + me_method, collapsed=True), rc.cost_mv(lam=lam),
                                      (kind, lam, i_pixel, subme, "collapsed"))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", dg.KINDS)
@pytest.mark.parametrize("cf", [1, 3])
def test_refine_subpel_oracle_vs_python(oracle, bd, kind, cf):
    """me_refine_subpel with chroma ME, subme 2 / 7 / 9, 16x16 / 8x8 / 4x4, lambda 40 and 0,
    unweighted and FADE_WEIGHTS (start costs as refine_cases.jobs gives them: every ninth 0, which
    no candidate beats -- at lambda 0 on const / periodic they tie with it)"""
    for i_pixel in (0, 3, 6):
        cc = dg.chroma_case(kind, bd, W, H, cf, seed=bd + cf, p=dg.period(i_pixel))
        pos, par, cost = rc.jobs(MBW, MBH, 1, i_pixel, seed=bd + i_pixel, cost_scale=1 << (bd - 8))
        if i_pixel >= 4:
            pos, par, cost = pos[::4], par[::4], cost[::4]
        for lam in (40, 0):
            cm, c0 = rc.cost_mv(lam=lam)
            for subme, weights in ((2, (None, None, None)), (7, (None, None, None)), (9, rc.FADE_WEIGHTS)):
                chroma = int(subme >= 5)
                got, ne = oracle.me_refine_subpel(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.origin, cc.stride,
                                                  i_pixel, subme, pos[:, 1:], par, cost, cm, c0, 0, False, counts=True,
                                                  ext=oracle.refine_ext(chroma, cf, 0, weights), fenc_c=cc.fenc_c,
                                                  fc_origin=cc.co, fcs=cc.cs, ref_c=cc.ref_c, rc_origin=cc.co,
                                                  rcs=cc.cs)
                for i in range(len(pos)):
                    want, wn = refine_chroma_py(cc, int(pos[i, 1]), int(pos[i, 2]), i_pixel, par[i], cost[i], cm, c0,
                                                subme, 0, chroma, weights)
                    assert tuple(got[i]) == want and ne[i] == wn, (kind, lam, i_pixel, subme, i, got[i], want,
                                                                   hex(ne[i]), hex(wn))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["const", "nearflat"])
@pytest.mark.parametrize("me_method", [1, 2])
def test_thresh_chain_and_refdupe_oracle_vs_python(oracle, bd, kind, me_method):
    """the ref = 3 chain (analyse.c:1260-1314) over three identical references -- every reference
    reaches the same cost, so (bcost * 7) >> 3 > thresh and bcost < thresh compare a cost with
    itself less the i_ref_cost differences -- then me_refine_qpel_refdupe on reference 0's result;
    16x16 and 8x8, subme 7 with chroma ME, lambda 40 and 0"""
    subme, me_range = 7, 16
    none = (None, None, None)
    ext = oracle.refine_ext(1, CF, 0, none)
    for i_pixel in (0, 3):
        mr = dg.multi_ref(kind, bd, W, H, CF, seed=3 + bd + i_pixel)
        for lam in (40, 0):
            cm, c0 = rc.cost_mv(lam=lam)
            n = len(mr.jobs(0, i_pixel, 0)[0])
            thr = np.full(n, INT_MAX, np.int32)
            thr_py = thr.copy()
            for k in range(3):
                pos, par, mvc = mr.jobs(k, i_pixel, seed=17 * k + me_method)
                rcost = np.full(n, 40 if k == 0 else 120 if k == 1 else 0, np.int32)
                r = mr.refs[k]
                got, ne = oracle.me_search_ref(bd, mr.fenc_y, mr.origin, mr.stride, r.luma, r.luma[0], mr.origin,
                                               mr.stride, i_pixel, me_method, subme, me_range, pos[:, 1:], par, mvc,
                                               cm, c0, ext=ext, fenc_c=mr.fenc_c, fc_origin=mr.co, fcs=mr.cs,
                                               ref_c=r.ref_c, rc_origin=mr.co, rcs=mr.cs, thresh=thr, ref_cost=rcost,
                                               out_fill=-7)
                want = _chain_py(mr, k, i_pixel, pos, par, mvc, cm, c0, me_method, subme, me_range, thr_py, rcost, 1)
                for i, w in enumerate(want):
                    assert tuple(got[i, :3]) == tuple(w[:3]), (kind, lam, k, i, got[i], w)
                    assert got[i, 3] == (-7 if w[3] is None else w[3]), (kind, lam, k, i, got[i], w)
                assert np.array_equal(thr, thr_py), (kind, lam, k)
                if k == 0:
                    out0, par0, pos0 = got.copy(), par, pos
            rpar = np.stack([out0[:, 1], out0[:, 2], par0[:, 0] + 4, par0[:, 1] - 4, par0[:, 6], par0[:, 7],
                             par0[:, 8], par0[:, 9]], 1).astype(np.int16)
            init = (out0[:, 0] + 40).astype(np.int32)
            rc1 = np.full(n, 120, np.int32)
            r = mr.refs[0]
            got, ne = oracle.me_refine_qpel_refdupe(bd, mr.fenc_y, mr.origin, mr.stride, r.luma, mr.origin, mr.stride,
                                                    i_pixel, subme, pos0[:, 1:], rpar, init, cm, c0, thresh=thr,
                                                    ref_cost=rc1, out_fill=-7, ext=ext, fenc_c=mr.fenc_c,
                                                    fc_origin=mr.co, fcs=mr.cs, ref_c=r.ref_c, rc_origin=mr.co,
                                                    rcs=mr.cs)
            for i in range(n):
                t = [int(thr_py[i])]
                w, wn = refine_chroma_py(_as_case(mr, 0), int(pos0[i, 1]), int(pos0[i, 2]), i_pixel, rpar[i], init[i],
                                         cm, c0, subme, 0, 1, none, refdupe=True, thresh=t, ref_cost=120)
                thr_py[i] = t[0]
                assert tuple(got[i, :3]) == tuple(w[:3]) and got[i, 3] == (-7 if w[3] is None else w[3]), \
                    (kind, lam, i, got[i], w)
                assert ne[i] == wn, (kind, lam, i, hex(ne[i]), hex(wn))
            assert np.array_equal(thr, thr_py), (kind, lam)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", dg.KINDS)
@pytest.mark.parametrize("satd", [1, 0])
def test_bidir_oracle_vs_python(oracle, bd, kind, satd):
    """me_refine_bidir, 16x16 and 8x8, the five weights (32 and != 32), lambda 40 and 0: on const
    at lambda 0 all 33 candidates of a pass cost the same"""
    for i_pixel in (0, 3):
        mr = dg.multi_ref(kind, bd, W, H, CF, seed=21 + bd + i_pixel, p=dg.period(i_pixel))
        pos, par, wt = bc.jobs(mr, i_pixel, seed=5 + i_pixel + satd)
        for lam in (40, 0):
            cm, c0 = rc.cost_mv(lam=lam)
            out, cost, ne = oracle.me_refine_bidir(bd, mr.fenc_y, mr.origin, mr.stride, mr.refs[0].luma,
                                                   mr.refs[1].luma, mr.origin, mr.stride, i_pixel, satd, pos[:, 1:],
                                                   par, wt, cm, c0)
            for i in range(len(pos)):
                want, wc, wn = bc.refine_bidir_py(mr.fenc_y, mr.refs[0].luma, mr.refs[1].luma, mr.origin, mr.stride,
                                                  int(pos[i, 1]), int(pos[i, 2]), i_pixel, satd, par[i], int(wt[i]),
                                                  cm, c0, bd)
                assert tuple(out[i]) == want and cost[i] == wc and ne[i] == wn, (kind, lam, i_pixel, i, out[i], want,
                                                                                 cost[i], wc, ne[i], wn)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", dg.KINDS)
def test_tesa_restatement_esa_form(oracle, bd, kind):
    """search_ref_tesa_py (the checker of me_search_ref_tesa) with me_method 3 and fpelcmp = SAD is
    oracle.me_search_ref's ESA on every kind, lambda 40 and 0, 16x16 / 8x8 / 4x8, me_range 8"""
    for i_pixel in (0, 3, 5):
        cc = dg.chroma_case(kind, bd, W, H, CF, seed=bd + i_pixel, p=dg.period(i_pixel))
        pos, par, mvc = _jobs(i_pixel, seed=1 + i_pixel)
        buf, i8, i4 = ts.integral_planes(oracle, bd, cc.luma[0], cc.origin, cc.stride, H)
        for lam in (40, 0):
            cm, c0 = rc.cost_mv(lam=lam)
            want, wne = oracle.me_search_ref(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.luma[0], cc.origin,
                                             cc.stride, i_pixel, 3, 1, 8, pos[:, 1:], par, mvc, cm, c0,
                                             ext=oracle.refine_ext(0, 1, 0, (None, None, None)))
            for i in range(len(pos)):
                r, nf, _ = ts.search_ref_tesa_py(cc.fenc_y, cc.luma, cc.luma[0], cc.origin, cc.stride, int(pos[i, 1]),
                                                 int(pos[i, 2]), i_pixel, par[i], mvc[i], cm, c0, 1, 8, buf,
                                                 i8 if i_pixel <= 3 else i4, H, me_method=3, fpel_satd=False, bd=bd)
                assert wne[i, 0] == nf[0] | (nf[1] << 16), (kind, lam, i_pixel, i, hex(wne[i, 0]), nf)
                assert tuple(want[i]) == tuple(r), (kind, lam, i_pixel, i, want[i], r)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", dg.KINDS)
def test_esa8_oracle_vs_python(oracle, bd, kind):
    """me_search_esa8, me_range 4, windows moved off the MB centre and clipped, the entry's cost
    table and a zero table, start costs random and high"""
    me_range = 4
    pl, stride, origin = dg.planes(kind, 2, W, H, bd, seed=7)
    f, r = pl[1].ravel(), pl[0].ravel()
    for lam, init in ((40, "random"), (0, "high")):
        cen, par, ic = ec.jobs(MBW, MBH, me_range, seed=bd, spread=3, frac=0.6, centre_amp=4, limit=20, init=init)
        cm, c0 = ec.cost_mv(lam=lam)
        got = oracle.me_search_esa8(bd, f, origin, stride, r, origin, stride, MBW, MBH, me_range, par, ic, cm, c0)
        want = ec.esa8_py(f, origin, stride, r, origin, stride, MBW, me_range, par, ic, cm, c0, range(MBW * MBH))
        for i, v in want.items():
            assert tuple(got[i]) == v, (kind, lam, i, tuple(got[i]), v)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["const", "nearflat", "periodic"])
@pytest.mark.parametrize("me_method", [1, 2])
def test_analyse_raster_oracle_vs_python(oracle, bd, kind, me_method):
    """mvpred_cases.analyse_p16x16 (the checker of me_analyse_p16x16) with the oracle's search per
    MB and with the Python restatement's gives the same field, subme 2 and 7, lambda 40 / 1 / 0;
    and its MBs do meet what the content is for: neighbours with equal mvs, so candidates that
    x264_predictor_clip drops as zero or equal to pmv"""
    import mvpred_cases as mp
    none = (None, None, None)
    cc = dg.chroma_case(kind, bd, W, H, CF, seed=bd, p=8)
    dropped = 0
    for lam in dg.LAMBDAS:
        cm, c0 = rc.cost_mv(lam=lam)
        for subme in (2, 7):
            chroma = int(subme >= 5)
            ext = oracle.refine_ext(chroma, CF, 0, none)
            seen = []

            def by_oracle(x, y, par, mvc):
                seen.append((tuple(par[:2]), [tuple(v) for v in mvc[:par[10]]]))
                o, n = oracle.me_search_ref(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.luma[0], cc.origin,
                                            cc.stride, 0, me_method, subme, 16, np.array([[16 * x, 16 * y]]), par[None],
                                            mvc[None], cm, c0, ext=ext, fenc_c=cc.fenc_c, fc_origin=cc.co, fcs=cc.cs,
                                            ref_c=cc.ref_c, rc_origin=cc.co, rcs=cc.cs)
                return o[0], n[0]

            def by_python(x, y, par, mvc):
                w, wn = sc.search_ref_py(cc.fenc_y, cc.luma, cc.luma[0], cc.origin, cc.stride, 16 * x, 16 * y, 0, par,
                                         mvc, cm, c0, me_method, subme, 16, bd=bd)
                rpar = (w[1], w[2], par[0], par[1], par[6], par[7], par[8], par[9])
                w, wrn = refine_chroma_py(cc, 16 * x, 16 * y, 0, rpar, w[0], cm, c0, subme, 0, chroma, none)
                return np.array(w), np.array([wn[0] | (wn[1] << 16), wrn])

            got, gne = mp.analyse_p16x16(by_oracle, MBW, MBH, 512)
            want, wne = mp.analyse_p16x16(by_python, MBW, MBH, 512)
            assert np.array_equal(got, want) and np.array_equal(gne, wne), (kind, lam, subme, got, want)
            dropped += sum(sum(v == (0, 0) or v == pmv for v in mvc) for pmv, mvc in seen)
    assert dropped > 20


# ---------------------------------------------------------------- the inputs reach their paths
def _pooled_rate(cases, jobs, i_pixel, lam):
    pos, par, _ = jobs
    cm, c0 = rc.cost_mv(lam=lam)
    t = 0.0
    for f, c in enumerate(cases):
        sel = pos[:, 0] == f
        t += sel.sum() * dg.first_diamond_tie_rate(c.fenc_y, c.luma[0], c.origin, c.stride, pos[sel, 1:], par[sel],
                                                   i_pixel, cm, c0)
    return t / len(pos)


def _gpu_jobs(bd, i_pixel):
    pos, par, mvc = dg.search_jobs(bd, i_pixel)
    sel = pos[:, 0] == 0
    return pos[sel], par[sel], mvc[sel]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
def test_search_tie_rates(bd, i_pixel):
    """first-diamond tie rates of the lists test_gpu_degenerate.py gives me_search_ref and
    me_search_ref_tesa (degenerate_cases.search_cases / search_jobs), from numpy_ref and the lists
    alone: 1.0 for const at lambda 0, at least 0.15 for const at lambda 40 and for nearflat at
    lambda 0 and 1.  Measured (nearflat 0, nearflat 1, const 40), 8 bit then 10 bit:
    16x16 .17 .19 .42 / .19 .19 .38; 16x8 .18 .19 .41 / .18 .19 .36; 8x16 .18 .21 .40 / .19 .25 .38;
    8x8 .19 .20 .40 / .19 .19 .42; 8x4 .25 .21 .44 / .24 .20 .44; 4x8 .20 .25 .44 / .23 .25 .44;
    4x4 .34 .22 .39 / .34 .23 .39.  Near-flat lists of the three large sizes average 0.08-0.12
    over seeds: degenerate_cases.SEARCH_SEEDS holds seeds whose lists clear the floor"""
    const = dg.search_cases("const", bd, i_pixel)
    flat = dg.search_cases("nearflat", bd, i_pixel)
    jobs = dg.search_jobs(bd, i_pixel)
    assert _pooled_rate(const, jobs, i_pixel, 0) == 1.0
    r = (_pooled_rate(flat, jobs, i_pixel, 0), _pooled_rate(flat, jobs, i_pixel, 1),
         _pooled_rate(const, jobs, i_pixel, 40))
    print("search", bd, i_pixel, ["%.2f" % v for v in r])
    assert min(r) >= 0.15, r


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3])
def test_chain_tie_rates(bd, i_pixel):
    """the same floors over the threshold chain's three lists (degenerate_cases.chain_inputs).
    Measured (nearflat 0, nearflat 1, const 40), 8 bit then 10 bit: 16x16 .18 .19 .36 / .18 .21 .42;
    8x8 .20 .18 .35 / .18 .18 .38"""
    r = []
    for kind, lam in (("const", 0), ("nearflat", 0), ("nearflat", 1), ("const", 40)):
        mr, jobs = dg.chain_inputs(kind, bd, i_pixel)
        cm, c0 = rc.cost_mv(lam=lam)
        t = [dg.first_diamond_tie_rate(mr.fenc_y, mr.refs[k].luma[0], mr.origin, mr.stride, jobs[k][0][:, 1:],
                                       jobs[k][1], i_pixel, cm, c0) for k in range(3)]
        r.append(sum(t) / 3)
    print("chain", bd, i_pixel, ["%.2f" % v for v in r[1:]])
    assert r[0] == 1.0 and min(r[1:]) >= 0.15, r


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 3, 6])
def test_periodic_and_extreme_reach(bd, i_pixel):
    """periodic: SAD(mv) == SAD(mv + (p, 0)) == SAD(mv + (0, p)) at the integer winner of every
    partition whose limits hold both; extreme (and its swap): every cost reached is the full-scale
    SAD bw * bh * ((1 << bd) - 1) plus its mv cost"""
    bw, bh = nr.SIZES[i_pixel]
    p = dg.period(i_pixel)
    pos, par, mvc = _gpu_jobs(bd, i_pixel)
    cc = dg.search_cases("periodic", bd, i_pixel)[0]
    cm, c0 = rc.cost_mv(lam=40)
    held = 0
    for i in range(0, len(pos), 3):
        x, y = int(pos[i, 1]), int(pos[i, 2])
        w, _ = sc.search_ref_py(cc.fenc_y, cc.luma, cc.luma[0], cc.origin, cc.stride, x, y, i_pixel, par[i], mvc[i],
                                cm, c0, 1, 1, 16, bd=bd)
        mx, my = w[1] >> 2, w[2] >> 2
        if mx + p > par[i, 4] or my + p > par[i, 5]:
            continue
        held += 1
        fb = nr.block(cc.fenc_y, cc.origin + y * cc.stride + x, cc.stride, bw, bh)
        s = [nr.sad(fb, nr.block(cc.luma[0], cc.origin + (y + my + dy) * cc.stride + x + mx + dx, cc.stride, bw, bh))
             for dx, dy in ((0, 0), (p, 0), (0, p))]
        assert s[0] == s[1] == s[2], (i, s)
    assert held > 4
    full = bw * bh * ((1 << bd) - 1)
    for kind in ("extreme", "extreme_swap"):
        cc = dg.search_cases(kind, bd, i_pixel)[0]
        top = 0
        for i in range(0, len(pos), 3):
            w, _ = sc.search_ref_py(cc.fenc_y, cc.luma, cc.luma[0], cc.origin, cc.stride, int(pos[i, 1]),
                                    int(pos[i, 2]), i_pixel, par[i], mvc[i], cm, c0, 1, 1, 16, bd=bd)
            assert w[0] == full + w[3], (kind, i, w)
            top = max(top, w[0])
        assert top > full


@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
def test_reach_stays_inside_the_padding(i_pixel):
    """from par alone, for every job list the GPU tests use (96x64 and 112x80; the usual and the
    collapsed limits; the refine and the bidir lists): limits +- the furthest unchecked reach,
    plus the block, plus the hpel margin, inside the padded plane"""
    import weightp_cases as wc
    for w, h in ((96, 64), (112, 80), (W, H)):
        stride, rows = wc._synth().plane_stride(w), h + 2 * dg.PAD
        for seed in range(12):
            for pos, par, _ in (sc.jobs(w // 16, h // 16, 2, i_pixel, seed=seed),
                                ts.degenerate_jobs(w // 16, h // 16, i_pixel, seed)):
                assert (par[:, 2] <= par[:, 4]).all() and (par[:, 3] <= par[:, 5]).all()
                assert dg.reach_inside(pos[:, 1:], par[:, 2:6], par[:, 6:10], i_pixel, w, h, stride, rows) == 0
            pos, par, _ = rc.jobs(w // 16, h // 16, 2, i_pixel, seed=seed)
            assert dg.reach_inside(pos[:, 1:], None, par[:, 4:8], i_pixel, w, h, stride, rows) == 0
            assert (par[:, 0] >= par[:, 4]).all() and (par[:, 0] <= par[:, 6]).all()
            assert (par[:, 1] >= par[:, 5]).all() and (par[:, 1] <= par[:, 7]).all()
    if i_pixel <= 3:
        mr = sc.MultiRef(8, 96, 64, 1, seed=1)
        pos, par, _ = bc.jobs(mr, i_pixel, seed=3)
        assert dg.reach_inside(pos[:, 1:], None, par[:, 8:12], i_pixel, 96, 64, mr.stride,
                               mr.fenc_y.size // mr.stride) == 0
        # the starts lie inside the limits (a start on the 8-qpel guard band returns at once, and
        # eight passes move a vector by at most eight qpel)
        for k in (0, 2):
            assert (par[:, k] >= par[:, 8]).all() and (par[:, k] <= par[:, 10]).all()
            assert (par[:, k + 1] >= par[:, 9]).all() and (par[:, k + 1] <= par[:, 11]).all()
