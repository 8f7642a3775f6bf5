"""CPU: pins tests/tesa_search_cases.py, the Python restatement x264hip_*_me_search_ref_tesa is
checked against, to what the oracle has -- its ESA form is oracle.me_search_ref's (predictor
stage, qpel conversion, counts), its 16x16 window is oracle.me_tesa's and tesa_cases.tesa_python's,
every row's ADS survivors are oracle.ads' on oracle.frame_integral's sums -- checks that the edge
inputs reach the paths they exist for, and that the header declares and the built library
exports the entry point.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import numpy_ref as nr
import refine_cases as rc
import search_cases as sc
import tesa_cases as tc
import tesa_search_cases as ts
from conftest import ROOT, ensure_built
from test_cpu_refine_chroma import _weigh


def _case(bd, W, H, fade, seed):
    cc = rc.ChromaCase(bd, W, H, 1, seed=seed, fade=fade)
    weights = rc.FADE_WEIGHTS if fade else (None, None, None)
    fw = cc.luma[0] if not fade else _weigh(cc.luma[0].astype(np.int64), weights[0], bd).astype(cc.luma[0].dtype)
    return cc, weights, fw


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("subme,fade", [(1, 0), (4, 1)])
def test_esa_form_is_the_oracles(oracle, bd, i_pixel, subme, fade):
    """me_method 3, fpelcmp = SAD: outputs and counts of oracle.me_search_ref's ESA (the integer
    stage alone: its refine is the oracle's own in both)"""
    W, H = 64, 48
    cc, weights, fw = _case(bd, W, H, fade, seed=bd + i_pixel)
    pos, par, mvc = sc.jobs(W // 16, H // 16, 1, i_pixel, seed=subme + i_pixel)
    if i_pixel >= 4:
        pos, par, mvc = ts.corner_rows(pos, par, mvc, W // 16, H // 16)
    cm, c0 = rc.cost_mv()
    want, wne = oracle.me_search_ref(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, fw, cc.origin, cc.stride, i_pixel, 3,
                                     subme, 16, pos[:, 1:], par, mvc, cm, c0,
                                     ext=oracle.refine_ext(0, 1, 0, weights))
    buf, i8, i4 = ts.integral_planes(oracle, bd, cc.luma[0], cc.origin, cc.stride, H)
    for i in range(len(pos)):
        r, nf, _ = ts.search_ref_tesa_py(cc.fenc_y, cc.luma, fw, cc.origin, cc.stride, int(pos[i, 1]), int(pos[i, 2]),
                                         i_pixel, par[i], mvc[i], cm, c0, subme, 16, buf, i8 if i_pixel <= 3 else i4,
                                         H, me_method=3, fpel_satd=False, weight0=weights[0], bd=bd)
        assert wne[i, 0] == nf[0] | (nf[1] << 16), (i, hex(wne[i, 0]), nf)
        if subme >= 2:
            rpar = np.array([[r[1], r[2], par[i, 0], par[i, 1], par[i, 6], par[i, 7], par[i, 8], par[i, 9]]], np.int16)
            r = oracle.me_refine_subpel(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.origin, cc.stride, i_pixel,
                                        subme, pos[i:i + 1, 1:], rpar, np.array([r[0]], np.int32), cm, c0,
                                        ext=oracle.refine_ext(0, 1, 0, weights))[0]
        assert tuple(want[i]) == tuple(r), (i, want[i], r)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("me_range,satd", [(16, True), (8, False), (24, True), (4, True), (32, False)])
def test_window_16x16_is_me_tesa(oracle, bd, me_range, satd):
    """i_pixel 0: tesa_window_py = oracle.me_tesa = tesa_cases.tesa_python from the same centre and
    init cost"""
    import weightp_cases as wc
    synth = wc._synth()
    W, H = 96, 64
    planes, stride, org = synth.make_sequence(2, W, H, bd, seed=11 + me_range)
    mbw, mbh = W // 16, H // 16
    f1, f0 = planes[1].ravel(), planes[0].ravel()
    integ = oracle.frame_integral(bd, f0, org, stride, H, tc.PAD, False).ravel()
    i_org = tc.PAD * stride + tc.PAD
    par, init = tc.params(mbw, mbh, me_range, seed=bd * 7 + me_range)
    cmv, c0 = tc.cost_mv()
    want = oracle.me_tesa(bd, f1, org, stride, f0, org, integ, i_org, stride, mbw, mbh, me_range, satd, par, init, cmv,
                          c0)
    for mb in range(mbw * mbh):
        x, y = 16 * (mb % mbw), 16 * (mb // mbw)
        p = [int(v) for v in par[mb]]
        fb = nr.block(f1, org + y * stride + x, stride, 16, 16)
        got = ts.tesa_window_py(0, fb, f0, org, stride, x, y, integ, i_org, H, (p[2], p[3]), tuple(p[4:8]), cmv, c0,
                                me_range, p[0], p[1], int(init[mb]), nr.satd if satd else nr.sad)
        assert tuple(want[mb]) == got[:4], (mb, want[mb], got)
        lit = tc.tesa_python(bd, f1, org, f0, org, integ, i_org, stride, mb % mbw, mb // mbw, me_range, satd, par[mb],
                             init[mb], cmv, c0, lambda o: nr.sad(fb, nr.block(f0, o, stride, 16, 16)),
                             lambda o: nr.satd(fb, nr.block(f0, o, stride, 16, 16)))
        assert lit == got[:4], (mb, lit, got)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_pixel", [0, 1, 2, 3, 4, 5, 6])
def test_rows_are_the_oracles_ads(oracle, bd, i_pixel):
    """every size: each scanned row's survivor list = oracle.ads (ads4 / ads2 / ads1) on
    oracle.frame_integral(sub8x8)'s plane of the partition's sad_size"""
    W, H = 64, 48
    cc, weights, fw = _case(bd, W, H, 0, seed=3 + bd + i_pixel)
    pos, par, mvc = ts.corner_rows(*sc.jobs(W // 16, H // 16, 1, i_pixel, seed=i_pixel), W // 16, H // 16)
    cm, c0 = rc.cost_mv()
    buf, i8, i4 = ts.integral_planes(oracle, bd, cc.luma[0], cc.origin, cc.stride, H)
    nsums = 4 if i_pixel == 0 else 1 if i_pixel in (3, 6) else 2
    rows = [0]

    def on_row(my, enc_dc, s_off, delta, cost_fpel, width, thresh, xs):
        rows[0] += 1
        want = oracle.ads(bd, nsums, enc_dc + [0] * (4 - len(enc_dc)), buf, s_off, delta, cost_fpel, 0, width, thresh)
        assert list(want) == xs, (my, list(want), xs)

    for i in range(0, len(pos), 2):
        ts.search_ref_tesa_py(cc.fenc_y, cc.luma, fw, cc.origin, cc.stride, int(pos[i, 1]), int(pos[i, 2]), i_pixel,
                              par[i], mvc[i], cm, c0, 2, 16, buf, i8 if i_pixel <= 3 else i4, H, bd=bd, on_row=on_row)
    assert rows[0] > 30                                   # rows were scanned


def test_refine_fpel_satd_is_the_oracles(oracle):
    """refine_fpel_satd_py (the refine restatement with fpelcmp = SATD, which the threshold chain
    test needs: the oracle's refine with fpel_satd takes no threshold) = the oracle's refine with
    fpel_satd, results and counts, where the threshold is off"""
    bd, W, H, cf = 8, 64, 48, 1
    cc = rc.ChromaCase(bd, W, H, cf, seed=5)
    cm, c0 = rc.cost_mv()
    for i_pixel, subme in ((0, 7), (3, 7), (1, 9), (2, 5)):
        pos, par, cost = rc.jobs(W // 16, H // 16, 1, i_pixel, seed=subme)
        chroma = 1
        want, wn = oracle.me_refine_subpel(bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.origin, cc.stride, i_pixel,
                                           subme, pos[:, 1:], par, cost, cm, c0, fpel_satd=True, counts=True,
                                           ext=oracle.refine_ext(chroma, cf, 0), fenc_c=cc.fenc_c, fc_origin=cc.co,
                                           fcs=cc.cs, ref_c=cc.ref_c, rc_origin=cc.co, rcs=cc.cs)
        for i in range(0, len(pos), 3):
            got, n = ts.refine_fpel_satd_py(cc, int(pos[i, 1]), int(pos[i, 2]), i_pixel, par[i], cost[i], cm, c0,
                                            subme, 0, chroma, (None, None, None))
            assert tuple(want[i]) == got and wn[i] == n, (i_pixel, subme, i, want[i], got, hex(wn[i]), hex(n))


@pytest.mark.parametrize("i_pixel", [0, 3, 5])
def test_edge_inputs_reach_their_paths(oracle, i_pixel):
    """the inputs of test_gpu_tesa_search.py's edge test take the paths they exist for: windows of
    width 0, rows skipped on bsad <= ycost, both prune loops, and (the sizes below 16x16) scanned
    windows that leave an empty list"""
    bd = 8
    ts.HITS.clear()
    for cases, (pos, par, mvc), (cm, c0), subme, chroma, W, H in ts.edge_inputs(bd, i_pixel):
        c = cases[0]
        integ = ts.integral_planes(oracle, bd, c.luma[0], c.origin, c.stride, H)
        ts.expected(oracle, bd, c, c.luma[0], i_pixel, subme, 16, pos[:, 1:], par, mvc, cm, c0, integ,
                    (None, None, None), chroma, 1)
    for k in ("width0", "row_skip", "halve", "drop_max") + (("empty_list",) if i_pixel else ()):
        assert ts.HITS[k] > 0, (k, dict(ts.HITS))


def test_entry_declared_and_exported():
    """include/x264hip.h declares x264hip_{8,10}_me_search_ref_tesa and the built library exports
    both"""
    hdr = open(os.path.join(ROOT, "include", "x264hip.h")).read()
    assert re.search(r"int x264hip_##BD##_me_search_ref_tesa\(", hdr)
    lib = ctypes.CDLL(ensure_built("hip"))
    for bd in (8, 10):
        assert hasattr(lib, f"x264hip_{bd}_me_search_ref_tesa")
