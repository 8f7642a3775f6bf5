"""CPU: the checker of the intra mode decision (tests/mbanalyse_cases.py) held to independent
evidence, and the host side of include/x264hip_mbanalyse.h.  No GPU.

* The tables of the checker and of the kernel source (csrc/mbanalysedev.h) equal
  tests/golden/mbanalyse_tables.json; the JSON equals a fresh parse of the reference where it is
  there.
* Hand-worked single-block vectors for the 4x4 and 8x8 rules: the tie orders, the - 3 * lambda, the
  <= 0 break, the i_best >= 0 guard, the i_best > 0 gate, favor_vertical on equality.
* The outputs of every decided-intra macroblock equal mbintra_cases.encode_mb fed the decided flags
  and modes on the reconstruction around it (the i_skip_intra equivalence).
* The I_4x4 pass in the kernel's form (every block scored, the early termination replayed
  afterwards) agrees with the literal loop on every try macroblock that reaches the pass.
* Coverage over exactly the GPU tests' inputs, per bit depth.
* The header's prototypes, the ctypes declarations, the exported symbols and the struct layout
  agree; every X264HIP_EINVAL case."""
import collections
import ctypes
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import mbanalyse_cases as ma
import mbenc_cases as mc
import mbintra_cases as mi
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mbanalyse.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mbanalyse_tables.json")
REFERENCE = os.environ.get("X264_REFERENCE_DIR", "/root/reference")     # the reference tree, where there is one


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def gpu_keys(bd):
    """the keys tests/test_gpu_mbanalyse.py runs at one bit depth"""
    ks = [key for key, _ in ma.gpu_keys(bd=bd)]
    return sorted(set(ks), key=ks.index)


# ------------------------------------------------------------------ 1. the tables
def _rows(flat, width):
    return tuple(tuple(flat[i:i + width]) for i in range(0, len(flat), width))


def test_checker_tables_equal_the_golden_file():
    g = golden()
    assert list(ma.LAMBDA_TAB) == g["x264_lambda_tab"]
    assert ma.I16x16_MODE_AVAILABLE == _rows(g["i16x16_mode_available"], 5)
    assert ma.CHROMA_MODE_AVAILABLE == _rows(g["chroma_mode_available"], 5)
    assert ma.I4x4_MODE_AVAILABLE == _rows(g["i4x4_mode_available0"], 10)
    assert ma.I8x8_MODE_AVAILABLE == _rows(g["i8x8_mode_available0"], 10)
    assert tuple(r for pair in ma.INTRA_ANALYSIS_SHORTCUT for r in pair) == _rows(g["intra_analysis_shortcut0"], 5)
    assert list(ma.I16x16_THRESH_LUT) == g["i16x16_thresh_lut"] and list(ma.I8x8_THRESH) == g["i8x8_thresh"]
    assert list(ma.COST_DIV_FIX8) == g["cost_div_fix8"]
    assert [ma.MB_B_COST[k] for k in ("i4", "i8", "i16")] == g["i_mb_b_cost_intra"]
    assert list(ma.PRED_MODE16x16_FIX) == g["x264_mb_pred_mode16x16_fix"]
    assert list(ma.CHROMA_PRED_MODE_FIX) == g["x264_mb_chroma_pred_mode_fix"]


def _source_lists(src, fn):
    """the modes( { ... } ) lists of device function fn, in case order"""
    m = re.search(r"\b" + fn + r"\([^)]*\)\s*\{([^\n]+\}|.*?\n\})", src, re.S)   # a one-line body, or up to the closing brace
    assert m, fn
    return [tuple(int(v) for v in re.findall(r"-?\d+", body)) for body in re.findall(r"modes\(\s*\{([^}]*)\}", m.group(1))]


def test_kernel_tables_equal_the_golden_file():
    g = golden()
    src = open(os.path.join(ROOT, "x264-i386pic_amd", "csrc", "mbanalysedev.h")).read()
    strip = lambda rows: [tuple(v for v in r if v >= 0) for r in rows]
    assert _source_lists(src, "i16x16_mode_available") == strip(_rows(g["i16x16_mode_available"], 5))
    assert _source_lists(src, "chroma_mode_available") == strip(_rows(g["chroma_mode_available"], 5))
    assert _source_lists(src, "i4x4_mode_available") == strip(_rows(g["i4x4_mode_available0"], 10))
    assert _source_lists(src, "i8x8_mode_available") == strip(_rows(g["i8x8_mode_available0"], 10))
    assert _source_lists(src, "intra_analysis_shortcut") == strip(_rows(g["intra_analysis_shortcut0"], 5))
    # the thresholds at i_subpel_refine 0..5 (2..5 are accepted), the rescale, the B prefix
    assert _source_lists(src, "i16x16_thresh_lut") == [tuple(g["i16x16_thresh_lut"][:6])]
    assert _source_lists(src, "i8x8_thresh") == [tuple(g["i8x8_thresh"][:6])]
    m = re.search(r"cost_div_fix8\( int idx \) \{ return idx == 0 \? (\d+) : idx == 1 \? (\d+) : (\d+); \}", src)
    assert m and [int(v) for v in m.groups()] == g["cost_div_fix8"]
    m = re.search(r"MB_B_COST_INTRA = (\d+);", src)
    assert m and [int(m.group(1))] * 3 == g["i_mb_b_cost_intra"]
    assert re.search(r"COST_MAX = 1 << 28;", src) and ma.COST_MAX == 1 << 28
    # the fixed-mode code lengths the source folds into two functions
    ue = ma.UE_SIZE
    want16 = [ue[g["x264_mb_pred_mode16x16_fix"][m]] for m in range(7)]
    wantc = [ue[g["x264_mb_chroma_pred_mode_fix"][m]] for m in range(7)]
    assert want16 == [1 if m == 0 else 5 if m == 3 else 3 for m in range(7)]          # ue_mode16
    assert wantc == [3 if m in (1, 2) else 5 if m == 3 else 1 for m in range(7)]       # ue_chroma
    assert "mode == 0 ? 1 : mode == 3 ? 5 : 3" in src and "mode == 1 || mode == 2 ? 3 : mode == 3 ? 5 : 1" in src


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference tree (X264_REFERENCE_DIR)")
def test_golden_file_equals_a_fresh_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_mbanalyse_tables",
                                                  os.path.join(ROOT, "tests", "golden", "make_mbanalyse_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.tables(REFERENCE) == golden()


# ------------------------------------------------------------------ 2. hand-worked single blocks
ALL4 = mi.MB_LEFT | mi.MB_TOP | mi.MB_TOPLEFT | mi.MB_TOPRIGHT


def _block4(top, left, lt, fenc4, bd=8):
    """FENC / FDEC buffers of macroblock block 0 with the 4x4 neighbours given"""
    dt = np.uint8 if bd == 8 else np.uint16
    fdec, fenc = np.zeros(mi.BUF, dt), np.zeros(16 * mi.FENC, dt)
    v = fdec.reshape(18, mi.FDEC)
    v[0, 8:16] = top
    v[1:5, 7] = left
    v[0, 7] = lt
    fenc.reshape(16, mi.FENC)[:4, :4] = fenc4
    return fenc, fdec


def test_i4x4_flat_block_ties():
    """every prediction of a flat block with flat neighbours is exact: all SATDs are 0"""
    lam = 4
    fenc, fdec = _block4([100] * 8, [100] * 4, 100, 100)
    cnt = collections.Counter()
    # predicted mode DC: satd[DC] = -3 * lambda < V = H = 0: DC stays (first of the comparison order),
    # favor_vertical false on equality, and i_best > 0 is false: no further mode is tried
    assert ma.i4x4_block(8, 0, ALL4, 2, lam, fenc, fdec, cnt) == (-3 * lam, 2)
    assert cnt["i4_x3", 1, 0] == 1 and cnt["i4_favor_tie"] == 1 and cnt["i4_best_gate_false"] == 1
    # predicted mode V: V wins with -3 * lambda; predicted H likewise
    assert ma.i4x4_block(8, 0, ALL4, 0, lam, fenc, fdec, cnt) == (-3 * lam, 0)
    assert ma.i4x4_block(8, 0, ALL4, 1, lam, fenc, fdec, cnt) == (-3 * lam, 1)
    # a predicted mode outside the three: all three tie at 0, DC is kept (H and V need <), gate false
    assert ma.i4x4_block(8, 0, ALL4, 5, lam, fenc, fdec, cnt) == (0, 2)
    assert cnt["i4_best_gate_false"] == 4


def test_i4x4_le0_break_and_bonus():
    """fenc = the HU prediction of a left ramp, top far off: V / H / DC are bad, favor_vertical is
    false (H < V), the shortcut list is DDR, HD, HU; with HU predicted its exact match gives
    0 - 3 * lambda <= 0 and breaks; with DDR predicted HU wins at 0 without a bonus"""
    lam = 2
    left = [10, 50, 90, 130]
    n = [200] * 8 + left + [200]
    hu = mi.pred4x4_dir(8, n)
    fenc, fdec = _block4([200] * 8, left, 200, hu)
    cnt = collections.Counter()
    assert ma.i4x4_block(8, 0, ALL4, 8, lam, fenc, fdec, cnt) == (-3 * lam, 8)
    assert cnt["i4_le0_break"] == 1 and cnt["i4_x3", 1, 0] == 1
    cnt = collections.Counter()
    best, mode = ma.i4x4_block(8, 0, ALL4, 4, lam, fenc, fdec, cnt)
    assert (best, mode) == (0, 8) and cnt["i4_le0_break"] == 0 and cnt["i4_pred_bonus"] == 1 and cnt["i4_shortcut_wins"] == 1


def test_i4x4_edge_lists():
    """without neighbours only DC_128; with the left column only DC_LEFT, H, HU in that order: on a
    flat block the first of the list keeps the tie"""
    cnt = collections.Counter()
    fenc, fdec = _block4([0] * 8, [0] * 4, 0, 128)
    assert ma.i4x4_block(8, 0, 0, 2, 3, fenc, fdec, cnt) == (-9, 11)       # DC_128 is fixed to DC: the bonus, and the <= 0 break
    assert cnt["i4_le0_break"] == 1
    fenc, fdec = _block4([0] * 8, [77] * 4, 0, 77)
    # DC_LEFT scores 0 first; H, the predicted mode, then scores 0 - 3 * lambda <= 0 and breaks
    assert ma.i4x4_block(8, 0, mi.MB_LEFT, 1, 3, fenc, fdec, cnt) == (-9, 1) and cnt["i4_le0_break"] == 2
    # with HU predicted DC_LEFT and H tie at 0, the first keeps it, and HU's bonus ends the loop
    assert ma.i4x4_block(8, 0, mi.MB_LEFT, 8, 3, fenc, fdec, cnt) == (-9, 8)
    # with V predicted (not in the list) nothing gets the bonus: the first of the list keeps the tie
    assert ma.i4x4_block(8, 0, mi.MB_LEFT, 0, 3, fenc, fdec, cnt) == (0, 9)
    # top and left without top-left (predict_mode[8] < 0; no picture position gives it): the short list
    fenc, fdec = _block4([100] * 8, [100] * 4, 0, 100)
    best, mode = ma.i4x4_block(8, 0, mi.MB_LEFT | mi.MB_TOP, 7, 3, fenc, fdec, cnt)
    assert cnt["i4_x3", 0, 0] == 1 and (best, mode) == (0, 2)


def _block8(top16, left8, lt, fenc8):
    fdec, fenc = np.zeros(mi.BUF, np.uint8), np.zeros(16 * mi.FENC, np.uint8)
    v = fdec.reshape(18, mi.FDEC)
    v[0, 8:24] = top16
    v[1:9, 7] = left8
    v[0, 7] = lt
    fenc.reshape(16, mi.FENC)[:8, :8] = fenc8
    return fenc, fdec


def test_i8x8_guard_and_tie_order():
    """a flat 8x8 block: with DC predicted the best of three runs i = 2 down to 0, DC first, at
    -3 * lambda; the mode loop is stopped by i_best >= 0 before its first mode.  With nothing of the
    three predicted all tie at 0, DC is kept, favor_vertical is false, and the shortcut modes DDR,
    HD, HU (all exact, 0) do not beat it with <"""
    lam = 5
    fenc, fdec = _block8([60] * 16, [60] * 8, 60, 60)
    cnt = collections.Counter()
    best, mode, _ = ma.i8x8_block(8, 0, ALL4, 2, lam, fenc, fdec, cnt)
    assert (best, mode) == (-3 * lam, 2) and cnt["i8_best_guard_stop"] == 1 and cnt["i8_favor_tie"] == 1
    cnt = collections.Counter()
    best, mode, _ = ma.i8x8_block(8, 0, ALL4, 6, lam, fenc, fdec, cnt)
    # HD is predicted: its exact match gets the bonus and wins; the loop then stops at i_best < 0
    assert (best, mode) == (-3 * lam, 6) and cnt["i8_x3", 1, 0] == 1 and cnt["i8_best_guard_stop"] == 1
    cnt = collections.Counter()
    best, mode, _ = ma.i8x8_block(8, 0, ALL4, 7, lam, fenc, fdec, cnt)
    assert (best, mode) == (0, 2) and cnt["i8_best_guard_stop"] == 0 and cnt["i8_shortcut_wins"] == 0


def test_predicted_mode_rules():
    assert ma.predict_intra4x4_mode(-1, 5) == 2 and ma.predict_intra4x4_mode(5, -1) == 2
    assert ma.predict_intra4x4_mode(9, 5) == 2 and ma.predict_intra4x4_mode(8, 11) == 2
    assert ma.predict_intra4x4_mode(7, 3) == 3 and ma.predict_intra4x4_mode(0, 8) == 0
    case = types.SimpleNamespace(mbw=3)
    flags = np.array([ma.INTRA, ma.INTRA | ma.T8, ma.INTRA | ma.I16, 0, ma.INTRA, 0], np.uint8)
    pm = np.arange(6 * 16, dtype=np.int8).reshape(6, 16) % 9
    nb = mi.MB_LEFT | mi.MB_TOP
    # macroblock 4: left (3) is inter -> DC; top (1) is I_8x8 -> DC
    assert ma.neighbour_modes(case, flags, pm, 4, nb) == [2] * 8
    # macroblock 5: left (4) is I_4x4 -> its blocks 5, 7, 13, 15; top (2) I_16x16 -> DC
    assert ma.neighbour_modes(case, flags, pm, 5, nb) == [int(pm[4][b]) for b in (5, 7, 13, 15)] + [2] * 4
    # macroblock 3: top (0) is I_4x4 -> its blocks 10, 11, 14, 15; no left
    assert ma.neighbour_modes(case, flags, pm, 3, mi.MB_TOP) == [-1] * 4 + [int(pm[0][b]) for b in (10, 11, 14, 15)]


# ------------------------------------------------------------------ 3. the cases
@pytest.mark.parametrize("bd", [8, 10])
def test_decided_macroblocks_equal_encode_mb_and_prefix_form(bd):
    """for the 5x4 x 2 cases of every format and slice type: a decided-intra macroblock's outputs
    are mbintra_cases.encode_mb's with the decided flags and modes on the final reconstruction
    around it, and the I_4x4 pass in the kernel's form gives the literal loop's cost, modes and
    stopping index on every try macroblock"""
    checked = passes = 0
    for cf in (0, 1, 2):
        for st in (0, 1, 2):
            key = ma.make_key(bd, cf, 5, 4, 2, st)
            case, out = ma.make_case(*key), ma.expected(key, 1)
            T = mc.tables(bd, case.cqm)
            for mb in np.flatnonzero(case.try_intra):
                qp = int(case.qp[mb])
                f, my, mx, nb, fenc_y, fenc_c, fdec_y, fdec_c = mi.mb_buffers(case, out.recon_y, out.recon_c, mb)
                if out.intra[mb]:
                    o = mi.encode_mb(bd, T, cf, 1, int(out.mb_flags_out[mb]), qp, int(case.qp_table[qp]), out.pred_mode[mb],
                                     int(out.chroma_pred_mode[mb]), nb, fenc_y, fdec_y, fenc_c, fdec_c, collections.Counter())
                    assert np.array_equal(o.level, out.level[mb]) and np.array_equal(o.nnz, out.nnz[mb])
                    assert np.array_equal(o.luma_dc, out.luma_dc[mb]) and np.array_equal(o.chroma_dc, out.chroma_dc[mb])
                    assert np.array_equal(fdec_y.reshape(18, mi.FDEC)[1:17, 8:24],
                                          out.recon_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16])
                    assert out.flags_out[mb] == out.mb_flags_out[mb] & 3
                    checked += 1
                # the two forms of the I_4x4 pass on this macroblock's neighbours
                lam = ma.LAMBDA_TAB[qp]
                nm = ma.neighbour_modes(case, out.mb_flags_out, out.pred_mode, mb, nb)
                for thresh in (ma.COST_MAX, int(out.cost[mb][2] if out.cost[mb][2] < ma.COST_MAX else out.cost[mb][0]) // 2):
                    b1 = mi.mb_buffers(case, out.recon_y, out.recon_c, mb)
                    b2 = mi.mb_buffers(case, out.recon_y, out.recon_c, mb)
                    lit = ma.i4x4_pass(bd, T, qp, lam, nb, nm, lam * 40, thresh, b1[4], b1[6], collections.Counter())
                    pre = ma.i4x4_prefix_form(bd, T, qp, lam, nb, nm, lam * 40, thresh, b2[4], b2[6])
                    assert lit[0] == pre[0] and lit[2] == pre[2], (key, mb, thresh)
                    assert lit[1][:lit[2] + 1] == pre[1][:lit[2] + 1]
                    passes += lit[2] < 15
    assert checked > 100 and passes > 50


@pytest.mark.parametrize("bd", [8, 10])
def test_coverage_of_the_gpu_inputs(bd):
    tot = collections.Counter()
    per_cf = {cf: collections.Counter() for cf in (0, 1, 2)}
    for key in gpu_keys(bd):
        for dec in (0, 1):
            c = ma.expected(key, dec).counters
            tot.update(c)
            per_cf[key[1]].update(c)
    c = tot
    for st in (0, 1, 2):
        for kind in ("i16", "i8", "i4"):
            assert c["decided", st, kind], (st, kind)
    assert c["decided", 1, None] and c["decided", 2, None]
    assert c["i16_plane_evaluated"] and c["i16_plane_skipped"] and c["return_740"] and c["return_860"]
    assert all(c["chosen16", m] for m in range(7))
    assert all(c["chosen4", m] for m in range(12)) and all(c["chosen8", m] for m in range(12))
    assert all(c["i8_loop_end", i, 1] for i in (0, 1, 2)) and c["i8_loop_end", 3, 0]
    assert c["i4_loop_break"] and c["i4_loop_complete"]
    for size in ("i4", "i8"):
        assert c[size + "_x3", 1, 0] and c[size + "_x3", 1, 1] and c[size + "_favor_tie"] and c[size + "_shortcut_wins"]
        # predict_mode[8] < 0 needs top and left without top-left, which no position of a
        # one-slice picture has: test_i4x4_edge_lists reaches it in the checker alone
        assert not c[size + "_x3", 0, 0] and not c[size + "_x3", 0, 1]
    assert c["i4_best_gate_false"] and c["i4_le0_break"] and c["i8_best_guard_stop"]
    for cf in (1, 2):
        c = per_cf[cf]
        assert all(c["chosenc", m] for m in range(7)), cf
        assert c["chroma_x3"] and c["chroma_list"]
        assert all(c["decided", st, kind] for st in (0, 1) for kind in ("i16", "i8", "i4")), cf


BOUNDS = (("chroma_list_cost",), ("chroma_x3_cost",), ("i16_x3_cost",), ("i16_plane_cost",), ("i16_cost",), ("i8_best",),
          ("i8_gate",), ("type_i", "i4"), ("type_i", "i8"), ("type_pb", "i4"), ("type_pb", "i8"))
RUNNING = ("i4_cost", "i8_cost")                                     # (bound, side, at the last block)


@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_keys_reach_every_bound_on_both_sides(bd):
    """over exactly what tests/test_gpu_mbanalyse.py runs at this depth, each cost the reference
    compares with a threshold or with another cost is seen below it, above it and exactly on it"""
    tot = collections.Counter()
    for key, dec in ma.gpu_keys(bd=bd):
        tot.update(ma.expected(key, dec).counters)
    for b in BOUNDS:
        assert tot[b + ("below",)] and tot[b + ("above",)], b
        assert tot[b + ("at",)], b
    for b in RUNNING:                                                # before the last block, where the loop can still stop
        assert tot[b, "below", 0] and tot[b, "at", 0] and tot[b, "above", 0], b
    assert tot["type_pb", "i16", "below"] and tot["type_pb", "i16", "above"]


@pytest.mark.parametrize("bd", [8, 10])
def test_every_boundary_picture_sits_on_its_bound(bd):
    """each picture of BOUNDARY, at each depth, has the comparison it is named for at equality"""
    for row, (what, at, _, _) in enumerate(ma.BOUNDARY):
        assert ma.expected(ma.boundary_key(bd, row), 1).counters[at] > 0, (bd, what)


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised selections of tests/test_gpu_mbanalyse.py add up to gpu_keys()"""
    picked = [kd for bd in (8, 10) for cf in (0, 1, 2) for st in (0, 1, 2) for kd in ma.gpu_keys("shapes", bd=bd, cf=cf, slice_type=st)]
    picked += [kd for bd in (8, 10) for kw in ma.OPTIONS for kd in ma.gpu_keys("options", bd=bd, **kw)]
    picked += [kd for bd in (8, 10) for c in ("flat", "checker") for kd in ma.gpu_keys("content", bd=bd, content=c)]
    picked += [kd for bd in (8, 10) for st in (0, 1) for kd in ma.gpu_keys("noise", bd=bd, slice_type=st)]
    picked += [kd for bd in (8, 10) for kd in ma.gpu_keys("boundary", bd=bd)]
    assert sorted(map(repr, picked)) == sorted(map(repr, ma.gpu_keys()))
    for key, _ in ma.gpu_keys("boundary"):
        assert key[2] <= 5 and key[3] <= 4 and key[4] <= 2


@pytest.mark.parametrize("bd", [8, 10])
def test_chroma_me_and_b_prefix_change_decisions(bd):
    """the same inputs with and without the chroma-ME leg, and a B picture's inputs taken as a P
    picture's, decide some macroblock differently"""
    a = ma.expected(ma.make_key(bd, 1, 5, 4, 2, 1, b_chroma_me=1), 1)
    b = ma.expected(ma.make_key(bd, 1, 5, 4, 2, 1), 1)
    assert np.array_equal(ma.make_case(*ma.make_key(bd, 1, 5, 4, 2, 1, b_chroma_me=1)).satd_inter,
                          ma.make_case(*ma.make_key(bd, 1, 5, 4, 2, 1)).satd_inter)
    assert (a.mb_flags_out != b.mb_flags_out).any()
    key = ma.make_key(bd, 2, 5, 4, 2, 2)
    case = ma.make_case(*key)
    as_p = types.SimpleNamespace(**vars(case))
    as_p.slice_type = ma.SLICE_P
    assert (ma.encode(as_p, 1).mb_flags_out != ma.expected(key, 1).mb_flags_out).any()


# ------------------------------------------------------------------ 4. the host side
_SCALARS = {"int": ctypes.c_int, "void": None}


def test_signatures_symbols_and_layout(tmp_path):
    so = ensure_built("hip")
    x = load_package()
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(x264hip_\w+)\s*\(([^)]*)\)\s*;", text)
    assert sorted(n for n, _ in protos) == sorted(f"x264hip_{bd}_{n}" for n in x._MBANALYSE for bd in (8, 10)) == \
        ["x264hip_10_mb_analyse_intra", "x264hip_8_mb_analyse_intra"]
    L = x.lib()
    for name, params in protos:
        fn = getattr(L, name)
        params = [p.strip() for p in params.split(",")]
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == 5
        for p, a in zip(params, fn.argtypes):
            assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p)
        assert params[-1] == "void *stream"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert {n for n, _ in protos} <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in ("mb_analyse_intra", "MbAnalyse", "MBANALYSE_OUTPUTS", "COST_MAX"):
        assert n in x.__all__
    assert all("mb_analyse_intra" not in t for t in (x._PER_DEPTH, x._PLAIN, x._MBINTRA, x._MBENC, x._MBSKIP))
    names = [n for n, _ in x.MbAnalyse._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "x264hip_mbanalyse.h"\nint main(void) {\n'
    src += '    printf("size %zu\\n", sizeof(x264hip_mbanalyse_t));\n'
    for n in names:
        src += f'    printf("{n} %zu\\n", offsetof(x264hip_mbanalyse_t, {n}));\n'
    src += "    return 0;\n}\n"
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(vals.pop("size")) == ctypes.sizeof(x.MbAnalyse)
    for n in names:
        assert getattr(x.MbAnalyse, n).offset == int(vals[n]), n
    # the fields x264hip_mbintra_t has, under the same names at the same offsets
    for n, _ in x.MbIntra._fields_:
        assert getattr(x.MbAnalyse, n).offset == getattr(x.MbIntra, n).offset, n


_TABLE = np.minimum(np.arange(64), 39).astype(np.uint8)
_LAMBDA = np.array(ma.LAMBDA_TAB[:64], np.uint16)
EINVAL, ADDR = -1, 0x40000000


def _a(x, **kw):
    """a valid x264hip_mbanalyse_t on made-up addresses"""
    a = x.MbAnalyse()
    a.chroma_format, a.b_dct_decimate, a.slice_type, a.i_subpel_refine, a.b_i4x4, a.b_i8x8 = 1, 1, 1, 5, 1, 1
    a.chroma_qp_table, a.lambda_tab = _TABLE.ctypes.data, _LAMBDA.ctypes.data
    k = 0
    for n, t in x.MbAnalyse._fields_:
        if t is ctypes.c_void_p and n not in ("chroma_qp_table", "lambda_tab"):
            setattr(a, n, ADDR + 0x1000000 * k)
            k += 1
        elif n.endswith("_frame_stride"):
            setattr(a, n, 192 * 128)
        elif n.endswith("_stride"):
            setattr(a, n, 192)
    for n, v in kw.items():
        setattr(a, n, v)
    return a


@pytest.mark.parametrize("bd", [8, 10])
def test_mb_analyse_intra_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced);
    an empty batch is X264HIP_OK"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_analyse_intra")
    call = lambda a, mbw=5, mbh=4, n=2: fn(ctypes.byref(a) if a is not None else None, mbw, mbh, n, None)
    assert call(None) == EINVAL
    assert call(_a(x), 0) == 0 and call(_a(x), n=0) == 0
    for field in ("lambda_tab", "try_intra", "cost", "mb_flags_out", "pred_mode", "chroma_pred_mode", "satd_inter",
                  "chroma_qp_table", "quant4_mf", "quant4_bias", "dequant4_mf", "fenc", "recon", "fenc_chroma", "recon_chroma",
                  "qp", "mb_flags", "level", "chroma_dc", "nnz", "cbp", "nz", "flags_out", "luma_dc"):
        assert call(_a(x, **{field: None}), 0) == EINVAL, field
    # what the format or the slice type does not need may be NULL
    assert call(_a(x, chroma_format=0, chroma_pred_mode=None, fenc_chroma=None, recon_chroma=None), 0) == 0
    assert call(_a(x, slice_type=0, satd_inter=None), 0) == 0
    assert call(_a(x, fast_intra=None), 0) == 0
    for kw in (dict(slice_type=-1), dict(slice_type=3), dict(i_subpel_refine=1), dict(i_subpel_refine=6),
               dict(chroma_format=3), dict(cost=ADDR + 2), dict(luma_dc=ADDR + 1), dict(recon=ADDR + 2),
               dict(recon_stride=190), dict(recon_chroma_frame_stride=192 * 64 + 2),
               dict(quant8_mf=None), dict(quant8_mf=None, quant8_bias=None, dequant8_mf=None)):
        assert call(_a(x, **kw), 0) == EINVAL, kw
    # without the 8x8 tables the entry stands when I_8x8 is off
    assert call(_a(x, b_i8x8=0, quant8_mf=None, quant8_bias=None, dequant8_mf=None), 0) == 0
    assert call(_a(x), -1) == EINVAL and call(_a(x), 1 << 15, 1 << 14, 1) == EINVAL
    bad = _TABLE.copy()
    bad[20] = 52 + 6 * (bd - 8)
    assert call(_a(x, chroma_qp_table=bad.ctypes.data), 0) == EINVAL
