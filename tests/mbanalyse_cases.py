"""The intra mode decision restated per macroblock from the reference's C (x264_mb_analyse_intra
and mb_analyse_intra_chroma, encoder/analyse.c:586-980; the decisions of x264_macroblock_analyse,
:2939-2946, :3181-3223, :3591-3618; x264_mb_predict_intra4x4_mode, common/macroblock.h:419-431;
the modes a macroblock hands to its neighbours, common/macroblock.c:1727-1737), and the inputs of
tests/test_cpu_mbanalyse.py and tests/test_gpu_mbanalyse.py.  No GPU code.  The method is
tests/mbintra_cases.py's:

* Only the control flow is Python, a literal restatement of the C in its serial order, with a
  counter per branch.  Every metric (satd, sa8d, intra_*_x3), predictor, transform and quantiser is
  the oracle's (tests/oracle_lib.py) or mbintra_cases', called on FENC / FDEC-layout buffers.
* The configuration is include/x264hip_mbanalyse.h's: i_mbrd = 0, the C path without
  intra_mbcmp_x9, no lossless, b_avoid_topright = 0, b_early_terminate = 1, one slice.
* encode(case, dec): mbenc_cases.encode for the inter macroblocks of a P / B picture, then the raster
  loop over the try and the given-mode intra macroblocks in place (the raster order and the
  device's anti-diagonal order see the same neighbours).  A macroblock decided intra is encoded by
  mbintra_cases.encode_mb on fresh buffers with the decided flags and modes.
* i4x4_prefix_form: the I_4x4 pass as the kernel runs it, every block scored and the early
  termination replayed afterwards; tests/test_cpu_mbanalyse.py holds it to the literal loop.
"""
import collections
import functools
import types

import numpy as np

import mbenc_cases as mc
import mbintra_cases as mi
import oracle_lib as orc

COST_MAX = 1 << 28
INTRA, T8, I16 = mi.INTRA, mi.T8, mi.I16
MB_LEFT, MB_TOP, MB_TOPRIGHT, MB_TOPLEFT = mi.MB_LEFT, mi.MB_TOP, mi.MB_TOPRIGHT, mi.MB_TOPLEFT
FENC, FDEC, OY, A = mi.FENC, mi.FDEC, mi.OY, mi.A
PIXEL_16x16, PIXEL_8x16, PIXEL_8x8, PIXEL_4x4 = 0, 2, 3, 6          # common/pixel.h
SLICE_I, SLICE_P, SLICE_B = 0, 1, 2

# the reference's tables (tests/golden/mbanalyse_tables.json pins them)
LAMBDA_TAB = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14,
              16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91, 102, 114, 128, 144, 161, 181, 203, 228, 256,
              287, 323, 362, 406, 456, 512, 575, 645, 724, 813, 912, 1024, 1149, 1290, 1448, 1625, 1825, 2048, 2299, 2580,
              2896)
I16x16_MODE_AVAILABLE = ((6, -1, -1, -1, -1), (4, 1, -1, -1, -1), (5, 0, -1, -1, -1), (0, 1, 2, -1, -1), (0, 1, 2, 3, -1))
CHROMA_MODE_AVAILABLE = ((6, -1, -1, -1, -1), (4, 1, -1, -1, -1), (5, 2, -1, -1, -1), (2, 1, 0, -1, -1), (2, 1, 0, 3, -1))
I4x4_MODE_AVAILABLE = ((11, -1, -1, -1, -1, -1, -1, -1, -1, -1), (9, 1, 8, -1, -1, -1, -1, -1, -1, -1),
                       (10, 0, 3, 7, -1, -1, -1, -1, -1, -1), (2, 1, 0, 3, 7, 8, -1, -1, -1, -1),
                       (2, 1, 0, 3, 4, 5, 6, 7, 8, -1))
I8x8_MODE_AVAILABLE = I4x4_MODE_AVAILABLE
INTRA_ANALYSIS_SHORTCUT = (((8, -1, -1, -1, -1), (3, 7, -1, -1, -1)), ((4, 6, 8, -1, -1), (3, 4, 5, 7, -1)))
I16x16_THRESH_LUT = (2, 2, 2, 3, 3, 4, 4, 4, 4, 4, 4)
I8x8_THRESH = (4, 4, 4, 5, 5, 5, 6, 6, 6, 6, 6)
COST_DIV_FIX8 = (1024, 512, 341)
MB_B_COST = {"i4": 9, "i8": 9, "i16": 9}                            # i_mb_b_cost_table[I_4x4 / I_8x8 / I_16x16]
PRED_MODE16x16_FIX = (0, 1, 2, 3, 2, 2, 2)
CHROMA_PRED_MODE_FIX = (0, 1, 2, 3, 0, 0, 0)
UE_SIZE = (1, 3, 3, 5)                                              # bs_size_ue( 0 .. 3 )


def avail_idx(n):
    """predict_*_mode_available, analyse.c:530-558"""
    idx = n & (MB_TOP | MB_LEFT | MB_TOPLEFT)
    return 4 if idx == (MB_TOP | MB_LEFT | MB_TOPLEFT) else idx & (MB_TOP | MB_LEFT)


def fix4(m):
    """x264_mb_pred_mode4x4_fix( m ), predict.h:84-92"""
    return -1 if m < 0 else 2 if m > 8 else m


def predict_intra4x4_mode(ma, mb):
    """x264_mb_predict_intra4x4_mode, macroblock.h:419-431"""
    m = min(fix4(ma), fix4(mb))
    return 2 if m < 0 else m


def cached_modes(cache, nm, idx):
    """(left, top) of intra4x4_pred_mode around block idx: the pass' own blocks, or the neighbour
    macroblocks' (nm: [0..3] left rows, [4..7] top columns)"""
    bx, by = mi.block_xy(idx)
    inv = {mi.block_xy(i): i for i in range(16)}
    left = cache[inv[bx - 1, by]] if bx else nm[by]
    top = cache[inv[bx, by - 1]] if by else nm[4 + bx]
    return int(left), int(top)


# ------------------------------------------------------------------ trial encodes
def trial_i4x4(bd, T, qp, mode, idx, fenc, fdec):
    """x264_mb_encode_i4x4 (encoder/macroblock.h:132-166) of block idx into fdec"""
    f = lambda name: orc.fn(bd, name)
    bx, by = mi.block_xy(idx)
    off = OY + 4 * bx + 4 * by * FDEC
    dct = np.zeros(16, orc.coef_dtype(bd))
    mi.predict(bd, "4x4", mode, fdec, off)
    f("sub4x4_dct")(A(dct), A(fenc, 4 * bx + 4 * by * FENC), A(fdec, off))
    if f("quant_4x4")(A(dct), A(T.q4m[mi.CQM_4IY][qp]), A(T.q4b[mi.CQM_4IY][qp])):
        f("dequant_4x4")(A(dct), A(T.dq4[mi.CQM_4IY]), qp)
        f("add4x4_idct")(A(fdec, off), A(dct))


def put_pred8x8(bd, mode, edge, fdec, off):
    """predict_8x8[mode]( p_dst, edge ), the DC variants from predict.c:700-715"""
    if mode <= 8:
        blk = orc.predict_8x8(bd, mode, edge)
    elif mode == 9:
        blk = (sum(int(v) for v in edge[7:15]) + 4) >> 3
    elif mode == 10:
        blk = (sum(int(v) for v in edge[16:24]) + 4) >> 3
    else:
        blk = 1 << (bd - 1)
    mi._put(fdec, off, 8, 8, blk)


def trial_i8x8(bd, T, qp, mode, idx, edge, fenc, fdec):
    """x264_mb_encode_i8x8 (encoder/macroblock.h:168-213) of block idx with the edge given"""
    f = lambda name: orc.fn(bd, name)
    x, y = idx & 1, idx >> 1
    off = OY + 8 * x + 8 * y * FDEC
    dct = np.zeros(64, orc.coef_dtype(bd))
    put_pred8x8(bd, mode, edge, fdec, off)
    f("sub8x8_dct8")(A(dct), A(fenc, 8 * x + 8 * y * FENC), A(fdec, off))
    if f("quant_8x8")(A(dct), A(T.q8m[mi.CQM_8IY][qp]), A(T.q8b[mi.CQM_8IY][qp])):
        f("dequant_8x8")(A(dct), A(T.dq8[mi.CQM_8IY]), qp)
        f("add8x8_idct8")(A(fdec, off), A(dct))


# ------------------------------------------------------------------ single blocks (analyse.c:759-835, 877-961)
def i4x4_block(bd, idx, n4, i_pred_mode, lam, fenc, fdec, cnt):
    """one iteration of the I_4x4 loop up to `i_cost += ...`: (i_best, mode)"""
    bx, by = mi.block_xy(idx)
    off, foff = OY + 4 * bx + 4 * by * FDEC, 4 * bx + 4 * by * FENC
    i_best = COST_MAX
    best = None
    predict_mode = list(I4x4_MODE_AVAILABLE[avail_idx(n4)])
    if (n4 & (MB_TOPRIGHT | MB_TOP)) == MB_TOP:
        fdec[off + 4 - FDEC:off + 8 - FDEC] = fdec[off + 3 - FDEC]      # :886-888
        cnt["i4_topright_emulated"] += 1
    if predict_mode[5] >= 0:
        satd = [int(v) for v in orc.intra_x3(bd, 0, 2, fenc, foff, fdec, off)]
        favor_vertical = satd[1] > satd[0]
        cnt["i4_favor_tie"] += satd[1] == satd[0]
        if i_pred_mode < 3:
            satd[i_pred_mode] -= 3 * lam
        i_best, best = satd[2], 2
        if satd[1] < i_best:
            i_best, best = satd[1], 1
        if satd[0] < i_best:
            i_best, best = satd[0], 0
        cnt["i4_x3", int(predict_mode[8] >= 0), int(favor_vertical)] += 1
        predict_mode = list(INTRA_ANALYSIS_SHORTCUT[predict_mode[8] >= 0][favor_vertical])
        x3_best = best
    else:
        x3_best = None
    if i_best > 0:
        for i_mode in predict_mode:
            if i_mode < 0:
                break
            mi.predict(bd, "4x4", i_mode, fdec, off)
            i_satd = orc.cmp(bd, "satd", PIXEL_4x4, fenc, foff, FENC, fdec, off, FDEC)
            if i_pred_mode == fix4(i_mode):
                i_satd -= lam * 3
                cnt["i4_pred_bonus"] += 1
                cnt["i4_bonus_satd", mc._side(i_satd, 0)] += 1
                if i_satd <= 0:
                    i_best, best = i_satd, i_mode
                    cnt["i4_le0_break"] += 1
                    break
            if i_satd < i_best:
                i_best, best = i_satd, i_mode
    else:
        cnt["i4_best_gate_false"] += 1
    if x3_best is not None and best != x3_best:
        cnt["i4_shortcut_wins"] += 1
    return i_best, best


def i8x8_block(bd, idx, n8, i_pred_mode, lam, fenc, fdec, cnt):
    """one iteration of the I_8x8 loop up to `i_cost += ...`: (i_best, mode, edge)"""
    x, y = idx & 1, idx >> 1
    off, foff = OY + 8 * x + 8 * y * FDEC, 8 * x + 8 * y * FENC
    i_best = COST_MAX
    best = None
    predict_mode = list(I8x8_MODE_AVAILABLE[avail_idx(n8)])
    edge = orc.predict_8x8_filter(bd, fdec, off, n8, 15)
    x3_best = None
    if predict_mode[5] >= 0:
        satd = [int(v) for v in orc.intra_x3(bd, 4, 3, fenc, foff, edge, 0)]
        favor_vertical = satd[1] > satd[0]
        cnt["i8_favor_tie"] += satd[1] == satd[0]
        if i_pred_mode < 3:
            satd[i_pred_mode] -= 3 * lam
        for i in (2, 1, 0):
            if satd[i] < i_best:
                i_best, best = satd[i], i
        cnt["i8_x3", int(predict_mode[8] >= 0), int(favor_vertical)] += 1
        predict_mode = list(INTRA_ANALYSIS_SHORTCUT[predict_mode[8] >= 0][favor_vertical])
        x3_best = best
    for i_mode in predict_mode:
        if i_mode < 0:
            break
        cnt["i8_best", mc._side(i_best, 0)] += 1
        if not i_best >= 0:
            cnt["i8_best_guard_stop"] += 1
            break
        put_pred8x8(bd, i_mode, edge, fdec, off)
        i_satd = orc.sa8d(bd, PIXEL_8x8, fdec, off, FDEC, fenc, foff, FENC)
        if i_pred_mode == fix4(i_mode):
            i_satd -= 3 * lam
            cnt["i8_pred_bonus"] += 1
        if i_satd < i_best:
            i_best, best = i_satd, i_mode
    if x3_best is not None and best != x3_best:
        cnt["i8_shortcut_wins"] += 1
    return i_best, best, edge


# ------------------------------------------------------------------ mb_analyse_intra_chroma, :615-664
def analyse_chroma(bd, cf, lam, nb, fenc_c, fdec_c, cnt):
    """(i_satd_chroma, i_predict8x8chroma)"""
    kind, ikind, pix = ("8x16c", 2, PIXEL_8x16) if cf == 2 else ("8x8c", 1, PIXEL_8x8)
    predict_mode = CHROMA_MODE_AVAILABLE[avail_idx(nb)]
    i_satd_chroma, best = COST_MAX, 0
    if predict_mode[3] >= 0:
        satdu = [int(v) for v in orc.intra_x3(bd, ikind, 2, fenc_c, 0, fdec_c, OY)] + [0]
        satdv = [int(v) for v in orc.intra_x3(bd, ikind, 2, fenc_c, 8, fdec_c, OY + 16)] + [0]
        mi.predict(bd, kind, 3, fdec_c, OY)
        mi.predict(bd, kind, 3, fdec_c, OY + 16)
        satdu[3] = orc.cmp(bd, "satd", pix, fenc_c, 0, FENC, fdec_c, OY, FDEC)
        satdv[3] = orc.cmp(bd, "satd", pix, fenc_c, 8, FENC, fdec_c, OY + 16, FDEC)
        cnt["chroma_x3"] += 1
        for i_mode in predict_mode:
            if i_mode < 0:
                break
            i_satd = satdu[i_mode] + satdv[i_mode] + lam * UE_SIZE[i_mode]
            cnt["chroma_x3_cost", mc._side(i_satd, i_satd_chroma)] += 1
            if i_satd < i_satd_chroma:
                i_satd_chroma, best = i_satd, i_mode
    else:
        cnt["chroma_list"] += 1
        for i_mode in predict_mode:
            if i_mode < 0:
                break
            mi.predict(bd, kind, i_mode, fdec_c, OY)
            mi.predict(bd, kind, i_mode, fdec_c, OY + 16)
            i_satd = (orc.cmp(bd, "satd", pix, fenc_c, 0, FENC, fdec_c, OY, FDEC) +
                      orc.cmp(bd, "satd", pix, fenc_c, 8, FENC, fdec_c, OY + 16, FDEC) +
                      lam * UE_SIZE[CHROMA_PRED_MODE_FIX[i_mode]])
            cnt["chroma_list_cost", mc._side(i_satd, i_satd_chroma)] += 1
            if i_satd < i_satd_chroma:
                i_satd_chroma, best = i_satd, i_mode
    return i_satd_chroma, best


# ------------------------------------------------------------------ mb_analyse_intra, :668-980
def i4x4_pass(bd, T, qp, lam, nb, nm, i_cost, i_satd_thresh, fenc, fdec, cnt):
    """:877-978, the literal loop: (i_satd_i4x4, modes[16], idx reached, per-block costs)"""
    cache = [2] * 16
    costs = []
    idx = 0
    while True:
        n4 = mi.neighbour4(idx, nb)
        i_pred_mode = predict_intra4x4_mode(*cached_modes(cache, nm, idx))
        i_best, mode = i4x4_block(bd, idx, n4, i_pred_mode, lam, fenc, fdec, cnt)
        cache[idx] = mode
        costs.append(i_best + 3 * lam)
        i_cost += i_best + 3 * lam
        cnt["i4_cost", mc._side(i_cost, i_satd_thresh), int(idx == 15)] += 1
        if i_cost > i_satd_thresh or idx == 15:
            break
        trial_i4x4(bd, T, qp, mode, idx, fenc, fdec)
        idx += 1
    return (i_cost if idx == 15 else COST_MAX), cache, idx, costs


def i4x4_prefix_form(bd, T, qp, lam, nb, nm, i_cost, i_satd_thresh, fenc, fdec):
    """the I_4x4 pass as the kernel runs it: all sixteen blocks scored and encoded, then the
    early termination replayed over the costs: (i_satd_i4x4, modes[16], idx reached)"""
    cnt = collections.Counter()
    cache = [2] * 16
    costs = []
    for idx in range(16):
        n4 = mi.neighbour4(idx, nb)
        i_pred_mode = predict_intra4x4_mode(*cached_modes(cache, nm, idx))
        i_best, mode = i4x4_block(bd, idx, n4, i_pred_mode, lam, fenc, fdec, cnt)
        cache[idx] = mode
        costs.append(i_best + 3 * lam)
        trial_i4x4(bd, T, qp, mode, idx, fenc, fdec)
    idx = 0
    while True:
        i_cost += costs[idx]
        if i_cost > i_satd_thresh or idx == 15:
            break
        idx += 1
    return (i_cost if idx == 15 else COST_MAX), cache, idx


def analyse_intra(bd, T, cfg, qp, lam, nb, nm, i_satd_inter, b_fast_intra, fenc, fdec, cnt):
    """mb_analyse_intra: a namespace with i_satd_i16x16 / i8x8 / i4x4, i_predict16x16,
    i_predict8x8[4], i_predict4x4[16]"""
    a = types.SimpleNamespace(i_satd_i16x16=COST_MAX, i_satd_i8x8=COST_MAX, i_satd_i4x4=COST_MAX, i_predict16x16=0,
                              i_predict8x8=[2] * 4, i_predict4x4=[2] * 16, x3=0)
    b_slice = cfg.slice_type == SLICE_B
    # I_16x16, :690-742
    predict_mode = I16x16_MODE_AVAILABLE[avail_idx(nb)]
    i16x16_thresh = (I16x16_THRESH_LUT[cfg.subme] * i_satd_inter) >> 1 if b_fast_intra else COST_MAX
    if predict_mode[3] >= 0:
        d = [int(v) for v in orc.intra_x3(bd, 3, 2, fenc, 0, fdec, OY)]
        for m in range(3):
            d[m] += lam * UE_SIZE[m]
            if d[m] < a.i_satd_i16x16:
                a.i_satd_i16x16, a.i_predict16x16 = d[m], m
        cnt["i16_x3_cost", mc._side(a.i_satd_i16x16, i16x16_thresh)] += 1
        a.x3 = a.i_satd_i16x16
        if a.i_satd_i16x16 <= i16x16_thresh:
            mi.predict(bd, "16x16", 3, fdec, OY)
            p = orc.cmp(bd, "satd", PIXEL_16x16, fenc, 0, FENC, fdec, OY, FDEC) + lam * UE_SIZE[3]
            cnt["i16_plane_evaluated"] += 1
            cnt["i16_plane_cost", mc._side(p, a.i_satd_i16x16)] += 1
            if p < a.i_satd_i16x16:
                a.i_satd_i16x16, a.i_predict16x16 = p, 3
        else:
            cnt["i16_plane_skipped"] += 1
    else:
        for i_mode in predict_mode:
            if i_mode < 0:
                break
            mi.predict(bd, "16x16", i_mode, fdec, OY)
            i_satd = orc.cmp(bd, "satd", PIXEL_16x16, fenc, 0, FENC, fdec, OY, FDEC) + lam * UE_SIZE[PRED_MODE16x16_FIX[i_mode]]
            if i_satd < a.i_satd_i16x16:
                a.i_satd_i16x16, a.i_predict16x16 = i_satd, i_mode
    if b_slice:
        a.i_satd_i16x16 += lam * MB_B_COST["i16"]
    cnt["i16_cost", mc._side(a.i_satd_i16x16, i16x16_thresh)] += 1
    if a.i_satd_i16x16 > i16x16_thresh:
        cnt["return_740"] += 1
        return a
    # I_8x8, :746-862
    if cfg.b_i8x8:
        i_satd_thresh = min(i_satd_inter, a.i_satd_i16x16)
        i_cost = lam * 4
        if b_slice:
            i_cost += lam * MB_B_COST["i8"]
        cache = [2] * 16
        idx = 0
        while True:
            n8 = mi.neighbour8(idx, nb)
            i_pred_mode = predict_intra4x4_mode(*cached_modes(cache, nm, 4 * idx))
            i_best, mode, edge = i8x8_block(bd, idx, n8, i_pred_mode, lam, fenc, fdec, cnt)
            a.i_predict8x8[idx] = mode
            i_cost += i_best + 3 * lam
            cnt["i8_cost", mc._side(i_cost, i_satd_thresh), int(idx == 3)] += 1
            if idx == 3 or i_cost > i_satd_thresh:
                break
            cache[4 * idx:4 * idx + 4] = [mode] * 4
            trial_i8x8(bd, T, qp, mode, idx, edge, fenc, fdec)
            idx += 1
        cnt["i8_loop_end", idx, int(i_cost > i_satd_thresh)] += 1
        if idx == 3:
            a.i_satd_i8x8 = i_cost
        else:
            a.i_satd_i8x8 = COST_MAX
            i_cost = (i_cost * COST_DIV_FIX8[idx]) >> 8
        cnt["i8_gate", mc._side(min(i_cost, a.i_satd_i16x16), (i_satd_inter * I8x8_THRESH[cfg.subme]) >> 2)] += 1
        if min(i_cost, a.i_satd_i16x16) > (i_satd_inter * I8x8_THRESH[cfg.subme]) >> 2:
            cnt["return_860"] += 1
            return a
    # I_4x4, :865-979
    if cfg.b_i4x4:
        i_cost = lam * (24 + 16)
        i_satd_thresh = min(i_satd_inter, a.i_satd_i16x16, a.i_satd_i8x8)
        if b_slice:
            i_cost += lam * MB_B_COST["i4"]
        a.i_satd_i4x4, a.i_predict4x4, idx, _ = i4x4_pass(bd, T, qp, lam, nb, nm, i_cost, i_satd_thresh, fenc, fdec, cnt)
        cnt["i4_loop_complete" if idx == 15 else "i4_loop_break"] += 1
    return a


def analyse_mb(bd, T, cf, cfg, qp, lam, nb, nm, satd_inter, b_fast_intra, fenc_y, fdec_y, fenc_c, fdec_c, cnt):
    """x264_macroblock_analyse's intra part for one try macroblock: (type 'i16' / 'i8' / 'i4' or None,
    modes[16], chroma mode, cost[4])"""
    i_satd_chroma, cmode = COST_MAX, 0
    if cfg.slice_type == SLICE_I:
        a = analyse_intra(bd, T, cfg, qp, lam, nb, nm, COST_MAX, b_fast_intra, fenc_y, fdec_y, cnt)
        i_cost, kind = a.i_satd_i16x16, "i16"
        cnt["type_i", "i4", mc._side(a.i_satd_i4x4, i_cost)] += 1
        if a.i_satd_i4x4 < i_cost:
            i_cost, kind = a.i_satd_i4x4, "i4"
        cnt["type_i", "i8", mc._side(a.i_satd_i8x8, i_cost)] += 1
        if a.i_satd_i8x8 < i_cost:
            i_cost, kind = a.i_satd_i8x8, "i8"
        chroma_first = False
    else:
        chroma_first = bool(cfg.b_chroma_me and cf)
        i_cost, kind = int(satd_inter), None
        if chroma_first:
            i_satd_chroma, cmode = analyse_chroma(bd, cf, lam, nb, fenc_c, fdec_c, cnt)
            a = analyse_intra(bd, T, cfg, qp, lam, nb, nm, i_cost - i_satd_chroma, b_fast_intra, fenc_y, fdec_y, cnt)
            a.i_satd_i16x16 += i_satd_chroma
            a.i_satd_i8x8 += i_satd_chroma
            a.i_satd_i4x4 += i_satd_chroma
        else:
            a = analyse_intra(bd, T, cfg, qp, lam, nb, nm, i_cost, b_fast_intra, fenc_y, fdec_y, cnt)
        cnt["type_pb", "i16", mc._side(a.i_satd_i16x16, i_cost)] += 1
        if a.i_satd_i16x16 < i_cost:
            i_cost, kind = a.i_satd_i16x16, "i16"
        cnt["type_pb", "i8", mc._side(a.i_satd_i8x8, i_cost)] += 1
        if a.i_satd_i8x8 < i_cost:
            i_cost, kind = a.i_satd_i8x8, "i8"
        cnt["type_pb", "i4", mc._side(a.i_satd_i4x4, i_cost)] += 1
        if a.i_satd_i4x4 < i_cost:
            i_cost, kind = a.i_satd_i4x4, "i4"
    if kind is not None and not chroma_first:                        # analyse_update_cache
        i_satd_chroma, cmode = analyse_chroma(bd, cf, lam, nb, fenc_c, fdec_c, cnt) if cf else (0, 0)
    if kind == "i16":
        modes = [a.i_predict16x16] + [2] * 15
    elif kind == "i8":
        modes = [a.i_predict8x8[i >> 2] for i in range(16)]
    else:
        modes = list(a.i_predict4x4)
    cnt["x3_of_last_mb"] = a.x3                                      # for make_case's "x3/2" rule: a note, no count
    return kind, modes, cmode, (a.i_satd_i16x16, a.i_satd_i8x8, a.i_satd_i4x4, i_satd_chroma)


# ------------------------------------------------------------------ frames
KIND_FLAGS = {"i4": INTRA, "i8": INTRA | T8, "i16": INTRA | I16}


def neighbour_modes(case, flags_now, pred_mode, mb, nb):
    """intra4x4_pred_mode of the left (rows) and top (columns) macroblocks as cache_load reads them"""
    nm = [-1] * 8
    for base, have, n, blocks in ((0, nb & MB_LEFT, mb - 1, (5, 7, 13, 15)), (4, nb & MB_TOP, mb - case.mbw, (10, 11, 14, 15))):
        if have:
            fl = int(flags_now[n])
            i4 = fl & INTRA and not fl & (T8 | I16)
            for k, b in enumerate(blocks):
                nm[base + k] = int(pred_mode[n][b]) if i4 else 2
    return nm


def encode(case, dec):
    """the outputs of (x264hip_*_mb_encode_inter on a P / B picture, then) x264hip_*_mb_analyse_intra
    for `case`: mbintra_cases.encode's outputs plus pred_mode, chroma_pred_mode, mb_flags_out,
    cost, tried / intra (bool per macroblock) and the branch counters"""
    bd, cf = case.bd, case.cf
    T = mc.tables(bd, case.cqm)
    if case.slice_type == SLICE_I:
        cd = orc.coef_dtype(bd)
        n = case.nmb
        out = types.SimpleNamespace(
            recon_y=case.pred_y.copy(), recon_c=case.pred_c.copy() if cf else None, level=np.zeros((n, 48, 16), cd),
            chroma_dc=np.zeros((n, 2, 8), cd), nnz=np.zeros((n, 48), np.uint8), cbp=np.zeros(n, np.int32),
            nz=np.zeros(n, np.int32), flags_out=np.zeros(n, np.uint8), counters=collections.Counter())
    else:
        out = mc.encode(case, dec)
    out.luma_dc = np.zeros((case.nmb, 16), orc.coef_dtype(bd))
    out.pred_mode = case.pred_mode.copy()
    out.chroma_pred_mode = case.chroma_pred_mode.copy()
    out.mb_flags_out = case.flags.copy()
    out.cost = np.zeros((case.nmb, 4), np.int32)
    out.intra = np.zeros(case.nmb, bool)
    out.x3 = [0] * case.nmb                                          # the I_16x16 cost before Plane (a list: no output)
    cnt = out.counters
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        tr = bool(case.try_intra[mb])
        if not tr and not fl & INTRA:
            continue
        qp = int(case.qp[mb])
        f, my, mx, nb, fenc_y, fenc_c, fdec_y, fdec_c = mi.mb_buffers(case, out.recon_y, out.recon_c, mb)
        modes, cmode = out.pred_mode[mb], int(out.chroma_pred_mode[mb])
        if tr:
            nm = neighbour_modes(case, out.mb_flags_out, out.pred_mode, mb, nb)
            kind, modes, cmode, cost = analyse_mb(bd, T, cf, case, qp, LAMBDA_TAB[qp], nb, nm, int(case.satd_inter[mb]),
                                                  bool(case.fast_intra[mb]), fenc_y, fdec_y, fenc_c, fdec_c, cnt)
            out.cost[mb] = cost
            out.x3[mb] = cnt.pop("x3_of_last_mb")
            cnt["decided", case.slice_type, kind] += 1
            if kind is None:
                continue
            fl = KIND_FLAGS[kind]
            out.mb_flags_out[mb] = fl
            out.pred_mode[mb] = modes
            if cf:
                out.chroma_pred_mode[mb] = cmode
            if kind == "i16":
                cnt["chosen16", modes[0]] += 1
            else:
                for i in range(0, 16, 4 if kind == "i8" else 1):
                    cnt["chosen" + kind[1:], modes[i]] += 1
            if cf:
                cnt["chosenc", cmode] += 1
            # the final encode starts from the neighbours alone (x264's i_skip_intra reuse gives the
            # same bytes: the trial and the final encode of a block see the same inputs)
            f, my, mx, nb, fenc_y, fenc_c, fdec_y, fdec_c = mi.mb_buffers(case, out.recon_y, out.recon_c, mb)
        out.intra[mb] = True
        o = mi.encode_mb(bd, T, cf, dec, fl, qp, int(case.qp_table[qp]), np.asarray(modes, np.int8), cmode, nb,
                         fenc_y, fdec_y, fenc_c, fdec_c, cnt)
        mi.put_back(case, out.recon_y, out.recon_c, f, my, mx, fdec_y, fdec_c)
        out.level[mb], out.chroma_dc[mb], out.nnz[mb], out.luma_dc[mb] = o.level, o.chroma_dc, o.nnz, o.luma_dc
        out.cbp[mb] = o.cbp_chroma << 4 | o.cbp_luma | o.nnz_ldc << 8 | o.nnz_dc[0] << 9 | o.nnz_dc[1] << 10
        if fl & T8:
            out.nz[mb] = sum(int(o.nnz[4 * i]) << i for i in range(4))
        else:
            out.nz[mb] = sum(int(o.nnz[i]) << i for i in range(16))
        out.flags_out[mb] = fl & 3
    return out


@functools.lru_cache(maxsize=None)
def expected(key, dec):
    """encode(make_case(*key), dec), computed once per process and shared; do not modify"""
    return encode(make_case(*key), dec)


# ------------------------------------------------------------------ inputs
SHAPES = ((1, 1, 1), (3, 1, 1), (1, 3, 1), (2, 2, 1), (5, 4, 2), (7, 3, 3))     # (mb_width, mb_height, frames)
FLAT_C, HGRAD, VGRAD, DIAG, STRIPES, TEX8, NOISE_C, KEEP = range(8)
QUIET, QUIET_HEAD, QUIET_RAMP = -1, -2, -3                                           # the boundary pictures' own, see make_case


def _content(rng, k, bd, h, w, qs):
    """one macroblock plane of content class k"""
    pm, scale = (1 << bd) - 1, 1 << (bd - 8)
    y, x = np.mgrid[0:h, 0:w]
    base = int(rng.integers(40, 200)) * scale
    if k == FLAT_C:
        v = np.full((h, w), base)
    elif k == HGRAD:
        v = base + int(rng.integers(-6, 7)) * scale * x
    elif k == VGRAD:
        v = base + int(rng.integers(-6, 7)) * scale * y
    elif k == DIAG:
        s = int(rng.choice([-1, 1]))
        v = base + int(rng.integers(2, 9)) * scale * ((x + s * y * int(rng.integers(1, 3))) // int(rng.integers(1, 4)))
    elif k == STRIPES:
        p = int(rng.integers(2, 6))
        v = base + int(rng.integers(20, 90)) * scale * ((((x if rng.random() < 0.5 else y) // p) & 1))
    elif k == TEX8:
        v = np.zeros((h, w))
        for by in range(0, h, 8):
            for bx in range(0, w, 8):
                a, b = rng.integers(-5, 6, 2)
                v[by:by + 8, bx:bx + 8] = int(rng.integers(40, 200)) * scale + scale * (a * x[:8, :8] + b * y[:8, :8])
    else:
        v = base + rng.normal(0, 30 * scale, (h, w))
    v = v + rng.normal(0, qs * rng.choice([0.0, 0.3, 1.0]), (h, w))
    return np.clip(np.rint(v), 0, pm)


@functools.lru_cache(maxsize=None)
def make_case(bd, cf, mbw, mbh, nframes, slice_type, cqm="flat", seed=0, b_i8x8=1, b_i4x4=1, b_chroma_me=0, subme=5,
              content=None, recipe=None):
    """mbintra_cases.make_case's inputs (an I picture: its all-intra case; P / B: its mixed case with
    the residual classes of mbenc_cases) plus: try_intra on most macroblocks, whose INTRA and type
    bits are cleared; fenc of two thirds of the try macroblocks replaced by a content class (flat,
    gradients, diagonal ramps, stripes, 8x8-structured texture, noise; a dither of up to a
    quantiser step); satd_inter drawn around the intra cost of a first pass that takes every
    macroblock as intra; fast_intra on a third of the P / B macroblocks.  content 'flat' /
    'checker': one whole picture of it at qp 0 and QP_MAX_SPEC alternating.
    recipe (qp, class, amp, density, rule, offset): a boundary picture at one qp, "grey" being mid grey
    + offset (with an offset the _128 predictions of a picture's first macroblock miss by a known
    amount, which is what lets I_4x4's forty lambdas tie with I_16x16).  Class QUIET: grey with
    single pixels of up to +-amp on density/16 of the positions; the costs are a few lambdas plus
    a few small SATDs, so that they tie with each other.  QUIET_HEAD: mid grey with noise of +-density
    inside the first `amp` 4x4 blocks only, so that the blocks after them cost nothing and a running
    cost stays on a threshold it has reached.  QUIET_RAMP: grey + ((amp * x + density * y) >> 3) over
    the picture with a speck of noise: Plane predicts it about as well as V / H / DC.  Otherwise a content class of _content, and satd_inter
    is set from the first pass by `rule` to put a threshold of the reference on a cost: "c", "c+1",
    "c-1" (the least intra cost), "i16/2" (2 * satd_inter = i_satd_i16x16, the fast-intra gate, with
    fast_intra set), "x3/2" (the same with the cost before Plane is tried), "i8" ((5 * satd_inter) >> 2 = min(I_8x8, I_16x16), :858), "max" (nothing stops)."""
    base = mi.make_case(bd, cf, mbw, mbh, nframes, cqm, seed, slice_type == SLICE_I)
    rng = np.random.default_rng([bd, cf, mbw, mbh, nframes, slice_type, seed, 0xa11a])
    case = types.SimpleNamespace(**vars(base))
    n, pm, crows = base.nmb, (1 << bd) - 1, base.chroma_rows
    case.slice_type, case.b_i8x8, case.b_i4x4, case.b_chroma_me, case.subme = slice_type, b_i8x8, b_i4x4, b_chroma_me, subme
    flags = base.flags.copy()
    qp = base.qp.copy()
    fenc_y = base.fenc_y.copy()
    fenc_c = base.fenc_c.copy() if cf else None
    try_intra = np.zeros(n, np.uint8)
    for mb in range(n):
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        given = bool(flags[mb] & INTRA)
        t = rng.random() < (0.8 if slice_type == SLICE_I else 0.7)
        if slice_type != SLICE_I and given:
            t = False
        if n <= 4:
            t = not given if slice_type != SLICE_I else mb != 1 or n == 1
        if content or (recipe and slice_type != SLICE_I):
            t = not given if recipe else True
        try_intra[mb] = t
        ys, cs, xs = slice(16 * my, 16 * my + 16), slice(crows * my, crows * my + crows), slice(16 * mx, 16 * mx + 16)
        if recipe:                                                   # the given macroblocks too
            q, klass, amp, density = recipe[:4]
            qp[mb] = q
            grey = (128 << (bd - 8)) + recipe[5]
            quiet = lambda h, w: grey + rng.integers(-amp, amp + 1, (h, w)) * (rng.integers(0, 16, (h, w)) < density)
            if klass == QUIET_HEAD:                                  # noise inside the first 4x4 blocks only
                blk = np.full((16, 16), grey)
                for idx in range(amp):
                    bx, by = mi.block_xy(idx)
                    blk[4 * by:4 * by + 3, 4 * bx:4 * bx + 3] += rng.integers(-density, density + 1, (3, 3))
                fenc_y[f, ys, xs] = blk
            elif klass == QUIET_RAMP:                                # a faint ramp across the picture and a speck of noise
                yy, xx = np.mgrid[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
                fenc_y[f, ys, xs] = grey + ((amp * xx + density * yy) >> 3) + rng.integers(-1, 2, (16, 16)) * (
                    rng.integers(0, 16, (16, 16)) < 1)
            else:
                fenc_y[f, ys, xs] = quiet(16, 16) if klass == QUIET else _content(rng, klass, bd, 16, 16, 0.0)
            if cf:
                fenc_c[f, cs, xs] = quiet(crows, 16) if klass in (QUIET, QUIET_HEAD, QUIET_RAMP) else grey
        if not t:
            continue
        flags[mb] &= ~np.uint8(INTRA | T8 | I16 | mc.SKIP)
        if recipe:
            continue
        if content:
            qp[mb] = 0 if (mx + my + f) & 1 else mc.qp_max_spec(bd)
            yy, xx = np.mgrid[0:16, 0:16]
            fenc_y[f, ys, xs] = ((yy + xx) & 1) * pm if content == "checker" else 128 << (bd - 8)
            if cf:
                cy, cx = np.mgrid[0:crows, 0:16]
                fenc_c[f, cs, xs] = ((cy + (cx >> 1)) & 1) * pm if content == "checker" else 128 << (bd - 8)
            continue
        k = int(rng.choice([FLAT_C, HGRAD, VGRAD, DIAG, DIAG, STRIPES, TEX8, TEX8, NOISE_C, KEEP, KEEP, KEEP]))
        if k != KEEP and base.klass[mb] != mc.CHECKER:
            qs = mc._qstep(int(qp[mb]))
            fenc_y[f, ys, xs] = _content(rng, k, bd, 16, 16, qs)
            if cf:
                kc = int(rng.choice([FLAT_C, HGRAD, VGRAD, DIAG, NOISE_C]))
                fenc_c[f, cs, xs][:, 0::2] = _content(rng, kc, bd, crows, 8, qs)
                fenc_c[f, cs, xs][:, 1::2] = _content(rng, kc, bd, crows, 8, qs)
    case.flags, case.qp, case.try_intra = flags, qp, try_intra
    case.fenc_y, case.fenc_c = fenc_y, fenc_c
    case.fast_intra = np.zeros(n, np.uint8)
    case.satd_inter = np.zeros(n, np.int32)
    case.nmb = n
    case.key = (bd, cf, mbw, mbh, nframes, slice_type, cqm, seed, b_i8x8, b_i4x4, b_chroma_me, subme, content)
    if recipe:
        case.key += (recipe,)
    if slice_type != SLICE_I:
        # a first pass with every try macroblock taken as an I picture's gives the scale of its costs
        probe = types.SimpleNamespace(**vars(case))
        probe.slice_type = SLICE_I
        probe.pred_y, probe.pred_c = mc.encode(case, 1).recon_y, mc.encode(case, 1).recon_c if cf else None
        first = encode(probe, 1)
        case.fast_intra = (rng.random(n) < 1 / 3).astype(np.uint8)
        for mb in range(n):
            if try_intra[mb]:
                c = int(min(first.cost[mb][:3]))
                u = rng.random()
                case.satd_inter[mb] = c if u < 0.1 else c + 1 if u < 0.2 else max(0, int(c * rng.uniform(0.3, 2.5)))
                if recipe:
                    i16, i8 = int(first.cost[mb][0]), int(first.cost[mb][1])
                    rule = recipe[4]
                    case.fast_intra[mb] = rule in ("i16/2", "x3/2")
                    case.satd_inter[mb] = {"c": c, "c+1": c + 1, "c-1": max(0, c - 1), "i16/2": i16 >> 1, "x3/2": first.x3[mb] >> 1,
                                           "i8": -(-4 * min(i8, i16) // 5), "max": COST_MAX - 1}[rule]
    return case


def case_keys(bd, cf, slice_type, **kw):
    """the case list of one (bit depth, chroma format, slice type): every shape"""
    return [make_key(bd, cf, w, h, n, slice_type, **kw) for w, h, n in SHAPES]


def make_key(bd, cf, mbw, mbh, nframes, slice_type, cqm="flat", seed=0, b_i8x8=1, b_i4x4=1, b_chroma_me=0, subme=5,
             content=None):
    return (bd, cf, mbw, mbh, nframes, slice_type, cqm, seed, b_i8x8, b_i4x4, b_chroma_me, subme, content)


# The boundary pictures: (what is pinned, the counter that says the picture is on the bound, the picture at
# 8 bit, the picture at 10 bit), a picture being (chroma format, mbw, mbh, slice type, seed, options,
# recipe).  On each, at its depth, the checker and the named comparison flipped at its boundary
# (tests/mutants.py) give other bytes.  The costs depend on the reconstruction around a macroblock
# and so on the depth's quantiser: where the 8-bit parameters miss the bound at 10 bit the 10-bit
# picture has parameters of its own, found by the same search.
def _p(cf, w, h, st, seed, recipe, **kw):
    return (cf, w, h, st, seed, kw, recipe)


BOUNDARY = (
    ("I_8x8 loop entered with i_best = 0 (the guard is `i_best >= 0`, not `> 0`)", ("i8_best", "at"),
     _p(0, 3, 2, 0, 753, (17, 3, 1, 2, "c-1", 0)), _p(1, 2, 2, 0, 446, (0, 2, 3, 2, "c-1", 0))),
    ("chroma x3: two modes tie, the first evaluated stays", ("chroma_x3_cost", "at"),
     _p(1, 2, 2, 0, 305, (20, -2, 5, 3, "c", 0), b_i8x8=0, b_chroma_me=1), _p(1, 3, 2, 1, 33, (20, -2, 7, 3, "max", 0), b_i8x8=0)),
    ("chroma x3 tie at 4:2:2", ("chroma_x3_cost", "at"),
     _p(2, 3, 2, 1, 377, (33, 6, 3, 4, "c-1", 0), b_i8x8=0), _p(2, 3, 2, 1, 593, (17, -2, 7, 2, "c+1", 0))),
    ("chroma mode list: two modes tie", ("chroma_list_cost", "at"),
     _p(1, 2, 2, 0, 924, (10, -1, 2, 2, "i16/2", 0)), _p(1, 3, 2, 1, 983, (17, -2, 7, 2, "c+1", 0))),
    ("I_4x4 running cost = the threshold: goes on", ("i4_cost", "at", 0),
     _p(0, 1, 1, 1, 525, (10, 1, 2, 8, "c", 0), b_i8x8=0), _p(0, 1, 1, 1, 525, (10, 1, 2, 8, "c", 0), b_i8x8=0)),
    ("I_4x4 running cost = the threshold, 4:2:0", ("i4_cost", "at", 0),
     _p(1, 2, 2, 1, 956, (20, 2, 0, 1, "c", 0), b_i8x8=0), _p(1, 2, 2, 1, 956, (20, 2, 0, 1, "c", 0), b_i8x8=0)),
    ("i_satd_i16x16 = i16x16_thresh after I_16x16: not returned", ("i16_cost", "at"),
     _p(0, 3, 2, 1, 795, (24, 1, 3, 4, "i16/2", 0)), _p(0, 3, 2, 1, 795, (24, 1, 3, 4, "i16/2", 0))),
    ("i_satd_i16x16 = i16x16_thresh before Plane: Plane still evaluated", ("i16_x3_cost", "at"),
     _p(0, 3, 2, 2, 470, (24, 6, 2, 1, "i16/2", 0)), _p(1, 3, 2, 2, 909, (0, -3, 5, -1, "x3/2", 0))),
    ("i_satd_i16x16 = i16x16_thresh, one macroblock", ("i16_cost", "at"),
     _p(0, 1, 1, 1, 329, (17, 2, 2, 2, "i16/2", 0), b_i8x8=0), _p(0, 1, 1, 1, 329, (17, 2, 2, 2, "i16/2", 0), b_i8x8=0)),
    ("min(I_8x8, I_16x16) = the I8x8_THRESH bound: I_4x4 still tried", ("i8_gate", "at"),
     _p(0, 1, 1, 1, 112, (17, 5, 1, 4, "i8", 0)), _p(1, 1, 1, 1, 31, (10, 5, 1, 2, "i8", 0))),
    ("Plane cost = the best of V / H / DC: not taken", ("i16_plane_cost", "at"),
     _p(0, 2, 2, 0, 81295, (17, -3, 0, 5, "max", 0)), _p(0, 3, 2, 0, 42954, (22, -3, 0, 3, "max", 0))),
    ("I picture: I_4x4 cost = I_16x16 cost, I_16x16 stays", ("type_i", "i4", "at"),
     _p(0, 1, 1, 0, 18581, (27, -2, 6, 2, "max", 3), b_i8x8=0), _p(0, 2, 1, 0, 59052, (27, -2, 15, 3, "max", 3), b_i8x8=0)),
    ("I picture: I_8x8 cost = the least so far, which stays", ("type_i", "i8", "at"),
     _p(1, 2, 2, 0, 337, (17, -1, 2, 8, "i16/2", 0)), _p(0, 3, 2, 0, 988, (20, -2, 8, 3, "i8", 0), b_chroma_me=1)),
    ("I_8x8 running cost = the threshold: goes on", ("i8_cost", "at", 0),
     _p(2, 2, 2, 0, 302, (17, -1, 1, 2, "max", 0)), _p(1, 3, 2, 0, 691, (10, -2, 4, 2, "max", 0))),
)


def boundary_key(bd, row):
    cf, w, h, st, seed, kw, recipe = BOUNDARY[row][2 if bd == 8 else 3]
    return make_key(bd, cf, w, h, 1, st, seed=seed, **kw) + (recipe,)


def boundary_keys():
    return [boundary_key(bd, row) for bd in (8, 10) for row in range(len(BOUNDARY))]


OPTIONS = (dict(b_i8x8=0), dict(b_i4x4=0), dict(cqm="jvt"), dict(b_chroma_me=1), dict(subme=2))
KEY_FIELDS = ("bd", "cf", "mbw", "mbh", "nframes", "slice_type", "cqm", "seed", "b_i8x8", "b_i4x4", "b_chroma_me", "subme",
              "content")
GPU_GROUPS = ("shapes", "options", "content", "noise", "boundary")


def gpu_keys(group=None, **where):
    """every (key, dec) tests/test_gpu_mbanalyse.py compares with the device byte for byte, which is
    the list the boundary mutants of tests/test_cpu_mutants.py are held to.  group: one of GPU_GROUPS
    (one test function each); where: fields of the key (KEY_FIELDS) or dec, the parametrised case."""
    both = (8, 10)
    keys = {"shapes": [(k, dec) for bd in both for cf in (0, 1, 2) for st in (0, 1, 2) for k in case_keys(bd, cf, st)
                       for dec in (0, 1)],
            "options": [(make_key(bd, cf, 5, 4, 2, st, **kw), 1) for bd in both for kw in OPTIONS
                        for cf, st in ((1, 1), (1, 0), (2, 2))],
            "content": [(make_key(bd, cf, w, h, 1, st, content=c), 1) for bd in both for c in ("flat", "checker")
                        for cf, w, h, st in ((1, 5, 4, 0), (2, 3, 2, 1))],
            "noise": [(make_key(bd, 1, 5, 4, 2, st), 1) for bd in both for st in (0, 1)],
            "boundary": [(k, 1) for k in boundary_keys()]}
    keys = [kd for g in GPU_GROUPS if group in (None, g) for kd in keys[g]]
    pick = lambda kd, n: kd[1] if n == "dec" else kd[0][KEY_FIELDS.index(n)]
    return [kd for kd in keys if all(pick(kd, n) == v for n, v in where.items())]


def key_size(kd):
    """macroblocks of a gpu_keys() entry: what its expected() costs"""
    return kd[0][2] * kd[0][3] * kd[0][4]
