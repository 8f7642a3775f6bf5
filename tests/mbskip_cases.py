"""P_SKIP / B_SKIP restated per macroblock from the reference's C, and the inputs of
tests/test_cpu_mbskip.py and tests/test_gpu_mbskip.py (include/x264hip_mbskip.h).  No GPU code.

* pskip_mv: x264_mb_predict_mv_pskip (common/mvpred.c:129-181) from the motion field; and
  pskip_mv_scan8, the same through a literal scan8 cache as x264_macroblock_cache_load fills it.
* probe_literal: x264_macroblock_probe_skip (encoder/macroblock.c:985-1139) as the C has it, early
  returns and all, with a counter per branch.  Every transform, quantiser, scan, score and ssd is
  the oracle's (tests/oracle_lib.py), called on FENC / FDEC-layout buffers; the prediction is
  tests/mc_cases.py's mc_luma / mc_chroma / mc_weight at the vector clipped to mc_cases.mv_limits.
* probe_predicate: the header's order-free form of the same test on tests/numpy_ref.py's matrix
  transforms.
* skip_convert: macroblock.c:953-971.
* make_case / make_field / make_convert_case: the seeded inputs.

x264_lambda2_tab is tests/golden/mbenc_tables.json's (through mbenc_cases)."""
import collections
import functools
import types

import numpy as np

import mbenc_cases as mbc
import mc_cases as mcc
import numpy_ref as nr
import oracle_lib as orc
import weightp_cases as wc

LAMBDA2 = mbc.LAMBDA2
INTRA, T8, D16, SKIP = mbc.INTRA, mbc.T8, mbc.D16, mbc.SKIP
CQM_4PY, CQM_4PC = mbc.CQM_4PY, mbc.CQM_4PC
FENC, FDEC = mbc.FENC, mbc.FDEC
PIXEL_8x16, PIXEL_8x8 = mbc.PIXEL_8x16, mbc.PIXEL_8x8
A = orc._addr
SHAPES = ((1, 1, 1), (3, 1, 1), (2, 2, 1), (5, 4, 2), (24, 14, 2))     # (mb_width, mb_height, frames)
LEGS = ("p", "pw", "b")                        # the P leg, the P leg weighted in all three planes, the B leg
WEIGHTS = ((57, 6, 9), (70, 6, -11), (61, 6, 5))                       # (scale, denom, offset) of Y, U, V
SCAN8_0 = 4 + 1 * 8


# ------------------------------------------------------------------ x264_mb_predict_mv_pskip
def _median(a, b, c):
    return max(min(a, b), min(max(a, b), c))


def _predict_16x16(ra, ma, rb, mb, rc, mc, i_ref=0):
    """mvpred.c:143-162 once the three neighbours are chosen"""
    cnt = (ra == i_ref) + (rb == i_ref) + (rc == i_ref)
    if cnt == 1:
        return ma if ra == i_ref else mb if rb == i_ref else mc
    if cnt == 0 and rb == -2 and rc == -2 and ra != -2:
        return ma
    return (_median(ma[0], mb[0], mc[0]), _median(ma[1], mb[1], mc[1]))


def pskip_one(mv0, ref0, f, y, x, mbw):
    """one macroblock by include/x264hip_mbskip.h's table"""
    ra = rb = rc = -2
    ma = mb = mc = (0, 0)
    if x > 0:
        ra, ma = int(ref0[f, 2 * y, 2 * x - 1]), tuple(int(v) for v in mv0[f, 4 * y, 4 * x - 1])
    if y > 0:
        rb, mb = int(ref0[f, 2 * y - 1, 2 * x]), tuple(int(v) for v in mv0[f, 4 * y - 1, 4 * x])
        if x < mbw - 1:
            rc, mc = int(ref0[f, 2 * y - 1, 2 * x + 2]), tuple(int(v) for v in mv0[f, 4 * y - 1, 4 * x + 4])
        elif x > 0:
            rc, mc = int(ref0[f, 2 * y - 1, 2 * x - 1]), tuple(int(v) for v in mv0[f, 4 * y - 1, 4 * x - 1])
    if ra == -2 or rb == -2 or (ra == 0 and ma == (0, 0)) or (rb == 0 and mb == (0, 0)):
        return (0, 0)
    return _predict_16x16(ra, ma, rb, mb, rc, mc)


def pskip_mv(mv0, ref0, mbw, mbh):
    """mv0 int16 [nf, 4*mbh, 4*mbw, 2], ref0 int8 [nf, 2*mbh, 2*mbw] -> int16 [mbs, 2]"""
    nf = mv0.shape[0]
    out = np.zeros((nf * mbw * mbh, 2), np.int16)
    for f in range(nf):
        for y in range(mbh):
            for x in range(mbw):
                out[(f * mbh + y) * mbw + x] = pskip_one(mv0, ref0, f, y, x, mbw)
    return out


def pskip_mv_scan8(mv0, ref0, mbw, mbh):
    """the same through h->mb.cache: ref[40] / mv[40] filled as x264_macroblock_cache_load does for a
    progressive one-slice picture (unavailable: ref -2, mv 0), then the C of mvpred.c:129-181 read
    literally off X264_SCAN8_0"""
    nf = mv0.shape[0]
    out = np.zeros((nf * mbw * mbh, 2), np.int16)
    for f in range(nf):
        for y in range(mbh):
            for x in range(mbw):
                ref = np.full(40, -2, np.int64)
                mv = np.zeros((40, 2), np.int64)
                if y > 0:
                    for i in range(4):
                        ref[SCAN8_0 - 8 + i] = ref0[f, 2 * y - 1, 2 * x + (i >> 1)]
                        mv[SCAN8_0 - 8 + i] = mv0[f, 4 * y - 1, 4 * x + i]
                    if x > 0:
                        ref[SCAN8_0 - 8 - 1] = ref0[f, 2 * y - 1, 2 * x - 1]
                        mv[SCAN8_0 - 8 - 1] = mv0[f, 4 * y - 1, 4 * x - 1]
                    if x < mbw - 1:
                        ref[SCAN8_0 - 8 + 4] = ref0[f, 2 * y - 1, 2 * x + 2]
                        mv[SCAN8_0 - 8 + 4] = mv0[f, 4 * y - 1, 4 * x + 4]
                if x > 0:
                    for i in range(4):
                        ref[SCAN8_0 - 1 + 8 * i] = ref0[f, 2 * y + (i >> 1), 2 * x - 1]
                        mv[SCAN8_0 - 1 + 8 * i] = mv0[f, 4 * y + i, 4 * x - 1]
                # x264_mb_predict_mv_pskip
                i_refa, i_refb = int(ref[SCAN8_0 - 1]), int(ref[SCAN8_0 - 8])
                mv_a, mv_b = mv[SCAN8_0 - 1], mv[SCAN8_0 - 8]
                if i_refa == -2 or i_refb == -2 or not (i_refa or mv_a.any()) or not (i_refb or mv_b.any()):
                    r = (0, 0)
                else:
                    # x264_mb_predict_mv_16x16( h, 0, 0, mv )
                    i_refc, mv_c = int(ref[SCAN8_0 - 8 + 4]), mv[SCAN8_0 - 8 + 4]
                    if i_refc == -2:
                        i_refc, mv_c = int(ref[SCAN8_0 - 8 - 1]), mv[SCAN8_0 - 8 - 1]
                    i_count = (i_refa == 0) + (i_refb == 0) + (i_refc == 0)
                    med = tuple(_median(int(mv_a[k]), int(mv_b[k]), int(mv_c[k])) for k in range(2))
                    if i_count > 1:
                        r = med
                    elif i_count == 1:
                        r = tuple(mv_a) if i_refa == 0 else tuple(mv_b) if i_refb == 0 else tuple(mv_c)
                    elif i_refb == -2 and i_refc == -2 and i_refa != -2:
                        r = tuple(mv_a)
                    else:
                        r = med
                out[(f * mbh + y) * mbw + x] = r
    return out


def make_field(mbw, mbh, nframes, seed, kind="mixed"):
    """a list-0 motion field as macroblock_cache_save leaves it.  mixed: intra macroblocks (ref -1,
    mv 0), 16x16, 16x8, 8x16 and 8x8 partitions (with 8x4 / 4x8 / 4x4 vectors inside), refs 0..2,
    a third of the vectors zero; p16: all 16x16 with ref 0.  Returns (mv0, ref0)."""
    rng = np.random.default_rng([mbw, mbh, nframes, seed, 166])
    mv0 = np.zeros((nframes, 4 * mbh, 4 * mbw, 2), np.int16)
    ref0 = np.zeros((nframes, 2 * mbh, 2 * mbw), np.int8)

    def vec():
        return (0, 0) if rng.random() < 0.33 else tuple(int(v) for v in rng.integers(-60, 61, 2))

    def rf():
        return int(rng.choice([0, 0, 0, 1, 2]))
    for f in range(nframes):
        for y in range(mbh):
            for x in range(mbw):
                m = mv0[f, 4 * y:4 * y + 4, 4 * x:4 * x + 4]
                r = ref0[f, 2 * y:2 * y + 2, 2 * x:2 * x + 2]
                u = rng.random()
                if kind == "p16":
                    m[:], r[:] = vec(), 0
                elif u < 0.12:
                    m[:], r[:] = 0, -1
                elif u < 0.45:
                    m[:], r[:] = vec(), rf()
                elif u < 0.6:
                    for h in range(2):
                        m[2 * h:2 * h + 2], r[h] = vec(), rf()
                elif u < 0.75:
                    for h in range(2):
                        m[:, 2 * h:2 * h + 2], r[:, h] = vec(), rf()
                else:
                    for i8 in range(4):
                        sy, sx = 2 * (i8 >> 1), 2 * (i8 & 1)
                        r[i8 >> 1, i8 & 1] = rf()
                        sub = rng.integers(4)
                        for i4 in range(4):
                            if i4 == 0 or (sub == 1 and i4 == 2) or (sub == 2 and i4 == 1) or sub == 3:
                                v = vec()
                            m[sy + (i4 >> 1), sx + (i4 & 1)] = v
    return mv0, ref0


# ------------------------------------------------------------------ x264_macroblock_probe_skip
def thresh_of(cf, qpc):
    return (LAMBDA2[qpc] + 16) >> 5 if cf == 2 else (LAMBDA2[qpc] + 32) >> 6


def probe_literal(bd, T, cf, qp, qpc, fenc, fdec, cnt):
    """macroblock_probe_skip_internal after the prediction is in fdec.  fenc / fdec: the planes in
    FENC / FDEC layout, flat: [Y] (format 0), [Y, C] with U at 0 and V at 8 (FENC) / 16 (FDEC)
    (4:2:0, 4:2:2), [Y, U, V] (4:4:4).  cnt: a Counter of the branches taken."""
    f = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    dct4x4 = np.zeros((8, 16), cd)
    dctscan = np.zeros(16, cd)
    i_qp = qp
    for p in range(3 if cf == 3 else 1):
        quant_cat = CQM_4PC if p else CQM_4PY
        i_decimate_mb = 0
        levels = False
        for i8x8 in range(4):
            fenc_offset = (i8x8 & 1) * 8 + (i8x8 >> 1) * FENC * 8
            fdec_offset = (i8x8 & 1) * 8 + (i8x8 >> 1) * FDEC * 8
            f("sub8x8_dct")(A(dct4x4), A(fenc[p], fenc_offset), A(fdec[p], fdec_offset))
            nz = f("quant_4x4x4")(A(dct4x4), A(T.q4m[quant_cat][i_qp]), A(T.q4b[quant_cat][i_qp]))
            for idx in mbc._bits(nz, 4):
                levels = True
                f("zigzag_scan_4x4")(0, A(dctscan), A(dct4x4[idx]))
                i_decimate_mb += f("decimate_score16")(A(dctscan))
                if i_decimate_mb >= 6:
                    cnt["luma_fail"] += 1
                    return 0
        if levels:
            cnt["luma_pass_levels"] += 1
        i_qp = qpc
    if cf in (1, 2):
        i_qp = qpc
        c422 = int(cf == 2)
        thresh = thresh_of(cf, i_qp)
        dct_dc = np.zeros(8, cd)
        dc_mf = int(T.q4m[CQM_4PC][i_qp + 3 * c422][0]) >> 1
        dc_bias = int(T.q4b[CQM_4PC][i_qp + 3 * c422][0]) << 1
        for ch in range(2):
            p_src, p_dst = 8 * ch, 16 * ch
            ssd = f("ssd")(PIXEL_8x16 if c422 else PIXEL_8x8, A(fdec[1], p_dst), FDEC, A(fenc[1], p_src), FENC)
            if ssd < thresh:
                cnt["chroma_ssd_lt_thresh"] += 1
                continue
            f("sub8x16_dct_dc" if c422 else "sub8x8_dct_dc")(A(dct_dc), A(fenc[1], p_src), A(fdec[1], p_dst))
            for i in range(c422 + 1):
                if f("quant_2x2_dc")(A(dct_dc, 4 * i), dc_mf, dc_bias):
                    cnt["chroma_dc_nonzero"] += 1
                    return 0
            if ssd < thresh * 4:
                cnt["chroma_ssd_lt_4thresh"] += 1
                continue
            for i in range(c422 + 1):
                f("sub8x8_dct")(A(dct4x4[4 * i]), A(fenc[1], p_src + 8 * i * FENC), A(fdec[1], p_dst + 8 * i * FDEC))
                dct4x4[4 * i:4 * i + 4, 0] = 0
            i_decimate_mb = 0
            for i8x8 in range(c422 + 1):
                nz = f("quant_4x4x4")(A(dct4x4[4 * i8x8]), A(T.q4m[CQM_4PC][i_qp]), A(T.q4b[CQM_4PC][i_qp]))
                for b in mbc._bits(nz, 4):
                    f("zigzag_scan_4x4")(0, A(dctscan), A(dct4x4[i8x8 * 4 + b]))
                    i_decimate_mb += f("decimate_score15")(A(dctscan))
                    if i_decimate_mb >= 7:
                        cnt["chroma_ac_fail"] += 1
                        return 0
            cnt["chroma_ac_pass"] += 1
    return 1


def _blocks4(d):
    """[h, w] -> [h/4 * w/4, 4, 4]"""
    h, w = d.shape
    return d.reshape(h // 4, 4, w // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 4, 4)


def _scan(dct):
    """zigzag_scan_4x4_frame of [n, 16]"""
    return dct[:, mbc.ZIG4[:, 1] * 4 + mbc.ZIG4[:, 0]]


def probe_predicate(bd, T, cf, qp, qpc, dy, du, dv):
    """include/x264hip_mbskip.h's order-free test from the differences fenc - prediction: dy [16, 16],
    du / dv [8 or 16, 8] (4:2:0 / 4:2:2) or [16, 16] (4:4:4), int64"""
    def plane_ok(d, cat, q):
        lev, _ = nr.quant(nr.sub4x4_dct(_blocks4(d), bd), T.q4m[cat][q].astype(np.int64), T.q4b[cat][q].astype(np.int64), bd)
        return sum(nr.decimate_score(b) for b in _scan(lev)) < 6
    ok = plane_ok(dy, CQM_4PY, qp)
    if cf == 3:
        ok = ok and plane_ok(du, CQM_4PC, qpc) and plane_ok(dv, CQM_4PC, qpc)
    if cf in (1, 2):
        c422 = int(cf == 2)
        thresh = thresh_of(cf, qpc)
        mf = int(T.q4m[CQM_4PC][qpc + 3 * c422][0]) >> 1
        bias = int(T.q4b[CQM_4PC][qpc + 3 * c422][0]) << 1

        def chroma_ok(d):
            ssd = int((d * d).sum())
            if ssd < thresh:
                return True
            dc = nr.sub8x16_dct_dc(d, bd) if c422 else nr.sub8x8_dct_dc(d, bd)
            if nr.quant(dc, mf, bias, bd)[0].any():
                return False
            if ssd < 4 * thresh:
                return True
            coef = nr.sub4x4_dct(_blocks4(d), bd)
            coef[:, 0] = 0
            lev, _ = nr.quant(coef, T.q4m[CQM_4PC][qpc].astype(np.int64), T.q4b[CQM_4PC][qpc].astype(np.int64), bd)
            return sum(nr.decimate_score(b[1:]) for b in _scan(lev)) < 7
        ok = ok and chroma_ok(du) and chroma_ok(dv)
    return int(ok)


# ------------------------------------------------------------------ prediction
def mb_positions(mbw, mbh, nframes):
    """(frame, x, y) of every macroblock in raster order, in pixels"""
    f, y, x = np.meshgrid(np.arange(nframes), 16 * np.arange(mbh), 16 * np.arange(mbw), indexing="ij")
    return f.reshape(-1), x.reshape(-1), y.reshape(-1)


def clip_mv(mv, mbw, mbh, nframes):
    """macroblock.c:1001-1002 with the limits of mc_cases.mv_limits"""
    _, x, y = mb_positions(mbw, mbh, nframes)
    mn_x, mn_y, mx_x, mx_y = mcc.mv_limits(x, y, mbw, mbh)
    mv = np.asarray(mv, np.int64)
    return np.clip(mv[:, 0], mn_x, mx_x), np.clip(mv[:, 1], mn_y, mx_y)


def predict(ref, mv, weights, mbw, mbh, nframes):
    """the prediction of every macroblock at its clipped vector: (Y [n, 16, 16], U, V) with U / V
    [n, 8 or 16, 8] (4:2:0 / 4:2:2), [n, 16, 16] (4:4:4) or None; weights: 3 x (scale, denom,
    offset) or None"""
    bd, cf = ref.bd, ref.cf
    f, x, y = mb_positions(mbw, mbh, nframes)
    mvx, mvy = clip_mv(mv, mbw, mbh, nframes)
    py = mcc.mc_luma(ref.luma, ref.oy, ref.ox, f, x, y, mvx, mvy, 16, 16, weights[0], bd)
    pu = pv = None
    if cf == 3:
        pu = mcc.mc_luma(ref.chroma[0:4], ref.coy, ref.cox, f, x, y, mvx, mvy, 16, 16, weights[1], bd)
        pv = mcc.mc_luma(ref.chroma[4:8], ref.coy, ref.cox, f, x, y, mvx, mvy, 16, 16, weights[2], bd)
    elif cf:
        vs = int(cf == 1)
        pu, pv = mcc.mc_chroma(ref.chroma[0], ref.coy, ref.cox, f, x, y >> vs, mvx, (2 * mvy) >> vs, 8, 16 >> vs)
        if weights[1] is not None:
            pu = mcc.mc_weight(pu, weights[1], bd)
        if weights[2] is not None:
            pv = mcc.mc_weight(pv, weights[2], bd)
    return py, pu, pv


def to_plane(blocks, mbw, mbh, nframes):
    """[n, h, w] macroblock blocks -> [nframes, mbh * h, mbw * w]"""
    h, w = blocks.shape[1:]
    return blocks.reshape(nframes, mbh, mbw, h, w).transpose(0, 1, 3, 2, 4).reshape(nframes, mbh * h, mbw * w)


def interleave(u, v):
    """[n, h, 8] x 2 -> [n, h, 16], U first"""
    return np.stack([u, v], -1).reshape(u.shape[0], u.shape[1], 16)


# ------------------------------------------------------------------ inputs
# the residual classes of a macroblock (fenc = prediction + residual)
ZERO, FAINT, BUMP, MED, NOISE, CNOISE, CFLAT, CAC, CBUMP, CHECKER = range(10)
_MIX = {False: [ZERO, ZERO, FAINT, FAINT, FAINT, BUMP, MED, MED, NOISE, NOISE, CHECKER],
        True: [ZERO, ZERO, FAINT, FAINT, FAINT, BUMP, MED, NOISE, NOISE, CNOISE, CNOISE, CNOISE, CFLAT, CFLAT, CAC, CAC,
               CAC, CBUMP, CHECKER]}


def _boundary_case(bd, cf, mbw, mbh, nframes, cqm, recipe, key):
    """leg "b" (the prediction handed over as planes) on mbenc_cases' boundary macroblocks: one per
    entry (qp, rects, waves) of `recipe`, fenc mid grey, prediction = fenc + the rectangles and waves"""
    base = mbc._boundary_case(bd, cf, mbw, mbh, nframes, cqm, tuple((q, 0, r, w) for q, r, w in recipe), key)
    n, crows = base.nmb, base.chroma_rows

    def blocks(plane, h, w):
        return plane.reshape(nframes, mbh, h, mbw, w).transpose(0, 1, 3, 2, 4).reshape(n, h, w).astype(np.int64)
    fy, py = blocks(base.fenc_y, 16, 16), blocks(base.pred_y, 16, 16)
    fu = fv = pu = pv = None
    if cf:
        fc, pc = blocks(base.fenc_c, crows, 16), blocks(base.pred_c, crows, 16)
        fu, fv, pu, pv = fc[..., 0::2], fc[..., 1::2], pc[..., 0::2], pc[..., 1::2]
    qp_table = mbc.chroma_qp_table(bd)
    return types.SimpleNamespace(
        bd=bd, cf=cf, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, leg="b", cqm=cqm, W=16 * mbw, H=16 * mbh, crows=crows,
        qp=base.qp, qpc=qp_table[base.qp].astype(np.int64), qp_table=qp_table, klass=np.full(n, -1), pskip_mv=np.zeros((n, 2), np.int16),
        weights=(None, None, None), ref=None, blocks=types.SimpleNamespace(fenc=(fy, fu, fv), pred=(py, pu, pv)),
        fenc=[base.fenc_y] + ([base.fenc_c] if cf else []), pred=[base.pred_y] + ([base.pred_c] if cf else []), key=key)


@functools.lru_cache(maxsize=None)
def make_case(bd, cf, mbw, mbh, nframes, leg, cqm="flat", seed=0, recipe=None):
    """Seeded inputs of one probe.  The reference is synthetic texture; each macroblock has a skip
    vector (zero, small, or anywhere inside its limits; at the four corner macroblocks of every
    frame beyond mv_max / below mv_min, so the clip acts) and fenc = its prediction at that vector
    + a residual class: zero; one or two faint flat 4x4 patches (a level of +-1 each: a score of 3
    or 6, either side of the luma bound); an isolated bump; noise around / well above the
    quantiser step; chroma noise around thresh and 4 * thresh; a flat chroma offset (the DC
    check); a zero-sum chroma pattern per 4x4 block (the AC check alone); a +-1 chroma pixel at low
    qp; a full-scale 0 / max checker against its inverse in the reference at qp 0 and qp_max_spec.
    leg "pw" weights all three planes; leg "b" hands the same prediction over as planes.
    recipe: the boundary picture, see _boundary_case."""
    if recipe is not None:
        return _boundary_case(bd, cf, mbw, mbh, nframes, cqm, boundary_recipe(cf, cqm) if recipe == "boundary" else recipe,
                              (bd, cf, mbw, mbh, nframes, leg, cqm, seed, recipe))
    rng = np.random.default_rng([bd, cf, mbw, mbh, nframes, LEGS.index(leg), cqm == "jvt", seed, 985])
    pm, qmax = (1 << bd) - 1, mbc.qp_max_spec(bd)
    n = nframes * mbw * mbh
    W, H = 16 * mbw, 16 * mbh
    hs, vs = (1, 1) if cf == 1 else (1, 0) if cf == 2 else (0, 0)
    crows, ccols = 16 >> vs, 16 >> hs
    qp_table = mbc.chroma_qp_table(bd)
    weights = WEIGHTS if leg == "pw" else (None, None, None)
    fr, px, py_ = mb_positions(mbw, mbh, nframes)
    corner = ((px == 0) | (px == W - 16)) & ((py_ == 0) | (py_ == H - 16))

    klass = rng.choice(_MIX[cf in (1, 2)], n)
    if n <= 4:
        klass = np.array([FAINT, NOISE, CNOISE if cf in (1, 2) else MED, CAC if cf in (1, 2) else ZERO])[np.arange(n) % 4]
    klass[corner & (klass == CHECKER)] = FAINT
    qp = rng.integers(0, qmax + 1, n)
    low = klass == CBUMP
    qp[low] = rng.integers(0, 24 + 6 * (bd - 8), int(low.sum()))
    chk = klass == CHECKER
    qp[chk] = rng.choice([0, qmax], int(chk.sum()))
    qpc = qp_table[qp].astype(np.int64)

    # the skip vectors
    mn_x, mn_y, mx_x, mx_y = mcc.mv_limits(px, py_, mbw, mbh)
    mv = np.zeros((n, 2), np.int64)
    u = rng.random(n)
    small = (u >= 0.4) & (u < 0.8)
    mv[small] = rng.integers(-24, 25, (int(small.sum()), 2))
    wide = u >= 0.8
    mv[wide, 0] = rng.integers(mn_x[wide], mx_x[wide] + 1)
    mv[wide, 1] = rng.integers(mn_y[wide], mx_y[wide] + 1)
    mv[chk] = 0
    right, low_ = px == W - 16, py_ == H - 16
    beyond = rng.integers(5, 400, (n, 2))
    mv[corner, 0] = np.where(right, mx_x + beyond[:, 0], mn_x - beyond[:, 0])[corner]
    mv[corner, 1] = np.where(low_, mx_y + beyond[:, 1], mn_y - beyond[:, 1])[corner]
    if n == 1:                                                  # the one macroblock is all four corners
        mv[0] = (mx_x[0] + 37, mn_y[0] - 91)

    # the reference, the inverse checker planted under the checker macroblocks
    yy, xx = np.mgrid[0:16, 0:16]
    chk_y = ((yy + xx) & 1) * pm
    cy, cx = np.mgrid[0:crows, 0:ccols]
    chk_c = ((cy + cx) & 1) * pm
    frames = []
    for f in range(nframes):
        y = np.array(wc._tex(H, W, bd, 1000 * seed + 17 * f + 1), np.int64)
        c = [np.array(wc._tex(H >> vs, W >> hs, bd, 1000 * seed + 17 * f + 5 + p), np.int64) for p in range(2)] if cf else []
        for mb in np.flatnonzero(chk & (fr == f)):
            y[py_[mb]:py_[mb] + 16, px[mb]:px[mb] + 16] = pm - chk_y
            for p in range(2 if cf else 0):
                c[p][py_[mb] >> vs:(py_[mb] >> vs) + crows, px[mb] >> hs:(px[mb] >> hs) + ccols] = pm - chk_c
        frames.append(wc.Frame(bd, W, H, cf, y, c))
    ref = mcc.Ref(frames)
    pred = predict(ref, mv, weights, mbw, mbh, nframes)

    # fenc = prediction + residual
    res_y = np.zeros((n, 16, 16))
    res_c = [np.zeros((n, crows, ccols)) for _ in range(2)]

    def patches(r, qs, count):
        for b in rng.choice(r.shape[0] // 4 * (r.shape[1] // 4), count, replace=False):
            y0, x0 = 4 * (b // (r.shape[1] // 4)), 4 * (b % (r.shape[1] // 4))
            r[y0:y0 + 4, x0:x0 + 4] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(0.2, 0.38)))
    for mb in range(n):
        k = int(klass[mb])
        qs, qsc = mbc._qstep(int(qp[mb])), mbc._qstep(int(qpc[mb]))
        ry = res_y[mb]
        rc = [res_c[0][mb], res_c[1][mb]]
        if k == FAINT:
            patches(ry, qs, int(rng.choice([1, 1, 2])))
            if cf == 3 and rng.random() < 0.3:
                patches(rc[rng.integers(2)], qsc, 1)
        elif k == BUMP:
            ry[rng.integers(16), rng.integers(16)] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(0.3, 1.2)))
        elif k in (MED, NOISE):
            a = rng.choice([0.3, 0.45, 0.6]) if k == MED else rng.choice([1.0, 2.0, 4.0])
            ry[:] = rng.normal(0, qs * a, (16, 16))
            for p in range(2):
                rc[p][:] = rng.normal(0, qsc * a * (1.0 if cf == 3 else 0.25), rc[p].shape)
        elif k == CNOISE:
            if rng.random() < 0.5:
                patches(ry, qs, 1)
            for p in range(2):
                rc[p][:] = rng.normal(0, qsc * rng.choice([0.04, 0.08, 0.12, 0.2]), rc[p].shape)
        elif k == CFLAT:
            rc[0][:] = rng.choice([-1, 1]) * max(1, round(qsc * rng.choice([0.1, 0.3, 1.0, 3.0])))
            rc[1][:] = rng.choice([-1, 0, 1]) * max(1, round(qsc * rng.choice([0.1, 0.3, 1.0])))
        elif k == CAC:
            a = max(1, round(qsc * rng.choice([0.1, 0.2, 0.35, 0.6, 1.5])))
            sign = np.where((cy + cx) & 1, -a, a)
            for p in range(2):
                on = rng.random((crows // 4, ccols // 4)) < rng.choice([0.3, 1.0])
                rc[p][:] = sign * np.repeat(np.repeat(on, 4, 0), 4, 1)
                if rng.random() < 0.4:
                    rc[p][:] = 0
        elif k == CBUMP:
            rc[rng.integers(2)][rng.integers(crows), rng.integers(ccols)] = rng.choice([-2, -1, 1, 2])
    fenc_y = np.clip(pred[0] + np.rint(res_y).astype(np.int64), 0, pm)
    fenc_y[chk] = chk_y
    fenc_u = fenc_v = None
    if cf:
        fenc_u = np.clip(pred[1] + np.rint(res_c[0]).astype(np.int64), 0, pm)
        fenc_v = np.clip(pred[2] + np.rint(res_c[1]).astype(np.int64), 0, pm)
        fenc_u[chk], fenc_v[chk] = chk_c, chk_c
    pdt = orc.pixel_dtype(bd)
    blocks = types.SimpleNamespace(fenc=(fenc_y, fenc_u, fenc_v), pred=pred)

    def planes(y, u, v):
        out = [to_plane(y, mbw, mbh, nframes).astype(pdt)]
        if cf == 3:
            out += [to_plane(u, mbw, mbh, nframes).astype(pdt), to_plane(v, mbw, mbh, nframes).astype(pdt)]
        elif cf:
            out += [to_plane(interleave(u, v), mbw, mbh, nframes).astype(pdt)]
        return out
    return types.SimpleNamespace(
        bd=bd, cf=cf, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, leg=leg, cqm=cqm, W=W, H=H, crows=crows,
        qp=qp.astype(np.int8), qpc=qpc, qp_table=qp_table, klass=klass, pskip_mv=mv.astype(np.int16), weights=weights,
        ref=ref, blocks=blocks, fenc=planes(*blocks.fenc), pred=planes(*pred),
        key=(bd, cf, mbw, mbh, nframes, leg, cqm, seed))


def _layout(y, u, v, cf, stride):
    """one macroblock's planes in FENC / FDEC layout, flat, as probe_literal takes them"""
    dt = y.dtype
    out = [np.zeros((16, stride), dt)]
    out[0][:, :16] = y
    if cf == 3:
        for p in (u, v):
            b = np.zeros((16, stride), dt)
            b[:, :16] = p
            out.append(b)
    elif cf:
        b = np.zeros((16, stride), dt)
        b[:u.shape[0], :8] = u
        b[:v.shape[0], stride // 2:stride // 2 + 8] = v
        out.append(b)
    return [b.reshape(-1) for b in out]


def probe(case):
    """(skip uint8 [mbs], the literal checker's branch counters) of a case"""
    T = mbc.tables(case.bd, case.cqm)
    pdt = orc.pixel_dtype(case.bd)
    cnt = collections.Counter()
    skip = np.zeros(case.nmb, np.uint8)
    for mb in range(case.nmb):
        e = [None if b is None else b[mb].astype(pdt) for b in case.blocks.fenc]
        p = [None if b is None else b[mb].astype(pdt) for b in case.blocks.pred]
        skip[mb] = probe_literal(case.bd, T, case.cf, int(case.qp[mb]), int(case.qpc[mb]), _layout(*e, case.cf, FENC),
                                 _layout(*p, case.cf, FDEC), cnt)
    return skip, cnt


def probe_by_predicate(case):
    T = mbc.tables(case.bd, case.cqm)
    skip = np.zeros(case.nmb, np.uint8)
    for mb in range(case.nmb):
        d = [None if e is None else e[mb].astype(np.int64) - p[mb].astype(np.int64)
             for e, p in zip(case.blocks.fenc, case.blocks.pred)]
        skip[mb] = probe_predicate(case.bd, T, case.cf, int(case.qp[mb]), int(case.qpc[mb]), *d)
    return skip


@functools.lru_cache(maxsize=None)
def expected(key):
    """probe(make_case(*key)), computed once per process and shared; do not modify"""
    return probe(make_case(*key))


def case_keys(bd, cf, leg):
    """the case list of one (bit depth, chroma format, leg): every shape with the flat matrices and
    the 5x4 x 2 one with the JVT matrices"""
    return [(bd, cf, w, h, n, leg, "flat", 0) for w, h, n in SHAPES] + [(bd, cf, 5, 4, 2, leg, "jvt", 0)]


# ------------------------------------------------------------------ the conversion
def skip_convert(mb_flags, cbp, mv0, ref0, pskip, b_bframe, direct, mbw, mbh):
    """macroblock.c:953-971 on x264hip_mbenc_t's mb_flags / cbp"""
    out = np.array(mb_flags, np.uint8)
    per = mbw * mbh
    for mb in range(out.size):
        fl = int(mb_flags[mb])
        if fl & INTRA or int(cbp[mb]) & 0x3f:
            continue
        if b_bframe:
            conv = bool(direct[mb])
        else:
            f, r = divmod(mb, per)
            y, x = divmod(r, mbw)
            conv = (not fl & SKIP and bool(fl & D16) and ref0[f, 2 * y, 2 * x] == 0 and
                    tuple(mv0[f, 4 * y, 4 * x]) == tuple(pskip[mb]))
        if conv:
            out[mb] |= SKIP
    return out


def make_convert_case(mbw, mbh, nframes, b_bframe, seed=0):
    """a field whose macroblocks are, in raster order, made skip candidates or not: a candidate is
    16x16 with ref 0 and the skip vector of its (final) neighbours; the others differ from one in
    the vector, the reference, the partition, the flags or the cbp"""
    rng = np.random.default_rng([mbw, mbh, nframes, int(b_bframe), seed, 953])
    mv0, ref0 = make_field(mbw, mbh, nframes, seed + 1)
    n = nframes * mbw * mbh
    flags = np.zeros(n, np.uint8)
    cbp = np.zeros(n, np.int32)
    direct = (rng.random(n) < 0.6).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    for mb in range(n):
        f, r = divmod(mb, mbw * mbh)
        y, x = divmod(r, mbw)
        m, rf = mv0[f, 4 * y:4 * y + 4, 4 * x:4 * x + 4], ref0[f, 2 * y:2 * y + 2, 2 * x:2 * x + 2]
        fl = (T8 if rng.random() < 0.3 else 0) | (D16 if rng.random() < 0.8 else 0)
        if (rf == -1).all():
            fl = INTRA | (fl & T8)
        elif rng.random() < 0.1:
            fl |= SKIP
        if fl & D16 and not fl & INTRA:
            m[:], rf[:] = pskip_one(mv0, ref0, f, y, x, mbw), 0
            u = rng.random()
            if u < 0.12:
                m[:, :, int(rng.integers(2))] += rng.choice([-1, 1])
            elif u < 0.2:
                rf[:] = 1
        flags[mb] = fl
        cbp[mb] = rng.choice([0, 0, 0, 0, 0x200, 0x400, 0x600, 1, 8, 0x10, 0x20, 0x2f])
    ps = pskip_mv(mv0, ref0, mbw, mbh)
    return types.SimpleNamespace(mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, b_bframe=b_bframe, flags=flags, cbp=cbp,
                                 mv0=mv0, ref0=ref0, pskip=ps, direct=direct)


# ------------------------------------------------------------------ what the GPU tests compare
# The boundary macroblocks of the probe: (what is pinned, chroma formats, (qp, rects, waves)), residuals of
# tests/mbenc_cases.py's kind.  On the ones marked * the comparison flipped at its boundary
# (tests/mutants.py) gives the other answer.
_U422 = (1, 0, 0, 16, 8)
BOUNDARY = (
    ("luma score 3 < 6: skip", (0, 1, 2), (17, ((0, 4, 0, 4, 4, -2),), ())),
    ("luma score = 6: no skip *", (0, 1, 2), (17, ((0, 4, 0, 4, 4, -2),), ((0, 0, 12, 0, 2, -1), (0, 0, 0, 0, 1, 1)))),
    ("chroma AC score = 7 at 4:2:0: no skip *", (1,), (22, (), ((1, 4, 0, 0, 1, 2), (1, 4, 4, 2, 0, -3), (1, 0, 4, 2, 0, 3)))),
    ("chroma AC score = 7 at 4:2:2: no skip *", (2,), (19, (), ((1, 4, 4, 2, 0, -2), (1, 4, 4, 0, 1, -1), (1, 4, 0, 2, 0, -2)))),
    ("ssd of U = thresh at 4:2:2 with a DC that quantises to a level: no skip *", (2,),
     (25, (_U422 + (1,), (1, 0, 2, 1, 1, -1), (1, 2, 7, 1, 1, 3), (1, 5, 2, 1, 1, 1)), ())),
    ("ssd of U = thresh = 36 at 4:2:0, qp 22, JVT matrices (the flat ones leave such a DC 0): no skip *", (1,),
     (22, tuple((1, 4 * (b >> 1), 4 * (b & 1), 3, 3, 1) for b in range(4)), ()), "jvt"),
)
GPU_GROUPS = ("pskip", "probe", "convert", "boundary")


def boundary_recipe(cf, cqm="flat"):
    return tuple(b[2] for b in BOUNDARY if cf in b[1] and (b[3:] or ("flat",))[0] == cqm)


def boundary_keys():
    """one row of boundary macroblocks per (bit depth, chroma format), on leg b"""
    return [(bd, cf, len(boundary_recipe(cf, cqm)), 1, 1, "b", cqm, 0, "boundary")
            for bd in (8, 10) for cf, cqm in ((0, "flat"), (1, "flat"), (2, "flat"), (1, "jvt"))]


def gpu_keys(group=None, **where):
    """every entry tests/test_gpu_mbskip.py compares with the device value for value, which is the
    list the boundary mutants of tests/test_cpu_mutants.py are held to: ("pskip", (mbw, mbh, nf),
    seed) for mb_predict_mv_pskip, ("probe", key) for mb_probe_skip, ("convert", (mbw, mbh, nf),
    b_bframe) for mb_skip_convert.  group: one of GPU_GROUPS (one test function each); where: bd /
    cf / leg of a probe key, shape or bframe of the other entries."""
    keys = {"pskip": [("pskip", sh, seed) for sh in SHAPES for seed in (0, 1)],
            "probe": [("probe", k) for bd in (8, 10) for cf in (0, 1, 2, 3) for leg in LEGS for k in case_keys(bd, cf, leg)],
            "convert": [("convert", sh, bf) for bf in (0, 1) for sh in SHAPES],
            "boundary": [("probe", k) for k in boundary_keys()]}
    keys = [e for g in GPU_GROUPS if group in (None, g) for e in keys[g]]
    pick = {"bd": lambda e: e[1][0], "cf": lambda e: e[1][1], "leg": lambda e: e[1][5], "shape": lambda e: e[1],
            "bframe": lambda e: e[2]}
    return [e for e in keys if all(pick[n](e) == v for n, v in where.items())]


def gpu_expected(entry):
    """what the device's output of a gpu_keys() entry is compared with"""
    if entry[0] == "pskip":
        mv0, ref0 = make_field(*entry[1], entry[2])
        return pskip_mv(mv0, ref0, entry[1][0], entry[1][1])
    if entry[0] == "probe":
        return expected(entry[1])[0]
    c = make_convert_case(*entry[1], entry[2])
    return skip_convert(c.flags, c.cbp, c.mv0, c.ref0, c.pskip, entry[2], c.direct, c.mbw, c.mbh)


def key_size(entry):
    """macroblocks of a gpu_keys() entry: what it costs"""
    k = entry[1]
    return k[2] * k[3] * k[4] if entry[0] == "probe" else k[0] * k[1] * k[2] // 8 + 1
