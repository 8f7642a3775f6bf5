"""The inter macroblock encode restated per macroblock, from the reference's C
(encoder/macroblock.c:259-490 and 618-972 with b_inter = 1, no lossless / trellis / noise
reduction), and the inputs of tests/test_cpu_mbenc.py and tests/test_gpu_mbenc.py.  No GPU code.

* Only the control flow is restated: every transform, quantiser, scan and score is the oracle's
  (tests/oracle_lib.py), called on FENC / FDEC-layout buffers exactly as x264 calls its tables.
  Of the arithmetic only the static inlines of macroblock.c:35-96 are Python: zigzag_scan_2x2_dc,
  zigzag_scan_2x4_dc, idct_dequant_2x2_dc, idct_dequant_2x2_dconly, dct2x2dc.
* encode(case) returns the outputs of include/x264hip_mbenc.h plus branch counters (which arm of
  the reference each macroblock took), so the coverage of the inputs can be asserted.
* decode(case, out) rebuilds the reconstruction from the outputs alone, as a decoder would.
* make_case: the seeded inputs.

x264_lambda2_tab is tests/golden/mbenc_tables.json's (tests/golden/make_mbenc_tables.py).
"""
import collections
import functools
import json
import os
import types

import numpy as np

import oracle_lib as orc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "mbenc_tables.json")) as _fh:
    LAMBDA2 = json.load(_fh)["x264_lambda2_tab"]
with open(os.path.join(HERE, "golden", "ref_tables.json")) as _fh:
    _R = json.load(_fh)
ZIG4 = np.array(_R["zigzag"]["ZIGZAG4_FRAME"]).reshape(16, 2)     # (y, x): level[i] = dct[x*4 + y]
ZIG8 = np.array(_R["zigzag"]["ZIGZAG8_FRAME"]).reshape(64, 2)
JVT = [_R["arrays"][k] for k in ("x264_cqm_jvt4i", "x264_cqm_jvt4p", "x264_cqm_jvt4i", "x264_cqm_jvt4p",
                                 "x264_cqm_jvt8i", "x264_cqm_jvt8p", "x264_cqm_jvt8i", "x264_cqm_jvt8p")]
FLAT = [[16] * 16] * 4 + [[16] * 64] * 4

INTRA, T8, D16, SKIP = 1, 2, 4, 8
CQM_4PY, CQM_4PC, CQM_8PY = 1, 3, 1
FENC, FDEC = 16, 32                                              # FENC_STRIDE, FDEC_STRIDE
PIXEL_8x16, PIXEL_8x8 = 2, 3
A = orc._addr


def qp_max_spec(bd):
    return 51 + 6 * (bd - 8)


def chroma_qp_table(bd, offset=0):
    """h->chroma_qp_table[0 .. QP_MAX_SPEC] (H.264 table 8-15 shifted by QP_BD_OFFSET)"""
    bdo = 6 * (bd - 8)
    tail = [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
    out = np.zeros(52 + bdo, np.uint8)
    for qp in range(52 + bdo):
        q = min(max(qp + offset, 0), 51 + bdo)
        out[qp] = q if q - bdo < 30 else tail[q - bdo - 30] + bdo
    return out


@functools.lru_cache(maxsize=None)
def tables(bd, cqm="flat"):
    lists = FLAT if cqm == "flat" else JVT
    q4m, q4b, q8m, q8b = orc.cqm_init(bd, lists)
    dq4, dq8 = orc.cqm_dequant(lists)
    return types.SimpleNamespace(q4m=q4m, q4b=q4b, q8m=q8m, q8b=q8b, dq4=dq4, dq8=dq8)


# ------------------------------------------------------------------ macroblock.c:35-96
def _wrap(bd, v):
    """a value stored to a dctcoef"""
    return int(np.array(v, np.int64).astype(orc.coef_dtype(bd)))


def zigzag_scan_2x2_dc(dct):
    return [dct[0], dct[2], dct[1], dct[3]]                       # ZIG(i,y,x) level[i] = dct[x*2+y]


def zigzag_scan_2x4_dc(dct):
    return [dct[0], dct[2], dct[1], dct[4], dct[6], dct[3], dct[5], dct[7]]


def _idct_dequant_2x2(bd, dct, dequant_mf, qp):
    d0, d1, d2, d3 = dct[0] + dct[1], dct[2] + dct[3], dct[0] - dct[1], dct[2] - dct[3]
    dmf = int(dequant_mf[qp % 6][0]) << (qp // 6)
    return [_wrap(bd, (v * dmf) >> 5) for v in (d0 + d1, d0 - d1, d2 + d3, d2 - d3)]


def idct_dequant_2x2_dc(bd, dct, dct4x4, dequant_mf, qp):
    for k, v in enumerate(_idct_dequant_2x2(bd, [int(x) for x in dct], dequant_mf, qp)):
        dct4x4[k][0] = v


def idct_dequant_2x2_dconly(bd, dct, dequant_mf, qp):
    dct[:4] = _idct_dequant_2x2(bd, [int(x) for x in dct[:4]], dequant_mf, qp)


def dct2x2dc(bd, d, dct4x4):
    a = [int(dct4x4[k][0]) for k in range(4)]
    d0, d1, d2, d3 = a[0] + a[1], a[2] + a[3], a[0] - a[1], a[2] - a[3]
    d[0], d[2], d[1], d[3] = _wrap(bd, d0 + d1), _wrap(bd, d2 + d3), _wrap(bd, d0 - d1), _wrap(bd, d2 - d3)
    for k in range(4):
        dct4x4[k][0] = 0


def _side(v, bound):
    """for the branch counters: which side of a bound of the reference a value fell on"""
    return "below" if v < bound else "above" if v > bound else "at"


def _bits(mask, n):
    return [i for i in range(n) if (mask >> i) & 1]


# ------------------------------------------------------------------ the macroblock
class MbOut:
    """what macroblock_encode_internal leaves besides fdec"""

    def __init__(self, bd):
        cd = orc.coef_dtype(bd)
        self.level = np.zeros((48, 16), cd)
        self.chroma_dc = np.zeros((2, 8), cd)
        self.nnz = np.zeros(48, np.uint8)
        self.cbp_luma = self.cbp_chroma = 0
        self.nnz_dc = [0, 0]


def encode_luma(bd, T, dec, t8, qp, fenc, fdec, o, cnt):
    """macroblock.c:801-921, one plane; fenc [16*16], fdec [16*32] (prediction in, reconstruction out)"""
    f = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    dct = np.zeros(256, cd)
    i_decimate_mb = 0
    plane_cbp = 0
    if t8:
        dct8 = dct.reshape(4, 64)
        f("sub16x16_dct8")(A(dct), A(fenc), A(fdec))
        nzs = part = 0
        for idx in range(4):
            nz = f("quant_8x8")(A(dct8[idx]), A(T.q8m[CQM_8PY][qp]), A(T.q8b[CQM_8PY][qp]))
            if nz:
                nzs += 1
                lev = o.level[4 * idx:4 * idx + 4].reshape(64)
                f("zigzag_scan_8x8")(0, A(lev), A(dct8[idx]))
                if dec:
                    s = f("decimate_score64")(A(lev))
                    cnt["score8x8", _side(s, 4)] += 1
                    i_decimate_mb += s
                    if s >= 4:
                        plane_cbp |= 1 << idx
                    else:
                        part += 1
                else:
                    plane_cbp |= 1 << idx
        if dec and nzs:
            cnt["score_mb", _side(i_decimate_mb, 6)] += 1
        if i_decimate_mb >= 6 or not dec:
            o.cbp_luma |= plane_cbp
            for idx in _bits(plane_cbp, 4):
                f("dequant_8x8")(A(dct8[idx]), A(T.dq8[CQM_8PY]), qp)
                f("add8x8_idct8")(A(fdec, 8 * (idx & 1) + 8 * (idx >> 1) * FDEC), A(dct8[idx]))
                o.nnz[4 * idx:4 * idx + 4] = 1                    # STORE_8x8_NNZ
            if nzs:
                cnt["luma8_part" if part else "luma8_whole"] += 1
        elif nzs:
            cnt["luma8_dropped"] += 1
    else:
        dct4 = dct.reshape(16, 16)
        f("sub16x16_dct")(A(dct), A(fenc), A(fdec))
        nzs = part = 0
        for i8 in range(4):
            i_decimate_8x8 = 0 if dec else 6
            nz = f("quant_4x4x4")(A(dct4[4 * i8]), A(T.q4m[CQM_4PY][qp]), A(T.q4b[CQM_4PY][qp]))
            if nz:
                nzs += 1
                for i4 in _bits(nz, 4):
                    idx = 4 * i8 + i4
                    f("zigzag_scan_4x4")(0, A(o.level[idx]), A(dct4[idx]))
                    f("dequant_4x4")(A(dct4[idx]), A(T.dq4[CQM_4PY]), qp)
                    if i_decimate_8x8 < 6:
                        i_decimate_8x8 += f("decimate_score16")(A(o.level[idx]))
                    o.nnz[idx] = 1
                i_decimate_mb += i_decimate_8x8
                if dec:
                    cnt["score8x8", _side(i_decimate_8x8, 4)] += 1
                if i_decimate_8x8 < 4:
                    o.nnz[4 * i8:4 * i8 + 4] = 0
                    part += 1
                else:
                    plane_cbp |= 1 << i8
        if dec and nzs:
            cnt["score_mb", _side(i_decimate_mb, 6)] += 1
        if i_decimate_mb < 6:
            plane_cbp = 0
            o.nnz[:16] = 0
            if nzs:
                cnt["luma4_dropped"] += 1
        else:
            o.cbp_luma |= plane_cbp
            for i8 in _bits(plane_cbp, 4):
                f("add8x8_idct")(A(fdec, (i8 & 1) * 8 + (i8 >> 1) * 8 * FDEC), A(dct4[4 * i8]))
            cnt["luma4_part" if part else "luma4_whole"] += 1


def mb_optimize_chroma_dc(bd, dct_dc, dequant_mf, qp, c422, cnt):
    """macroblock.c:245-257"""
    dmf = int(dequant_mf[qp % 6][0]) << (qp // 6)
    cnt["dmf", _side(dmf, 32 * 64)] += 1
    if dmf > 32 * 64:
        cnt["dmf_shortcut"] += 1
        return 1
    cnt["dmf_search"] += 1
    r = orc.fn(bd, "optimize_chroma_2x4_dc" if c422 else "optimize_chroma_2x2_dc")(A(dct_dc), dmf)
    if not r:
        cnt["chroma_opt0"] += 1
    return r


def encode_chroma(bd, T, dec, c422, qp, fenc, fdec, o, cnt):
    """mb_encode_chroma_internal, macroblock.c:259-490 with b_inter = 1; fenc [16*16] (U, V at +8),
    fdec [16*32] (U, V at +16); qp is the chroma qp"""
    f = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    dequant_mf = T.dq4[CQM_4PC]
    dct_dc = np.zeros(8, cd)
    ndc = 8 if c422 else 4
    qdc = qp + 3 * c422
    dc_mf, dc_bias = int(T.q4m[CQM_4PC][qdc][0]) >> 1, int(T.q4b[CQM_4PC][qdc][0]) << 1

    def quant_dc():
        nz = 0
        for i in range(c422 + 1):
            nz |= f("quant_2x2_dc")(A(dct_dc, 4 * i), dc_mf, dc_bias)
        return nz

    def dc_only(ch, p_dst):
        if c422:
            o.chroma_dc[ch][:] = zigzag_scan_2x4_dc(dct_dc)
            f("idct_dequant_2x4_dconly")(A(dct_dc), A(dequant_mf), qp + 3)
        else:
            o.chroma_dc[ch][:4] = zigzag_scan_2x2_dc(dct_dc)
            idct_dequant_2x2_dconly(bd, dct_dc, dequant_mf, qp)
        for i in range(c422 + 1):
            f("add8x8_idct_dc")(A(fdec, p_dst + 8 * i * FDEC), A(dct_dc, 4 * i))

    if dec:
        cnt["chroma_qp", _side(qp, 18)] += 1
    if dec and qp >= 18:
        thresh = (LAMBDA2[qp] + 16) >> 5 if c422 else (LAMBDA2[qp] + 32) >> 6
        ssd = np.zeros(2, np.int32)
        score = f("var2")(PIXEL_8x16 if c422 else PIXEL_8x8, A(fenc), A(fdec), A(ssd))
        cnt["var2", _side(score, thresh * 4)] += 1
        if score < thresh * 4:
            for ch in range(2):
                cnt["ssd", _side(ssd[ch], thresh)] += 1
                if ssd[ch] > thresh:
                    p_src, p_dst = 8 * ch, 16 * ch
                    dct_dc[:] = 0
                    f("sub8x16_dct_dc" if c422 else "sub8x8_dct_dc")(A(dct_dc), A(fenc, p_src), A(fdec, p_dst))
                    if quant_dc():
                        if not mb_optimize_chroma_dc(bd, dct_dc, dequant_mf, qdc, c422, cnt):
                            continue
                        o.nnz_dc[ch] = 1
                        dc_only(ch, p_dst)
                        o.cbp_chroma = 1
            cnt["chroma_early_dc" if o.cbp_chroma else "chroma_early_none"] += 1
            return

    tails = set()
    for ch in range(2):
        p_src, p_dst = 8 * ch, 16 * ch
        i_decimate_score = 0 if dec else 7
        nz_ac = 0
        dct4x4 = np.zeros((8, 16), cd)
        for i in range(c422 + 1):
            f("sub8x8_dct")(A(dct4x4[4 * i]), A(fenc, p_src + 8 * i * FENC), A(fdec, p_dst + 8 * i * FDEC))
        dct_dc[:] = 0
        if c422:
            f("dct2x4dc")(A(dct_dc), A(dct4x4))
        else:
            dct2x2dc(bd, dct_dc, dct4x4)
        for i8x8 in range(c422 + 1):
            nz = f("quant_4x4x4")(A(dct4x4[4 * i8x8]), A(T.q4m[CQM_4PC][qp]), A(T.q4b[CQM_4PC][qp]))
            nz_ac |= nz
            for i4x4 in _bits(nz, 4):
                idx = 16 + ch * 16 + i8x8 * 8 + i4x4
                f("zigzag_scan_4x4")(0, A(o.level[idx]), A(dct4x4[i8x8 * 4 + i4x4]))
                f("dequant_4x4")(A(dct4x4[i8x8 * 4 + i4x4]), A(dequant_mf), qp)
                if i_decimate_score < 7:
                    i_decimate_score += f("decimate_score15")(A(o.level[idx]))
                o.nnz[idx] = 1
        nz_dc = quant_dc()
        o.nnz_dc[ch] = int(nz_dc != 0)
        if dec and nz_ac:
            cnt["score_chroma", _side(i_decimate_score, 7)] += 1
        if i_decimate_score < 7 or not nz_ac:
            o.nnz[16 + 16 * ch:32 + 16 * ch] = 0
            if not nz_dc:
                tails.add("empty")
                continue
            if not mb_optimize_chroma_dc(bd, dct_dc, dequant_mf, qdc, c422, cnt):
                o.nnz_dc[ch] = 0
                tails.add("empty")
                continue
            dc_only(ch, p_dst)
            tails.add("dconly")
        else:
            o.cbp_chroma = 1
            tails.add("dcac")
            if nz_dc:
                if c422:
                    o.chroma_dc[ch][:] = zigzag_scan_2x4_dc(dct_dc)
                    f("idct_dequant_2x4_dc")(A(dct_dc), A(dct4x4), A(dequant_mf), qp + 3)
                else:
                    o.chroma_dc[ch][:4] = zigzag_scan_2x2_dc(dct_dc)
                    idct_dequant_2x2_dc(bd, dct_dc, dct4x4, dequant_mf, qp)
            for i in range(c422 + 1):
                f("add8x8_idct")(A(fdec, p_dst + 8 * i * FDEC), A(dct4x4[4 * i]))
    for t in tails:
        cnt["chroma_" + t] += 1
    o.cbp_chroma += o.nnz_dc[0] | o.nnz_dc[1] | o.cbp_chroma        # macroblock.c:487-489


def encode_mb(bd, T, cf, dec, flags, qp, qpc, fenc_y, fdec_y, fenc_c, fdec_c, cnt):
    """one inter macroblock; the fdec buffers hold the prediction and get the reconstruction.
    Returns MbOut with the levels of every block whose nnz is 0 cleared (include/x264hip_mbenc.h)."""
    o = MbOut(bd)
    if flags & SKIP:                                              # macroblock_encode_skip
        return o
    tag = "8" if flags & T8 else "4"
    c = collections.Counter()
    encode_luma(bd, T, dec, bool(flags & T8), qp, fenc_y, fdec_y, o, c)
    if cf:
        encode_chroma(bd, T, dec, int(cf == 2), qpc, fenc_c, fdec_c, o, c)
    for k, v in c.items():
        cnt[(tag, k)] += v
    if flags & T8:
        for idx in range(4):
            if not o.nnz[4 * idx]:
                o.level[4 * idx:4 * idx + 4] = 0
    else:
        o.level[:16][o.nnz[:16] == 0] = 0
    o.level[16:][o.nnz[16:] == 0] = 0
    for ch in range(2):
        if not o.nnz_dc[ch]:
            o.chroma_dc[ch] = 0
    return o


# ------------------------------------------------------------------ frames
def _mb_views(case, planes_y, planes_c, mb):
    """copies of macroblock mb's pixels in FENC / FDEC layout from [n, H, W] planes"""
    per = case.mbw * case.mbh
    f, r = divmod(mb, per)
    my, mx = divmod(r, case.mbw)
    ch = case.chroma_rows
    out = []
    for stride, (py, pc) in ((FENC, (planes_y[0], planes_c[0])), (FDEC, (planes_y[1], planes_c[1]))):
        y = np.zeros((16, stride), py.dtype)
        y[:, :16] = py[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
        c = np.zeros((16, stride), py.dtype)
        if case.cf:
            uv = pc[f, ch * my:ch * my + ch, 16 * mx:16 * mx + 16]
            c[:ch, :8] = uv[:, 0::2]
            c[:ch, stride // 2:stride // 2 + 8] = uv[:, 1::2]
        out += [y.reshape(-1), c.reshape(-1)]
    return f, my, mx, out


def _put_back(case, recon_y, recon_c, f, my, mx, fdec_y, fdec_c):
    ch = case.chroma_rows
    recon_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = fdec_y.reshape(16, FDEC)[:, :16]
    if case.cf:
        c = fdec_c.reshape(16, FDEC)
        recon_c[f, ch * my:ch * my + ch, 16 * mx:16 * mx + 16:2] = c[:ch, :8]
        recon_c[f, ch * my:ch * my + ch, 16 * mx + 1:16 * mx + 16:2] = c[:ch, 16:24]


def encode(case, dec, pred_y=None, pred_c=None):
    """the outputs of x264hip_*_mb_encode_inter for `case` with b_dct_decimate = dec, and the branch
    counters {(transform tag, branch): macroblocks}.  Elements of intra macroblocks are left at
    the initial value: recon = pred there, every array 0 except flags_out."""
    bd, cf = case.bd, case.cf
    T = tables(bd, case.cqm)
    pred_y = case.pred_y if pred_y is None else pred_y
    pred_c = case.pred_c if pred_c is None else pred_c
    cd = orc.coef_dtype(bd)
    n = case.nmb
    out = types.SimpleNamespace(
        recon_y=pred_y.copy(), recon_c=pred_c.copy() if cf else None, level=np.zeros((n, 48, 16), cd),
        chroma_dc=np.zeros((n, 2, 8), cd), nnz=np.zeros((n, 48), np.uint8), cbp=np.zeros(n, np.int32),
        nz=np.zeros(n, np.int32), flags_out=np.zeros(n, np.uint8), counters=collections.Counter())
    for mb in range(n):
        fl = int(case.flags[mb])
        if fl & INTRA:
            out.flags_out[mb] = fl
            continue
        qp = int(case.qp[mb])
        f, my, mx, (fenc_y, fenc_c, fdec_y, fdec_c) = _mb_views(case, (case.fenc_y, pred_y), (case.fenc_c, pred_c), mb)
        o = encode_mb(bd, T, cf, dec, fl, qp, int(case.qp_table[qp]), fenc_y, fdec_y, fenc_c, fdec_c, out.counters)
        _put_back(case, out.recon_y, out.recon_c, f, my, mx, fdec_y, fdec_c)
        out.level[mb], out.chroma_dc[mb], out.nnz[mb] = o.level, o.chroma_dc, o.nnz
        cbp = o.cbp_chroma << 4 | o.cbp_luma | o.nnz_dc[0] << 9 | o.nnz_dc[1] << 10
        out.cbp[mb] = cbp
        if fl & T8:
            out.nz[mb] = sum(int(o.nnz[4 * i]) << i for i in range(4))
        else:
            out.nz[mb] = sum(int(o.nnz[i]) << i for i in range(16))
        out.flags_out[mb] = (fl & 3) | (D16 if (fl & D16) and not cbp else 0)
    return out


@functools.lru_cache(maxsize=None)
def expected(key, dec):
    """encode(make_case(*key), dec), computed once per process and shared; do not modify"""
    return encode(make_case(*key), dec)


def _unzig(level, zig, w):
    d = np.zeros(w * w, level.dtype)
    for i, (y, x) in enumerate(zig):
        d[x * w + y] = level[i]
    return d


def decode(case, out, pred_y=None, pred_c=None):
    """The reconstruction a decoder derives from level / chroma_dc / mb_flags / qp alone: every
    block is un-zigzagged with the scans pinned in tests/golden/ref_tables.json, dequantised and
    inverse-transformed with the oracle's primitives and added to the prediction.  Chroma takes the
    one path of the standard (the inverse DC transform's values go to entry 0 of the 4x4 blocks,
    then the 4x4 inverse transform), never the encoder's DC-only shortcut."""
    bd, cf = case.bd, case.cf
    T = tables(bd, case.cqm)
    f_ = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    pred_y = case.pred_y if pred_y is None else pred_y
    pred_c = case.pred_c if pred_c is None else pred_c
    recon_y, recon_c = pred_y.copy(), pred_c.copy() if cf else None
    c422 = int(cf == 2)
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if fl & INTRA:
            continue
        qp = int(case.qp[mb])
        qpc = int(case.qp_table[qp])
        f, my, mx, (_, _, fdec_y, fdec_c) = _mb_views(case, (case.fenc_y, pred_y), (case.fenc_c, pred_c), mb)
        lev = out.level[mb]
        if fl & T8:
            for idx in range(4):
                l8 = np.ascontiguousarray(lev[4 * idx:4 * idx + 4].reshape(64))
                if l8.any():
                    d = _unzig(l8, ZIG8, 8)
                    f_("dequant_8x8")(A(d), A(T.dq8[CQM_8PY]), qp)
                    f_("add8x8_idct8")(A(fdec_y, 8 * (idx & 1) + 8 * (idx >> 1) * FDEC), A(d))
        else:
            for idx in range(16):
                if lev[idx].any():
                    d = _unzig(lev[idx], ZIG4, 4)
                    f_("dequant_4x4")(A(d), A(T.dq4[CQM_4PY]), qp)
                    i8, i4 = idx >> 2, idx & 3
                    f_("add4x4_idct")(A(fdec_y, (i8 & 1) * 8 + (i4 & 1) * 4 + ((i8 >> 1) * 8 + (i4 >> 1) * 4) * FDEC), A(d))
        for ch in range(2 if cf else 0):
            dcl = [int(v) for v in out.chroma_dc[mb][ch]]
            dcv = np.zeros((8, 16), cd)
            if c422:
                inv = [0] * 8
                for i, v in enumerate(zigzag_scan_2x4_dc(list(range(8)))):
                    inv[v] = dcl[i]
                dc = np.array(inv, cd)
                f_("idct_dequant_2x4_dc")(A(dc), A(dcv), A(T.dq4[CQM_4PC]), qpc + 3)
            else:
                inv = [0] * 4
                for i, v in enumerate(zigzag_scan_2x2_dc(list(range(4)))):
                    inv[v] = dcl[i]
                idct_dequant_2x2_dc(bd, inv, dcv, T.dq4[CQM_4PC], qpc)
            for k in range(8 if c422 else 4):
                idx = 16 + ch * 16 + (k >> 2) * 8 + (k & 3)
                d = np.zeros(16, cd)
                if lev[idx].any():
                    d = _unzig(lev[idx], ZIG4, 4)
                    f_("dequant_4x4")(A(d), A(T.dq4[CQM_4PC]), qpc)
                d[0] = dcv[k][0]
                f_("add4x4_idct")(A(fdec_c, 16 * ch + (k & 1) * 4 + (k >> 1) * 4 * FDEC), A(d))
        _put_back(case, recon_y, recon_c, f, my, mx, fdec_y, fdec_c)
    return recon_y, recon_c


# ------------------------------------------------------------------ inputs
# the residual classes of a macroblock (pred = fenc + residual)
ZERO, BUMP, NOISE, QUADS, CFLAT, CDC1, CHECKER = range(7)
SHAPES = ((1, 1, 1), (3, 1, 1), (5, 4, 2), (24, 14, 2))        # (mb_width, mb_height, frames)


def _qstep(qp):
    return 0.625 * 2.0 ** (qp / 6.0)


H4 = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]])        # the 4x4 core transform's rows


def _boundary_case(bd, cf, mbw, mbh, nframes, cqm, recipe, key):
    """one macroblock per entry (qp, mb_flags, rects, waves) of `recipe`: mid-grey fenc, pred = fenc +
    the rectangles (plane 0 / 1 / 2 = Y / U / V, y, x, h, w, amplitude) + the waves (plane, y, x, u, v,
    c: c * outer(H4[u], H4[v]) on the 4x4 block at y, x), added up.  A few flat patches and basis
    functions of a small whole amplitude quantise to a handful of +-1 levels, whose decimate scores
    add up to the small totals the reference compares with 4, 6 and 7, and put the chroma var2 / ssd
    exactly on the thresholds of the early-out.  BOUNDARY names what each entry pins."""
    n = nframes * mbw * mbh
    assert n == len(recipe)
    crows = {0: 0, 1: 8, 2: 16}[cf]
    grey = 128 << (bd - 8)
    res_y = np.zeros((nframes, 16 * mbh, 16 * mbw), np.int64)
    res_c = np.zeros((nframes, crows * mbh, 16 * mbw), np.int64)
    for mb, (q, fl, rects, waves) in enumerate(recipe):
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        mb_y = res_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
        mb_c = res_c[f, crows * my:crows * my + crows, 16 * mx:16 * mx + 16]
        planes = (mb_y, mb_c[:, 0::2], mb_c[:, 1::2])
        for plane, y, x, h, w, a in rects:
            if plane == 0 or cf:
                assert y + h <= planes[plane].shape[0] and x + w <= planes[plane].shape[1]
                planes[plane][y:y + h, x:x + w] += a
        for plane, y, x, u, v, c in waves:
            if plane == 0 or cf:
                assert y + 4 <= planes[plane].shape[0] and x + 4 <= planes[plane].shape[1]
                planes[plane][y:y + 4, x:x + 4] += c * np.outer(H4[u], H4[v])
    fenc_y, pred_y = np.full_like(res_y, grey), grey + res_y
    fenc_c, pred_c = (np.full_like(res_c, grey), grey + res_c) if cf else (None, None)
    pdt = orc.pixel_dtype(bd)
    pm = (1 << bd) - 1
    assert 0 <= pred_y.min() and pred_y.max() <= pm and (not cf or (0 <= pred_c.min() and pred_c.max() <= pm))
    return types.SimpleNamespace(
        bd=bd, cf=cf, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, cqm=cqm, chroma_rows=crows,
        fenc_y=fenc_y.astype(pdt), pred_y=pred_y.astype(pdt), fenc_c=fenc_c.astype(pdt) if cf else None,
        pred_c=pred_c.astype(pdt) if cf else None, qp=np.array([r[0] for r in recipe], np.int8),
        flags=np.array([r[1] for r in recipe], np.uint8), klass=np.full(n, -1, np.int32), qp_table=chroma_qp_table(bd),
        key=key)


@functools.lru_cache(maxsize=None)
def make_case(bd, cf, mbw, mbh, nframes, cqm="flat", seed=0, recipe=None):
    """recipe "boundary": the boundary macroblocks of BOUNDARY (or a recipe itself), see
    _boundary_case.  Otherwise:
    Seeded inputs.  fenc is synthetic texture; pred = fenc + a per-macroblock residual class:
    zero; one isolated bump of +-1..2 quantiser steps; noise scaled to the macroblock's qp; noise
    with a strength per 8x8 quadrant (nothing / a faint flat patch / strong), which is what takes
    the per-8x8 and per-macroblock decimation apart; a flat chroma offset; a +-1 chroma DC at low
    qp; a full-scale 0 / max checker at qp 0 and at qp_max_spec.  qp varies per macroblock over
    0..qp_max_spec; mb_flags mixes transform 4 / 8, D_16x16, skip and intra."""
    if recipe is not None:
        return _boundary_case(bd, cf, mbw, mbh, nframes, cqm, boundary_recipe(cf, cqm)[2] if recipe == "boundary" else recipe,
                              (bd, cf, mbw, mbh, nframes, cqm, seed, recipe))
    rng = np.random.default_rng([bd, cf, mbw, mbh, nframes, seed, 264])
    pm, qmax = (1 << bd) - 1, qp_max_spec(bd)
    scale = 1 << (bd - 8)
    n = nframes * mbw * mbh
    W, H = 16 * mbw, 16 * mbh
    crows = {0: 0, 1: 8, 2: 16}[cf]
    yy, xx = np.mgrid[0:H, 0:W]

    def texture(h, w, f, k):
        y, x = np.mgrid[0:h, 0:w]
        t = 128 + 60 * np.sin(x / (5.0 + k) + f) * np.cos(y / (7.0 + k)) + 0.4 * (x - y) + rng.normal(0, 6, (h, w))
        return np.clip(np.rint(t * scale), 0, pm)

    fenc_y = np.stack([texture(H, W, f, 0) for f in range(nframes)]).astype(np.int64)
    fenc_c = np.stack([texture(crows * mbh, W, f, 3) for f in range(nframes)]).astype(np.int64) if cf else None
    res_y = np.zeros_like(fenc_y)
    res_c = np.zeros_like(fenc_c) if cf else None
    qp = np.zeros(n, np.int8)
    flags = np.zeros(n, np.uint8)
    klass = np.zeros(n, np.int32)
    for mb in range(n):
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        k = int(rng.choice([ZERO, BUMP, NOISE, NOISE, QUADS, QUADS, QUADS, CFLAT, CFLAT, CDC1, CDC1, CHECKER]))
        if n <= 3:
            k = (NOISE, QUADS, CFLAT)[mb % 3]
        q = int(rng.integers(0, qmax + 1))
        if k == CDC1:
            q = int(rng.integers(0, 18 + 6 * (bd - 8)))
        if k == CHECKER:
            q = int(rng.choice([0, qmax]))
        fl = (T8 if rng.random() < 0.5 else 0) | (D16 if rng.random() < 0.5 else 0)
        u = rng.random()
        if n > 3 and u < 0.08:
            fl |= INTRA
        elif n > 3 and u < 0.16:
            fl |= SKIP
        qp[mb], flags[mb], klass[mb] = q, fl, k
        qs = _qstep(q)
        ys, cs = slice(16 * my, 16 * my + 16), slice(crows * my, crows * my + crows)
        xs = slice(16 * mx, 16 * mx + 16)
        ry = np.zeros((16, 16))
        rc = np.zeros((crows, 16))
        if k == BUMP:
            ry[rng.integers(16), rng.integers(16)] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(1, 2)))
            if cf:
                rc[rng.integers(crows), rng.integers(16)] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(1, 2)))
        elif k == NOISE:
            a = qs * rng.choice([0.25, 0.5, 1.0, 2.0, 4.0])
            ry = rng.normal(0, a, (16, 16))
            rc = rng.normal(0, a * rng.choice([0.25, 1.0]), (crows, 16))
        elif k == QUADS:
            for i8 in range(4):
                sl = (slice(8 * (i8 >> 1), 8 * (i8 >> 1) + 8), slice(8 * (i8 & 1), 8 * (i8 & 1) + 8))
                m = rng.choice(3, p=[0.35, 0.4, 0.25])
                if m == 1:        # a faint flat 4x4 patch: one small level
                    y0, x0 = 4 * rng.integers(2), 4 * rng.integers(2)
                    ry[sl][y0:y0 + 4, x0:x0 + 4] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(0.45, 0.8)))
                elif m == 2:
                    ry[sl] = rng.normal(0, qs * rng.choice([1.0, 3.0]), (8, 8))
            rc = rng.normal(0, qs * rng.choice([0.1, 0.3, 0.6]), (crows, 16))
        elif k == CFLAT:
            ry = rng.normal(0, qs * 0.3, (16, 16))
            if cf:
                rc[:, 0::2] = rng.choice([-1, 1]) * max(1, round(qs * rng.choice([0.2, 0.5, 1.0, 3.0])))
                rc[:, 1::2] = rng.choice([-1, 0, 1]) * max(1, round(qs * rng.choice([0.2, 0.5, 1.0])))
        elif k == CDC1:
            if cf:
                y0, x0 = 4 * rng.integers(crows // 4), 8 * rng.integers(2)
                rc[y0:y0 + 4, x0 + rng.integers(2):x0 + 8:2] = rng.choice([-1, 1])
                if rng.random() < 0.5:
                    rc[:, rng.integers(2)::2] += rng.choice([-1, 1])
        res_y[f, ys, xs] = np.rint(ry)
        if cf:
            res_c[f, cs, xs] = np.rint(rc)
        if k == CHECKER:
            chk = ((yy[ys, xs] + xx[ys, xs]) & 1) * pm
            fenc_y[f, ys, xs] = chk
            res_y[f, ys, xs] = pm - 2 * chk                       # pred = the inverse checker
            if cf:
                cy, cx = np.mgrid[0:crows, 0:16]
                chk = ((cy + (cx >> 1)) & 1) * pm
                fenc_c[f, cs, xs] = chk
                res_c[f, cs, xs] = pm - 2 * chk
    pdt = orc.pixel_dtype(bd)
    case = types.SimpleNamespace(
        bd=bd, cf=cf, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, cqm=cqm, chroma_rows=crows,
        fenc_y=fenc_y.astype(pdt), pred_y=np.clip(fenc_y + res_y, 0, pm).astype(pdt),
        fenc_c=fenc_c.astype(pdt) if cf else None,
        pred_c=np.clip(fenc_c + res_c, 0, pm).astype(pdt) if cf else None,
        qp=qp, flags=flags, klass=klass, qp_table=chroma_qp_table(bd), key=(bd, cf, mbw, mbh, nframes, cqm, seed))
    return case


def case_keys(bd, cf):
    """the case list of one (bit depth, chroma format): every shape with the flat matrices"""
    return [(bd, cf, w, h, n, "flat", 0) for w, h, n in SHAPES]


# The boundary macroblocks: (what is pinned, chroma formats, (qp, mb_flags, rects, waves)).  Each puts one
# comparison of the reference exactly on its bound (the counters of encode() say so, and
# tests/test_cpu_mbenc.py asserts it); the flipped comparison (tests/mutants.py) gives other bytes on
# the ones marked *.  They were found by search over a few rectangles and waves per macroblock.
_U422 = (1, 0, 0, 16, 8)
_RAMP420 = ((1, 4, 4, 4, 1, 2), (1, 4, 7, 4, 1, -2), (1, 4, 5, 1, 2, 3), (1, 5, 5, 1, 2, 1), (1, 6, 5, 1, 2, -2), (1, 7, 5, 1, 2, -4),
            (1, 4, 5, 4, 1, 1))
# (with the flat matrices no 4:2:0 plane whose ssd is at most thresh has a DC that quantises to a level, at any
# chroma qp from 18 up: the least ssd for one, sum^2 / 64, is above thresh.  The JVT matrices quantise the DC finer.)
BOUNDARY = (
    ("8x8 transform, decimate_score64 of a block = 4 *", (0, 1, 2), (22, T8, ((0, 4, 0, 4, 4, 9),), ((0, 8, 0, 2, 0, 4),))),
    ("8x8 transform, macroblock score = 6 *", (0, 1, 2), (17, T8, ((0, 8, 12, 4, 4, 2),), ())),
    ("8x8 transform, macroblock score = 6 at qp 30 *", (0, 1, 2), (30, T8, (), ((0, 0, 12, 2, 1, 9),))),
    ("4x4 transform, score of an 8x8 = 4 *", (0, 1, 2), (17, 0, ((0, 4, 12, 4, 4, 2),), ((0, 4, 8, 0, 2, -1), (0, 0, 0, 1, 0, 3)))),
    ("4x4 transform, macroblock score = 6 *", (0, 1, 2), (17, 0, ((0, 4, 0, 4, 4, -2),), ((0, 0, 12, 0, 2, -1), (0, 0, 0, 0, 1, 1)))),
    ("chroma score = 7 at 4:2:0 *", (1,), (22, 0, (), ((1, 4, 0, 0, 1, 2), (1, 4, 4, 2, 0, -3), (1, 0, 4, 2, 0, 3)))),
    ("chroma score = 7 at 4:2:2 *", (2,), (19, 0, (), ((1, 4, 4, 2, 0, -2), (1, 4, 4, 0, 1, -1), (1, 4, 0, 2, 0, -2)))),
    ("chroma qp 17: no early-out", (1, 2), (17, 0, (), ((1, 0, 4, 1, 1, -1),))),
    ("chroma qp = 18: the early-out drops what the full path codes *", (1, 2), (18, 0, (), ((1, 0, 4, 1, 1, -1),))),
    ("chroma qp 19", (1, 2), (19, 0, (), ((1, 0, 4, 1, 1, -1),))),
    ("var2 = 4 * thresh = 92 at 4:2:0, qp 20: two flat columns round a ramp *", (1,), (20, 0, _RAMP420, ())),
    ("ssd of U = thresh = 36 at 4:2:0, qp 22, JVT matrices: a DC the early-out must not code *", (1,),
     (22, 0, tuple((1, 4 * (b >> 1), 4 * (b & 1), 3, 3, 1) for b in range(4)), ()), "jvt"),
    ("var2 = 4 * thresh at 4:2:2, qp 18 *", (2,), (18, 0, (), ((1, 0, 4, 1, 1, 1), (1, 0, 0, 2, 0, 1)))),
    ("ssd of U = thresh at 4:2:2, qp 25: a DC the early-out must not code *", (2,),
     (25, 0, (_U422 + (1,), (1, 0, 2, 1, 1, -1), (1, 2, 7, 1, 1, 3), (1, 5, 2, 1, 1, 1)), ())),
    ("chroma DC dmf 1792 < 32 * 64 at 4:2:2 (qp 18 + 3)", (2,), (18, 0, (_U422 + (-1,),), ())),
    ("chroma DC dmf = 32 * 64 at 4:2:2 (qp 19 + 3): optimised *", (2,), (19, 0, (_U422 + (-1,),), ())),
    ("chroma DC dmf 2304 at 4:2:2 (qp 20 + 3): not optimised", (2,), (20, 0, (_U422 + (-1,),), ())),
    ("chroma DC dmf = 32 * 64 at 4:2:0 (qp 22)", (1,), (22, 0, ((1, 0, 0, 8, 8, -2),), ())),
)


def boundary_recipe(cf, cqm="flat"):
    """the boundary macroblocks of chroma format cf and the matrices cqm as one picture: (mbw, mbh,
    recipe, names)"""
    rows = [(b[0], b[2]) for b in BOUNDARY if cf in b[1] and (b[3:] or ("flat",))[0] == cqm]
    mbw = min(5, len(rows))
    mbh = -(-len(rows) // mbw)
    rows += [("filler", (26, 0, (), ()))] * (mbw * mbh - len(rows))
    return mbw, mbh, tuple(e for _, e in rows), [n for n, _ in rows]


def boundary_keys():
    """one picture per (bit depth, chroma format); at 10 bit the same residuals at the same qp meet
    the same quantiser (the tables hold QP_BD_OFFSET), with pixels two bits wider"""
    keys = []
    for bd in (8, 10):
        for cf, cqm in ((0, "flat"), (1, "flat"), (2, "flat"), (1, "jvt")):
            mbw, mbh, _, _ = boundary_recipe(cf, cqm)
            keys.append((bd, cf, mbw, mbh, 1, cqm, 0, "boundary"))
    return keys


def jvt_keys():
    return [(bd, cf, 5, 4, 2, "jvt", 0) for bd in (8, 10) for cf in (1, 2)]


GPU_GROUPS = ("shapes", "jvt", "boundary")


def gpu_keys(group=None, **where):
    """every (key, dec) tests/test_gpu_mbenc.py compares with the device byte for byte, which is the
    list the boundary mutants of tests/test_cpu_mutants.py are held to.  group: one of GPU_GROUPS
    (one test function each); where: bd / cf / dec of one parametrised case of that function."""
    keys = {"shapes": [(k, dec) for bd in (8, 10) for cf in (0, 1, 2) for dec in (0, 1) for k in case_keys(bd, cf)],
            "jvt": [(k, 1) for k in jvt_keys()],
            "boundary": [(k, 1) for k in boundary_keys()]}
    keys = [kd for g in GPU_GROUPS if group in (None, g) for kd in keys[g]]
    pick = {"bd": lambda kd: kd[0][0], "cf": lambda kd: kd[0][1], "dec": lambda kd: kd[1]}
    return [kd for kd in keys if all(pick[n](kd) == v for n, v in where.items())]


def key_size(kd):
    """macroblocks of a gpu_keys() entry: what its expected() costs"""
    return kd[0][2] * kd[0][3] * kd[0][4]
