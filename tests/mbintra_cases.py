"""The intra macroblock encode restated per macroblock, from the reference's C
(encoder/macroblock.c:126-239, 706-768, 924-951, encoder/macroblock.h:132-213 and
mb_encode_chroma_internal, macroblock.c:259-490, with b_inter = 0; no lossless / trellis / noise
reduction / i_skip_intra), and the inputs of tests/test_cpu_mbintra.py and
tests/test_gpu_mbintra.py.  No GPU code.  The method is tests/mbenc_cases.py's:

* Only the control flow is restated: every transform, quantiser, scan and score is the oracle's
  (tests/oracle_lib.py), called on FENC / FDEC-layout buffers exactly as x264 calls its tables.
* Prediction: where the oracle has the mode it is the oracle's (predict_8x8_filter, predict_8x8
  modes 0..8, 4x4 / 16x16 V, H, DC, chroma DC, H, V, the 8x8c plane mode).  The rest is restated
  here from common/predict.c: the 4x4 directional modes (:534-630, pinned by
  tests/golden/intra4x4_golden.npz), 16x16 P (:132-160), 8x16c P (:443-469) and every
  _dc_left / _dc_top / _dc_128 variant (:80-103, 167-220, 314-360, 481-494, 700-715).
* encode(case, dec) runs mbenc_cases.encode (the inter macroblocks), then the raster loop over the
  intra macroblocks in place; it returns the outputs of include/x264hip_mbintra.h plus branch
  counters, so the coverage of the inputs can be asserted.
* decode(case, out) rebuilds the reconstruction from the outputs alone, as a decoder would.
* make_case: mbenc_cases.make_case's inputs plus the type bits and the modes, drawn only from the
  modes valid at each position; all_intra marks every macroblock intra (an I picture).
"""
import functools
import types

import numpy as np

import mbenc_cases as mc
import oracle_lib as orc

INTRA, T8, I16 = mc.INTRA, mc.T8, 16
CQM_4IY, CQM_4IC, CQM_8IY = 0, 2, 0                              # reference common/set.h
MB_LEFT, MB_TOP, MB_TOPRIGHT, MB_TOPLEFT = 1, 2, 4, 8            # common/macroblock.h:33-36
# x264_pred_i4x4_neighbors, common/macroblock.h:43-57
PRED4_NEIGHBORS = (MB_TOP, MB_LEFT, MB_LEFT | MB_TOP, MB_TOP | MB_TOPRIGHT, MB_LEFT | MB_TOPLEFT | MB_TOP,
                   MB_LEFT | MB_TOPLEFT | MB_TOP, MB_LEFT | MB_TOPLEFT | MB_TOP, MB_TOP | MB_TOPRIGHT, MB_LEFT, MB_LEFT,
                   MB_TOP, 0)
BLOCK_IDX_XY_1D = (0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15)   # common/macroblock.h:217-220
FENC, FDEC = mc.FENC, mc.FDEC
A = orc._addr
# the FDEC-layout buffers of one macroblock: pixel (0,0) at OY (chroma: U at OY, V at OY + 16), so
# that the row above, the column left and the top-right samples are inside the buffer
OY = FDEC + 8
BUF = 18 * FDEC
KIND = {"4x4": 0, "8x8c": 1, "8x16c": 2, "16x16": 3}              # the oracle's predict( kind, ... )


def block_xy(idx):
    """(bx, by) of 4x4 block idx of h->dct.luma4x4's order"""
    return (idx >> 2 & 1) * 2 + (idx & 1), (idx >> 3) * 2 + (idx >> 1 & 1)


def mb_neighbours(mx, my, mbw):
    """i_neighbour_intra of a picture with one slice and no constrained intra prediction"""
    n = (MB_LEFT if mx > 0 else 0) | (MB_TOP if my > 0 else 0)
    if mx > 0 and my > 0:
        n |= MB_TOPLEFT
    if my > 0 and mx + 1 < mbw:
        n |= MB_TOPRIGHT
    return n


def neighbour4(idx, nb):
    """i_neighbour4[idx], common/macroblock.c:489-498, 1340-1351"""
    top = nb & MB_TOP
    if idx == 0:
        return (nb & (MB_TOP | MB_LEFT | MB_TOPLEFT)) | (MB_TOPRIGHT if top else 0)
    if idx in (1, 4):
        return MB_LEFT | ((MB_TOP | MB_TOPLEFT | MB_TOPRIGHT) if top else 0)
    if idx in (2, 8, 10):
        return MB_TOP | MB_TOPRIGHT | ((MB_LEFT | MB_TOPLEFT) if nb & MB_LEFT else 0)
    if idx == 5:
        return MB_LEFT | (nb & MB_TOPRIGHT) | ((MB_TOP | MB_TOPLEFT) if top else 0)
    if idx in (6, 9, 12, 14):
        return MB_LEFT | MB_TOP | MB_TOPLEFT | MB_TOPRIGHT
    return MB_LEFT | MB_TOP | MB_TOPLEFT


def neighbour8(idx, nb):
    """i_neighbour8[idx], common/macroblock.c:498, 1340-1351"""
    return (neighbour4(0, nb), neighbour4(5, nb), neighbour4(2, nb), MB_LEFT | MB_TOP | MB_TOPLEFT)[idx]


# ------------------------------------------------------------------ prediction (common/predict.c)
def F1(a, b):
    return (a + b + 1) >> 1


def F2(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def pred4x4_dir(mode, n):
    """predict_4x4_{ddl,ddr,vr,hd,vl,hu}_c (predict.c:534-621) in closed form; n: the 13
    neighbours t0..t7, l0..l3, lt.  Returns [4][4] (row, column)."""
    t, lf, lt = [int(v) for v in n[0:8]], [int(v) for v in n[8:12]], int(n[12])
    e = [lf[3], lf[2], lf[1], lf[0], lt] + t[:4]                 # l3 .. l0, lt, t0 .. t3
    p = np.zeros((4, 4), np.int64)
    for y in range(4):
        for x in range(4):
            if mode == 3:
                z = x + y
                v = F2(t[z], t[z + 1], t[min(z + 2, 7)])
            elif mode == 4:
                c = 4 + x - y
                v = F2(e[c - 1], e[c], e[c + 1])
            elif mode == 5:
                z = 2 * x - y
                if z < 0:
                    v = F2(e[4 + z], e[5 + z], e[6 + z])
                elif z % 2 == 0:
                    v = F1(e[4 + z // 2], e[5 + z // 2])
                else:
                    v = F2(e[4 + z // 2], e[5 + z // 2], e[6 + z // 2])
            elif mode == 6:
                z = 2 * y - x
                if z < 0:
                    v = F2(e[2 - z], e[3 - z], e[4 - z])
                elif z % 2 == 0:
                    v = F1(e[4 - z // 2], e[3 - z // 2])
                else:
                    v = F2(e[4 - z // 2], e[3 - z // 2], e[2 - z // 2])
            elif mode == 7:
                c = x + (y >> 1)
                v = F2(t[c], t[c + 1], t[c + 2]) if y & 1 else F1(t[c], t[c + 1])
            else:
                z = x + 2 * y
                c = z >> 1
                if z > 5:
                    v = lf[3]
                elif z == 5:
                    v = F2(lf[2], lf[3], lf[3])
                else:
                    v = F2(lf[c], lf[c + 1], lf[c + 2]) if z & 1 else F1(lf[c], lf[c + 1])
            p[y, x] = v
    return p


def _px(buf, off, x, y):
    return int(buf[off + x + y * FDEC])


def _put(buf, off, w, h, block):
    """a w x h block (or one value) to the FDEC-layout buffer at element offset off"""
    buf[off:off + h * FDEC].reshape(h, FDEC)[:, :w] = block


def _plane(bd, buf, off, w, h, a, b, c, xo, yo):
    """the plane modes' last loop: clip( (a - xo*b - yo*c + 16 + b*x + c*y) >> 5 )"""
    yy, xx = np.mgrid[0:h, 0:w]
    _put(buf, off, w, h, np.clip((a - xo * b - yo * c + 16 + b * xx + c * yy) >> 5, 0, (1 << bd) - 1))


def predict(bd, kind, mode, buf, off):
    """predict_4x4 / predict_16x16 / predict_chroma [mode] on the FDEC-layout buffer at element
    offset off, x264's mode numbers (common/predict.h:36-82)"""
    S = lambda x, y: _px(buf, off, x, y)
    half = 1 << (bd - 1)
    if kind == "4x4":
        if mode <= 2:
            orc.fn(bd, "predict")(KIND[kind], mode, A(buf, off))
        elif mode <= 8:
            n = [S(x, -1) for x in range(8)] + [S(-1, y) for y in range(4)] + [S(-1, -1)]
            _put(buf, off, 4, 4, pred4x4_dir(mode, n))
        elif mode == 9:                                          # predict.c:485-489
            _put(buf, off, 4, 4, (sum(S(-1, y) for y in range(4)) + 2) >> 2)
        elif mode == 10:                                         # :490-494
            _put(buf, off, 4, 4, (sum(S(x, -1) for x in range(4)) + 2) >> 2)
        else:
            _put(buf, off, 4, 4, half)
    elif kind == "16x16":
        if mode <= 2:
            orc.fn(bd, "predict")(KIND[kind], mode, A(buf, off))
        elif mode == 3:                                          # predict.c:132-160
            H = sum((i + 1) * (S(8 + i, -1) - S(6 - i, -1)) for i in range(8))
            V = sum((i + 1) * (S(-1, 8 + i) - S(-1, 6 - i)) for i in range(8))
            _plane(bd, buf, off, 16, 16, 16 * (S(-1, 15) + S(15, -1)), (5 * H + 32) >> 6, (5 * V + 32) >> 6, 7, 7)
        elif mode == 4:                                          # :80-89
            _put(buf, off, 16, 16, (sum(S(-1, y) for y in range(16)) + 8) >> 4)
        elif mode == 5:                                          # :90-99
            _put(buf, off, 16, 16, (sum(S(x, -1) for x in range(16)) + 8) >> 4)
        else:
            _put(buf, off, 16, 16, half)
    else:
        h = 8 if kind == "8x8c" else 16
        if mode <= 2 or (mode == 3 and h == 8):
            orc.fn(bd, "predict")(KIND[kind], mode, A(buf, off))
        elif mode == 3:                                          # predict_8x16c_p_c, predict.c:443-469
            H = sum((i + 1) * (S(4 + i, -1) - S(2 - i, -1)) for i in range(4))
            V = sum((i + 1) * (S(-1, 8 + i) - S(-1, 6 - i)) for i in range(8))
            _plane(bd, buf, off, 8, 16, 16 * (S(-1, 15) + S(7, -1)), (17 * H + 16) >> 5, (5 * V + 32) >> 6, 3, 7)
        elif mode == 4:                                          # :176-201, 323-341: per four rows
            for i in range(h // 4):
                _put(buf, off + 4 * i * FDEC, 8, 4, (sum(S(-1, 4 * i + y) for y in range(4)) + 2) >> 2)
        elif mode == 5:                                          # :202-220, 342-360: per four columns
            for i in range(2):
                _put(buf, off + 4 * i, 4, h, (sum(S(4 * i + x, -1) for x in range(4)) + 2) >> 2)
        else:
            _put(buf, off, 8, h, half)


def predict8x8(bd, mode, n8, buf, off, cnt=None):
    """predict_8x8_filter with x264_pred_i4x4_neighbors[mode], then predict_8x8[mode]
    (encoder/macroblock.h:178-190); the DC variants from predict.c:700-715"""
    filters = PRED4_NEIGHBORS[mode]
    if cnt is not None:
        if filters & (MB_LEFT | MB_TOP):
            cnt["have_lt", bool(n8 & MB_TOPLEFT)] += 1
        if filters & MB_TOP:
            cnt["have_tr", bool(n8 & MB_TOPRIGHT)] += 1
    edge = orc.predict_8x8_filter(bd, buf, off, n8, filters)
    if mode <= 8:
        blk = orc.predict_8x8(bd, mode, edge)
    elif mode == 9:
        blk = (sum(int(v) for v in edge[7:15]) + 4) >> 3
    elif mode == 10:
        blk = (sum(int(v) for v in edge[16:24]) + 4) >> 3
    else:
        blk = 1 << (bd - 1)
    _put(buf, off, 8, 8, blk)


# ------------------------------------------------------------------ the macroblock
class MbOut(mc.MbOut):
    def __init__(self, bd):
        super().__init__(bd)
        self.luma_dc = np.zeros(16, orc.coef_dtype(bd))
        self.nnz_ldc = 0


def encode_i16x16(bd, T, dec, qp, mode, fenc, fdec, o, cnt):
    """mb_encode_i16x16, macroblock.c:126-239"""
    f = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    dct4x4 = np.zeros((16, 16), cd)
    dct_dc = np.zeros(16, cd)
    decimate_score = 0 if dec else 9
    block_cbp = 0
    predict(bd, "16x16", mode, fdec, OY)
    f("sub16x16_dct")(A(dct4x4), A(fenc), A(fdec, OY))
    for idx in range(16):
        dct_dc[BLOCK_IDX_XY_1D[idx]] = dct4x4[idx][0]
        dct4x4[idx][0] = 0
    mf, bias = T.q4m[CQM_4IY][qp], T.q4b[CQM_4IY][qp]
    for i8 in range(4):
        nz = f("quant_4x4x4")(A(dct4x4[4 * i8]), A(mf), A(bias))
        if nz:
            block_cbp = 0xf
            for i4 in mc._bits(nz, 4):
                idx = 4 * i8 + i4
                f("zigzag_scan_4x4")(0, A(o.level[idx]), A(dct4x4[idx]))
                f("dequant_4x4")(A(dct4x4[idx]), A(T.dq4[CQM_4IY]), qp)
                if decimate_score < 6:
                    decimate_score += f("decimate_score15")(A(o.level[idx]))
                o.nnz[idx] = 1
    if dec and block_cbp:
        cnt["i16_score", mc._side(decimate_score, 6)] += 1
    if decimate_score < 6:
        if block_cbp:
            cnt["i16_decimated"] += 1
        o.nnz[:16] = 0                                            # CLEAR_16x16_NNZ
        block_cbp = 0
    else:
        o.cbp_luma |= block_cbp
    f("dct4x4dc")(A(dct_dc))
    nz = f("quant_4x4_dc")(A(dct_dc), int(mf[0]) >> 1, int(bias[0]) << 1)
    o.nnz_ldc = int(nz != 0)
    if nz:
        f("zigzag_scan_4x4")(0, A(o.luma_dc), A(dct_dc))
        f("idct4x4dc")(A(dct_dc))
        f("dequant_4x4_dc")(A(dct_dc), A(T.dq4[CQM_4IY]), qp)
        if block_cbp:
            for i in range(16):
                dct4x4[i][0] = dct_dc[BLOCK_IDX_XY_1D[i]]
    if block_cbp:
        f("add16x16_idct")(A(fdec, OY), A(dct4x4))
        cnt["i16_idct_dc" if nz else "i16_idct_nodc"] += 1
    elif nz:
        f("add16x16_idct_dc")(A(fdec, OY), A(dct_dc))
        cnt["i16_dc_only"] += 1
    else:
        cnt["i16_pred_only"] += 1


def encode_i4x4(bd, T, qp, modes, nb, fenc, fdec, o, cnt):
    """macroblock.c:738-768 and x264_mb_encode_i4x4, encoder/macroblock.h:132-166"""
    f = lambda name: orc.fn(bd, name)
    dct = np.zeros(16, orc.coef_dtype(bd))
    for idx in range(16):
        bx, by = block_xy(idx)
        off = OY + 4 * bx + 4 * by * FDEC
        n4 = neighbour4(idx, nb)
        if n4 & MB_TOP:
            emulate = (n4 & (MB_TOPRIGHT | MB_TOP)) == MB_TOP
            cnt["topright_emulated" if emulate else "topright_real"] += 1
            if emulate:
                fdec[off + 4 - FDEC:off + 8 - FDEC] = fdec[off + 3 - FDEC]
        cnt["mode4", int(modes[idx])] += 1
        predict(bd, "4x4", int(modes[idx]), fdec, off)
        f("sub4x4_dct")(A(dct), A(fenc, 4 * bx + 4 * by * FENC), A(fdec, off))
        nz = f("quant_4x4")(A(dct), A(T.q4m[CQM_4IY][qp]), A(T.q4b[CQM_4IY][qp]))
        o.nnz[idx] = nz
        if nz:
            o.cbp_luma |= 1 << (idx >> 2)
            f("zigzag_scan_4x4")(0, A(o.level[idx]), A(dct))
            f("dequant_4x4")(A(dct), A(T.dq4[CQM_4IY]), qp)
            f("add4x4_idct")(A(fdec, off), A(dct))


def encode_i8x8(bd, T, qp, modes, nb, fenc, fdec, o, cnt):
    """macroblock.c:713-737 and x264_mb_encode_i8x8, encoder/macroblock.h:168-213"""
    f = lambda name: orc.fn(bd, name)
    dct = np.zeros(64, orc.coef_dtype(bd))
    for idx in range(4):
        x, y = idx & 1, idx >> 1
        off = OY + 8 * x + 8 * y * FDEC
        mode = int(modes[4 * idx])
        cnt["mode8", mode] += 1
        predict8x8(bd, mode, neighbour8(idx, nb), fdec, off, cnt)
        f("sub8x8_dct8")(A(dct), A(fenc, 8 * x + 8 * y * FENC), A(fdec, off))
        nz = f("quant_8x8")(A(dct), A(T.q8m[CQM_8IY][qp]), A(T.q8b[CQM_8IY][qp]))
        if nz:
            o.cbp_luma |= 1 << idx
            lev = o.level[4 * idx:4 * idx + 4].reshape(64)
            f("zigzag_scan_8x8")(0, A(lev), A(dct))
            f("dequant_8x8")(A(dct), A(T.dq8[CQM_8IY]), qp)
            f("add8x8_idct8")(A(fdec, off), A(dct))
            o.nnz[4 * idx:4 * idx + 4] = 1                        # STORE_8x8_NNZ


def encode_chroma(bd, T, c422, qp, mode, fenc, fdec, o, cnt):
    """macroblock.c:924-941, then mb_encode_chroma_internal (:259-490) with b_inter = 0: no early
    termination, i_decimate_score starts at 7.  fenc [16*16] (U, V at +8); fdec: U at OY, V at
    OY + 16; qp is the chroma qp"""
    f = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    dequant_mf = T.dq4[CQM_4IC]
    dct_dc = np.zeros(8, cd)
    qdc = qp + 3 * c422
    dc_mf, dc_bias = int(T.q4m[CQM_4IC][qdc][0]) >> 1, int(T.q4b[CQM_4IC][qdc][0]) << 1
    kind = "8x16c" if c422 else "8x8c"
    cnt["modec", mode] += 1
    for ch in range(2):
        predict(bd, kind, mode, fdec, OY + 16 * ch)
    tails = set()
    for ch in range(2):
        p_src, p_dst = 8 * ch, OY + 16 * ch
        nz_ac = 0
        dct4x4 = np.zeros((8, 16), cd)
        for i in range(c422 + 1):
            f("sub8x8_dct")(A(dct4x4[4 * i]), A(fenc, p_src + 8 * i * FENC), A(fdec, p_dst + 8 * i * FDEC))
        dct_dc[:] = 0
        if c422:
            f("dct2x4dc")(A(dct_dc), A(dct4x4))
        else:
            mc.dct2x2dc(bd, dct_dc, dct4x4)
        for i8x8 in range(c422 + 1):
            nz = f("quant_4x4x4")(A(dct4x4[4 * i8x8]), A(T.q4m[CQM_4IC][qp]), A(T.q4b[CQM_4IC][qp]))
            nz_ac |= nz
            for i4x4 in mc._bits(nz, 4):
                idx = 16 + ch * 16 + i8x8 * 8 + i4x4
                f("zigzag_scan_4x4")(0, A(o.level[idx]), A(dct4x4[i8x8 * 4 + i4x4]))
                f("dequant_4x4")(A(dct4x4[i8x8 * 4 + i4x4]), A(dequant_mf), qp)
                o.nnz[idx] = 1
        nz_dc = 0
        for i in range(c422 + 1):
            nz_dc |= f("quant_2x2_dc")(A(dct_dc, 4 * i), dc_mf, dc_bias)
        o.nnz_dc[ch] = int(nz_dc != 0)
        if not nz_ac:                                             # (i_decimate_score = 7: never decimated)
            o.nnz[16 + 16 * ch:32 + 16 * ch] = 0
            if not nz_dc:
                tails.add("empty")
                continue
            if not mc.mb_optimize_chroma_dc(bd, dct_dc, dequant_mf, qdc, c422, cnt):
                o.nnz_dc[ch] = 0
                tails.add("empty")
                continue
            if c422:
                o.chroma_dc[ch][:] = mc.zigzag_scan_2x4_dc(dct_dc)
                f("idct_dequant_2x4_dconly")(A(dct_dc), A(dequant_mf), qp + 3)
            else:
                o.chroma_dc[ch][:4] = mc.zigzag_scan_2x2_dc(dct_dc)
                mc.idct_dequant_2x2_dconly(bd, dct_dc, dequant_mf, qp)
            for i in range(c422 + 1):
                f("add8x8_idct_dc")(A(fdec, p_dst + 8 * i * FDEC), A(dct_dc, 4 * i))
            tails.add("dconly")
        else:
            o.cbp_chroma = 1
            tails.add("dcac")
            if nz_dc:
                if c422:
                    o.chroma_dc[ch][:] = mc.zigzag_scan_2x4_dc(dct_dc)
                    f("idct_dequant_2x4_dc")(A(dct_dc), A(dct4x4), A(dequant_mf), qp + 3)
                else:
                    o.chroma_dc[ch][:4] = mc.zigzag_scan_2x2_dc(dct_dc)
                    mc.idct_dequant_2x2_dc(bd, dct_dc, dct4x4, dequant_mf, qp)
            for i in range(c422 + 1):
                f("add8x8_idct")(A(fdec, p_dst + 8 * i * FDEC), A(dct4x4[4 * i]))
    for t in tails:
        cnt["chroma_" + t] += 1
    o.cbp_chroma += o.nnz_dc[0] | o.nnz_dc[1] | o.cbp_chroma        # macroblock.c:487-489


def mb_type(fl, have8=True):
    """'i8' / 'i16' / 'i4' of an intra macroblock's mb_flags (include/x264hip_mbintra.h)"""
    if fl & T8:
        return "i8" if have8 else "i4as8"
    return "i16" if fl & I16 else "i4"


def encode_mb(bd, T, cf, dec, fl, qp, qpc, modes, cmode, nb, fenc_y, fdec_y, fenc_c, fdec_c, cnt):
    """one intra macroblock; the fdec buffers hold the neighbours around OY and get the
    reconstruction.  Returns MbOut with the levels of every block whose nnz is 0 cleared."""
    o = MbOut(bd)
    kind = mb_type(fl)
    cnt["type", kind] += 1
    if kind == "i16":
        cnt["mode16", int(modes[0])] += 1
        encode_i16x16(bd, T, dec, qp, int(modes[0]), fenc_y, fdec_y, o, cnt)
    elif kind == "i8":
        encode_i8x8(bd, T, qp, modes, nb, fenc_y, fdec_y, o, cnt)
    else:
        encode_i4x4(bd, T, qp, modes, nb, fenc_y, fdec_y, o, cnt)
    if cf:
        encode_chroma(bd, T, int(cf == 2), qpc, int(cmode), fenc_c, fdec_c, o, cnt)
    if kind == "i8":
        for idx in range(4):
            if not o.nnz[4 * idx]:
                o.level[4 * idx:4 * idx + 4] = 0
    else:
        o.level[:16][o.nnz[:16] == 0] = 0
    o.level[16:][o.nnz[16:] == 0] = 0
    for ch in range(2):
        if not o.nnz_dc[ch]:
            o.chroma_dc[ch] = 0
    if not o.nnz_ldc:
        o.luma_dc[:] = 0
    return o


# ------------------------------------------------------------------ frames
def _coords(case, mb):
    f, r = divmod(mb, case.mbw * case.mbh)
    my, mx = divmod(r, case.mbw)
    return f, my, mx


def mb_buffers(case, recon_y, recon_c, mb):
    """fenc in FENC layout and the FDEC-layout buffers of macroblock mb with the neighbours the
    picture has (zeros elsewhere, and in the macroblock itself: its content reaches nothing)"""
    f, my, mx = _coords(case, mb)
    nb = mb_neighbours(mx, my, case.mbw)
    ch = case.chroma_rows
    dt = recon_y.dtype
    fenc_y = np.zeros((16, FENC), dt)
    fenc_y[:, :16] = case.fenc_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
    fenc_c = np.zeros((16, FENC), dt)
    fdec_y, fdec_c = np.zeros(BUF, dt), np.zeros(BUF, dt)
    vy = fdec_y.reshape(18, FDEC)
    y0, x0 = 16 * my, 16 * mx
    if nb & MB_TOP:
        vy[0, 8:24] = recon_y[f, y0 - 1, x0:x0 + 16]
    if nb & MB_TOPRIGHT:
        vy[0, 24:32] = recon_y[f, y0 - 1, x0 + 16:x0 + 24]
    if nb & MB_TOPLEFT:
        vy[0, 7] = recon_y[f, y0 - 1, x0 - 1]
    if nb & MB_LEFT:
        vy[1:17, 7] = recon_y[f, y0:y0 + 16, x0 - 1]
    if case.cf:
        uv = case.fenc_c[f, ch * my:ch * my + ch, x0:x0 + 16]
        fenc_c[:ch, :8] = uv[:, 0::2]
        fenc_c[:ch, 8:16] = uv[:, 1::2]
        vc = fdec_c.reshape(18, FDEC)
        c0 = ch * my
        for k in range(2):
            col = 8 + 16 * k
            if nb & MB_TOP:
                vc[0, col:col + 8] = recon_c[f, c0 - 1, x0 + k:x0 + 16:2]
            if nb & MB_TOPLEFT:
                vc[0, col - 1] = recon_c[f, c0 - 1, x0 - 2 + k]
            if nb & MB_LEFT:
                vc[1:1 + ch, col - 1] = recon_c[f, c0:c0 + ch, x0 - 2 + k]
    return f, my, mx, nb, fenc_y.reshape(-1), fenc_c.reshape(-1), fdec_y, fdec_c


def put_back(case, recon_y, recon_c, f, my, mx, fdec_y, fdec_c):
    ch = case.chroma_rows
    recon_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = fdec_y.reshape(18, FDEC)[1:17, 8:24]
    if case.cf:
        c = fdec_c.reshape(18, FDEC)
        recon_c[f, ch * my:ch * my + ch, 16 * mx:16 * mx + 16:2] = c[1:1 + ch, 8:16]
        recon_c[f, ch * my:ch * my + ch, 16 * mx + 1:16 * mx + 16:2] = c[1:1 + ch, 24:32]


def encode(case, dec, recon_y=None, recon_c=None):
    """the outputs of x264hip_*_mb_encode_inter followed by x264hip_*_mb_encode_intra for `case`
    with b_dct_decimate = dec (every array of include/x264hip_mbintra.h; luma_dc rows of inter
    macroblocks stay 0), and the branch counters.  recon_y / recon_c: the planes before the inter
    call (default the case's prediction)."""
    bd, cf = case.bd, case.cf
    T = mc.tables(bd, case.cqm)
    out = mc.encode(case, dec, recon_y, recon_c)
    out.luma_dc = np.zeros((case.nmb, 16), orc.coef_dtype(bd))
    cnt = out.counters
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if not fl & INTRA:
            continue
        qp = int(case.qp[mb])
        f, my, mx, nb, fenc_y, fenc_c, fdec_y, fdec_c = mb_buffers(case, out.recon_y, out.recon_c, mb)
        if nb & MB_LEFT and nb & MB_TOP and nb & MB_TOPRIGHT and not any(
                case.flags[mb + d] & INTRA for d in (-1, -case.mbw, -case.mbw + 1)):
            cnt["inter_neighbours"] += 1
        o = encode_mb(bd, T, cf, dec, fl, qp, int(case.qp_table[qp]), case.pred_mode[mb], case.chroma_pred_mode[mb], nb,
                      fenc_y, fdec_y, fenc_c, fdec_c, cnt)
        put_back(case, out.recon_y, out.recon_c, f, my, mx, fdec_y, fdec_c)
        out.level[mb], out.chroma_dc[mb], out.nnz[mb], out.luma_dc[mb] = o.level, o.chroma_dc, o.nnz, o.luma_dc
        cbp = o.cbp_chroma << 4 | o.cbp_luma | o.nnz_ldc << 8 | o.nnz_dc[0] << 9 | o.nnz_dc[1] << 10
        out.cbp[mb] = cbp
        cnt["intra"] += 1
        cnt["intra_coded"] += cbp != 0
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


def decode(case, out, recon_y=None, recon_c=None):
    """The reconstruction a decoder derives from level / luma_dc / chroma_dc / mb_flags / modes / qp
    alone: mbenc_cases.decode for the inter macroblocks, then the intra macroblocks in raster
    order, each predicted from the decoded picture around it; every block is un-zigzagged with the
    scans pinned in tests/golden/ref_tables.json, dequantised and inverse-transformed with the
    oracle's primitives on the one path of the standard (the inverse DC transform's values go to
    entry 0 of the 4x4 blocks), never the encoder's DC-only shortcuts."""
    bd, cf = case.bd, case.cf
    T = mc.tables(bd, case.cqm)
    f_ = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    c422 = int(cf == 2)
    recon_y, recon_c = mc.decode(case, out, recon_y, recon_c)
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if not fl & INTRA:
            continue
        qp = int(case.qp[mb])
        qpc = int(case.qp_table[qp])
        f, my, mx, nb, _, _, fdec_y, fdec_c = mb_buffers(case, recon_y, recon_c, mb)
        lev, modes = out.level[mb], case.pred_mode[mb]
        kind = mb_type(fl)
        if kind == "i16":
            predict(bd, "16x16", int(modes[0]), fdec_y, OY)
            dc = mc._unzig(out.luma_dc[mb], mc.ZIG4, 4)
            f_("idct4x4dc")(A(dc))
            f_("dequant_4x4_dc")(A(dc), A(T.dq4[CQM_4IY]), qp)
        for idx in range(16 if kind != "i8" else 0):
            bx, by = block_xy(idx)
            off = OY + 4 * bx + 4 * by * FDEC
            if kind == "i4":
                if (neighbour4(idx, nb) & (MB_TOPRIGHT | MB_TOP)) == MB_TOP:
                    fdec_y[off + 4 - FDEC:off + 8 - FDEC] = fdec_y[off + 3 - FDEC]
                predict(bd, "4x4", int(modes[idx]), fdec_y, off)
            d = np.zeros(16, cd)
            if lev[idx].any():
                d = mc._unzig(lev[idx], mc.ZIG4, 4)
                f_("dequant_4x4")(A(d), A(T.dq4[CQM_4IY]), qp)
            if kind == "i16":
                d[0] = dc[BLOCK_IDX_XY_1D[idx]]
            if d.any():
                f_("add4x4_idct")(A(fdec_y, off), A(d))
        for idx in range(4 if kind == "i8" else 0):
            off = OY + 8 * (idx & 1) + 8 * (idx >> 1) * FDEC
            predict8x8(bd, int(modes[4 * idx]), neighbour8(idx, nb), fdec_y, off)
            l8 = np.ascontiguousarray(lev[4 * idx:4 * idx + 4].reshape(64))
            if l8.any():
                d = mc._unzig(l8, mc.ZIG8, 8)
                f_("dequant_8x8")(A(d), A(T.dq8[CQM_8IY]), qp)
                f_("add8x8_idct8")(A(fdec_y, off), A(d))
        for ch in range(2 if cf else 0):
            predict(bd, "8x16c" if c422 else "8x8c", int(case.chroma_pred_mode[mb]), fdec_c, OY + 16 * ch)
            dcl = [int(v) for v in out.chroma_dc[mb][ch]]
            dcv = np.zeros((8, 16), cd)
            if c422:
                inv = [0] * 8
                for i, v in enumerate(mc.zigzag_scan_2x4_dc(list(range(8)))):
                    inv[v] = dcl[i]
                dcc = np.array(inv, cd)
                f_("idct_dequant_2x4_dc")(A(dcc), A(dcv), A(T.dq4[CQM_4IC]), qpc + 3)
            else:
                inv = [0] * 4
                for i, v in enumerate(mc.zigzag_scan_2x2_dc(list(range(4)))):
                    inv[v] = dcl[i]
                mc.idct_dequant_2x2_dc(bd, inv, dcv, T.dq4[CQM_4IC], qpc)
            for k in range(8 if c422 else 4):
                idx = 16 + ch * 16 + (k >> 2) * 8 + (k & 3)
                d = np.zeros(16, cd)
                if lev[idx].any():
                    d = mc._unzig(lev[idx], mc.ZIG4, 4)
                    f_("dequant_4x4")(A(d), A(T.dq4[CQM_4IC]), qpc)
                d[0] = dcv[k][0]
                f_("add4x4_idct")(A(fdec_c, OY + 16 * ch + (k & 1) * 4 + (k >> 1) * 4 * FDEC), A(d))
        put_back(case, recon_y, recon_c, f, my, mx, fdec_y, fdec_c)
    return recon_y, recon_c


# ------------------------------------------------------------------ inputs
# (mb_width, mb_height, frames, all_intra): the shapes of tests/test_gpu_mbintra.py
SHAPES = ((1, 1, 1, True), (3, 1, 1, True), (1, 3, 1, True), (2, 2, 1, True), (5, 4, 2, False), (24, 14, 2, False))
ALL_INTRA_PICTURE = (5, 4, 1, True)


def valid_modes(kind, n):
    """the modes of predict.h that read no neighbour outside n (TOPRIGHT is emulated for 4x4 and by
    the 8x8 filter wherever TOP exists)"""
    t, l = bool(n & MB_TOP), bool(n & MB_LEFT)
    tl = bool(n & MB_TOPLEFT) and t and l
    if kind in ("4x4", "8x8"):
        ok = {0: t, 1: l, 2: t and l, 3: t, 4: tl, 5: tl, 6: tl, 7: t, 8: l, 9: l, 10: t, 11: True}
    elif kind == "16x16":
        ok = {0: t, 1: l, 2: t and l, 3: tl, 4: l, 5: t, 6: True}
    else:
        ok = {0: t and l, 1: l, 2: t, 3: tl, 4: l, 5: t, 6: True}
    return [m for m, v in ok.items() if v]


def _boundary_case(bd, cf, mbw, mbh, nframes, cqm, recipe, key):
    """one I_16x16 / DC_128 macroblock per entry (qp, rects, waves) of `recipe`, chroma DC_128: the
    prediction is mid grey whatever the neighbours, fenc = mid grey + mbenc_cases' rectangles and
    waves, so the residual and with it the AC decimate score is the recipe's alone"""
    base = mc._boundary_case(bd, cf, mbw, mbh, nframes, cqm, tuple((q, 0, r, w) for q, r, w in recipe), key)
    case = types.SimpleNamespace(**vars(base))
    case.fenc_y, case.fenc_c = base.pred_y, base.pred_c            # grey + the residual
    case.pred_y, case.pred_c = base.fenc_y, base.fenc_c            # what an inter call would start from: unused
    case.flags = np.full(base.nmb, INTRA | I16, np.uint8)
    case.pred_mode = np.zeros((base.nmb, 16), np.int8)
    case.pred_mode[:, 0] = 6
    case.chroma_pred_mode = np.full(base.nmb, 6, np.int8)
    case.all_intra = True
    return case


@functools.lru_cache(maxsize=None)
def make_case(bd, cf, mbw, mbh, nframes, cqm="flat", seed=0, all_intra=False, recipe=None):
    """mbenc_cases.make_case's inputs (same fenc, prediction, qp and flags, its INTRA macroblocks;
    all_intra: every macroblock INTRA, no skip; only the qp of a third of the intra macroblocks is
    redrawn, see below; recipe: the boundary picture, see _boundary_case) plus the type of each intra macroblock (I_4x4,
    I_8x8 through T8, I_16x16 through bit 4) and its modes, drawn from the modes valid at its
    position.  A full-scale checker macroblock at qp_max_spec becomes I_16x16 / DC_128: its DC
    quantises to nothing while its AC does not, the one arm of mb_encode_i16x16 noise does not
    reach."""
    if recipe is not None:
        return _boundary_case(bd, cf, mbw, mbh, nframes, cqm, BOUNDARY_RECIPE if recipe == "boundary" else recipe,
                              (bd, cf, mbw, mbh, nframes, cqm, seed, all_intra, recipe))
    base = mc.make_case(bd, cf, mbw, mbh, nframes, cqm, seed)
    rng = np.random.default_rng([bd, cf, mbw, mbh, nframes, seed, int(all_intra), 2640])
    case = types.SimpleNamespace(**vars(base))
    flags = base.flags.copy()
    if all_intra:
        flags = (flags & ~np.uint8(mc.SKIP)) | np.uint8(INTRA)
    pred_mode = np.zeros((base.nmb, 16), np.int8)
    chroma_pred_mode = np.zeros(base.nmb, np.int8)
    qmax = mc.qp_max_spec(bd)
    qp = base.qp.copy()
    for mb in range(base.nmb):
        if not flags[mb] & INTRA:
            continue
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        nb = mb_neighbours(mx, my, mbw)
        kind = ("i4", "i8", "i16")[int(rng.integers(3))]
        flags[mb] &= ~np.uint8(T8 | I16)
        if base.klass[mb] == mc.CHECKER and base.qp[mb] == qmax:
            kind = "i16"
        if kind == "i16":
            flags[mb] |= I16
            pred_mode[mb, 0] = rng.choice(valid_modes("16x16", nb))
            if base.klass[mb] == mc.CHECKER and base.qp[mb] == qmax:
                pred_mode[mb, 0] = 6
        elif kind == "i8":
            flags[mb] |= T8
            for i in range(4):
                pred_mode[mb, 4 * i] = rng.choice(valid_modes("8x8", neighbour8(i, nb)))
        else:
            for i in range(16):
                pred_mode[mb, i] = rng.choice(valid_modes("4x4", neighbour4(i, nb)))
        chroma_pred_mode[mb] = rng.choice(valid_modes("chroma", nb))
        # a third of the intra macroblocks at the top of the qp range: there the residual of a good
        # prediction quantises to a few +-1 or to nothing (the decimation, the empty tails)
        if not (base.klass[mb] == mc.CHECKER) and rng.random() < 1 / 3:
            qp[mb] = qmax - int(rng.integers(0, 7))
    case.qp = qp
    case.flags, case.pred_mode, case.chroma_pred_mode = flags, pred_mode, chroma_pred_mode
    if all_intra and base.nmb > 4:
        # the I picture's two last macroblock rows are quiet: mid grey with a +-2 dither, half of
        # the macroblocks with one isolated bump of one to two quantiser steps.  There every mode
        # predicts almost exactly, which is what reaches "the prediction alone", the I_16x16
        # decimation and the empty chroma tail.
        pm, scale = (1 << bd) - 1, 1 << (bd - 8)
        case.fenc_y = base.fenc_y.copy()
        case.fenc_c = base.fenc_c.copy() if cf else None
        crows = base.chroma_rows
        for mb in range(base.nmb):
            f, r = divmod(mb, mbw * mbh)
            my, mx = divmod(r, mbw)
            if my < mbh - 2:
                continue
            yy, xx = np.mgrid[0:16, 0:16]
            blk = (128 * scale + ((7 * xx + 13 * yy + mb) % 5 - 2)).astype(np.int64)
            amp = max(1, round(mc._qstep(int(qp[mb])) * rng.uniform(1, 2)))
            if rng.random() < 0.5:
                blk[rng.integers(16), rng.integers(16)] += rng.choice([-1, 1]) * amp
            case.fenc_y[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = np.clip(blk, 0, pm)
            if cf:
                cy, cx = np.mgrid[0:crows, 0:16]
                case.fenc_c[f, crows * my:crows * my + crows, 16 * mx:16 * mx + 16] = \
                    128 * scale + ((3 * cx + 5 * cy + mb) % 3 - 1)
    case.all_intra = all_intra
    case.key = (bd, cf, mbw, mbh, nframes, cqm, seed, all_intra)
    return case


def case_keys(bd, cf):
    """the case list of one (bit depth, chroma format): every shape with the flat matrices"""
    return [(bd, cf, w, h, n, "flat", 0, ai) for w, h, n, ai in SHAPES]


def all_intra_key(bd, cf):
    """the I picture of tests/test_gpu_mbintra.py"""
    w, h, n, ai = ALL_INTRA_PICTURE
    return (bd, cf, w, h, n, "flat", 0, ai)


def jvt_keys():
    return [(bd, cf, 5, 4, 2, "jvt", 0, False) for bd in (8, 10) for cf in (1, 2)]


# The boundary macroblocks, (what is pinned, (qp, rects, waves)): the AC decimate score of
# mb_encode_i16x16 (macroblock.c:214) just below, exactly at and above 6.  On the ones marked * the
# flipped comparison (tests/mutants.py) gives other bytes.  Found by search over one or two waves.
BOUNDARY = (
    ("I_16x16 AC score 3 < 6: decimated", (28, (), ((0, 8, 8, 1, 1, -2),))),
    ("I_16x16 AC score = 6: kept *", (28, (), ((0, 4, 12, 0, 1, -3), (0, 8, 12, 0, 1, -2)))),
    ("I_16x16 AC score > 6", (28, (), ((0, 8, 4, 1, 0, 10),))),
    ("I_16x16 AC score = 6 at qp 36 *", (36, (), ((0, 0, 4, 0, 1, 5), (0, 12, 8, 0, 1, 9)))),
)
BOUNDARY_RECIPE = tuple(e for _, e in BOUNDARY)


def boundary_keys():
    """the boundary macroblocks as a 2x2 picture per (bit depth, chroma format)"""
    return [(bd, cf, 2, 2, 1, "flat", 0, True, "boundary") for bd in (8, 10) for cf in (0, 1, 2)]


GPU_GROUPS = ("shapes", "jvt", "all_intra", "boundary")


def gpu_keys(group=None, **where):
    """every (key, dec) tests/test_gpu_mbintra.py compares with the device byte for byte, which is
    the list the boundary mutants of tests/test_cpu_mutants.py are held to.  group: one of GPU_GROUPS
    (one test function each); where: bd / cf / dec of one parametrised case of that function."""
    keys = {"shapes": [(k, dec) for bd in (8, 10) for cf in (0, 1, 2) for dec in (0, 1) for k in case_keys(bd, cf)],
            "jvt": [(k, 1) for k in jvt_keys()],
            "all_intra": [(all_intra_key(bd, cf), dec) for bd in (8, 10) for cf in (0, 1, 2) for dec in (1, 0)],
            "boundary": [(k, 1) for k in boundary_keys()]}
    keys = [kd for g in GPU_GROUPS if group in (None, g) for kd in keys[g]]
    pick = {"bd": lambda kd: kd[0][0], "cf": lambda kd: kd[0][1], "dec": lambda kd: kd[1]}
    return [kd for kd in keys if all(pick[n](kd) == v for n, v in where.items())]


def key_size(kd):
    """macroblocks of a gpu_keys() entry: what its expected() costs"""
    return kd[0][2] * kd[0][3] * kd[0][4]
