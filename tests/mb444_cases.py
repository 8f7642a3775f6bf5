"""The 4:4:4 macroblock encodes restated per macroblock, from the reference's C
(encoder/macroblock.c:706-921 with plane_count = 3, chroma = 0; no lossless / trellis / noise
reduction / i_skip_intra), and the inputs of tests/test_cpu_mb444.py and tests/test_gpu_mb444.py.
No GPU code.  The method is tests/mbenc_cases.py's and tests/mbintra_cases.py's, imported:

* Only the control flow is Python: every transform, quantiser, scan, score and predictor is the
  oracle's (tests/oracle_lib.py) or mbintra_cases'.
* Inter: encode_inter_plane is the body of the reference's plane loop with i_decimate_mb handed in
  and out, so the carry across planes (macroblock.c:771, never reset) is the caller's loop.
* Intra: the three planes are independent, and a plane is mbintra_cases' luma path
  (encode_i16x16 / encode_i4x4 / encode_i8x8) on views: the plane's slice of level / nnz / luma_dc
  and a table set whose category 0 is the plane's (CQM_4IC / CQM_8IC for U and V).
* The 8x8 chroma categories come from the unchanged oracle by a second call with lists 6 and 7 in
  the places of 4 and 5 and the deadzones 21 / 11: its categories 0, 1 are then CQM_8IC, CQM_8PC.
* encode(case, dec) returns the outputs of include/x264hip_mb444.h after both entries plus the
  branch counters and, per inter macroblock, what each plane did (rec); decode(case, out)
  rebuilds the reconstruction from level / luma_dc alone.
"""
import collections
import functools
import types

import numpy as np

import checkasm_bufs as cb
import mbenc_cases as mc
import mbintra_cases as mi
import oracle_lib as orc

INTRA, T8, D16, SKIP, I16 = mc.INTRA, mc.T8, mc.D16, mc.SKIP, mi.I16
FENC, FDEC, OY, BUF = mc.FENC, mc.FDEC, mi.OY, mi.BUF
A = orc._addr
# reference common/set.h: the 4x4 and the 8x8 categories share the numbering
CQM_IY, CQM_PY, CQM_IC, CQM_PC = range(4)
LISTS = {"flat": [cb.FLAT16] * 8,
         "distinct": [cb.JVT4I, cb.JVT4P, cb.CQM_TEST4, cb.FLAT16, cb.JVT8I, cb.JVT8P, cb.CQM_TEST8, cb.FLAT16]}
SHAPES = ((1, 1, 1), (3, 1, 1), (5, 4, 2), (1, 3, 1), (2, 2, 1), (7, 3, 3))   # (mb_width, mb_height, frames)
I_ONLY_SHAPES = ((1, 3, 1), (2, 2, 1))                           # for the intra launches' diagonal walk: I pictures only
CHAIN_SHAPE = (5, 4, 2)
SEED = 0                                                         # tests/test_cpu_mb444.py holds it to the coverage conditions


def lists_of(cqm):
    """scaling_list[8]: four lists of 16, four of 64 entries"""
    return [list(l[:16]) for l in LISTS[cqm][:4]] + [list(l) for l in LISTS[cqm][4:]]


@functools.lru_cache(maxsize=None)
def tables(bd, cqm="flat", luma_only=False):
    """the tables of x264_cqm_init with num_8x8_lists = 4: q8m / q8b [4][QP+1][64], dq8 [4][6][64].
    luma_only: the chroma categories replaced by the luma ones (what a plane loop that forgot the
    category would read)"""
    lists = lists_of(cqm)
    q4m, q4b, q8m, q8b = orc.cqm_init(bd, lists)
    dq4, dq8 = orc.cqm_dequant(lists)
    second = lists[:4] + [lists[6], lists[7]] + lists[6:]
    _, _, c8m, c8b = orc.cqm_init(bd, second, dz_inter=21, dz_intra=11)
    _, cdq8 = orc.cqm_dequant(second)
    q8m, q8b = np.concatenate([q8m[:2], c8m[:2]]), np.concatenate([q8b[:2], c8b[:2]])
    dq8 = np.concatenate([dq8, cdq8])
    if luma_only:
        q4m, q4b, dq4, q8m, q8b, dq8 = (np.concatenate([t[:2], t[:2]]) for t in (q4m, q4b, dq4, q8m, q8b, dq8))
    return types.SimpleNamespace(q4m=q4m, q4b=q4b, q8m=q8m, q8b=q8b, dq4=dq4, dq8=dq8)


def plane_tables(T, cat):
    """T with category `cat` in place 0: what mbintra_cases' luma path reads as CQM_4IY / CQM_8IY"""
    return types.SimpleNamespace(**{n: getattr(T, n)[cat:cat + 1] for n in ("q4m", "q4b", "q8m", "q8b", "dq4", "dq8")})


class MbOut:
    """what macroblock_encode_internal leaves besides fdec"""

    def __init__(self, bd):
        cd = orc.coef_dtype(bd)
        self.level = np.zeros((48, 16), cd)
        self.nnz = np.zeros(48, np.uint8)
        self.luma_dc = np.zeros((3, 16), cd)
        self.nnz_ldc = [0, 0, 0]
        self.cbp_luma = 0


# ------------------------------------------------------------------ inter
def encode_inter_plane(bd, T, dec, t8, p, qp, fenc, fdec, o, i_decimate_mb, rec=None):
    """macroblock.c:806-843 (t8) / :848-920, the body of the plane loop for plane p; fenc [16*16],
    fdec [16*32] (prediction in, reconstruction out); qp is the plane's.  Returns i_decimate_mb
    as the next plane meets it.  rec: a list that gets what the plane did."""
    f = lambda name: orc.fn(bd, name)
    dct = np.zeros(256, orc.coef_dtype(bd))
    cat = CQM_PC if p else CQM_PY
    plane_cbp = own = nzs = part = 0
    if t8:
        dct8 = dct.reshape(4, 64)
        f("sub16x16_dct8")(A(dct), A(fenc), A(fdec))
        for idx in range(4):
            nz = f("quant_8x8")(A(dct8[idx]), A(T.q8m[cat][qp]), A(T.q8b[cat][qp]))
            if nz:
                nzs += 1
                lev = o.level[16 * p + 4 * idx:16 * p + 4 * idx + 4].reshape(64)
                f("zigzag_scan_8x8")(0, A(lev), A(dct8[idx]))
                if dec:
                    s = f("decimate_score64")(A(lev))
                    i_decimate_mb += s
                    own += s
                    if s >= 4:
                        plane_cbp |= 1 << idx
                    else:
                        part += 1
                else:
                    plane_cbp |= 1 << idx
        kept = i_decimate_mb >= 6 or not dec
        if kept:
            o.cbp_luma |= plane_cbp
            for idx in mc._bits(plane_cbp, 4):
                f("dequant_8x8")(A(dct8[idx]), A(T.dq8[cat]), qp)
                f("add8x8_idct8")(A(fdec, 8 * (idx & 1) + 8 * (idx >> 1) * FDEC), A(dct8[idx]))
                o.nnz[16 * p + 4 * idx:16 * p + 4 * idx + 4] = 1  # STORE_8x8_NNZ
    else:
        dct4 = dct.reshape(16, 16)
        f("sub16x16_dct")(A(dct), A(fenc), A(fdec))
        for i8 in range(4):
            i_decimate_8x8 = 0 if dec else 6
            nz = f("quant_4x4x4")(A(dct4[4 * i8]), A(T.q4m[cat][qp]), A(T.q4b[cat][qp]))
            if nz:
                nzs += 1
                for i4 in mc._bits(nz, 4):
                    idx = 4 * i8 + i4
                    f("zigzag_scan_4x4")(0, A(o.level[16 * p + idx]), A(dct4[idx]))
                    f("dequant_4x4")(A(dct4[idx]), A(T.dq4[cat]), qp)
                    if i_decimate_8x8 < 6:
                        i_decimate_8x8 += f("decimate_score16")(A(o.level[16 * p + idx]))
                    o.nnz[16 * p + idx] = 1
                i_decimate_mb += i_decimate_8x8
                own += i_decimate_8x8
                if i_decimate_8x8 < 4:
                    o.nnz[16 * p + 4 * i8:16 * p + 4 * i8 + 4] = 0
                    part += 1
                else:
                    plane_cbp |= 1 << i8
        kept = i_decimate_mb >= 6
        if not kept:
            plane_cbp = 0
            o.nnz[16 * p:16 * p + 16] = 0
        else:
            o.cbp_luma |= plane_cbp
            for i8 in mc._bits(plane_cbp, 4):
                f("add8x8_idct")(A(fdec, (i8 & 1) * 8 + (i8 >> 1) * 8 * FDEC), A(dct4[4 * i8]))
    if rec is not None:
        rec.append(types.SimpleNamespace(nonzero=nzs > 0, own=own, cbp=plane_cbp if kept else 0,
                                         part=part if kept and plane_cbp else 0))
    return i_decimate_mb


def clear_levels(o, t8):
    """every block whose final non_zero_count is 0 is zeros (include/x264hip_mb444.h)"""
    if t8:
        for b in range(0, 48, 4):
            if not o.nnz[b]:
                o.level[b:b + 4] = 0
    else:
        o.level[o.nnz == 0] = 0
    for p in range(3):
        if not o.nnz_ldc[p]:
            o.luma_dc[p] = 0


def _fenc_block(plane, f, my, mx):
    b = np.zeros((16, FENC), plane.dtype)
    b[:, :16] = plane[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
    return b.reshape(-1)


def _fdec_block(plane, f, my, mx):
    b = np.zeros((16, FDEC), plane.dtype)
    b[:, :16] = plane[f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
    return b.reshape(-1)


def _nz_mask(o, t8):
    """x264hip_deblock_strength_t.nz from plane 0's nnz"""
    return sum(int(o.nnz[4 * i]) << i for i in range(4)) if t8 else sum(int(o.nnz[i]) << i for i in range(16))


def plane_qp(case, mb, p):
    qp = int(case.qp[mb])
    return int(case.qp_table[qp]) if p else qp


def _shim(case, p):
    """plane p as a luma-only case of mbintra_cases (mb_buffers / put_back)"""
    return types.SimpleNamespace(mbw=case.mbw, mbh=case.mbh, cf=0, chroma_rows=0, fenc_y=case.fenc[p], fenc_c=None)


def encode(case, dec, recon=None, T=None):
    """the outputs of x264hip_*_mb_encode_inter_444 followed by x264hip_*_mb_encode_intra_444 with
    b_dct_decimate = dec; recon: the three planes before the inter call (default the prediction).
    Besides the header's arrays: counters {(plane, arm of mbintra_cases) or name: count} and rec
    {mb: [per plane what encode_inter_plane recorded]} of the coded inter macroblocks."""
    bd, n = case.bd, case.nmb
    T = tables(bd, case.cqm) if T is None else T
    cd = orc.coef_dtype(bd)
    pred = case.pred if recon is None else recon
    out = types.SimpleNamespace(
        recon=[a.copy() for a in pred], level=np.zeros((n, 48, 16), cd), nnz=np.zeros((n, 48), np.uint8),
        cbp=np.zeros(n, np.int32), nz=np.zeros(n, np.int32), flags_out=np.zeros(n, np.uint8),
        luma_dc=np.zeros((n, 3, 16), cd), counters=collections.Counter(), rec={})
    per = case.mbw * case.mbh
    for mb in range(n):                                           # the inter entry
        fl = int(case.flags[mb])
        if fl & INTRA:
            out.flags_out[mb] = fl
            continue
        f, r = divmod(mb, per)
        my, mx = divmod(r, case.mbw)
        o = MbOut(bd)
        if not fl & SKIP:                                         # (skip: recon = pred, everything zero)
            i_decimate_mb, rec = 0, []
            for p in range(3):
                fenc, fdec = _fenc_block(case.fenc[p], f, my, mx), _fdec_block(pred[p], f, my, mx)
                i_decimate_mb = encode_inter_plane(bd, T, dec, bool(fl & T8), p, plane_qp(case, mb, p), fenc, fdec, o,
                                                   i_decimate_mb, rec)
                out.recon[p][f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = fdec.reshape(16, FDEC)[:, :16]
            out.rec[mb] = rec
            clear_levels(o, bool(fl & T8))
        out.level[mb], out.nnz[mb], out.cbp[mb], out.nz[mb] = o.level, o.nnz, o.cbp_luma, _nz_mask(o, fl & T8)
        out.flags_out[mb] = (fl & 3) | (D16 if (fl & D16) and not o.cbp_luma else 0)
    for mb in range(n):                                           # the intra entry, raster order
        fl = int(case.flags[mb])
        if not fl & INTRA:
            continue
        o = MbOut(bd)
        kind = mi.mb_type(fl)
        out.counters["type", kind] += 1
        for p in range(3):
            sh = _shim(case, p)
            f, my, mx, nb, fenc, _, fdec, _ = mi.mb_buffers(sh, out.recon[p], None, mb)
            Tp = plane_tables(T, CQM_IC if p else CQM_IY)
            v = types.SimpleNamespace(level=o.level[16 * p:16 * p + 16], nnz=o.nnz[16 * p:16 * p + 16], luma_dc=o.luma_dc[p],
                                      cbp_luma=0, nnz_ldc=0)
            cnt = collections.Counter()
            qp, modes = plane_qp(case, mb, p), case.pred_mode[mb]
            if kind == "i16":
                cnt["mode16", int(modes[0])] += 1
                mi.encode_i16x16(bd, Tp, dec, qp, int(modes[0]), fenc, fdec, v, cnt)
            elif kind == "i8":
                mi.encode_i8x8(bd, Tp, qp, modes, nb, fenc, fdec, v, cnt)
            else:
                mi.encode_i4x4(bd, Tp, qp, modes, nb, fenc, fdec, v, cnt)
            o.cbp_luma |= v.cbp_luma
            o.nnz_ldc[p] = v.nnz_ldc
            mi.put_back(sh, out.recon[p], None, f, my, mx, fdec, None)
            for key, c in cnt.items():
                out.counters[p, key] += c
        clear_levels(o, kind == "i8")
        cbp = o.cbp_luma | sum(o.nnz_ldc[p] << (8 + p) for p in range(3))     # macroblock.c:946-950
        out.level[mb], out.nnz[mb], out.luma_dc[mb], out.cbp[mb] = o.level, o.nnz, o.luma_dc, cbp
        out.nz[mb] = _nz_mask(o, fl & T8)
        out.flags_out[mb] = fl & 3
        out.counters["intra"] += 1
        out.counters["intra_coded"] += cbp != 0
    return out


@functools.lru_cache(maxsize=None)
def expected(key, dec):
    """encode(make_case(*key), dec), computed once per process and shared; do not modify"""
    return encode(make_case(*key), dec)


def decode(case, out, recon=None):
    """The three planes a decoder derives from level / luma_dc / mb_flags / modes / qp alone: every
    block un-zigzagged with the scans pinned in tests/golden/ref_tables.json, dequantised with
    the plane's category and inverse-transformed with the oracle's primitives; inter macroblocks
    first, then the intra ones in raster order, each plane predicted from its own decoded
    neighbours; the I_16x16 DC goes to entry 0 of the 4x4 blocks, never the DC-only shortcut."""
    bd = case.bd
    T = tables(bd, case.cqm)
    f_ = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    rec = [a.copy() for a in (case.pred if recon is None else recon)]
    per = case.mbw * case.mbh

    def residual(lev, t8, cat, qp, fdec, base, dc=None):
        """lev: the plane's 16 rows of level; base: the offset of pixel (0,0) in fdec"""
        if t8:
            for idx in range(4):
                l8 = np.ascontiguousarray(lev[4 * idx:4 * idx + 4].reshape(64))
                if l8.any():
                    d = mc._unzig(l8, mc.ZIG8, 8)
                    f_("dequant_8x8")(A(d), A(T.dq8[cat]), qp)
                    f_("add8x8_idct8")(A(fdec, base + 8 * (idx & 1) + 8 * (idx >> 1) * FDEC), A(d))
            return
        for idx in range(16):
            d = np.zeros(16, cd)
            if lev[idx].any():
                d = mc._unzig(lev[idx], mc.ZIG4, 4)
                f_("dequant_4x4")(A(d), A(T.dq4[cat]), qp)
            if dc is not None:
                d[0] = dc[mi.BLOCK_IDX_XY_1D[idx]]
            if d.any():
                bx, by = mi.block_xy(idx)
                f_("add4x4_idct")(A(fdec, base + 4 * bx + 4 * by * FDEC), A(d))

    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if fl & (INTRA | SKIP):
            continue
        f, r = divmod(mb, per)
        my, mx = divmod(r, case.mbw)
        for p in range(3):
            fdec = _fdec_block(rec[p], f, my, mx)
            residual(out.level[mb][16 * p:16 * p + 16], fl & T8, CQM_PC if p else CQM_PY, plane_qp(case, mb, p), fdec, 0)
            rec[p][f, 16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = fdec.reshape(16, FDEC)[:, :16]
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if not fl & INTRA:
            continue
        kind, modes = mi.mb_type(fl), case.pred_mode[mb]
        for p in range(3):
            sh = _shim(case, p)
            cat, qp = (CQM_IC if p else CQM_IY), plane_qp(case, mb, p)
            f, my, mx, nb, _, _, fdec, _ = mi.mb_buffers(sh, rec[p], None, mb)
            lev = out.level[mb][16 * p:16 * p + 16]
            if kind == "i16":
                mi.predict(bd, "16x16", int(modes[0]), fdec, OY)
                dc = mc._unzig(out.luma_dc[mb][p], mc.ZIG4, 4)
                f_("idct4x4dc")(A(dc))
                f_("dequant_4x4_dc")(A(dc), A(T.dq4[cat]), qp)
                residual(lev, 0, cat, qp, fdec, OY, dc)
            elif kind == "i8":
                for idx in range(4):
                    off = OY + 8 * (idx & 1) + 8 * (idx >> 1) * FDEC
                    mi.predict8x8(bd, int(modes[4 * idx]), mi.neighbour8(idx, nb), fdec, off)
                    l8 = np.ascontiguousarray(lev[4 * idx:4 * idx + 4].reshape(64))
                    if l8.any():
                        d = mc._unzig(l8, mc.ZIG8, 8)
                        f_("dequant_8x8")(A(d), A(T.dq8[cat]), qp)
                        f_("add8x8_idct8")(A(fdec, off), A(d))
            else:
                for idx in range(16):
                    bx, by = mi.block_xy(idx)
                    off = OY + 4 * bx + 4 * by * FDEC
                    if (mi.neighbour4(idx, nb) & (mi.MB_TOPRIGHT | mi.MB_TOP)) == mi.MB_TOP:
                        fdec[off + 4 - FDEC:off + 8 - FDEC] = fdec[off + 3 - FDEC]
                    mi.predict(bd, "4x4", int(modes[idx]), fdec, off)
                    if lev[idx].any():
                        d = mc._unzig(lev[idx], mc.ZIG4, 4)
                        f_("dequant_4x4")(A(d), A(T.dq4[cat]), qp)
                        f_("add4x4_idct")(A(fdec, off), A(d))
            mi.put_back(sh, rec[p], None, f, my, mx, fdec, None)
    return rec


# ------------------------------------------------------------------ inputs
ZERO, BUMP, NOISE, QUADS, CHECKER, CARRY = range(6)               # a plane's residual class


def _residual(rng, k, qs):
    """mbenc_cases.make_case's luma residual of class k at quantiser step qs, [16, 16]"""
    r = np.zeros((16, 16))
    if k == BUMP:
        r[rng.integers(16), rng.integers(16)] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(1, 2)))
    elif k == NOISE:
        r = rng.normal(0, qs * rng.choice([0.25, 0.5, 1.0, 2.0, 4.0]), (16, 16))
    elif k == QUADS:
        for i8 in range(4):
            sl = (slice(8 * (i8 >> 1), 8 * (i8 >> 1) + 8), slice(8 * (i8 & 1), 8 * (i8 & 1) + 8))
            m = rng.choice(3, p=[0.35, 0.4, 0.25])
            if m == 1:
                y0, x0 = 4 * rng.integers(2), 4 * rng.integers(2)
                r[sl][y0:y0 + 4, x0:x0 + 4] = rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(0.45, 0.8)))
            elif m == 2:
                r[sl] = rng.normal(0, qs * rng.choice([1.0, 3.0]), (8, 8))
    return np.rint(r)


def carry_levels(rng, t8, faint):
    """the levels of a CARRY macroblock, [3][16][16] by plane and h->dct.luma4x4 index (a
    transform-8 block's 64 at rows 4*idx ..): in shuffled plane order a lone +-1 DC (decimate
    score 3); inside one 8x8 a +-1 DC plus a lone +-1 at zigzag index 1..5 of a second 4x4 block
    (index 5..19 of the same block at transform 8), score 4 or 5; and nothing or a lone DC.
    faint: every plane nonzero and the scores (3, 1, 1): all three are dropped."""
    lev = np.zeros((3, 16, 16), np.int64)
    sign = lambda: int(rng.choice([-1, 1]))
    order = rng.permutation(3)

    def put(p, i8, block, k, v):
        if t8:
            lev[p].reshape(4, 64)[i8, k] = v
        else:
            lev[p, 4 * i8 + block, k] = v
    put(order[0], rng.integers(4), rng.integers(4), 0, sign())
    if faint:
        for p in order[1:]:
            put(p, rng.integers(4), rng.integers(4), int(rng.integers(12, 28)) if t8 else int(rng.integers(3, 6)), sign())
        return lev
    i8, a = rng.integers(4), rng.integers(4)
    put(order[1], i8, a, 0, sign())
    if t8:
        put(order[1], i8, 0, int(rng.integers(5, 20)), sign())
    else:
        put(order[1], i8, (a + 1 + rng.integers(3)) % 4, int(rng.integers(1, 6)), sign())
    if rng.random() < 0.5:
        put(order[2], rng.integers(4), rng.integers(4), 0, sign())
    return lev


def inverse_of(bd, T, t8, cat, qp, lev, grey):
    """the 16x16 block whose residual against flat `grey` is the inverse transform of `lev`"""
    f_ = lambda name: orc.fn(bd, name)
    cd = orc.coef_dtype(bd)
    fdec = np.full(16 * FDEC, grey, orc.pixel_dtype(bd))
    if t8:
        for idx in range(4):
            l8 = np.ascontiguousarray(lev.reshape(4, 64)[idx]).astype(cd)
            if l8.any():
                d = mc._unzig(l8, mc.ZIG8, 8)
                f_("dequant_8x8")(A(d), A(T.dq8[cat]), qp)
                f_("add8x8_idct8")(A(fdec, 8 * (idx & 1) + 8 * (idx >> 1) * FDEC), A(d))
    else:
        for idx in range(16):
            if lev[idx].any():
                d = mc._unzig(lev[idx].astype(cd), mc.ZIG4, 4)
                f_("dequant_4x4")(A(d), A(T.dq4[cat]), qp)
                bx, by = mi.block_xy(idx)
                f_("add4x4_idct")(A(fdec, 4 * bx + 4 * by * FDEC), A(d))
    return fdec.reshape(16, FDEC)[:, :16].astype(np.int64)


def _boundary_case(bd, mbw, mbh, nframes, cqm, recipe, key):
    """one inter macroblock per entry (qp, mb_flags, rects, waves) of `recipe`: the three planes mid
    grey, pred = fenc + mbenc_cases' rectangles and waves (plane 0 / 1 / 2 = Y / U / V, all 16x16).
    The decimate score runs on from plane to plane (macroblock.c:806-920 inside the plane loop), so
    a plane is kept or dropped by what it and the planes before it add up to."""
    n = nframes * mbw * mbh
    assert n == len(recipe)
    grey = 128 << (bd - 8)
    res = [np.zeros((nframes, 16 * mbh, 16 * mbw), np.int64) for _ in range(3)]
    for mb, (q, fl, rects, waves) in enumerate(recipe):
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        for plane, y, x, h, w, a in rects:
            assert y + h <= 16 and x + w <= 16
            res[plane][f, 16 * my + y:16 * my + y + h, 16 * mx + x:16 * mx + x + w] += a
        for plane, y, x, u, v, c in waves:
            res[plane][f, 16 * my + y:16 * my + y + 4, 16 * mx + x:16 * mx + x + 4] += c * np.outer(mc.H4[u], mc.H4[v])
    pdt = orc.pixel_dtype(bd)
    assert all(0 <= grey + a.min() and grey + a.max() < (1 << bd) for a in res)
    return types.SimpleNamespace(
        bd=bd, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, cqm=cqm, all_intra=False,
        fenc=[np.full_like(a, grey).astype(pdt) for a in res], pred=[(grey + a).astype(pdt) for a in res],
        qp=np.array([r[0] for r in recipe], np.int8), flags=np.array([r[1] for r in recipe], np.uint8),
        klass=np.full((n, 3), -1, np.int32), pred_mode=np.zeros((n, 16), np.int8), qp_table=mc.chroma_qp_table(bd), key=key)


@functools.lru_cache(maxsize=None)
def make_case(bd, mbw, mbh, nframes, cqm="flat", seed=0, all_intra=False, recipe=None):
    """Seeded inputs.  Plane 0, qp, mb_flags and the intra types and modes are
    mbintra_cases.make_case's luma-only case; U and V get a texture of their own and, per plane, a
    residual class of mbenc_cases.make_case scaled to the chroma qp (a full-scale checker wherever
    luma has one).  In pictures of more than three macroblocks about a third of the coded inter
    macroblocks are CARRY: all three planes flat mid grey plus the inverse transform of
    carry_levels at qp >= 24 + 6 * (bd - 8).  all_intra: the quiet last two rows in all planes.
    recipe: the boundary picture, see _boundary_case."""
    if recipe is not None:
        return _boundary_case(bd, mbw, mbh, nframes, cqm, BOUNDARY_RECIPE if recipe == "boundary" else recipe,
                              (bd, mbw, mbh, nframes, cqm, seed, all_intra, recipe))
    base = mi.make_case(bd, 0, mbw, mbh, nframes, "flat", seed, all_intra)
    rng = np.random.default_rng([bd, mbw, mbh, nframes, seed, int(all_intra), 444])
    T = tables(bd, cqm)
    pm, qmax, scale = (1 << bd) - 1, mc.qp_max_spec(bd), 1 << (bd - 8)
    n, W, H = base.nmb, 16 * mbw, 16 * mbh
    qp_table = base.qp_table

    def texture(f, k):
        y, x = np.mgrid[0:H, 0:W]
        t = 128 + 50 * np.cos(x / (6.0 + k) - f) * np.sin(y / (4.0 + k)) + 0.3 * (y - x) + rng.normal(0, 5, (H, W))
        return np.clip(np.rint(t * scale), 0, pm)
    fenc = [base.fenc_y.astype(np.int64)] + [np.stack([texture(f, 2 * p) for f in range(nframes)]).astype(np.int64)
                                             for p in (1, 2)]
    pred = [base.pred_y.astype(np.int64)] + [a.copy() for a in fenc[1:]]
    qp, klass = base.qp.copy(), np.zeros((n, 3), np.int32)
    klass[:, 0] = np.where(base.klass == mc.CHECKER, CHECKER, -1)
    yy, xx = np.mgrid[0:16, 0:16]
    for mb in range(n):
        f, r = divmod(mb, mbw * mbh)
        my, mx = divmod(r, mbw)
        sl = (f, slice(16 * my, 16 * my + 16), slice(16 * mx, 16 * mx + 16))
        fl = int(base.flags[mb])
        if n > 3 and not fl & (INTRA | SKIP) and base.klass[mb] != mc.CHECKER and rng.random() < 0.35:
            qp[mb] = int(rng.integers(24 + 6 * (bd - 8), qmax + 1))
            lev = carry_levels(rng, bool(fl & T8), rng.random() < 0.2)
            klass[mb] = CARRY
            for p in range(3):
                q = int(qp_table[qp[mb]]) if p else int(qp[mb])
                pred[p][sl] = 128 * scale
                fenc[p][sl] = inverse_of(bd, T, bool(fl & T8), CQM_PC if p else CQM_PY, q, lev[p], 128 * scale)
            continue
        for p in (1, 2):
            qs = mc._qstep(int(qp_table[qp[mb]]))
            if base.klass[mb] == mc.CHECKER:
                k = CHECKER
                chk = ((yy + xx + p) & 1) * pm
                fenc[p][sl] = chk
                pred[p][sl] = pm - chk                            # the inverse checker
            else:
                k = int(rng.choice([ZERO, BUMP, NOISE, NOISE, QUADS, QUADS]))
                if n <= 3:
                    k = (QUADS, NOISE, BUMP)[(mb + p) % 3]
                pred[p][sl] = np.clip(fenc[p][sl] + _residual(rng, k, qs), 0, pm)
            klass[mb, p] = k
            if all_intra and n > 4 and my >= mbh - 2:
                blk = 128 * scale + ((5 * xx + 11 * yy + mb + p) % 5 - 2)
                if rng.random() < 0.5:
                    blk[rng.integers(16), rng.integers(16)] += rng.choice([-1, 1]) * max(1, round(qs * rng.uniform(1, 2)))
                fenc[p][sl] = np.clip(blk, 0, pm)
    pdt = orc.pixel_dtype(bd)
    return types.SimpleNamespace(
        bd=bd, mbw=mbw, mbh=mbh, nframes=nframes, nmb=n, cqm=cqm, all_intra=all_intra,
        fenc=[a.astype(pdt) for a in fenc], pred=[a.astype(pdt) for a in pred], qp=qp, flags=base.flags, klass=klass,
        pred_mode=base.pred_mode, qp_table=qp_table, key=(bd, mbw, mbh, nframes, cqm, seed, all_intra))


def luma_case(case):
    """plane 0 as a luma-only case of mbenc_cases / mbintra_cases"""
    return types.SimpleNamespace(
        bd=case.bd, cf=0, mbw=case.mbw, mbh=case.mbh, nframes=case.nframes, nmb=case.nmb, cqm="flat", chroma_rows=0,
        fenc_y=case.fenc[0], pred_y=case.pred[0], fenc_c=None, pred_c=None, qp=case.qp, flags=case.flags,
        pred_mode=case.pred_mode, chroma_pred_mode=np.zeros(case.nmb, np.int8), qp_table=case.qp_table)


def case_keys(bd):
    """what tests/test_gpu_mb444.py runs at one bit depth: every shape as a mixed picture and as
    an I picture with the flat matrices (I_ONLY_SHAPES: as an I picture), and the distinct matrices
    once each way (the pictures of up to three macroblocks have no intra one when mixed)"""
    keys = [(bd, w, h, n, "flat", SEED, ai) for ai in (False, True) for w, h, n in SHAPES
            if ai or (w, h, n) not in I_ONLY_SHAPES]
    return keys + DISTINCT_KEYS(bd)


def DISTINCT_KEYS(bd):
    return [(bd, 7, 3, 3, "distinct", SEED, False), (bd, 5, 4, 2, "distinct", SEED, True)]


def _on_plane(p, items):
    return tuple((p,) + it[1:] for it in items)


_L4 = (((0, 4, 0, 4, 4, -2),), ((0, 0, 12, 0, 2, -1), (0, 0, 0, 0, 1, 1)))        # mbenc_cases' "4x4 transform, macroblock score = 6"
# The boundary macroblocks, (what is pinned, (qp, mb_flags, rects, waves)): the decimate score that runs
# on through the planes exactly 6 when plane 0, 1 or 2 ends, nothing in the other planes.  The
# flipped comparison (tests/mutants.py) drops that plane.  Found by search over one wave per plane.
BOUNDARY = (
    ("8x8 transform: score = 6 after plane 0", (22, T8, (), ((0, 12, 8, 1, 1, 2),))),
    ("8x8 transform: score = 6 after plane 1", (17, T8, (), ((1, 12, 4, 1, 1, 1),))),
    ("8x8 transform: score = 6 after plane 2", (17, T8, (), ((2, 8, 8, 1, 1, -1),))),
    ("4x4 transform: score = 6 after plane 0", (17, 0, _L4[0], _L4[1])),
    ("4x4 transform: score = 6 after plane 1", (17, 0, _on_plane(1, _L4[0]), _on_plane(1, _L4[1]))),
    ("4x4 transform: score = 6 after plane 2", (17, 0, _on_plane(2, _L4[0]), _on_plane(2, _L4[1]))),
    ("8x8 transform: 1 carried over from plane 0 and 5 of plane 2's own = 6: plane 2 kept",
     (22, T8, (), ((0, 0, 8, 2, 1, -1), (0, 4, 8, 2, 0, -3), (1, 12, 0, 2, 0, 3), (2, 0, 12, 1, 1, 1), (2, 4, 4, 1, 2, -3)))),
    ("nothing to code", (26, 0, (), ())),
)
BOUNDARY_RECIPE = tuple(e for _, e in BOUNDARY)


def boundary_keys():
    """the boundary macroblocks as a 4x2 picture per bit depth"""
    return [(bd, 4, 2, 1, "flat", SEED, False, "boundary") for bd in (8, 10)]


GPU_GROUPS = ("shapes", "distinct", "boundary")


def gpu_keys(group=None, **where):
    """every (key, dec) tests/test_gpu_mb444.py compares with the device byte for byte, which is the
    list the boundary mutants of tests/test_cpu_mutants.py are held to.  group: one of GPU_GROUPS
    (one test function each); where: bd / dec of one parametrised case of that function."""
    keys = {"shapes": [(k, dec) for bd in (8, 10) for dec in (0, 1) for k in case_keys(bd) if k[4] == "flat"],
            "distinct": [(k, 1) for bd in (8, 10) for k in DISTINCT_KEYS(bd)],
            "boundary": [(k, 1) for k in boundary_keys()]}
    keys = [kd for g in GPU_GROUPS if group in (None, g) for kd in keys[g]]
    pick = {"bd": lambda kd: kd[0][0], "dec": lambda kd: kd[1]}
    return [kd for kd in keys if all(pick[n](kd) == v for n, v in where.items())]


def key_size(kd):
    """macroblocks of a gpu_keys() entry: what its expected() costs"""
    return kd[0][1] * kd[0][2] * kd[0][3]
