"""x264_frame_deblock_row restated in numpy, from the reference's C (common/deblock.c), and the
inputs of tests/test_cpu_deblock.py and tests/test_gpu_deblock.py.  No GPU code.

* edge_luma / edge_chroma / edge_luma_intra / edge_chroma_intra: the line filters
  (deblock.c:79-109, 137-150, 183-221, 241-253) on the lines of one edge at once -- the lines of
  an edge do not read each other;
* deblock_edge / deblock_edge_intra (deblock.c:306-338), FILTER (deblock.c:417-447) and the
  macroblock loop (deblock.c:391-605 for SLICE_MBAFF == 0) in `deblock`, whose order= argument
  walks the macroblocks in "raster" order (x264's), by anti-diagonal x + 2y ("diag": what the
  device runs) or filters every vertical edge of the frame before the first horizontal one
  ("vh": a different picture, which is why the order matters);
* deblock_strength_py: deblock_strength_c (deblock.c:277-304) with the intra values of
  x264_macroblock_deblock_strength (macroblock.c:1441-1447), over whole frames;
* make_case / make_strength_case: the inputs.

The three tables are tests/golden/deblock_tables.json's (tests/golden/make_deblock_tables.py).
"""
import functools
import json
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "deblock_tables.json")) as _fh:
    _T = json.load(_fh)
ALPHA = np.array(_T["i_alpha_table"], np.int32)                  # alpha_table(x) = ALPHA[x + 24], deblock.c:74-76
BETA = np.array(_T["i_beta_table"], np.int32)
TC0 = np.array(_T["i_tc0_table"], np.int32).reshape(88, 4)


def pdt(bd):
    return np.uint8 if bd == 8 else np.uint16


def clip3(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


# ------------------------------------------------------------------ the line filters
# P: int32 [lines, 8] = p3 p2 p1 p0 q0 q1 q2 q3 across the edge (chroma: [lines, 4] = p1 p0 q0 q1), a
# view that is filtered in place; tc: one value per line
def edge_luma(P, alpha, beta, tc0, bd):
    """deblock_edge_luma_c, deblock.c:79-109; deblock_luma_c skips the lines whose tc0 < 0 (:114)"""
    tc0 = np.broadcast_to(np.asarray(tc0, np.int32), P.shape[:1])
    p2, p1, p0, q0, q1, q2 = (P[:, k].copy() for k in range(1, 7))
    f = (tc0 >= 0) & (abs(p0 - q0) < alpha) & (abs(p1 - p0) < beta) & (abs(q1 - q0) < beta)       # :88
    ap, aq = abs(p2 - p0) < beta, abs(q2 - q0) < beta                                             # :92, :98
    tc = tc0 + ap + aq                                                                            # :96, :102
    avg = (p0 + q0 + 1) >> 1
    P[:, 2] = np.where(f & ap & (tc0 != 0), p1 + clip3(((p2 + avg) >> 1) - p1, -tc0, tc0), p1)    # :95
    P[:, 5] = np.where(f & aq & (tc0 != 0), q1 + clip3(((q2 + avg) >> 1) - q1, -tc0, tc0), q1)    # :101
    delta = clip3((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc)                                # :105
    pm = (1 << bd) - 1
    P[:, 3] = np.where(f, clip3(p0 + delta, 0, pm), p0)                                           # :106
    P[:, 4] = np.where(f, clip3(q0 - delta, 0, pm), q0)                                           # :107


def edge_chroma(P, alpha, beta, tc, bd):
    """deblock_edge_chroma_c, deblock.c:137-150; deblock_chroma_c skips the lines whose tc <= 0 (:156)"""
    tc = np.broadcast_to(np.asarray(tc, np.int32), P.shape[:1])
    p1, p0, q0, q1 = (P[:, k].copy() for k in range(4))
    f = (tc > 0) & (abs(p0 - q0) < alpha) & (abs(p1 - p0) < beta) & (abs(q1 - q0) < beta)         # :144
    delta = clip3((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc)                                # :146
    pm = (1 << bd) - 1
    P[:, 1] = np.where(f, clip3(p0 + delta, 0, pm), p0)
    P[:, 2] = np.where(f, clip3(q0 - delta, 0, pm), q0)


def edge_luma_intra(P, alpha, beta):
    """deblock_edge_luma_intra_c, deblock.c:183-221"""
    p3, p2, p1, p0, q0, q1, q2, q3 = (P[:, k].copy() for k in range(8))
    f = (abs(p0 - q0) < alpha) & (abs(p1 - p0) < beta) & (abs(q1 - q0) < beta)                    # :192
    strong = abs(p0 - q0) < ((alpha >> 2) + 2)                                                    # :194
    sp, sq = f & strong & (abs(p2 - p0) < beta), f & strong & (abs(q2 - q0) < beta)               # :196, :205
    P[:, 3] = np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3,                         # :199
                       np.where(f, (2 * p1 + p0 + q1 + 2) >> 2, p0))                              # :204, :217
    P[:, 2] = np.where(sp, (p2 + p1 + p0 + q0 + 2) >> 2, p1)                                      # :200
    P[:, 1] = np.where(sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)                         # :201
    P[:, 4] = np.where(sq, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3,                         # :208
                       np.where(f, (2 * q1 + q0 + p1 + 2) >> 2, q0))                              # :213, :218
    P[:, 5] = np.where(sq, (p0 + q0 + q1 + q2 + 2) >> 2, q1)                                      # :209
    P[:, 6] = np.where(sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)                         # :210


def edge_chroma_intra(P, alpha, beta):
    """deblock_edge_chroma_intra_c, deblock.c:241-253"""
    p1, p0, q0, q1 = (P[:, k].copy() for k in range(4))
    f = (abs(p0 - q0) < alpha) & (abs(p1 - p0) < beta) & (abs(q1 - q0) < beta)                    # :248
    P[:, 1] = np.where(f, (2 * p1 + p0 + q1 + 2) >> 2, p0)
    P[:, 2] = np.where(f, (2 * q1 + q0 + p1 + 2) >> 2, q0)


# ------------------------------------------------------------------ deblock_edge, deblock_edge_intra
def alpha_beta(qp, a, b, bd):
    """deblock.c:309-312"""
    return int(ALPHA[qp + a + 24]) << (bd - 8), int(BETA[qp + b + 24]) << (bd - 8)


def deblock_edge(P, bS, per, qp, a, b, b_chroma, luma, bd):
    """deblock.c:306-324 on the lines P of one edge; bS[i] covers `per` lines (deblock.c:110-122,
    151-181: 4 for the luma filters and deblock_h_chroma_422, 2 for the other chroma filters)"""
    alpha, beta = alpha_beta(qp, a, b, bd)
    if not np.any(bS) or not alpha or not beta:                                                   # :315
        return
    tc = np.repeat(TC0[qp + a + 24][np.asarray(bS, np.int64)] * (1 << (bd - 8)) + b_chroma, per)  # :318-321
    (edge_luma if luma else edge_chroma)(P, alpha, beta, tc, bd)


def deblock_edge_intra(P, qp, a, b, luma, bd):
    """deblock.c:326-338"""
    alpha, beta = alpha_beta(qp, a, b, bd)
    if not alpha or not beta:
        return
    (edge_luma_intra if luma else edge_chroma_intra)(P, alpha, beta)


def _lines(plane, x0, y0, dir, at, lines, half):
    """the view [lines, 2 * half] across the edge `at` pixels into the block at (x0, y0): a vertical
    edge (dir 0) has rows for lines, a horizontal one (dir 1) columns"""
    if dir == 0:
        return plane[y0:y0 + lines, x0 + at - half:x0 + at + half]
    return plane[y0 + at - half:y0 + at + half, x0:x0 + lines].T


# ------------------------------------------------------------------ x264_frame_deblock_row
def deblock(c, order="raster"):
    """the planes deblock.c:378-606 leaves for the inputs `c` (make_case): (luma [nf, H, W], [chroma
    planes in c's layout]).  order: "raster", "diag" or "vh" (above)."""
    bd, cf, mbw, mbh = c.bd, c.cf, c.mbw, c.mbh
    qbd = 6 * (bd - 8)
    a, b = c.alpha_c0_offset - qbd, c.beta_offset - qbd                                           # :381-382
    qp_thresh = 15 - min(a, b) - max(0, c.chroma_qp_index_offset)                                 # :383
    Y = c.luma.astype(np.int32)
    if cf in (1, 2):
        U, V = c.chroma[0][..., 0::2].astype(np.int32), c.chroma[0][..., 1::2].astype(np.int32)
    elif cf == 3:
        U, V = c.chroma[0].astype(np.int32), c.chroma[1].astype(np.int32)
    ch = 8 if cf == 1 else 16                                                                     # :388
    qps = c.qp.reshape(c.nf, mbh, mbw).astype(np.int64)
    flags = c.mb_flags.reshape(c.nf, mbh, mbw)
    bs = c.bs.reshape(c.nf, mbh, mbw, 2, 4, 4)
    sl = None if c.slice_table is None else c.slice_table.reshape(c.nf, mbh, mbw)
    cqt = c.chroma_qp_table.astype(np.int64)

    def mb(f, mx, my, dirs):
        t8, intra_cur = bool(flags[f, my, mx] & 2), bool(flags[f, my, mx] & 1)                    # :397-398
        left = mx > 0 and (sl is None or sl[f, my, mx - 1] == sl[f, my, mx])                      # :370-372
        top = my > 0 and (sl is None or sl[f, my - 1, mx] == sl[f, my, mx])                       # :373-375
        qp = int(qps[f, my, mx])
        qpc = int(cqt[qp])                                                                        # :414
        first_edge_only = (bool(flags[f, my, mx] & 4) and not intra_cur) or qp <= qp_thresh       # :415

        def FILTER(intra, dir, edge, q, cq):                                                      # :417-447
            bS = bs[f, my, mx, dir, edge]

            def one(plane, x0, y0, at, lines, per, qq, luma):
                P = _lines(plane[f], x0, y0, dir, at, lines, 4 if luma else 2)
                if intra:
                    deblock_edge_intra(P, qq, a, b, luma, bd)
                else:
                    deblock_edge(P, bS, per, qq, a, b, 0 if luma else 1, luma, bd)
            if not (edge & 1) or not t8:                                                          # :420
                one(Y, 16 * mx, 16 * my, 4 * edge, 16, 4, q, True)                                # :422
                if cf == 3:                                                                       # :425-433
                    one(U, 16 * mx, 16 * my, 4 * edge, 16, 4, cq, True)
                    one(V, 16 * mx, 16 * my, 4 * edge, 16, 4, cq, True)
                elif cf == 1 and not (edge & 1):                                                  # :434-439
                    one(U, 8 * mx, 8 * my, 2 * edge, 8, 2, cq, False)
                    one(V, 8 * mx, 8 * my, 2 * edge, 8, 2, cq, False)
            if cf == 2 and (dir or not (edge & 1)):                                               # :441-446
                at, lines, per = (4 * edge, 8, 2) if dir else (2 * edge, 16, 4)
                one(U, 8 * mx, 16 * my, at, lines, per, cq, False)
                one(V, 8 * mx, 16 * my, at, lines, per, cq, False)

        for dir in dirs:
            nb = left if dir == 0 else top
            if nb:                                                                                # :449, :543
                fn, qn = (flags[f, my, mx - 1], qps[f, my, mx - 1]) if dir == 0 else \
                         (flags[f, my - 1, mx], qps[f, my - 1, mx])
                qe = (qp + int(qn) + 1) >> 1                                                      # :515, :572
                qce = (qpc + int(cqt[int(qn)]) + 1) >> 1                                          # :516, :573
                FILTER(intra_cur or bool(fn & 1), dir, 0, qe, qce)                                # :530-533, :584-593
            if not first_edge_only:                                                               # :536, :597
                for edge in (1, 2, 3):
                    FILTER(False, dir, edge, qp, qpc)

    cells = [(mx, my) for my in range(mbh) for mx in range(mbw)]
    if order == "diag":
        cells.sort(key=lambda p: (p[0] + 2 * p[1], p[1]))
    for f in range(c.nf):
        if order == "vh":
            for d in (0, 1):
                for mx, my in cells:
                    mb(f, mx, my, (d,))
        else:
            assert order in ("raster", "diag")
            for mx, my in cells:
                mb(f, mx, my, (0, 1))
    dt = pdt(bd)
    if cf == 0:
        return Y.astype(dt), []
    if cf == 3:
        return Y.astype(dt), [U.astype(dt), V.astype(dt)]
    nv = np.empty(c.chroma[0].shape, dt)
    nv[..., 0::2], nv[..., 1::2] = U, V
    return Y.astype(dt), [nv]


# ------------------------------------------------------------------ deblock_strength
def deblock_strength_py(nz, mb_flags, mv, ref, mbw, mbh, nf, mvy_limit=4):
    """bs [nf * mbh * mbw, 2, 4, 4] (include/x264hip_deblock.h's rule): mv = [mv0] or [mv0, mv1]
    ([nf, 4 mbh, 4 mbw, 2]), ref likewise ([nf, 2 mbh, 2 mbw]).  Whole 4x4-block grids at once."""
    flags = mb_flags.reshape(nf, mbh, mbw)
    nzm = nz.reshape(nf, mbh, mbw).astype(np.int64)
    by, bx = np.mgrid[0:4, 0:4]
    i8 = (by >> 1) * 2 + (bx >> 1)
    bit4, bit8 = 4 * i8 + (by & 1) * 2 + (bx & 1), i8
    t8 = (flags & 2 != 0)[..., None, None]
    nzb = (nzm[..., None, None] >> np.where(t8, bit8, bit4)) & 1                    # [nf, mbh, mbw, 4, 4] (by, bx)
    nzg = nzb.transpose(0, 1, 3, 2, 4).reshape(nf, 4 * mbh, 4 * mbw)
    intra = np.repeat(np.repeat(flags & 1 != 0, 4, 1), 4, 2)
    out = np.zeros((nf, mbh, mbw, 2, 4, 4), np.uint8)
    for dir in (0, 1):
        def prev(g):
            """g at the block before each one across the edge (the first row / column: itself)"""
            p = g.copy()
            if dir == 0:
                p[:, :, 1:] = g[:, :, :-1]
            else:
                p[:, 1:] = g[:, :-1]
            return p
        v = np.zeros((nf, 4 * mbh, 4 * mbw), bool)
        for m, r in zip(mv, ref):                                                   # deblock.c:291-296
            r4 = np.repeat(np.repeat(r, 2, 1), 2, 2).astype(np.int64)
            m = m.astype(np.int64)
            v |= (r4 != prev(r4)) | (abs(m[..., 0] - prev(m[..., 0])) >= 4) | (abs(m[..., 1] - prev(m[..., 1])) >= mvy_limit)
        s = np.where((nzg | prev(nzg)) != 0, 2, v.astype(np.int64))                 # deblock.c:289-301
        gy, gx = np.mgrid[0:4 * mbh, 0:4 * mbw]
        pos = gx if dir == 0 else gy
        mb_edge = pos % 4 == 0
        s = np.where(intra & ~mb_edge, 3, s)                                        # macroblock.c:1441-1447
        s = np.where(mb_edge & (intra | prev(intra)), 4, s)
        s = np.where(pos == 0, 0, s)                                                # the picture border
        s = s.reshape(nf, mbh, 4, mbw, 4).transpose(0, 1, 3, 2, 4)                  # [nf, mbh, mbw, by, bx]
        out[:, :, :, dir] = s.transpose(0, 1, 2, 4, 3) if dir == 0 else s           # [edge][i]: dir 0 = [bx][by]
    return out.reshape(-1, 2, 4, 4)


# ------------------------------------------------------------------ inputs
def chroma_qp_table(bd, offset=0):
    """h->chroma_qp_table[0 .. QP_MAX_SPEC]: H.264 table 8-15 shifted by QP_BD_OFFSET"""
    bdo = 6 * (bd - 8)
    tail = [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
    out = np.zeros(52 + bdo, np.uint8)
    for qp in range(52 + bdo):
        q = min(max(qp + offset, 0), 51 + bdo)
        out[qp] = q if q - bdo < 30 else tail[q - bdo - 30] + bdo
    return out


def picture(rs, nf, w, h, bd, bw=4, bh=4):
    """a smooth ramp, a per-block offset in +-5 (blocks of bw x bh: the transform blocks of the
    plane) and noise in +-1, times 4 at 10 bit: blocking the filter acts on"""
    y, x = np.mgrid[0:h, 0:w]
    ramp = 48 + abs(((x + y) >> 2) % 320 - 160)
    out = np.empty((nf, h, w), np.int64)
    for f in range(nf):
        off = rs.integers(-5, 6, ((h + bh - 1) // bh, (w + bw - 1) // bw))
        blk = np.repeat(np.repeat(off, bh, 0), bw, 1)[:h, :w]
        out[f] = ramp + 3 * f + blk + rs.integers(-1, 2, (h, w))
    return (np.clip(out, 0, 255) << (bd - 8)).astype(pdt(bd))


@functools.lru_cache(maxsize=None)
def make_case(bd, cf, mbw, mbh, nf=1, seed=1, offsets=(0, 0), qp_lo=30, qp_hi=51, slices=False, cqio=0):
    """the inputs of one deblock_frames call (read-only: cached and shared between tests).  qp per
    MB random in qp_lo..qp_hi, about 20 % of the MBs intra, 30 % transform 8x8, 15 % with flag bit
    2; bs random in {0, 1, 2} with 3 on the inner edges of intra MBs; slices: two slices split in
    the middle of a row."""
    rs = np.random.default_rng([seed, bd, cf, mbw, mbh, nf])
    n = nf * mbw * mbh
    w, h = 16 * mbw, 16 * mbh
    luma = picture(rs, nf, w, h, bd)
    if cf == 0:
        chroma = []
    elif cf == 3:
        chroma = [picture(rs, nf, w, h, bd), picture(rs, nf, w, h, bd)]
    else:
        ch = h // 2 if cf == 1 else h
        nv = np.empty((nf, ch, w), pdt(bd))
        nv[..., 0::2] = picture(rs, nf, w // 2, ch, bd)
        nv[..., 1::2] = picture(rs, nf, w // 2, ch, bd)
        chroma = [nv]
    qp = rs.integers(qp_lo, qp_hi + 1, n).astype(np.int8)
    r = rs.random((3, n))
    flags = ((r[0] < 0.2) * 1 + (r[1] < 0.3) * 2 + (r[2] < 0.15) * 4).astype(np.uint8)
    bs = rs.integers(0, 3, (n, 2, 4, 4)).astype(np.uint8)
    bs[(flags & 1) != 0, :, 1:] = 3
    slice_table = None
    if slices:
        first = (mbh // 2) * mbw + mbw // 2                     # the second slice starts mid-row
        slice_table = np.tile((np.arange(mbw * mbh) >= first).astype(np.int32), nf)
    c = types.SimpleNamespace(bd=bd, cf=cf, mbw=mbw, mbh=mbh, nf=nf, luma=luma, chroma=chroma, qp=qp, mb_flags=flags,
                              bs=bs, slice_table=slice_table, alpha_c0_offset=offsets[0], beta_offset=offsets[1],
                              chroma_qp_index_offset=cqio, chroma_qp_table=chroma_qp_table(bd, cqio))
    for arr in [luma, qp, flags, bs] + chroma + ([slice_table] if slices else []):
        arr.setflags(write=False)
    return c


def with_(c, **kw):
    """a copy of the inputs with fields replaced"""
    d = dict(vars(c))
    d.update(kw)
    return types.SimpleNamespace(**d)


@functools.lru_cache(maxsize=None)
def expected(key, order="raster"):
    """deblock( make_case( *key ), order ), computed once"""
    return deblock(make_case(*key), order)


@functools.lru_cache(maxsize=None)
def make_strength_case(mbw, mbh, nf, bframe, seed=1):
    """nz as mb_dct_quant writes it (16 bits for a transform-4 MB, 4 for a transform-8 one), about
    20 % intra MBs (ref -1, no vectors) and 30 % transform 8x8; references per 8x8 block mostly 0;
    vectors = a common base plus a per-block step from {0, +-3, +-4} and, vertically, {+-1, +-2}
    too, so neighbouring differences straddle 4 and an mvy_limit of 2 or 4"""
    rs = np.random.default_rng([seed, mbw, mbh, nf, bframe])
    n = nf * mbw * mbh
    r = rs.random((2, n))
    flags = ((r[0] < 0.2) * 1 + (r[1] < 0.3) * 2).astype(np.uint8)
    nz = np.where(flags & 2, rs.integers(0, 16, n) & rs.integers(0, 16, n),
                  rs.integers(0, 1 << 16, n) & rs.integers(0, 1 << 16, n) & rs.integers(0, 1 << 16, n)).astype(np.int32)
    nz[rs.random(n) < 0.3] = 0
    intra8 = np.repeat(np.repeat((flags & 1).reshape(nf, mbh, mbw) != 0, 2, 1), 2, 2)
    mvs, refs = [], []
    for _ in range(2 if bframe else 1):
        ref = np.where(rs.random((nf, 2 * mbh, 2 * mbw)) < 0.85, 0, 1).astype(np.int8)
        ref[intra8] = -1
        mv = np.empty((nf, 4 * mbh, 4 * mbw, 2), np.int16)
        mv[..., 0] = 20 + rs.choice([0, 0, 0, 0, 3, -3, 4, -4], (nf, 4 * mbh, 4 * mbw))
        mv[..., 1] = -8 + rs.choice([0, 0, 0, 0, 1, -1, 2, -2, 3, -3, 4, -4], (nf, 4 * mbh, 4 * mbw))
        mv[np.repeat(np.repeat(intra8, 2, 1), 2, 2)] = 0
        mvs.append(mv)
        refs.append(ref)
    for arr in [flags, nz] + mvs + refs:
        arr.setflags(write=False)
    return types.SimpleNamespace(mbw=mbw, mbh=mbh, nf=nf, bframe=bframe, nz=nz, mb_flags=flags, mv=mvs, ref=refs)


# ------------------------------------------------------------------ the GPU cases (tests/test_gpu_deblock.py)
# key = make_case's arguments: (bd, cf, mbw, mbh, nf, seed, offsets, qp_lo, qp_hi, slices, cqio)
def key(bd, cf, mbw, mbh, nf=1, seed=1, offsets=(0, 0), qp_lo=30, qp_hi=51, slices=False, cqio=0):
    return (bd, cf, mbw, mbh, nf, seed, offsets, qp_lo, qp_hi, slices, cqio)


MAIN = [key(bd, 1, 5, 4, offsets=o) for bd in (8, 10) for o in ((0, 0), (-4, 2), (6, -6))]
FORMATS = [key(8, 0, 5, 4), key(8, 2, 5, 4), key(8, 3, 5, 4), key(10, 3, 5, 4)]
SHAPES = [key(8, 1, w, h, seed=2) for w, h in ((1, 1), (1, 5), (5, 1), (2, 2))]
FRAMES = [key(8, 1, 7, 5, nf=3, seed=3), key(10, 1, 7, 5, nf=3, seed=3)]
LONG = [key(bd, 1, 24, 14, nf=2, seed=4) for bd in (8, 10)]
LOW_QP = [key(bd, 1, 5, 4, seed=5, qp_lo=0, qp_hi=15) for bd in (8, 10)]
TOP = [key(8, 1, 5, 4, seed=6, offsets=(12, 12), qp_lo=51, qp_hi=51),
       key(10, 1, 5, 4, seed=6, offsets=(12, 12), qp_lo=63, qp_hi=63),
       key(10, 2, 5, 4, seed=6, offsets=(12, 12), qp_lo=63, qp_hi=63, cqio=4)]
SLICES = [key(8, 1, 5, 4, seed=7, slices=True), key(10, 2, 5, 4, seed=7, slices=True)]
# every input the GPU tests run; ACTIVE: those the activity conditions of test_cpu_deblock.py hold
# for (the low-qp inputs are there to show that nothing changes)
ACTIVE = MAIN + FORMATS + FRAMES + LONG + TOP + SLICES
ALL = ACTIVE + SHAPES + LOW_QP


def case_id(k):
    bd, cf, mbw, mbh, nf, seed, off, lo, hi, sl, cqio = k
    return "%dbit-cf%d-%dx%dx%d-o%d,%d-qp%d..%d%s" % (bd, cf, mbw, mbh, nf, off[0], off[1], lo, hi, "-slices" if sl else "")


# ------------------------------------------------------------------ what the GPU tests compare
STRENGTH_SHAPES = ((5, 4, 2), (24, 14, 1))
# The boundary pictures of deblock_frames, (what is pinned, key): 2x2 macroblocks at the foot of the
# qp range where alpha and beta are small (4..15 and 2..6 times the depth's scale), so that the
# steps of picture() -- block offsets in +-5, noise in +-1 -- land on them, one below and one above.
# At each depth these pictures alone tell every flipped alpha / beta / tc0 comparison of the line
# filters from the checker (tests/test_cpu_deblock.py); the seeds were found by search.
def _low(bd, cf, seed):
    lo = 16 + 6 * (bd - 8)
    return key(bd, cf, 2, 2, seed=seed, qp_lo=lo, qp_hi=lo + 11)


BOUNDARY = [("alpha / beta / tc0 ties, %d bit, format %d, seed %d" % (bd, cf, seed), _low(bd, cf, seed))
            for bd, cf, seed in ((8, 1, 22), (8, 1, 21), (8, 2, 24), (8, 3, 28), (10, 2, 24), (10, 1, 20), (10, 3, 28))]
# deblock_strength: vector steps of exactly 4 (and mvy_limit) next to 3 and less, on one small field each way
BOUNDARY_STRENGTH = [("mv steps at the limit", (2, 2, 1, bf), lim) for bf in (False, True) for lim in (4, 2)]
GPU_GROUPS = ("frames", "low_qp", "slices", "strength", "boundary")


def boundary_keys():
    return [e[1] for e in BOUNDARY]


def gpu_keys(group=None):
    """every entry tests/test_gpu_deblock.py compares with the device value for value, which is the
    list the boundary mutants of tests/test_cpu_mutants.py are held to: ("frames", key) for
    deblock_frames, ("strength", (mbw, mbh, nf, bframe), mvy_limit) for deblock_strength.  group:
    one of GPU_GROUPS (one test function each)."""
    keys = {"frames": [("frames", k) for k in MAIN + FORMATS + SHAPES + FRAMES + LONG + TOP],
            "low_qp": [("frames", k) for k in LOW_QP], "slices": [("frames", k) for k in SLICES],
            "strength": [("strength", sh + (bf,), lim) for lim in (4, 2) for bf in (False, True) for sh in STRENGTH_SHAPES],
            "boundary": [("frames", k) for k in boundary_keys()] + [("strength",) + tuple(e[1:]) for e in BOUNDARY_STRENGTH]}
    return [e for g in GPU_GROUPS if group in (None, g) for e in keys[g]]


def gpu_expected(entry):
    """what the device's output of a gpu_keys() entry is compared with"""
    if entry[0] == "frames":
        return expected(entry[1])
    s = make_strength_case(*entry[1])
    return deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf, entry[2])


def key_size(entry):
    """macroblocks of a gpu_keys() entry: what it costs"""
    k = entry[1]
    return k[2] * k[3] * k[4] if entry[0] == "frames" else k[0] * k[1] * k[2] // 8 + 1
