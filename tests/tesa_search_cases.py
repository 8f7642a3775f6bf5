"""The literal Python restatement of x264_me_search_ref with X264_ME_TESA for one partition of any
size (reference encoder/me.c:214-318 predictor stage, :618-749 window, :774-789 qpel conversion)
and the inputs of tests/test_cpu_tesa_search.py and tests/test_gpu_tesa_search.py.

The oracle has no TESA for partitions, so this restatement is the checker of
x264hip_*_me_search_ref_tesa; test_cpu_tesa_search.py pins it piecewise to what the oracle has:
with me_method 3 and fpelcmp = SAD it is oracle.me_search_ref's ESA (predictor stage, qpel
conversion), its 16x16 window is oracle.me_tesa's and tesa_cases.tesa_python's, and every row's
ADS survivors are oracle.ads' on oracle.frame_integral's sums.  The predictor stage's SATD form
and the windows of the other sizes rest on this restatement alone.  The per-row ADS and SADs are
numpy over the row; the list logic keeps the reference's statements."""
import collections

import numpy as np

import numpy_ref as nr
import refine_cases as rc
import search_cases as sc
from degenerate_cases import flat_case  # noqa: F401  (the near-flat case lives with the other degenerate content)
from test_cpu_refine_chroma import _weigh

PAD = 32
# how often the restatement took each path worth a test: rows skipped on bsad <= ycost, windows of
# width 0, empty survivor lists of scanned windows, passes of the halving loop, entries the second
# loop dropped
HITS = collections.Counter()


def _pack(a, b):
    return (a & 0xFFFF) | ((b & 0xFFFF) << 16)


def _s16(v):
    return v - 65536 if v >= 32768 else v


def ads_layout(i_pixel, stride):
    """(sad_size edge, enc_dc block offsets (x, y), integral offsets, delta) of the partition's ads
    (me.c:637-651; ads4 / ads2 / ads1 by size, pixel.c:840-842, 1605-1608)"""
    s = 8 if i_pixel <= 3 else 4
    delta = s * stride if i_pixel in (0, 2, 5) else s
    if i_pixel == 0:                                       # ads4: sums[0], [8], [delta], [delta + 8]
        return s, [(0, 0), (s, 0), (0, s), (s, s)], [0, 8, delta, delta + 8], delta
    if i_pixel in (3, 6):                                  # ads1
        return s, [(0, 0)], [0], delta
    # ads2: enc_dc[0], enc_dc[1] (= the block below for 8x16 / 4x8, me.c:650-651) at sums[0], [delta]
    return s, [(0, 0), (0, s) if i_pixel in (2, 5) else (s, 0)], [0, delta], delta


def tesa_window_py(i_pixel, fb, fw, origin, stride, x, y, integral, i_org, lines, mvp, lim, cm, c0, me_range, bmx, bmy,
                   bcost, fpelcmp, me_method=4, on_row=None):
    """the window stage (me.c:621-749) around (bmx, bmy) with cost bcost: fb the fenc block, fw the
    plane the integer search reads ((0,0) at `origin`), integral the uint16 sums plane of the
    partition's sad_size with (0,0) at i_org (lines = the frame's height: every sum read must lie
    in the region frame_integral writes), mvp qpel, lim = (xmin, ymin, xmax, ymax), fpelcmp(a, b)
    the final COST_MV's compare.  me_method 3: the exhaustive form of :627-631.  on_row(my, enc_dc,
    sums offset, delta, cost_fpel_mvx, width, thresh, xs): called with every row's ADS call.
    Returns (bcost, bmx, bmy, COST_MV calls, scan SAD calls, nmvsad before the prunes)."""
    bw, bh = nr.SIZES[i_pixel]
    xmin, ymin, xmax, ymax = lim
    cx = lambda v: int(cm[c0 + v - mvp[0]])                # noqa: E731  p_cost_mvx[v]
    cy = lambda v: int(cm[c0 + v - mvp[1]])                # noqa: E731
    p2 = fw.reshape(-1, stride)
    oy, ox = divmod(origin, stride)
    ref_at = lambda mx, my: p2[oy + y + my:oy + y + my + bh, ox + x + mx:ox + x + mx + bw].astype(np.int64)  # noqa: E731
    min_x, min_y = max(bmx - me_range, xmin), max(bmy - me_range, ymin)
    max_x, max_y = min(bmx + me_range, xmax), min(bmy + me_range, ymax)
    width = (max_x - min_x + 3) & ~3
    if width == 0:
        HITS["width0"] += 1
    if me_method == 3:
        n = 0
        for my in range(min_y, max_y + 1):
            for mx in range(min_x, min_x + width):
                n += 1
                c = nr.sad(fb, ref_at(mx, my)) + cx(4 * mx) + cy(4 * my)
                if c < bcost:
                    bcost, bmx, bmy = c, mx, my
        return bcost, bmx, bmy, n, 0, 0
    s, blocks, offs, delta = ads_layout(i_pixel, stride)
    enc_dc = [int(fb[by:by + s, bx:bx + s].sum()) for bx, by in blocks]
    xcost = np.array([cx(4 * (min_x + i)) for i in range(width)], np.int64)
    sad_thresh = 10 if me_range <= 16 else 11 if me_range <= 24 else 12
    bsad = nr.sad(fb, ref_at(bmx, bmy)) + cx(4 * bmx) + cy(4 * bmy)
    nscan = 1
    mvsads = []
    for my in range(min_y, max_y + 1):
        ycost = cy(4 * my)
        if bsad <= ycost:
            HITS["row_skip"] += 1
            continue
        bsad -= ycost
        thresh = bsad * 17 >> 4
        xs = []
        if width:
            # every sum read lies in the rows [1 - 32, lines + 32 - 8) and the columns
            # [-32, stride - 32 - 8) frame_integral writes (x264hip.h, frame_integral)
            srow, scol = y + my, x + min_x
            last = max(offs)
            assert 1 - PAD <= srow and srow + last // stride < lines + PAD - 8, (srow, last)
            assert -PAD <= scol and scol + width - 1 + last % stride < stride - PAD - 8, (scol, width)
            base = i_org + srow * stride + scol
            ads = xcost.copy()
            for dc, o in zip(enc_dc, offs):
                ads += np.abs(dc - integral[base + o:base + o + width].astype(np.int64))
            xs = [int(i) for i in np.nonzero(ads < thresh)[0]]
        if on_row is not None:
            on_row(my, enc_dc, i_org + (y + my) * stride + x + min_x, delta, xcost.astype(np.uint16), width, thresh, xs)
        if xs:
            strip = p2[oy + y + my:oy + y + my + bh, ox + x + min_x:ox + x + min_x + width + bw - 1].astype(np.int64)
            win = np.lib.stride_tricks.sliding_window_view(strip, bw, axis=1)          # [bh, width, bw]
            sads = np.abs(win - fb[:, None, :]).sum(axis=(0, 2))
        for i in xs:
            nscan += 1
            mx = min_x + i
            sad = int(sads[i]) + int(xcost[i])
            if sad < bsad * sad_thresh >> 3:
                if sad < bsad:
                    bsad = sad
                mvsads.append([sad + ycost, mx, my])
        bsad += ycost
    nlist = nmvsad = len(mvsads)
    if not nmvsad and width:
        HITS["empty_list"] += 1
    limit = me_range >> 1
    sad_thresh = bsad * sad_thresh >> 3
    while nmvsad > limit * 2 and sad_thresh > bsad:
        HITS["halve"] += 1
        sad_thresh = (sad_thresh + bsad) >> 1
        i = 0
        while i < nmvsad and mvsads[i][0] <= sad_thresh:
            i += 1
        for j in range(i, nmvsad):
            mvsads[i] = list(mvsads[j])
            sad = mvsads[j][0] & 0xFFFFFFFF
            i += ((sad - (sad_thresh + 1)) & 0xFFFFFFFF) >> 31
        nmvsad = i
    while nmvsad > limit:
        HITS["drop_max"] += 1
        bi = 0
        for i in range(1, nmvsad):
            if mvsads[i][0] > mvsads[bi][0]:
                bi = i
        nmvsad -= 1
        mvsads[bi] = list(mvsads[nmvsad])
    for k in range(nmvsad):
        _, mx, my = mvsads[k]
        c = fpelcmp(fb, ref_at(mx, my)) + cx(4 * mx) + cy(4 * my)
        if c < bcost:
            bcost, bmx, bmy = c, mx, my
    return bcost, bmx, bmy, nmvsad, nscan, nlist


def search_ref_tesa_py(fenc, planes, fw, origin, stride, x, y, i_pixel, par, mvc, cm, c0, subme, me_range, integral,
                       i_org, lines, me_method=4, fpel_satd=True, weight0=None, bd=8, on_row=None, stage=None):
    """x264_me_search_ref's integer stage with ESA (me_method 3) or TESA (4) for one partition:
    the predictor stage (me.c:214-318) with fpelcmp = SATD when fpel_satd and subme > 1
    (encoder.c:1423-1426), tesa_window_py, the qpel conversion (me.c:774-789).  integral: the
    sums plane of the partition's sad_size.  stage: a dict that receives the predictor stage's
    bmx, bmy, bcost and pmv.  Returns (cost, mvx, mvy, cost_mv), (fpelcmp calls, get_ref calls),
    (scan SAD calls, nmvsad before the prunes)."""
    bw, bh = nr.SIZES[i_pixel]
    fb = nr.block(fenc, origin + y * stride + x, stride, bw, bh)
    fpelcmp = nr.satd if fpel_satd and subme > 1 else nr.sad
    nf = [0, 0]

    def fpel(mx, my):
        nf[0] += 1
        return fpelcmp(fb, nr.block(fw, origin + (y + my) * stride + x + mx, stride, bw, bh))

    def hpel(mx, my):                                          # COST_MV_HPEL's compare (me.c:72-79)
        nf[1] += 1
        return fpelcmp(fb, _weigh(nr.get_ref(planes, origin + y * stride + x, stride, mx, my, bw, bh), weight0, bd))

    mvp = (int(par[0]), int(par[1]))
    xmin, ymin, xmax, ymax = (int(v) for v in par[2:6])
    i_mvc = int(par[10])
    cmx = lambda v: int(cm[c0 + v - mvp[0]])                    # noqa: E731
    cmy = lambda v: int(cm[c0 + v - mvp[1]])                    # noqa: E731
    bits = lambda mx, my: cmx(4 * mx) + cmy(4 * my)             # noqa: E731
    clip = lambda v, lo, hi: min(max(v, lo), hi)                # noqa: E731
    st = {"bcost": 1 << 28}

    def cost_mv(mx, my):
        c = fpel(mx, my) + bits(mx, my)
        if c < st["bcost"]:
            st["bcost"], st["bmx"], st["bmy"] = c, mx, my

    bpred_cost, bpred_mv = 1 << 28, 0
    if subme >= 3:                                             # me.c:214-283
        bpx, bpy = clip(mvp[0], 4 * xmin, 4 * xmax), clip(mvp[1], 4 * ymin, 4 * ymax)
        pmv = _pack(bpx, bpy)
        bpred_cost = hpel(bpx, bpy) + cmx(bpx) + cmy(bpy)
        pmv_cost = bpred_cost
        valid = []
        for i in range(i_mvc):                                 # x264_predictor_clip
            v = _pack(int(mvc[i][0]), int(mvc[i][1]))
            if not v or v == pmv:
                continue
            valid.append((clip(int(mvc[i][0]), 4 * xmin, 4 * xmax), clip(int(mvc[i][1]), 4 * ymin, 4 * ymax)))
        if valid:
            tmp = [None, (bpx, bpy)] + valid
            bpred_cost <<= 4
            for i in range(1, len(valid) + 1):
                mx, my = tmp[i + 1]
                c = hpel(mx, my) + cmx(mx) + cmy(my)
                if (c << 4) + i < bpred_cost:
                    bpred_cost = (c << 4) + i
            bpx, bpy = tmp[(bpred_cost & 15) + 1]
            bpred_cost >>= 4
        st["bmx"], st["bmy"] = (bpx + 2) >> 2, (bpy + 2) >> 2
        bpred_mv = _pack(bpx, bpy)
        if bpred_mv & 0x00030003:
            cost_mv(st["bmx"], st["bmy"])
        else:
            st["bcost"] = bpred_cost
        if pmv:
            if st["bmx"] | st["bmy"]:
                cost_mv(0, 0)
        elif pmv_cost < st["bcost"]:
            st["bcost"], st["bmx"], st["bmy"] = pmv_cost, 0, 0
    else:                                                      # me.c:284-318
        pmx = clip((mvp[0] + 2) >> 2, xmin, xmax)
        pmy = clip((mvp[1] + 2) >> 2, ymin, ymax)
        st["bmx"], st["bmy"] = pmx, pmy
        pmv = _pack(pmx, pmy)
        st["bcost"] = fpel(pmx, pmy)
        valid = []
        for i in range(i_mvc):                                 # x264_predictor_roundclip
            mx, my = (int(mvc[i][0]) + 2) >> 2, (int(mvc[i][1]) + 2) >> 2
            v = _pack(mx, my)
            if not v or v == pmv:
                continue
            valid.append((clip(mx, xmin, xmax), clip(my, ymin, ymax)))
        if valid:
            tmp = [None, (pmx, pmy)] + valid
            b = st["bcost"] << 4
            for i in range(1, len(valid) + 1):
                mx, my = tmp[i + 1]
                c = fpel(mx, my) + bits(mx, my)
                if (c << 4) + i < b:
                    b = (c << 4) + i
            st["bmx"], st["bmy"] = tmp[(b & 15) + 1]
            st["bcost"] = b >> 4
        if pmv:
            cost_mv(0, 0)

    if stage is not None:
        stage.update(bmx=st["bmx"], bmy=st["bmy"], bcost=st["bcost"], pmv=pmv)
    bcost, bmx, bmy, n, nscan, nlist = tesa_window_py(
        i_pixel, fb, fw, origin, stride, x, y, integral, i_org, lines, mvp, (xmin, ymin, xmax, ymax), cm, c0,
        me_range, st["bmx"], st["bmy"], st["bcost"], fpelcmp, me_method, on_row)
    nf[0] += n
    if subme < 3:                                              # me.c:774-789
        cmv = bits(bmx, bmy)
        return (bcost + (cmv if _pack(bmx, bmy) == pmv else 0), 4 * bmx, 4 * bmy, cmv), tuple(nf), (nscan, nlist)
    if bpred_cost < bcost:
        mx, my = _s16(bpred_mv & 0xFFFF), _s16(bpred_mv >> 16)
    else:
        mx, my = 4 * bmx, 4 * bmy
    return (min(bpred_cost, bcost), mx, my, cmx(mx) + cmy(my)), tuple(nf), (nscan, nlist)


def refine_fpel_satd_py(*args, **kw):
    """test_cpu_refine_chroma.refine_chroma_py with fpelcmp = SATD (TESA at subme > 1): its
    fpelcmp calls are its numpy_ref.sad calls -- the predictor's subpel component and the halfpel
    diamond (me.c:889-917) -- so it runs over a numpy_ref whose sad is satd.  Counted as SADs there;
    the result moves them to the SATD field, where the oracle counts them.  Only with chroma ME on
    (args[10], i_pixel <= PIXEL_8x8): the SATD re-score of the halfpel winner (me.c:920-924) then
    runs as refine_chroma_py has it; with mbcmp = fpelcmp and no chroma ME the reference skips it"""
    import test_cpu_refine_chroma as trc
    assert args[10] and args[3] <= 3

    class FpelSatd:
        def __getattr__(self, k):
            return nr.satd if k == "sad" else getattr(nr, k)

    trc.nr = FpelSatd()
    try:
        res, n = trc.refine_chroma_py(*args, **kw)
    finally:
        trc.nr = nr
    return res, (((n & 0xFFFF) + ((n >> 16) & 0xFF)) << 16) | (n & 0xFF000000)


# ---------------------------------------------------------------- inputs
def degenerate_jobs(mbw, mbh, i_pixel, seed):
    """search_cases.jobs with every third partition's x limits equal (a window of width 0) and
    every fifth's y limits equal (one row), at the predictor's rounded position"""
    pos, par, mvc = sc.jobs(mbw, mbh, 1, i_pixel, seed=seed)
    for i in range(len(par)):
        px = int(np.clip((int(par[i, 0]) + 2) >> 2, par[i, 2], par[i, 4]))
        py = int(np.clip((int(par[i, 1]) + 2) >> 2, par[i, 3], par[i, 5]))
        if i % 3 == 0:
            par[i, 2] = par[i, 4] = px
        if i % 5 == 0:
            par[i, 3] = par[i, 5] = py
    return pos, par, mvc


def corner_rows(pos, par, mvc, mbw, mbh):
    """the partitions of the first MB row and the four corner MBs (a short checker run that still
    meets every frame edge)"""
    mbx, mby = pos[:, 1] // 16, pos[:, 2] // 16
    sel = (mby == 0) | (((mbx == 0) | (mbx == mbw - 1)) & (mby == mbh - 1))
    return pos[sel], par[sel], mvc[sel]


def edge_inputs(bd, i_pixel):
    """the edge test's runs as (cases, jobs, cost table, subme, chroma ME, W, H): degenerate limits
    (windows of width 0, one-row windows); near-flat content under a high-lambda mv cost (rows
    skipped on bsad <= ycost), under lambda 1 (bsad of a few units: bsad * sad_thresh >> 3 = bsad,
    so even the centre fails the strict < and scanned windows leave empty lists) and under a zero
    table (SAD ties by the hundred through both prune loops); a 336x48 frame (another stride, mv
    limits down to -16 * 20 - 24).  The sub-8x8 sizes run on corner_rows' partitions"""
    def jobs(mbw, mbh, j):
        return corner_rows(*j, mbw, mbh) if i_pixel >= 4 else j
    W, H = 96, 64
    runs = [([rc.ChromaCase(bd, W, H, 1, seed=bd)], jobs(6, 4, degenerate_jobs(6, 4, i_pixel, 2)), rc.cost_mv(), 4, 0,
             W, H)]
    flat = [flat_case(bd, W, H, 1, seed=4 + bd)]
    for lam in (600, 1, 0):
        runs.append((flat, jobs(6, 4, sc.jobs(6, 4, 1, i_pixel, seed=bd + 1)), rc.cost_mv(lam=lam), 1, 0, W, H))
    runs.append(([rc.ChromaCase(bd, 336, 48, 1, seed=bd + 1)], jobs(21, 3, sc.jobs(21, 3, 1, i_pixel, seed=bd + 8)),
                 rc.cost_mv(), 7, 1, 336, 48))
    return runs


def integral_planes(oracle, bd, plane, origin, stride, lines):
    """oracle.frame_integral(sub8x8) as (flat uint16 buffer, i_org of the 8x8 plane, of the 4x4)"""
    buf = oracle.frame_integral(bd, plane, origin, stride, lines, PAD, True).ravel()
    i8 = PAD * stride + PAD
    return buf, i8, i8 + stride * (lines + 2 * PAD)


def expected(oracle, bd, cc, fw, i_pixel, subme, me_range, pos_xy, par, mvc, cm, c0, integ, weights, chroma, cf,
             fpel_satd=True):
    """the whole call for one frame's partitions: search_ref_tesa_py, then the oracle's
    refine_subpel with fpelcmp = SATD; returns out [n, 4], nevals [n, 2], scan [n, 2]"""
    buf, i8, i4 = integ
    n = len(pos_xy)
    out = np.zeros((n, 4), np.int32)
    ne = np.zeros((n, 2), np.int32)
    scan = np.zeros((n, 2), np.int32)
    for i in range(n):
        x, y = int(pos_xy[i, 0]), int(pos_xy[i, 1])
        r, nf, sn = search_ref_tesa_py(cc.fenc_y, cc.luma, fw, cc.origin, cc.stride, x, y, i_pixel, par[i], mvc[i], cm,
                                       c0, subme, me_range, buf, i8 if i_pixel <= 3 else i4, cc.H,
                                       fpel_satd=fpel_satd, weight0=weights[0], bd=bd)
        out[i], ne[i, 0], scan[i] = r, nf[0] | (nf[1] << 16), sn
    if subme >= 2:
        rpar = np.stack([out[:, 1], out[:, 2], par[:, 0], par[:, 1], par[:, 6], par[:, 7], par[:, 8], par[:, 9]],
                        1).astype(np.int16)
        out, ne[:, 1] = oracle.me_refine_subpel(
            bd, cc.fenc_y, cc.origin, cc.stride, cc.luma, cc.origin, cc.stride, i_pixel, subme, pos_xy, rpar,
            out[:, 0].copy(), cm, c0, fpel_satd=fpel_satd, counts=True, ext=oracle.refine_ext(chroma, cf, 0, weights),
            fenc_c=cc.fenc_c, fc_origin=cc.co, fcs=cc.cs, ref_c=cc.ref_c, rc_origin=cc.co, rcs=cc.cs)
    return out, ne, scan
