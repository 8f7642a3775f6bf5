"""Degenerate content for the motion-search tests (test_cpu_degenerate.py, test_gpu_degenerate.py):
the frames of a refine_cases.ChromaCase, a search_cases.MultiRef or a synth-layout sequence with
luma and chroma of the current and the reference frames replaced by content on which candidates
cost the same (the order equal costs resolve in decides the result) or differ by the whole sample
range (the largest SADs and packed cost codes the kernels can meet), the hpel planes recomputed
from the new planes.  The geometry stays the existing job lists' (search_cases.jobs,
refine_cases.jobs, bidir_cases.jobs, tesa_search_cases.degenerate_jobs).

Kinds: const (every sample 100 << (bd - 8)), nearflat (the texture's top three bits around a mid
level), periodic (a pattern of period p in x and y over the whole padded plane: SADs at mv and
mv +- p are equal, so distant candidates tie), extreme (fenc all (1 << bd) - 1, references all 0)
and extreme_swap (fenc all 0, references all max).  Used with refine_cases.cost_mv(lam) for
lambda 40 (only the ties symmetric about mvp stay), 1 and 0 (every SAD tie is a cost tie)."""
import numpy as np

import numpy_ref as nr
import refine_cases as rc
import search_cases as sc

PAD = 32
KINDS = ("const", "nearflat", "periodic", "extreme", "extreme_swap")
LAMBDAS = (40, 1, 0)


def period(i_pixel):
    """periodic's p: 8 for the 16x16 size, 4 below"""
    return 8 if i_pixel == 0 else 4


def _nearflat(a, bd):
    return ((a.astype(np.int64) >> (bd - 3)) + (100 << (bd - 8))).astype(a.dtype)


def fill(kind, src, bd, role, p=4, nv=False):
    """the replacement of the padded plane src [rows, stride] ((0, 0) at (PAD, PAD); nv: U / V
    interleaved, two elements per chroma pixel); role "fenc" or "ref" """
    h, w = src.shape
    if kind == "nearflat":
        return _nearflat(src, bd)
    if kind == "const":
        v = np.full((h, w), 100 << (bd - 8))
    elif kind == "periodic":
        yy = np.arange(h)[:, None] - PAD
        xx = (np.arange(w)[None, :] - PAD) >> (1 if nv else 0)
        v = (((xx % p) * 37 + (yy % p) * 53) % 200 + 20) << (bd - 8)
    elif kind in ("extreme", "extreme_swap"):
        v = np.full((h, w), ((1 << bd) - 1) if (role == "fenc") == (kind == "extreme") else 0)
    else:
        raise ValueError(kind)
    return v.astype(src.dtype)


def _frame(fr, kind, bd, role, p):
    fr.y = fill(kind, fr.y, bd, role, p)
    if fr.cf in (1, 2):
        fr.nv = fill(kind, fr.nv, bd, role, p, nv=True)
    elif fr.cf == 3:
        fr.u, fr.v = fill(kind, fr.u, bd, role, p), fill(kind, fr.v, bd, role, p)


def chroma_case(kind, bd, W, H, cf, seed, p=4, fade=False):
    """refine_cases.ChromaCase(bd, W, H, cf, seed, fade) with the kind's content in every plane"""
    cc = rc.ChromaCase(bd, W, H, cf, seed=seed, fade=fade)
    _frame(cc.ref, kind, bd, "ref", p)
    _frame(cc.fenc, kind, bd, "fenc", p)
    r, f = cc.ref, cc.fenc
    cc.luma = [r.y.ravel()] + [h.ravel() for h in nr.hpel_planes(r.y, PAD, W, H, bd)]
    cc.fenc_y = f.y.ravel()
    if cf in (1, 2):
        cc.fenc_c, cc.ref_c = [f.nv.ravel()], [r.nv.ravel()]
    else:
        cc.fenc_c, cc.ref_c = [f.u.ravel(), f.v.ravel()], []
        for pl in (r.u, r.v):
            cc.ref_c += [pl.ravel()] + [h.ravel() for h in nr.hpel_planes(pl, PAD, W, H, bd)]
    return cc


def flat_case(bd, W, H, cf, seed):
    """a ChromaCase whose luma is near flat (the texture's top three bits around a mid level): with
    a high-lambda mv cost the rows' ycost reaches bsad (the row skip) and survivor lists empty"""
    cc = rc.ChromaCase(bd, W, H, cf, seed=seed)
    for fr in (cc.ref, cc.fenc):
        fr.y = _nearflat(fr.y, bd)
    cc.luma = [cc.ref.y.ravel()] + [h.ravel() for h in nr.hpel_planes(cc.ref.y, PAD, W, H, bd)]
    cc.fenc_y = cc.fenc.y.ravel()
    return cc


def multi_ref(kind, bd, W, H, cf, seed, p=4):
    """search_cases.MultiRef(bd, W, H, cf, seed) with the kind's content: the current frame, and
    reference 0's planes in all three references (identical references: costs tie across them and
    the p_halfpel_thresh comparison of me.c:931-944 sits on its boundary)"""
    mr = sc.MultiRef(bd, W, H, cf, seed=seed)
    rows, crows = mr.fenc_y.size // mr.stride, mr.fenc_c[0].size // mr.cs
    mr.fenc_y = fill(kind, mr.fenc_y.reshape(rows, -1), bd, "fenc", p).ravel()
    mr.fenc_c = [fill(kind, c.reshape(crows, -1), bd, "fenc", p, nv=cf in (1, 2)).ravel() for c in mr.fenc_c]
    r = mr.refs[0]
    y = fill(kind, r.luma[0].reshape(rows, -1), bd, "ref", p)
    r.luma = [y.ravel()] + [h.ravel() for h in nr.hpel_planes(y, PAD, W, H, bd)]
    if cf in (1, 2):
        r.ref_c = [fill(kind, r.ref_c[0].reshape(crows, -1), bd, "ref", p, nv=True).ravel()]
    else:
        out = []
        for k in (0, 4):
            c = fill(kind, r.ref_c[k].reshape(crows, -1), bd, "ref", p)
            out += [c.ravel()] + [h.ravel() for h in nr.hpel_planes(c, PAD, W, H, bd)]
        r.ref_c = out
    for o in mr.refs[1:]:
        o.luma, o.ref_c = r.luma, r.ref_c
    return mr


def planes(kind, nframes, W, H, bd, seed=1, p=4, refs=(0,)):
    """synth.make_sequence's layout (planes [nframes, H + 2 PAD, stride], stride, origin) with the
    kind's content: the frames `refs` in the reference's role, the others in fenc's"""
    import weightp_cases as wc
    pl, stride, origin = wc._synth().make_sequence(nframes, W, H, bd, seed=seed)
    for k in range(nframes):
        pl[k] = fill(kind, pl[k], bd, "ref" if k in refs else "fenc", p)
    return pl, stride, origin


# ---------------------------------------------------------------- the 96x64 lists of the GPU tests
GW, GH = 96, 64
# (bd, i_pixel): per frame (content seed, search_cases.jobs seed), chosen so that each frame's
# list clears test_cpu_degenerate.py's tie-rate floors (0.15: nearflat at lambda 0 and 1, const
# at lambda 40).  A 16x16 / 16x8 / 8x16 near-flat list averages 0.08-0.12, the smaller sizes
# 0.15-0.40: the large sizes' seeds are the ones whose lists tie most often.
SEARCH_SEEDS = {
    (8, 0): ((1, 2), (4, 3)), (8, 1): ((1, 9), (5, 0)), (8, 2): ((6, 8), (11, 7)), (8, 3): ((1, 3), (2, 7)),
    (8, 4): ((1, 0), (2, 1)), (8, 5): ((1, 0), (2, 1)), (8, 6): ((1, 0), (2, 1)),
    (10, 0): ((1, 2), (5, 2)), (10, 1): ((1, 6), (4, 2)), (10, 2): ((6, 8), (11, 5)), (10, 3): ((1, 3), (2, 2)),
    (10, 4): ((1, 0), (2, 1)), (10, 5): ((1, 0), (2, 1)), (10, 6): ((1, 0), (2, 1))}
# (bd, i_pixel): MultiRef content seed, MultiRef.jobs seed per reference
CHAIN_SEEDS = {(8, 0): (7, (32, 28, 2)), (8, 3): (2, (5, 0, 3)), (10, 0): (14, (36, 3, 40)), (10, 3): (1, (3, 4, 4))}


def search_cases(kind, bd, i_pixel, cf=1, nframes=2):
    """the frame pairs of one me_search_ref / me_search_ref_tesa launch"""
    return [chroma_case(kind, bd, GW, GH, cf, seed=cs, p=period(i_pixel))
            for cs, _ in SEARCH_SEEDS[bd, i_pixel][:nframes]]


def search_jobs(bd, i_pixel, nframes=2, collapsed=False):
    """their partitions: search_cases.jobs per frame (collapsed: tesa_search_cases.degenerate_jobs,
    x limits collapsed to one column on every third partition, y limits to one row on every
    fifth); the sub-8x8 sizes on corner_rows' partitions"""
    import tesa_search_cases as ts
    out = []
    for f, (_, js) in enumerate(SEARCH_SEEDS[bd, i_pixel][:nframes]):
        j = ts.degenerate_jobs(GW // 16, GH // 16, i_pixel, js) if collapsed else \
            sc.jobs(GW // 16, GH // 16, 1, i_pixel, seed=js)
        if i_pixel >= 4:
            j = ts.corner_rows(*j, GW // 16, GH // 16)
        j[0][:, 0] = f
        out.append(j)
    return tuple(np.concatenate([j[k] for j in out]) for k in range(3))


def chain_inputs(kind, bd, i_pixel):
    """the threshold chain's MultiRef and its three job lists"""
    cs, js = CHAIN_SEEDS[bd, i_pixel]
    mr = multi_ref(kind, bd, GW, GH, 1, seed=cs)
    return mr, [mr.jobs(k, i_pixel, seed=js[k]) for k in range(3)]


# ---------------------------------------------------------------- what the inputs reach (numpy_ref and par alone)
def first_diamond_tie_rate(fenc, fw, origin, stride, pos_xy, par, i_pixel, cm, c0):
    """the share of the partitions whose five costs (SAD + mv cost) of the first radius-1 diamond
    at the rounded, clipped predictor attain their minimum more than once"""
    bw, bh = nr.SIZES[i_pixel]
    ties = 0
    for (x, y), q in zip(pos_xy, par):
        x, y = int(x), int(y)
        mvp = (int(q[0]), int(q[1]))
        pmx = min(max((mvp[0] + 2) >> 2, int(q[2])), int(q[4]))
        pmy = min(max((mvp[1] + 2) >> 2, int(q[3])), int(q[5]))
        fb = nr.block(fenc, origin + y * stride + x, stride, bw, bh)
        cs = []
        for dx, dy in ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0)):
            mx, my = pmx + dx, pmy + dy
            cs.append(nr.sad(fb, nr.block(fw, origin + (y + my) * stride + x + mx, stride, bw, bh)) +
                      int(cm[c0 + 4 * mx - mvp[0]]) + int(cm[c0 + 4 * my - mvp[1]]))
        ties += cs.count(min(cs)) > 1
    return ties / len(par)


def reach_inside(pos_xy, par_fpel, par_spel, i_pixel, W, H, stride, rows):
    """from the limits alone: every block any schedule can read lies inside the padded plane.
    par_fpel [n, 4] = mv_limit_fpel (min x, y, max x, y) or None; par_spel [n, 4] = mv_min_spel /
    mv_max_spel.  The furthest reach that is not range-checked: DIA1 one pixel past the limit,
    the hexagon two and its square refine one more (3), plus the 6-tap hpel margin (3); the qpel
    refine stops on the spel limits, its get_ref reads one sample further.  Returns the number of
    partitions outside"""
    bw, bh = nr.SIZES[i_pixel]
    assert stride >= W + 2 * PAD and rows == H + 2 * PAD
    x, y = pos_xy[:, 0].astype(np.int64), pos_xy[:, 1].astype(np.int64)
    bad = np.zeros(len(x), bool)
    if par_fpel is not None:
        f = par_fpel.astype(np.int64)
        r = 3 + 3
        bad |= (x + f[:, 0] - r < -PAD) | (y + f[:, 1] - r < -PAD)
        bad |= (x + f[:, 2] + r + bw > W + PAD) | (y + f[:, 3] + r + bh > H + PAD)
    s = par_spel.astype(np.int64)
    bad |= (x + (s[:, 0] >> 2) - 1 < -PAD) | (y + (s[:, 1] >> 2) - 1 < -PAD)
    bad |= (x + (s[:, 2] >> 2) + 2 + bw > W + PAD) | (y + (s[:, 3] >> 2) + 2 + bh > H + PAD)
    return int(bad.sum())
