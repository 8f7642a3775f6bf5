"""TEST INFRASTRUCTURE: numpy restatement of x264's MB-tree, the checker of the MB-tree entries
(include/x264hip_mbtree.h) and of mbtree_plan.

Restated from the reference's text: mbtree_propagate_cost / mbtree_propagate_list (common/mc.c:509-598),
macroblock_tree_finish / _propagate / macroblock_tree (encoder/slicetype.c:1026-1184, the
i_lookahead > 0 branch) and x264_log2 (common/base.h:226-230, tables common/tables.c:66-90).

Every float is an np.float32 scalar or array, so each operation rounds once to single precision in
the source's order: what the reference's C build computes (tests/test_cpu_mbtree.py compares this
file with a C build of the same expression under the reference's compiler flags).
"""
import json
import math
import os

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
LOWRES_COST_MASK, LOWRES_COST_SHIFT = (1 << 14) - 1, 14
MBTREE_PRECISION = F(0.5)

HERE = os.path.dirname(os.path.abspath(__file__))

# x264_log2_lut / x264_log2_lz_lut (decimals -> double -> float, as a C initialiser converts them)
LOG2_LUT = np.array([
    0.00000, 0.01123, 0.02237, 0.03342, 0.04439, 0.05528, 0.06609, 0.07682,
    0.08746, 0.09803, 0.10852, 0.11894, 0.12928, 0.13955, 0.14975, 0.15987,
    0.16993, 0.17991, 0.18982, 0.19967, 0.20945, 0.21917, 0.22882, 0.23840,
    0.24793, 0.25739, 0.26679, 0.27612, 0.28540, 0.29462, 0.30378, 0.31288,
    0.32193, 0.33092, 0.33985, 0.34873, 0.35755, 0.36632, 0.37504, 0.38370,
    0.39232, 0.40088, 0.40939, 0.41785, 0.42626, 0.43463, 0.44294, 0.45121,
    0.45943, 0.46761, 0.47573, 0.48382, 0.49185, 0.49985, 0.50779, 0.51570,
    0.52356, 0.53138, 0.53916, 0.54689, 0.55459, 0.56224, 0.56986, 0.57743,
    0.58496, 0.59246, 0.59991, 0.60733, 0.61471, 0.62205, 0.62936, 0.63662,
    0.64386, 0.65105, 0.65821, 0.66534, 0.67243, 0.67948, 0.68650, 0.69349,
    0.70044, 0.70736, 0.71425, 0.72110, 0.72792, 0.73471, 0.74147, 0.74819,
    0.75489, 0.76155, 0.76818, 0.77479, 0.78136, 0.78790, 0.79442, 0.80090,
    0.80735, 0.81378, 0.82018, 0.82655, 0.83289, 0.83920, 0.84549, 0.85175,
    0.85798, 0.86419, 0.87036, 0.87652, 0.88264, 0.88874, 0.89482, 0.90087,
    0.90689, 0.91289, 0.91886, 0.92481, 0.93074, 0.93664, 0.94251, 0.94837,
    0.95420, 0.96000, 0.96578, 0.97154, 0.97728, 0.98299, 0.98868, 0.99435,
], np.float64).astype(F)
LOG2_LZ_LUT = np.arange(31, -1, -1).astype(F)


def fixture_tables():
    """(lut float32 [128], lz_lut float32 [32]) of tests/golden/mbtree_tables.json"""
    with open(os.path.join(HERE, "golden", "mbtree_tables.json")) as fh:
        t = json.load(fh)
    return tuple(np.array([float(v) for v in t[k]], np.float64).astype(F)
                 for k in ("x264_log2_lut", "x264_log2_lz_lut"))


# ------------------------------------------------------------------ table entries (mc.c)
def propagate_cost(propagate_in, intra_costs, inter_costs, inv_qscales, fps_factor):
    """mbtree_propagate_cost (mc.c:511-525) of a run of MBs: int64 amounts.  intra cost 0 (outside
    the reference's domain: 0 / 0) gives 0, the product's one addition."""
    fps = F(fps_factor)
    intra = np.asarray(intra_costs).astype(np.int64)
    inter = np.minimum(intra, np.asarray(inter_costs).astype(np.int64) & LOWRES_COST_MASK)
    propagate_intra = (intra * np.asarray(inv_qscales).astype(np.int64)).astype(F)
    propagate_amount = np.asarray(propagate_in).astype(F) + propagate_intra * fps
    propagate_num = (intra - inter).astype(F)
    propagate_denom = np.where(intra == 0, 1, intra).astype(F)
    q = propagate_amount * propagate_num / propagate_denom
    assert q.dtype == F
    out = np.minimum((q + F(0.5)).astype(np.int64), 32767)
    return np.where(intra == 0, 0, out)


def clip_add_to(ref_costs):
    """MC_CLIP_ADD into `ref_costs` (a flat uint16 plane) as the `add` of propagate_list"""
    def add(idx, v):
        ref_costs[idx] = min(int(ref_costs[idx]) + v, 32767)
    return add


def propagate_list(add, mvs, propagate_amount, lowres_costs, bipred_weight, mb_y, width, height, lst):
    """mbtree_propagate_list (mc.c:527-598) of row mb_y, literally, unsigned arithmetic included;
    every MC_CLIP_ADD( ref_costs[idx], v ) is add( idx, v ), in the reference's order."""
    stride = width
    for i in range(width):
        lists_used = int(lowres_costs[i]) >> LOWRES_COST_SHIFT
        if not lists_used & (1 << lst):
            continue
        listamount = int(propagate_amount[i])
        if lists_used == 3:
            listamount = (listamount * bipred_weight + 32) >> 6
        x, y = int(mvs[i][0]), int(mvs[i][1])
        if x == 0 and y == 0:
            add(mb_y * stride + i, listamount)
            continue
        mbx = ((x >> 5) + i) & M32
        mby = ((y >> 5) + mb_y) & M32
        idx0 = (mbx + mby * stride) & M32
        idx2 = (idx0 + stride) & M32
        x &= 31
        y &= 31
        w0 = ((32 - y) * (32 - x) * listamount + 512) >> 10
        w1 = ((32 - y) * x * listamount + 512) >> 10
        w2 = (y * (32 - x) * listamount + 512) >> 10
        w3 = (y * x * listamount + 512) >> 10
        if mbx < ((width - 1) & M32) and mby < ((height - 1) & M32):
            add(idx0, w0)
            add((idx0 + 1) & M32, w1)
            add(idx2, w2)
            add((idx2 + 1) & M32, w3)
        else:
            if mby < height:
                if mbx < width:
                    add(idx0, w0)
                if (mbx + 1) & M32 < width:
                    add((idx0 + 1) & M32, w1)
            if (mby + 1) & M32 < height:
                if mbx < width:
                    add(idx2, w2)
                if (mbx + 1) & M32 < width:
                    add((idx2 + 1) & M32, w3)


class Step:
    """one macroblock_tree_propagate step over host arrays (the fields of x264hip_mbtree_step_t);
    ref_costs are flat uint16 planes, changed in place"""

    def __init__(self, intra_cost, lowres_costs, mvs, ref_costs, fps_factor, inv_qscale=None, propagate_in=None,
                 bipred_weight=32):
        self.intra_cost, self.lowres_costs, self.mvs, self.ref_costs = intra_cost, lowres_costs, mvs, ref_costs
        self.fps_factor, self.inv_qscale, self.propagate_in = F(fps_factor), inv_qscale, propagate_in
        self.bipred_weight = bipred_weight


def step_adds(step, width, height):
    """the MC_CLIP_ADDs of one step in the reference's order (the row loop of slicetype.c:1069-1085):
    [(list, idx, v)]"""
    n = width * height
    invq = step.inv_qscale if step.inv_qscale is not None else np.full(n, 256, np.uint16)
    pin = step.propagate_in if step.propagate_in is not None else np.zeros(n, np.uint16)
    weights = (step.bipred_weight, 64 - step.bipred_weight)
    out = []
    for mb_y in range(height):
        r = slice(mb_y * width, (mb_y + 1) * width)
        buf = propagate_cost(pin[r], step.intra_cost[r], step.lowres_costs[r], invq[r], step.fps_factor)
        for lst in (0, 1):
            if step.mvs[lst] is None:
                continue
            propagate_list(lambda idx, v: out.append((lst, idx, v)), step.mvs[lst][r], buf, step.lowres_costs[r],
                           weights[lst], mb_y, width, height, lst)
    return out


def propagate_sequential(step, width, height):
    """one step, every MC_CLIP_ADD applied as it comes (the reference's own order)"""
    for lst, idx, v in step_adds(step, width, height):
        clip_add_to(step.ref_costs[lst])(idx, v)


def propagate_batched(steps, width, height):
    """the steps of one x264hip_mbtree_propagate call: the adds of all steps summed per
    destination element, the clip applied once"""
    n = width * height
    acc = {}
    for s in steps:
        for lst, idx, v in step_adds(s, width, height):
            plane = s.ref_costs[lst]
            key = plane.__array_interface__["data"][0]
            if key not in acc:
                acc[key] = (plane, np.zeros(n, np.int64))
            acc[key][1][idx] += v
    for plane, a in acc.values():
        plane[:] = np.minimum(plane.astype(np.int64) + a, 32767).astype(np.uint16)


# ------------------------------------------------------------------ finish (slicetype.c:1029-1049)
def x264_log2(x, lut=LOG2_LUT, lz_lut=LOG2_LZ_LUT):
    """x264_log2 of an array of uint32 values >= 1"""
    x = np.asarray(x).astype(np.uint64)
    lz = (32 - np.frexp(x.astype(np.float64))[1]).astype(np.uint64)
    idx = (((x << lz) & np.uint64(M32)) >> np.uint64(24)) & np.uint64(0x7f)
    return lut[idx.astype(np.int64)] + lz_lut[lz.astype(np.int64)]


def finish(intra_cost, inv_qscale, propagate_cost_plane, qp_offset_aq, qp_offset, fps_factor, weightdelta, strength):
    """the MB loop of macroblock_tree_finish: writes qp_offset (float32 [n]) where the scaled
    intra cost is non-zero"""
    n = len(intra_cost)
    invq = inv_qscale if inv_qscale is not None else np.full(n, 256, np.uint16)
    ic = (intra_cost.astype(np.int64) * invq.astype(np.int64) + 128) >> 8
    pc = (propagate_cost_plane.astype(np.int64) * int(fps_factor) + 128) >> 8
    on = ic != 0
    safe = np.where(on, ic, 1)
    log2_ratio = x264_log2(safe + pc) - x264_log2(safe) + F(weightdelta)
    res = qp_offset_aq.astype(F) - F(strength) * log2_ratio
    assert res.dtype == F
    qp_offset[on] = res[on]


# ------------------------------------------------------------------ macroblock_tree
class Frame:
    """the fields of x264_frame_t MB-tree touches.  lowres_costs[(b - p0, p1 - b)] and
    lowres_mvs[(list, distance - 1)] appear when slicetype_frame_cost( p0, p1, b ) has run."""

    def __init__(self, i_type, n, duration=0.04, inv_qscale=None, rng=None):
        self.i_type = i_type
        self.f_duration = F(duration)
        # (kept from the frame's first analysis in x264; a later slicetype_frame_cost leaves it)
        self.i_intra_cost = rng.integers(1, 0x4000, n).astype(np.uint16) if rng is not None else None
        self.i_inv_qscale_factor = inv_qscale if inv_qscale is not None else np.full(n, 256, np.uint16)
        # stale contents: macroblock_tree has to zero what it accumulates into
        self.i_propagate_cost = (rng.integers(0, 32768, n).astype(np.uint16) if rng is not None
                                 else np.zeros(n, np.uint16))
        self.lowres_costs, self.lowres_mvs = {}, {}
        self.f_qp_offset_aq = (rng.uniform(-2, 2, n).astype(F) if rng is not None else np.zeros(n, F))
        self.f_qp_offset = np.full(n, F(99.0))
        self.f_weighted_cost_delta = {}


class Params:
    def __init__(self, width, height, bframe_pyramid=False, vbv=False, weighted_bipred=True, qcompress=0.6):
        self.width, self.height = width, height
        self.bframe_pyramid, self.vbv, self.weighted_bipred = bframe_pyramid, vbv, weighted_bipred
        self.strength = F(5.0) * (F(1.0) - F(qcompress))


def clip_duration(f):
    return min(max(F(f), F(0.01)), F(1.0))


def average_duration(frames):
    """slicetype.c:1098-1101"""
    total = F(0.0)
    for f in frames:
        total = total + f.f_duration
    return total / F(len(frames))


def propagate_fps_factor(frame, avg):
    """slicetype.c:1063"""
    return clip_duration(frame.f_duration) / (clip_duration(avg) * F(256.0)) * MBTREE_PRECISION


def finish_params(frame, avg, ref0_distance):
    """(fps_factor, weightdelta) of slicetype.c:1031-1034"""
    fps = int(math.floor(float(clip_duration(avg) / clip_duration(frame.f_duration) * F(256) / MBTREE_PRECISION) + 0.5))
    weightdelta = F(0.0)
    if ref0_distance and frame.f_weighted_cost_delta.get(ref0_distance - 1, 0) > 0:
        weightdelta = F(1.0 - float(frame.f_weighted_cost_delta[ref0_distance - 1]))
    return fps, weightdelta


def bipred_weight(par, p0, p1, b):
    """slicetype.c:1054-1055"""
    dist_scale_factor = (((b - p0) << 8) + ((p1 - p0) >> 1)) // (p1 - p0)
    return 64 - (dist_scale_factor >> 2) if par.weighted_bipred else 32


def make_step(par, frames, avg, p0, p1, b, referenced):
    """the Step of macroblock_tree_propagate( p0, p1, b, referenced ) (slicetype.c:1053-1063)"""
    fr = frames[b]
    mvs = [fr.lowres_mvs[(0, b - p0 - 1)] if b != p0 else None, fr.lowres_mvs[(1, p1 - b - 1)] if b != p1 else None]
    return Step(fr.i_intra_cost, fr.lowres_costs[(b - p0, p1 - b)], mvs,
                [frames[p0].i_propagate_cost, frames[p1].i_propagate_cost], propagate_fps_factor(fr, avg),
                fr.i_inv_qscale_factor, fr.i_propagate_cost if referenced else None, bipred_weight(par, p0, p1, b))


def tree_finish(par, frame, avg, ref0_distance):
    fps, wd = finish_params(frame, avg, ref0_distance)
    finish(frame.i_intra_cost, frame.i_inv_qscale_factor, frame.i_propagate_cost, frame.f_qp_offset_aq,
           frame.f_qp_offset, fps, wd, par.strength)


def tree_propagate(par, frames, avg, p0, p1, b, referenced):
    """macroblock_tree_propagate (slicetype.c:1051-1089)"""
    if not referenced:
        frames[b].i_propagate_cost[:par.width] = 0          # slicetype.c:1066-1067
    propagate_sequential(make_step(par, frames, avg, p0, p1, b, referenced), par.width, par.height)
    if par.vbv and referenced:
        tree_finish(par, frames[b], avg, b - p0 if b == p1 else 0)


def macroblock_tree(par, frames, frame_cost, b_intra):
    """macroblock_tree (slicetype.c:1091-1184, i_lookahead > 0), literally and unbatched.
    frame_cost( p0, p1, b ) is slicetype_frame_cost."""
    num_frames = len(frames) - 1
    idx = 0 if b_intra else 1
    bframes = 0
    avg = average_duration(frames)
    isb = [f.i_type == "B" for f in frames]
    i = num_frames
    if b_intra:
        frame_cost(0, 0, 0)
    while i > 0 and isb[i]:
        i -= 1
    last_nonb = i
    if last_nonb < idx:
        return
    frames[last_nonb].i_propagate_cost[:] = 0
    while True:
        cond = i > idx
        i -= 1
        if not cond:
            break
        cur_nonb = i
        while isb[cur_nonb] and cur_nonb > 0:
            cur_nonb -= 1
        if cur_nonb < idx:
            break
        frame_cost(cur_nonb, last_nonb, last_nonb)
        frames[cur_nonb].i_propagate_cost[:] = 0
        bframes = last_nonb - cur_nonb - 1
        if par.bframe_pyramid and bframes > 1:
            middle = (bframes + 1) // 2 + cur_nonb
            frame_cost(cur_nonb, last_nonb, middle)
            frames[middle].i_propagate_cost[:] = 0
            while i > cur_nonb:
                p0 = middle if i > middle else cur_nonb
                p1 = middle if i < middle else last_nonb
                if i != middle:
                    frame_cost(p0, p1, i)
                    tree_propagate(par, frames, avg, p0, p1, i, 0)
                i -= 1
            tree_propagate(par, frames, avg, cur_nonb, last_nonb, middle, 1)
        else:
            while i > cur_nonb:
                frame_cost(cur_nonb, last_nonb, i)
                tree_propagate(par, frames, avg, cur_nonb, last_nonb, i, 0)
                i -= 1
        tree_propagate(par, frames, avg, cur_nonb, last_nonb, last_nonb, 1)
        last_nonb = cur_nonb
    tree_finish(par, frames[last_nonb], avg, last_nonb)
    if par.bframe_pyramid and bframes > 1 and not par.vbv:
        tree_finish(par, frames[last_nonb + (bframes + 1) // 2], avg, 0)


class HostBackend:
    """runs mbtree_plan's operations with the restatement, a propagate operation as one batched
    call.  An unreferenced step leaves its own frame's plane unused; the reference clears that
    plane's first row on the way (slicetype.c:1066-1067), reproduced here so whole planes compare."""

    def __init__(self, par, frames, frame_cost):
        self.par, self.frames, self.frame_cost = par, frames, frame_cost
        self.avg = average_duration(frames)

    def zero(self, f):
        self.frames[f].i_propagate_cost[:] = 0

    def cost(self, p0, p1, b):
        self.frame_cost(p0, p1, b)

    def propagate(self, steps):
        for p0, p1, b, referenced in steps:
            if not referenced:
                self.frames[b].i_propagate_cost[:self.par.width] = 0
        propagate_batched([make_step(self.par, self.frames, self.avg, *s) for s in steps], self.par.width,
                          self.par.height)

    def finish(self, f, ref0_distance):
        tree_finish(self.par, self.frames[f], self.avg, ref0_distance)


def run_plan(ops, backend):
    for op, *args in ops:
        getattr(backend, op)(*args)


# ------------------------------------------------------------------ crafted inputs
def random_frame_costs(seed, frames, width, height):
    """a slicetype_frame_cost stand-in: fills i_intra_cost / lowres_costs / lowres_mvs /
    f_weighted_cost_delta of frame b with crafted values on first request.  Each array's values
    depend on the seed and on which array it is only, not on the order of the requests."""
    n = width * height

    def rng(*key):
        return np.random.default_rng([seed, *key])

    def frame_cost(p0, p1, b):
        fr = frames[b]
        if fr.i_intra_cost is None:
            fr.i_intra_cost = rng(1, b).integers(1, 0x4000, n).astype(np.uint16)
        if b == p0:
            return
        key = (b - p0, p1 - b)
        if key not in fr.lowres_costs:
            r = rng(2, b, *key)
            lists = r.integers(1, 4, n) if b != p1 else np.ones(n, np.int64)
            fr.lowres_costs[key] = ((lists << 14) + r.integers(0, 0x4000, n)).astype(np.uint16)
        for lst, d in ((0, b - p0 - 1), (1, p1 - b - 1)):
            if (lst == 0 or b != p1) and (lst, d) not in fr.lowres_mvs:
                fr.lowres_mvs[(lst, d)] = crafted_mvs(rng(3, b, lst, d), width, height)
        if b == p1 and b - p0 - 1 not in fr.f_weighted_cost_delta:
            fr.f_weighted_cost_delta[b - p0 - 1] = F(rng(4, b, p0).choice([0.0, 0.7, 0.93]))
    return frame_cost


def crafted_mvs(rng, width, height):
    """int16 [n, 2]: a third exactly zero, the rest wide enough to land on mbx in -2 .. width + 1
    and mby in -2 .. height + 1 from every MB, every fractional phase"""
    n = width * height
    mx = rng.integers(-(width + 2) * 32, (width + 2) * 32, n)
    my = rng.integers(-(height + 2) * 32, (height + 2) * 32, n)
    near = rng.random(n) < 0.4                                 # short vectors: interior hits on large grids
    mx = np.where(near, rng.integers(-70, 70, n), mx)
    my = np.where(near, rng.integers(-70, 70, n), my)
    zero = rng.random(n) < 1 / 3
    mv = np.stack([np.where(zero, 0, mx), np.where(zero, 0, my)], 1)
    return np.clip(mv, -32768, 32767).astype(np.int16)


def crafted_step(rng, width, height, ref_costs, invq_mode="mid", fps_factor=0.0013, weight=32, referenced=True,
                 list1=True):
    """One Step of crafted inputs: lists_used over all four values, inter above intra for a
    quarter of the MBs, inv_qscale None / 50..1050 / up to 0x7fff, mvs as crafted_mvs."""
    n = width * height
    intra = rng.integers(1, 0x8000, n)
    small = rng.random(n) < 0.5
    intra = np.where(small, rng.integers(1, 3000, n), intra).astype(np.uint16)
    inter = (intra * rng.random(n)).astype(np.int64)
    inter = np.where(rng.random(n) < 0.25, np.minimum(intra.astype(np.int64) + rng.integers(0, 500, n), 0x3fff), inter)
    inter = np.minimum(inter, 0x3fff)
    lists = rng.integers(0, 4, n)
    costs = ((lists << 14) + inter).astype(np.uint16)
    invq = {"none": None, "mid": rng.integers(50, 1051, n).astype(np.uint16),
            "max": np.where(rng.random(n) < 0.2, 0x7fff, rng.integers(1, 0x8000, n)).astype(np.uint16)}[invq_mode]
    pin = rng.integers(0, 32768, n).astype(np.uint16) if referenced else None
    mvs = [crafted_mvs(rng, width, height), crafted_mvs(rng, width, height) if list1 else None]
    return Step(intra, costs, mvs, ref_costs, fps_factor, invq, pin, weight)


def saturating_step(rng, width, height, ref_costs, target=None):
    """every MB aimed at one target MB (integer vectors), large amounts: with planes starting at
    30000..32767 every add clips"""
    n = width * height
    t = n // 2 if target is None else target
    ty, tx = divmod(t, width)
    yy, xx = np.divmod(np.arange(n), width)
    mv = np.stack([(tx - xx) * 32, (ty - yy) * 32], 1).astype(np.int16)
    intra = rng.integers(2000, 0x8000, n).astype(np.uint16)
    costs = ((rng.integers(1, 4, n) << 14) + rng.integers(0, 300, n)).astype(np.uint16)
    return Step(intra, costs, [mv, mv.copy()], ref_costs, 0.19, None, None, 21)
