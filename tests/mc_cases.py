"""x264_mb_mc restated in numpy, from the reference's C (common/mc.c:49-283 pixel_avg,
pixel_avg_weight_wxh, mc_weight, mc_luma, get_ref, mc_chroma; common/macroblock.c:31-153
mb_mc_0xywh / 1xywh / 01xywh), and the inputs of tests/test_cpu_mc.py and tests/test_gpu_mbmc.py.

Planes are numpy arrays [frames, rows, stride] with pixel (0,0) of a frame at (oy, ox); every
routine works on a list of n blocks at once (fancy indexing over [n, h, w] index arrays), the
one-block forms the CPU tests compare with the oracle are the same code with n = 1."""
import numpy as np

import numpy_ref as nr
import weightp_cases as wc

PAD = 32
PIXEL_SIZES = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
HPEL_REF0 = np.array([0, 1, 1, 1, 0, 1, 1, 1, 2, 3, 3, 3, 0, 1, 1, 1])      # common/tables.c:183
HPEL_REF1 = np.array([0, 0, 1, 0, 2, 2, 3, 2, 2, 2, 3, 2, 2, 2, 3, 2])      # common/tables.c:184


def pixel_max(bd):
    return (1 << bd) - 1


def _i(a):
    return np.atleast_1d(np.asarray(a, np.int64))


# ------------------------------------------------------------------ mc.c
def get_ref(planes, oy, ox, f, x, y, mvx, mvy, w, h):
    """get_ref with x264_weight_none (mc.c:221-249) of n blocks: planes = [F, H, V, C] arrays
    [frames, rows, stride]; f, x, y, mvx, mvy: [n] (block position in pixels, mv in quarter pixels).
    Returns int64 [n, h, w]."""
    f, x, y, mvx, mvy = _i(f), _i(x), _i(y), _i(mvx), _i(mvy)
    P = np.stack(planes)
    idx = ((mvy & 3) << 2) + (mvx & 3)
    Y = (oy + y + (mvy >> 2))[:, None, None] + np.arange(h)[None, :, None]
    X = (ox + x + (mvx >> 2))[:, None, None] + np.arange(w)[None, None, :]
    F = f[:, None, None]
    src1 = P[HPEL_REF0[idx][:, None, None], F, Y + ((mvy & 3) == 3)[:, None, None], X].astype(np.int64)
    src2 = P[HPEL_REF1[idx][:, None, None], F, Y, X + ((mvx & 3) == 3)[:, None, None]].astype(np.int64)
    return np.where(((idx & 5) != 0)[:, None, None], (src1 + src2 + 1) >> 1, src1)


def mc_weight(block, weight, bd, raw=False):
    """mc_weight (mc.c:117-137): weight = (scale, denom, offset); raw: before x264_clip_pixel"""
    scale, denom, offset = weight
    off = offset * (1 << (bd - 8))
    b = np.asarray(block, np.int64)
    v = ((b * scale + (1 << (denom - 1))) >> denom) + off if denom >= 1 else b * scale + off
    return v if raw else np.clip(v, 0, pixel_max(bd))


def mc_luma(planes, oy, ox, f, x, y, mvx, mvy, w, h, weight, bd):
    """mc_luma (mc.c:198-219): the qpel average first, then the weight (None = weightfn NULL)"""
    b = get_ref(planes, oy, ox, f, x, y, mvx, mvy, w, h)
    return b if weight is None else mc_weight(b, weight, bd)


def mc_chroma(nv, oy, ox, f, col, row, mvx, mvy, w, h):
    """mc_chroma (mc.c:252-283) of n blocks of w x h chroma pixels of the interleaved plane nv
    [frames, rows, stride]: the block's first U sample at interleaved column col, row `row`; mvx, mvy
    in eighth chroma pixels.  Returns (u, v) int64 [n, h, w]."""
    f, col, row, mvx, mvy = _i(f), _i(col), _i(row), _i(mvx), _i(mvy)
    d8x, d8y = (mvx & 7)[:, None, None], (mvy & 7)[:, None, None]
    cA, cB, cC, cD = (8 - d8x) * (8 - d8y), d8x * (8 - d8y), (8 - d8x) * d8y, d8x * d8y
    Y = (oy + row + (mvy >> 3))[:, None, None] + np.arange(h + 1)[None, :, None]
    X = (ox + col + (mvx >> 3) * 2)[:, None, None] + 2 * np.arange(w + 1)[None, None, :]
    out = []
    for p in range(2):
        s = nv[f[:, None, None], Y, X + p].astype(np.int64)
        out.append((cA * s[:, :-1, :-1] + cB * s[:, :-1, 1:] + cC * s[:, 1:, :-1] + cD * s[:, 1:, 1:] + 32) >> 6)
    return out[0], out[1]


def avg(a, b, i_weight, bd, raw=False):
    """mc.avg[i_mode] (PIXEL_AVG_C, mc.c:90-99): weight 32 = pixel_avg_wxh, else
    pixel_avg_weight_wxh with its clip.  i_weight: scalar or [n]."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    w1 = np.asarray(i_weight, np.int64).reshape(-1, *([1] * (a.ndim - 1))) if np.ndim(i_weight) else np.int64(i_weight)
    wv = (a * w1 + b * (64 - w1) + (1 << 5)) >> 6
    if raw:
        return wv
    return np.where(w1 == 32, (a + b + 1) >> 1, np.clip(wv, 0, pixel_max(bd)))


# ------------------------------------------------------------------ reference pictures
class Ref:
    """the planes of one reference list for frames 0..n-1, from weightp_cases.Frame objects: luma F,
    H, V, C [n, rows, stride] ((0,0) at (32, 32)); chroma = [NV12 / NV16 plane] ((0,0) at row 32,
    interleaved column 32) or U's F, H, V, C then V's (4:4:4)"""

    def __init__(self, frames):
        f0 = frames[0]
        self.bd, self.W, self.H, self.cf = f0.bd, f0.W, f0.H, f0.cf

        def four(name):
            per = [[getattr(fr, name)] + nr.hpel_planes(getattr(fr, name), PAD, self.W, self.H, self.bd) for fr in frames]
            return [np.stack([p[k] for p in per]) for k in range(4)]
        self.luma = four("y")
        self.stride, self.oy, self.ox = f0.ys, PAD, PAD
        self.cs, self.coy, self.cox = f0.cs, PAD, PAD
        if self.cf in (1, 2):
            self.chroma = [np.stack([fr.nv for fr in frames])]
        elif self.cf == 3:
            self.chroma = four("u") + four("v")
        else:
            self.chroma = []

    @property
    def origin(self):
        return self.oy * self.stride + self.ox

    @property
    def corigin(self):
        return self.coy * self.cs + self.cox


def make_ref(bd, W, H, cf, nframes, seed, level="mid"):
    """nframes pictures: "mid" = weightp_cases' smooth textures; "full" = uniform over the whole
    range; "bright" / "dark" = uniform over the top / bottom fifth (so weights and the bipred
    weights clip)"""
    rng = np.random.default_rng(seed)
    pm = pixel_max(bd)
    hs, vs = (1, 1) if cf == 1 else (1, 0) if cf == 2 else (0, 0)
    frames = []
    for k in range(nframes):
        if level == "mid":
            frames.append(wc.make_pair(bd, W, H, cf, seed=seed + 31 * k)[k & 1])
            continue
        lo, hi = {"full": (0, pm), "bright": (pm - pm // 5, pm), "dark": (0, pm // 5)}[level]
        y = rng.integers(lo, hi + 1, (H, W))
        c = [rng.integers(lo, hi + 1, (H >> vs, W >> hs)) for _ in range(2)] if cf else []
        frames.append(wc.Frame(bd, W, H, cf, y, c))
    return Ref(frames)


def mv_limits(x, y, mbw, mbh):
    """h->mb.mv_min / mv_max of the MB holding pixel (x, y) (analyse.c:330-349, progressive, one
    thread): 24 pixels past the frame, in quarter pixels"""
    mbx, mby = np.asarray(x) // 16, np.asarray(y) // 16
    return (4 * (-16 * mbx - 24), 4 * (-16 * mby - 24), 4 * (16 * (mbw - mbx - 1) + 24), 4 * (16 * (mbh - mby - 1) + 24))


def block_positions(W, H, nframes, i_pixel, checker=False):
    """pos [n, 3] of every i_pixel block of every frame in raster order (checker: every other block,
    a checkerboard)"""
    bw, bh = PIXEL_SIZES[i_pixel]
    pos = [(f, x, y) for f in range(nframes) for y in range(0, H, bh) for x in range(0, W, bw)
           if not checker or ((x // bw + y // bh) & 1) == 0]
    return np.array(pos, np.int32)


def make_par(pos, mv0, mv1, W, H):
    """par [n, 8] = (mv0, mv1, mv_min, mv_max) with analyse.c's limits of each block's MB"""
    mn_x, mn_y, mx_x, mx_y = mv_limits(pos[:, 1], pos[:, 2], W // 16, H // 16)
    return np.stack([mv0[:, 0], mv0[:, 1], mv1[:, 0], mv1[:, 1], mn_x, mn_y, mx_x, mx_y], 1).astype(np.int16)


def phase_mvs(pos, W, H, seed, base=0):
    """one mv per block, inside mv_min / mv_max: block i takes the eighth-pel phase (mvx & 7,
    mvy & 7) number (base + i) % 64 -- so 64 consecutive blocks (over several calls: base) meet all
    64 chroma phases and, four times over, all 16 luma phases -- and a random integer part over the
    whole legal range, negative vectors and vectors up to 24 pixels into the padding included"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    mn_x, mn_y, mx_x, mx_y = mv_limits(pos[:, 1], pos[:, 2], W // 16, H // 16)
    k = (base + np.arange(n)) % 64
    ix = rng.integers(mn_x >> 3, ((mx_x - 7) >> 3) + 1, n)
    iy = rng.integers(mn_y >> 3, ((mx_y - 7) >> 3) + 1, n)
    return np.stack([8 * ix + (k & 7), 8 * iy + (k >> 3)], 1).astype(np.int64)


def edge_mvs(pos, W, H, seed):
    """one mv per block at or beyond the limits: a third on mv_min / mv_max themselves (the deepest
    legal reads), the rest 25 .. 110 pixels outside, which the clip must bring back"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    mn_x, mn_y, mx_x, mx_y = mv_limits(pos[:, 1], pos[:, 2], W // 16, H // 16)
    hi = rng.random((n, 2)) < 0.5
    mv = np.stack([np.where(hi[:, 0], mx_x, mn_x), np.where(hi[:, 1], mx_y, mn_y)], 1).astype(np.int64)
    out = rng.random(n) >= 1 / 3
    mv[out] += np.where(hi[out], 1, -1) * rng.integers(100, 440, (int(out.sum()), 2))
    one = out & (rng.random(n) < 0.5)                       # only one component outside
    mv[one, 1] = phase_mvs(pos, W, H, seed + 1)[one, 1]
    return mv


# ------------------------------------------------------------------ x264_mb_mc of a block list
def mb_mc(bd, cf, i_pixel, ref0, ref1, pos, par, mode, weights, pred, p_oy, p_ox, pred_c=(), c_oy=0, c_ox=0,
          stats=None):
    """x264_mb_mc of the blocks pos / par / mode (include/x264hip_mc.h's layout) into pred [frames,
    rows, stride] ((0,0) at (p_oy, p_ox)) and pred_c ([UV plane] or [U, V]; (0,0) at (c_oy, c_ox), the
    interleaved column for 4:2:0 / 4:2:2), in place.  ref0 / ref1: Ref (ref1 None when unused);
    weights = 3 x ((scale, denom, offset) or None).  stats (a dict) receives: luma_phases /
    chroma_phases (sets), clipped (blocks whose used mv the clip changed), over / under (any
    weighted or bipred value beyond the pixel range before its clip)."""
    bw, bh = PIXEL_SIZES[i_pixel]
    pos, par = np.asarray(pos, np.int64), np.asarray(par, np.int64)
    n = len(pos)
    lists = np.ones(n, np.int64) if mode is None else np.asarray(mode, np.int64) & 3
    biw = np.full(n, 32, np.int64) if mode is None else np.asarray(mode, np.int64) >> 8
    st = stats if stats is not None else {}
    st.setdefault("luma_phases", set()); st.setdefault("chroma_phases", set())
    st.setdefault("clipped", 0); st.setdefault("over", False); st.setdefault("under", False)
    pm = pixel_max(bd)

    def note(v):
        st["over"] |= bool((v > pm).any())
        st["under"] |= bool((v < 0).any())

    f, x, y = pos[:, 0], pos[:, 1], pos[:, 2]
    mv = []
    for l in range(2):
        mvx = np.clip(par[:, 2 * l], par[:, 4], par[:, 6])          # x264_clip3 (macroblock.c:41-42)
        mvy = np.clip(par[:, 2 * l + 1], par[:, 5], par[:, 7])
        used = (lists & (1 << l)) != 0
        st["clipped"] += int(((mvx != par[:, 2 * l]) | (mvy != par[:, 2 * l + 1]))[used].sum())
        mv.append((mvx, mvy))
    refs = (ref0, ref1)
    vs = 1 if cf == 1 else 0

    def scatter(dst, oy, ox, fr, row, col, blk, step=1):
        h, w = blk.shape[1:]
        Y = (oy + row)[:, None, None] + np.arange(h)[None, :, None]
        X = (ox + col)[:, None, None] + step * np.arange(w)[None, None, :]
        dst[fr[:, None, None], Y, X] = blk.astype(dst.dtype)

    for kind in (1, 2, 3):
        sel = np.flatnonzero(lists == kind)
        if not len(sel):
            continue
        fs, xs, ys = f[sel], x[sel], y[sel]
        used = [l for l in range(2) if kind & (1 << l)]
        for l in used:
            st["luma_phases"] |= set((((mv[l][1][sel] & 3) << 2) + (mv[l][0][sel] & 3)).tolist())

        def plane_pred(name, k0, wt):
            """MC_LUMA / MC_LUMA_BI of one plane (luma, or U / V at 4:4:4)"""
            def gr(l):
                r = refs[l]
                planes, oy, ox = (r.luma, r.oy, r.ox) if name == "y" else (r.chroma[k0:k0 + 4], r.coy, r.cox)
                return get_ref(planes, oy, ox, fs, xs, ys, mv[l][0][sel], mv[l][1][sel], bw, bh)
            if kind == 3:
                a, b = gr(0), gr(1)
                note(avg(a, b, biw[sel], bd, raw=True)[biw[sel] != 32])
                return avg(a, b, biw[sel], bd)
            b = gr(used[0])
            if kind == 1 and wt is not None:                  # list ? x264_weight_none : &h->sh.weight
                note(mc_weight(b, wt, bd, raw=True))
                return mc_weight(b, wt, bd)
            return b

        scatter(pred, p_oy, p_ox, fs, ys, xs, plane_pred("y", 0, weights[0]))
        if cf == 3:
            scatter(pred_c[0], c_oy, c_ox, fs, ys, xs, plane_pred("u", 0, weights[1]))
            scatter(pred_c[1], c_oy, c_ox, fs, ys, xs, plane_pred("v", 4, weights[2]))
        elif cf:
            cw, ch = bw // 2, bh >> vs

            def mcc(l):
                r = refs[l]
                cmvy = (2 * mv[l][1][sel]) >> vs              # macroblock.c:64
                st["chroma_phases"] |= set((((cmvy & 7) << 3) + (mv[l][0][sel] & 7)).tolist())
                return mc_chroma(r.chroma[0], r.coy, r.cox, fs, xs, ys >> vs, mv[l][0][sel], cmvy, cw, ch)
            if kind == 3:
                (u0, v0), (u1, v1) = mcc(0), mcc(1)
                for a, b in ((u0, u1), (v0, v1)):
                    note(avg(a, b, biw[sel], bd, raw=True)[biw[sel] != 32])
                uv = [avg(u0, u1, biw[sel], bd), avg(v0, v1, biw[sel], bd)]
            else:
                uv = list(mcc(used[0]))
                if kind == 1:
                    for p in range(2):
                        if weights[1 + p] is not None:
                            note(mc_weight(uv[p], weights[1 + p], bd, raw=True))
                            uv[p] = mc_weight(uv[p], weights[1 + p], bd)
            for p in range(2):
                scatter(pred_c[0], c_oy, c_ox + p, fs, ys >> vs, xs, uv[p], step=2)
    return st


def pred_planes(ref, sentinel=None, rows_extra=0, stride_extra=0, frames=None):
    """prediction planes shaped like ref's (optionally with more rows / a longer stride, so every
    stride and frame stride differs from the reference's), filled with `sentinel` (default 0):
    (pred, pred_c list)"""
    nf = frames if frames is not None else ref.luma[0].shape[0]
    dt = ref.luma[0].dtype
    fill = 0 if sentinel is None else sentinel
    rows, stride = ref.luma[0].shape[1:]
    pred = np.full((nf, rows + rows_extra, stride + stride_extra), fill, dt)
    pred_c = []
    if ref.cf:
        crows, cs = ref.chroma[0].shape[1:]
        for _ in range(2 if ref.cf == 3 else 1):
            pred_c.append(np.full((nf, crows + 2 * rows_extra, cs + 2 * stride_extra), fill, dt))
    return pred, pred_c
