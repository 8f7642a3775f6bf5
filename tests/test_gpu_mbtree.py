"""GPU parity of MB-tree (x264hip_mbtree_propagate / x264hip_mbtree_finish, include/x264hip_mbtree.h)
against the numpy restatement of the reference (tests/mbtree_cases.py), bit for bit: planes as
uint16, qp offsets as the uint32 views of their floats."""
import ctypes

import numpy as np
import pytest
import torch

import mbtree_cases as mt

pytestmark = pytest.mark.gpu

FPS = (1 / 512, 0.0013, 0.19)


def _dev(a):
    """a host uint16 / int16 / float32 array on the device (uint16 as int16 bits)"""
    if a is None:
        return None
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


class _Planes:
    """host destination planes and their device copies, one device tensor per distinct host plane"""

    def __init__(self):
        self.host, self.dev = [], []

    def dev_of(self, plane):
        for h, d in zip(self.host, self.dev):
            if h is plane:
                return d
        self.host.append(plane)
        self.dev.append(_dev(plane))
        return self.dev[-1]


def _gpu_step(hip, s, planes):
    return hip.mbtree_step(_dev(s.intra_cost), _dev(s.lowres_costs), _dev(s.mvs[0]), planes.dev_of(s.ref_costs[0]),
                           s.fps_factor, _dev(s.mvs[1]),
                           None if s.mvs[1] is None else planes.dev_of(s.ref_costs[1]),
                           _dev(s.inv_qscale), _dev(s.propagate_in), s.bipred_weight)


def _check(hip, steps, w, h, tag):
    """the steps as one device call == the steps one after another through the literal restatement"""
    planes = _Planes()
    gsteps = [_gpu_step(hip, s, planes) for s in steps]          # uploads the planes' initial state
    start = [p.copy() for p in planes.host]
    hip.mbtree_propagate(gsteps, w, h)
    torch.cuda.synchronize()
    for s in steps:
        mt.propagate_sequential(s, w, h)
    for k, (want, d, s0) in enumerate(zip(planes.host, planes.dev, start)):
        got = _u16(d)
        bad = np.flatnonzero(got != want)[:4]
        assert not len(bad), (*tag, "plane", k, bad, got[bad], want[bad], s0[bad])
    if w * h >= 20:                                               # (a handful of MBs may all miss)
        assert any(not np.array_equal(p, s0) for p, s0 in zip(planes.host, start)), (*tag, "nothing propagated")
    return planes


def _start_planes(rng, n, count=2, lo=0, hi=20000):
    return [rng.integers(lo, hi, n).astype(np.uint16) for _ in range(count)]


GRIDS = [(2, 2), (1, 5), (5, 1), (6, 4), (11, 9), (120, 68)]


@pytest.mark.parametrize("grid", GRIDS)
def test_propagate_single_step(hip, grid):
    """n = 1: inv_qscale NULL / 50..1050 / up to 0x7fff, the three fps factors, bipred weights 32
    and 21, propagate_in NULL and set, both lists, list 1 absent, both lists into one plane"""
    w, h = grid
    n = w * h
    rng = np.random.default_rng(100 + n)
    combos = [("none", FPS[0], 32, False, True, False), ("mid", FPS[1], 21, True, True, False),
              ("max", FPS[2], 32, True, True, True), ("mid", FPS[2], 21, False, False, False)]
    if n > 1000:
        combos = combos[1:3]
    for invq, fps, weight, referenced, list1, same in combos:
        a, b = _start_planes(rng, n)
        s = mt.crafted_step(rng, w, h, [a, a if same else b], invq, fps, weight, referenced, list1)
        planes = _check(hip, [s], w, h, (grid, invq, fps, weight, referenced, list1, same))
        if not list1:
            assert len(planes.host) == 1


@pytest.mark.parametrize("grid", GRIDS)
def test_propagate_three_steps_shared_destinations(hip, grid):
    """n = 3 sharing both destination planes (the B frames between two non-B frames), one of them
    reading a propagate_in plane that is no destination"""
    w, h = grid
    n = w * h
    rng = np.random.default_rng(200 + n)
    dst = _start_planes(rng, n)
    steps = [mt.crafted_step(rng, w, h, dst, ("none", "mid", "max")[k], FPS[k], (32, 21, 21)[k], referenced=k == 1)
             for k in range(3)]
    planes = _check(hip, steps, w, h, (grid,))
    assert len(planes.host) == 2


@pytest.mark.parametrize("n_steps", [1, 3])
def test_propagate_saturation(hip, n_steps):
    """planes starting at 30000..32767 and every MB of every step aimed at one element: the
    accumulators take many times 32767 and the merge clips once"""
    w, h = 11, 9
    n = w * h
    rng = np.random.default_rng(5)
    dst = _start_planes(rng, n, lo=30000, hi=32768)
    steps = [mt.saturating_step(rng, w, h, dst, target=40) for _ in range(n_steps)]
    adds = mt.step_adds(steps[0], w, h)
    assert sum(v for _, i, v in adds if i == 40) > 10 * 32767
    planes = _check(hip, steps, w, h, ("saturation", n_steps))
    assert planes.host[0][40] == 32767 and planes.host[1][40] == 32767


def test_propagate_zero_intra_cost(hip):
    """intra_cost == 0, where the reference divides 0 by 0: the entry propagates amount 0 (the one
    deliberate addition, x264hip_mbtree.h), and the other MBs are unaffected"""
    w, h = 6, 4
    rng = np.random.default_rng(12)
    dst = _start_planes(rng, w * h)
    s = mt.crafted_step(rng, w, h, dst, "mid", FPS[2], 21, referenced=True)
    s.intra_cost[::3] = 0
    assert all(v == 0 for v in mt.propagate_cost(s.propagate_in[::3], s.intra_cost[::3], s.lowres_costs[::3],
                                                 s.inv_qscale[::3], s.fps_factor))
    _check(hip, [s], w, h, ("intra 0",))


def test_propagate_more_steps_than_one_launch(hip):
    """17 steps on 2x2: the call splits after 16 (the launch's argument block), merged between"""
    w, h = 2, 2
    rng = np.random.default_rng(6)
    dst = _start_planes(rng, 4, hi=200)
    steps = [mt.crafted_step(rng, w, h, dst, "mid", FPS[1], 21, referenced=False) for _ in range(17)]
    start = [p.copy() for p in dst]
    _check(hip, steps, w, h, ("17 steps",))
    assert any(not np.array_equal(p, s0) for p, s0 in zip(dst, start))
    # the 17th step alone changes the result: the second launch ran
    again = [p.copy() for p in start]
    for s in steps[:16]:
        s.ref_costs = again
        mt.propagate_sequential(s, w, h)
    assert any(not np.array_equal(a, p) for a, p in zip(again, dst))


def test_propagate_accumulator_bound_split(hip):
    """363x361 = 131043 MBs, above the 131000 source MBs a 32-bit accumulator is safe for: each
    step is a launch of its own, walked in two MB ranges with a merge between"""
    w, h = 363, 361
    rng = np.random.default_rng(8)
    dst = _start_planes(rng, w * h)
    steps = [mt.crafted_step(rng, w, h, dst, "mid", FPS[k + 1], 21, referenced=False) for k in range(2)]
    _check(hip, steps, w, h, ("131043 MBs",))


def test_propagate_deterministic(hip):
    """the same n = 3 call twice from the same initial planes: identical planes"""
    w, h = 120, 68
    n = w * h
    rng = np.random.default_rng(9)
    dst = _start_planes(rng, n)
    steps = [mt.crafted_step(rng, w, h, dst, "mid", FPS[k], 21, referenced=False) for k in range(3)]
    runs = []
    for _ in range(2):
        planes = _Planes()
        gsteps = [_gpu_step(hip, s, planes) for s in steps]
        hip.mbtree_propagate(gsteps, w, h)
        torch.cuda.synchronize()
        runs.append([_u16(d) for d in planes.dev])
    for a, b, s0 in zip(runs[0], runs[1], dst):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, s0)


SENTINEL = np.float32(-12345.625)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("weightdelta", [0.0, 0.3])
@pytest.mark.parametrize("fps_factor", [5, 512, 51200])
def test_finish(hip, fps_factor, weightdelta, in_place):
    """random inputs over several blocks and a partial one, elements whose scaled intra cost is 0
    (left as they were: a sentinel, or the aq offset in place), propagate costs 0 and 32767"""
    n = 1000
    rng = np.random.default_rng(fps_factor)
    intra = np.where(rng.random(n) < 0.3, rng.integers(1, 40, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    with_aq = fps_factor != 512
    invq = np.where(rng.random(n) < 0.3, rng.integers(1, 4, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    prop = rng.integers(0, 32768, n).astype(np.uint16)
    prop[::7] = 0
    prop[3::7] = 32767
    aq = rng.uniform(-3, 3, n).astype(np.float32)
    strength = np.float32(5.0) * (np.float32(1.0) - np.float32(0.6))
    ic = (intra.astype(np.int64) * (invq if with_aq else 256) + 128) >> 8
    if with_aq:
        assert 20 < np.count_nonzero(ic == 0) < n // 2
    want = aq.copy() if in_place else np.full(n, SENTINEL)
    mt.finish(intra, invq if with_aq else None, prop, aq, want, fps_factor, weightdelta, strength)
    d_aq = _dev(aq)
    out = d_aq if in_place else _dev(np.full(n, SENTINEL))
    got = hip.mbtree_finish(_dev(intra), _dev(prop), d_aq, fps_factor, weightdelta, float(strength),
                            inv_qscale=_dev(invq) if with_aq else None, qp_offset=out)
    torch.cuda.synchronize()
    assert got is out
    g = got.cpu().numpy()
    bad = np.flatnonzero(g.view(np.uint32) != want.view(np.uint32))[:4]
    assert not len(bad), (bad, g[bad], want[bad], intra[bad], prop[bad])
    if not in_place:
        assert np.array_equal(d_aq.cpu().numpy().view(np.uint32), aq.view(np.uint32))
        assert np.all(g[ic == 0] == SENTINEL) and np.all(g[ic != 0] != SENTINEL)


class _DeviceBackend:
    """mbtree_plan's operations through the device entries, over per-frame device arrays"""

    def __init__(self, hip, par, host_frames, dev):
        self.hip, self.par, self.frames, self.dev = hip, par, host_frames, dev
        self.avg = mt.average_duration(host_frames)

    def zero(self, f):
        self.dev[f]["propagate"].zero_()

    def cost(self, p0, p1, b):
        assert b == p0 or (b - p0, p1 - b) in self.dev[b]["costs"]        # computed before the plan runs

    def propagate(self, steps):
        gs = []
        for p0, p1, b, referenced in steps:
            d = self.dev[b]
            gs.append(self.hip.mbtree_step(
                d["intra"], d["costs"][(b - p0, p1 - b)], d["mvs"][(0, b - p0 - 1)], self.dev[p0]["propagate"],
                mt.propagate_fps_factor(self.frames[b], self.avg),
                d["mvs"][(1, p1 - b - 1)] if b != p1 else None, self.dev[p1]["propagate"] if b != p1 else None,
                d["invq"], d["propagate"] if referenced else None, mt.bipred_weight(self.par, p0, p1, b)))
        self.hip.mbtree_propagate(gs, self.par.width, self.par.height)

    def finish(self, f, ref0_distance):
        fps, wd = mt.finish_params(self.frames[f], self.avg, ref0_distance)
        d = self.dev[f]
        self.hip.mbtree_finish(d["intra"], d["propagate"], d["aq"], fps, wd, float(self.par.strength),
                               inv_qscale=d["invq"], qp_offset=d["qp"])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(96, 64), (176, 144)])
def test_end_to_end_ibbp(hip, oracle, bd, size):
    """four frames typed IBBP: lowres planes, intra costs, the P cost (0,3,3) and the bidir costs
    (0,3,1), (0,3,2) on the device, mbtree_plan run through the device entries; expected: the
    literal macroblock_tree transcription over the same device-produced costs and mvs (pinned by
    test_gpu_lookahead)"""
    from x264hip import synth
    W, H = size
    frames, stride, origin = synth.make_sequence(4, W, H, bd)
    dev = torch.from_numpy(frames.view(np.int16) if bd == 10 else frames).cuda()
    lows, ls = hip.frame_init_lowres(dev, origin, stride, W, H)
    w, h = W // 16, H // 16
    n = w * h
    intra, _, _ = hip.lowres_intra_cost(lows[0], ls, w, h, True, True, 1)
    cm, c0 = oracle.cost_mv_table(1, 512)
    cmd = (torch.from_numpy(cm.view(np.int16)).cuda(), c0)
    aq_on = W == 176
    rng = np.random.default_rng(W + bd)
    par = mt.Params(w, h, False, False, weighted_bipred=True)
    host = [mt.Frame(t, n, 0.04, rng.integers(50, 1051, n).astype(np.uint16) if aq_on else None, rng)
            for t in "IBBP"]
    # P cost: frame 3 from frame 0
    p_mvs, _, p_lc, _, _ = hip.lowres_inter_cost(lows[0][3:4], [p[0:1] for p in lows], ls, w, h, intra[3:4], cmd)
    dv = [dict(intra=intra[f], costs={}, mvs={}, invq=_dev(host[f].i_inv_qscale_factor) if aq_on else None,
               propagate=_dev(host[f].i_propagate_cost), aq=_dev(host[f].f_qp_offset_aq),
               qp=_dev(host[f].f_qp_offset)) for f in range(4)]
    dv[3]["costs"][(3, 0)] = p_lc[0]
    dv[3]["mvs"][(0, 2)] = p_mvs[0]
    # bidir costs: frames 1 and 2 between 0 and 3
    for b in (1, 2):
        mvs = [torch.zeros((1, n, 2), dtype=torch.int16, device="cuda") for _ in range(2)]
        costs = [torch.zeros((1, n), dtype=torch.int32, device="cuda") for _ in range(2)]
        dsf = ((b << 8) + 1) // 3
        lc, _, _ = hip.lowres_bidir_cost(lows[0][b:b + 1], [p[0:1] for p in lows], [p[3:4] for p in lows], ls, w, h,
                                         cmd, 3, mvs[0], costs[0], mvs[1], costs[1], p1_mvs=p_mvs,
                                         dist_scale_factor=dsf, bipred_weight=mt.bipred_weight(par, 0, 3, b))
        dv[b]["costs"][(b, 3 - b)] = lc[0]
        dv[b]["mvs"][(0, b - 1)] = mvs[0][0]
        dv[b]["mvs"][(1, 3 - b - 1)] = mvs[1][0]
    torch.cuda.synchronize()
    for f in range(4):
        host[f].i_intra_cost = _u16(dv[f]["intra"]).copy()
        host[f].lowres_costs = {k: _u16(v).copy() for k, v in dv[f]["costs"].items()}
        host[f].lowres_mvs = {k: v.cpu().numpy().copy() for k, v in dv[f]["mvs"].items()}
    mt.run_plan(hip.mbtree_plan("IBBP"), _DeviceBackend(hip, par, host, dv))
    torch.cuda.synchronize()
    mt.macroblock_tree(par, host, lambda p0, p1, b: None, True)
    for f in (0, 3):                                            # the planes MB-tree accumulates into
        got = _u16(dv[f]["propagate"])
        bad = np.flatnonzero(got != host[f].i_propagate_cost)[:4]
        assert not len(bad), (f, bad, got[bad], host[f].i_propagate_cost[bad])
    assert host[0].i_propagate_cost.any()
    for f in range(4):
        got = dv[f]["qp"].cpu().numpy()
        bad = np.flatnonzero(got.view(np.uint32) != host[f].f_qp_offset.view(np.uint32))[:4]
        assert not len(bad), (f, bad, got[bad], host[f].f_qp_offset[bad])
    assert np.any(host[0].f_qp_offset != np.float32(99.0)) and np.all(host[1].f_qp_offset == np.float32(99.0))


def test_propagate_argument_errors(hip):
    """the X264HIP_EINVAL cases of x264hip_mbtree.h on real device planes; the planes stay as they were"""
    w, h = 6, 4
    n = w * h
    rng = np.random.default_rng(1)
    buf = torch.from_numpy(rng.integers(0, 9000, 8 * n).astype(np.int16)).cuda()
    before = buf.clone()
    P = [buf[k * n:(k + 1) * n] for k in range(8)]
    mv = torch.zeros((2, n, 2), dtype=torch.int16, device="cuda")
    L = hip.lib()
    V = ctypes.c_void_p

    def step(**kw):
        f = dict(intra_cost=P[0].data_ptr(), lowres_costs=P[1].data_ptr(), inv_qscale=None, propagate_in=None,
                 mvs=(V * 2)(mv[0].data_ptr(), mv[1].data_ptr()), ref_costs=(V * 2)(P[2].data_ptr(), P[3].data_ptr()),
                 fps_factor=0.002, bipred_weight=32)
        f.update(kw)
        return hip.MbtreeStep(**f)

    def call(steps, count=None, w_=w, h_=h):
        arr = (hip.MbtreeStep * max(1, len(steps)))(*steps)
        return L.x264hip_mbtree_propagate(arr, len(steps) if count is None else count, w_, h_, None)

    E = -1
    assert call([step()], count=0) == E and call([step()], count=-2) == E
    assert call([step()], w_=0) == E and call([step()], h_=0) == E and call([step()], w_=-6) == E
    assert L.x264hip_mbtree_propagate(None, 1, w, h, None) == E
    assert call([step(intra_cost=None)]) == E and call([step(lowres_costs=None)]) == E
    assert call([step(mvs=(V * 2)(None, mv[1].data_ptr()))]) == E
    assert call([step(ref_costs=(V * 2)(None, P[3].data_ptr()))]) == E
    assert call([step(ref_costs=(V * 2)(P[2].data_ptr(), None))]) == E
    assert call([step(bipred_weight=-1)]) == E and call([step(bipred_weight=65)]) == E
    assert call([step(propagate_in=P[2].data_ptr())]) == E
    assert call([step(), step(propagate_in=P[3].data_ptr())]) == E
    assert call([step(propagate_in=P[4].data_ptr()), step(ref_costs=(V * 2)(P[4].data_ptr(), P[3].data_ptr()))]) == E
    assert call([step(ref_costs=(V * 2)(P[2].data_ptr(), P[2].data_ptr() + 2))]) == E
    assert call([step(), step(ref_costs=(V * 2)(P[3].data_ptr() - 2 * (n - 1), P[5].data_ptr()))]) == E
    with pytest.raises(RuntimeError):
        hip.mbtree_propagate([], w, h)
    fin = L.x264hip_mbtree_finish
    f32 = torch.zeros(n, dtype=torch.float32, device="cuda")
    assert fin(None, None, P[1].data_ptr(), f32.data_ptr(), f32.data_ptr(), n, 512, 0.0, 2.0, None) == E
    assert fin(P[0].data_ptr(), None, P[1].data_ptr(), f32.data_ptr(), None, n, 512, 0.0, 2.0, None) == E
    assert fin(P[0].data_ptr(), None, P[1].data_ptr(), f32.data_ptr(), f32.data_ptr(), 0, 512, 0.0, 2.0, None) == E
    assert fin(P[0].data_ptr(), None, P[1].data_ptr(), f32.data_ptr(), f32.data_ptr(), n, 0, 0.0, 2.0, None) == E
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and not f32.any().item()
    # the accepted neighbours of the refused forms: identical and adjacent destinations
    assert call([step(ref_costs=(V * 2)(P[2].data_ptr(), P[2].data_ptr()))]) == 0
    assert call([step(propagate_in=P[4].data_ptr())]) == 0
    torch.cuda.synchronize()
