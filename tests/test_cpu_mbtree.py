"""CPU: MB-tree's checker, plan and ABI (no kernel is launched).

* the clip-adds of mbtree_propagate_list commute (what lets the device sum them with atomics
  and lets several steps share one call);
* the numpy restatement's float expression equals a C build of it under the reference's own
  compiler flags and under strict flags;
* mbtree_plan's operations, run batched, give what the literal macroblock_tree loop gives;
* include/x264hip_mbtree.h's prototypes, the ctypes declarations and the exported symbols agree;
* the x264_log2 tables of the product and of the restatement equal the recorded reference text."""
import copy
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mbtree_cases as mt
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mbtree.h")
KERNELS = os.path.join(ROOT, "x264-i386pic_amd", "csrc", "mbtree.hip")


# ------------------------------------------------------------------ tables
def _hip_floats(name):
    src = open(KERNELS).read()
    m = re.search(r"\b" + name + r"\s*\[\d+\]\s*=\s*\{([^{}]*)\}", src)
    assert m, name
    return np.array([float(v) for v in re.findall(r"-?\d+(?:\.\d+)?", m.group(1))], np.float64).astype(np.float32)


def test_log2_tables_match_fixture():
    lut, lz = mt.fixture_tables()
    assert len(lut) == 128 and len(lz) == 32
    assert lut[0] == 0 and lut[127] == np.float32(0.99435) and np.all(np.diff(lut) > 0)
    assert np.array_equal(lz, np.arange(31, -1, -1, dtype=np.float32))
    assert np.array_equal(mt.LOG2_LUT.view(np.uint32), lut.view(np.uint32))
    assert np.array_equal(mt.LOG2_LZ_LUT.view(np.uint32), lz.view(np.uint32))
    assert np.array_equal(_hip_floats("k_log2_lut").view(np.uint32), lut.view(np.uint32))
    assert np.array_equal(_hip_floats("k_log2_lz_lut").view(np.uint32), lz.view(np.uint32))
    # the product's initialisers carry no float suffix: like the reference's they are doubles
    # converted to float, the conversion the fixture's reader applies
    assert not re.search(r"\d\.\d+f", open(KERNELS).read().split("k_log2_lut")[1].split("};")[0])


def test_x264_log2_restatement():
    x = np.array([1, 2, 3, 255, 256, 257, 0x7fff, 0x12345678, 0xffffffff], np.uint64)
    got = mt.x264_log2(x)
    assert got.dtype == np.float32
    assert got[0] == 0 and got[1] == 1 and got[4] == 8
    assert np.all(np.abs(got - np.log2(x.astype(np.float64))) < 0.012)      # the table's step


# ------------------------------------------------------------------ order independence
def _apply(plane, adds):
    for _, idx, v in adds:
        plane[idx] = min(int(plane[idx]) + v, 32767)


@pytest.mark.parametrize("size", [(6, 4), (11, 9)])
@pytest.mark.parametrize("saturate", [True, False])
def test_clip_adds_commute(size, saturate):
    """sequential MC_CLIP_ADDs == sum per destination then one clip == the same adds shuffled"""
    w, h = size
    n = w * h
    rng = np.random.default_rng(7 + w)
    start = rng.integers(30000, 32768, n).astype(np.uint16) if saturate else rng.integers(0, 9000, n).astype(np.uint16)
    plane = start.copy()
    step = (mt.saturating_step(rng, w, h, [plane, plane]) if saturate
            else mt.crafted_step(rng, w, h, [plane, plane], "mid", 0.0013, 21))
    adds = mt.step_adds(step, w, h)
    assert len(adds) > n // 2
    mt.propagate_sequential(step, w, h)
    if saturate:
        assert plane[n // 2] == 32767 and sum(v for _, i, v in adds if i == n // 2) > 10 * 32767
    summed = start.astype(np.int64)
    for _, idx, v in adds:
        assert v >= 0
        summed[idx] += v
    assert np.array_equal(plane, np.minimum(summed, 32767))
    for seed in range(3):
        shuffled = start.copy()
        order = np.random.default_rng(seed).permutation(len(adds))
        _apply(shuffled, [adds[k] for k in order])
        assert np.array_equal(shuffled, plane)
    again = start.copy()
    step.ref_costs = [again, again]
    mt.propagate_batched([step], w, h)
    assert np.array_equal(again, plane)


@pytest.mark.parametrize("saturate", [True, False])
def test_batched_steps_equal_sequential_steps(saturate):
    """three steps sharing both destination planes: one batched call == one after another"""
    w, h = 11, 9
    n = w * h
    rng = np.random.default_rng(3)
    lo = 30000 if saturate else 0
    start = [rng.integers(lo, 32768 if saturate else 6000, n).astype(np.uint16) for _ in range(2)]
    seq = [p.copy() for p in start]
    bat = [p.copy() for p in start]
    steps = []
    for k in range(3):
        s = (mt.saturating_step(rng, w, h, seq, target=5 + k) if saturate
             else mt.crafted_step(rng, w, h, seq, ("none", "mid", "max")[k], (1 / 512, 0.0013, 0.19)[k], 21,
                                  referenced=False))
        steps.append(s)
        mt.propagate_sequential(s, w, h)
    for s in steps:
        s.ref_costs = bat
    mt.propagate_batched(steps, w, h)
    for a, b, s0 in zip(seq, bat, start):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, s0)


def test_unsigned_edge_rules():
    """the literal unsigned compares accept exactly the shares inside the frame (what the kernel
    tests with signed coordinates), for mbx / mby from -2 to one past the edge"""
    w, h = 3, 2
    for mb_y in range(h):
        for dx in range(-3 * 32 - 7, 3 * 32 + 8, 13):
            for dy in range(-2 * 32 - 5, 2 * 32 + 6, 11):
                mvs = np.array([[dx, dy]] * w, np.int16)
                costs = np.full(w, 1 << 14, np.uint16)
                amount = np.full(w, 1000)
                got = []
                mt.propagate_list(lambda idx, v: got.append((idx, v)), mvs, amount, costs, 32, mb_y, w, h, 0)
                want = []
                for i in range(w):
                    if dx == 0 and dy == 0:
                        want.append((mb_y * w + i, 1000))
                        continue
                    mbx, mby, x, y = (dx >> 5) + i, (dy >> 5) + mb_y, dx & 31, dy & 31
                    wt = [(32 - y) * (32 - x), (32 - y) * x, y * (32 - x), y * x]
                    for k in range(4):
                        cx, cy = mbx + (k & 1), mby + (k >> 1)
                        if 0 <= cx < w and 0 <= cy < h:
                            want.append((cy * w + cx, (wt[k] * 1000 + 512) >> 10))
                assert got == want, (mb_y, dx, dy)


# ------------------------------------------------------------------ float contract
@pytest.fixture(scope="module")
def float_builds(tmp_path_factory):
    gcc = shutil.which("gcc")
    assert gcc, "the float contract is checked against gcc builds"
    d = tmp_path_factory.mktemp("mbtree_float")
    src = os.path.join(ROOT, "tests", "c", "mbtree_float.c")
    out = {}
    for tag, flags in (("reference", ["-O3", "-ffast-math", "-fno-tree-vectorize"]),
                       ("strict", ["-O2", "-ffp-contract=off"])):
        exe = str(d / tag)
        subprocess.run([gcc, "-std=gnu99", *flags, src, "-o", exe], check=True)
        out[tag] = exe
    return d, out


def test_float_contract_against_c_builds(float_builds):
    """propagate_cost of the restatement == the C expression built with the reference's flags
    (-O3 -ffast-math -fno-tree-vectorize) == built strictly, on 2^20 + 77 inputs of the domain
    (intra / inv_qscale in [1, 0x7fff], fps_factor in (0, 1], propagate_in <= 32767)"""
    d, builds = float_builds
    n, chunk = (1 << 20) + 77, 1024
    rng = np.random.default_rng(11)
    pin = np.where(rng.random(n) < 0.3, 0, rng.integers(0, 32768, n)).astype(np.uint16)
    intra = np.where(rng.random(n) < 0.5, rng.integers(1, 4000, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    inter = ((rng.integers(0, 4, n) << 14) + np.minimum((intra * rng.random(n) * 1.3).astype(np.int64), 0x3fff))
    inter = inter.astype(np.uint16)
    invq = np.where(rng.random(n) < 0.5, rng.integers(50, 1051, n), rng.integers(1, 0x8000, n)).astype(np.uint16)
    invq[:9] = 0x7fff
    intra[:9] = 0x7fff
    nch = (n + chunk - 1) // chunk
    fps = np.exp(rng.uniform(np.log(1e-4), 0, nch)).astype(np.float32)
    fps[:4] = [1.0, 1 / 512, 0.0013, 0.19]
    want = np.empty(n, np.int64)
    for c in range(nch):
        r = slice(c * chunk, (c + 1) * chunk)
        want[r] = mt.propagate_cost(pin[r], intra[r], inter[r], invq[r], fps[c])
    assert want.min() == 0 and want.max() == 32767 and len(np.unique(want)) > 20000
    inp = d / "in.bin"
    with open(inp, "wb") as fh:
        np.array([n, chunk], np.int32).tofile(fh)
        for a in (pin, intra, inter, invq, fps):
            a.tofile(fh)
    for tag, exe in builds.items():
        outp = d / f"{tag}.bin"
        subprocess.run([exe, str(inp), str(outp)], check=True)
        got = np.fromfile(outp, np.int16).astype(np.int64)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (tag, len(bad), bad[:4], got[bad[:4]], want[bad[:4]])


def test_zero_intra_cost_is_amount_zero():
    got = mt.propagate_cost(np.array([5, 5]), np.array([0, 9]), np.array([0, 3]), np.array([256, 256]), 0.5)
    assert got[0] == 0 and got[1] > 0


# ------------------------------------------------------------------ plan
def test_plan_worked_example():
    x = load_package()
    assert x.mbtree_plan("IBBP") == [
        ("cost", 0, 0, 0), ("zero", 3), ("cost", 0, 3, 3), ("zero", 0), ("cost", 0, 3, 2), ("cost", 0, 3, 1),
        ("propagate", [(0, 3, 2, False), (0, 3, 1, False)]), ("propagate", [(0, 3, 3, True)]), ("finish", 0, 0)]
    # pyramid: the outer Bs of one mini-GOP share a call over three destination planes
    ops = x.mbtree_plan("IBBBP", bframe_pyramid=True)
    assert ("propagate", [(2, 4, 3, False), (0, 2, 1, False)]) in ops
    assert ops[-3:] == [("propagate", [(0, 4, 4, True)]), ("finish", 0, 0), ("finish", 2, 0)]
    assert x.mbtree_plan("PBB", b_intra=False) == []            # nothing but trailing Bs after frame 0
    assert x.mbtree_plan("IP", vbv=True)[-3:] == [("propagate", [(0, 1, 1, True)]), ("finish", 1, 1), ("finish", 0, 0)]


def _frames(types, n, seed, aq):
    rng = np.random.default_rng(seed)
    dur = [0.04, 0.02, 1 / 30, 0.04, 0.005, 0.05, 2.0, 0.04]
    return [mt.Frame(t, n, dur[i % len(dur)],
                     rng.integers(50, 1051, n).astype(np.uint16) if aq else None, rng)
            for i, t in enumerate(types)]


@pytest.mark.parametrize("vbv", [False, True])
@pytest.mark.parametrize("pyramid", [False, True])
@pytest.mark.parametrize("types,b_intra", [("IP", True), ("IBP", True), ("IBBP", True), ("IBBBPBBP", True),
                                            ("IBBPBB", True), ("PBBP", False), ("PPBBPBP", False)])
def test_plan_equals_literal_macroblock_tree(types, b_intra, pyramid, vbv):
    """mbtree_plan's operations run with the restatement (each propagate operation as one batched
    call) leave every i_propagate_cost plane and every f_qp_offset as the literal, unbatched
    macroblock_tree transcription does, from stale planes and the same costs"""
    x = load_package()
    w, h = 5, 4
    n = w * h
    seed = len(types) * 4 + pyramid * 2 + vbv
    par = mt.Params(w, h, pyramid, vbv)
    lit = _frames(types, n, seed, aq=True)
    bat = copy.deepcopy(lit)
    mt.macroblock_tree(par, lit, mt.random_frame_costs(seed, lit, w, h), b_intra)
    ops = x.mbtree_plan(types, bframe_pyramid=pyramid, vbv=vbv, b_intra=b_intra)
    mt.run_plan(ops, mt.HostBackend(par, bat, mt.random_frame_costs(seed, bat, w, h)))
    for i, (a, b) in enumerate(zip(lit, bat)):
        assert np.array_equal(a.i_propagate_cost, b.i_propagate_cost), (i, "i_propagate_cost")
        assert np.array_equal(a.f_qp_offset.view(np.uint32), b.f_qp_offset.view(np.uint32)), (i, "f_qp_offset")
        assert sorted(a.lowres_costs) == sorted(b.lowres_costs), (i, "requested costs")
    # the run did something: every finished frame has offsets, every propagate step left cost
    finished = [o[1] for o in ops if o[0] == "finish"]
    assert finished
    for f in finished:
        assert np.any(lit[f].f_qp_offset != np.float32(99.0)), f
    for o in ops:
        if o[0] == "propagate":
            assert lit[o[1][0][0]].i_propagate_cost.any()


# ------------------------------------------------------------------ ABI
_SCALARS = {"intptr_t": ctypes.c_ssize_t, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float}


def _prototypes():
    """{name: (return text, [parameter text])} of the x264hip_mbtree_* functions a C compiler sees
    in x264hip_mbtree.h (test_abi.py's method; x264hip.h's own prototypes are left to that file)"""
    src = subprocess.run(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), HEADER],
                         capture_output=True, text=True, check=True).stdout
    protos = {}
    for decl in " ".join(src.split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_mbtree_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1):
            assert m.group(2) not in protos
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text or "[" in text:
        return ctypes.c_void_p
    ctype = [w for w in text.split() if w != "const"][0]
    assert ctype in _SCALARS, f"unclassified C type {text!r}"
    return _SCALARS[ctype]


def test_mbtree_signatures_match_header():
    x = load_package()
    protos = _prototypes()
    assert sorted(protos) == sorted(f"x264hip_mbtree_{n}" for n in x._MBTREE) == \
        ["x264hip_mbtree_finish", "x264hip_mbtree_propagate"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret), name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for i, (p, a) in enumerate(zip(params, fn.argtypes)):
            assert a is _ctype_of(p), (name, i, p, a)
    assert ctypes.c_float in L.x264hip_mbtree_finish.argtypes


def test_mbtree_symbols_exported_and_header_stands_apart():
    so = ensure_built("hip")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(_prototypes()) <= exported
    assert "mbtree" not in open(os.path.join(ROOT, "include", "x264hip.h")).read()
    assert '#include "x264hip.h"' in open(HEADER).read()


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "x264hip_mbtree.h"
#define P(F) printf(#F " %zu\n", offsetof(x264hip_mbtree_step_t, F));
int main(void) {
    printf("size %zu\n", sizeof(x264hip_mbtree_step_t));
    P(intra_cost) P(lowres_costs) P(inv_qscale) P(propagate_in) P(mvs) P(ref_costs) P(fps_factor) P(bipred_weight)
    return 0;
}
"""


def test_step_layout_matches_ctypes(tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    S = load_package().MbtreeStep
    assert int(vals.pop("size")) == ctypes.sizeof(S) == 72
    assert [n for n, _ in S._fields_] == list(vals)
    for name, off in vals.items():
        assert getattr(S, name).offset == int(off), name


def test_mbtree_argument_errors():
    """argument errors are X264HIP_EINVAL before any HIP call (no pointer is dereferenced)"""
    x = load_package()
    L = x.lib()
    V = ctypes.c_void_p
    n = 64                                                    # 8 x 8 MBs: planes of 128 bytes
    A, B, C, D, E, Fp, G = (V(0x10000 + 0x1000 * k) for k in range(7))

    def step(**kw):
        f = dict(intra_cost=A, lowres_costs=B, inv_qscale=None, propagate_in=None, mvs=(V * 2)(C, D),
                 ref_costs=(V * 2)(E, Fp), fps_factor=0.002, bipred_weight=32)
        f.update(kw)
        return x.MbtreeStep(**f)

    def call(steps, count=None, w=8, h=8):
        arr = (x.MbtreeStep * max(1, len(steps)))(*steps)
        return L.x264hip_mbtree_propagate(arr, len(steps) if count is None else count, w, h, None)

    EINVAL = -1
    assert call([step()], count=0) == EINVAL
    assert L.x264hip_mbtree_propagate(None, 1, 8, 8, None) == EINVAL
    assert call([step()], w=0) == EINVAL and call([step()], h=-1) == EINVAL
    for name in ("intra_cost", "lowres_costs"):
        assert call([step(**{name: None})]) == EINVAL, name
    assert call([step(mvs=(V * 2)(None, D))]) == EINVAL
    assert call([step(ref_costs=(V * 2)(None, Fp))]) == EINVAL
    assert call([step(ref_costs=(V * 2)(E, None))]) == EINVAL
    assert call([step(bipred_weight=-1)]) == EINVAL and call([step(bipred_weight=65)]) == EINVAL
    # a destination that is some step's source, in the same step or another
    assert call([step(propagate_in=E)]) == EINVAL
    assert call([step(), step(propagate_in=Fp)]) == EINVAL
    assert call([step(propagate_in=G), step(ref_costs=(V * 2)(G, Fp))]) == EINVAL
    # destinations that overlap without being identical (planes are n * 2 bytes)
    assert call([step(ref_costs=(V * 2)(E, V(E.value + 2 * n - 2)))]) == EINVAL
    assert call([step(), step(ref_costs=(V * 2)(V(Fp.value - 64), G))]) == EINVAL
    fin = L.x264hip_mbtree_finish
    assert fin(None, None, B, C, C, n, 512, 0.0, 2.0, None) == EINVAL
    assert fin(A, None, None, C, C, n, 512, 0.0, 2.0, None) == EINVAL
    assert fin(A, None, B, None, C, n, 512, 0.0, 2.0, None) == EINVAL
    assert fin(A, None, B, C, None, n, 512, 0.0, 2.0, None) == EINVAL
    assert fin(A, None, B, C, C, 0, 512, 0.0, 2.0, None) == EINVAL
    assert fin(A, None, B, C, C, n, 0, 0.0, 2.0, None) == EINVAL


def test_mbtree_entries_return_enodev_without_device():
    """a valid call is X264HIP_ENODEV where no device exists (no pointer is dereferenced on the host)"""
    x = load_package()
    L = x.lib()
    if L.x264hip_available():
        pytest.skip("a gfx950 device is visible: the calls would run on these made-up addresses")
    V = ctypes.c_void_p
    n = 64
    A, B, C, D, E, Fp, G = (V(0x10000 + 0x1000 * k) for k in range(7))

    def step(**kw):
        f = dict(intra_cost=A, lowres_costs=B, inv_qscale=None, propagate_in=None, mvs=(V * 2)(C, D),
                 ref_costs=(V * 2)(E, Fp), fps_factor=0.002, bipred_weight=32)
        f.update(kw)
        return x.MbtreeStep(**f)

    def call(steps):
        arr = (x.MbtreeStep * len(steps))(*steps)
        return L.x264hip_mbtree_propagate(arr, len(steps), 8, 8, None)

    ENODEV = -3
    fin = L.x264hip_mbtree_finish
    # valid forms: identical destinations, list 1 absent with ref_costs[1] unset, adjacent planes
    assert call([step()]) == ENODEV
    assert call([step(ref_costs=(V * 2)(E, E)), step(propagate_in=G)]) == ENODEV
    assert call([step(mvs=(V * 2)(C, None), ref_costs=(V * 2)(E, None))]) == ENODEV
    assert call([step(ref_costs=(V * 2)(E, V(E.value + 2 * n)))]) == ENODEV
    assert fin(A, None, B, C, C, n, 512, 0.0, 2.0, None) == ENODEV
    assert fin(A, D, B, C, E, n, 51200, 0.3, 2.0, None) == ENODEV
