"""CPU: the checker and the ABI of batched motion compensation (no kernel is launched).

* tests/mc_cases.py's numpy restatement of get_ref / mc_weight / mc_chroma equals the oracle
  library's exported functions: all 16 luma phases, all 64 chroma phases, every block size, 8 and
  10 bit, weights with denom 0 and >= 1 and both offset signs, on planes at the top and the bottom
  of the range (both clips fire);
* the averaging rule equals a literal per-pixel loop of mc.c:49-99 for i_weight 32, 24, 44, -8, 72;
* the block-list mb_mc equals the one-block routines called block by block;
* include/x264hip_mc.h's prototypes, the ctypes declarations, the exported symbols and the struct
  layout agree, and x264hip.h knows nothing of them;
* every X264HIP_EINVAL case, and X264HIP_ENODEV without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mc_cases as mcc
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mc.h")
WEIGHTS = [(70, 6, -3), (2, 0, 5), (1, 0, -9), (33, 5, 12), (127, 7, -40)]


def _planes(bd, level, seed):
    """four full-range planes [1, 96, 128] whose values sit at the top / bottom / all over the range"""
    rng = np.random.default_rng(seed)
    pm = mcc.pixel_max(bd)
    lo, hi = {"top": (pm - 6, pm), "bottom": (0, 6), "full": (0, pm)}[level]
    dt = np.uint8 if bd == 8 else np.uint16
    return [rng.integers(lo, hi + 1, (1, 96, 128)).astype(dt) for _ in range(4)]


def _oracle_get_ref(oracle, bd, planes, off, stride, mvx, mvy, w, h):
    dt = planes[0].dtype
    dst = np.zeros(16 * 16, dt)
    ds = ctypes.c_ssize_t(16)
    ptrs = (ctypes.c_void_p * 4)(*[p.ctypes.data + off * p.itemsize for p in planes])
    r = oracle.fn(bd, "get_ref")(dst.ctypes.data, ctypes.byref(ds), ptrs, stride, mvx, mvy, w, h)
    if r == dst.ctypes.data:
        return dst.reshape(16, 16)[:h, :w].astype(np.int64)
    src = [p for p in planes if p.ctypes.data <= r < p.ctypes.data + p.nbytes]
    assert len(src) == 1 and ds.value == stride
    o = (r - src[0].ctypes.data) // src[0].itemsize
    flat = src[0].ravel()
    return np.stack([flat[o + yy * stride:o + yy * stride + w] for yy in range(h)]).astype(np.int64)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("level", ["top", "bottom", "full"])
def test_get_ref_and_weight_equal_oracle(oracle, bd, level):
    planes = _planes(bd, level, bd + len(level))
    stride, oy, ox = 128, 40, 48
    pm = mcc.pixel_max(bd)
    over = under = False
    seen = set()
    for i_pixel, (w, h) in enumerate(mcc.PIXEL_SIZES):
        for ph in range(16):
            mvx, mvy = 4 * (ph % 5 - 2) + (ph & 3), 4 * (2 - ph % 3) + (ph >> 2)
            seen.add(((mvy & 3) << 2) + (mvx & 3))
            got = mcc.get_ref(planes, oy, ox, 0, 4, 8, mvx, mvy, w, h)[0]
            want = _oracle_get_ref(oracle, bd, planes, (oy + 8) * stride + ox + 4, stride, mvx, mvy, w, h)
            assert np.array_equal(got, want), (i_pixel, mvx, mvy)
            wt = WEIGHTS[(ph + i_pixel) % len(WEIGHTS)]
            dst = np.zeros((h, w), planes[0].dtype)
            src = np.ascontiguousarray(want.astype(planes[0].dtype))
            oracle.fn(bd, "mc_weight")(dst.ctypes.data, w, src.ctypes.data, w, *wt, w, h)
            assert np.array_equal(mcc.mc_weight(got, wt, bd), dst), (i_pixel, mvx, mvy, wt)
            assert np.array_equal(mcc.mc_luma(planes, oy, ox, 0, 4, 8, mvx, mvy, w, h, wt, bd)[0], dst)
            raw = mcc.mc_weight(got, wt, bd, raw=True)
            over |= bool((raw > pm).any())
            under |= bool((raw < 0).any())
    assert seen == set(range(16))
    assert {d for _, d, _ in WEIGHTS} >= {0, 5, 6} and any(o < 0 for _, _, o in WEIGHTS)
    if level == "top":
        assert over
    if level == "bottom":
        assert under


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("level", ["top", "bottom", "full"])
def test_mc_chroma_equals_oracle(oracle, bd, level):
    nv = _planes(bd, level, 3 * bd)[0]
    stride, oy, ox = 128, 40, 48
    sizes = sorted({(w // 2, h >> vs) for w, h in mcc.PIXEL_SIZES for vs in (0, 1)})
    assert (2, 2) in sizes and (8, 16) in sizes
    for k, (w, h) in enumerate(sizes):
        for ph in range(64):
            mvx, mvy = 8 * ((ph + k) % 5 - 2) + (ph & 7), 8 * (1 - (ph + k) % 3) + (ph >> 3)
            gu, gv = mcc.mc_chroma(nv, oy, ox, 0, 8, 6, mvx, mvy, w, h)
            wu, wv = oracle.mc_chroma(bd, nv.ravel(), (oy + 6) * stride + ox + 8, stride, mvx, mvy, w, h)
            assert np.array_equal(gu[0], wu) and np.array_equal(gv[0], wv), (w, h, mvx, mvy)


def _avg_literal(a, b, w1, pm):
    """PIXEL_AVG_C (mc.c:90-99) pixel by pixel"""
    out = np.zeros_like(a)
    for yy in range(a.shape[0]):
        for xx in range(a.shape[1]):
            if w1 == 32:
                out[yy, xx] = (int(a[yy, xx]) + int(b[yy, xx]) + 1) >> 1
            else:
                v = (int(a[yy, xx]) * w1 + int(b[yy, xx]) * (64 - w1) + (1 << 5)) >> 6
                out[yy, xx] = 0 if v < 0 else pm if v > pm else v
    return out


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i_weight", [32, 24, 44, -8, 72])
def test_avg_rule_equals_literal_loop(bd, i_weight):
    rng = np.random.default_rng(i_weight + bd)
    pm = mcc.pixel_max(bd)
    a = rng.integers(0, pm + 1, (16, 16)).astype(np.int64)
    b = rng.integers(0, pm + 1, (16, 16)).astype(np.int64)
    a[0, :4], b[0, :4] = [pm, 0, pm, 0], [0, pm, pm, 0]
    want = _avg_literal(a, b, i_weight, pm)
    assert np.array_equal(mcc.avg(a, b, i_weight, bd), want)
    # the per-block form: three blocks, each with its own weight
    ws = np.array([i_weight, 32, 64 - i_weight])
    got = mcc.avg(np.stack([a, a, b]), np.stack([b, b, a]), ws, bd)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], _avg_literal(a, b, 32, pm))
    assert np.array_equal(got[2], _avg_literal(b, a, 64 - i_weight, pm))
    if i_weight in (-8, 72):
        raw = mcc.avg(a, b, i_weight, bd, raw=True)
        assert (raw > pm).any() and (raw < 0).any()


@pytest.mark.parametrize("bd,cf,i_pixel", [(8, 1, 0), (10, 2, 3), (8, 3, 5), (10, 1, 6), (8, 0, 1)])
def test_block_list_equals_block_by_block(bd, cf, i_pixel):
    """mb_mc of a mixed list (lists 1 / 2 / 3, weights, clipped mvs) == the one-block routines run
    block after block as mb_mc_0xywh / 1xywh / 01xywh call them"""
    W, H = 48, 32
    r0, r1 = mcc.make_ref(bd, W, H, cf, 2, 5, "full"), mcc.make_ref(bd, W, H, cf, 2, 9, "full")
    pos = mcc.block_positions(W, H, 2, i_pixel)
    mv0, mv1 = mcc.phase_mvs(pos, W, H, 1), mcc.phase_mvs(pos, W, H, 2, base=5)
    mv0[::4], mv1[1::3] = mcc.edge_mvs(pos, W, H, 3)[::4], mcc.edge_mvs(pos, W, H, 4)[1::3]
    par = mcc.make_par(pos, mv0, mv1, W, H)
    n = len(pos)
    mode = ((np.arange(n) % 3 + 1) | (np.array([32, 24, 44, -8, 72])[np.arange(n) % 5] << 8)).astype(np.int32)
    weights = ((70, 6, -3), None, (2, 0, 5))
    pred, pred_c = mcc.pred_planes(r0, sentinel=77)
    st = mcc.mb_mc(bd, cf, i_pixel, r0, r1, pos, par, mode, weights, pred, 32, 32, pred_c, 32, 32)
    assert st["clipped"] > 0
    bw, bh = mcc.PIXEL_SIZES[i_pixel]
    vs = 1 if cf == 1 else 0
    want, want_c = mcc.pred_planes(r0, sentinel=77)
    for (f, x, y), p, m in zip(pos.tolist(), par.astype(np.int64).tolist(), mode.tolist()):
        lists, biw = m & 3, m >> 8
        mv = [(min(max(p[2 * l], p[4]), p[6]), min(max(p[2 * l + 1], p[5]), p[7])) for l in range(2)]
        refs = (r0, r1)

        def luma_like(planes_of, wt):
            if lists == 3:
                a, b = (mcc.get_ref(planes_of(refs[l]), 32, 32, f, x, y, *mv[l], bw, bh)[0] for l in range(2))
                return mcc.avg(a, b, biw, bd)
            l = 0 if lists == 1 else 1
            return mcc.mc_luma(planes_of(refs[l]), 32, 32, f, x, y, *mv[l], bw, bh, wt if lists == 1 else None, bd)[0]
        want[f, 32 + y:32 + y + bh, 32 + x:32 + x + bw] = luma_like(lambda r: r.luma, weights[0])
        if cf == 3:
            for pl in range(2):
                want_c[pl][f, 32 + y:32 + y + bh, 32 + x:32 + x + bw] = luma_like(
                    lambda r: r.chroma[4 * pl:4 * pl + 4], weights[1 + pl])
        elif cf:
            cw, ch = bw // 2, bh >> vs
            uv = [mcc.mc_chroma(refs[l].chroma[0], 32, 32, f, x, y >> vs, mv[l][0], (2 * mv[l][1]) >> vs, cw, ch)
                  for l in range(2)]
            for pl in range(2):
                if lists == 3:
                    blk = mcc.avg(uv[0][pl][0], uv[1][pl][0], biw, bd)
                else:
                    blk = uv[0 if lists == 1 else 1][pl][0]
                    if lists == 1 and weights[1 + pl] is not None:
                        blk = mcc.mc_weight(blk, weights[1 + pl], bd)
                want_c[0][f, 32 + (y >> vs):32 + (y >> vs) + ch, 32 + x + pl:32 + x + pl + 2 * cw:2] = blk
    assert np.array_equal(pred, want)
    for a, b in zip(pred_c, want_c):
        assert np.array_equal(a, b)
    assert (pred != 77).any()


def test_restatement_speed_1080p():
    """a 1080p frame of 4x4 blocks through the restatement in well under a second per plane set"""
    import time
    r0 = mcc.make_ref(8, 1920, 1088, 1, 1, 3, "full")
    pos = mcc.block_positions(1920, 1088, 1, 6)
    par = mcc.make_par(pos, mcc.phase_mvs(pos, 1920, 1088, 4), np.zeros((len(pos), 2), np.int64), 1920, 1088)
    pred, pred_c = mcc.pred_planes(r0)
    t = time.perf_counter()
    mcc.mb_mc(8, 1, 6, r0, None, pos, par, None, (None, None, None), pred, 32, 32, pred_c, 32, 32)
    assert time.perf_counter() - t < 5.0          # measured ~0.5 s; the bound only catches a per-block loop


# ------------------------------------------------------------------ ABI
_SCALARS = {"intptr_t": ctypes.c_ssize_t, "int": ctypes.c_int}


def _prototypes():
    """{name: (return text, [parameter text])} of the x264hip_*_mb_mc functions a C compiler sees in
    x264hip_mc.h (the header's own declarations only: x264hip.h's are test_abi.py's)"""
    src = subprocess.run(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"), HEADER],
                         capture_output=True, text=True, check=True).stdout
    own = subprocess.run(["gcc", "-E", "-P", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "include", "x264hip.h")], capture_output=True, text=True, check=True).stdout
    known = set(re.findall(r"\b(x264hip_\w+)\s*\(", own))
    protos = {}
    for decl in " ".join(src.split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1) and m.group(2) not in known:
            assert m.group(2) not in protos
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text or "[" in text:
        return ctypes.c_void_p
    ctype = [w for w in text.split() if w != "const"][0]
    assert ctype in _SCALARS, f"unclassified C type {text!r}"
    return _SCALARS[ctype]


def test_mc_signatures_match_header():
    ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    assert sorted(protos) == sorted(f"x264hip_{bd}_{n}" for n in x._MC for bd in (8, 10)) == \
        ["x264hip_10_mb_mc", "x264hip_8_mb_mc"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret), name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params) == 7, name
        for i, (p, a) in enumerate(zip(params, fn.argtypes)):
            assert a is _ctype_of(p), (name, i, p, a)
    assert "mb_mc" in x.__all__ and "Mc" in x.__all__ and callable(x.mb_mc)


def test_mc_symbols_exported_and_header_stands_apart():
    so = ensure_built("hip")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(_prototypes()) <= exported
    assert "mb_mc" not in open(os.path.join(ROOT, "include", "x264hip.h")).read()
    assert '#include "x264hip.h"' in open(HEADER).read()


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "x264hip_mc.h"
#define P(F) printf(#F " %zu\n", offsetof(x264hip_mc_t, F));
#define R(F) printf(#F " %zu\n", offsetof(x264hip_mc_ref_t, F));
int main(void) {
    printf("size %zu\n", sizeof(x264hip_mc_t));
    P(chroma_format) P(ref) P(ref_stride) P(ref_frame_stride) P(ref_chroma_stride) P(ref_chroma_frame_stride)
    P(weight) P(pred) P(pred_stride) P(pred_frame_stride) P(pred_chroma) P(pred_chroma_stride)
    P(pred_chroma_frame_stride)
    printf("refsize %zu\n", sizeof(x264hip_mc_ref_t));
    R(luma) R(chroma)
    return 0;
}
"""


def test_mc_layout_matches_ctypes(tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines()]
    k = [n for n, _ in lines].index("refsize")
    vals, rvals = dict(lines[:k]), dict(lines[k:])
    x = load_package()
    S, Rf = x.Mc, x.McRef
    assert int(vals.pop("size")) == ctypes.sizeof(S) == 336
    assert [n for n, _ in S._fields_] == list(vals)
    for name, off in vals.items():
        assert getattr(S, name).offset == int(off), name
    assert int(rvals.pop("refsize")) == ctypes.sizeof(Rf) == 96
    assert [n for n, _ in Rf._fields_] == list(rvals)
    for name, off in rvals.items():
        assert getattr(Rf, name).offset == int(off), name


V = ctypes.c_void_p


def _mc(x, cf=1, **kw):
    """a valid x264hip_mc_t on made-up, aligned addresses"""
    m = x.Mc()
    m.chroma_format = cf
    for l in range(2):
        for k in range(4):
            m.ref[l].luma[k] = 0x100000 * (1 + 4 * l + k)
        for k in range(8):
            m.ref[l].chroma[k] = 0x1000000 * (1 + 8 * l + k)
    m.ref_stride, m.ref_frame_stride, m.ref_chroma_stride, m.ref_chroma_frame_stride = 192, 192 * 128, 192, 192 * 96
    m.pred, m.pred_stride, m.pred_frame_stride = 0x40000000, 192, 192 * 128
    m.pred_chroma[0], m.pred_chroma[1] = 0x50000000, 0x60000000
    m.pred_chroma_stride, m.pred_chroma_frame_stride = 192, 192 * 96
    for name, v in kw.items():
        setattr(m, name, v)
    return m


POS, PAR, MODE = V(0x70000000), V(0x71000000), V(0x72000000)


@pytest.mark.parametrize("bd", [8, 10])
def test_mc_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_mc")
    EINVAL = -1

    def call(m, i_pixel=0, pos=POS, par=PAR, mode=MODE, n=4):
        return fn(ctypes.byref(m) if m is not None else None, i_pixel, pos, par, mode, n, None)

    assert call(_mc(x), n=-1) == EINVAL
    assert call(None) == EINVAL
    assert call(_mc(x), pos=None) == EINVAL and call(_mc(x), par=None) == EINVAL
    assert call(_mc(x), i_pixel=-1) == EINVAL and call(_mc(x), i_pixel=7) == EINVAL
    assert call(_mc(x, cf=-1)) == EINVAL and call(_mc(x, cf=4)) == EINVAL
    assert call(_mc(x, pred=None)) == EINVAL
    for cf in (1, 2, 3):
        m = _mc(x, cf=cf)
        m.pred_chroma[0] = None
        assert call(m) == EINVAL, cf
    m = _mc(x, cf=3)
    m.pred_chroma[1] = None
    assert call(m) == EINVAL
    for k in range(4):                                      # mode == NULL needs list 0's planes
        m = _mc(x, cf=0)
        m.ref[0].luma[k] = None
        assert call(m, mode=None) == EINVAL, k
    m = _mc(x, cf=1)
    m.ref[0].chroma[0] = None
    assert call(m, mode=None) == EINVAL
    m = _mc(x, cf=3)
    m.ref[0].chroma[6] = None
    assert call(m, mode=None) == EINVAL
    m = _mc(x)
    m.weight[1] = x.Weight(1, 64, 8, 0)
    assert call(m) == EINVAL
    assert call(_mc(x, pred=0x40000002)) == EINVAL and call(_mc(x, pred_stride=190)) == EINVAL
    # the same errors with n == 0; a valid call with n == 0 is OK everywhere
    assert call(None, n=0) == EINVAL and call(_mc(x, pred=None), n=0) == EINVAL
    for cf in range(4):
        assert call(_mc(x, cf=cf), n=0) == 0 and call(_mc(x, cf=cf), mode=None, n=0) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_mc_entries_return_enodev_without_device(bd):
    """a valid call is X264HIP_ENODEV where no device exists (nothing is dereferenced on the host)"""
    ensure_built("hip")
    x = load_package()
    L = x.lib()
    if L.x264hip_available():
        pytest.skip("a gfx950 device is visible: the calls would run on these made-up addresses")
    fn = getattr(L, f"x264hip_{bd}_mb_mc")
    ENODEV = -3
    for cf in range(4):
        for i_pixel in (0, 6):
            assert fn(ctypes.byref(_mc(x, cf=cf)), i_pixel, POS, PAR, MODE, 4, None) == ENODEV
            assert fn(ctypes.byref(_mc(x, cf=cf)), i_pixel, POS, PAR, None, 4, None) == ENODEV
    m = _mc(x, cf=0)                                        # list 1 all NULL, no chroma at format 0
    for k in range(4):
        m.ref[1].luma[k] = None
    m.pred_chroma[0] = m.pred_chroma[1] = None
    assert fn(ctypes.byref(m), 3, POS, PAR, None, 1, None) == ENODEV
