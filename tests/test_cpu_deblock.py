"""CPU: the checker, the inputs and the ABI of the deblocking entries (no kernel is launched).

* hand-worked vectors of the four line filters of tests/deblock_cases.py: a row that fires and
  one that does not, the tc clip at both depths;
* the anti-diagonal order x + 2y equals raster order on every input the GPU tests run;
* conditions on those inputs, so the GPU tests cannot pass vacuously: filtering all vertical
  edges before all horizontal ones gives a different picture in >= 1 % of the luma pixels, and
  >= 25 % of the luma pixels change (the generator at 5x4 MBs, qp 40, every bs 2: 6.6 % and 84 %);
* deblock_strength_py against a block-pair-by-block-pair loop written from the rule;
* the three tables: tests/golden/deblock_tables.json, the product's __constant__ copies and,
  where X264_REFERENCE_DIR names the reference tree, its text;
* include/x264hip_deblock.h's prototypes, the ctypes declarations, the exported symbols and the
  struct layouts agree; every X264HIP_EINVAL case; X264HIP_ENODEV without a device."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import deblock_cases as dc
from conftest import ROOT, ensure_built, load_package
from test_ref_tables import c_array

HEADER = os.path.join(ROOT, "include", "x264hip_deblock.h")


# ------------------------------------------------------------------ the line filters, by hand
def _rows(*rows):
    return np.array(rows, np.int32)


def test_edge_luma_by_hand():
    # alpha 20, beta 6.  Row 0, tc0 2: |p0-q0| = 8, both sides flat, so tc = 4; avg = 104,
    # p1' = 100 + clip(102 - 100, +-2) = 102, q1' = 108 + clip(106 - 108, +-2) = 106,
    # delta = clip((32 - 8 + 4) >> 3 = 3, +-4) = 3.  Row 1, tc0 0: p1, q1 stay, tc = 2, delta clipped
    # 3 -> 2.  Row 2: |p0-q0| = 25 >= alpha.  Row 3: tc0 < 0.
    P = _rows([100, 100, 100, 100, 108, 108, 108, 108], [100, 100, 100, 100, 108, 108, 108, 108],
              [100, 100, 100, 100, 125, 125, 125, 125], [100, 100, 100, 100, 108, 108, 108, 108])
    dc.edge_luma(P, 20, 6, [2, 0, 2, -1], 8)
    assert P.tolist() == [[100, 100, 102, 103, 105, 106, 108, 108], [100, 100, 100, 102, 106, 108, 108, 108],
                          [100, 100, 100, 100, 125, 125, 125, 125], [100, 100, 100, 100, 108, 108, 108, 108]]
    # 10 bit: alpha 80, beta 24, tc0 8: tc = 10, delta = (128 - 32 + 4) >> 3 = 12 clipped to 10;
    # row 1 mirrored at the top of the range: delta = -92 >> 3 = -12 clipped to -10
    P = _rows([400, 400, 400, 400, 432, 432, 432, 432], [1023, 1023, 1023, 1023, 991, 991, 991, 991],
              [400, 400, 400, 400, 480, 480, 480, 480])
    dc.edge_luma(P, 80, 24, [8, 8, 8], 10)
    assert P.tolist() == [[400, 400, 408, 410, 422, 424, 432, 432], [1023, 1023, 1015, 1013, 1001, 999, 991, 991],
                          [400, 400, 400, 400, 480, 480, 480, 480]]


def test_edge_chroma_by_hand():
    # delta = 3 before the clip: tc 2 clips it, tc 4 does not, tc 0 skips the line, row 3 does not fire
    P = _rows([100, 100, 108, 108], [100, 100, 108, 108], [100, 100, 108, 108], [100, 100, 125, 125])
    dc.edge_chroma(P, 20, 6, [2, 4, 0, 2], 8)
    assert P.tolist() == [[100, 102, 106, 108], [100, 103, 105, 108], [100, 100, 108, 108], [100, 100, 125, 125]]
    P = _rows([400, 400, 432, 432], [400, 400, 500, 500])          # 10 bit: tc = 2 * 4 + 1, delta 12 -> 9
    dc.edge_chroma(P, 80, 24, [9, 9], 10)
    assert P.tolist() == [[400, 409, 423, 432], [400, 400, 500, 500]]


def test_edge_luma_intra_by_hand():
    # beta 6.  alpha 20: |p0-q0| = 8 >= (20 >> 2) + 2, the weak filter: p0' = (200 + 100 + 108 + 2) >> 2.
    P = _rows([100, 100, 100, 100, 108, 108, 108, 108])
    dc.edge_luma_intra(P, 20, 6)
    assert P.tolist() == [[100, 100, 100, 102, 106, 108, 108, 108]]
    # alpha 40: 8 < 12, the strong filter on both sides; row 1 does not fire
    P = _rows([100, 100, 100, 100, 108, 108, 108, 108], [100, 100, 100, 100, 150, 150, 150, 150])
    dc.edge_luma_intra(P, 40, 6)
    assert P.tolist() == [[100, 101, 102, 103, 105, 106, 107, 108], [100, 100, 100, 100, 150, 150, 150, 150]]
    # strong on the p side only: |q2-q0| = 6 >= beta
    P = _rows([100, 100, 100, 100, 108, 110, 114, 114])
    dc.edge_luma_intra(P, 40, 6)
    assert P.tolist() == [[100, 101, 102, 103, (220 + 108 + 100 + 2) >> 2, 110, 114, 114]]


def test_edge_chroma_intra_by_hand():
    P = _rows([100, 100, 108, 108], [100, 100, 125, 125])
    dc.edge_chroma_intra(P, 20, 6)
    assert P.tolist() == [[100, 102, 106, 108], [100, 100, 125, 125]]


def test_deblock_edge_early_returns_and_tc():
    """deblock.c:315: no bS, alpha 0 or beta 0 leaves the lines alone; tc = tc0 * 2^(depth-8) + b_chroma"""
    base = _rows(*[[100, 100, 100, 100, 108, 108, 108, 108]] * 16)
    P = base.copy()
    dc.deblock_edge(P, [0, 0, 0, 0], 4, 40, 0, 0, 0, True, 8)
    assert np.array_equal(P, base)
    P = base.copy()
    dc.deblock_edge(P, [2, 2, 2, 2], 4, 15, 0, 0, 0, True, 8)                 # alpha_table(15) = 0
    assert np.array_equal(P, base)
    P = base.copy()
    dc.deblock_edge(P, [2, 0, 1, 3], 4, 40, 0, 0, 0, True, 8)                 # bS 0: tc0 -1, its 4 lines skipped
    assert not np.array_equal(P[0:4], base[0:4]) and np.array_equal(P[4:8], base[4:8])
    assert not np.array_equal(P[8:12], base[8:12]) and not np.array_equal(P[12:16], base[12:16])
    assert dc.alpha_beta(40, 0, 0, 8) == (int(dc.ALPHA[64]), int(dc.BETA[64]))
    assert dc.alpha_beta(52, -12, -12, 10) == (int(dc.ALPHA[64]) << 2, int(dc.BETA[64]) << 2)


# ------------------------------------------------------------------ the order, and the inputs
def _same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("key", dc.ALL, ids=dc.case_id)
def test_diagonal_order_equals_raster_order(key):
    assert _same(dc.deblock(dc.make_case(*key), "diag"), dc.expected(key))


@pytest.mark.parametrize("key", dc.ACTIVE, ids=dc.case_id)
def test_inputs_are_active_and_order_sensitive(key):
    c = dc.make_case(*key)
    want = dc.expected(key)
    changed = (want[0] != c.luma).mean()
    vh = (dc.deblock(c, "vh")[0] != want[0]).mean()
    print("changed %.3f, vertical-then-horizontal differs in %.4f" % (changed, vh))
    assert changed >= 0.25
    assert vh >= 0.01
    if c.cf:
        assert all((w != p).mean() >= 0.1 for w, p in zip(want[1], c.chroma))


def test_generator_reference_figures():
    """the issue's figures for the generator at 5x4 MBs, qp 40, seed 1, every bs 2"""
    c = dc.make_case(8, 1, 5, 4, 1, 1, (0, 0), 40, 40)
    c = dc.with_(c, bs=np.full_like(c.bs, 2), mb_flags=np.zeros_like(c.mb_flags))
    want = dc.deblock(c)
    assert (want[0] != c.luma).mean() >= 0.25 and (dc.deblock(c, "vh")[0] != want[0]).mean() >= 0.01


@pytest.mark.parametrize("key", dc.LOW_QP, ids=dc.case_id)
def test_low_qp_changes_nothing(key):
    c = dc.make_case(*key)
    assert _same(dc.expected(key), (c.luma, c.chroma))


def test_slices_leave_the_split_alone():
    """idc 2: the edges between the slices are not filtered, with NULL they are"""
    for key in dc.SLICES:
        c = dc.make_case(*key)
        with_t, without = dc.expected(key), dc.deblock(dc.with_(c, slice_table=None))
        assert not np.array_equal(with_t[0], without[0])


# ------------------------------------------------------------------ deblock_strength
def _strength_loop(s, mvy_limit):
    """the rule of include/x264hip_deblock.h, one pair of 4x4 blocks at a time"""
    out = np.zeros((s.nf, s.mbh, s.mbw, 2, 4, 4), np.uint8)
    fl = s.mb_flags.reshape(s.nf, s.mbh, s.mbw)
    nz = s.nz.reshape(s.nf, s.mbh, s.mbw)

    def coded(f, gx, gy):
        mx, my, bx, by = gx // 4, gy // 4, gx % 4, gy % 4
        i8 = (by // 2) * 2 + bx // 2
        bit = i8 if fl[f, my, mx] & 2 else 4 * i8 + (by % 2) * 2 + bx % 2
        return (int(nz[f, my, mx]) >> bit) & 1

    for f in range(s.nf):
        for gy in range(4 * s.mbh):
            for gx in range(4 * s.mbw):
                for dir in (0, 1):
                    px, py = (gx - 1, gy) if dir == 0 else (gx, gy - 1)
                    edge, i = (gx % 4, gy % 4) if dir == 0 else (gy % 4, gx % 4)
                    if px < 0 or py < 0:
                        v = 0
                    elif (fl[f, gy // 4, gx // 4] | fl[f, py // 4, px // 4]) & 1:
                        v = 4 if edge == 0 else 3
                    elif coded(f, gx, gy) or coded(f, px, py):
                        v = 2
                    else:
                        v = 0
                        for mv, ref in zip(s.mv, s.ref):
                            if ref[f, gy // 2, gx // 2] != ref[f, py // 2, px // 2] or \
                               abs(int(mv[f, gy, gx, 0]) - int(mv[f, py, px, 0])) >= 4 or \
                               abs(int(mv[f, gy, gx, 1]) - int(mv[f, py, px, 1])) >= mvy_limit:
                                v = 1
                    out[f, gy // 4, gx // 4, dir, edge, i] = v
    return out.reshape(-1, 2, 4, 4)


@pytest.mark.parametrize("bframe", [False, True])
@pytest.mark.parametrize("mvy_limit", [4, 2])
def test_strength_restatements_agree(bframe, mvy_limit):
    s = dc.make_strength_case(5, 4, 2, bframe)
    got = dc.deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf, mvy_limit)
    want = _strength_loop(s, mvy_limit)
    assert np.array_equal(got, want)
    # every value occurs, and the vector thresholds are straddled: differences of 3 and of 4
    assert set(np.unique(want)) == {0, 1, 2, 3, 4}
    d = np.abs(np.diff(s.mv[0][..., 0].astype(np.int64), axis=2))
    assert (d == 3).any() and (d == 4).any()
    dy = np.abs(np.diff(s.mv[0][..., 1].astype(np.int64), axis=1))
    assert (dy == mvy_limit - 1).any() and (dy == mvy_limit).any()
    other = dc.deblock_strength_py(s.nz, s.mb_flags, s.mv, s.ref, s.mbw, s.mbh, s.nf, 6 - mvy_limit)
    assert not np.array_equal(other, got)


# ------------------------------------------------------------------ the tables
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "deblock_tables.json")) as fh:
        return json.load(fh)


def test_tables_pinned():
    g = _golden()
    src = os.path.join(ROOT, "x264-i386pic_amd", "csrc", "deblock.hip")
    assert c_array(src, "c_alpha_table") == g["i_alpha_table"] and len(g["i_alpha_table"]) == 88
    assert c_array(src, "c_beta_table") == g["i_beta_table"] and len(g["i_beta_table"]) == 88
    assert c_array(src, "c_tc0_table") == g["i_tc0_table"] and len(g["i_tc0_table"]) == 88 * 4
    # what the standard's tables look like: non-decreasing, zero below index 16 + 24, the ends clamped
    for name in ("i_alpha_table", "i_beta_table"):
        t = g[name]
        assert t == sorted(t) and not any(t[:40]) and t[40] > 0 and len(set(t[75:])) == 1
    assert (g["i_alpha_table"][-1], g["i_beta_table"][-1]) == (255, 18)
    tc = np.array(g["i_tc0_table"]).reshape(88, 4)
    assert (tc[:, 0] == -1).all() and (np.diff(tc[:, 1:], axis=1) >= 0).all() and tc[-1].tolist() == [-1, 13, 17, 25]


def test_tables_equal_the_reference_text():
    ref = os.environ.get("X264_REFERENCE_DIR", "")
    if not os.path.exists(os.path.join(ref, "common", "deblock.c")):
        pytest.skip("X264_REFERENCE_DIR does not name the reference tree")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_deblock_tables
    assert make_deblock_tables.tables(ref) == _golden()


def test_chroma_qp_table():
    x = load_package()
    for bd in (8, 10):
        for off in (0, 4, -3):
            t = x.chroma_qp_table(bd, off)
            assert np.array_equal(t, dc.chroma_qp_table(bd, off)) and len(t) == 52 + 6 * (bd - 8)
    t = x.chroma_qp_table(8).tolist()
    assert t[:30] == list(range(30)) and t[30:34] == [29, 30, 31, 32] and t[51] == 39
    assert x.chroma_qp_table(10).tolist()[63] == 51


# ------------------------------------------------------------------ ABI
_SCALARS = {"intptr_t": ctypes.c_ssize_t, "int": ctypes.c_int}


def _prototypes():
    """{name: (return text, [parameter text])} of the functions x264hip_deblock.h itself declares"""
    inc = os.path.join(ROOT, "include")
    src = subprocess.run(["gcc", "-E", "-P", "-I", inc, HEADER], capture_output=True, text=True, check=True).stdout
    own = subprocess.run(["gcc", "-E", "-P", "-I", inc, os.path.join(inc, "x264hip.h")], capture_output=True, text=True,
                         check=True).stdout
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


def test_deblock_signatures_match_header():
    ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    names = sorted([f"x264hip_{bd}_{n}" for n in x._DEBLOCK for bd in (8, 10)] + [f"x264hip_{n}" for n in x._DEBLOCK_PLAIN])
    assert sorted(protos) == names == ["x264hip_10_deblock_frames", "x264hip_8_deblock_frames", "x264hip_deblock_strength"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret), name
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for i, (p, a) in enumerate(zip(params, fn.argtypes)):
            assert a is _ctype_of(p), (name, i, p, a)
        assert params[-1] == "void *stream"
    for n in ("deblock_strength", "deblock_frames", "Deblock", "DeblockStrength", "chroma_qp_table"):
        assert n in x.__all__ and callable(getattr(x, n))


def test_deblock_symbols_exported_and_header_stands_apart():
    so = ensure_built("hip")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(_prototypes()) <= exported
    assert "deblock" not in open(os.path.join(ROOT, "include", "x264hip.h")).read()
    text = open(HEADER).read()
    assert '#include "x264hip.h"' in text
    for word in ("mbaff", "effective_qp", "x264_macroblock_deblock", "x264_deblock_function_t", "no padding",
                 "not re-expanded"):
        assert word in text.lower(), word


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "x264hip_deblock.h"
#define P(F) printf(#F " %zu\n", offsetof(x264hip_deblock_t, F));
#define S(F) printf(#F " %zu\n", offsetof(x264hip_deblock_strength_t, F));
int main(void) {
    printf("size %zu\n", sizeof(x264hip_deblock_t));
    P(chroma_format) P(alpha_c0_offset) P(beta_offset) P(chroma_qp_index_offset) P(chroma_qp_table) P(luma)
    P(luma_stride) P(luma_frame_stride) P(chroma) P(chroma_stride) P(chroma_frame_stride) P(qp) P(mb_flags) P(bs)
    P(slice_table)
    printf("ssize %zu\n", sizeof(x264hip_deblock_strength_t));
    S(nz) S(mb_flags) S(mv) S(ref) S(bframe) S(mvy_limit)
    return 0;
}
"""


def test_deblock_layout_matches_ctypes(tmp_path):
    c = tmp_path / "probe.c"
    c.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    k = [n for n, _ in lines].index("ssize")
    vals, svals = dict(lines[:k]), dict(lines[k:])
    x = load_package()
    for S, v, key in ((x.Deblock, vals, "size"), (x.DeblockStrength, svals, "ssize")):
        assert int(v.pop(key)) == ctypes.sizeof(S)
        assert [n for n, _ in S._fields_] == list(v)
        for name, off in v.items():
            assert getattr(S, name).offset == int(off), name


V = ctypes.c_void_p
_TABLE = np.arange(64, dtype=np.uint8)


def _d(x, cf=1, **kw):
    """a valid x264hip_deblock_t on made-up addresses"""
    d = x.Deblock()
    d.chroma_format = cf
    d.chroma_qp_table = _TABLE.ctypes.data
    d.luma, d.luma_stride, d.luma_frame_stride = 0x40000000, 192, 192 * 128
    d.chroma[0], d.chroma[1] = 0x50000000, 0x60000000
    d.chroma_stride, d.chroma_frame_stride = 192, 192 * 128
    d.qp, d.mb_flags, d.bs = 0x70000000, 0x71000000, 0x72000000
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _s(x, **kw):
    s = x.DeblockStrength()
    s.nz, s.mb_flags = 0x70000000, 0x71000000
    s.mv[0], s.mv[1], s.ref[0], s.ref[1] = 0x73000000, 0x74000000, 0x75000000, 0x76000000
    s.bframe, s.mvy_limit = 1, 4
    for name, v in kw.items():
        setattr(s, name, v)
    return s


BS = V(0x72000000)
EINVAL, ENODEV = -1, -3


@pytest.mark.parametrize("bd", [8, 10])
def test_deblock_frames_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_deblock_frames")

    def call(d, mbw=5, mbh=4, n=2):
        return fn(ctypes.byref(d) if d is not None else None, mbw, mbh, n, None)

    assert call(None) == EINVAL
    for field in ("luma", "qp", "mb_flags", "bs", "chroma_qp_table"):
        assert call(_d(x, **{field: None})) == EINVAL, field
    for cf in (1, 2, 3):
        d = _d(x, cf=cf)
        d.chroma[0] = None
        assert call(d) == EINVAL, cf
    d = _d(x, cf=3)
    d.chroma[1] = None
    assert call(d) == EINVAL
    for off in (-13, 13):
        assert call(_d(x, alpha_c0_offset=off)) == EINVAL and call(_d(x, beta_offset=off)) == EINVAL
    assert call(_d(x), mbw=-1) == EINVAL and call(_d(x), mbh=-1) == EINVAL and call(_d(x), n=-1) == EINVAL
    assert call(_d(x, cf=-1)) == EINVAL and call(_d(x, cf=4)) == EINVAL
    assert call(_d(x), mbw=1 << 15, mbh=1 << 14, n=1) == EINVAL                       # more than 2^28 MBs
    # nothing to do is OK without a launch (and without a device), whatever the format; errors stay errors
    for cf in range(4):
        d = _d(x, cf=cf)
        if cf != 3:
            d.chroma[1] = None
        assert call(d, n=0) == 0 and call(d, mbw=0) == 0 and call(d, mbh=0) == 0
    assert call(_d(x, luma=None), n=0) == EINVAL and call(None, n=0) == EINVAL


def test_deblock_strength_argument_errors():
    ensure_built("hip")
    x = load_package()
    fn = x.lib().x264hip_deblock_strength

    def call(s, mbw=5, mbh=4, n=2, bs=BS):
        return fn(ctypes.byref(s) if s is not None else None, mbw, mbh, n, bs, None)

    assert call(None) == EINVAL and call(_s(x), bs=None) == EINVAL
    assert call(_s(x, nz=None)) == EINVAL and call(_s(x, mb_flags=None)) == EINVAL
    for arr, k in (("mv", 0), ("ref", 0), ("mv", 1), ("ref", 1)):
        s = _s(x)
        getattr(s, arr)[k] = None
        assert call(s) == EINVAL, (arr, k)
    assert call(_s(x, mvy_limit=0)) == EINVAL
    assert call(_s(x), mbw=-1) == EINVAL and call(_s(x), n=-1) == EINVAL
    s = _s(x, bframe=0)                                       # a P frame needs no list 1
    s.mv[1] = s.ref[1] = None
    assert call(s, n=0) == 0 and call(_s(x), mbh=0) == 0
    assert call(_s(x, nz=None), n=0) == EINVAL


def test_deblock_entries_return_enodev_without_device():
    """a valid call is X264HIP_ENODEV where no device exists (nothing is dereferenced on the host
    but the struct and the chroma qp table)"""
    ensure_built("hip")
    x = load_package()
    L = x.lib()
    if L.x264hip_available():
        pytest.skip("a gfx950 device is visible: the calls would run on these made-up addresses")
    for bd in (8, 10):
        for cf in range(4):
            assert getattr(L, f"x264hip_{bd}_deblock_frames")(ctypes.byref(_d(x, cf=cf)), 5, 4, 2, None) == ENODEV
    assert L.x264hip_deblock_strength(ctypes.byref(_s(x)), 5, 4, 2, BS, None) == ENODEV


# ------------------------------------------------------------------ the boundary pictures
@pytest.mark.parametrize("bd", [8, 10])
def test_boundary_pictures_alone_meet_every_line_filter_bound(bd):
    """at each depth the pictures of deblock_cases.BOUNDARY by themselves tell every alpha / beta /
    tc0 comparison of the four line filters, flipped at its boundary (tests/mutants.py), from the
    checker: each bound is met exactly, and the step either side of it is filtered differently"""
    import mutants as mu
    keys = [k for k in dc.boundary_keys() if k[0] == bd]
    assert keys and all(k[2] * k[3] * k[4] <= 40 for k in keys)
    filters = ("edge_luma", "edge_chroma", "edge_luma_intra", "edge_chroma_intra")
    sites = [s for s in mu.sites("deblock_cases") if s.func in filters and s.text != "tc > 0"]
    assert len(sites) == 18
    for s in sites:
        m = mu.load("deblock_cases", s.index)
        assert any(mu.differs(m.expected(k), dc.expected(k)) for k in keys), (bd, s.func, s.text)


def test_boundary_fields_meet_the_vector_limits():
    import mutants as mu
    for s in mu.sites("deblock_cases"):
        if s.func == "deblock_strength_py":
            m = mu.load("deblock_cases", s.index)
            entries = dc.gpu_keys("boundary")
            assert any(e[0] == "strength" and mu.differs(m.gpu_expected(e), dc.gpu_expected(e)) for e in entries), s.text


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised lists of tests/test_gpu_deblock.py add up to gpu_keys(), nothing twice"""
    picked = [e for g in dc.GPU_GROUPS for e in dc.gpu_keys(g)]
    assert picked == dc.gpu_keys() and len(set(picked)) == len(picked)
    assert {e[1] for e in dc.gpu_keys() if e[0] == "frames"} >= set(dc.ALL)
