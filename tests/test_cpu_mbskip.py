"""CPU: the checkers of P_SKIP / B_SKIP (tests/mbskip_cases.py) held to independent evidence, and
the host side of include/x264hip_mbskip.h's three entries.  No GPU.

* x264_lambda2_tab: the kernel source's host copy equals tests/golden/mbenc_tables.json.
* The skip vector: the table form agrees with a literal scan8-cache restatement on random fields,
  and on all-16x16 ref-0 fields with the zero rule plus mvpred_cases.predict_mv_16x16; hand-made
  fields pin each rule.
* The probe: the literal checker (early returns, a counter per branch) agrees on every case with
  the order-free predicate form on tests/numpy_ref.py's matrix transforms; the case lists reach
  every branch, and between 20 % and 80 % of the macroblocks of every larger case probe as skip.
* The conversion: each clause failing alone.
* The header's prototypes, the ctypes declarations, the exported symbols and the struct layout
  agree; every X264HIP_EINVAL case; the wrappers' refusals."""
import collections
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mbskip_cases as ms
import mvpred_cases as mvp
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mbskip.h")
LISTS = [(bd, cf, leg) for bd in (8, 10) for cf in (0, 1, 2, 3) for leg in ms.LEGS]
LUMA = ("luma_fail", "luma_pass_levels")
CHROMA = ("chroma_ssd_lt_thresh", "chroma_dc_nonzero", "chroma_ssd_lt_4thresh", "chroma_ac_fail", "chroma_ac_pass")


# ------------------------------------------------------------------ 1. the table
def test_lambda2_table_pinned():
    src = open(os.path.join(ROOT, "x264-i386pic_amd", "csrc", "mbskip.hip")).read()
    m = re.search(r"k_lambda2_tab\[82\]\s*=\s*\{([^}]*)\}", src)
    assert m
    with open(os.path.join(ROOT, "tests", "golden", "mbenc_tables.json")) as fh:
        want = json.load(fh)["x264_lambda2_tab"]
    assert [int(v) for v in re.findall(r"\d+", m.group(1))] == want == list(ms.LAMBDA2)
    # the thresholds live here, not in the inter encode's source
    assert "mbskip" not in open(os.path.join(ROOT, "x264-i386pic_amd", "csrc", "mbenc.hip")).read()
    assert ms.thresh_of(1, 30) == (14745 + 32) >> 6 and ms.thresh_of(2, 30) == (14745 + 16) >> 5


# ------------------------------------------------------------------ 2. the skip vector
@pytest.mark.parametrize("shape", ms.SHAPES)
def test_pskip_agrees_with_the_scan8_cache(shape):
    mbw, mbh, nf = shape
    for seed in range(3 if mbw < 24 else 1):
        mv0, ref0 = ms.make_field(mbw, mbh, nf, seed)
        got = ms.pskip_mv(mv0, ref0, mbw, mbh)
        assert np.array_equal(got, ms.pskip_mv_scan8(mv0, ref0, mbw, mbh)), (shape, seed)
    if mbw * mbh >= 20:
        assert got.any() and (got == 0).all(axis=1).any()
        assert (ref0 == -1).any() and (ref0 == 2).any()


@pytest.mark.parametrize("shape", [(3, 1, 1), (2, 2, 1), (5, 4, 2), (24, 14, 2)])
def test_pskip_on_p16x16_fields_is_the_zero_rule_plus_the_16x16_predictor(shape):
    mbw, mbh, nf = shape
    mv0, ref0 = ms.make_field(mbw, mbh, nf, 5, kind="p16")
    got = ms.pskip_mv(mv0, ref0, mbw, mbh)
    used = 0
    for f in range(nf):
        field = {(y, x): tuple(int(v) for v in mv0[f, 4 * y, 4 * x]) for y in range(mbh) for x in range(mbw)}
        for y in range(mbh):
            for x in range(mbw):
                if x == 0 or y == 0 or field[(y, x - 1)] == (0, 0) or field[(y - 1, x)] == (0, 0):
                    want = (0, 0)
                else:
                    want = tuple(mvp.predict_mv_16x16(field, x, y, mbw))
                    used += 1
                assert tuple(got[(f * mbh + y) * mbw + x]) == want, (f, y, x)
    assert used or mbw * mbh < 20


def _field(mbw, mbh, mbs):
    """a field from {(y, x): (ref, (mvx, mvy))}, the rest intra"""
    mv0 = np.zeros((1, 4 * mbh, 4 * mbw, 2), np.int16)
    ref0 = np.full((1, 2 * mbh, 2 * mbw), -1, np.int8)
    for (y, x), (r, v) in mbs.items():
        ref0[0, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = r
        mv0[0, 4 * y:4 * y + 4, 4 * x:4 * x + 4] = v
    return mv0, ref0


def _at(mv0, ref0, mbw, mbh, y, x):
    a, b = ms.pskip_mv(mv0, ref0, mbw, mbh), ms.pskip_mv_scan8(mv0, ref0, mbw, mbh)
    assert np.array_equal(a, b)
    return tuple(int(v) for v in a[y * mbw + x])


def test_pskip_rules_by_hand():
    A_, B_, C_, D_ = (1, 0), (0, 1), (0, 2), (0, 0)               # left, top, top right, top left of (1, 1)
    full = {A_: (0, (8, -4)), B_: (0, (20, 12)), C_: (0, (-6, 2)), D_: (0, (100, 100))}
    # three matching refs: the median, component by component
    assert _at(*_field(3, 2, full), 3, 2, 1, 1) == (8, 2)
    # no left (x = 0), no top (y = 0)
    assert _at(*_field(3, 2, full), 3, 2, 1, 0) == (0, 0)
    assert _at(*_field(3, 2, full), 3, 2, 0, 1) == (0, 0)
    # a zero-mv ref-0 left / top; a zero mv with another ref does not count
    assert _at(*_field(3, 2, {**full, A_: (0, (0, 0))}), 3, 2, 1, 1) == (0, 0)
    assert _at(*_field(3, 2, {**full, B_: (0, (0, 0))}), 3, 2, 1, 1) == (0, 0)
    assert _at(*_field(3, 2, {**full, A_: (1, (0, 0))}), 3, 2, 1, 1) == (0, 2)
    # an intra neighbour (ref -1, mv 0) is available and matches nothing: two matching refs, the median with its 0
    assert _at(*_field(3, 2, {B_: full[B_], C_: full[C_]}), 3, 2, 1, 1) == (0, 2)
    # exactly one matching ref: that neighbour's mv
    assert _at(*_field(3, 2, {**full, B_: (1, (20, 12)), C_: (2, (-6, 2))}), 3, 2, 1, 1) == (8, -4)
    assert _at(*_field(3, 2, {**full, A_: (1, (8, -4)), C_: (2, (-6, 2))}), 3, 2, 1, 1) == (20, 12)
    assert _at(*_field(3, 2, {**full, A_: (1, (8, -4)), B_: (2, (20, 12))}), 3, 2, 1, 1) == (-6, 2)
    # none: the median of all three
    assert _at(*_field(3, 2, {A_: (1, (8, -4)), B_: (2, (20, 12)), C_: (1, (-6, 2))}), 3, 2, 1, 1) == (8, 2)
    # the right column: the top-left macroblock stands in for the top-right one
    two = {(1, 0): (0, (8, -4)), (0, 1): (0, (20, 12)), (0, 0): (0, (100, 100))}
    assert _at(*_field(2, 2, two), 2, 2, 1, 1) == (20, 12)
    assert _at(*_field(2, 2, {**two, (0, 0): (1, (100, 100)), (0, 1): (2, (20, 12))}), 2, 2, 1, 1) == (8, -4)
    # partitions: a reads the top-right 4x4 of the left macroblock, b the bottom-left of the top one, c the
    # bottom-left of the top-right one
    mv0, ref0 = _field(3, 2, full)
    mv0[0, 4, 3], mv0[0, 3, 4], mv0[0, 3, 8] = (1, 1), (2, 2), (3, 3)
    assert _at(mv0, ref0, 3, 2, 1, 1) == (2, 2)
    # nothing is read across a frame boundary: frame 1's first row has no top
    mv0, ref0 = ms.make_field(5, 4, 2, 3, kind="p16")
    assert not ms.pskip_mv(mv0, ref0, 5, 4)[20:25].any()


# ------------------------------------------------------------------ 3. the probe
@pytest.mark.parametrize("bd,cf,leg", LISTS)
def test_literal_and_predicate_forms_agree_and_the_lists_reach_every_branch(bd, cf, leg):
    cnt = collections.Counter()
    for key in ms.case_keys(bd, cf, leg):
        case = ms.make_case(*key)
        skip, c = ms.expected(key)
        cnt.update(c)
        assert np.array_equal(skip, ms.probe_by_predicate(case)), key
        if case.nmb >= 40:
            assert 0.2 <= skip.mean() <= 0.8, (key, skip.mean())
    # the chroma branches exist at 4:2:0 and 4:2:2 only
    for b in LUMA + (CHROMA if cf in (1, 2) else ()):
        assert cnt[b] > 0, b


def test_cases_clip_their_corner_vectors_and_mix_everything():
    case = ms.make_case(8, 1, 5, 4, 2, "p")
    mvx, mvy = ms.clip_mv(case.pskip_mv, case.mbw, case.mbh, case.nframes)
    changed = (mvx != case.pskip_mv[:, 0]) | (mvy != case.pskip_mv[:, 1])
    corners = [f * 20 + m for f in range(2) for m in (0, 4, 15, 19)]
    assert changed[corners].all()
    assert (mvx[[4, 19]] < case.pskip_mv[[4, 19], 0]).all() and (case.pskip_mv[[0, 15], 0] < mvx[[0, 15]]).all()
    assert (mvy[[15, 19]] < case.pskip_mv[[15, 19], 1]).all() and (case.pskip_mv[[0, 4], 1] < mvy[[0, 4]]).all()
    big = ms.make_case(10, 2, 24, 14, 2, "pw")
    assert big.qp.min() == 0 and big.qp.max() == 63 and set(np.unique(big.klass)) == set(range(10))
    assert (big.pskip_mv == 0).all(axis=1).any() and (big.pskip_mv[:, 0] & 3).any() and (big.pskip_mv[:, 1] & 7).any()
    chk = big.klass == ms.CHECKER
    assert set(np.unique(big.qp[chk])) == {0, 63}
    # full scale: the checker against its weighted inverse
    d = big.blocks.fenc[0][chk].astype(np.int64) - big.blocks.pred[0][chk]
    assert np.abs(d).max() >= 900
    assert ms.make_case(8, 1, 5, 4, 2, "p", "jvt").cqm == "jvt"
    # the legs differ in what they are given
    assert big.weights == ms.WEIGHTS and case.weights == (None, None, None)


# ------------------------------------------------------------------ 4. the conversion
def test_skip_convert_each_clause_alone():
    mv0, ref0 = _field(2, 1, {(0, 0): (0, (0, 0)), (0, 1): (0, (0, 0))})
    ps = ms.pskip_mv(mv0, ref0, 2, 1)
    assert not ps.any()

    def conv(fl=ms.D16, cbp=0, mv=(0, 0), ref=0, bframe=0, direct=0):
        m, r = mv0.copy(), ref0.copy()
        m[0, 0, 4], r[0, 0, 2] = mv, ref
        out = ms.skip_convert(np.array([0, fl], np.uint8), np.array([0, cbp], np.int32), m, r, ps, bframe,
                              np.array([0, direct], np.uint8), 2, 1)
        assert int(out[1]) & ~ms.SKIP == fl & ~ms.SKIP and out[0] == 0
        return bool(out[1] & ms.SKIP) and not fl & ms.SKIP
    assert conv() and conv(fl=ms.D16 | ms.T8) and conv(cbp=0x600)
    for kw in (dict(fl=ms.D16 | ms.INTRA), dict(fl=ms.D16 | ms.SKIP), dict(fl=0), dict(cbp=1), dict(cbp=0x10), dict(cbp=0x20),
               dict(mv=(1, 0)), dict(mv=(0, -1)), dict(ref=1)):
        assert not conv(**kw), kw
    # only the macroblock's first 4x4 and 8x8 are compared (x264_scan8[0])
    m = mv0.copy()
    m[0, 1, 5] = (9, 9)
    assert ms.skip_convert(np.array([0, ms.D16], np.uint8), np.zeros(2, np.int32), m, ref0, ps, 0, None, 2, 1)[1] & ms.SKIP
    # B: direct, not intra, nothing coded; the partition, the vector and the reference do not matter
    assert conv(fl=0, bframe=1, direct=7, mv=(3, 3), ref=1)
    for kw in (dict(direct=0), dict(direct=1, fl=ms.INTRA), dict(direct=1, cbp=4), dict(direct=1, cbp=0x10)):
        assert not conv(bframe=1, **{"fl": 0, **kw}), kw


@pytest.mark.parametrize("bframe", [0, 1])
def test_convert_cases_convert_some(bframe):
    c = ms.make_convert_case(5, 4, 2, bframe)
    out = ms.skip_convert(c.flags, c.cbp, c.mv0, c.ref0, c.pskip, bframe, c.direct, 5, 4)
    new = (out & ms.SKIP != 0) & (c.flags & ms.SKIP == 0)
    assert 3 <= new.sum() <= c.nmb - 3 and np.array_equal(out & (255 - ms.SKIP), c.flags & (255 - ms.SKIP))
    assert (c.flags & ms.INTRA).any() and (c.flags & ms.SKIP).any() and c.pskip.any()


# ------------------------------------------------------------------ 5. the host side
_SCALARS = {"int": ctypes.c_int, "intptr_t": ctypes.c_ssize_t}


def _prototypes():
    inc = os.path.join(ROOT, "include")

    def names(path):
        return subprocess.run(["gcc", "-E", "-P", "-I", inc, path], capture_output=True, text=True, check=True).stdout
    known = set()
    for h in ("x264hip.h", "x264hip_mbenc.h", "x264hip_mc.h"):
        known |= set(re.findall(r"\b(x264hip_\w+)\s*\(", names(os.path.join(inc, h))))
    protos = {}
    for decl in " ".join(names(HEADER).split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1) and m.group(2) not in known:
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text:
        return ctypes.c_void_p
    return _SCALARS[[w for w in text.split() if w != "const"][0]]


def test_mbskip_signatures_symbols_and_header():
    so = ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    names = [f"x264hip_{bd}_{n}" for n in x._MBSKIP for bd in (8, 10)] + [f"x264hip_{n}" for n in x._MBSKIP_PLAIN]
    assert sorted(protos) == sorted(names) == ["x264hip_10_mb_probe_skip", "x264hip_8_mb_probe_skip",
                                               "x264hip_mb_predict_mv_pskip", "x264hip_mb_skip_convert"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret) and len(fn.argtypes) == len(params), name
        for p, a in zip(params, fn.argtypes):
            assert a is _ctype_of(p), (name, p, a)
        assert params[-1] == "void *stream"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(protos) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in ("mb_predict_mv_pskip", "mb_probe_skip", "mb_skip_convert", "MbSkip"):
        assert n in x.__all__ and callable(getattr(x, n))
    # tables of their own: the footprint and stream walks are keyed on the others
    for n in list(x._MBSKIP) + list(x._MBSKIP_PLAIN):
        assert all(n not in t for t in (x._PER_DEPTH, x._PLAIN, x._MC, x._MBTREE))
    text = open(HEADER).read()
    assert '#include "x264hip_mbenc.h"' in text and '#include "x264hip_mc.h"' in text
    for word in ("mvpred.c:166-181", "macroblock.c:985-1139", "macroblock.c:953-971", "analyse.c:1294-1307, 3002-3013",
                 "direct vectors", "noise reduction", "several slices", "MBAFF", "frame-thread limit", "b_skip_mc",
                 "order in which they fire"):
        assert word in text, word
    inc = os.path.join(ROOT, "include")
    assert "x264hip_mbskip.h" in open(os.path.join(inc, "x264hip_mbenc.h")).read()
    assert "x264hip_mbskip.h" in open(os.path.join(inc, "x264hip_mc.h")).read()


def test_mbskip_layout_matches_ctypes(tmp_path):
    x = load_package()
    names = [n for n, _ in x.MbSkip._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "x264hip_mbskip.h"\nint main(void) {\n'
    src += '    printf("size %zu\\n", sizeof(x264hip_mbskip_t));\n'
    for n in names:
        src += f'    printf("{n} %zu\\n", offsetof(x264hip_mbskip_t, {n}));\n'
    src += "    return 0;\n}\n"
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(vals.pop("size")) == ctypes.sizeof(x.MbSkip)
    for n in names:
        assert getattr(x.MbSkip, n).offset == int(vals[n]), n
    assert x.MbSkip.skip.offset + 8 == ctypes.sizeof(x.MbSkip)


_TABLE = np.minimum(np.arange(64), 39).astype(np.uint8)
EINVAL, ENODEV = -1, -3
ADDR = 0x40000000


def _s(x, cf=1, bidir=0, **kw):
    """a valid x264hip_mbskip_t on made-up addresses"""
    s = x.MbSkip()
    s.chroma_format, s.b_bidir = cf, bidir
    s.chroma_qp_table = _TABLE.ctypes.data
    k = 0
    for n in ("quant4_mf", "quant4_bias", "fenc", "pskip_mv", "pred", "qp", "skip"):
        setattr(s, n, ADDR + 0x1000000 * k)
        k += 1
    for arr in (s.fenc_chroma, s.pred_chroma, s.ref.luma, s.ref.chroma):
        for i in range(len(arr)):
            arr[i] = ADDR + 0x1000000 * k
            k += 1
    for n, _ in x.MbSkip._fields_:
        if n.endswith("_frame_stride"):
            setattr(s, n, 192 * 128)
        elif n.endswith("_stride"):
            setattr(s, n, 192)
    for name, v in kw.items():
        setattr(s, name, v)
    return s


@pytest.mark.parametrize("bd", [8, 10])
def test_mb_probe_skip_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_probe_skip")

    def call(s, mbw=5, mbh=4, n=2):
        return fn(ctypes.byref(s) if s is not None else None, mbw, mbh, n, None)

    def without(arr_name, i, **kw):
        s = _s(x, **kw)
        arr = s.ref.luma if arr_name == "luma" else s.ref.chroma if arr_name == "chroma" else getattr(s, arr_name)
        arr[i] = None
        return s
    assert call(None) == EINVAL
    for bidir in (0, 1):
        for field in ("chroma_qp_table", "quant4_mf", "quant4_bias", "fenc", "qp", "skip"):
            assert call(_s(x, bidir=bidir, **{field: None})) == EINVAL, field
        assert call(_s(x, cf=-1, bidir=bidir)) == EINVAL and call(_s(x, cf=4, bidir=bidir)) == EINVAL
        for cf in (1, 2, 3):
            assert call(without("fenc_chroma", 0, cf=cf, bidir=bidir)) == EINVAL
        assert call(without("fenc_chroma", 1, cf=3, bidir=bidir)) == EINVAL
        assert call(_s(x, bidir=bidir), mbw=-1) == EINVAL and call(_s(x, bidir=bidir), mbh=-1) == EINVAL
        assert call(_s(x, bidir=bidir), n=-1) == EINVAL
        assert call(_s(x, bidir=bidir), mbw=1 << 15, mbh=1 << 14, n=1) == EINVAL         # more than 2^28 MBs
        bad = _TABLE.copy()
        bad[7] = 52 + 6 * (bd - 8)
        assert call(_s(x, bidir=bidir, chroma_qp_table=bad.ctypes.data)) == EINVAL
        bad[7] = 51 + 6 * (bd - 8) - 2                             # in range at 4:2:0, past the tables at 4:2:2
        assert call(_s(x, cf=2, bidir=bidir, chroma_qp_table=bad.ctypes.data)) == EINVAL
    # the P leg's own
    assert call(_s(x, pskip_mv=None)) == EINVAL and call(_s(x, pskip_mv=ADDR + 2)) == EINVAL
    for k in range(4):
        assert call(without("luma", k)) == EINVAL
    assert call(without("chroma", 0, cf=1)) == EINVAL and call(without("chroma", 0, cf=2)) == EINVAL
    for k in range(8):
        assert call(without("chroma", k, cf=3)) == EINVAL
    for plane in range(3):
        for denom in (-1, 8):
            s = _s(x)
            s.weight[plane] = x.Weight(1, 64, denom, 0)
            assert call(s) == EINVAL, (plane, denom)
    px = 1 if bd == 8 else 2
    s = _s(x)
    s.ref.chroma[0] = ADDR + px
    assert call(s) == EINVAL and call(_s(x, ref_chroma_stride=191)) == EINVAL
    assert call(_s(x, ref_chroma_frame_stride=191)) == EINVAL
    # the B leg's own; each leg ignores the other's fields
    assert call(_s(x, bidir=1, pred=None)) == EINVAL
    for cf in (1, 2, 3):
        assert call(without("pred_chroma", 0, cf=cf, bidir=1)) == EINVAL
    assert call(without("pred_chroma", 1, cf=3, bidir=1)) == EINVAL
    # nothing to do is OK without a launch (and without a device); errors stay errors
    for cf in range(4):
        p, b = _s(x, cf=cf, pred=None), _s(x, cf=cf, bidir=1, pskip_mv=None)
        p.pred_chroma[0] = p.pred_chroma[1] = None
        for k in range(4):
            b.ref.luma[k] = None
        for k in range(8):
            b.ref.chroma[k] = None
        b.weight[0] = x.Weight(1, 64, 9, 0)
        for s in (p, b):
            assert call(s, n=0) == 0 and call(s, mbw=0) == 0 and call(s, mbh=0) == 0
    assert call(_s(x, fenc=None), n=0) == EINVAL and call(None, n=0) == EINVAL
    if not x.lib().x264hip_available():
        assert call(_s(x)) == ENODEV and call(_s(x, bidir=1)) == ENODEV


def test_pskip_and_convert_argument_errors():
    ensure_built("hip")
    x = load_package()
    L = x.lib()
    a = [ADDR + 0x1000000 * k for k in range(8)]

    def pskip(mv0=a[0], ref0=a[1], mbw=5, mbh=4, n=2, out=a[2]):
        return L.x264hip_mb_predict_mv_pskip(mv0, ref0, mbw, mbh, n, out, None)
    for kw in (dict(mv0=None), dict(ref0=None), dict(out=None), dict(mbw=-1), dict(mbh=-1), dict(n=-1),
               dict(mbw=1 << 15, mbh=1 << 14, n=1), dict(mv0=a[0] + 2), dict(out=a[2] + 2)):
        assert pskip(**kw) == EINVAL, kw
    assert pskip(n=0) == 0 and pskip(mbw=0) == 0 and pskip(mbh=0) == 0 and pskip(mv0=None, n=0) == EINVAL

    def conv(fl=a[0], cbp=a[1], mv0=a[2], ref0=a[3], ps=a[4], bframe=0, direct=None, mbw=5, mbh=4, n=2, out=a[6]):
        return L.x264hip_mb_skip_convert(fl, cbp, mv0, ref0, ps, bframe, direct, mbw, mbh, n, out, None)
    for kw in (dict(fl=None), dict(cbp=None), dict(out=None), dict(mv0=None), dict(ref0=None), dict(ps=None),
               dict(bframe=1), dict(mbw=-1), dict(mbh=-1), dict(n=-1), dict(mbw=1 << 15, mbh=1 << 14, n=1),
               dict(cbp=a[1] + 2), dict(ps=a[4] + 2)):
        assert conv(**kw) == EINVAL, kw
    assert conv(n=0) == 0 and conv(bframe=1, direct=a[5], mv0=None, ref0=None, ps=None, mbw=0) == 0
    assert conv(out=a[0], n=0) == 0                               # flags may be mb_flags
    if not L.x264hip_available():
        assert pskip() == ENODEV and conv() == ENODEV and conv(bframe=1, direct=a[5]) == ENODEV


def test_wrapper_refusals_need_no_device():
    import torch
    x = load_package()
    y = torch.zeros((1, 16, 16), dtype=torch.uint8)
    plane = (y, 0, 16, 256)
    q = (torch.zeros(1, dtype=torch.int16), torch.zeros(1, dtype=torch.int16))
    qp, sk = torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.uint8)
    mv, ps = torch.zeros(32, dtype=torch.int16), torch.zeros(2, dtype=torch.int16)
    ok = dict(fenc=plane, mb_width=1, mb_height=1, nframes=1, qp=qp, quant4=q)
    with pytest.raises(ValueError, match="chroma_format"):
        x.mb_probe_skip(**ok, chroma_format=4, pred=plane)
    with pytest.raises(ValueError, match="fenc_chroma"):
        x.mb_probe_skip(**ok, chroma_format=1, pred=plane)
    with pytest.raises(ValueError, match="ref_chroma"):
        x.mb_probe_skip(**ok, chroma_format=1, fenc_chroma=plane, ref=([y] * 4, 0, 16), pskip_mv=ps)
    with pytest.raises(ValueError, match="needs ref and pskip_mv"):
        x.mb_probe_skip(**ok)
    with pytest.raises(ValueError, match="negative"):
        x.mb_probe_skip(**{**ok, "nframes": -1}, pred=plane)
    with pytest.raises(ValueError, match="QP_MAX_SPEC"):
        x.mb_probe_skip(**ok, pred=plane, qp_table=np.zeros(51, np.uint8))
    with pytest.raises(ValueError, match="qp must be"):
        x.mb_probe_skip(**{**ok, "mb_width": 2}, pred=plane)
    with pytest.raises(ValueError, match="skip must be"):
        x.mb_probe_skip(**ok, pred=plane, skip=torch.zeros(1, dtype=torch.int8))
    with pytest.raises(ValueError, match="mv0 must be"):
        x.mb_predict_mv_pskip(mv[:8], torch.zeros(4, dtype=torch.int8), 1, 1)
    with pytest.raises(ValueError, match="ref0 must be"):
        x.mb_predict_mv_pskip(mv, torch.zeros(4, dtype=torch.uint8), 1, 1)
    with pytest.raises(ValueError, match="needs direct"):
        x.mb_skip_convert(sk, torch.zeros(1, dtype=torch.int32), 1, 1, b_bframe=True)
    with pytest.raises(ValueError, match="needs mv0"):
        x.mb_skip_convert(sk, torch.zeros(1, dtype=torch.int32), 1, 1)
    with pytest.raises(ValueError, match="cbp must be"):
        x.mb_skip_convert(sk, torch.zeros(1, dtype=torch.int16), 1, 1, b_bframe=True, direct=sk)


# ------------------------------------------------------------------ the boundary macroblocks
@pytest.mark.parametrize("bd", [8, 10])
def test_boundary_macroblocks_meet_the_probe_thresholds(bd):
    """at each depth the pictures of mbskip_cases.BOUNDARY by themselves tell the luma bound 6, the
    chroma AC bound 7 and `ssd < thresh` (at 4:2:0 and at 4:2:2), flipped at their boundary
    (tests/mutants.py), from the checker; and the macroblock next to the luma one skips at 3"""
    import mutants as mu
    keys = [k for k in ms.boundary_keys() if k[0] == bd]
    for text, cfs in (("i_decimate_mb >= 6", (0, 1, 2)), ("i_decimate_mb >= 7", (1, 2)), ("ssd < thresh", (1, 2))):
        (site,) = [s for s in mu.sites("mbskip_cases") if s.func == "probe_literal" and s.text == text]
        m = mu.load("mbskip_cases", site.index)
        for cf in cfs:
            mine = [k for k in keys if k[1] == cf]
            assert any(not np.array_equal(m.expected(k)[0], ms.expected(k)[0]) for k in mine), (bd, text, cf)
    for k in keys:
        if k[6] == "flat":
            assert ms.expected(k)[0][:2].tolist() == [1, 0], k


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised selections of tests/test_gpu_mbskip.py add up to gpu_keys(), nothing twice"""
    picked = [e for sh in ms.SHAPES for e in ms.gpu_keys("pskip", shape=sh)]
    picked += [e for bd in (8, 10) for cf in (0, 1, 2, 3) for leg in ms.LEGS for e in ms.gpu_keys("probe", bd=bd, cf=cf, leg=leg)]
    picked += [e for bf in (0, 1) for e in ms.gpu_keys("convert", bframe=bf)] + ms.gpu_keys("boundary")
    assert sorted(map(repr, picked)) == sorted(map(repr, ms.gpu_keys())) and len(set(picked)) == len(picked)
