"""CPU: the checker of the inter macroblock encode (tests/mbenc_cases.py) held to independent
evidence, and the host side of x264hip_*_mb_encode_inter.  No GPU.

* x264_lambda2_tab: the kernel source's copy and the checker's equal tests/golden/mbenc_tables.json.
* Luma anchor: without decimation and chroma the checker's reconstruction and nz equal the
  oracle's mb_dct_quant -> mb_dequant_idct_add chain.
* The five restated static inlines of encoder/macroblock.c:35-96 on hand-worked vectors.
* Decoder agreement: the reconstruction rebuilt from level / chroma_dc alone equals recon.
* Coverage: conditions on the inputs, asserted from the checker's branch counters over exactly
  the case lists tests/test_gpu_mbenc.py runs.
* include/x264hip_mbenc.h's prototypes, the ctypes declarations, the exported symbols and the
  struct layout agree; every X264HIP_EINVAL case; the wrapper's refusals."""
import collections
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import mbenc_cases as mc
import oracle_lib as orc
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mbenc.h")
LISTS = [(bd, cf) for bd in (8, 10) for cf in (0, 1, 2)]


# ------------------------------------------------------------------ 1. the table
def test_lambda2_table_pinned():
    src = open(os.path.join(ROOT, "x264-i386pic_amd", "csrc", "mbenc.hip")).read()
    m = re.search(r"c_lambda2_tab\[82\]\s*=\s*\{([^}]*)\}", src)
    assert m
    kernel = [int(v) for v in re.findall(r"\d+", m.group(1))]
    import json
    with open(os.path.join(ROOT, "tests", "golden", "mbenc_tables.json")) as fh:
        want = json.load(fh)["x264_lambda2_tab"]
    assert len(want) == 82 and kernel == want and list(mc.LAMBDA2) == want
    assert want[0] == 14 and want[18] == 921 and want[81] == 134217727


# ------------------------------------------------------------------ 2. the luma anchor
def _uniform(case, qp, flags):
    c = types.SimpleNamespace(**vars(case))
    c.qp = np.full(case.nmb, qp, np.int8)
    c.flags = np.full(case.nmb, flags, np.uint8)
    return c


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("transform", [4, 8])
@pytest.mark.parametrize("qp", [5, 26, 44])
def test_luma_equals_the_two_launch_chain(bd, transform, qp):
    """b_dct_decimate = 0, chroma_format = 0: macroblock.c:806-919 is mb_dct_quant followed by
    mb_dequant_idct_add, which the oracle has as two frame-level entries of their own"""
    case = _uniform(mc.make_case(bd, 0, 5, 4, 2), qp, mc.T8 if transform == 8 else 0)
    got = mc.encode(case, 0)
    T = mc.tables(bd)
    mf, bias = (T.q8m, T.q8b) if transform == 8 else (T.q4m, T.q4b)
    dmf = T.dq8[mc.CQM_8PY] if transform == 8 else T.dq4[mc.CQM_4PY]
    W = 16 * case.mbw
    per = case.mbw * case.mbh
    for f in range(case.nframes):
        fenc, pred = case.fenc_y[f].reshape(-1).copy(), case.pred_y[f].reshape(-1).copy()
        dct, nz = orc.mb_dct_quant(bd, transform, fenc, 0, W, pred, 0, W, case.mbw, case.mbh, mf[1][qp], bias[1][qp])
        recon = np.zeros_like(pred)
        orc.mb_dequant_idct_add(bd, transform, dct, case.mbw, case.mbh, dmf, np.full(per, qp, np.int32), pred, 0, W,
                                recon, 0, W)
        assert np.array_equal(recon.reshape(case.pred_y[f].shape), got.recon_y[f])
        assert np.array_equal(nz, got.nz[f * per:(f + 1) * per])
    assert got.nz.any() and (got.recon_y != case.pred_y).any()


# ------------------------------------------------------------------ 3. the restated inlines
def test_zigzag_dc_by_hand():
    assert mc.zigzag_scan_2x2_dc([10, 11, 12, 13]) == [10, 12, 11, 13]
    assert mc.zigzag_scan_2x4_dc([0, 1, 2, 3, 4, 5, 6, 7]) == [0, 2, 1, 4, 6, 3, 5, 7]


def test_dct2x2dc_by_hand():
    d4 = np.zeros((4, 16), np.int16)
    d4[:, 0] = [1, 2, 3, 4]
    d4[:, 1] = 9
    d = np.zeros(4, np.int16)
    mc.dct2x2dc(8, d, d4)
    # d0 = 1+2, d1 = 3+4, d2 = 1-2, d3 = 3-4: (d0+d1, d0-d1, d2+d3, d2-d3)
    assert d.tolist() == [10, -4, -2, 0]
    assert not d4[:, 0].any() and (d4[:, 1] == 9).all()


def test_idct_dequant_2x2_by_hand():
    dmf = np.zeros((6, 16), np.int32)
    dmf[:, 0] = [160, 176, 208, 224, 256, 288]
    # qp 13: dmf = 176 << 2 = 704; dct (3, -1, 2, 0): d0 = 2, d1 = 2, d2 = 4, d3 = 2
    want = [(4 * 704) >> 5, 0, (6 * 704) >> 5, (2 * 704) >> 5]
    dct = np.array([3, -1, 2, 0, 77, 77, 77, 77], np.int16)
    mc.idct_dequant_2x2_dconly(8, dct, dmf, 13)
    assert dct.tolist() == want + [77] * 4
    d4 = np.full((4, 16), 5, np.int16)
    mc.idct_dequant_2x2_dc(8, [3, -1, 2, 0], d4, dmf, 13)
    assert d4[:, 0].tolist() == want and (d4[:, 1:] == 5).all()
    # a negative product shifts arithmetically; the store wraps to int16 at 8 bit
    mc.idct_dequant_2x2_dc(8, [-1, 0, 0, 0], d4, dmf, 0)
    assert d4[:, 0].tolist() == [-160 >> 5] * 4
    mc.idct_dequant_2x2_dc(8, [1000, 0, 0, 0], d4, dmf, 47)       # 1000 * (288 << 7) >> 5 = 1152000
    assert d4[0, 0] == np.array(1152000).astype(np.int16)
    d32 = np.zeros((4, 16), np.int32)
    mc.idct_dequant_2x2_dc(10, [1000, 0, 0, 0], d32, dmf, 47)
    assert d32[0, 0] == 1152000


# ------------------------------------------------------------------ 4. decoder agreement
@pytest.mark.parametrize("bd,cf", LISTS)
@pytest.mark.parametrize("dec", [0, 1])
def test_decoder_agreement(bd, cf, dec):
    """the outputs alone determine recon; and a block whose nnz is 0 has no level"""
    for key in mc.case_keys(bd, cf) + [(bd, cf, 5, 4, 2, "jvt", 0)]:
        case, out = mc.make_case(*key), mc.expected(key, dec)
        ry, rc = mc.decode(case, out)
        assert np.array_equal(ry, out.recon_y), key
        if cf:
            assert np.array_equal(rc, out.recon_c), key
        t8 = (case.flags & mc.T8) != 0
        lev_nz = out.level.reshape(case.nmb, 48, 16).any(axis=2)
        l8 = out.level[:, :16].reshape(case.nmb, 4, 64).any(axis=2)
        assert not (lev_nz[~t8] & (out.nnz[~t8] == 0)).any(), key
        assert not (l8[t8] & (out.nnz[t8][:, 0:16:4] == 0)).any(), key
        assert not (lev_nz[:, 16:] & (out.nnz[:, 16:] == 0)).any(), key
        dc_nz = np.stack([(out.cbp >> 9) & 1, (out.cbp >> 10) & 1], axis=1)
        assert not (out.chroma_dc.any(axis=2) & (dc_nz == 0)).any(), key
        intra = (case.flags & mc.INTRA) != 0
        assert not out.level[intra].any() and not out.cbp[intra].any() and not out.nnz[intra].any()
        assert np.array_equal(out.flags_out[intra], case.flags[intra])


# ------------------------------------------------------------------ 5. coverage of the inputs
LUMA = ("dropped", "part", "whole")
CHROMA = ("chroma_early_none", "chroma_early_dc", "chroma_opt0", "chroma_dconly", "chroma_empty", "chroma_dcac",
          "dmf_shortcut", "dmf_search")


@pytest.mark.parametrize("bd,cf", LISTS)
def test_case_lists_reach_every_branch(bd, cf):
    cnt = collections.Counter()
    coded = cbp = changed = differs = 0
    for key in mc.case_keys(bd, cf):
        case = mc.make_case(*key)
        o1, o0 = mc.expected(key, 1), mc.expected(key, 0)
        cnt.update(o1.counters)
        cnt.update(o0.counters)
        live = (case.flags & (mc.INTRA | mc.SKIP)) == 0
        coded += int(live.sum())
        cbp += int((o1.cbp[live] != 0).sum())
        d = o1.recon_y != case.pred_y
        dd = o1.recon_y != o0.recon_y
        per_mb = lambda a, rows: a.reshape(case.nframes, case.mbh, rows, case.mbw, 16).any(axis=(2, 4)).reshape(-1)
        ch, df = per_mb(d, 16), per_mb(dd, 16)
        if cf:
            ch = ch | per_mb(o1.recon_c != case.pred_c, case.chroma_rows)
            df = df | per_mb(o1.recon_c != o0.recon_c, case.chroma_rows)
        changed += int(ch[live].sum())
        differs += int(df.sum())
    for tag in ("4", "8"):
        for b in LUMA:
            assert cnt[(tag, f"luma{tag}_{b}")] > 0, (tag, b)
        for b in CHROMA if cf else ():
            assert cnt[(tag, b)] > 0, (tag, b)
    assert cbp * 10 >= coded and changed * 10 >= coded, (coded, cbp, changed)
    assert differs >= 1


@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_keys_reach_every_bound_on_both_sides(bd):
    """over what tests/test_gpu_mbenc.py runs, every bound of the reference the checker restates is
    met from below, from above and exactly: the decimate scores 4 / 6 (both transforms) and 7
    (chroma), chroma qp 18, var2 against 4 * thresh, ssd against thresh, dmf against 32 * 64; and
    the exact hits are the boundary pictures' own"""
    cnt, own = collections.Counter(), collections.Counter()
    for key, dec in mc.gpu_keys(bd=bd, dec=1):
        cnt.update(mc.expected(key, dec).counters)
        if key in mc.boundary_keys():
            own.update(mc.expected(key, dec).counters)
    bounds = [(t, b) for t in ("4", "8") for b in ("score8x8", "score_mb")]
    bounds += [("4", b) for b in ("score_chroma", "chroma_qp", "var2", "ssd", "dmf")]
    for tag, b in bounds:
        for side in ("below", "at", "above"):
            assert cnt[(tag, (b, side))] > 0, (tag, b, side)
        assert own[(tag, (b, "at"))] > 0, (tag, b)
    for cf in (1, 2):                                                # the early-out's equalities in each chroma format
        at = collections.Counter()
        for key in mc.boundary_keys():
            if key[0] == bd and key[1] == cf:
                at.update(mc.expected(key, 1).counters)
        for b in ("score_chroma", "chroma_qp", "var2", "ssd", "dmf"):
            assert at[("4", (b, "at"))] > 0, (cf, b)


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised selections of tests/test_gpu_mbenc.py add up to gpu_keys(), nothing twice"""
    picked = [kd for bd in (8, 10) for cf in (0, 1, 2) for dec in (0, 1) for kd in mc.gpu_keys("shapes", bd=bd, cf=cf, dec=dec)]
    picked += [kd for bd in (8, 10) for cf in (1, 2) for kd in mc.gpu_keys("jvt", bd=bd, cf=cf)]
    picked += mc.gpu_keys("boundary")
    assert sorted(map(repr, picked)) == sorted(map(repr, mc.gpu_keys())) and len(set(picked)) == len(picked)
    for key, _ in mc.gpu_keys("boundary"):
        assert key[2] * key[3] * key[4] <= 40 and key[2] <= 5 and key[3] <= 4


def test_case_lists_mix_every_kind_of_macroblock():
    case = mc.make_case(8, 1, 5, 4, 2)
    fl = case.flags
    for bit in (mc.INTRA, mc.T8, mc.D16, mc.SKIP):
        assert (fl & bit).any() and not (fl & bit).all()
    big = mc.make_case(10, 2, 24, 14, 2)
    assert big.qp.min() == 0 and big.qp.max() == mc.qp_max_spec(10)
    qpc = big.qp_table[big.qp]
    assert (qpc < 18).any() and (qpc >= 18).any()
    assert set(np.unique(big.klass)) == set(range(7))


# ------------------------------------------------------------------ 6. the host side
_SCALARS = {"int": ctypes.c_int, "intptr_t": ctypes.c_ssize_t}


def _prototypes():
    inc = os.path.join(ROOT, "include")
    src = subprocess.run(["gcc", "-E", "-P", "-I", inc, HEADER], capture_output=True, text=True, check=True).stdout
    own = subprocess.run(["gcc", "-E", "-P", "-I", inc, os.path.join(inc, "x264hip.h")], capture_output=True, text=True,
                         check=True).stdout
    known = set(re.findall(r"\b(x264hip_\w+)\s*\(", own))
    protos = {}
    for decl in " ".join(src.split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1) and m.group(2) not in known:
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text:
        return ctypes.c_void_p
    return _SCALARS[[w for w in text.split() if w != "const"][0]]


def test_mbenc_signatures_symbols_and_header():
    so = ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    assert sorted(protos) == sorted(f"x264hip_{bd}_{n}" for n in x._MBENC for bd in (8, 10)) == \
        ["x264hip_10_mb_encode_inter", "x264hip_8_mb_encode_inter"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret) and len(fn.argtypes) == len(params), name
        for p, a in zip(params, fn.argtypes):
            assert a is _ctype_of(p), (name, p, a)
        assert params[-1] == "void *stream"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(protos) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in ("mb_encode_inter", "MbEnc"):
        assert n in x.__all__ and callable(getattr(x, n))
    text = open(HEADER).read()
    assert '#include "x264hip.h"' in text
    assert "mb_encode" not in open(os.path.join(ROOT, "include", "x264hip.h")).read()
    for word in ("4:4:4", "intra", "lossless", "trellis", "noise reduction", "pskip_mv", "zigzag_interleave_8x8_cavlc",
                 "macroblock.c:618-972", "macroblock.c:259-490"):
        assert word in text, word
    assert (x.MBENC_INTRA, x.MBENC_T8x8, x.MBENC_D16x16, x.MBENC_SKIP) == (mc.INTRA, mc.T8, mc.D16, mc.SKIP)


def test_mbenc_layout_matches_ctypes(tmp_path):
    x = load_package()
    names = [n for n, _ in x.MbEnc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "x264hip_mbenc.h"\nint main(void) {\n'
    src += '    printf("size %zu\\n", sizeof(x264hip_mbenc_t));\n'
    for n in names:
        src += f'    printf("{n} %zu\\n", offsetof(x264hip_mbenc_t, {n}));\n'
    src += "    return 0;\n}\n"
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(vals.pop("size")) == ctypes.sizeof(x.MbEnc)
    for n in names:
        assert getattr(x.MbEnc, n).offset == int(vals[n]), n
    # every member of the C struct is in the ctypes one: the sizes agree and the last member ends it
    assert x.MbEnc.flags_out.offset + 8 == ctypes.sizeof(x.MbEnc)


_TABLE = np.minimum(np.arange(64), 39).astype(np.uint8)
EINVAL, ENODEV = -1, -3
_POINTERS = ("chroma_qp_table", "quant4_mf", "quant4_bias", "dequant4_mf", "fenc", "pred", "recon", "qp", "mb_flags",
             "level", "chroma_dc", "nnz", "cbp", "nz", "flags_out")


def _e(x, cf=1, **kw):
    """a valid x264hip_mbenc_t on made-up addresses"""
    e = x.MbEnc()
    e.chroma_format, e.b_dct_decimate = cf, 1
    e.chroma_qp_table = _TABLE.ctypes.data
    for k, n in enumerate(n for n, _ in x.MbEnc._fields_ if n not in ("chroma_format", "b_dct_decimate",
                                                                       "chroma_qp_table") and "stride" not in n):
        setattr(e, n, 0x40000000 + 0x1000000 * k)
    for n, _ in x.MbEnc._fields_:
        if n.endswith("_frame_stride"):
            setattr(e, n, 192 * 128)
        elif n.endswith("_stride"):
            setattr(e, n, 192)
    for name, v in kw.items():
        setattr(e, name, v)
    return e


@pytest.mark.parametrize("bd", [8, 10])
def test_mb_encode_inter_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_encode_inter")

    def call(e, mbw=5, mbh=4, n=2):
        return fn(ctypes.byref(e) if e is not None else None, mbw, mbh, n, None)

    assert call(None) == EINVAL
    for field in _POINTERS:
        assert call(_e(x, **{field: None})) == EINVAL, field
    for cf in (1, 2):
        for field in ("fenc_chroma", "pred_chroma", "recon_chroma"):
            assert call(_e(x, cf=cf, **{field: None})) == EINVAL, (cf, field)
    assert call(_e(x, cf=-1)) == EINVAL and call(_e(x, cf=3)) == EINVAL
    # the transform-8 tables come together or not at all
    for field in ("quant8_mf", "quant8_bias", "dequant8_mf"):
        assert call(_e(x, **{field: None})) == EINVAL, field
    assert call(_e(x), mbw=-1) == EINVAL and call(_e(x), mbh=-1) == EINVAL and call(_e(x), n=-1) == EINVAL
    assert call(_e(x), mbw=1 << 15, mbh=1 << 14, n=1) == EINVAL                      # more than 2^28 MBs
    for field in ("recon_stride", "recon_frame_stride", "recon_chroma_stride", "recon_chroma_frame_stride"):
        assert call(_e(x, **{field: 190})) == EINVAL, field
    px = 1 if bd == 8 else 2
    assert call(_e(x, recon=0x40000000 + 2 * px)) == EINVAL and call(_e(x, recon_chroma=0x40000000 + px)) == EINVAL
    bad = _TABLE.copy()
    bad[7] = 52 + 6 * (bd - 8)
    assert call(_e(x, chroma_qp_table=bad.ctypes.data)) == EINVAL
    bad[7] = 51 + 6 * (bd - 8) - 2                                 # in range at 4:2:0, past the tables at 4:2:2
    assert call(_e(x, cf=2, chroma_qp_table=bad.ctypes.data)) == EINVAL
    # nothing to do is OK without a launch (and without a device); errors stay errors
    for cf in range(3):
        e = _e(x, cf=cf)
        if not cf:
            e.fenc_chroma = e.pred_chroma = e.recon_chroma = None
        assert call(e, n=0) == 0 and call(e, mbw=0) == 0 and call(e, mbh=0) == 0
    e = _e(x)
    e.quant8_mf = e.quant8_bias = e.dequant8_mf = None
    assert call(e, n=0) == 0
    assert call(_e(x, pred=None), n=0) == EINVAL and call(None, n=0) == EINVAL
    if not x.lib().x264hip_available():
        assert call(_e(x)) == ENODEV


def test_wrapper_refusals_need_no_device():
    import torch
    x = load_package()
    y = torch.zeros((1, 16, 16), dtype=torch.uint8)
    plane = (y, 0, 16, 256)
    q = (torch.zeros(1, dtype=torch.int16), torch.zeros(1, dtype=torch.int16))
    dq = torch.zeros(1, dtype=torch.int32)
    qp, fl = torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.uint8)
    ok = dict(fenc=plane, pred=plane, mb_width=1, mb_height=1, nframes=1, qp=qp, mb_flags=fl, quant4=q, dequant4_mf=dq)
    with pytest.raises(ValueError, match="chroma_format"):
        x.mb_encode_inter(**ok, chroma_format=3)
    with pytest.raises(ValueError, match="fenc_chroma"):
        x.mb_encode_inter(**ok, chroma_format=1)
    with pytest.raises(ValueError, match="come together"):
        x.mb_encode_inter(**ok, quant8=q)
    with pytest.raises(ValueError, match="negative"):
        x.mb_encode_inter(**{**ok, "nframes": -1})
    with pytest.raises(ValueError, match="QP_MAX_SPEC"):
        x.mb_encode_inter(**ok, qp_table=np.zeros(51, np.uint8))
    with pytest.raises(ValueError, match="one element per macroblock"):
        x.mb_encode_inter(**{**ok, "mb_width": 2})
    with pytest.raises(ValueError, match="level"):
        x.mb_encode_inter(**ok, outs={"level": torch.zeros(4, dtype=torch.int16)})
