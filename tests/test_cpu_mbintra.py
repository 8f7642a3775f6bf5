"""CPU: the checker of the intra macroblock encode (tests/mbintra_cases.py) held to independent
evidence, and the host side of x264hip_*_mb_encode_intra.  No GPU.

1. The Python 4x4 directional predictors equal tests/golden/intra4x4_golden.npz (the reference's
   own per-pixel lists).
2. Where the oracle has a mode, the Python dispatcher equals it on random FDEC buffers.
3. The _dc_left / _dc_top / _dc_128 variants and 16x16 P / 8x16c P on hand-worked vectors.
4. I_16x16 anchor: a DC-only macroblock reconstructs to prediction + add16x16_idct_dc.
5. I_4x4 anchor: V everywhere, no residual: the top row repeated.
6. Decoder agreement: the reconstruction rebuilt from the outputs alone equals recon.
7. Coverage: conditions on the inputs, asserted from the checker's branch counters over exactly
   the case lists tests/test_gpu_mbintra.py runs.
8. include/x264hip_mbintra.h's prototypes, the ctypes declarations, the exported symbols and the
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
import mbintra_cases as mi
import oracle_lib as orc
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mbintra.h")
FDEC, OY = mi.FDEC, mi.OY


def _rand_buf(bd, seed):
    return np.random.default_rng(seed).integers(0, 1 << bd, mi.BUF).astype(orc.pixel_dtype(bd))


def _block(buf, off, w, h):
    return buf[off:off + h * FDEC].reshape(h, FDEC)[:, :w].astype(np.int64)


# ------------------------------------------------------------------ 1. the golden 4x4 lists
@pytest.mark.parametrize("bd", [8, 10])
def test_directional_4x4_equal_the_reference_lists(bd):
    g = np.load(os.path.join(ROOT, "tests", "golden", "intra4x4_golden.npz"))
    nb, want = g[f"neighbours_{bd}"], g[f"pred_{bd}"]
    assert nb.shape[1] == 13 and want.shape[1:] == (6, 4, 4) and nb.max() == (1 << bd) - 1
    for i in range(len(nb)):
        for k in range(6):
            assert np.array_equal(mi.pred4x4_dir(3 + k, nb[i]), want[i, k]), (i, 3 + k)
    # through the dispatcher too: the neighbours laid out around a block of an FDEC buffer
    buf = np.zeros(mi.BUF, orc.pixel_dtype(bd))
    for i in range(8):
        buf[OY - FDEC:OY - FDEC + 8], buf[OY - 1:OY - 1 + 4 * FDEC:FDEC], buf[OY - FDEC - 1] = nb[i, :8], nb[i, 8:12], nb[i, 12]
        for k in range(6):
            mi.predict(bd, "4x4", 3 + k, buf, OY)
            assert np.array_equal(_block(buf, OY, 4, 4), want[i, k]), (i, 3 + k)


# ------------------------------------------------------------------ 2. the oracle's modes
@pytest.mark.parametrize("bd", [8, 10])
def test_dispatcher_equals_the_oracle_where_it_has_the_mode(bd):
    """4x4 / 16x16 V, H, DC, chroma DC, H, V for 8 and 16 rows, 8x8c P, predict_8x8 0..8: the
    dispatcher's result against a direct call (the Python restatements of the same modes below)"""
    for seed in range(4):
        src = _rand_buf(bd, seed)
        for kind, (w, h) in (("4x4", (4, 4)), ("16x16", (16, 16)), ("8x8c", (8, 8)), ("8x16c", (8, 16))):
            for mode in range(4 if kind == "8x8c" else 3):
                a, b = src.copy(), src.copy()
                mi.predict(bd, kind, mode, a, OY)
                orc.fn(bd, "predict")(mi.KIND[kind], mode, orc._addr(b, OY))
                assert np.array_equal(a, b), (kind, mode)
                S = lambda x, y: int(src[OY + x + y * FDEC])
                blk = _block(a, OY, w, h)
                square = kind in ("4x4", "16x16")
                if mode == (0 if square else 2):
                    assert all((blk[:, x] == S(x, -1)).all() for x in range(w)), (kind, mode)
                if mode == 1:
                    assert all((blk[y] == S(-1, y)).all() for y in range(h)), (kind, mode)
                if square and mode == 2:
                    s = sum(S(x, -1) for x in range(w)) + sum(S(-1, y) for y in range(h))
                    assert (blk == (s + w) >> (3 if w == 4 else 5)).all()
        for mode in range(9):
            for n8 in (15, 11, 7, 3):
                a = src.copy()
                mi.predict8x8(bd, mode, n8, a, OY)
                edge = orc.predict_8x8_filter(bd, src, OY, n8, mi.PRED4_NEIGHBORS[mode])
                assert np.array_equal(_block(a, OY, 8, 8), orc.predict_8x8(bd, mode, edge)), (mode, n8)


# ------------------------------------------------------------------ 3. hand-worked vectors
@pytest.mark.parametrize("bd", [8, 10])
def test_dc_variants_and_planes_on_hand_worked_vectors(bd):
    pm, half = (1 << bd) - 1, 1 << (bd - 1)
    dt = orc.pixel_dtype(bd)

    def buf_with(top, left, lt):
        """top[x] at (x, -1), left[y] at (-1, y), lt at (-1, -1); the block itself holds rubbish"""
        b = np.full(mi.BUF, 77, dt)
        b[OY - FDEC:OY - FDEC + len(top)] = top
        b[OY - 1:OY - 1 + len(left) * FDEC:FDEC] = left
        b[OY - FDEC - 1] = lt
        return b

    ramp = np.arange(16)
    # --- 16x16: left = 10 + y, top = 100 + 2x
    b = buf_with(100 + 2 * ramp, 10 + ramp, 5)
    for mode, want in ((4, (sum(10 + ramp) + 8) >> 4), (5, (sum(100 + 2 * ramp) + 8) >> 4), (6, half)):
        mi.predict(bd, "16x16", mode, b, OY)
        assert (_block(b, OY, 16, 16) == want).all(), mode
    assert (sum(10 + ramp) + 8) >> 4 == 18 and (sum(100 + 2 * ramp) + 8) >> 4 == 115
    # --- 4x4: left = 1, 2, 3, 5 (sum 11), top = 9, 9, 10, 10 (sum 38)
    b = buf_with([9, 9, 10, 10, 0, 0, 0, 0], [1, 2, 3, 5], 0)
    for mode, want in ((9, 3), (10, 10), (11, half)):            # (11 + 2) >> 2, (38 + 2) >> 2
        mi.predict(bd, "4x4", mode, b, OY)
        assert (_block(b, OY, 4, 4) == want).all(), mode
    # --- 8x8 luma: DC_LEFT / DC_TOP read the filtered edge; a flat edge filters to itself
    for mode, want in ((9, 40), (10, 60), (11, half)):
        b = buf_with([60] * 16, [40] * 8, 40 if mode == 9 else 60)
        mi.predict8x8(bd, mode, 15, b, OY)
        assert (_block(b, OY, 8, 8) == want).all(), mode
    # --- chroma, 8 and 16 rows: left = 4 * (y // 4) + 1 (every four rows their own value), top = 20 | 30
    for kind, h in (("8x8c", 8), ("8x16c", 16)):
        left = 4 * (np.arange(h) // 4) + 1
        b = buf_with([20] * 4 + [30] * 4, left, 0)
        mi.predict(bd, kind, 4, b, OY)
        assert np.array_equal(_block(b, OY, 8, h), np.repeat(left[:, None], 8, 1)), kind
        mi.predict(bd, kind, 5, b, OY)
        assert np.array_equal(_block(b, OY, 8, h), np.repeat(np.array([20] * 4 + [30] * 4)[None], h, 0)), kind
        mi.predict(bd, kind, 6, b, OY)
        assert (_block(b, OY, 8, h) == half).all(), kind
    # --- the plane modes: a flat neighbourhood comes back (H = V = 0, a = 32 v: (32 v + 16) >> 5 = v)
    for kind, w, h in (("16x16", 16, 16), ("8x16c", 8, 16), ("8x8c", 8, 8)):
        for v in (0, 1, 93, pm):
            b = buf_with([v] * w, [v] * h, v)
            mi.predict(bd, kind, 3, b, OY)
            assert (_block(b, OY, w, h) == v).all(), (kind, v)
    # --- a plane in, the same plane out: p(x, y) = 50 + 2x + 3y continued into the border
    #     16x16: H = sum (i+1) * 2 * (2i+2) = 4 * 204 = 816, b = (5*816 + 32) >> 6 = 64 = 2 << 5; V: c = 96
    for kind, w, h in (("16x16", 16, 16), ("8x16c", 8, 16)):
        b = buf_with(50 + 2 * np.arange(w) - 3, 50 - 2 + 3 * np.arange(h), 50 - 2 - 3)
        mi.predict(bd, kind, 3, b, OY)
        yy, xx = np.mgrid[0:h, 0:w]
        assert np.array_equal(_block(b, OY, w, h), 50 + 2 * xx + 3 * yy), kind
    # --- the clip: full-scale neighbours, 0 before the middle and the maximum after, overshoot at both ends
    for kind, w, h in (("16x16", 16, 16), ("8x16c", 8, 16)):
        top = np.where(np.arange(w) < w // 2, 0, pm)
        left = np.where(np.arange(h) < h // 2, 0, pm)
        b = buf_with(top, left, 0)
        mi.predict(bd, kind, 3, b, OY)
        blk = _block(b, OY, w, h)
        assert blk.min() == 0 and blk.max() == pm and blk[0, 0] == 0 and blk[h - 1, w - 1] == pm
        assert (np.diff(blk, axis=1) >= 0).all() and (np.diff(blk, axis=0) >= 0).all()
    # 16x16 by hand: H = V = pm * (1 + .. + 8) - 0 = 36 pm (i = 7 reads lt = 0), b = c = (180 pm + 32) >> 6
    b = buf_with(np.where(ramp < 8, 0, pm), np.where(ramp < 8, 0, pm), 0)
    mi.predict(bd, "16x16", 3, b, OY)
    bb = (5 * 36 * pm + 32) >> 6
    i00 = 16 * 2 * pm - 14 * bb + 16
    assert _block(b, OY, 16, 16)[3, 9] == min(max((i00 + 9 * bb + 3 * bb) >> 5, 0), pm)


# ------------------------------------------------------------------ 4. and 5. the anchors
def _single(bd, cf, fenc, qp, flags, modes, cmode=6):
    """a 1x1 picture with the given luma fenc [16, 16]"""
    base = mi.make_case(bd, cf, 1, 1, 1, "flat", 0, True)
    case = types.SimpleNamespace(**vars(base))
    case.fenc_y = np.asarray(fenc, orc.pixel_dtype(bd)).reshape(1, 16, 16)
    case.qp = np.array([qp], np.int8)
    case.flags = np.array([flags], np.uint8)
    case.pred_mode = np.asarray(modes, np.int8).reshape(1, 16)
    case.chroma_pred_mode = np.array([cmode], np.int8)
    return case


@pytest.mark.parametrize("bd", [8, 10])
def test_i16x16_dc_only_anchor(bd):
    """b_dct_decimate = 0, a flat macroblock 40 above DC_128's prediction: every AC is zero, luma_dc
    is not, and recon is the prediction + the oracle's add16x16_idct_dc of the dequantised DCs"""
    half = 1 << (bd - 1)
    qp = 20 + 6 * (bd - 8)
    case = _single(bd, 0, np.full((16, 16), half + 40), qp, mi.INTRA | mi.I16, [6] + [0] * 15)
    out = mi.encode(case, 0)
    assert out.counters["i16_dc_only"] == 1 and not out.level.any() and not out.nnz.any()
    assert out.luma_dc[0, 0] != 0 and not out.luma_dc[0, 1:].any() and out.cbp[0] == 1 << 8 and out.nz[0] == 0
    T = mc.tables(bd)
    dc = mc._unzig(out.luma_dc[0], mc.ZIG4, 4)
    orc.fn(bd, "idct4x4dc")(orc._addr(dc))
    orc.fn(bd, "dequant_4x4_dc")(orc._addr(dc), orc._addr(T.dq4[mi.CQM_4IY]), qp)
    want = np.full(16 * FDEC, half, orc.pixel_dtype(bd))
    orc.fn(bd, "add16x16_idct_dc")(orc._addr(want), orc._addr(dc))
    assert np.array_equal(out.recon_y[0], want.reshape(16, FDEC)[:, :16])
    assert abs(int(out.recon_y[0, 0, 0]) - (half + 40)) <= 3 and (out.recon_y == out.recon_y[0, 0, 0]).all()


@pytest.mark.parametrize("bd", [8, 10])
def test_i4x4_vertical_anchor(bd):
    """one I_4x4 macroblock below an inter one, V everywhere, fenc flat at a high qp: nothing is
    coded and recon is the row above repeated"""
    base = mi.make_case(bd, 0, 1, 3, 1, "flat", 0, True)
    case = types.SimpleNamespace(**vars(base))
    case.flags = np.array([0, mi.INTRA, 0], np.uint8)
    case.qp = np.full(3, mc.qp_max_spec(bd), np.int8)
    case.pred_mode = np.zeros((3, 16), np.int8)
    case.fenc_y = base.fenc_y.copy()
    case.fenc_y[0, 16:32] = 100 << (bd - 8)
    top = (100 << (bd - 8)) + (np.arange(16) % 3) - 1
    recon = base.pred_y.copy()
    recon[0, 15] = top
    pred = recon.copy()
    pred[0, :16] = case.fenc_y[0, :16]                               # (the inter macroblocks: no residual)
    pred[0, 15] = top
    pred[0, 32:] = case.fenc_y[0, 32:]
    out = mi.encode(case, 1, pred, None)
    assert np.array_equal(out.recon_y[0, 15], top)
    assert np.array_equal(out.recon_y[0, 16:32], np.repeat(top[None], 16, 0))
    assert out.cbp[1] == 0 and not out.level[1].any() and not out.nnz[1].any() and out.flags_out[1] == mi.INTRA


# ------------------------------------------------------------------ 6. decoder agreement
LISTS = [(bd, cf) for bd in (8, 10) for cf in (0, 1, 2)]


def gpu_keys(bd, cf):
    """every key tests/test_gpu_mbintra.py runs at this bit depth and chroma format"""
    keys = [key for key, _ in mi.gpu_keys(bd=bd, cf=cf)]
    return sorted(set(keys), key=keys.index)


@pytest.mark.parametrize("bd,cf", LISTS)
def test_decoder_agreement(bd, cf):
    for key in gpu_keys(bd, cf):
        case = mi.make_case(*key)
        for dec in (0, 1):
            out = mi.expected(key, dec)
            ry, rc = mi.decode(case, out)
            assert np.array_equal(ry, out.recon_y), (key, dec)
            if cf:
                assert np.array_equal(rc, out.recon_c), (key, dec)
            # no level exists where nnz is 0
            assert not out.level[out.nnz.repeat(16, 1).reshape(out.level.shape) == 0].any()
            assert not out.luma_dc[(out.cbp >> 8 & 1) == 0].any()
            assert not out.chroma_dc[:, 0][(out.cbp >> 9 & 1) == 0].any()
            assert not out.chroma_dc[:, 1][(out.cbp >> 10 & 1) == 0].any()


# ------------------------------------------------------------------ 7. coverage
@pytest.mark.parametrize("cf", [0, 1, 2])
def test_inputs_reach_every_branch(cf):
    """conditions on the inputs, per chroma format, over both bit depths, both b_dct_decimate and
    exactly the keys the GPU tests run"""
    cnt = {0: collections.Counter(), 1: collections.Counter()}
    for bd in (8, 10):
        for key in gpu_keys(bd, cf):
            for dec in (0, 1):
                cnt[dec].update(mi.expected(key, dec).counters)
    both = cnt[0] + cnt[1]
    for m in range(12):
        assert both["mode4", m] and both["mode8", m], m
    for m in range(7):
        assert both["mode16", m] and (not cf or both["modec", m]), m
    for arm in ("i16_idct_dc", "i16_idct_nodc", "i16_dc_only", "i16_pred_only"):
        assert both[arm], arm
    assert cnt[1]["i16_decimated"] and not cnt[0]["i16_decimated"]
    own = collections.Counter()
    for key in mi.boundary_keys():
        if key[1] == cf:
            own.update(mi.expected(key, 1).counters)
    for side in ("below", "at", "above"):                            # the AC decimate score against 6
        assert cnt[1]["i16_score", side] and own["i16_score", side], side
    for tail in ("chroma_empty", "chroma_dconly", "chroma_dcac") if cf else ():
        assert both[tail], tail
    assert both["topright_emulated"] and both["topright_real"]
    for side in (False, True):
        assert both["have_lt", side] and both["have_tr", side], side
    assert both["inter_neighbours"]
    assert both["intra_coded"] * 10 >= both["intra"] > 0
    for t in ("i4", "i8", "i16"):
        assert both["type", t], t


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised selections of tests/test_gpu_mbintra.py add up to gpu_keys(), nothing twice"""
    grid = [(bd, cf, dec) for bd in (8, 10) for cf in (0, 1, 2) for dec in (0, 1)]
    picked = [kd for bd, cf, dec in grid for kd in mi.gpu_keys("shapes", bd=bd, cf=cf, dec=dec)]
    picked += [kd for bd in (8, 10) for cf in (1, 2) for kd in mi.gpu_keys("jvt", bd=bd, cf=cf)]
    picked += [kd for bd in (8, 10) for cf in (0, 1, 2) for kd in mi.gpu_keys("all_intra", bd=bd, cf=cf)]
    picked += mi.gpu_keys("boundary")
    assert sorted(map(repr, picked)) == sorted(map(repr, mi.gpu_keys())) and len(set(picked)) == len(picked)


def test_case_lists():
    """the mixed pictures hold both kinds of macroblock, the small ones and the I picture only intra
    ones, and every mode is valid where it stands"""
    for key in gpu_keys(8, 1):
        case = mi.make_case(*key)
        intra = (case.flags & mi.INTRA) != 0
        assert intra.all() if key[-1] else (intra.any() and not intra.all()), key
        assert not (case.flags[intra] & mc.SKIP).any()
        for mb in np.flatnonzero(intra):
            _, my, mx = mi._coords(case, mb)
            nb = mi.mb_neighbours(mx, my, case.mbw)
            kind = mi.mb_type(int(case.flags[mb]))
            if kind == "i16":
                assert case.pred_mode[mb, 0] in mi.valid_modes("16x16", nb)
            elif kind == "i8":
                assert all(case.pred_mode[mb, 4 * i] in mi.valid_modes("8x8", mi.neighbour8(i, nb)) for i in range(4))
            else:
                assert all(case.pred_mode[mb, i] in mi.valid_modes("4x4", mi.neighbour4(i, nb)) for i in range(16))
            assert case.chroma_pred_mode[mb] in mi.valid_modes("chroma", nb)
    assert mi.valid_modes("4x4", 0) == [11] and mi.valid_modes("16x16", 0) == [6] and mi.valid_modes("chroma", 0) == [6]
    # i_neighbour4 / i_neighbour8 in the middle of a picture and at its first macroblock
    assert [mi.neighbour4(i, 15) for i in range(16)] == [15, 15, 15, 11, 15, 15, 15, 11, 15, 15, 15, 11, 15, 11, 15, 11]
    assert [mi.neighbour8(i, 15) for i in range(4)] == [15, 15, 15, 11]
    assert mi.neighbour4(0, 0) == 0 and mi.neighbour4(1, 0) == 1 and mi.neighbour4(2, 0) == 6 and mi.neighbour4(5, 0) == 1
    assert mi.neighbour4(5, 11) == 11 and mi.neighbour8(1, 11) == 11          # no top-right macroblock


# ------------------------------------------------------------------ 8. the host side
_SCALARS = {"int": ctypes.c_int, "intptr_t": ctypes.c_ssize_t}


def _prototypes():
    """the functions include/x264hip_mbintra.h declares itself (not those of the headers it includes)"""
    inc = os.path.join(ROOT, "include")
    pre = lambda path: subprocess.run(["gcc", "-E", "-P", "-I", inc, path], capture_output=True, text=True, check=True).stdout
    known = set(re.findall(r"\b(x264hip_\w+)\s*\(", pre(os.path.join(inc, "x264hip_mbenc.h"))))
    protos = {}
    for decl in " ".join(pre(HEADER).split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1) and m.group(2) not in known:
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text:
        return ctypes.c_void_p
    return _SCALARS[[w for w in text.split() if w != "const"][0]]


def test_mbintra_signatures_symbols_and_header():
    so = ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    assert sorted(protos) == sorted(f"x264hip_{bd}_{n}" for n in x._MBINTRA for bd in (8, 10)) == \
        ["x264hip_10_mb_encode_intra", "x264hip_8_mb_encode_intra"]
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret) and len(fn.argtypes) == len(params), name
        for p, a in zip(params, fn.argtypes):
            assert a is _ctype_of(p), (name, p, a)
        assert params[-1] == "void *stream"
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(protos) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in ("mb_encode_intra", "MbIntra", "MBINTRA_I16x16", "MBINTRA_OUTPUTS"):
        assert n in x.__all__ and hasattr(x, n)
    assert callable(x.mb_encode_intra)
    text = open(HEADER).read()
    assert '#include "x264hip_mbenc.h"' in text
    for h in ("x264hip.h", "x264hip_mbenc.h"):
        assert "mb_encode_intra" not in open(os.path.join(ROOT, "include", h)).read()
    for word in ("I_PCM", "4:4:4", "slices", "constrained_intra_pred", "lossless", "trellis", "noise reduction",
                 "i_skip_intra", "mode decision", "macroblock.c:706-768", "macroblock.c:259-490", "macroblock.h:132-213",
                 "x + 2y", "pred_mode[4*(i>>2)]"):
        assert word in text, word
    assert x.MBINTRA_I16x16 == mi.I16 == 16 and re.search(r"#define\s+X264HIP_MBINTRA_I16x16\s+16\b", text)
    assert x.MBINTRA_OUTPUTS == x.MBENC_OUTPUTS + ("luma_dc",)


def test_mbintra_layout_matches_ctypes(tmp_path):
    x = load_package()
    names = [n for n, _ in x.MbIntra._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "x264hip_mbintra.h"\nint main(void) {\n'
    src += '    printf("size %zu\\n", sizeof(x264hip_mbintra_t));\n'
    for n in names:
        src += f'    printf("{n} %zu\\n", offsetof(x264hip_mbintra_t, {n}));\n'
    src += "    return 0;\n}\n"
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(vals.pop("size")) == ctypes.sizeof(x.MbIntra)
    for n in names:
        assert getattr(x.MbIntra, n).offset == int(vals[n]), n
    # every member of the C struct is in the ctypes one: the sizes agree and the last member ends it
    assert x.MbIntra.luma_dc.offset + 8 == ctypes.sizeof(x.MbIntra)


_TABLE = np.minimum(np.arange(64), 39).astype(np.uint8)
EINVAL, ENODEV = -1, -3
_POINTERS = ("chroma_qp_table", "quant4_mf", "quant4_bias", "dequant4_mf", "fenc", "recon", "qp", "mb_flags", "pred_mode",
             "level", "chroma_dc", "nnz", "cbp", "nz", "flags_out", "luma_dc")


def _e(x, cf=1, **kw):
    """a valid x264hip_mbintra_t on made-up addresses"""
    e = x.MbIntra()
    e.chroma_format, e.b_dct_decimate = cf, 1
    e.chroma_qp_table = _TABLE.ctypes.data
    for k, n in enumerate(n for n, _ in x.MbIntra._fields_ if n not in ("chroma_format", "b_dct_decimate",
                                                                         "chroma_qp_table") and "stride" not in n):
        setattr(e, n, 0x40000000 + 0x1000000 * k)
    for n, _ in x.MbIntra._fields_:
        if n.endswith("_frame_stride"):
            setattr(e, n, 192 * 128)
        elif n.endswith("_stride"):
            setattr(e, n, 192)
    for name, v in kw.items():
        setattr(e, name, v)
    return e


@pytest.mark.parametrize("bd", [8, 10])
def test_mb_encode_intra_argument_errors(bd):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_encode_intra")

    def call(e, mbw=5, mbh=4, n=2):
        return fn(ctypes.byref(e) if e is not None else None, mbw, mbh, n, None)

    assert call(None) == EINVAL
    for field in _POINTERS:
        assert call(_e(x, **{field: None})) == EINVAL, field
    for cf in (1, 2):
        for field in ("fenc_chroma", "recon_chroma", "chroma_pred_mode"):
            assert call(_e(x, cf=cf, **{field: None})) == EINVAL, (cf, field)
    assert call(_e(x, cf=-1)) == EINVAL and call(_e(x, cf=3)) == EINVAL
    # the 8x8 tables come together or not at all
    for field in ("quant8_mf", "quant8_bias", "dequant8_mf"):
        assert call(_e(x, **{field: None})) == EINVAL, field
    assert call(_e(x), mbw=-1) == EINVAL and call(_e(x), mbh=-1) == EINVAL and call(_e(x), n=-1) == EINVAL
    assert call(_e(x), mbw=1 << 15, mbh=1 << 14, n=1) == EINVAL                      # more than 2^28 MBs
    for field in ("recon_stride", "recon_frame_stride", "recon_chroma_stride", "recon_chroma_frame_stride"):
        assert call(_e(x, **{field: 190})) == EINVAL, field
    px = 1 if bd == 8 else 2
    assert call(_e(x, recon=0x40000000 + 2 * px)) == EINVAL and call(_e(x, recon_chroma=0x40000000 + px)) == EINVAL
    for field in ("level", "chroma_dc", "luma_dc", "cbp", "nz"):
        assert call(_e(x, **{field: 0x40000001})) == EINVAL, field
    bad = _TABLE.copy()
    bad[7] = 52 + 6 * (bd - 8)
    assert call(_e(x, chroma_qp_table=bad.ctypes.data)) == EINVAL
    bad[7] = 51 + 6 * (bd - 8) - 2                                 # in range at 4:2:0, past the tables at 4:2:2
    assert call(_e(x, cf=2, chroma_qp_table=bad.ctypes.data)) == EINVAL
    # nothing to do is OK without a launch (and without a device); errors stay errors
    for cf in range(3):
        e = _e(x, cf=cf)
        if not cf:
            e.fenc_chroma = e.recon_chroma = e.chroma_pred_mode = None
        assert call(e, n=0) == 0 and call(e, mbw=0) == 0 and call(e, mbh=0) == 0
    e = _e(x)
    e.quant8_mf = e.quant8_bias = e.dequant8_mf = None
    assert call(e, n=0) == 0
    assert call(_e(x, recon=None), n=0) == EINVAL and call(None, n=0) == EINVAL
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
    pm, cm = torch.zeros(16, dtype=torch.int8), torch.zeros(1, dtype=torch.int8)
    ok = dict(fenc=plane, recon=plane, mb_width=1, mb_height=1, nframes=1, qp=qp, mb_flags=fl, pred_mode=pm, quant4=q,
              dequant4_mf=dq)
    with pytest.raises(ValueError, match="chroma_format"):
        x.mb_encode_intra(**ok, chroma_format=3)
    with pytest.raises(ValueError, match="fenc_chroma"):
        x.mb_encode_intra(**ok, chroma_format=1)
    with pytest.raises(ValueError, match="chroma_pred_mode"):
        x.mb_encode_intra(**ok, chroma_format=1, fenc_chroma=plane, recon_chroma=plane)
    with pytest.raises(ValueError, match="come together"):
        x.mb_encode_intra(**ok, quant8=q)
    with pytest.raises(ValueError, match="negative"):
        x.mb_encode_intra(**{**ok, "nframes": -1})
    with pytest.raises(ValueError, match="QP_MAX_SPEC"):
        x.mb_encode_intra(**ok, qp_table=np.zeros(51, np.uint8))
    with pytest.raises(ValueError, match="one element per macroblock"):
        x.mb_encode_intra(**{**ok, "mb_width": 2})
    with pytest.raises(ValueError, match="16 modes per macroblock"):
        x.mb_encode_intra(**{**ok, "pred_mode": pm[:8]})
    with pytest.raises(ValueError, match="16 modes per macroblock"):
        x.mb_encode_intra(**{**ok, "pred_mode": pm.to(torch.uint8)})
    with pytest.raises(ValueError, match="one mode per macroblock"):
        x.mb_encode_intra(**ok, chroma_format=1, fenc_chroma=plane, recon_chroma=plane, chroma_pred_mode=cm.to(torch.uint8))
    with pytest.raises(ValueError, match="luma_dc"):
        x.mb_encode_intra(**ok, outs={"luma_dc": torch.zeros(4, dtype=torch.int16)})
