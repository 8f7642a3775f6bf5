"""CPU: the checker of the 4:4:4 macroblock encodes (tests/mb444_cases.py) tied to the existing
ones, and the host side of include/x264hip_mb444.h.  No GPU.

* Plane 0 of the 4:4:4 checker equals the luma-only checkers of mbenc_cases / mbintra_cases on the
  same picture (nothing carries into the first plane); U's and V's pixels fed as plane 0 with the
  carry forced to 0 equal mbenc_cases.encode_luma.
* Decoder agreement: the planes rebuilt from level / luma_dc alone equal recon, inter and intra.
* cqm_init444 / cqm_dequant444 equal the oracle's two-call construction and, where they overlap,
  the existing cqm_init / cqm_dequant.
* The header's prototypes, the ctypes declarations, the exported symbols and the struct layout
  agree; every X264HIP_EINVAL case; the wrappers' refusals.
* Coverage: conditions on the committed seed, asserted from the checker alone over exactly the
  keys tests/test_gpu_mb444.py runs."""
import collections
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import checkasm_bufs as cb
import mb444_cases as m4
import mbenc_cases as mc
import mbintra_cases as mi
import oracle_lib as orc
from conftest import ROOT, ensure_built, load_package

HEADER = os.path.join(ROOT, "include", "x264hip_mb444.h")
FLAT_KEYS = {bd: [k for k in m4.case_keys(bd) if k[4] == "flat"] for bd in (8, 10)}


# ------------------------------------------------------------------ 1. ties to the existing checkers
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("dec", [0, 1])
def test_plane_0_is_the_luma_only_checker(bd, dec):
    """plane 0 meets i_decimate_mb = 0 and the luma categories: everything it leaves is what
    mbenc_cases.encode followed by mbintra_cases.encode leave on the same luma-only picture;
    cbp and flags_out, which see all planes, agree wherever U and V code nothing"""
    for key in FLAT_KEYS[bd]:
        case, got = m4.make_case(*key), m4.expected(key, dec)
        want = mi.encode(m4.luma_case(case), dec)
        assert np.array_equal(got.recon[0], want.recon_y), key
        assert np.array_equal(got.level[:, :16], want.level[:, :16]) and np.array_equal(got.nnz[:, :16], want.nnz[:, :16]), key
        assert np.array_equal(got.nz, want.nz) and np.array_equal(got.luma_dc[:, 0], want.luma_dc), key
        assert np.array_equal(got.cbp & 0x10f, want.cbp | (got.cbp & 0xf)), key      # plane 0's bits are in
        quiet = ~got.nnz[:, 16:].any(axis=1) & ~got.luma_dc[:, 1:].any(axis=(1, 2))
        assert np.array_equal(got.cbp[quiet], want.cbp[quiet]) and np.array_equal(got.flags_out[quiet], want.flags_out[quiet])
        assert not (got.cbp & ~0x70f).any()                       # i_cbp_chroma = 0, bits 4-5


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("dec", [0, 1])
def test_each_plane_alone_without_carry_is_encode_luma(bd, dec):
    """U's and V's (and Y's) pixels as plane 0 with i_decimate_mb = 0 handed in: the restated
    plane body equals mbenc_cases.encode_luma, block for block"""
    key = (bd, 7, 3, 3, "flat", m4.SEED, False)
    case, T4, T = m4.make_case(*key), m4.tables(bd), mc.tables(bd)
    seen = collections.Counter()
    for mb in range(case.nmb):
        fl = int(case.flags[mb])
        if fl & (m4.INTRA | m4.SKIP):
            continue
        f, r = divmod(mb, case.mbw * case.mbh)
        my, mx = divmod(r, case.mbw)
        for p in range(3):
            qp = m4.plane_qp(case, mb, p)
            fenc = m4._fenc_block(case.fenc[p], f, my, mx)
            fd1, fd2 = m4._fdec_block(case.pred[p], f, my, mx), m4._fdec_block(case.pred[p], f, my, mx)
            o1, o2 = m4.MbOut(bd), mc.MbOut(bd)
            score = m4.encode_inter_plane(bd, T4, dec, bool(fl & m4.T8), 0, qp, fenc, fd1, o1, 0)
            cnt = collections.Counter()
            mc.encode_luma(bd, T, dec, bool(fl & m4.T8), qp, fenc, fd2, o2, cnt)
            assert np.array_equal(fd1, fd2) and np.array_equal(o1.nnz[:16], o2.nnz[:16]) and o1.cbp_luma == o2.cbp_luma
            assert np.array_equal(o1.level[:16][o1.nnz[:16] != 0], o2.level[:16][o2.nnz[:16] != 0])
            assert not o1.nnz[16:].any() and not o1.level[16:].any() and score >= 0
            seen.update(k for k in cnt)
    arms = {k.split("_")[1] for k in seen if isinstance(k, str)}     # (the tuple keys count sides of bounds)
    assert arms >= ({"dropped", "part", "whole"} if dec else {"whole"}), seen


# ------------------------------------------------------------------ 2. decoder agreement
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("dec", [0, 1])
def test_decoder_agreement(bd, dec):
    """the outputs alone determine the three planes; a block whose nnz is 0 has no level"""
    for key in m4.case_keys(bd):
        case, out = m4.make_case(*key), m4.expected(key, dec)
        rec = m4.decode(case, out)
        for p in range(3):
            assert np.array_equal(rec[p], out.recon[p]), (key, p)
        t8 = (case.flags & m4.T8) != 0
        lev_nz = out.level.any(axis=2)
        l8 = out.level.reshape(case.nmb, 12, 64).any(axis=2)
        assert not (lev_nz[~t8] & (out.nnz[~t8] == 0)).any(), key
        assert not (l8[t8] & (out.nnz[t8][:, 0:48:4] == 0)).any(), key
        dc_nz = np.stack([(out.cbp >> (8 + p)) & 1 for p in range(3)], axis=1)
        assert not (out.luma_dc.any(axis=2) & (dc_nz == 0)).any(), key
        skip = (case.flags & (m4.SKIP | m4.INTRA)) == m4.SKIP
        assert not out.level[skip].any() and not out.cbp[skip].any() and not out.nnz[skip].any()
        for p in range(3):
            grid = np.repeat(np.repeat(skip.reshape(case.nframes, case.mbh, case.mbw), 16, 1), 16, 2)
            assert np.array_equal(out.recon[p][grid], case.pred[p][grid])


# ------------------------------------------------------------------ 3. the tables
def _lists(name, bd):
    if name == "rand":
        cb.srand(cb.SEED)
        return [list(l[:16]) for l in cb.cqm_lists(4, bd)[:4]] + [list(l) for l in cb.cqm_lists(4, bd)[4:]]
    return m4.lists_of(name)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("name", ["flat", "distinct", "rand"])
def test_cqm444_equals_the_two_call_oracle(oracle, bd, name):
    x = load_package()
    lists = _lists(name, bd)
    for dz_inter, dz_intra in ((21, 11), (0, 0), (5, 30)):
        got = x.cqm_init444(bd, lists, dz_inter, dz_intra)
        q4m, q4b, q8m, q8b = oracle.cqm_init(bd, lists, dz_inter, dz_intra)
        second = lists[:4] + [lists[6], lists[7]] + lists[6:]
        _, _, c8m, c8b = oracle.cqm_init(bd, second, dz_inter=21, dz_intra=11)
        want = (q4m, q4b, np.concatenate([q8m[:2], c8m[:2]]), np.concatenate([q8b[:2], c8b[:2]]))
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (name, dz_inter)
        old = x.cqm_init(bd, lists, dz_inter, dz_intra)
        assert np.array_equal(got[0], old[0]) and np.array_equal(got[1], old[1])
        assert np.array_equal(got[2][:2], old[2][:2]) and np.array_equal(got[3][:2], old[3][:2])
        assert not old[2][2:].any() and not old[3][2:].any()      # the existing entry still leaves them alone
    dq4, dq8 = x.cqm_dequant444(lists)
    o4, o8 = oracle.cqm_dequant(lists)
    _, c8 = oracle.cqm_dequant(lists[:4] + [lists[6], lists[7]] + lists[6:])
    assert dq8.shape == (4, 6, 64) and np.array_equal(dq4, o4) and np.array_equal(dq8, np.concatenate([o8, c8]))
    e4, e8 = x.cqm_dequant(lists)
    assert np.array_equal(dq4, e4) and np.array_equal(dq8[:2], e8) and e8.shape == (2, 6, 64)
    if name == "distinct":
        T = m4.tables(bd, "distinct")
        assert np.array_equal(T.q8m, got[2]) and np.array_equal(T.dq8, dq8)
        for t in (got[0], got[2], dq4, dq8):                      # pairwise different: a wrong category shows
            assert all(not np.array_equal(t[i], t[j]) for i in range(4) for j in range(i))


# ------------------------------------------------------------------ 4. the host side
_SCALARS = {"int": ctypes.c_int, "intptr_t": ctypes.c_ssize_t}


def _prototypes():
    inc = os.path.join(ROOT, "include")
    src = subprocess.run(["gcc", "-E", "-P", "-I", inc, HEADER], capture_output=True, text=True, check=True).stdout
    own = subprocess.run(["gcc", "-E", "-P", "-I", inc, os.path.join(inc, "x264hip_mbintra.h")], capture_output=True,
                         text=True, check=True).stdout
    known = set(re.findall(r"\b(x264hip_\w+)\s*\(", own))
    protos = {}
    for decl in " ".join(src.split()).split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(x264hip_\w+)\s*\((.*)\)\s*", decl)
        if m and "typedef" not in m.group(1) and m.group(2) not in known:
            protos[m.group(2)] = (m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
    return protos


def _ctype_of(text):
    if "*" in text or "[" in text:
        return ctypes.c_void_p
    if text == "void":
        return None
    return _SCALARS[[w for w in text.split() if w != "const"][0]]


def test_mb444_signatures_symbols_and_header():
    so = ensure_built("hip")
    x = load_package()
    protos = _prototypes()
    names = [f"x264hip_{bd}_{n}" for n in x._MB444 for bd in (8, 10)] + [f"x264hip_{n}" for n in x._MB444_PLAIN]
    assert sorted(protos) == sorted(names) and len(names) == 7
    L = x.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is _ctype_of(ret) and len(fn.argtypes) == len(params), name
        for p, a in zip(params, fn.argtypes):
            assert a is _ctype_of(p), (name, p, a)
        assert ("encode" in name) == (params[-1] == "void *stream")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(protos) <= {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in ("cqm_init444", "cqm_dequant444", "mb_encode_inter_444", "mb_encode_intra_444"):
        assert n in x.__all__ and callable(getattr(x, n))
        assert n not in x._PER_DEPTH and n not in x._PLAIN
    text = open(HEADER).read()
    assert '#include "x264hip_mbintra.h"' in text
    for h in ("x264hip.h", "x264hip_mbenc.h", "x264hip_mbintra.h"):
        other = open(os.path.join(ROOT, "include", h)).read()
        assert not re.search(r"x264hip_\w*444\w*\s*\(", other) and "x264hip_mb444_t" not in other
        assert h == "x264hip.h" or "x264hip_mb444.h" in other     # their "Not included: 4:4:4" points here
    for word in ("macroblock.c:769-921", "mb_encode_i16x16 :126-239", "macroblock.h:132-213", ":771", ":907", ":833", "CQM_8PC",
                 "CQM_8IC", "CQM_4PC", "CQM_4IC", "num_8x8_lists = 4", "I_PCM", "slices", "constrained_intra_pred",
                 "lossless", "trellis", "noise", "CAVLC", "953-971", "macroblock.c:1451", "macroblock.c:1617", "x + 2y",
                 "16p + 4*idx", "8 + p"):
        assert word in text, word
    assert x.MB444_OUTPUTS == ("level", "nnz", "cbp", "nz", "flags_out", "luma_dc")


def test_mb444_layout_matches_ctypes(tmp_path):
    x = load_package()
    names = [n for n, _ in x.Mb444._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "x264hip_mb444.h"\nint main(void) {\n'
    src += '    printf("size %zu\\n", sizeof(x264hip_mb444_t));\n'
    for n in names:
        src += f'    printf("{n} %zu\\n", offsetof(x264hip_mb444_t, {n}));\n'
    src += "    return 0;\n}\n"
    c, exe = tmp_path / "probe.c", tmp_path / "probe"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    vals = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                    check=True).stdout.splitlines())
    assert int(vals.pop("size")) == ctypes.sizeof(x.Mb444)
    for n in names:
        assert getattr(x.Mb444, n).offset == int(vals[n]), n
    assert x.Mb444.luma_dc.offset + 8 == ctypes.sizeof(x.Mb444)
    assert x.Mb444.fenc.size == x.Mb444.pred.size == x.Mb444.recon.size == 24


_TABLE = np.minimum(np.arange(64), 39).astype(np.uint8)
EINVAL, ENODEV = -1, -3
_COMMON = ("chroma_qp_table", "quant4_mf", "quant4_bias", "dequant4_mf", "qp", "mb_flags", "level", "nnz", "cbp", "nz",
           "flags_out")
_PLANES = ("fenc", "pred", "recon")


def _e(x, **kw):
    """a valid x264hip_mb444_t on made-up addresses"""
    e = x.Mb444()
    e.b_dct_decimate = 1
    e.chroma_qp_table = _TABLE.ctypes.data
    k = 0
    for n, t in x.Mb444._fields_:
        if n in ("b_dct_decimate", "chroma_qp_table"):
            continue
        if n.endswith("_frame_stride"):
            setattr(e, n, 192 * 128)
        elif n.endswith("_stride"):
            setattr(e, n, 192)
        elif n in _PLANES:
            for p in range(3):
                getattr(e, n)[p] = 0x40000000 + 0x1000000 * k
                k += 1
        else:
            setattr(e, n, 0x40000000 + 0x1000000 * k)
            k += 1
    for name, v in kw.items():
        if isinstance(name, str) and "[" in name:
            getattr(e, name[:-3])[int(name[-2])] = v
        else:
            setattr(e, name, v)
    return e


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("which", ["inter", "intra"])
def test_mb_encode_444_argument_errors(bd, which):
    """every argument error is X264HIP_EINVAL before any HIP call (no device pointer is dereferenced)"""
    ensure_built("hip")
    x = load_package()
    fn = getattr(x.lib(), f"x264hip_{bd}_mb_encode_{which}_444")
    intra = which == "intra"

    def call(e, mbw=5, mbh=4, n=2):
        return fn(ctypes.byref(e) if e is not None else None, mbw, mbh, n, None)

    assert call(None) == EINVAL
    for field in _COMMON:
        assert call(_e(x, **{field: None})) == EINVAL, field
    for p in range(3):
        assert call(_e(x, **{f"fenc[{p}]": None})) == EINVAL and call(_e(x, **{f"recon[{p}]": None})) == EINVAL, p
        # the field of the other entry is not looked at
        assert call(_e(x, **{f"pred[{p}]": None}), n=0) == (0 if intra else EINVAL), p
    for field in ("pred_mode", "luma_dc"):
        assert call(_e(x, **{field: None}), n=0) == (EINVAL if intra else 0), field
    for field in ("quant8_mf", "quant8_bias", "dequant8_mf"):     # together or not at all
        assert call(_e(x, **{field: None})) == EINVAL, field
    assert call(_e(x), mbw=-1) == EINVAL and call(_e(x), mbh=-1) == EINVAL and call(_e(x), n=-1) == EINVAL
    assert call(_e(x), mbw=1 << 15, mbh=1 << 14, n=1) == EINVAL                      # more than 2^28 MBs
    for field in ("recon_stride", "recon_frame_stride", "recon_chroma_stride", "recon_chroma_frame_stride"):
        assert call(_e(x, **{field: 190})) == EINVAL, field
    px = 1 if bd == 8 else 2
    for p in range(3):
        assert call(_e(x, **{f"recon[{p}]": 0x40000000 + 2 * px})) == EINVAL, p
    co = 2 if bd == 8 else 4
    assert call(_e(x, level=0x40000000 + co // 2)) == EINVAL and call(_e(x, cbp=0x40000002)) == EINVAL
    assert call(_e(x, nz=0x40000002)) == EINVAL
    assert call(_e(x, luma_dc=0x40000000 + co // 2), n=0) == (EINVAL if intra else 0)
    bad = _TABLE.copy()
    bad[7] = 52 + 6 * (bd - 8)
    assert call(_e(x, chroma_qp_table=bad.ctypes.data)) == EINVAL
    # nothing to do is OK without a launch (and without a device); errors stay errors
    e = _e(x)
    assert call(e, n=0) == 0 and call(e, mbw=0) == 0 and call(e, mbh=0) == 0
    e.quant8_mf = e.quant8_bias = e.dequant8_mf = None
    assert call(e, n=0) == 0
    assert call(_e(x, qp=None), n=0) == EINVAL and call(None, n=0) == EINVAL
    if not x.lib().x264hip_available():
        assert call(_e(x)) == ENODEV


def test_existing_entries_still_refuse_444():
    """chroma_format 3 stays X264HIP_EINVAL in x264hip_*_mb_encode_inter / _intra"""
    import test_cpu_mbenc as t
    x = load_package()
    for bd in (8, 10):
        assert getattr(x.lib(), f"x264hip_{bd}_mb_encode_inter")(ctypes.byref(t._e(x, cf=3)), 5, 4, 2, None) == EINVAL


def test_wrapper_refusals_need_no_device():
    import torch
    x = load_package()
    y = torch.zeros((1, 16, 16), dtype=torch.uint8)
    pic = ((y, 0, 16, 256), ([y, y], 0, 16, 256))
    q = (torch.zeros(1, dtype=torch.int16), torch.zeros(1, dtype=torch.int16))
    dq = torch.zeros(1, dtype=torch.int32)
    qp, fl = torch.zeros(1, dtype=torch.int8), torch.zeros(1, dtype=torch.uint8)
    pm = torch.zeros(16, dtype=torch.int8)
    inter = dict(fenc=pic, pred=pic, mb_width=1, mb_height=1, nframes=1, qp=qp, mb_flags=fl, quant4=q, dequant4_mf=dq)
    intra = dict(fenc=pic, recon=pic, mb_width=1, mb_height=1, nframes=1, qp=qp, mb_flags=fl, pred_mode=pm, quant4=q,
                 dequant4_mf=dq)
    for fn, ok in ((x.mb_encode_inter_444, inter), (x.mb_encode_intra_444, intra)):
        with pytest.raises(ValueError, match=r"\(luma, chroma\)"):
            fn(**{**ok, "fenc": (y, 0, 16, 256)})
        with pytest.raises(ValueError, match=r"\(luma, chroma\)"):
            fn(**{**ok, "fenc": ((y, 0, 16, 256), ([y], 0, 16, 256))})
        with pytest.raises(ValueError, match="come together"):
            fn(**ok, quant8=q)
        with pytest.raises(ValueError, match="negative"):
            fn(**{**ok, "nframes": -1})
        with pytest.raises(ValueError, match="QP_MAX_SPEC"):
            fn(**ok, qp_table=np.zeros(51, np.uint8))
        with pytest.raises(ValueError, match="one element per macroblock"):
            fn(**{**ok, "mb_width": 2})
        with pytest.raises(ValueError, match="level"):
            fn(**ok, outs={"level": torch.zeros(4, dtype=torch.int16)})
        with pytest.raises(ValueError, match="luma_dc"):
            fn(**ok, outs={"luma_dc": torch.zeros((1, 16), dtype=torch.int16)})
        with pytest.raises(TypeError, match="bit depth"):
            fn(**{**ok, "fenc": ((y, 0, 16, 256), ([y, y.to(torch.int16)], 0, 16, 256))})
    with pytest.raises(ValueError, match="pred_mode"):
        x.mb_encode_intra_444(**{**intra, "pred_mode": pm[:8]})


# ------------------------------------------------------------------ 5. coverage of the committed seed
def _inter_conditions(bd, t8):
    """the cross-plane conditions over the inter macroblocks of one transform size, dec = 1"""
    c = collections.Counter()
    for key in m4.case_keys(bd):
        case, out = m4.make_case(*key), m4.expected(key, 1)
        for mb, rec in out.rec.items():
            if bool(case.flags[mb] & m4.T8) != t8:
                continue
            c["coded"] += 1
            kept = [r.cbp != 0 for r in rec]
            for p in (1, 2):
                c[f"carried_{p}"] += kept[p] and rec[p].own < 6
            c["first_dropped_later_kept"] += rec[0].nonzero and not kept[0] and (kept[1] or kept[2])
            c["all_dropped"] += all(r.nonzero for r in rec) and not any(kept)
            c["all_kept"] += all(kept)
            c["part_in_kept"] += any(r.part for r in rec)
            c["chroma_only"] += not kept[0] and (kept[1] or kept[2])
            c["cbp"] += any(kept)
    return c


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("t8", [False, True])
def test_inter_inputs_reach_the_cross_plane_rule(bd, t8):
    c = _inter_conditions(bd, t8)
    for name in ("carried_1", "carried_2", "first_dropped_later_kept", "all_dropped", "all_kept", "part_in_kept"):
        assert c[name] >= 1, (name, dict(c))
    assert c["chroma_only"] * 10 >= c["coded"] and c["cbp"] * 2 >= c["coded"], dict(c)


@pytest.mark.parametrize("bd", [8, 10])
def test_intra_inputs_reach_every_arm_in_u_and_v(bd):
    cnt = {0: collections.Counter(), 1: collections.Counter()}
    for key in m4.case_keys(bd):
        for dec in (0, 1):
            cnt[dec].update(m4.expected(key, dec).counters)
    both = cnt[0] + cnt[1]
    for p in (1, 2):
        for m in range(12):
            assert both[p, ("mode4", m)] and both[p, ("mode8", m)], (p, m)
        for m in range(7):
            assert both[p, ("mode16", m)], (p, m)
        for arm in ("i16_idct_dc", "i16_idct_nodc", "i16_dc_only", "i16_pred_only", "topright_emulated", "topright_real"):
            assert both[p, arm], (p, arm)
        assert cnt[1][p, "i16_decimated"] and not cnt[0][p, "i16_decimated"], p
        for side in (False, True):
            assert both[p, ("have_lt", side)] and both[p, ("have_tr", side)], (p, side)
    for t in ("i4", "i8", "i16"):
        assert both["type", t], t
    assert both["intra_coded"] * 10 >= both["intra"] > 0


@pytest.mark.parametrize("bd", [8, 10])
def test_a_wrong_category_changes_the_outputs(bd):
    """with the distinct matrices, reading CQM_xPY for CQM_xPC (CQM_xIY for CQM_xIC) changes some
    macroblock of every kind: inter and intra, both transform sizes"""
    changed = collections.Counter()
    for key in m4.DISTINCT_KEYS(bd):
        case, good = m4.make_case(*key), m4.expected(key, 1)
        bad = m4.encode(case, 1, T=m4.tables(bd, "distinct", luma_only=True))
        differ = (good.level != bad.level).any(axis=(1, 2)) | (good.luma_dc != bad.luma_dc).any(axis=(1, 2))
        for p in range(3):
            d = (good.recon[p] != bad.recon[p]).reshape(case.nframes, case.mbh, 16, case.mbw, 16).any(axis=(2, 4))
            differ |= d.reshape(-1)
            assert p or np.array_equal(good.recon[0], bad.recon[0])       # plane 0 reads the luma categories
        for mb in np.flatnonzero(differ):
            fl = int(case.flags[mb])
            changed["intra" if fl & m4.INTRA else "inter", bool(fl & m4.T8)] += 1
    for kind in ("inter", "intra"):
        for t8 in (False, True):
            assert changed[kind, t8] >= 1, (kind, t8, dict(changed))


@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_keys_reach_the_running_score_on_both_sides_of_6(bd):
    """over what tests/test_gpu_mb444.py runs with decimation, the score that runs on through the
    planes ends a plane below 6, above 6 and exactly at 6 with either transform, and the boundary
    picture has it at 6 after each of the three planes"""
    seen = set()
    for key, dec in m4.gpu_keys(bd=bd, dec=1):
        case, out = m4.make_case(*key), m4.expected(key, dec)
        for mb, rec in out.rec.items():
            run = 0
            for p in range(3):
                run += rec[p].own
                if rec[p].nonzero:
                    seen.add((bool(case.flags[mb] & m4.T8), (run > 6) - (run < 6), key in m4.boundary_keys(), p))
    for t8 in (False, True):
        assert {(t8, -1), (t8, 0), (t8, 1)} <= {s[:2] for s in seen}, t8
        assert {(t8, 0, True, p) for p in range(3)} <= seen, t8
    # and once through a carry: the 6 is what an earlier plane left plus the plane's own
    for key in m4.boundary_keys():
        if key[0] == bd:
            owns = [[r.own for r in rec] for rec in m4.expected(key, 1).rec.values()]
            assert any(0 < o[0] and o[1] == 0 and 0 < o[2] < 6 and sum(o) == 6 for o in owns), owns


def test_gpu_keys_are_the_groups_of_the_gpu_tests():
    """the parametrised selections of tests/test_gpu_mb444.py add up to gpu_keys(), nothing twice"""
    picked = [kd for bd in (8, 10) for dec in (0, 1) for kd in m4.gpu_keys("shapes", bd=bd, dec=dec)]
    picked += [kd for bd in (8, 10) for kd in m4.gpu_keys("distinct", bd=bd)] + m4.gpu_keys("boundary")
    assert sorted(map(repr, picked)) == sorted(map(repr, m4.gpu_keys())) and len(set(picked)) == len(picked)


def test_case_lists():
    keys = m4.case_keys(8)
    assert {k[1:4] for k in keys} == set(m4.SHAPES) and m4.SHAPES[-1] == (7, 3, 3)
    case = m4.make_case(8, 7, 3, 3)
    fl = case.flags
    for bit in (m4.INTRA, m4.T8, m4.D16, m4.SKIP):
        assert (fl & bit).any() and not (fl & bit).all()
    assert (case.klass[:, 0] == m4.CARRY).any() and (case.qp[case.klass[:, 0] == m4.CARRY] >= 24).all()
    assert m4.make_case(8, 7, 3, 3, "flat", m4.SEED, True).flags.all()
    # the recipe of the CARRY class: own-plane scores (3, 4|5, 0|3) in some order
    ok = 0
    for key in (keys[2], keys[3]):
        c, out = m4.make_case(*key), m4.expected(key, 1)
        for mb in np.flatnonzero(c.klass[:, 0] == m4.CARRY):
            own = sorted(r.own for r in out.rec[mb])
            ok += own in ([0, 3, 4], [0, 3, 5], [3, 3, 4], [3, 3, 5])
    assert ok >= 4
