"""CPU: the constant tables the oracle and the product restate, pinned to the reference's
own text.  Parity of the arithmetic stays unpinned (the reference
cannot be built here), but every table both sides copied from it is
checked value for value against the reference source's numbers, recorded from its text in
tests/golden/ref_tables.json (tests/golden/make_ref_tables.py):

* common/set.c:31-71        dequant4/8_scale, quant4/8_scale, quant8_scan
* common/tables.c:183-184   x264_hpel_ref0 / x264_hpel_ref1
* encoder/me.c:53-56        mod6m1, hex2, square1
* common/dct.c:768-816      the 8x8 / 4x4 frame and field zigzag scans (ZIG(i,y,x) lists)
"""
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ORACLE = os.path.join(ROOT, "oracle", "oracle.c")
CSRC = os.path.join(ROOT, "x264-i386pic_amd", "csrc")


def _text(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def c_array(path, name, nth=0):
    """Integers of the brace initialiser of array `name` in a C/C++/HIP file (comments
    stripped), in order; `nth` picks among several definitions of the name."""
    src = _text(path)
    hits = [m for m in re.finditer(r"\b" + re.escape(name) + r"\s*(?:\[[^\]]*\]\s*)+=\s*\{", src)]
    assert len(hits) > nth, (path, name)
    i = hits[nth].end() - 1
    depth, j = 0, i
    while True:
        if src[j] == "{":
            depth += 1
        elif src[j] == "}":
            depth -= 1
            if depth == 0:
                break
        j += 1
    return [int(v) for v in re.findall(r"-?\d+", src[i:j + 1])]


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "ref_tables.json")) as fh:
        return json.load(fh)


def ref_array(name):
    """Integers of the reference's constant table `name`, as recorded."""
    return list(_golden()["arrays"][name])


def zig_macro(name):
    """(y, x) pairs of dct.c's ZIGZAG macro `name` in scan order, as recorded."""
    return list(_golden()["zigzag"][name])


@pytest.mark.parametrize("ref_name,ours", [
    ("dequant4_scale", [(ORACLE, "dequant4_scale"), (os.path.join(CSRC, "capi.cpp"), "k_dequant4_scale")]),
    ("dequant8_scale", [(ORACLE, "dequant8_scale"), (os.path.join(CSRC, "capi.cpp"), "k_dequant8_scale")]),
    ("quant4_scale", [(ORACLE, "quant4_scale"), (os.path.join(CSRC, "capi.cpp"), "k_quant4_scale")]),
    ("quant8_scale", [(ORACLE, "quant8_scale"), (os.path.join(CSRC, "capi.cpp"), "k_quant8_scale")]),
    ("quant8_scan", [(ORACLE, "quant8_scan"), (os.path.join(CSRC, "capi.cpp"), "k_quant8_scan"),
                     (os.path.join(CSRC, "capi.cpp"), "k_quant8_scan16")]),
])
def test_cqm_scale_tables(ref_name, ours):
    want = ref_array(ref_name)
    assert len(want) in (16, 18, 36)
    for path, name in ours:
        assert c_array(path, name) == want, (path, name)


def test_hpel_ref_tables():
    for k in (0, 1):
        want = ref_array("x264_hpel_ref%d" % k)
        assert len(want) == 16
        assert c_array(ORACLE, "hpel_ref%d" % k) == want
        assert c_array(os.path.join(CSRC, "mcdev.h"), "c_ref%d" % k) == want


def test_me_pattern_tables():
    la = os.path.join(CSRC, "hipcommon.h")
    for ref_name, orc_name, hip_name, n in (("mod6m1", "lr_mod6m1", "c_mod6m1", 8),
                                           ("hex2", "lr_hex2", "c_hex2", 16),
                                           ("square1", "lr_square1", "c_square1", 18)):
        want = ref_array(ref_name)
        assert len(want) == n
        assert c_array(ORACLE, orc_name) == want, orc_name
        assert c_array(la, hip_name) == want, hip_name


def brace_lists(path):
    """Integers of every brace initialiser of a file that holds numbers only (comments
    stripped; nested groups flattened, each inner group also on its own)."""
    src = _text(path)
    out = []
    for m in re.finditer(r"\{", src):
        depth, j = 0, m.start()
        while j < len(src):
            if src[j] == "{":
                depth += 1
            elif src[j] == "}":
                depth -= 1
                if depth == 0:
                    break
            j += 1
        body = src[m.start():j + 1]
        if re.fullmatch(r"[\s\d,{}+-]*", body):
            out.append([int(v) for v in re.findall(r"-?\d+", body)])
    return out


def test_single_copies_of_small_tables():
    """The hpel_ref tables live in csrc/mcdev.h and the search patterns in csrc/hipcommon.h, once:
    no other file under csrc/ restates one of them as a brace initialiser."""
    owner = {"x264_hpel_ref0": "mcdev.h", "x264_hpel_ref1": "mcdev.h", "hex2": "hipcommon.h",
             "mod6m1": "hipcommon.h", "square1": "hipcommon.h"}
    want = {name: ref_array(name) for name in owner}
    seen = {name: 0 for name in owner}
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if not os.path.isfile(path) or not fn.endswith((".hip", ".h", ".cpp", ".inc")):
            continue
        for lst in brace_lists(path):
            for name, w in want.items():
                if lst == w:
                    assert fn == owner[name], (fn, name)
                    seen[name] += 1
    assert all(n == 1 for n in seen.values()), seen


def test_zigzag_scans():
    f8, d8 = zig_macro("ZIGZAG8_FRAME"), zig_macro("ZIGZAG8_FIELD")
    f4, d4 = zig_macro("ZIGZAG4_FRAME"), zig_macro("ZIGZAG4_FIELD")
    assert len(f8) == len(d8) == 128 and len(f4) == len(d4) == 32
    assert c_array(ORACLE, "zz8_frame") == f8
    assert c_array(ORACLE, "zz8_field") == d8
    assert c_array(ORACLE, "zz4_frame") == f4
    assert c_array(ORACLE, "zz4_field") == d4
    idct = os.path.join(CSRC, "idct.hip")
    assert c_array(idct, "c_zz8") == f8 + d8
    assert c_array(idct, "c_zz4") == f4 + d4
    assert c_array(idct, "yx", 0) == f8 + d8           # ZZ<8, FIELD>'s compile-time copy
    assert c_array(idct, "yx", 1) == f4 + d4           # ZZ<4, FIELD>
    # every scan is a permutation of the block
    for t, w in ((f8, 8), (d8, 8), (f4, 4), (d4, 4)):
        pos = np.array(t).reshape(-1, 2)
        assert len({(y, x) for y, x in pos}) == w * w


def test_zigzag_4x4_field_copy_regions():
    """zigzag_scan_4x4_field (dct.c:835-841) copies level[0..1] and [6..15] straight from
    dct and permutes 2..5: the ZIGZAG4_FIELD list agrees, i.e. dct[x*4+y] == index i there."""
    d4 = np.array(zig_macro("ZIGZAG4_FIELD")).reshape(-1, 2)
    for i in list(range(2)) + list(range(6, 16)):
        y, x = d4[i]
        assert x * 4 + y == i


def test_jvt_cqm_lists():
    """The JVT default scaling lists the checkasm CQM cases use (tests/checkasm_bufs.py,
    checkasm.c:2098-2113) equal common/tables.c:191-226."""
    import checkasm_bufs as cb
    for ours, name in ((cb.JVT4I, "x264_cqm_jvt4i"), (cb.JVT4P, "x264_cqm_jvt4p"), (cb.JVT8I, "x264_cqm_jvt8i"),
                       (cb.JVT8P, "x264_cqm_jvt8p")):
        assert list(ours) == ref_array(name), name
