#!/usr/bin/env python3
"""Regenerates tests/golden/ref_tables.json — TEST INFRASTRUCTURE.

Reads the reference's sources as text and records, as plain data, what
tests/test_ref_tables.py and tests/test_abi.py pin the project to:

* "arrays":  the integers of the constant tables (common/set.c quant / dequant scales,
             common/tables.c hpel_ref and the JVT scaling lists, encoder/me.c search patterns);
* "zigzag":  the (y, x) pairs of common/dct.c's ZIGZAG macros in scan order;
* "structs": the ordered (field name, array extent) lists of the function tables in
             common/pixel.h, dct.h and quant.h.

Only these numbers and names are committed; the tests read the .json and never the reference.

usage: python tests/golden/make_ref_tables.py REFERENCE_DIR
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_abi import _struct_fields  # noqa: E402
from test_ref_tables import c_array  # noqa: E402

ARRAYS = (("common/set.c", ("dequant4_scale", "dequant8_scale", "quant4_scale", "quant8_scale", "quant8_scan")),
          ("common/tables.c", ("x264_hpel_ref0", "x264_hpel_ref1", "x264_cqm_jvt4i", "x264_cqm_jvt4p",
                               "x264_cqm_jvt8i", "x264_cqm_jvt8p")),
          ("encoder/me.c", ("mod6m1", "hex2", "square1")))
ZIGZAG = ("ZIGZAG8_FRAME", "ZIGZAG8_FIELD", "ZIGZAG4_FRAME", "ZIGZAG4_FIELD")
STRUCTS = (("pixel.h", "x264_pixel_function_t"), ("dct.h", "x264_dct_function_t"),
           ("dct.h", "x264_zigzag_function_t"), ("quant.h", "x264_quant_function_t"))


def zig_macro(src, name):
    """(y, x) pairs of dct.c's ZIGZAG macro `name` in scan order (ZIG / ZIGDC(i,y,x))."""
    m = re.search(r"#define " + name + r"\\\n((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, name
    items = re.findall(r"ZIG(?:DC)?\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))
    items = sorted((int(i), int(y), int(x)) for i, y, x in items)
    assert [i for i, _, _ in items] == list(range(len(items)))
    return [v for _, y, x in items for v in (y, x)]


def ref_struct(path, tname):
    src = open(path).read()
    m = re.search(r"typedef struct\s*\{([^{}]*)\}\s*" + tname + r"\s*;", src, re.S)
    assert m, tname
    return [list(f) for f in _struct_fields(m.group(1))]


def main(ref):
    out = {"arrays": {}, "zigzag": {}, "structs": {}}
    for rel, names in ARRAYS:
        for name in names:
            out["arrays"][name] = c_array(os.path.join(ref, rel), name)
    dct = open(os.path.join(ref, "common", "dct.c")).read()
    for name in ZIGZAG:
        out["zigzag"][name] = zig_macro(dct, name)
    for rel, tname in STRUCTS:
        out["structs"][tname] = ref_struct(os.path.join(ref, "common", rel), tname)
    with open(os.path.join(HERE, "ref_tables.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
