#!/usr/bin/env python3
"""Regenerates tests/golden/mbenc_tables.json — TEST INFRASTRUCTURE.

Reads the reference's common/tables.c as text and records the integers of x264_lambda2_tab
(QP_MAX_MAX + 1 = 82 entries), which the chroma early termination of the inter macroblock encode
reads (encoder/macroblock.c:285).  tests/test_cpu_mbenc.py pins the product's copy
(x264-i386pic_amd/csrc/mbenc.hip) and the checker's (tests/mbenc_cases.py) to them.

Only these numbers are committed; the tests read the .json and never need the reference.

usage: python tests/golden/make_mbenc_tables.py REFERENCE_DIR
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_deblock_tables import int_array  # noqa: E402

NAMES = {"x264_lambda2_tab": 82}


def tables(ref):
    src = open(os.path.join(ref, "common", "tables.c")).read()
    out = {name: int_array(src, name) for name in NAMES}
    for name, n in NAMES.items():
        assert len(out[name]) == n, (name, len(out[name]))
    return out


def main(ref):
    with open(os.path.join(HERE, "mbenc_tables.json"), "w") as fh:
        json.dump(tables(ref), fh, indent=None, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
