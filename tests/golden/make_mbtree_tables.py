#!/usr/bin/env python3
"""Regenerates tests/golden/mbtree_tables.json — TEST INFRASTRUCTURE.

Reads the reference's common/tables.c as text and records, as decimal strings exactly as written
there, the two tables of x264_log2 (x264_log2_lut[128], x264_log2_lz_lut[32]) that
macroblock_tree_finish reads.  tests/test_cpu_mbtree.py pins the product's copy
(x264-i386pic_amd/csrc/mbtree.hip) and the checker's (tests/mbtree_cases.py) to them.

Only these numbers are committed; the tests read the .json and never the reference.

usage: python tests/golden/make_mbtree_tables.py REFERENCE_DIR
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("x264_log2_lut", "x264_log2_lz_lut")


def float_array(src, name):
    """the literals of the brace initialiser of float array `name`, as written (comments stripped)"""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    m = re.search(r"\b" + re.escape(name) + r"\s*\[[^\]]*\]\s*=\s*\{([^{}]*)\}", src)
    assert m, name
    return re.findall(r"-?\d+(?:\.\d+)?", m.group(1))


def main(ref):
    src = open(os.path.join(ref, "common", "tables.c")).read()
    out = {name: float_array(src, name) for name in NAMES}
    with open(os.path.join(HERE, "mbtree_tables.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
