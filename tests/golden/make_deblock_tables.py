#!/usr/bin/env python3
"""Regenerates tests/golden/deblock_tables.json — TEST INFRASTRUCTURE.

Reads the reference's common/deblock.c as text and records the integers of the three tables of
the deblocking filter (i_alpha_table[88], i_beta_table[88], i_tc0_table[88][4], indexed by
qp + offset + 24).  tests/test_cpu_deblock.py pins the product's copy
(x264-i386pic_amd/csrc/deblock.hip) and the checker's (tests/deblock_cases.py) to them.

Only these numbers are committed; the tests read the .json and never need the reference.

usage: python tests/golden/make_deblock_tables.py REFERENCE_DIR
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {"i_alpha_table": 88, "i_beta_table": 88, "i_tc0_table": 88 * 4}


def int_array(src, name):
    """the integers of the brace initialiser of array `name`, in order (comments stripped)"""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    m = re.search(r"\b" + re.escape(name) + r"\s*(?:\[[^\]]*\]\s*)+=\s*\{", src)
    assert m, name
    i = j = m.end() - 1
    depth = 0
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            break
        j += 1
    return [int(v) for v in re.findall(r"-?\d+", src[i:j + 1])]


def tables(ref):
    src = open(os.path.join(ref, "common", "deblock.c")).read()
    out = {name: int_array(src, name) for name in NAMES}
    for name, n in NAMES.items():
        assert len(out[name]) == n, (name, len(out[name]))
    return out


def main(ref):
    with open(os.path.join(HERE, "deblock_tables.json"), "w") as fh:
        json.dump(tables(ref), fh, indent=None, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
