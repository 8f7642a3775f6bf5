#!/usr/bin/env python3
"""Regenerates tests/golden/intra4x4_golden.npz — TEST INFRASTRUCTURE.

Pins the closed-form 4x4 directional intra predictors (tests/mbintra_cases.py pred4x4_dir and
csrc/mbintra.hip pred4x4: DDL, DDR, VR, HD, VL, HU) against the reference's own per-pixel
assignment lists in common/predict.c:534-630.  As make_intra_golden.py, this script reads that
file as text: every `SRC(x,y)=...= F1/F2(...)` statement of the six functions is turned into a
table "pixel (x,y) of mode m is F1/F2 of these neighbours", and the tables are evaluated on seeded
random and extreme neighbours.  Only the resulting data (neighbours and predicted blocks) is
committed; the tests read the .npz and never the reference.

The 13 neighbours: t0..t7 at 0..7 (top and top-right), l0..l3 at 8..11, lt at 12.

usage: python tests/golden/make_intra4x4_golden.py <reference>/common/predict.c
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("ddl", "ddr", "vr", "hd", "vl", "hu")   # I_PRED_4x4_DDL .. I_PRED_4x4_HU = 3 .. 8


def neighbour_index(name):
    if name == "lt":
        return 12
    return (8 if name[0] == "l" else 0) + int(name[1:])


def parse_term(term):
    """'F2(a,b,c)' / 'F1(a,b)' / 'l3' -> (kind, [neighbour indices])"""
    term = term.strip()
    m = re.fullmatch(r"(F[12])\((.*)\)", term)
    if m:
        return m.group(1), [neighbour_index(a.strip()) for a in m.group(2).split(",")]
    return "id", [neighbour_index(term)]


def mode_table(text, name):
    """{(x, y): (kind, indices)} for predict_4x4_<name>_c; a statement may run over two lines"""
    body = text[text.index(f"static void predict_4x4_{name}_c"):]
    body = body[:body.index("\n}\n")]
    table = {}
    body = re.sub(r"PREDICT_4x4_LOAD_\w+", "", body)             # (the neighbour loads: no semicolon)
    body = body[body.index("{") + 1:]
    for stmt in (s.strip() for s in body.replace("\n", " ").split(";")):
        if stmt.startswith("SRC("):                              # (not `int lt = SRC(-1,-1)`)
            lhs, rhs = stmt.rsplit("=", 1)
            for xs, ys in re.findall(r"SRC\((\d),(\d)\)", lhs):
                table[(int(xs), int(ys))] = parse_term(rhs)
    assert len(table) == 16, (name, len(table))
    return table


def evaluate(table, n):
    out = np.zeros((4, 4), np.int64)
    for (x, y), (kind, idx) in table.items():
        v = [int(n[i]) for i in idx]
        out[y, x] = (v[0] if kind == "id" else (v[0] + v[1] + 1) >> 1 if kind == "F1"
                     else (v[0] + 2 * v[1] + v[2] + 2) >> 2)
    return out


def main():
    text = open(sys.argv[1]).read()
    text = text[text.index("static void predict_4x4_ddl_c"):text.index("8x8 prediction for intra luma block")]
    tables = [mode_table(text, m) for m in MODES]
    rs = np.random.default_rng(20261020)
    data = {}
    for bd in (8, 10):
        n = 64
        nb = rs.integers(0, 1 << bd, size=(n, 13)).astype(np.uint16)
        nb[0] = 0
        nb[1] = (1 << bd) - 1
        nb[2, ::2] = (1 << bd) - 1          # alternating extremes stress the rounding
        nb[3, 1::2] = (1 << bd) - 1
        pred = np.zeros((n, len(MODES), 4, 4), np.uint16)
        for i in range(n):
            for k, t in enumerate(tables):
                pred[i, k] = evaluate(t, nb[i])
        data[f"neighbours_{bd}"] = nb
        data[f"pred_{bd}"] = pred
    np.savez_compressed(os.path.join(HERE, "intra4x4_golden.npz"), **data)
    print("wrote intra4x4_golden.npz")


if __name__ == "__main__":
    main()
