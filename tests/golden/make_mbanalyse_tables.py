#!/usr/bin/env python3
"""Regenerates tests/golden/mbanalyse_tables.json — TEST INFRASTRUCTURE.

Reads the reference's common/tables.c, common/predict.h, common/macroblock.h and
encoder/analyse.c as text and records the numbers the intra mode decision reads:
x264_lambda_tab; i16x16_mode_available, chroma_mode_available, i8x8_mode_available[0],
i4x4_mode_available[0] (rows flattened, -1 padding kept); intra_analysis_shortcut[0];
i16x16_thresh_lut, i8x8_thresh, cost_div_fix8; the I_4x4, I_8x8 and I_16x16 entries of
i_mb_b_cost_table; x264_mb_pred_mode16x16_fix and x264_mb_chroma_pred_mode_fix.  The mode names of
the initialisers are resolved through the enums of common/predict.h.
tests/test_cpu_mbanalyse.py pins the product's copy (x264-i386pic_amd/csrc/mbanalysedev.h) and the
checker's (tests/mbanalyse_cases.py) to them.

Only these numbers are committed; the tests read the .json and never need the reference.

usage: python tests/golden/make_mbanalyse_tables.py REFERENCE_DIR
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def strip(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def enums(src):
    """{name: value} of every enum of the text (values given or counted up)"""
    out = {}
    for body in re.findall(r"\benum\s+\w*\s*\{(.*?)\}", strip(src), flags=re.S):
        v = -1
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            m = re.match(r"(\w+)\s*(?:=\s*(-?\w+))?$", item)
            assert m, item
            g = m.group(2)
            v = v + 1 if g is None else out[g] if g in out else int(g, 0)
            out[m.group(1)] = v
    return out


def array(src, name, names):
    """the entries of the brace initialiser of array `name`, flattened, identifiers through names"""
    src = strip(src)
    m = re.search(r"\b" + re.escape(name) + r"\s*(?:\[[^\]]*\]\s*)+=\s*\{", src)
    assert m, name
    i = j = m.end() - 1
    depth = 0
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            break
        j += 1
    return [int(t) if re.match(r"-?\d+$", t) else names[t] for t in re.findall(r"-?\w+", src[i:j + 1])]


def tables(ref):
    rd = lambda *p: open(os.path.join(ref, *p)).read()
    predict_h, analyse_c = rd("common", "predict.h"), rd("encoder", "analyse.c")
    names = enums(predict_h)
    mbtype = enums(rd("common", "macroblock.h"))
    out = {"x264_lambda_tab": array(rd("common", "tables.c"), "x264_lambda_tab", {})}
    out["i16x16_mode_available"] = array(analyse_c, "i16x16_mode_available", names)
    out["chroma_mode_available"] = array(analyse_c, "chroma_mode_available", names)
    out["i8x8_mode_available0"] = array(analyse_c, "i8x8_mode_available", names)[:50]
    out["i4x4_mode_available0"] = array(analyse_c, "i4x4_mode_available", names)[:50]
    out["intra_analysis_shortcut0"] = array(analyse_c, "intra_analysis_shortcut", names)[:20]
    for n in ("i16x16_thresh_lut", "i8x8_thresh", "cost_div_fix8"):
        out[n] = array(analyse_c, n, {})
    cost = array(analyse_c, "i_mb_b_cost_table", {})
    out["i_mb_b_cost_intra"] = [cost[mbtype[t]] for t in ("I_4x4", "I_8x8", "I_16x16")]
    out["x264_mb_pred_mode16x16_fix"] = array(predict_h, "x264_mb_pred_mode16x16_fix", names)
    out["x264_mb_chroma_pred_mode_fix"] = array(predict_h, "x264_mb_chroma_pred_mode_fix", names)
    sizes = {"x264_lambda_tab": 82, "i16x16_mode_available": 25, "chroma_mode_available": 25, "i8x8_mode_available0": 50,
             "i4x4_mode_available0": 50, "intra_analysis_shortcut0": 20, "i16x16_thresh_lut": 11, "i8x8_thresh": 11,
             "cost_div_fix8": 3, "i_mb_b_cost_intra": 3, "x264_mb_pred_mode16x16_fix": 7, "x264_mb_chroma_pred_mode_fix": 7}
    for n, k in sizes.items():
        assert len(out[n]) == k, (n, len(out[n]))
    return out


def main(ref):
    with open(os.path.join(HERE, "mbanalyse_tables.json"), "w") as fh:
        json.dump(tables(ref), fh, indent=None, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
