"""Boundary mutants of the Python checkers (tests/*_cases.py).  No GPU code.

A mutant is a checker module with one ordering comparison flipped at its boundary (`<` <-> `<=`,
`>` <-> `>=`): the checker a kernel would agree with if it restated that one comparison of the
reference the wrong way at equality.  tests/test_cpu_mutants.py asks that for every mutant some case
the GPU tests run (the module's gpu_keys()) gives other expected bytes, which is what makes the GPU
byte comparison able to see such a kernel.

sites(name)        the comparisons of module `name` that get a mutant, in source order
load(name, site)   the module executed in a namespace of its own with that site flipped (its
                   lru_caches are its own); the INPUTS functions of EXCLUDED_FUNCTIONS are the unmutated module's,
                   so a mutant is fed the inputs the GPU tests feed the device
differs(a, b)      whether two results of expected() differ in any ndarray field

What is left out of the mutant set is named here by function or by statement kind, never by line.
"""
import ast
import collections
import importlib
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLIP = {ast.Lt: ast.LtE, ast.LtE: ast.Lt, ast.Gt: ast.GtE, ast.GtE: ast.Gt}

# ------------------------------------------------------------------ the exclusions
# By function (with everything nested in it).  INPUTS build the cases: a mutant gets the unmutated
# module's, so that it is fed what the device is fed.  COUNTING only feeds the branch counters.
# UNREACHED are run by no expected(): the decoders the device's outputs are fed to and the like.
# chroma_qp_table (`q - bdo < 30`) counts as an input: the table it builds is handed to the device as
# well as to the checker, so a flip in it would change both sides alike.
INPUTS, COUNTING, UNREACHED = "inputs", "counting", "unreached"
EXCLUDED_FUNCTIONS = {
    "mbenc_cases": {
        "make_case": INPUTS, "_boundary_case": INPUTS, "boundary_recipe": INPUTS, "boundary_keys": INPUTS,
        "gpu_keys": INPUTS, "chroma_qp_table": INPUTS, "_side": COUNTING, "decode": UNREACHED, "_unzig": UNREACHED},
    "mbanalyse_cases": {
        "make_case": INPUTS, "_content": INPUTS, "case_keys": INPUTS, "make_key": INPUTS, "boundary_keys": INPUTS,
        "gpu_keys": INPUTS, "key_size": INPUTS, "i4x4_prefix_form": UNREACHED},
    "deblock_cases": {
        "make_case": INPUTS, "picture": INPUTS, "make_strength_case": INPUTS, "chroma_qp_table": INPUTS, "key": INPUTS,
        "boundary_keys": INPUTS, "gpu_keys": INPUTS, "key_size": INPUTS},
    "mbskip_cases": {
        "make_case": INPUTS, "make_field": INPUTS, "make_convert_case": INPUTS, "case_keys": INPUTS, "boundary_keys": INPUTS,
        "_boundary_case": INPUTS, "boundary_recipe": INPUTS, "gpu_keys": INPUTS, "key_size": INPUTS, "pskip_mv_scan8": UNREACHED, "probe_predicate": UNREACHED,
        "probe_by_predicate": UNREACHED},
    "mb444_cases": {
        "make_case": INPUTS, "_residual": INPUTS, "carry_levels": INPUTS, "inverse_of": INPUTS, "case_keys": INPUTS,
        "DISTINCT_KEYS": INPUTS, "boundary_keys": INPUTS, "_boundary_case": INPUTS, "gpu_keys": INPUTS,
        "decode": UNREACHED},
    "mbintra_cases": {
        "make_case": INPUTS, "_boundary_case": INPUTS, "boundary_keys": INPUTS, "case_keys": INPUTS, "all_intra_key": INPUTS,
        "jvt_keys": INPUTS, "gpu_keys": INPUTS, "key_size": INPUTS, "valid_modes": INPUTS, "decode": UNREACHED},
}


def _is_counter_update(stmt):
    """`cnt[...] += ...`: the statement only counts which arm ran"""
    if not (isinstance(stmt, ast.AugAssign) and isinstance(stmt.target, ast.Subscript)):
        return False
    v = stmt.target.value
    return (isinstance(v, ast.Name) and v.id == "cnt") or (isinstance(v, ast.Attribute) and v.attr == "counters")


def _is_record(stmt):
    """`rec.append(...)`: the statement only records what an arm did, for the CPU tests"""
    c = stmt.value if isinstance(stmt, ast.Expr) else None
    return (isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == "append" and
            isinstance(c.func.value, ast.Name) and c.func.value.id == "rec")


EXCLUDED_STATEMENTS = (("argument assertion", lambda s: isinstance(s, ast.Assert)),
                       ("branch counter", _is_counter_update), ("branch record", _is_record))

Site = collections.namedtuple("Site", "index lineno func text")


def _source(name):
    path = os.path.join(HERE, name + ".py")
    with open(path) as fh:
        return path, fh.read()


def _walk(tree, name):
    """(Compare node, operator index, enclosing function) of every site, in source order"""
    skip = EXCLUDED_FUNCTIONS.get(name, {})
    found = []

    def visit(node, funcs):
        if isinstance(node, (ast.FunctionDef, ast.Lambda)):
            fn = getattr(node, "name", "<lambda>")
            funcs = funcs + (fn,)
        if any(f in skip for f in funcs):
            return
        if isinstance(node, ast.stmt) and any(test(node) for _, test in EXCLUDED_STATEMENTS):
            return
        if isinstance(node, ast.Compare):
            for k, op in enumerate(node.ops):
                if type(op) in FLIP:
                    found.append((node, k, ".".join(funcs) or "<module>"))
        for child in ast.iter_child_nodes(node):
            visit(child, funcs)
    visit(tree, ())
    found.sort(key=lambda t: (t[0].lineno, t[0].col_offset, t[1]))
    return found


def sites(name):
    path, src = _source(name)
    return [Site(i, node.lineno, func, ast.get_source_segment(src, node))
            for i, (node, _, func) in enumerate(_walk(ast.parse(src, path), name))]


def load(name, site=None):
    """module `name` executed afresh, comparison `site` (an index of sites(name)) flipped"""
    path, src = _source(name)
    tree = ast.parse(src, path)
    if site is not None:
        node, k, _ = _walk(tree, name)[site]
        node.ops[k] = FLIP[type(node.ops[k])]()
    mod = types.ModuleType("%s_mutant_%s" % (name, site))
    mod.__file__ = path
    exec(compile(tree, path, "exec"), mod.__dict__)
    original = importlib.import_module(name)
    for fn, kind in EXCLUDED_FUNCTIONS.get(name, {}).items():
        if kind == INPUTS:
            setattr(mod, fn, getattr(original, fn))
    return mod


def differs(a, b):
    """any ndarray field of two results unequal (a field missing on one side counts)"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and
                    a.dtype == b.dtype and np.array_equal(a, b))
    if isinstance(a, (tuple, list)):
        return len(a) != len(b) or any(differs(x, y) for x, y in zip(a, b))
    if isinstance(a, types.SimpleNamespace):
        va, vb = vars(a), vars(b)
        return any(differs(v, vb.get(k)) for k, v in va.items() if isinstance(v, (np.ndarray, tuple, list)))
    return False


def first_kill(name, site, keys, call, original_result):
    """(key, how): the first of `keys` on which mutant `site` gives other bytes than the unmutated
    checker ("other bytes") or raises (the exception's type and text: a flipped bound check that
    reads outside a picture does), or (None, None).  call(module, key) computes the result."""
    mod = load(name, site)
    for key in keys:
        want = original_result(key)
        try:
            got = call(mod, key)
        except Exception as e:
            return key, "%s: %s" % (type(e).__name__, e)
        if differs(got, want):
            return key, "other bytes"
    return None, None
