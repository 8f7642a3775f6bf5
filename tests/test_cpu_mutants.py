"""CPU: the cases the GPU parity tests run tell every boundary mutant of their checker from the
checker.  No GPU.

The GPU tests of the coding loop compare the device's bytes with a Python checker's on a fixed list
of cases, the module's gpu_keys().  A kernel that restates one `<` of the reference as `<=` differs
from the reference only where two numbers are equal, so such a test sees it only if a case lands
there.  For every ordering comparison of a checker, tests/mutants.py builds the checker with that
comparison flipped at its boundary; here each such mutant must give other expected bytes than the
checker on at least one entry of gpu_keys() (every ndarray of the result compared; an exception of
the mutant counts).  A mutant nothing tells apart fails, and the message names the comparison.

EQUIVALENT lists the mutants no input can tell apart, each with the argument.  It may not hold a
comparison that decides an output at equality; those are met by boundary cases in the case modules
(BOUNDARY in tests/mbenc_cases.py and its like).  To add one: find by search a small input on
which the checker and the mutant disagree, freeze its generator parameters in the module's
boundary table, and it reaches the GPU test through gpu_keys().

Besides the mode lists' `>= 0` sentinels, EQUIVALENT holds comparisons one would take for deciding
ones: the guards `if score < 6: score += ...` (`< 7` in chroma) in front of a later test of the same
score against the same bound, `i_satd <= 0`, whose break only saves work, the chroma filter's
`tc > 0` and the deblocking `qp <= qp_thresh`.  Each entry says why; a listed mutant that any case
of up to 5x4 x 2 macroblocks does tell apart fails the test as well."""
import importlib
import time

import pytest

import mutants as mu

MODULES = ("mbenc_cases", "mbintra_cases", "mb444_cases", "mbskip_cases", "mbanalyse_cases", "deblock_cases")

# the number of mutants per module when this test was written: a refactor of a checker must not
# silently empty the set
SITES_AT_LEAST = {"mbenc_cases": 11, "mbintra_cases": 16, "mbanalyse_cases": 42, "mb444_cases": 5, "mbskip_cases": 8, "deblock_cases": 24}

# (module, function, comparison text) -> why the flip cannot change any output for any input
EQUIVALENT = {
    ("mbenc_cases", "encode_luma", "i_decimate_8x8 < 6"):
        "guards an addition of a score >= 0 to a sum that is only compared with 4 and (summed) with 6: at 6 both "
        "comparisons are decided, adding more cannot undo them",
    ("mbenc_cases", "encode_chroma", "i_decimate_score < 7", 0):
        "the first of the two (the guard of `+= decimate_score15`): at 7 the only later comparison, `< 7`, is decided "
        "and the addend is >= 0",
    ("mbintra_cases", "mb_neighbours", "my > 0", 2):
        "the third (`my > 0 and mx + 1 < mbw`): flipped, a macroblock of the top row gets MB_TOPRIGHT without MB_TOP.  The "
        "flag reaches only neighbour4(5) / neighbour8(1), and every reader masks it with MB_TOP: the top-right emulation "
        "tests (n & (TOPRIGHT | TOP)) == TOP, the 8x8 edge filter reads top-right inside its top branch, which only modes "
        "that need MB_TOP ask for, and no mode valid without a top neighbour reads the row mb_buffers copies",
    ("mbintra_cases", "encode_i16x16", "decimate_score < 6", 0):
        "the first of the two (the guard of `+= decimate_score15`): at 6 the only later comparison, `< 6`, is decided "
        "and the addend is >= 0",
    ("mbskip_cases", "pskip_one", "x > 0", 1):
        "the second (`elif x > 0` after `if x < mbw - 1`): flipped, it is taken at x = 0 of a picture one macroblock wide and "
        "reads a C neighbour; but there ra = -2, and the next statement returns (0, 0) before rc or mc is looked at",
    ("deblock_cases", "edge_chroma", "tc > 0"):
        "at tc = 0 (bS 0 at 8 bit: tc0 -1 plus 1) the flip filters the line with delta = clip3(.., -0, 0) = 0, which "
        "leaves p0 and q0 as they are (they are inside the pixel range)",
    ("deblock_cases", "deblock.mb", "qp <= qp_thresh"):
        "qp_thresh = 15 - min(a, b) - max(0, chroma_qp_index_offset) is the largest qp at which no edge of the macroblock "
        "can be filtered: at qp = qp_thresh, qp + a or qp + b is at most 15 (and the chroma qp, at most qp + max(0, offset), "
        "likewise), where i_alpha_table or i_beta_table is 0 and deblock_edge returns at once; the inner edges use no "
        "neighbour's qp",
    ("mb444_cases", "encode_inter_plane", "i_decimate_8x8 < 6"):
        "guards an addition of a score >= 0 to a sum that is only compared with 4 and (summed) with 6: at 6 both "
        "comparisons are decided, adding more cannot undo them",
    ("mbanalyse_cases", "i4x4_block", "predict_mode[5] >= 0"): "entry 5 of a row of I4x4_MODE_AVAILABLE is -1, 8 or 5, never 0",
    ("mbanalyse_cases", "i4x4_block", "predict_mode[8] >= 0"): "entry 8 of a row of I4x4_MODE_AVAILABLE is -1 or 8, never 0",
    ("mbanalyse_cases", "i8x8_block", "predict_mode[5] >= 0"): "entry 5 of a row of I8x8_MODE_AVAILABLE is -1, 8 or 5, never 0",
    ("mbanalyse_cases", "i8x8_block", "predict_mode[8] >= 0"): "entry 8 of a row of I8x8_MODE_AVAILABLE is -1 or 8, never 0",
    ("mbanalyse_cases", "analyse_chroma", "predict_mode[3] >= 0"): "entry 3 of a row of CHROMA_MODE_AVAILABLE is -1 or 3, never 0",
    ("mbanalyse_cases", "analyse_intra", "predict_mode[3] >= 0"): "entry 3 of a row of I16x16_MODE_AVAILABLE is -1 or 3, never 0",
    ("mbanalyse_cases", "analyse_chroma", "i_mode < 0", 1):
        "the second (the loop without x3): it walks the rows (6), (4, 1), (5, 2) of CHROMA_MODE_AVAILABLE, which hold no 0 "
        "before their -1",
    ("mbanalyse_cases", "i4x4_block", "i_satd <= 0"):
        "at i_satd = 0 the flip only skips the break.  The loop runs with i_best > 0, so `i_satd < i_best` makes the same "
        "assignment; of the modes that follow only the predicted one could go below 0, and a list holds it once",
}


def _equivalent(name, site, nth):
    return EQUIVALENT.get((name, site.func, site.text)) or EQUIVALENT.get((name, site.func, site.text, nth))


def _nth(sites, site):
    """which of the comparisons with this text in this function `site` is, in source order"""
    return [s.index for s in sites if (s.func, s.text) == (site.func, site.text)].index(site.index)


def _params():
    out = []
    for name in MODULES:
        for s in mu.sites(name):
            out.append(pytest.param(name, s.index, id="%s-%d-L%d" % (name.replace("_cases", ""), s.index, s.lineno)))
    return out


def _ordered_keys(name):
    """the module's gpu_keys() without repeats, the boundary cases first, then the cheapest first"""
    mod = importlib.import_module(name)
    front = set(mod.boundary_keys())
    return sorted(dict.fromkeys(mod.gpu_keys()), key=lambda e: (e[0] not in front and e[1] not in front, mod.key_size(e)))


def _call(mod, entry):
    return mod.gpu_expected(entry) if hasattr(mod, "gpu_expected") else mod.expected(*entry)


@pytest.mark.parametrize("name", MODULES)
def test_generator_finds_the_comparisons(name):
    sites = mu.sites(name)
    assert len(sites) >= SITES_AT_LEAST[name], (name, len(sites))
    mod = importlib.import_module(name)
    for fn in mu.EXCLUDED_FUNCTIONS[name]:
        assert callable(getattr(mod, fn, None)), "%s.%s is excluded from the mutants but does not exist" % (name, fn)
    for key in EQUIVALENT:
        assert any((key[0], s.func, s.text) == key[:3] for s in sites if key[0] == name) or key[0] != name, key


@pytest.mark.parametrize("name", MODULES)
def test_unflipped_module_reproduces_the_checker(name):
    """load() with no site flipped gives the checker's own bytes: what a mutant differs by is its flip"""
    orig = importlib.import_module(name)
    copy = mu.load(name, None)
    for entry in _ordered_keys(name)[:6]:
        assert not mu.differs(_call(copy, entry), _call(orig, entry)), entry


@pytest.mark.parametrize("name,index", _params())
def test_some_gpu_case_kills_the_mutant(name, index):
    sites = mu.sites(name)
    site = sites[index]
    orig = importlib.import_module(name)
    why = _equivalent(name, site, _nth(sites, site))
    t0 = time.time()
    keys = _ordered_keys(name)
    if why:                                                          # argued: every case up to 5x4 x 2 as a cross-check
        keys = [e for e in keys if orig.key_size(e) <= 40]
    killer, how = mu.first_kill(name, index, keys, _call, lambda e: _call(orig, e))
    print("%s:%d %s `%s`: %s in %.2f s" % (name, site.lineno, site.func, site.text,
                                            "killed by %r (%s)" % (killer, how) if killer else "survives", time.time() - t0))
    if why:
        assert killer is None, "%s:%d `%s` is listed as equivalent (%s) but %r tells it apart: drop the entry" % (
            name, site.lineno, site.text, why, killer)
    else:
        assert killer is not None, ("no case of %s.gpu_keys() tells `%s` (%s:%d, in %s) from its boundary flip: a kernel "
                                    "that ties this comparison the other way passes the GPU tests" % (
                                        name, site.text, name, site.lineno, site.func))
