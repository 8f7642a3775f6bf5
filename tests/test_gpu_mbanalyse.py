"""GPU: x264hip_*_mb_analyse_intra against the checker of tests/mbanalyse_cases.py, bit-exact in
every array it writes.

As tests/test_gpu_mbintra.py: every buffer of a call is carved out of one byte arena
(tests/footprint.py), planes between guard rows, lists between 4096 guard bytes, each
per-macroblock output array optionally one element into its buffer, and the whole arena is compared
with the bytes expected after the calls.  A P / B picture runs mb_encode_inter, then
mb_analyse_intra on the same recon planes and output arrays; an I picture runs mb_analyse_intra
alone.  Before the analysis the recon pixels of every try macroblock of an I picture and of the
try macroblocks that come out intra on a P / B picture hold the arena's fill: their prior content
must reach nothing.  Never reads the reference."""
import types

import numpy as np
import pytest

import footprint as fp
import mbanalyse_cases as ma
import mbenc_cases as mc
import mbintra_cases as mi
from test_gpu_mbintra import INTER_OUTS, OUT_WIDTH, T, _inner_of, _np_pix, _tuple, cdt, dev_tables, pdt, pix_t, report, udt

pytestmark = pytest.mark.gpu

WIDTH = dict(OUT_WIDTH, mb_flags_out=1, cost=4)


def lam_tab(bd):
    return np.array(ma.LAMBDA_TAB[:52 + 6 * (bd - 8)], np.uint16)


def grid(case, sel, rows):
    g = np.asarray(sel, bool).reshape(case.nframes, case.mbh, case.mbw)
    return np.repeat(np.repeat(g, rows, 1), 16, 2)


def setup(ar, key, dec, shift, noise=False, scribble=True):
    case = ma.make_case(*key)
    want = ma.expected(key, dec)
    bd = case.bd
    tb = mc.tables(bd, case.cqm)
    nf, W, H, CH = case.nframes, 16 * case.mbw, 16 * case.mbh, case.chroma_rows * case.mbh
    c = types.SimpleNamespace(case=case, bd=bd, shift=shift, planes={}, want=want, dec=dec, fill=ar.fill)
    # the macroblocks whose recon the analysis writes: their prior content is the arena's fill; on
    # a P / B picture it is put there after the inter call (scribble below)
    c.scribble = want.intra & (case.try_intra != 0) & scribble

    def plane(name, h, data, extra):
        b = ar.plane(name, nf, W, h, pdt(bd), extra=extra)
        _inner_of(b, b.np(ar.host))[...] = data
        c.planes[name] = b
    plane("fenc", H, case.fenc_y, 0)
    plane("recon", H, case.pred_y, 32)
    if case.cf:
        plane("fenc_c", CH, case.fenc_c, 32)
        plane("recon_c", CH, case.pred_c, 16)
    c.qp = ar.list("qp", case.nmb, np.int8, case.qp)
    c.flags = ar.list("flags", case.nmb, np.uint8, case.flags)
    c.tr = ar.list("try_intra", case.nmb, np.uint8, case.try_intra)
    c.satd = ar.list("satd_inter", case.nmb, np.int32, case.satd_inter)
    c.fast = ar.list("fast_intra", case.nmb, np.uint8, case.fast_intra)
    c.pmode = ar.list("pred_mode", case.nmb * 16, np.int8, case.pred_mode)
    c.cmode = ar.list("chroma_pred_mode", case.nmb, np.int8, case.chroma_pred_mode)
    ut = udt(bd)
    c.tabs = [ar.list(n, a.shape, a.dtype, a) for n, a in (("q4m", tb.q4m.astype(ut)), ("q4b", tb.q4b.astype(ut)),
                                                          ("q8m", tb.q8m.astype(ut)), ("q8b", tb.q8b.astype(ut)),
                                                          ("dq4", tb.dq4), ("dq8", tb.dq8))]
    dts = {"level": cdt(bd), "chroma_dc": cdt(bd), "nnz": np.uint8, "cbp": np.int32, "nz": np.int32,
           "flags_out": np.uint8, "luma_dc": cdt(bd), "mb_flags_out": np.uint8, "cost": np.int32}
    c.outs = {n: ar.list(n, case.nmb * w + 2 * shift, dts[n]) for n, w in WIDTH.items()}
    if noise:
        # everything the entry may not read: the modes of the try macroblocks, satd_inter and
        # fast_intra of the others (satd_inter of all of them on an I picture)
        rng = np.random.default_rng(7)
        tried = case.try_intra != 0
        c.pmode.data(ar.host).reshape(case.nmb, 16)[tried] = rng.integers(-128, 128, (int(tried.sum()), 16))
        c.cmode.data(ar.host)[tried] = rng.integers(-128, 128, int(tried.sum()))
        unread = ~tried if case.slice_type != ma.SLICE_I else np.ones(case.nmb, bool)
        c.satd.data(ar.host)[unread] = rng.integers(-2 ** 31, 2 ** 31 - 1, int(unread.sum()))
        c.fast.data(ar.host)[~tried] = rng.integers(0, 256, int((~tried).sum()))
    return c


def call(hip, c, dev, tight=False):
    """mb_encode_inter on a P / B picture, the scribble, then mb_analyse_intra, in place"""
    import torch
    case, p, s = c.case, c.planes, c.shift
    tabs = [T(b, dev) for b in c.tabs]
    outs = {n: T(b, dev)[s:s + case.nmb * WIDTH[n]] for n, b in c.outs.items()}
    cf = case.cf
    fenc, recon = _tuple(p["fenc"], dev), _tuple(p["recon"], dev)
    fenc_c = _tuple(p["fenc_c"], dev) if cf else None
    recon_c = _tuple(p["recon_c"], dev) if cf else None
    common = dict(quant8=(tabs[2], tabs[3]), dequant8_mf=tabs[5], chroma_format=cf, fenc_chroma=fenc_c,
                  b_dct_decimate=c.dec, qp_table=case.qp_table)
    if case.slice_type != ma.SLICE_I:
        hip.mb_encode_inter(fenc, recon, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev),
                            (tabs[0], tabs[1]), tabs[4], pred_chroma=recon_c, outs={n: outs[n] for n in INTER_OUTS}, **common)
    for name, rows in (("recon", 16), ("recon_c", case.chroma_rows)):
        if name in p and c.scribble.any():
            pic = _inner_of(p[name], p[name].t(dev))
            v = np.array([fp.fill_value(pdt(c.bd), c.fill)], pdt(c.bd))
            pic[torch.from_numpy(grid(case, c.scribble, rows)).cuda()] = int(v.view(np.int16 if c.bd == 10 else np.uint8)[0])
    hip.mb_analyse_intra(fenc, recon, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev), T(c.tr, dev),
                         T(c.pmode, dev), lam_tab(c.bd), (tabs[0], tabs[1]), tabs[4], recon_chroma=recon_c,
                         chroma_pred_mode=T(c.cmode, dev) if cf else None, slice_type=case.slice_type,
                         i_subpel_refine=case.subme, b_i4x4=case.b_i4x4, b_i8x8=case.b_i8x8, b_chroma_me=case.b_chroma_me,
                         satd_inter=T(c.satd, dev), fast_intra=T(c.fast, dev), outs=outs, **common)


def expected_bytes(ar, c):
    """the arena after the calls"""
    case, want = c.case, c.want
    host = ar.bytes().copy()
    for name, exp in (("recon", want.recon_y), ("recon_c", want.recon_c)):
        if name in c.planes:
            b = c.planes[name]
            _inner_of(b, b.np(host))[...] = exp
    tried = case.try_intra != 0
    every = np.ones(case.nmb, bool)
    inter_written = every if case.slice_type != ma.SLICE_I else want.intra
    rows_of = {"luma_dc": want.intra, "mb_flags_out": tried, "cost": tried}
    for n, b in c.outs.items():
        w = WIDTH[n]
        data = b.data(host)[c.shift:c.shift + case.nmb * w].reshape(case.nmb, w)
        exp = getattr(want, n).reshape(case.nmb, w)
        rows = rows_of.get(n, inter_written)
        data[rows] = exp[rows]
    decided = want.intra & tried
    c.pmode.data(host).reshape(case.nmb, 16)[decided] = want.pred_mode[decided]
    if case.cf:
        c.cmode.data(host)[decided] = want.chroma_pred_mode[decided]
    return host


def run(hip, key, dec=1, shift=0, fill=fp.FILLS[0], noise=False):
    import torch
    ar = fp.Arena(fill)
    c = setup(ar, key, dec, shift, noise)
    dev = ar.device()
    call(hip, c, dev)
    torch.cuda.synchronize()
    got, want = dev.cpu().numpy(), expected_bytes(ar, c)
    assert np.array_equal(got, want), (key, dec, shift, report(ar, got, want))
    return c


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2])
@pytest.mark.parametrize("slice_type", [0, 1, 2])
def test_mb_analyse_intra_bit_exact(hip, bd, cf, slice_type):
    """every shape -- 1x1, 3x1, 1x3, 2x2 (the picture edges: only the _128 / _LEFT / _TOP lists, one
    macroblock with a top-right neighbour), 5x4 x 2 and 7x3 x 3 frames (the x + 2y skew, a frame
    boundary inside a launch, a right edge without top-right) -- with the output arrays aligned
    and one element off, decimation on and off, both arena fills"""
    entries = ma.gpu_keys("shapes", bd=bd, cf=cf, slice_type=slice_type)
    keys = sorted(set(k for k, _ in entries), key=[k for k, _ in entries].index)
    assert len(keys) == len(ma.SHAPES) and all((k, d) in entries for k in keys for d in (0, 1))
    for i, key in enumerate(keys):
        run(hip, key, dec=i & 1, shift=i & 1, fill=fp.FILLS[i & 1])
        run(hip, key, dec=1 - (i & 1), shift=1 - (i & 1), fill=fp.FILLS[1 - (i & 1)])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kw", ma.OPTIONS)
def test_mb_analyse_intra_options(hip, bd, kw):
    """I_8x8 off, I_4x4 off, the JVT matrices, the chroma-ME leg, i_subpel_refine 2, on a P and an I
    picture at 4:2:0 and a B picture at 4:2:2"""
    (p, dp), (i, di), (b, db) = ma.gpu_keys("options", bd=bd, **kw)
    assert (p[1], p[5], i[1], i[5], b[1], b[5]) == (1, 1, 1, 0, 2, 2)
    run(hip, p, dec=dp, shift=1)
    run(hip, i, dec=di)
    run(hip, b, dec=db)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("content", ["flat", "checker"])
def test_flat_and_checkerboard(hip, bd, content):
    """a flat picture (every cost a tie) and a full-scale checkerboard (the top of the cost range)
    at qp 0 and QP_MAX_SPEC"""
    (a, da), (b, db) = ma.gpu_keys("content", bd=bd, content=content)
    run(hip, a, dec=da)
    run(hip, b, dec=db)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("slice_type", [0, 1])
def test_noise_over_what_may_not_be_read(hip, bd, slice_type):
    """pred_mode / chroma_pred_mode of the try macroblocks, satd_inter where it is not read and
    fast_intra of the other macroblocks hold noise: the bytes are those of the clean run, the
    noise of the macroblocks that stay inter still in place"""
    (key, dec), = ma.gpu_keys("noise", bd=bd, slice_type=slice_type)
    run(hip, key, dec=dec, noise=True, shift=1, fill=fp.FILLS[1])


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("what", [b[0] for b in ma.BOUNDARY], ids=lambda w: w.split(":")[0].replace(" ", "_")[:48])
def test_boundary_cases_bit_exact(hip, bd, what):
    """the pictures of mbanalyse_cases.BOUNDARY: a cost exactly on the fast-intra gate, the Plane
    gate, the I_8x8 bound, an early termination or another type's cost, chroma modes that tie: a
    kernel that ties one of these the other way differs here, in cost[] at the least"""
    key = ma.boundary_key(bd, [b[0] for b in ma.BOUNDARY].index(what))
    (key, dec), = [kd for kd in ma.gpu_keys("boundary", bd=bd) if kd[0] == key]
    run(hip, key, dec=dec, shift=0)
    run(hip, key, dec=dec, shift=1, fill=fp.FILLS[1])


@pytest.mark.parametrize("bd", [8, 10])
def test_side_stream_behind_a_delay(hip, bd):
    """on a non-default stream behind the delay kernel the calls (a launch per diagonal) wait for
    their stream and leave the bytes of the null-stream run, which are the checker's"""
    import torch
    import stream_cases as sc
    key = ma.make_key(bd, 1, 5, 4, 2, 1)
    row = types.SimpleNamespace(name="mb_analyse_intra", entries=("mb_encode_inter", "mb_analyse_intra"), cases=[("case", {})],
                                setup=lambda ar, bd: setup(ar, key, 1, 0, scribble=False), call=call, variants=[],
                                variant_case=lambda bd, case: True)
    p = sc.Prepared(row, bd)
    want = sc.null_run(hip, p)
    got, ended = sc.side_run(hip, p, torch.cuda.Stream())
    assert not ended, "the delay had ended when the call returned: the run shows nothing"
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    ar = fp.Arena(fp.FILLS[0])
    assert np.array_equal(want, expected_bytes(ar, setup(ar, key, 1, 0, scribble=False)))


# ------------------------------------------------------------------ plain tensors
def run_plain(hip, case, dec=1, analyse=True, flags=None, pred_mode=None, chroma_pred_mode=None):
    """the wrappers on dense tensors in place; analyse False: mb_encode_intra with the flags and
    modes given.  Returns the outputs as numpy plus recon_y / recon_c."""
    import torch
    q4, q8, dq4, dq8 = dev_tables(hip, case.bd, case.cqm)
    W = 16 * case.mbw
    dense = lambda a: (pix_t(a), 0, W, a.shape[1] * W)
    cf = case.cf
    recon, recon_c = dense(case.pred_y), dense(case.pred_c) if cf else None
    fenc, fenc_c = dense(case.fenc_y), dense(case.fenc_c) if cf else None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    qp, fl = t(case.qp), t(case.flags if flags is None else flags)
    pm = t(case.pred_mode if pred_mode is None else pred_mode)
    cm = t(case.chroma_pred_mode if chroma_pred_mode is None else chroma_pred_mode) if cf else None
    common = dict(quant8=q8, dequant8_mf=dq8, chroma_format=cf, fenc_chroma=fenc_c, b_dct_decimate=dec, qp_table=case.qp_table)
    out = None
    if case.slice_type != ma.SLICE_I:
        out = hip.mb_encode_inter(fenc, recon, case.mbw, case.mbh, case.nframes, qp, t(case.flags), q4, dq4,
                                  pred_chroma=recon_c, **common)
    if analyse:
        out = hip.mb_analyse_intra(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl, t(case.try_intra), pm, lam_tab(case.bd),
                                   q4, dq4, recon_chroma=recon_c, chroma_pred_mode=cm, slice_type=case.slice_type,
                                   i_subpel_refine=case.subme, b_i4x4=case.b_i4x4, b_i8x8=case.b_i8x8,
                                   b_chroma_me=case.b_chroma_me, satd_inter=t(case.satd_inter), fast_intra=t(case.fast_intra),
                                   outs=out, **common)
        names = hip.MBANALYSE_OUTPUTS
    else:
        out = hip.mb_encode_intra(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl, pm, q4, dq4, recon_chroma=recon_c,
                                  chroma_pred_mode=cm, outs=out, **common)
        names = hip.MBINTRA_OUTPUTS
    torch.cuda.synchronize()
    res = types.SimpleNamespace(**{n: out[n].cpu().numpy() for n in names})
    res.recon_y = _np_pix(recon[0], case.bd).reshape(case.pred_y.shape)
    res.recon_c = _np_pix(recon_c[0], case.bd).reshape(case.pred_c.shape) if cf else None
    res.pred_mode, res.chroma_pred_mode = pm.cpu().numpy(), cm.cpu().numpy() if cf else None
    return res


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("slice_type", [0, 1])
def test_decided_modes_fed_to_mb_encode_intra(hip, bd, slice_type):
    """the device's decided flags and modes fed to mb_encode_intra on fresh planes give identical
    bytes in every array and pixel (what x264's i_skip_intra reuse relies on)"""
    case = ma.make_case(*ma.make_key(bd, 1, 5, 4, 2, slice_type))
    a = run_plain(hip, case)
    b = run_plain(hip, case, analyse=False, flags=a.mb_flags_out, pred_mode=a.pred_mode, chroma_pred_mode=a.chroma_pred_mode)
    assert (a.mb_flags_out != case.flags).any()
    for n in ("level", "chroma_dc", "nnz", "cbp", "nz", "flags_out", "luma_dc", "recon_y", "recon_c"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 2])
def test_no_try_macroblock_equals_mb_encode_intra(hip, bd, cf):
    """with try_intra all zero the entry is mb_encode_intra on mbintra_cases' inputs"""
    base = mi.make_case(bd, cf, 5, 4, 2)
    case = types.SimpleNamespace(**vars(base), slice_type=1, subme=5, b_i4x4=1, b_i8x8=1, b_chroma_me=0,
                                 try_intra=np.zeros(base.nmb, np.uint8), satd_inter=np.zeros(base.nmb, np.int32),
                                 fast_intra=np.zeros(base.nmb, np.uint8))
    a = run_plain(hip, case)
    want = mi.expected(base.key, 1)
    for n in ("level", "chroma_dc", "nnz", "cbp", "nz", "flags_out", "luma_dc", "recon_y"):
        assert np.array_equal(getattr(a, n).reshape(getattr(want, n).shape), getattr(want, n)), n
    assert np.array_equal(a.mb_flags_out, case.flags) and not a.cost.any()
    assert np.array_equal(a.pred_mode, case.pred_mode)


def test_zero_macroblocks_and_refusals(hip):
    import torch
    case = ma.make_case(*ma.make_key(8, 1, 3, 1, 1, 1))
    q4, q8, dq4, dq8 = dev_tables(hip, 8, "flat")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    y, c = pix_t(case.pred_y), pix_t(case.pred_c)
    before, before_c = y.clone(), c.clone()
    cost = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    fenc, fenc_c = (pix_t(case.fenc_y), 0, 48, 48 * 16), (pix_t(case.fenc_c), 0, 48, 48 * 8)
    ok = dict(fenc=fenc, recon=(y, 0, 48, 48 * 16), mb_width=3, mb_height=1, nframes=1, qp=t(case.qp), mb_flags=t(case.flags),
              try_intra=t(case.try_intra), pred_mode=t(case.pred_mode), lambda_tab=lam_tab(8), quant4=q4, dequant4_mf=dq4,
              quant8=q8, dequant8_mf=dq8, chroma_format=1, fenc_chroma=fenc_c, recon_chroma=(c, 0, 48, 48 * 8),
              chroma_pred_mode=t(case.chroma_pred_mode), slice_type=1, satd_inter=t(case.satd_inter),
              outs={"cost": cost[:12]})
    for kw in (dict(mb_width=0), dict(nframes=0)):
        hip.mb_analyse_intra(**{**ok, **kw})
    torch.cuda.synchronize()
    assert torch.equal(y, before) and torch.equal(c, before_c) and bool((cost == 0x5A5A5A5A).all())
    # the wrapper's refusals
    for kw in (dict(slice_type=3), dict(i_subpel_refine=1), dict(i_subpel_refine=6), dict(satd_inter=None),
               dict(quant8=None, dequant8_mf=None), dict(lambda_tab=lam_tab(8)[:51]), dict(chroma_pred_mode=None),
               dict(try_intra=t(case.try_intra)[:2]), dict(outs={"cost": cost[:11]})):
        with pytest.raises(ValueError):
            hip.mb_analyse_intra(**{**ok, **kw})
    # the entry's: planes off their 4-pixel boundary (tests/test_cpu_mbanalyse.py has every X264HIP_EINVAL)
    for kw in (dict(recon=(y, 2, 48, 48 * 16)), dict(recon=(y, 0, 50, 48 * 16)), dict(recon_chroma=(c, 1, 48, 48 * 8))):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            hip.mb_analyse_intra(**{**ok, **kw})
    torch.cuda.synchronize()
    assert torch.equal(y, before) and torch.equal(c, before_c) and bool((cost == 0x5A5A5A5A).all())


# ------------------------------------------------------------------ the I chain
@pytest.mark.parametrize("bd", [8, 10])
def test_i_chain_analyse_deblock(hip, bd):
    """mb_analyse_intra -> deblock_strength -> deblock_frames on the device, nothing read back in
    between, against the checkers chained the same way"""
    import torch
    import deblock_cases as dc
    cf, mbw, mbh, nf = 1, 5, 4, 2
    W, H = 16 * mbw, 16 * mbh
    key = ma.make_key(bd, cf, mbw, mbh, nf, 0)
    case, enc = ma.make_case(*key), ma.expected(key, 1)
    mv0 = np.zeros((nf, 4 * mbh, 4 * mbw, 2), np.int16)
    ref0 = np.full((nf, 2 * mbh, 2 * mbw), -1, np.int8)
    bs = dc.deblock_strength_py(enc.nz, enc.flags_out, [mv0], [ref0], mbw, mbh, nf)
    dcase = types.SimpleNamespace(bd=bd, cf=cf, mbw=mbw, mbh=mbh, nf=nf, alpha_c0_offset=0, beta_offset=0,
                                  chroma_qp_index_offset=0, luma=enc.recon_y, chroma=[enc.recon_c], qp=case.qp,
                                  mb_flags=enc.flags_out, bs=bs.reshape(-1, 2, 4, 4), slice_table=None,
                                  chroma_qp_table=case.qp_table)
    want_y, want_c = dc.deblock(dcase)
    q4, q8, dq4, dq8 = dev_tables(hip, bd, "flat")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    y, c = pix_t(case.pred_y), pix_t(case.pred_c)
    qp_t = t(case.qp)
    out = hip.mb_analyse_intra((pix_t(case.fenc_y), 0, W, H * W), (y, 0, W, H * W), mbw, mbh, nf, qp_t, t(case.flags),
                               t(case.try_intra), t(case.pred_mode), lam_tab(bd), q4, dq4, quant8=q8, dequant8_mf=dq8,
                               chroma_format=cf, fenc_chroma=(pix_t(case.fenc_c), 0, W, H // 2 * W),
                               recon_chroma=(c, 0, W, H // 2 * W), chroma_pred_mode=t(case.chroma_pred_mode), slice_type=0,
                               qp_table=case.qp_table)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], t(mv0), t(ref0), mbw, mbh, nf)
    hip.deblock_frames(y, 0, W, mbw, mbh, qp_t, out["flags_out"], bs_t, chroma=(cf, [c], 0, W), qp_table=case.qp_table)
    torch.cuda.synchronize()
    assert np.array_equal(bs_t.cpu().numpy().reshape(bs.shape), bs)
    assert np.array_equal(_np_pix(y, bd).reshape(want_y.shape), want_y.astype(pdt(bd)))
    assert np.array_equal(_np_pix(c, bd).reshape(want_c[0].shape), want_c[0].astype(pdt(bd)))
    assert (want_y != enc.recon_y).any()


@pytest.mark.parametrize("bd", [8, 10])
def test_p_chain_mc_encode_analyse_convert_deblock(hip, bd):
    """mb_mc -> mb_encode_inter -> mb_analyse_intra -> mb_skip_convert -> deblock_strength ->
    deblock_frames on the device, nothing read back in between, against the checkers chained the
    same way"""
    import torch
    import deblock_cases as dc
    import mbskip_cases as ms
    import mc_cases as mcc
    cf, mbw, mbh, nf = 1, 5, 4, 2
    W, H = 16 * mbw, 16 * mbh
    base = ma.make_case(*ma.make_key(bd, cf, mbw, mbh, nf, 1))
    ref = mcc.make_ref(bd, W, H, cf, nf, 7)
    pos = mcc.block_positions(W, H, nf, 0)
    mv = mcc.phase_mvs(pos, W, H, 11)
    mv = (mv // 16) % 5 - 2 + (mv & 3)                            # small vectors: the residual stays codable
    par = mcc.make_par(pos, mv, mv, W, H)
    # the checkers
    pred, pred_c = mcc.pred_planes(ref)
    mcc.mb_mc(bd, cf, 0, ref, None, pos, par, None, (None, None, None), pred, ref.oy, ref.ox, pred_c, ref.coy, ref.cox)
    case = types.SimpleNamespace(**vars(base))
    case.pred_y = pred[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W].copy()
    case.pred_c = pred_c[0][:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W].copy()
    enc = ma.encode(case, 1)
    decided = enc.intra & (case.try_intra != 0)
    assert decided.any() and (~enc.intra & (case.try_intra != 0)).any()
    mv0 = np.repeat(np.repeat(mv.reshape(nf, mbh, mbw, 2), 4, 1), 4, 2).astype(np.int16)
    ref0 = np.zeros((nf, 2 * mbh, 2 * mbw), np.int8)
    want_ps = ms.pskip_mv(mv0, ref0, mbw, mbh)
    want_flags = ms.skip_convert(enc.mb_flags_out, enc.cbp, mv0, ref0, want_ps, 0, None, mbw, mbh)
    bs = dc.deblock_strength_py(enc.nz, enc.flags_out, [mv0], [ref0], mbw, mbh, nf)
    dcase = types.SimpleNamespace(bd=bd, cf=cf, mbw=mbw, mbh=mbh, nf=nf, alpha_c0_offset=0, beta_offset=0,
                                  chroma_qp_index_offset=0, luma=enc.recon_y, chroma=[enc.recon_c], qp=case.qp,
                                  mb_flags=enc.flags_out, bs=bs.reshape(-1, 2, 4, 4), slice_table=None,
                                  chroma_qp_table=case.qp_table)
    want_y, want_c = dc.deblock(dcase)
    # the device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    luma, nv = [pix_t(a) for a in ref.luma], [pix_t(a) for a in ref.chroma]
    p, pc = hip.mb_mc(luma, None, ref.origin, ref.stride, 0, t(pos), t(par), None, chroma=(cf, nv, None, ref.corigin, ref.cs))
    ptup, ctup = (p, ref.origin, ref.stride, p[0].numel()), (pc[0], ref.corigin, ref.cs, pc[0][0].numel())
    q4, q8, dq4, dq8 = dev_tables(hip, bd, "flat")
    qp_t, fl_t, mv0_t, ref0_t = t(case.qp), t(case.flags), t(mv0), t(ref0)
    fenc, fenc_c = (pix_t(case.fenc_y), 0, W, H * W), (pix_t(case.fenc_c), 0, W, H // 2 * W)
    common = dict(quant8=q8, dequant8_mf=dq8, chroma_format=cf, fenc_chroma=fenc_c, b_dct_decimate=1, qp_table=case.qp_table)
    out = hip.mb_encode_inter(fenc, ptup, mbw, mbh, nf, qp_t, fl_t, q4, dq4, pred_chroma=ctup, **common)
    out = hip.mb_analyse_intra(fenc, ptup, mbw, mbh, nf, qp_t, fl_t, t(case.try_intra), t(case.pred_mode), lam_tab(bd), q4, dq4,
                               recon_chroma=ctup, chroma_pred_mode=t(case.chroma_pred_mode), slice_type=1,
                               satd_inter=t(case.satd_inter), fast_intra=t(case.fast_intra), outs=out, **common)
    ps_t = hip.mb_predict_mv_pskip(mv0_t, ref0_t, mbw, mbh, nf)
    final_t = hip.mb_skip_convert(out["mb_flags_out"], out["cbp"], mbw, mbh, nf, mv0=mv0_t, ref0=ref0_t, pskip_mv=ps_t)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], mv0_t, ref0_t, mbw, mbh, nf)
    hip.deblock_frames(p, ref.origin, ref.stride, mbw, mbh, qp_t, out["flags_out"], bs_t,
                       chroma=(cf, [pc[0]], ref.corigin, ref.cs), qp_table=case.qp_table)
    torch.cuda.synchronize()
    assert np.array_equal(out["mb_flags_out"].cpu().numpy(), enc.mb_flags_out)
    assert np.array_equal(out["cost"].cpu().numpy()[case.try_intra != 0], enc.cost[case.try_intra != 0])
    assert np.array_equal(final_t.cpu().numpy(), want_flags)
    assert np.array_equal(bs_t.cpu().numpy().reshape(bs.shape), bs)
    got_y = _np_pix(p, bd)[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W]
    got_c = _np_pix(pc[0], bd)[:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W]
    assert np.array_equal(got_y, want_y.astype(got_y.dtype)) and np.array_equal(got_c, want_c[0].astype(got_c.dtype))
