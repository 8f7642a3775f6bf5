"""GPU: x264hip_*_mb_encode_intra against the checker of tests/mbintra_cases.py, bit-exact in every
output array.

As tests/test_gpu_mbenc.py: every buffer of a call is carved out of one byte arena
(tests/footprint.py), planes between guard rows with a different stride each, lists between guard
bytes, each per-macroblock output array optionally one element into its buffer, and the whole
arena is compared with the bytes expected after the call.  A mixed picture runs
mb_encode_inter, then mb_encode_intra on the same recon planes and output arrays; an all-intra
picture runs mb_encode_intra alone.  Before the calls the recon pixels of the intra macroblocks
hold the arena's fill: their prior content must reach nothing.  No test passes an invalid mode."""
import types

import numpy as np
import pytest

import footprint as fp
import mbenc_cases as mc
import mbintra_cases as mi

pytestmark = pytest.mark.gpu

FILL = fp.FILLS[0]
OUT_WIDTH = {"level": 48 * 16, "chroma_dc": 16, "nnz": 48, "cbp": 1, "nz": 1, "flags_out": 1, "luma_dc": 16}
INTER_OUTS = ("level", "chroma_dc", "nnz", "cbp", "nz", "flags_out")


def pdt(bd):
    return np.uint8 if bd == 8 else np.uint16


def cdt(bd):
    return np.int16 if bd == 8 else np.int32


def udt(bd):
    return np.uint16 if bd == 8 else np.uint32


def T(buf, dev):
    return buf.dt(dev) if isinstance(buf, fp.ListBuf) else buf.t(dev)


def _inner_of(buf, full):
    """the picture (no padding) inside a plane buffer's whole region: [nframes, height, width]"""
    r, c = buf.guard_rows + buf.pad_y, buf.pad_x
    return full[:, r:r + buf.height, c:c + buf.width]


def intra_grid(case, rows):
    """[nframes, rows*mbh, 16*mbw] bool: the pixels of the intra macroblocks"""
    g = ((case.flags & mi.INTRA) != 0).reshape(case.nframes, case.mbh, case.mbw)
    return np.repeat(np.repeat(g, rows, 1), 16, 2)


def setup(ar, bd, key, shift):
    """carve the buffers of one run; shift: the output arrays start `shift` elements into their
    buffers.  recon starts as the prediction with the arena's fill over the intra macroblocks."""
    case = mi.make_case(*key)
    tb = mc.tables(bd, case.cqm)
    nf, W, H, CH = case.nframes, 16 * case.mbw, 16 * case.mbh, case.chroma_rows * case.mbh
    c = types.SimpleNamespace(case=case, bd=bd, shift=shift, planes={})

    def plane(name, h, data, extra, rows=0):
        b = ar.plane(name, nf, W, h, pdt(bd), extra=extra)
        pic = _inner_of(b, b.np(ar.host))
        pic[...] = data
        if rows:
            pic[intra_grid(case, rows)] = fp.fill_value(pdt(bd), ar.fill)
        c.planes[name] = b
    plane("fenc", H, case.fenc_y, 0)
    plane("recon", H, case.pred_y, 32, 16)
    if case.cf:
        plane("fenc_c", CH, case.fenc_c, 32)
        plane("recon_c", CH, case.pred_c, 16, case.chroma_rows)
    c.qp = ar.list("qp", case.nmb, np.int8, case.qp)
    c.flags = ar.list("flags", case.nmb, np.uint8, case.flags)
    c.pmode = ar.list("pred_mode", case.nmb * 16, np.int8, case.pred_mode)
    c.cmode = ar.list("chroma_pred_mode", case.nmb, np.int8, case.chroma_pred_mode)
    ut = udt(bd)
    c.tabs = [ar.list(n, a.shape, a.dtype, a) for n, a in (("q4m", tb.q4m.astype(ut)), ("q4b", tb.q4b.astype(ut)),
                                                          ("q8m", tb.q8m.astype(ut)), ("q8b", tb.q8b.astype(ut)),
                                                          ("dq4", tb.dq4), ("dq8", tb.dq8))]
    dts = {"level": cdt(bd), "chroma_dc": cdt(bd), "nnz": np.uint8, "cbp": np.int32, "nz": np.int32,
           "flags_out": np.uint8, "luma_dc": cdt(bd)}
    c.outs = {n: ar.list(n, case.nmb * w + 2 * shift, dts[n]) for n, w in OUT_WIDTH.items()}
    return c


def _tuple(buf, dev):
    return (T(buf, dev), buf.origin, buf.stride, buf.frame_stride)


def call(hip, c, dev, tight=False, dec=1):
    """mb_encode_inter (unless the picture is all intra), then mb_encode_intra, in place"""
    case, p, s = c.case, c.planes, c.shift
    tabs = [T(b, dev) for b in c.tabs]
    outs = {n: T(b, dev)[s:s + case.nmb * OUT_WIDTH[n]] for n, b in c.outs.items()}
    cf = case.cf
    fenc, recon = _tuple(p["fenc"], dev), _tuple(p["recon"], dev)
    fenc_c = _tuple(p["fenc_c"], dev) if cf else None
    recon_c = _tuple(p["recon_c"], dev) if cf else None
    common = dict(quant8=(tabs[2], tabs[3]), dequant8_mf=tabs[5], chroma_format=cf, fenc_chroma=fenc_c, b_dct_decimate=dec,
                  qp_table=case.qp_table)
    if not case.all_intra:
        hip.mb_encode_inter(fenc, recon, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev),
                            (tabs[0], tabs[1]), tabs[4], pred_chroma=recon_c, outs={n: outs[n] for n in INTER_OUTS}, **common)
    hip.mb_encode_intra(fenc, recon, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev), T(c.pmode, dev),
                        (tabs[0], tabs[1]), tabs[4], recon_chroma=recon_c, chroma_pred_mode=T(c.cmode, dev) if cf else None,
                        outs=outs, **common)


def masks(c):
    """{buffer name: the elements the two calls write}: every pixel of the picture and every
    element of the arrays (each macroblock belongs to one call), luma_dc of the intra macroblocks"""
    case = c.case
    out = {}
    for name in ("recon", "recon_c"):
        if name in c.planes:
            b = c.planes[name]
            out[name] = b.rect(0, b.width, 0, b.height)
    intra = (case.flags & mi.INTRA) != 0
    for n, b in c.outs.items():
        pm = np.zeros(b.pshape, bool)
        w = OUT_WIDTH[n]
        pm[c.shift:c.shift + case.nmb * w] = np.repeat(intra if n == "luma_dc" else np.ones(case.nmb, bool), w)
        out[n] = b.mask(pm)
    return out


def expected_bytes(ar, c, dec):
    """the arena after the calls"""
    case = c.case
    want = mi.expected(case.key, dec)
    host = ar.bytes().copy()
    for name, exp in (("recon", want.recon_y), ("recon_c", want.recon_c)):
        if name in c.planes:
            b = c.planes[name]
            _inner_of(b, b.np(host))[...] = exp
    intra = (case.flags & mi.INTRA) != 0
    for n, b in c.outs.items():
        w = OUT_WIDTH[n]
        data = b.data(host)[c.shift:c.shift + case.nmb * w].reshape(case.nmb, w)
        exp = getattr(want, n).reshape(case.nmb, w)
        rows = intra if n == "luma_dc" else np.ones(case.nmb, bool)
        data[rows] = exp[rows]
    return host


def report(ar, got, want):
    """which buffers differ, and where"""
    lines = []
    for b in ar.bufs:
        g, w = b.np(got), b.np(want)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            lines.append("%s: %d element(s), first %s got %s want %s" % (
                b.name, len(at), [b.coords(i) for i in at[:4]], g[g != w][:4].tolist(), w[g != w][:4].tolist()))
    return "; ".join(lines) or "bytes between the buffers"


def run(hip, key, dec, shift):
    import torch
    ar = fp.Arena(FILL)
    c = setup(ar, key[0], key, shift)
    dev = ar.device()
    call(hip, c, dev, dec=dec)
    torch.cuda.synchronize()
    got, want = dev.cpu().numpy(), expected_bytes(ar, c, dec)
    assert np.array_equal(got, want), (key, dec, shift, report(ar, got, want))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2])
@pytest.mark.parametrize("dec", [0, 1])
def test_mb_encode_intra_bit_exact(hip, bd, cf, dec):
    """every shape of the case list -- 1x1 (no neighbour: only the _128 modes, a quarter-filled
    wave), 3x1 and 1x3 (left only, top only), 2x2 (one macroblock with a top-right neighbour), all
    intra; 5x4 x 2 frames (mixed inter and intra after mb_encode_inter, a frame stride, the x + 2y
    skew, a right edge without top-right), 24x14 x 2 frames (many workgroups, 50 launches) -- with
    the output arrays aligned and one element off"""
    keys = mi.gpu_keys("shapes", bd=bd, cf=cf, dec=dec)
    assert len(keys) == len(mi.SHAPES)
    for key, dec in keys:
        run(hip, key, dec, shift=0)
        run(hip, key, dec, shift=1)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2])
def test_mb_encode_intra_custom_matrices(hip, bd, cf):
    """the JVT matrices: the intra luma, intra chroma and 8x8 lists differ from each other and from
    the inter ones"""
    (key, dec), = mi.gpu_keys("jvt", bd=bd, cf=cf)
    run(hip, key, dec, shift=1)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2])
def test_all_intra_picture(hip, bd, cf):
    """an I picture, 5x4, with no inter call before it; its two last macroblock rows are quiet"""
    (k1, d1), (k0, d0) = mi.gpu_keys("all_intra", bd=bd, cf=cf)
    assert (d1, d0) == (1, 0)
    run(hip, k1, d1, shift=0)
    run(hip, k0, d0, shift=1)


@pytest.mark.parametrize("key,dec", mi.gpu_keys("boundary"), ids=lambda v: "%dbit-cf%d" % v[:2] if isinstance(v, tuple) else None)
def test_boundary_cases_bit_exact(hip, key, dec):
    """the macroblocks of mbintra_cases.BOUNDARY: the AC decimate score of an I_16x16 macroblock
    below, exactly at and above 6; a kernel that decimates at 6 differs here"""
    try:
        run(hip, key, dec, shift=0)
        run(hip, key, dec, shift=1)
    except AssertionError as e:
        raise AssertionError("%s\nmacroblocks: %s" % (e, [(i, n) for i, (n, _) in enumerate(mi.BOUNDARY)]))


# ------------------------------------------------------------------ plain tensors
def dev_tables(hip, bd, cqm):
    import torch
    lists = mc.FLAT if cqm == "flat" else mc.JVT
    q = hip.cqm_init(bd, lists)
    dq4, dq8 = hip.cqm_dequant(lists)
    vt = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    q = [torch.from_numpy(a.view(vt[a.dtype])).cuda() for a in q]
    return (q[0], q[1]), (q[2], q[3]), torch.from_numpy(dq4).cuda(), torch.from_numpy(dq8).cuda()


def pix_t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()


def _np_pix(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


def run_plain(hip, case, dec, recon=None, recon_c=None):
    """the two wrappers on dense tensors, in place, the intra call on the dict the inter call
    returned; recon / recon_c: plane tuples already on the device (default the case's prediction).
    Returns (outputs as numpy, the dict, recon, recon_c)."""
    import torch
    q4, q8, dq4, dq8 = dev_tables(hip, case.bd, case.cqm)
    W = 16 * case.mbw

    def dense(a):
        return (pix_t(a), 0, W, a.shape[1] * W)
    cf = case.cf
    recon = dense(case.pred_y) if recon is None else recon
    if cf and recon_c is None:
        recon_c = dense(case.pred_c)
    fenc, fenc_c = dense(case.fenc_y), dense(case.fenc_c) if cf else None
    qp, fl = torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda()
    out = None
    if not case.all_intra:
        out = hip.mb_encode_inter(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl, q4, dq4, quant8=q8, dequant8_mf=dq8,
                                  chroma_format=cf, fenc_chroma=fenc_c, pred_chroma=recon_c if cf else None,
                                  b_dct_decimate=dec, qp_table=case.qp_table)
    out = hip.mb_encode_intra(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl, torch.from_numpy(case.pred_mode).cuda(),
                              q4, dq4, quant8=q8, dequant8_mf=dq8, chroma_format=cf, fenc_chroma=fenc_c,
                              recon_chroma=recon_c if cf else None,
                              chroma_pred_mode=torch.from_numpy(case.chroma_pred_mode).cuda() if cf else None,
                              b_dct_decimate=dec, qp_table=case.qp_table, outs=out)
    torch.cuda.synchronize()
    res = types.SimpleNamespace(**{n: out[n].cpu().numpy() for n in hip.MBINTRA_OUTPUTS})
    return res, out, recon, recon_c


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2])
def test_decoder_agreement_on_device_outputs(hip, bd, cf):
    """the device's own level / luma_dc / chroma_dc decode to the device's own recon"""
    case = mi.make_case(bd, cf, 24, 14, 2)
    out, _, recon, recon_c = run_plain(hip, case, 1)
    ry, rc = mi.decode(case, out)
    assert np.array_equal(ry, _np_pix(recon[0], bd))
    assert np.array_equal(rc, _np_pix(recon_c[0], bd))
    assert not out.level[out.nnz.repeat(16, 1).reshape(out.level.shape) == 0].any()


def test_zero_macroblocks_and_refusals(hip):
    import torch
    case = mi.make_case(8, 1, 3, 1, 1, "flat", 0, True)
    q4, q8, dq4, dq8 = dev_tables(hip, 8, "flat")
    y, c = pix_t(case.pred_y), pix_t(case.pred_c)
    before, before_c = y.clone(), c.clone()
    lvl = torch.full((3 * 48 * 16,), 0x5A5A, dtype=torch.int16, device="cuda")
    args = dict(mb_height=1, qp=torch.from_numpy(case.qp).cuda(), mb_flags=torch.from_numpy(case.flags).cuda(),
                pred_mode=torch.from_numpy(case.pred_mode).cuda(), quant4=q4, dequant4_mf=dq4, quant8=q8, dequant8_mf=dq8,
                chroma_format=1, chroma_pred_mode=torch.from_numpy(case.chroma_pred_mode).cuda(), outs={"level": lvl})
    fenc, fenc_c = (pix_t(case.fenc_y), 0, 48, 48 * 16), (pix_t(case.fenc_c), 0, 48, 48 * 8)
    for mbw, nf in ((0, 1), (3, 0)):
        hip.mb_encode_intra(fenc, (y, 0, 48, 48 * 16), mbw, nframes=nf, fenc_chroma=fenc_c, recon_chroma=(c, 0, 48, 48 * 8),
                            **args)
    torch.cuda.synchronize()
    assert torch.equal(y, before) and torch.equal(c, before_c) and bool((lvl == 0x5A5A).all())
    for bad in (dict(recon=(y, 0, 50, 48 * 16)), dict(recon=(y, 2, 48, 48 * 16)), dict(recon_chroma=(c, 0, 48, 48 * 8 + 2)),
                dict(recon_chroma=(c, 1, 48, 48 * 8))):
        kw = dict(recon=(y, 0, 48, 48 * 16), recon_chroma=(c, 0, 48, 48 * 8))
        kw.update(bad)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            hip.mb_encode_intra(fenc, kw["recon"], 3, nframes=1, fenc_chroma=fenc_c, recon_chroma=kw["recon_chroma"], **args)
    torch.cuda.synchronize()
    assert torch.equal(y, before) and torch.equal(c, before_c) and bool((lvl == 0x5A5A).all())


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("bd", [8, 10])
def test_chain_mc_encode_deblock(hip, bd):
    """mb_mc -> mb_encode_inter -> mb_encode_intra -> deblock_strength -> deblock_frames on the
    device, nothing read back in between, against the checkers chained the same way"""
    import torch
    import deblock_cases as dc
    import mc_cases as mcc
    cf, mbw, mbh, nf = 1, 5, 4, 2
    W, H = 16 * mbw, 16 * mbh
    base = mi.make_case(bd, cf, mbw, mbh, nf)
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
    enc = mi.encode(case, 1)
    mv0 = np.repeat(np.repeat(mv.reshape(nf, mbh, mbw, 2), 4, 1), 4, 2).astype(np.int16)
    intra = (case.flags & mi.INTRA).reshape(nf, mbh, mbw) != 0
    assert intra.any() and not intra.all()
    ref0 = np.where(np.repeat(np.repeat(intra, 2, 1), 2, 2), -1, 0).astype(np.int8)
    bs = dc.deblock_strength_py(enc.nz, enc.flags_out, [mv0], [ref0], mbw, mbh, nf)
    dcase = types.SimpleNamespace(bd=bd, cf=cf, mbw=mbw, mbh=mbh, nf=nf, alpha_c0_offset=0, beta_offset=0,
                                  chroma_qp_index_offset=0, luma=enc.recon_y, chroma=[enc.recon_c], qp=case.qp,
                                  mb_flags=enc.flags_out, bs=bs.reshape(-1, 2, 4, 4), slice_table=None,
                                  chroma_qp_table=case.qp_table)
    want_y, want_c = dc.deblock(dcase)
    # the device
    luma = [pix_t(a) for a in ref.luma]
    nv = [pix_t(a) for a in ref.chroma]
    pos_t, par_t = torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda()
    p, pc = hip.mb_mc(luma, None, ref.origin, ref.stride, 0, pos_t, par_t, None,
                      chroma=(cf, nv, None, ref.corigin, ref.cs))
    ptup = (p, ref.origin, ref.stride, p[0].numel())
    ctup = (pc[0], ref.corigin, ref.cs, pc[0][0].numel())
    q4, q8, dq4, dq8 = dev_tables(hip, bd, "flat")
    qp_t, fl_t = torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda()
    fenc, fenc_c = (pix_t(case.fenc_y), 0, W, H * W), (pix_t(case.fenc_c), 0, W, H // 2 * W)
    out = hip.mb_encode_inter(fenc, ptup, mbw, mbh, nf, qp_t, fl_t, q4, dq4, quant8=q8, dequant8_mf=dq8, chroma_format=cf,
                              fenc_chroma=fenc_c, pred_chroma=ctup, b_dct_decimate=1, qp_table=case.qp_table)
    out = hip.mb_encode_intra(fenc, ptup, mbw, mbh, nf, qp_t, fl_t, torch.from_numpy(case.pred_mode).cuda(), q4, dq4,
                              quant8=q8, dequant8_mf=dq8, chroma_format=cf, fenc_chroma=fenc_c, recon_chroma=ctup,
                              chroma_pred_mode=torch.from_numpy(case.chroma_pred_mode).cuda(), b_dct_decimate=1,
                              qp_table=case.qp_table, outs=out)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], torch.from_numpy(mv0).cuda(), torch.from_numpy(ref0).cuda(),
                                mbw, mbh, nf)
    hip.deblock_frames(p, ref.origin, ref.stride, mbw, mbh, qp_t, out["flags_out"], bs_t,
                       chroma=(cf, [pc[0]], ref.corigin, ref.cs), qp_table=case.qp_table)
    torch.cuda.synchronize()
    got_y = _np_pix(p, bd)[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W]
    got_c = _np_pix(pc[0], bd)[:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W]
    assert np.array_equal(out["nz"].cpu().numpy(), enc.nz) and np.array_equal(bs_t.cpu().numpy().reshape(bs.shape), bs)
    assert np.array_equal(out["flags_out"].cpu().numpy(), enc.flags_out)
    assert np.array_equal(got_y, want_y.astype(got_y.dtype)) and np.array_equal(got_c, want_c[0].astype(got_c.dtype))
    assert (enc.recon_y != case.pred_y).any() and (want_y != enc.recon_y).any()


# ------------------------------------------------------------------ stream order and guard bands
def _row(key, shift):
    return types.SimpleNamespace(name="mb_encode_intra", entries=("mb_encode_inter", "mb_encode_intra"), cases=[("case", {})],
                                 setup=lambda ar, bd: setup(ar, bd, key, shift), call=call, variants=[],
                                 variant_case=lambda bd, case: True)


@pytest.mark.parametrize("bd", [8, 10])
def test_side_stream_behind_a_delay(hip, bd):
    """on a non-default stream behind the delay kernel the calls (a launch per diagonal) wait for
    their stream (the inputs land after they are enqueued) and leave the bytes of the null-stream run"""
    import torch
    import stream_cases as sc
    key = (bd, 1, 5, 4, 2, "flat", 0, False)
    p = sc.Prepared(_row(key, 0), bd)
    want = sc.null_run(hip, p)
    stream = torch.cuda.Stream()
    got, ended = sc.side_run(hip, p, stream)
    assert not ended, "the delay had ended when the call returned: the run shows nothing"
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    ar = fp.Arena(FILL)
    c = setup(ar, bd, key, 0)
    assert np.array_equal(want, expected_bytes(ar, c, 1))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("key", [(2, 5, 4, 2, "flat", 0, False), (1, 5, 4, 1, "flat", 0, True)])
def test_guard_bands(hip, bd, key):
    """two arenas filled with different bytes, the intra macroblocks' own initial recon pixels
    included: nothing outside the documented footprint changes, and inside it the two runs agree
    (no result depends on a guard byte or on an intra macroblock's prior content)"""
    import torch
    runs = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill)
        c = setup(ar, bd, (bd,) + key, 1)
        dev = ar.device()
        call(hip, c, dev)
        torch.cuda.synchronize()
        runs.append((ar, c, dev.cpu().numpy()))
    (a1, c1, after1), (a2, _, after2) = runs
    fp.check_arena(a1, after1, a2, after2, masks(c1))
