"""GPU: x264hip_*_mb_encode_inter against the checker of tests/mbenc_cases.py, bit-exact in every
output array.

Every buffer of a call is carved out of one byte arena (tests/footprint.py): planes stand between
guard rows with frame strides larger than the plane and a different stride each (fenc, pred,
recon), lists between guard bytes, and each per-macroblock output array is handed over one element
into its buffer, so it has a sentinel element either side and loses its 16-byte alignment.  The
whole arena is compared with the bytes expected after the call, which also says that the elements
of intra macroblocks, the guards and the inputs are untouched."""
import types

import numpy as np
import pytest

import footprint as fp
import mbenc_cases as mc

pytestmark = pytest.mark.gpu

FILL = fp.FILLS[0]
OUT_WIDTH = {"level": 48 * 16, "chroma_dc": 16, "nnz": 48, "cbp": 1, "nz": 1, "flags_out": 1}


def pdt(bd):
    return np.uint8 if bd == 8 else np.uint16


def cdt(bd):
    return np.int16 if bd == 8 else np.int32


def T(buf, dev):
    return buf.dt(dev) if isinstance(buf, fp.ListBuf) else buf.t(dev)


def _inner_of(buf, full):
    """the picture (no padding) inside a plane buffer's whole region: [nframes, height, width]"""
    r, c = buf.guard_rows + buf.pad_y, buf.pad_x
    return full[:, r:r + buf.height, c:c + buf.width]


def _inner(buf, host):
    return _inner_of(buf, buf.np(host))


def setup(ar, bd, key, alias, shift):
    """carve the buffers of one call; alias: reconstruct in place; shift: the output arrays start
    `shift` elements into their buffers"""
    case = mc.make_case(*key)
    tb = mc.tables(bd, case.cqm)
    nf, W, H, CH = case.nframes, 16 * case.mbw, 16 * case.mbh, case.chroma_rows * case.mbh
    c = types.SimpleNamespace(case=case, bd=bd, alias=alias, shift=shift, planes={})

    def plane(name, h, data, extra):
        b = ar.plane(name, nf, W, h, pdt(bd), extra=extra)
        if data is not None:
            _inner(b, ar.host)[...] = data
        c.planes[name] = b
        return b
    plane("fenc", H, case.fenc_y, 0)
    plane("pred", H, case.pred_y, 16)
    if not alias:
        plane("recon", H, None, 32)
    if case.cf:
        plane("fenc_c", CH, case.fenc_c, 32)
        plane("pred_c", CH, case.pred_c, 0)
        if not alias:
            plane("recon_c", CH, None, 16)
    c.qp = ar.list("qp", case.nmb, np.int8, case.qp)
    c.flags = ar.list("flags", case.nmb, np.uint8, case.flags)
    ut = orc_udt(bd)
    c.tabs = [ar.list(n, a.shape, a.dtype, a) for n, a in (("q4m", tb.q4m.astype(ut)), ("q4b", tb.q4b.astype(ut)),
                                                          ("q8m", tb.q8m.astype(ut)), ("q8b", tb.q8b.astype(ut)),
                                                          ("dq4", tb.dq4), ("dq8", tb.dq8))]
    dts = {"level": cdt(bd), "chroma_dc": cdt(bd), "nnz": np.uint8, "cbp": np.int32, "nz": np.int32,
           "flags_out": np.uint8}
    c.outs = {n: ar.list(n, case.nmb * w + 2 * shift, dts[n]) for n, w in OUT_WIDTH.items()}
    return c


def orc_udt(bd):
    return np.uint16 if bd == 8 else np.uint32


def _tuple(buf, dev):
    return (T(buf, dev), buf.origin, buf.stride, buf.frame_stride)


def call(hip, c, dev, tight=False, dec=1):
    case, p, s = c.case, c.planes, c.shift
    tabs = [T(b, dev) for b in c.tabs]
    outs = {n: T(b, dev)[s:s + case.nmb * OUT_WIDTH[n]] for n, b in c.outs.items()}
    cf = case.cf
    hip.mb_encode_inter(
        _tuple(p["fenc"], dev), _tuple(p["pred"], dev), case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev),
        (tabs[0], tabs[1]), tabs[4], quant8=(tabs[2], tabs[3]), dequant8_mf=tabs[5], chroma_format=cf,
        fenc_chroma=_tuple(p["fenc_c"], dev) if cf else None, pred_chroma=_tuple(p["pred_c"], dev) if cf else None,
        recon=None if c.alias else _tuple(p["recon"], dev),
        recon_chroma=None if c.alias or not cf else _tuple(p["recon_c"], dev),
        b_dct_decimate=dec, qp_table=case.qp_table, outs=outs)


def masks(c):
    """{buffer name: the elements include/x264hip_mbenc.h says the call writes}"""
    case = c.case
    live = (case.flags & mc.INTRA) == 0
    grid = live.reshape(case.nframes, case.mbh, case.mbw)
    out = {}
    for name, rows in (("pred" if c.alias else "recon", 16), ("pred_c" if c.alias else "recon_c", case.chroma_rows)):
        if name in c.planes:
            b = c.planes[name]
            m = b.none()
            r, x = b.guard_rows + b.pad_y, b.pad_x
            m[:, r:r + b.height, x:x + b.width] = np.repeat(np.repeat(grid, rows, 1), 16, 2)
            out[name] = m
    for n, b in c.outs.items():
        pm = np.zeros(b.pshape, bool)
        w = OUT_WIDTH[n]
        pm[c.shift:c.shift + case.nmb * w] = np.repeat(np.ones(case.nmb, bool) if n == "flags_out" else live, w)
        out[n] = b.mask(pm)
    return out


def expected_bytes(ar, c, dec):
    """the arena after the call"""
    case = c.case
    want = mc.expected(case.key, dec)
    host = ar.bytes().copy()
    ms = masks(c)
    for name, exp in (("pred" if c.alias else "recon", want.recon_y), ("pred_c" if c.alias else "recon_c", want.recon_c)):
        if name in c.planes:
            b = c.planes[name]
            full = b.np(host)
            pic = np.zeros(full.shape, full.dtype)
            _inner_of(b, pic)[...] = exp
            full[ms[name]] = pic[ms[name]]
    for n, b in c.outs.items():
        w = OUT_WIDTH[n]
        data = b.data(host)[c.shift:c.shift + case.nmb * w].reshape(case.nmb, w)
        exp = getattr(want, n).reshape(case.nmb, w)
        rows = np.ones(case.nmb, bool) if n == "flags_out" else (case.flags & mc.INTRA) == 0
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


def run(hip, key, dec, alias, shift):
    import torch
    ar = fp.Arena(FILL)
    c = setup(ar, key[0], key, alias, shift)
    dev = ar.device()
    call(hip, c, dev, dec=dec)
    torch.cuda.synchronize()
    got, want = dev.cpu().numpy(), expected_bytes(ar, c, dec)
    assert np.array_equal(got, want), (key, dec, alias, shift, report(ar, got, want))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [0, 1, 2])
@pytest.mark.parametrize("dec", [0, 1])
def test_mb_encode_inter_bit_exact(hip, bd, cf, dec):
    """every shape of the case list: 1x1 and 3x1 (a partly filled wave), 5x4 x 2 frames (mixed flags
    inside a wave, a frame stride, a last workgroup half full), 24x14 x 2 frames (many workgroups);
    recon apart from pred with aligned arrays, and in place with the arrays one element off"""
    keys = mc.gpu_keys("shapes", bd=bd, cf=cf, dec=dec)
    assert len(keys) == len(mc.SHAPES)
    for key, dec in keys:
        run(hip, key, dec, alias=False, shift=0)
        run(hip, key, dec, alias=True, shift=1)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2])
def test_mb_encode_inter_custom_matrices(hip, bd, cf):
    """the JVT matrices: the luma, chroma and 8x8 lists differ from each other"""
    (key, dec), = mc.gpu_keys("jvt", bd=bd, cf=cf)
    run(hip, key, dec, alias=False, shift=1)


@pytest.mark.parametrize("key,dec", mc.gpu_keys("boundary"), ids=lambda v: "%dbit-cf%d-%s" % (v[0], v[1], v[5]) if isinstance(v, tuple) else None)
def test_boundary_cases_bit_exact(hip, key, dec):
    """the macroblocks of mbenc_cases.BOUNDARY, each with one comparison of the reference exactly on
    its bound (a decimate score of 4 / 6 / 7, chroma qp 18, var2 and ssd on the early-out's
    thresholds, dmf = 32 * 64): a kernel that ties one of them the other way differs here"""
    try:
        run(hip, key, dec, alias=False, shift=0)
        run(hip, key, dec, alias=True, shift=1)
    except AssertionError as e:
        raise AssertionError("%s\nmacroblocks: %s" % (e, list(enumerate(mc.boundary_recipe(key[1], key[5])[3]))))


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


def run_plain(hip, case, dec, pred=None, pred_c=None):
    """the wrapper on dense tensors, in place; pred / pred_c: (tensor, origin, stride, frame stride)
    of planes already on the device.  Returns (outputs as numpy, pred, pred_c tuples)."""
    import torch
    q4, q8, dq4, dq8 = dev_tables(hip, case.bd, case.cqm)
    W = 16 * case.mbw

    def dense(a):
        return (pix_t(a), 0, W, a.shape[1] * W)
    pred = dense(case.pred_y) if pred is None else pred
    cf = case.cf
    if cf and pred_c is None:
        pred_c = dense(case.pred_c)
    out = hip.mb_encode_inter(dense(case.fenc_y), pred, case.mbw, case.mbh, case.nframes,
                              torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda(), q4, dq4, quant8=q8,
                              dequant8_mf=dq8, chroma_format=cf, fenc_chroma=dense(case.fenc_c) if cf else None,
                              pred_chroma=pred_c if cf else None, b_dct_decimate=dec, qp_table=case.qp_table)
    torch.cuda.synchronize()
    res = types.SimpleNamespace(**{n: out[n].cpu().numpy() for n in hip.MBENC_OUTPUTS})
    return res, pred, pred_c


def _np_pix(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("cf", [1, 2])
def test_decoder_agreement_on_device_outputs(hip, bd, cf):
    """the device's own level / chroma_dc decode to the device's own recon"""
    case = mc.make_case(bd, cf, 24, 14, 2)
    out, pred, pred_c = run_plain(hip, case, 1)
    ry, rc = mc.decode(case, out)
    assert np.array_equal(ry, _np_pix(pred[0], bd))
    assert np.array_equal(rc, _np_pix(pred_c[0], bd))


def test_zero_macroblocks_and_refusals(hip):
    import torch
    case = mc.make_case(8, 1, 3, 1, 1)
    q4, q8, dq4, dq8 = dev_tables(hip, 8, "flat")
    y, c = pix_t(case.pred_y), pix_t(case.pred_c)
    before = y.clone()
    lvl = torch.full((3 * 48 * 16,), 0x5A5A, dtype=torch.int16, device="cuda")
    args = dict(mb_height=1, qp=torch.from_numpy(case.qp).cuda(), mb_flags=torch.from_numpy(case.flags).cuda(),
                quant4=q4, dequant4_mf=dq4, quant8=q8, dequant8_mf=dq8, chroma_format=1, outs={"level": lvl})
    fenc, fenc_c = (pix_t(case.fenc_y), 0, 48, 48 * 16), (pix_t(case.fenc_c), 0, 48, 48 * 8)
    for mbw, nf in ((0, 1), (3, 0)):
        hip.mb_encode_inter(fenc, (y, 0, 48, 48 * 16), mbw, nframes=nf, fenc_chroma=fenc_c, pred_chroma=(c, 0, 48, 48 * 8),
                            **args)
    torch.cuda.synchronize()
    assert torch.equal(y, before) and bool((lvl == 0x5A5A).all())
    for bad in (dict(pred=(y, 0, 50, 48 * 16)), dict(pred=(y, 2, 48, 48 * 16)), dict(pred_chroma=(c, 0, 48, 48 * 8 + 2))):
        kw = dict(pred=(y, 0, 48, 48 * 16), pred_chroma=(c, 0, 48, 48 * 8))
        kw.update(bad)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            hip.mb_encode_inter(fenc, kw["pred"], 3, nframes=1, fenc_chroma=fenc_c, pred_chroma=kw["pred_chroma"], **args)
    torch.cuda.synchronize()
    assert torch.equal(y, before) and bool((lvl == 0x5A5A).all())


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("bd", [8, 10])
def test_chain_mc_encode_deblock(hip, bd):
    """mb_mc -> mb_encode_inter -> deblock_strength -> deblock_frames on the device, nothing read
    back in between, against the checkers chained the same way"""
    import torch
    import deblock_cases as dc
    import mc_cases as mcc
    cf, mbw, mbh, nf = 1, 5, 4, 2
    W, H = 16 * mbw, 16 * mbh
    base = mc.make_case(bd, cf, mbw, mbh, nf)
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
    enc = mc.encode(case, 1)
    mv0 = np.repeat(np.repeat(mv.reshape(nf, mbh, mbw, 2), 4, 1), 4, 2).astype(np.int16)
    intra = (case.flags & mc.INTRA).reshape(nf, mbh, mbw) != 0
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
    out = hip.mb_encode_inter((pix_t(case.fenc_y), 0, W, H * W), ptup, mbw, mbh, nf, qp_t, fl_t, q4, dq4, quant8=q8,
                              dequant8_mf=dq8, chroma_format=cf, fenc_chroma=(pix_t(case.fenc_c), 0, W, H // 2 * W),
                              pred_chroma=ctup, b_dct_decimate=1, qp_table=case.qp_table)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], torch.from_numpy(mv0).cuda(), torch.from_numpy(ref0).cuda(),
                                mbw, mbh, nf)
    hip.deblock_frames(p, ref.origin, ref.stride, mbw, mbh, qp_t, out["flags_out"], bs_t,
                       chroma=(cf, [pc[0]], ref.corigin, ref.cs), qp_table=case.qp_table)
    torch.cuda.synchronize()
    got_y = _np_pix(p, bd)[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W]
    got_c = _np_pix(pc[0], bd)[:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W]
    assert np.array_equal(out["nz"].cpu().numpy(), enc.nz) and np.array_equal(bs_t.cpu().numpy().reshape(bs.shape), bs)
    assert np.array_equal(got_y, want_y.astype(got_y.dtype)) and np.array_equal(got_c, want_c[0].astype(got_c.dtype))
    assert (enc.recon_y != case.pred_y).any() and (want_y != enc.recon_y).any()


# ------------------------------------------------------------------ stream order and guard bands
def _row(key, alias, shift):
    return types.SimpleNamespace(name="mb_encode_inter", entries=("mb_encode_inter",), cases=[("case", {})],
                                 setup=lambda ar, bd: setup(ar, bd, key, alias, shift), call=call, variants=[],
                                 variant_case=lambda bd, case: True)


@pytest.mark.parametrize("bd", [8, 10])
def test_side_stream_behind_a_delay(hip, bd):
    """on a non-default stream behind the delay kernel the call waits for its stream (the inputs land
    after it is enqueued) and leaves the bytes of the null-stream run"""
    import torch
    import stream_cases as sc
    p = sc.Prepared(_row((bd, 1, 5, 4, 2, "flat", 0), False, 0), bd)
    want = sc.null_run(hip, p)
    stream = torch.cuda.Stream()
    got, ended = sc.side_run(hip, p, stream)
    assert not ended, "the delay had ended when the call returned: the run shows nothing"
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    ar = fp.Arena(FILL)
    c = setup(ar, bd, (bd, 1, 5, 4, 2, "flat", 0), False, 0)
    assert np.array_equal(want, expected_bytes(ar, c, 1))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("alias", [False, True])
def test_guard_bands(hip, bd, alias):
    """two arenas filled with different bytes: nothing outside the documented footprint changes, and
    inside it the two runs agree (no result depends on a guard byte)"""
    import torch
    key = (bd, 2, 5, 4, 2, "flat", 0)
    runs = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill)
        c = setup(ar, bd, key, alias, 1)
        dev = ar.device()
        call(hip, c, dev)
        torch.cuda.synchronize()
        runs.append((ar, c, dev.cpu().numpy()))
    (a1, c1, after1), (a2, _, after2) = runs
    fp.check_arena(a1, after1, a2, after2, masks(c1))
