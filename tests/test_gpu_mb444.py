"""GPU: x264hip_*_mb_encode_inter_444 and x264hip_*_mb_encode_intra_444 against the checker of
tests/mb444_cases.py, bit-exact in every output array.

As tests/test_gpu_mbenc.py and tests/test_gpu_mbintra.py: every buffer of a run is carved out of one
byte arena (tests/footprint.py), the nine planes between guard rows (Y, and U / V which share
theirs, of fenc, pred and recon: six strides, all different), lists between guard bytes, each
output array optionally one element into its buffer, and the whole arena is compared with the
bytes expected after the calls.  A mixed picture runs the inter entry, then the intra entry on
the same recon planes and arrays; an I picture the intra entry alone.  Before the calls the
recon pixels of the intra macroblocks hold the arena's fill.  No test passes an invalid mode."""
import types

import numpy as np
import pytest

import footprint as fp
import mb444_cases as m4

pytestmark = pytest.mark.gpu

FILL = fp.FILLS[0]
OUT_WIDTH = {"level": 48 * 16, "nnz": 48, "cbp": 1, "nz": 1, "flags_out": 1, "luma_dc": 48}
EXTRA = {"fenc": (0, 48), "pred": (32, 80), "recon": (16, 96)}   # stride slack of (Y, U and V)


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


def intra_grid(case):
    """[nframes, 16*mbh, 16*mbw] bool: the pixels of the intra macroblocks"""
    g = ((case.flags & m4.INTRA) != 0).reshape(case.nframes, case.mbh, case.mbw)
    return np.repeat(np.repeat(g, 16, 1), 16, 2)


def setup(ar, bd, key, shift, apart=False, pred=None):
    """carve the buffers of one run.  shift: the output arrays start `shift` elements into their
    buffers.  In place recon is pred, with the arena's fill over the intra macroblocks; apart it
    is three planes of its own that start as fill.  pred: other prediction planes than the case's."""
    case = m4.make_case(*key)
    tb = m4.tables(bd, case.cqm)
    nf, W, H = case.nframes, 16 * case.mbw, 16 * case.mbh
    c = types.SimpleNamespace(case=case, bd=bd, shift=shift, apart=apart, planes={})
    grid = intra_grid(case)

    def planes(name, data, holes):
        for p in range(3):
            b = ar.plane("%s%d" % (name, p), nf, W, H, pdt(bd), extra=EXTRA[name][p != 0])
            if data is not None:
                pic = _inner_of(b, b.np(ar.host))
                pic[...] = data[p]
                if holes:
                    pic[grid] = fp.fill_value(pdt(bd), ar.fill)
            c.planes[name, p] = b
        assert c.planes[name, 1].stride == c.planes[name, 2].stride != c.planes[name, 0].stride
    planes("fenc", case.fenc, False)
    planes("pred", case.pred if pred is None else pred, not apart)
    if apart:
        planes("recon", None, False)
    assert len({c.planes[n, p].stride for n in ("fenc", "pred") + (("recon",) if apart else ()) for p in (0, 1)}) == (6 if apart else 4)
    c.qp = ar.list("qp", case.nmb, np.int8, case.qp)
    c.flags = ar.list("flags", case.nmb, np.uint8, case.flags)
    c.pmode = ar.list("pred_mode", case.nmb * 16, np.int8, case.pred_mode)
    ut = udt(bd)
    c.tabs = [ar.list(n, a.shape, a.dtype, a) for n, a in (("q4m", tb.q4m.astype(ut)), ("q4b", tb.q4b.astype(ut)),
                                                          ("q8m", tb.q8m.astype(ut)), ("q8b", tb.q8b.astype(ut)),
                                                          ("dq4", tb.dq4), ("dq8", tb.dq8))]
    dts = {"level": cdt(bd), "nnz": np.uint8, "cbp": np.int32, "nz": np.int32, "flags_out": np.uint8, "luma_dc": cdt(bd)}
    c.outs = {n: ar.list(n, case.nmb * w + 2 * shift, dts[n]) for n, w in OUT_WIDTH.items()}
    return c


def _picture(c, name, dev):
    y, u, v = (c.planes[name, p] for p in range(3))
    assert (u.origin, u.frame_stride) == (v.origin, v.frame_stride)
    return ((T(y, dev), y.origin, y.stride, y.frame_stride), ([T(u, dev), T(v, dev)], u.origin, u.stride, u.frame_stride))


def call(hip, c, dev, tight=False, dec=1, stream=None):
    """mb_encode_inter_444 (unless the picture is all intra), then mb_encode_intra_444"""
    case, s = c.case, c.shift
    tabs = [T(b, dev) for b in c.tabs]
    outs = {n: T(b, dev)[s:s + case.nmb * OUT_WIDTH[n]] for n, b in c.outs.items()}
    fenc, pred = _picture(c, "fenc", dev), _picture(c, "pred", dev)
    recon = _picture(c, "recon", dev) if c.apart else pred
    common = dict(quant8=(tabs[2], tabs[3]), dequant8_mf=tabs[5], b_dct_decimate=dec, qp_table=case.qp_table, outs=outs,
                  stream=stream)
    if not case.all_intra:
        hip.mb_encode_inter_444(fenc, pred, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev),
                                (tabs[0], tabs[1]), tabs[4], recon=recon, **common)
    hip.mb_encode_intra_444(fenc, recon, case.mbw, case.mbh, case.nframes, T(c.qp, dev), T(c.flags, dev), T(c.pmode, dev),
                            (tabs[0], tabs[1]), tabs[4], **common)


def masks(c):
    """{buffer name: the elements the two calls write}: every pixel of the three recon pictures and
    every element of the arrays (each macroblock belongs to one call), luma_dc of the intra ones"""
    case = c.case
    out = {}
    for p in range(3):
        b = c.planes["recon" if c.apart else "pred", p]
        out[b.name] = b.rect(0, b.width, 0, b.height)
    intra = (case.flags & m4.INTRA) != 0
    for n, b in c.outs.items():
        pm = np.zeros(b.pshape, bool)
        w = OUT_WIDTH[n]
        pm[c.shift:c.shift + case.nmb * w] = np.repeat(intra if n == "luma_dc" else np.ones(case.nmb, bool), w)
        out[n] = b.mask(pm)
    return out


def expected_bytes(ar, c, want):
    """the arena after the calls; want: mb444_cases.encode's result for what the arena holds"""
    case = c.case
    host = ar.bytes().copy()
    for p in range(3):
        b = c.planes["recon" if c.apart else "pred", p]
        _inner_of(b, b.np(host))[...] = want.recon[p]
    intra = (case.flags & m4.INTRA) != 0
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


def run(hip, key, dec, shift, apart):
    import torch
    ar = fp.Arena(FILL)
    c = setup(ar, key[0], key, shift, apart)
    dev = ar.device()
    call(hip, c, dev, dec=dec)
    torch.cuda.synchronize()
    got, want = dev.cpu().numpy(), expected_bytes(ar, c, m4.expected(key, dec))
    assert np.array_equal(got, want), (key, dec, shift, apart, report(ar, got, want))


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("apart", [False, True], ids=["inplace", "apart"])
def test_mb_encode_444_bit_exact(hip, bd, dec, apart):
    """every shape -- 1x1x1 (one wave, no neighbour), 3x1x1, 5x4 x 2 frames, 7x3 x 3 frames (63
    macroblocks: no multiple of the four a workgroup of the inter kernel holds, diagonals of 1..3
    macroblocks per frame) -- as a mixed picture (inter entry, then intra entry) and as an I picture,
    and 1x3x1 and 2x2x1 (one and two macroblocks wide: diagonals that start below row 0) as I
    pictures, flat matrices, the output arrays aligned and one element off"""
    keys = m4.gpu_keys("shapes", bd=bd, dec=dec)
    assert len(keys) == 2 * len(m4.SHAPES) - len(m4.I_ONLY_SHAPES)
    for i, (key, dec) in enumerate(keys):
        run(hip, key, dec, shift=(i + apart) & 1, apart=apart)
        if not apart:
            run(hip, key, dec, shift=(i + 1) & 1, apart=False)


@pytest.mark.parametrize("bd", [8, 10])
def test_mb_encode_444_distinct_matrices(hip, bd):
    """eight pairwise different lists: every plane of every kind of macroblock reads its own
    category (a mixed 7x3x3 and a 5x4x2 I picture)"""
    for key, dec in m4.gpu_keys("distinct", bd=bd):
        run(hip, key, dec, shift=1, apart=False)


@pytest.mark.parametrize("key,dec", m4.gpu_keys("boundary"), ids=lambda v: "%dbit" % v[0] if isinstance(v, tuple) else None)
def test_boundary_cases_bit_exact(hip, key, dec):
    """the macroblocks of mb444_cases.BOUNDARY: the decimate score that runs on through the planes is
    exactly 6 when plane 0, 1 or 2 ends, with either transform; a kernel that drops a plane at 6
    differs here"""
    try:
        run(hip, key, dec, shift=0, apart=False)
        run(hip, key, dec, shift=1, apart=True)
    except AssertionError as e:
        raise AssertionError("%s\nmacroblocks: %s" % (e, [(i, n) for i, (n, _) in enumerate(m4.BOUNDARY)]))


# ------------------------------------------------------------------ plain tensors
def dev_tables(hip, bd, cqm):
    """the product's own table functions, on the device"""
    import torch
    lists = m4.lists_of(cqm)
    q = hip.cqm_init444(bd, lists)
    dq4, dq8 = hip.cqm_dequant444(lists)
    vt = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    q = [torch.from_numpy(a.view(vt[a.dtype])).cuda() for a in q]
    return (q[0], q[1]), (q[2], q[3]), torch.from_numpy(dq4).cuda(), torch.from_numpy(dq8).cuda()


def pix_t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()


def _np_pix(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


def dense(planes):
    """a dense picture tuple of three [n, H, W] arrays"""
    n, H, W = planes[0].shape
    y, u, v = (pix_t(a) for a in planes)
    return ((y, 0, W, H * W), ([u, v], 0, W, H * W))


def run_plain(hip, case, dec, cqm="flat"):
    """the two wrappers on dense tensors with the product's tables, in place, the intra call on the
    dict the inter call returned.  Returns (outputs as numpy, recon planes as numpy)."""
    import torch
    q4, q8, dq4, dq8 = dev_tables(hip, case.bd, cqm)
    fenc, recon = dense(case.fenc), dense(case.pred)
    qp, fl = torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda()
    out = hip.mb_encode_inter_444(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl, q4, dq4, quant8=q8, dequant8_mf=dq8,
                                  b_dct_decimate=dec, qp_table=case.qp_table)
    assert out["recon"] is recon
    out = hip.mb_encode_intra_444(fenc, recon, case.mbw, case.mbh, case.nframes, qp, fl,
                                  torch.from_numpy(case.pred_mode).cuda(), q4, dq4, quant8=q8, dequant8_mf=dq8,
                                  b_dct_decimate=dec, qp_table=case.qp_table, outs=out)
    torch.cuda.synchronize()
    res = types.SimpleNamespace(**{n: out[n].cpu().numpy() for n in hip.MB444_OUTPUTS})
    return res, [_np_pix(t, case.bd) for t in (recon[0][0], *recon[1][0])]


@pytest.mark.parametrize("bd", [8, 10])
def test_decoder_agreement_on_device_outputs(hip, bd):
    """the device's own level / luma_dc decode to the device's own three planes, with the tables
    of cqm_init444 / cqm_dequant444 and the distinct matrices; and they are the checker's"""
    key = m4.DISTINCT_KEYS(bd)[0]
    case = m4.make_case(*key)
    out, recon = run_plain(hip, case, 1, "distinct")
    rec = m4.decode(case, out)
    want = m4.expected(key, 1)
    for p in range(3):
        assert np.array_equal(rec[p], recon[p]) and np.array_equal(recon[p], want.recon[p]), p
    assert not out.level[out.nnz.repeat(16, 1).reshape(out.level.shape) == 0].any()
    for n in ("level", "nnz", "cbp", "nz", "flags_out", "luma_dc"):
        assert np.array_equal(getattr(out, n), getattr(want, n)), n


def test_zero_macroblocks_and_refusals(hip):
    import torch
    case = m4.make_case(8, 3, 1, 1, "flat", m4.SEED, True)
    q4, q8, dq4, dq8 = dev_tables(hip, 8, "flat")
    fenc, recon = dense(case.fenc), dense(case.pred)
    planes = [recon[0][0], *recon[1][0]]
    before = [t.clone() for t in planes]
    lvl = torch.full((3 * 48 * 16,), 0x5A5A, dtype=torch.int16, device="cuda")
    qp, fl = torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda()
    pm = torch.from_numpy(case.pred_mode).cuda()
    tabs = dict(quant4=q4, dequant4_mf=dq4, quant8=q8, dequant8_mf=dq8, outs={"level": lvl})

    def both(recon, mbw, nf):
        hip.mb_encode_inter_444(fenc, recon, mbw, 1, nf, qp, fl, **tabs)
        hip.mb_encode_intra_444(fenc, recon, mbw, 1, nf, qp, fl, pm, **tabs)
    for mbw, nf in ((0, 1), (3, 0)):
        both(recon, mbw, nf)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(planes, before)) and bool((lvl == 0x5A5A).all())
    (y, o, s, fs), (uv, co, cs, cfs) = recon
    for bad in (((y, o, 50, fs), (uv, co, cs, cfs)), ((y, 2, s, fs), (uv, co, cs, cfs)), ((y, o, s, fs), (uv, co, cs, cfs + 2)),
                ((y, o, s, fs), (uv, 1, cs, cfs)), ((y, o, s, fs), (uv, co, 46, cfs))):
        for fn in (lambda: hip.mb_encode_inter_444(fenc, recon, 3, 1, 1, qp, fl, recon=bad, **tabs),
                   lambda: hip.mb_encode_intra_444(fenc, bad, 3, 1, 1, qp, fl, pm, **tabs)):
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                fn()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(planes, before)) and bool((lvl == 0x5A5A).all())


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("bd", [8, 10])
def test_chain_mc_encode_deblock(hip, bd):
    """mb_mc (chroma_format 3) -> mb_encode_inter_444 -> mb_encode_intra_444 -> deblock_strength ->
    deblock_frames (chroma_format 3) on the device, nothing read back in between, against the
    checkers chained the same way"""
    import torch
    import deblock_cases as dc
    import mc_cases as mcc
    mbw, mbh, nf = m4.CHAIN_SHAPE
    W, H = 16 * mbw, 16 * mbh
    base = m4.make_case(bd, mbw, mbh, nf)
    ref = mcc.make_ref(bd, W, H, 3, nf, 7)
    pos = mcc.block_positions(W, H, nf, 0)
    mv = mcc.phase_mvs(pos, W, H, 11)
    mv = (mv // 16) % 5 - 2 + (mv & 3)                            # small vectors: the residual stays codable
    par = mcc.make_par(pos, mv, mv, W, H)
    # the checkers
    pred, pred_c = mcc.pred_planes(ref)
    mcc.mb_mc(bd, 3, 0, ref, None, pos, par, None, (None, None, None), pred, ref.oy, ref.ox, pred_c, ref.coy, ref.cox)
    case = types.SimpleNamespace(**vars(base))
    case.pred = [pred[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W].copy()] + \
        [a[:, ref.coy:ref.coy + H, ref.cox:ref.cox + W].copy() for a in pred_c]
    enc = m4.encode(case, 1)
    mv0 = np.repeat(np.repeat(mv.reshape(nf, mbh, mbw, 2), 4, 1), 4, 2).astype(np.int16)
    intra = (case.flags & m4.INTRA).reshape(nf, mbh, mbw) != 0
    assert intra.any() and not intra.all()
    ref0 = np.where(np.repeat(np.repeat(intra, 2, 1), 2, 2), -1, 0).astype(np.int8)
    bs = dc.deblock_strength_py(enc.nz, enc.flags_out, [mv0], [ref0], mbw, mbh, nf)
    dcase = types.SimpleNamespace(bd=bd, cf=3, mbw=mbw, mbh=mbh, nf=nf, alpha_c0_offset=0, beta_offset=0,
                                  chroma_qp_index_offset=0, luma=enc.recon[0], chroma=enc.recon[1:], qp=case.qp,
                                  mb_flags=enc.flags_out, bs=bs.reshape(-1, 2, 4, 4), slice_table=None,
                                  chroma_qp_table=case.qp_table)
    want_y, want_c = dc.deblock(dcase)
    # the device
    luma = [pix_t(a) for a in ref.luma]
    chroma = [pix_t(a) for a in ref.chroma]
    pos_t, par_t = torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda()
    p, pc = hip.mb_mc(luma, None, ref.origin, ref.stride, 0, pos_t, par_t, None, chroma=(3, chroma, None, ref.corigin, ref.cs))
    assert len(pc) == 2
    picture = ((p, ref.origin, ref.stride, p[0].numel()), (pc, ref.corigin, ref.cs, pc[0][0].numel()))
    q4, q8, dq4, dq8 = dev_tables(hip, bd, "flat")
    qp_t, fl_t = torch.from_numpy(case.qp).cuda(), torch.from_numpy(case.flags).cuda()
    fenc = dense(case.fenc)
    out = hip.mb_encode_inter_444(fenc, picture, mbw, mbh, nf, qp_t, fl_t, q4, dq4, quant8=q8, dequant8_mf=dq8,
                                  b_dct_decimate=1, qp_table=case.qp_table)
    out = hip.mb_encode_intra_444(fenc, picture, mbw, mbh, nf, qp_t, fl_t, torch.from_numpy(case.pred_mode).cuda(), q4, dq4,
                                  quant8=q8, dequant8_mf=dq8, b_dct_decimate=1, qp_table=case.qp_table, outs=out)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], torch.from_numpy(mv0).cuda(), torch.from_numpy(ref0).cuda(),
                                mbw, mbh, nf)
    hip.deblock_frames(p, ref.origin, ref.stride, mbw, mbh, qp_t, out["flags_out"], bs_t,
                       chroma=(3, pc, ref.corigin, ref.cs), qp_table=case.qp_table)
    torch.cuda.synchronize()
    assert np.array_equal(out["nz"].cpu().numpy(), enc.nz) and np.array_equal(bs_t.cpu().numpy().reshape(bs.shape), bs)
    assert np.array_equal(out["flags_out"].cpu().numpy(), enc.flags_out) and np.array_equal(out["cbp"].cpu().numpy(), enc.cbp)
    got_y = _np_pix(p, bd)[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W]
    assert np.array_equal(got_y, want_y.astype(got_y.dtype))
    for k in range(2):
        got_c = _np_pix(pc[k], bd)[:, ref.coy:ref.coy + H, ref.cox:ref.cox + W]
        assert np.array_equal(got_c, want_c[k].astype(got_c.dtype)), k
        assert (enc.recon[1 + k] != case.pred[1 + k]).any() and (want_c[k] != enc.recon[1 + k]).any()
    assert (enc.recon[0] != case.pred[0]).any() and (want_y != enc.recon[0]).any()


# ------------------------------------------------------------------ stream order and guard bands
def _row(key, shift):
    return types.SimpleNamespace(name="mb_encode_444", entries=("mb_encode_inter_444", "mb_encode_intra_444"),
                                 cases=[("case", {})], setup=lambda ar, bd: setup(ar, bd, key, shift), call=call, variants=[],
                                 variant_case=lambda bd, case: True)


@pytest.mark.parametrize("bd", [8, 10])
def test_side_stream_behind_a_delay(hip, bd):
    """on a non-default stream behind the delay kernel both entries (the intra one a launch per
    diagonal) wait for their stream (the inputs land after they are enqueued) and leave the bytes of
    the null-stream run"""
    import torch
    import stream_cases as sc
    key = (bd, 5, 4, 2, "flat", m4.SEED, False)
    p = sc.Prepared(_row(key, 0), bd)
    want = sc.null_run(hip, p)
    stream = torch.cuda.Stream()
    got, ended = sc.side_run(hip, p, stream)
    assert not ended, "the delay had ended when the call returned: the run shows nothing"
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    ar = fp.Arena(FILL)
    c = setup(ar, bd, key, 0)
    assert np.array_equal(want, expected_bytes(ar, c, m4.expected(key, 1)))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("key,apart", [((5, 4, 2, "flat", m4.SEED, False), True), ((7, 3, 3, "flat", m4.SEED, False), False),
                                       ((5, 4, 2, "flat", m4.SEED, True), False)])
def test_guard_bands(hip, bd, key, apart):
    """two arenas filled with different bytes, the intra macroblocks' own initial recon pixels
    included: nothing outside the documented footprint changes, and inside it the two runs agree
    (no result depends on a guard byte or on an intra macroblock's prior content)"""
    import torch
    runs = []
    for fill in fp.FILLS:
        ar = fp.Arena(fill)
        c = setup(ar, bd, (bd,) + key, 1, apart)
        dev = ar.device()
        call(hip, c, dev)
        torch.cuda.synchronize()
        runs.append((ar, c, dev.cpu().numpy()))
    (a1, c1, after1), (a2, _, after2) = runs
    fp.check_arena(a1, after1, a2, after2, masks(c1))
