"""GPU: x264hip_mb_predict_mv_pskip, x264hip_*_mb_probe_skip and x264hip_mb_skip_convert against
the checkers of tests/mbskip_cases.py, bit-exact.

Every output array stands between 4096 guard bytes in a buffer filled with one byte value; a call
runs on two fills, the guards must keep theirs, the two results must agree, and every input must
hold the same bytes afterwards.  The shapes (mb_width, mb_height, frames) are the smallest that
hold no neighbour (1,1,1), no top (3,1,1), the top-left fallback (2,2,1), a frame boundary inside
a wave (5,4,2) and a full workgroup plus a tail (24,14,2)."""
import functools
import types

import numpy as np
import pytest

import mbenc_cases as mbc
import mbskip_cases as ms
import mc_cases as mcc
import stream_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 4096
FILLS = (0xA5, 0x5A)


def pix_t(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


@functools.lru_cache(maxsize=None)
def dev_quant4(hip, bd, cqm):
    import torch
    q = hip.cqm_init(bd, mbc.FLAT if cqm == "flat" else mbc.JVT)
    vt = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    return tuple(torch.from_numpy(a.view(vt[a.dtype])).cuda() for a in q[:2])


def dev_tables(hip, bd):
    """the flat matrices' tables as mb_encode_inter takes them"""
    import torch
    q = hip.cqm_init(bd, mbc.FLAT)
    dq4, dq8 = hip.cqm_dequant(mbc.FLAT)
    vt = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    q = [torch.from_numpy(a.view(vt[a.dtype])).cuda() for a in q]
    return (q[0], q[1]), (q[2], q[3]), torch.from_numpy(dq4).cuda(), torch.from_numpy(dq8).cuda()


def np_pix(t, bd):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bd == 10 else a


class Out:
    """`count` elements of `dtype` between GUARD bytes of `fill`, `shift` elements off the aligned start"""

    def __init__(self, count, dtype, fill, shift=0):
        import torch
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.fill, self.lo, self.n = fill, GUARD + shift * self.size, count * self.size
        self.buf = torch.full((GUARD + 16 + self.n + GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.t = self.buf[self.lo:self.lo + self.n].view(dtype)

    def check(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == self.fill).all() and (b[self.lo + self.n:] == self.fill).all(), "a guard byte changed"
        return self.t.cpu().numpy()


class Inputs:
    """device copies of the inputs, and whether they still hold their bytes"""

    def __init__(self):
        self.kept = []

    def __call__(self, t):
        self.kept.append((t, t.clone()))
        return t

    def check(self):
        import torch
        assert all(torch.equal(a, b) for a, b in self.kept), "an input changed"


# ------------------------------------------------------------------ the skip vector
@pytest.mark.parametrize("shape", ms.SHAPES)
def test_mb_predict_mv_pskip_bit_exact(hip, shape):
    """random fields: mixed partitions, refs -1..2, zero vectors, intra macroblocks"""
    import torch
    mbw, mbh, nf = shape
    assert [e[2] for e in ms.gpu_keys("pskip", shape=shape)] == list(range(len(FILLS)))
    for seed, fill in enumerate(FILLS):
        mv0, ref0 = ms.make_field(mbw, mbh, nf, seed)
        ins = Inputs()
        out = Out(2 * nf * mbw * mbh, torch.int16, fill, shift=2 * seed)
        sc.guarded(lambda: hip.mb_predict_mv_pskip(ins(torch.from_numpy(mv0).cuda()), ins(torch.from_numpy(ref0).cuda()),
                                                   mbw, mbh, nf, pskip_mv=out.t))
        torch.cuda.synchronize()
        assert np.array_equal(out.check().reshape(-1, 2), ms.pskip_mv(mv0, ref0, mbw, mbh)), (shape, seed)
        ins.check()


# ------------------------------------------------------------------ the probe
def probe_args(hip, case, ins, up=pix_t):
    """the wrapper's arguments for a case on dense fenc / pred planes and the padded reference"""
    cf, W, H = case.cf, case.W, case.H

    def dense(planes):
        y = (ins(up(planes[0])), 0, W, H * W)
        if cf == 3:
            return y, ([ins(up(planes[1])), ins(up(planes[2]))], 0, W, H * W)
        if cf:
            return y, (ins(up(planes[1])), 0, W, planes[1].shape[1] * W)
        return y, None
    fenc, fenc_c = dense(case.fenc)
    kw = dict(fenc=fenc, mb_width=case.mbw, mb_height=case.mbh, nframes=case.nframes, qp=ins(up(case.qp)),
              quant4=dev_quant4(hip, case.bd, case.cqm), chroma_format=cf, fenc_chroma=fenc_c, qp_table=case.qp_table)
    if case.leg == "b":
        kw["pred"], kw["pred_chroma"] = dense(case.pred)
    else:
        r = case.ref
        kw["ref"] = ([ins(up(p)) for p in r.luma], r.origin, r.stride)
        if cf:
            kw["ref_chroma"] = ([ins(up(p)) for p in r.chroma], r.corigin, r.cs)
        kw["pskip_mv"] = ins(up(case.pskip_mv))
        kw["weight"] = case.weights
    return kw


def run_probe(hip, key, fill, shift):
    import torch
    case = ms.make_case(*key)
    ins = Inputs()
    out = Out(case.nmb, torch.uint8, fill, shift)
    kw = probe_args(hip, case, ins)
    sc.guarded(lambda: hip.mb_probe_skip(**kw, skip=out.t))
    torch.cuda.synchronize()
    got = out.check()
    want = ms.expected(key)[0]
    assert np.array_equal(got, want), (key, shift, np.flatnonzero(got != want)[:8], case.klass[got != want][:8])
    ins.check()


@pytest.mark.parametrize("leg", ms.LEGS)
@pytest.mark.parametrize("cf", [0, 1, 2, 3])
@pytest.mark.parametrize("bd", [8, 10])
def test_mb_probe_skip_bit_exact(hip, bd, cf, leg):
    """every shape with the flat matrices and 5x4 x 2 with the JVT ones: skip aligned (the four
    results of a wave stored as one dword) and one and three bytes off (stored one by one); the
    cases hold full-scale checker residuals at qp 0 and QP_MAX_SPEC and, at the four corners of
    every frame, skip vectors beyond mv_max / below mv_min"""
    keys = [e[1] for e in ms.gpu_keys("probe", bd=bd, cf=cf, leg=leg)]
    assert len(keys) == len(ms.SHAPES) + 1
    for i, key in enumerate(keys):
        run_probe(hip, key, FILLS[0], 0)
        run_probe(hip, key, FILLS[1], 1 + 2 * (i & 1))


@pytest.mark.parametrize("key", [e[1] for e in ms.gpu_keys("boundary")], ids=lambda k: "%dbit-cf%d-%s" % (k[0], k[1], k[6]))
def test_boundary_cases_bit_exact(hip, key):
    """the macroblocks of mbskip_cases.BOUNDARY on the B leg: a luma score of exactly 6, a chroma AC
    score of exactly 7, a chroma ssd of exactly thresh whose DC still quantises to a level; a kernel
    that ties one of the probe's thresholds the other way answers differently here"""
    try:
        run_probe(hip, key, FILLS[0], 0)
        run_probe(hip, key, FILLS[1], 1)
    except AssertionError as e:
        raise AssertionError("%s\nmacroblocks: %s" % (e, [b[0] for b in ms.BOUNDARY if key[1] in b[1] and (b[3:] or ("flat",))[0] == key[6]]))


# ------------------------------------------------------------------ the conversion
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("bframe", [0, 1])
def test_mb_skip_convert_bit_exact(hip, bframe, alias):
    import torch
    shapes = [e[1] for e in ms.gpu_keys("convert", bframe=bframe)]
    assert shapes == list(ms.SHAPES)
    for shape in shapes:
        c = ms.make_convert_case(*shape, bframe)
        want = ms.skip_convert(c.flags, c.cbp, c.mv0, c.ref0, c.pskip, bframe, c.direct, c.mbw, c.mbh)
        for k, fill in enumerate(FILLS):
            ins = Inputs()
            out = Out(c.nmb, torch.uint8, fill, shift=k)
            if alias:
                out.t.copy_(torch.from_numpy(c.flags))
                fl = out.t
            else:
                fl = ins(torch.from_numpy(c.flags).cuda())
            p = dict(mv0=ins(torch.from_numpy(c.mv0).cuda()), ref0=ins(torch.from_numpy(c.ref0).cuda()),
                     pskip_mv=ins(torch.from_numpy(c.pskip).cuda()))
            b = dict(direct=ins(torch.from_numpy(c.direct).cuda()))
            sc.guarded(lambda: hip.mb_skip_convert(fl, ins(torch.from_numpy(c.cbp).cuda()), c.mbw, c.mbh, c.nframes,
                                                   b_bframe=bool(bframe), flags=out.t, **(b if bframe else p)))
            torch.cuda.synchronize()
            assert np.array_equal(out.check(), want), (shape, bframe, alias, k)
            ins.check()


# ------------------------------------------------------------------ stream order
def test_side_stream_behind_a_delay(hip):
    """each entry on a non-default stream behind the delay kernel: its inputs land on that stream
    after the delay, an event behind the delay is still pending when the call returns, and the
    results are the null-stream ones"""
    import torch
    stream = torch.cuda.Stream()
    pinned = []

    def later(a):
        """a device tensor of a's shape whose bytes arrive on `stream`, behind whatever it holds"""
        a = np.ascontiguousarray(a)
        host = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).pin_memory()
        dev = torch.zeros_like(host, device="cuda")
        pinned.append((dev, host))
        return dev

    def behind_the_delay(enqueue):
        torch.cuda.synchronize()

        def go():
            with torch.cuda.stream(stream):
                torch.cuda._sleep(sc.DELAY_CYCLES)
                ev = torch.cuda.Event()
                ev.record(stream)
                for dev, host in pinned:
                    dev.copy_(host, non_blocking=True)
                enqueue()
                ended = ev.query()
            stream.synchronize()
            return ended
        ended = sc.guarded(go)
        pinned.clear()
        assert not ended, "the delay had ended when the call returned: the run shows nothing"

    mbw, mbh, nf = 5, 4, 2
    mv0, ref0 = ms.make_field(mbw, mbh, nf, 9)
    out = torch.zeros((nf * mbw * mbh, 2), dtype=torch.int16, device="cuda")
    a, b = later(mv0), later(ref0)
    behind_the_delay(lambda: hip.mb_predict_mv_pskip(a, b, mbw, mbh, nf, pskip_mv=out, stream=stream))
    assert np.array_equal(out.cpu().numpy(), ms.pskip_mv(mv0, ref0, mbw, mbh))

    for key in ((8, 1, 5, 4, 2, "pw", "flat", 0), (10, 2, 5, 4, 2, "b", "flat", 0)):
        case = ms.make_case(*key)
        skip = torch.full((case.nmb,), 7, dtype=torch.uint8, device="cuda")
        kw = probe_args(hip, case, lambda t: t, up=later)
        behind_the_delay(lambda: hip.mb_probe_skip(**kw, skip=skip))           # the current stream
        assert np.array_equal(skip.cpu().numpy(), ms.expected(key)[0]), key

    for bframe in (0, 1):
        c = ms.make_convert_case(mbw, mbh, nf, bframe)
        flags = torch.zeros(c.nmb, dtype=torch.uint8, device="cuda")
        t = {n: later(getattr(c, n)) for n in ("flags", "cbp", "mv0", "ref0", "pskip", "direct")}
        kw = dict(direct=t["direct"]) if bframe else dict(mv0=t["mv0"], ref0=t["ref0"], pskip_mv=t["pskip"])
        behind_the_delay(lambda: hip.mb_skip_convert(t["flags"], t["cbp"], mbw, mbh, nf, b_bframe=bool(bframe),
                                                     flags=flags, stream=stream, **kw))
        want = ms.skip_convert(c.flags, c.cbp, c.mv0, c.ref0, c.pskip, bframe, c.direct, mbw, mbh)
        assert np.array_equal(flags.cpu().numpy(), want), bframe


# ------------------------------------------------------------------ nothing to do, and the refusals
def test_zero_macroblocks_and_refusals(hip):
    import torch
    case = ms.make_case(8, 1, 3, 1, 1, "p")
    ins = Inputs()
    kw = probe_args(hip, case, ins)
    skip = torch.full((3,), 0x5A, dtype=torch.uint8, device="cuda")
    ps = torch.full((3, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    fl = torch.full((3,), 0x5A, dtype=torch.uint8, device="cuda")
    mv0, ref0 = (torch.from_numpy(a).cuda() for a in ms.make_field(3, 1, 1, 0))
    cbp = torch.zeros(3, dtype=torch.int32, device="cuda")
    for mbw, nf in ((0, 1), (3, 0)):
        hip.mb_probe_skip(**{**kw, "mb_width": mbw, "nframes": nf}, skip=skip)
        hip.mb_predict_mv_pskip(mv0, ref0, mbw, 1, nf, pskip_mv=ps)
        hip.mb_skip_convert(fl, cbp, mbw, 1, nf, mv0=mv0, ref0=ref0, pskip_mv=ps, flags=fl)
    torch.cuda.synchronize()
    assert bool((skip == 0x5A).all()) and bool((ps == 0x5A5A).all()) and bool((fl == 0x5A).all())
    # X264HIP_EINVAL reaches the caller as an error: a skip vector array off its 4-byte boundary, a weight's denom
    odd = torch.zeros(8, dtype=torch.int16, device="cuda")[1:7]
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        hip.mb_probe_skip(**{**kw, "pskip_mv": odd}, skip=skip)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        hip.mb_probe_skip(**{**kw, "weight": ((64, 8, 0), None, None)}, skip=skip)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        hip.mb_predict_mv_pskip(mv0, ref0, 3, 1, 1, pskip_mv=odd)
    bad = case.qp_table.copy()
    bad[5] = 52
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        hip.mb_probe_skip(**{**kw, "qp_table": bad}, skip=skip)
    torch.cuda.synchronize()
    assert bool((skip == 0x5A).all()) and bool((ps == 0x5A5A).all())
    ins.check()


# ------------------------------------------------------------------ the chain
def chain_expected(bd):
    """the inputs of test_chain_p_picture and what the Python checkers make of them"""
    import deblock_cases as dc
    cf, mbw, mbh, nf = 1, 5, 4, 2
    W, H, n = 16 * mbw, 16 * mbh, nf * mbw * mbh
    rng = np.random.default_rng([bd, 2640])
    base = mbc.make_case(bd, cf, mbw, mbh, nf)
    ref = mcc.make_ref(bd, W, H, cf, nf, 7)
    # the field: in raster order an intra macroblock, a 16x16 at its skip vector, or a 16x16 elsewhere
    mv0 = np.zeros((nf, 4 * mbh, 4 * mbw, 2), np.int16)
    ref0 = np.zeros((nf, 2 * mbh, 2 * mbw), np.int8)
    intra = rng.random(n) < 0.1
    intra[[3, 27]] = True
    for mb in range(n):
        f, r = divmod(mb, mbw * mbh)
        y, x = divmod(r, mbw)
        m, rf = mv0[f, 4 * y:4 * y + 4, 4 * x:4 * x + 4], ref0[f, 2 * y:2 * y + 2, 2 * x:2 * x + 2]
        if intra[mb]:
            rf[:] = -1
        elif rng.random() < 0.5:
            m[:] = ms.pskip_one(mv0, ref0, f, y, x, mbw)
        else:
            m[:] = rng.choice([-1, 1], 2) * rng.integers(1, 10, 2)
    mv_mb = mv0[:, ::4, ::4].reshape(n, 2).astype(np.int64)
    # fenc = the prediction at the macroblock's vector + nothing, a faint patch, noise at its qp, or a faint
    # patch in each of two 8x8 blocks: a score of 3 + 3 fails the probe's bound of 6, while the encode drops
    # either 8x8 below 4 and leaves nothing coded
    qp = rng.integers(22, 40, n).astype(np.int8)
    py, pu, pv = ms.predict(ref, mv_mb, (None,) * 3, mbw, mbh, nf)
    res = np.zeros((n, 16, 16))
    for mb in range(n):
        k, qs = rng.integers(5), mbc._qstep(int(qp[mb]))
        if k == 1:
            res[mb, 4:8, 8:12] = max(1, round(0.3 * qs))
        elif k == 2:
            res[mb] = rng.normal(0, 0.35 * qs, (16, 16))
        elif k == 3:
            res[mb] = rng.normal(0, 2 * qs, (16, 16))
        elif k == 4:
            res[mb, 4:8, 8:12] = res[mb, 8:12, 0:4] = max(1, round(0.3 * qs))
    pm = (1 << bd) - 1
    pdt = mbc.orc.pixel_dtype(bd)
    fenc = (np.clip(py + np.rint(res).astype(np.int64), 0, pm), pu, pv)
    flags = np.where(intra, mbc.INTRA, mbc.D16).astype(np.uint8) | (base.flags & mbc.T8)

    # ---- the checkers
    want_ps = ms.pskip_mv(mv0, ref0, mbw, mbh)
    pcase = types.SimpleNamespace(bd=bd, cf=cf, cqm="flat", nmb=n, qp=qp, qpc=base.qp_table[qp].astype(np.int64),
                                  blocks=types.SimpleNamespace(fenc=fenc, pred=ms.predict(ref, want_ps, (None,) * 3, mbw, mbh, nf)))
    want_skip, _ = ms.probe(pcase)
    send = (want_skip != 0) & ~intra & (mv_mb == want_ps).all(axis=1)
    flags_in = flags | np.where(send, mbc.SKIP, 0).astype(np.uint8)
    pos = mcc.block_positions(W, H, nf, 0)
    par = mcc.make_par(pos, mv_mb, mv_mb, W, H)
    pred, pred_c = mcc.pred_planes(ref)
    mcc.mb_mc(bd, cf, 0, ref, None, pos, par, None, (None, None, None), pred, ref.oy, ref.ox, pred_c, ref.coy, ref.cox)
    case = types.SimpleNamespace(**vars(base))
    case.qp, case.flags = qp, flags_in
    case.fenc_y = ms.to_plane(fenc[0], mbw, mbh, nf).astype(pdt)
    case.fenc_c = ms.to_plane(ms.interleave(pu, pv), mbw, mbh, nf).astype(pdt)
    case.pred_y = pred[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W].copy()
    case.pred_c = pred_c[0][:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W].copy()
    enc = mbc.encode(case, 1)
    want_flags = ms.skip_convert(flags_in, enc.cbp, mv0, ref0, want_ps, 0, None, mbw, mbh)
    bs = dc.deblock_strength_py(enc.nz, enc.flags_out, [mv0], [ref0], mbw, mbh, nf)
    dcase = types.SimpleNamespace(bd=bd, cf=cf, mbw=mbw, mbh=mbh, nf=nf, alpha_c0_offset=0, beta_offset=0,
                                  chroma_qp_index_offset=0, luma=enc.recon_y, chroma=[enc.recon_c], qp=qp,
                                  mb_flags=enc.flags_out, bs=bs.reshape(-1, 2, 4, 4), slice_table=None,
                                  chroma_qp_table=base.qp_table)
    want_y, want_c = dc.deblock(dcase)
    # the chain means something: skips are sent, macroblocks are coded, and the conversion finds more
    converted = (want_flags & mbc.SKIP != 0) & ~send
    assert send.sum() >= 5 and (enc.cbp != 0).sum() >= 5 and converted.sum() >= 1, (send.sum(), converted.sum())
    moving = want_ps[send].any(axis=1)
    assert moving.any() and not moving.all() and (want_skip != 0).sum() >= send.sum()
    return types.SimpleNamespace(**locals())


@pytest.mark.parametrize("bd", [8, 10])
def test_chain_p_picture(hip, bd):
    """mb_predict_mv_pskip -> mb_probe_skip -> mb_mc (skip macroblocks at the skip vector) ->
    mb_encode_inter -> mb_skip_convert -> deblock_strength -> deblock_frames on the device, against
    the Python checkers chained the same way.  A macroblock is sent as a skip when it probes as one
    and its vector in the field is its skip vector; the others are coded, and the conversion
    catches those that come out empty at their skip vector."""
    import torch
    e = chain_expected(bd)
    cf, mbw, mbh, nf, W, H, n, ref, base, case = e.cf, e.mbw, e.mbh, e.nf, e.W, e.H, e.n, e.ref, e.base, e.case
    mv0, ref0, qp, intra, flags, pos, par = e.mv0, e.ref0, e.qp, e.intra, e.flags, e.pos, e.par
    # nothing is read back until the end
    luma, nv = [pix_t(a) for a in ref.luma], [pix_t(a) for a in ref.chroma]
    mv0_t, ref0_t, qp_t = torch.from_numpy(mv0).cuda(), torch.from_numpy(ref0).cuda(), torch.from_numpy(qp).cuda()
    fenc_t = (pix_t(case.fenc_y), 0, W, H * W)
    fenc_ct = (pix_t(case.fenc_c), 0, W, H // 2 * W)
    q4, q8, dq4, dq8 = dev_tables(hip, bd)
    ps_t = hip.mb_predict_mv_pskip(mv0_t, ref0_t, mbw, mbh, nf)
    skip_t = hip.mb_probe_skip(fenc_t, mbw, mbh, nf, qp_t, q4, chroma_format=cf, fenc_chroma=fenc_ct,
                               ref=(luma, ref.origin, ref.stride), ref_chroma=(nv, ref.corigin, ref.cs), pskip_mv=ps_t,
                               qp_table=base.qp_table)
    # the caller's choice of what to send as a skip, in tensor operations on the device
    mvmb_t = mv0_t[:, ::4, ::4].reshape(n, 2)
    intra_t = torch.from_numpy(intra).cuda()
    send_t = (skip_t != 0) & ~intra_t & (mvmb_t == ps_t).all(dim=1)
    flags_t = torch.from_numpy(flags).cuda() | (send_t.to(torch.uint8) * mbc.SKIP)
    par_t = torch.from_numpy(par).cuda()
    p, pc = hip.mb_mc(luma, None, ref.origin, ref.stride, 0, torch.from_numpy(pos).cuda(), par_t, None,
                      chroma=(cf, nv, None, ref.corigin, ref.cs))
    ptup, ctup = (p, ref.origin, ref.stride, p[0].numel()), (pc[0], ref.corigin, ref.cs, pc[0][0].numel())
    out = hip.mb_encode_inter(fenc_t, ptup, mbw, mbh, nf, qp_t, flags_t, q4, dq4, quant8=q8, dequant8_mf=dq8,
                              chroma_format=cf, fenc_chroma=fenc_ct, pred_chroma=ctup, b_dct_decimate=1,
                              qp_table=base.qp_table)
    final_t = hip.mb_skip_convert(flags_t, out["cbp"], mbw, mbh, nf, mv0=mv0_t, ref0=ref0_t, pskip_mv=ps_t)
    bs_t = hip.deblock_strength(out["nz"], out["flags_out"], mv0_t, ref0_t, mbw, mbh, nf)
    hip.deblock_frames(p, ref.origin, ref.stride, mbw, mbh, qp_t, out["flags_out"], bs_t,
                       chroma=(cf, [pc[0]], ref.corigin, ref.cs), qp_table=base.qp_table)
    torch.cuda.synchronize()
    assert np.array_equal(ps_t.cpu().numpy(), e.want_ps) and np.array_equal(skip_t.cpu().numpy(), e.want_skip)
    assert np.array_equal(flags_t.cpu().numpy(), e.flags_in) and np.array_equal(out["cbp"].cpu().numpy(), e.enc.cbp)
    assert np.array_equal(final_t.cpu().numpy(), e.want_flags)
    assert np.array_equal(bs_t.cpu().numpy().reshape(e.bs.shape), e.bs)
    got_y = np_pix(p, bd)[:, ref.oy:ref.oy + H, ref.ox:ref.ox + W]
    got_c = np_pix(pc[0], bd)[:, ref.coy:ref.coy + H // 2, ref.cox:ref.cox + W]
    assert np.array_equal(got_y, e.want_y.astype(got_y.dtype)) and np.array_equal(got_c, e.want_c[0].astype(got_c.dtype))
