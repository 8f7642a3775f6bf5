"""Time the skip probe (x264hip_*_mb_probe_skip) on 1080p 4:2:0 frames (120 x 68 MBs), n_frames 1
and 16, 8 and 10 bit: the P leg unweighted and weighted in all three planes, and the B leg.  In the
same run, alternating, on the same planes and vectors: what a caller had to run before to learn
the same thing -- mb_mc (16x16, list 0, the skip vectors) + mb_encode_inter, then a read-back of
cbp.  The two do different work (the encode reconstructs and writes every coefficient; its
thresholds are not the probe's), so their ratio is recorded, not judged.  The small entries
mb_predict_mv_pskip and mb_skip_convert are timed beside them.

Content: a ramp with texture as the reference (H, V, C are shifted copies: only the phase of a
vector picks them); half the skip vectors zero, the rest up to +-16 pixels; fenc = the prediction
at the skip vector (made by mb_mc on the device) + for half the macroblocks noise of about one
quantiser step of the macroblock's qp (20..40 + QP_BD_OFFSET), so skips and failures share waves.
`skip_share` is the share of macroblocks that probed as skip.

bytes: what one probe must move -- fenc and the prediction's source read once (luma + chroma), qp
and the skip vector read, skip written -- and `hbm_share` = bytes / graph time / 8 TB/s.

Method (tools/mbenc_time.py's): each leg is captured into a graph of CALLS calls, warmed up, then
ROUNDS interleaved rounds of one replay between two device events: `graph_ms` is the median ms per
call (min, max beside it); `stream_ms` the same number of calls enqueued without a graph.  Writes
one JSON line (and --out FILE).

usage: python tools/mbskip_time.py [--rounds 7] [--calls 3] [--out profiles/mbskip_time.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

W, H = 1920, 1088
MBW, MBH = W // 16, H // 16
PAD = 32
WARMUP_REPLAYS = 3
HBM_PEAK = 8e12
FLAT = [[16] * 16] * 4 + [[16] * 64] * 4
WEIGHTS = ((57, 6, 9), (70, 6, -11), (61, 6, 5))


def picture(rng, nf, w, h, bd):
    y, x = np.mgrid[0:h, 0:w]
    ramp = 48 + abs(((x + y) >> 2) % 320 - 160) + 20 * np.sin(x / 9.0) * np.cos(y / 7.0)
    return np.clip(np.rint(ramp[None] + rng.normal(0, 3, (nf, h, w))), 0, 255) * (1 << (bd - 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    x = load_package()
    x.init(0)
    rng = np.random.default_rng(1)
    legs, info, shares = {}, {}, {}
    stride = x.plane_stride(W)
    origin = PAD * stride + PAD
    for bd in (8, 10):
        pdt = np.uint8 if bd == 8 else np.int16
        tdt = torch.uint8 if bd == 8 else torch.int16
        px, co = (1, 2) if bd == 8 else (2, 4)
        pm = (1 << bd) - 1
        q = x.cqm_init(bd, FLAT)
        vt = np.int16 if bd == 8 else np.int32
        q = [torch.from_numpy(t.view(vt)).cuda() for t in q]
        dq4, dq8 = (torch.from_numpy(t).cuda() for t in x.cqm_dequant(FLAT))
        table = x.chroma_qp_table(bd)
        for nf in (1, 16):
            n = nf * MBW * MBH
            rows, crows = H + 2 * PAD, H // 2 + 2 * PAD
            fstride, cfstride = rows * stride, crows * stride
            F = torch.from_numpy(picture(rng, nf, stride, rows, bd).astype(np.int64).astype(pdt)).cuda()
            luma = [F, torch.roll(F, 1, 2), torch.roll(F, 1, 1), torch.roll(F, (1, 1), (1, 2))]
            nv = torch.from_numpy(picture(rng, nf, stride, crows, bd).astype(np.int64).astype(pdt)).cuda()
            qp_h = (rng.integers(20, 41, n) + 6 * (bd - 8)).astype(np.int8)
            step = 0.625 * 2.0 ** ((qp_h.astype(np.float64) - 6 * (bd - 8)) / 6.0) * (1 << (bd - 8))
            noisy = rng.random(n) < 0.5
            amp = torch.from_numpy(np.repeat(np.repeat((step * noisy).reshape(nf, MBH, MBW), 16, 1), 16, 2)).cuda()
            mv_h = np.where(rng.random((n, 1)) < 0.5, 0, rng.integers(-64, 65, (n, 2))).astype(np.int16)
            f, my, mx = np.meshgrid(np.arange(nf), np.arange(MBH), np.arange(MBW), indexing="ij")
            pos_h = np.stack([f, 16 * mx, 16 * my], -1).reshape(n, 3).astype(np.int32)
            lim = np.stack([4 * (-16 * mx - 24), 4 * (-16 * my - 24), 4 * (16 * (MBW - mx - 1) + 24),
                            4 * (16 * (MBH - my - 1) + 24)], -1).reshape(n, 4)
            par_h = np.concatenate([mv_h, mv_h, lim], 1).astype(np.int16)
            pos, par, mv = (torch.from_numpy(t).cuda() for t in (pos_h, par_h, mv_h))
            qp = torch.from_numpy(qp_h).cuda()
            flags = torch.full((n,), x.MBENC_D16x16, dtype=torch.uint8, device="cuda")
            chroma = (1, [nv], None, origin, stride)

            def noised(p, rows_, amp_):
                """the picture area of a padded plane + the macroblocks' noise"""
                inner = p[:, PAD:PAD + rows_, PAD:PAD + W].to(torch.float64)
                g = torch.from_numpy(rng.normal(0, 1, tuple(inner.shape))).cuda()
                out = p.clone()
                out[:, PAD:PAD + rows_, PAD:PAD + W] = torch.clamp(torch.round(inner + g * amp_), 0, pm).to(tdt)
                return out
            preds = {}
            for w_name, wt in (("", (None,) * 3), ("_weighted", WEIGHTS)):
                pred, pred_c = x.mb_mc(luma, None, origin, stride, 0, pos, par, None, chroma=chroma, weight=wt)
                torch.cuda.synchronize()
                fy, fc = noised(pred, H, amp), noised(pred_c[0], H // 2, 0.5 * amp[:, ::2])
                preds[w_name] = (pred, pred_c, fy, fc)
                skip = torch.zeros(n, dtype=torch.uint8, device="cuda")
                name = "probe_p%s_%dbit_n%d" % (w_name, bd, nf)
                legs[name] = (lambda fy=fy, fc=fc, nf=nf, qp=qp, q=q, mv=mv, wt=wt, skip=skip, luma=luma, nv=nv, table=table:
                              x.mb_probe_skip((fy, origin, stride, fstride), MBW, MBH, nf, qp, (q[0], q[1]), chroma_format=1,
                                              fenc_chroma=(fc, origin, stride, cfstride), ref=(luma, origin, stride),
                                              ref_chroma=([nv], origin, stride), pskip_mv=mv, weight=wt, qp_table=table,
                                              skip=skip))
                pixels = nf * W * H * 3 // 2
                info[name] = {"n_frames": nf, "bit_depth": bd, "launches": 1, "bytes": 2 * pixels * px + n * (1 + 1 + 4)}
                shares[name] = skip
            pred, pred_c, fy, fc = preds[""]
            skip_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
            name = "probe_b_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda fy=fy, fc=fc, nf=nf, qp=qp, q=q, skip=skip_b, p=pred.clone(), pc=pred_c[0].clone(),
                          table=table:
                          x.mb_probe_skip((fy, origin, stride, fstride), MBW, MBH, nf, qp, (q[0], q[1]), chroma_format=1,
                                          fenc_chroma=(fc, origin, stride, cfstride), pred=(p, origin, stride, fstride),
                                          pred_chroma=(pc, origin, stride, cfstride), qp_table=table, skip=skip))
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": 1,
                          "bytes": 2 * nf * W * H * 3 // 2 * px + n * (1 + 1)}
            shares[name] = skip_b
            # what answered the question before: mb_mc at the skip vectors + mb_encode_inter, in place
            cdt = torch.int16 if bd == 8 else torch.int32
            outs = {"level": torch.zeros((n, 48, 16), dtype=cdt, device="cuda"),
                    "chroma_dc": torch.zeros((n, 2, 8), dtype=cdt, device="cuda"),
                    "nnz": torch.zeros((n, 48), dtype=torch.uint8, device="cuda"),
                    "cbp": torch.zeros(n, dtype=torch.int32, device="cuda"),
                    "nz": torch.zeros(n, dtype=torch.int32, device="cuda"),
                    "flags_out": torch.zeros(n, dtype=torch.uint8, device="cuda")}
            name = "mc_encode_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda fy=fy, fc=fc, nf=nf, qp=qp, q=q, pos=pos, par=par, luma=luma, chroma=chroma, p=pred,
                          pc=pred_c, flags=flags, outs=outs, dq4=dq4, dq8=dq8, table=table: (
                x.mb_mc(luma, None, origin, stride, 0, pos, par, None, chroma=chroma,
                        outs=(p, origin, stride, pc, origin, stride)),
                x.mb_encode_inter((fy, origin, stride, fstride), (p, origin, stride, fstride), MBW, MBH, nf, qp, flags,
                                  (q[0], q[1]), dq4, quant8=(q[2], q[3]), dequant8_mf=dq8, chroma_format=1,
                                  fenc_chroma=(fc, origin, stride, cfstride), pred_chroma=(pc[0], origin, stride, cfstride),
                                  b_dct_decimate=True, qp_table=table, outs=outs)))
            pixels = nf * W * H * 3 // 2
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": 2,
                          "bytes": 5 * pixels * px + n * (48 * 16 + 16) * co + n * (48 + 4 + 4 + 1 + 16 + 12)}
            if bd == 8:
                mv0 = torch.from_numpy(rng.integers(-40, 41, (nf, 4 * MBH, 4 * MBW, 2)).astype(np.int16)).cuda()
                ref0 = torch.from_numpy(rng.integers(-1, 2, (nf, 2 * MBH, 2 * MBW)).astype(np.int8)).cuda()
                ps = torch.zeros((n, 2), dtype=torch.int16, device="cuda")
                fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
                legs["predict_mv_pskip_n%d" % nf] = (lambda mv0=mv0, ref0=ref0, nf=nf, ps=ps:
                                                      x.mb_predict_mv_pskip(mv0, ref0, MBW, MBH, nf, pskip_mv=ps))
                info["predict_mv_pskip_n%d" % nf] = {"n_frames": nf, "launches": 1, "bytes": n * (3 * 4 + 3 + 4)}
                legs["skip_convert_n%d" % nf] = (lambda mv0=mv0, ref0=ref0, nf=nf, ps=ps, fl=fl, flags=flags, cbp=outs["cbp"]:
                                                  x.mb_skip_convert(flags, cbp, MBW, MBH, nf, mv0=mv0, ref0=ref0, pskip_mv=ps,
                                                                    flags=fl))
                info["skip_convert_n%d" % nf] = {"n_frames": nf, "launches": 1, "bytes": n * (1 + 4 + 4 + 1 + 4 + 1)}

    runs = {}
    side = torch.cuda.Stream()
    for k, fn in legs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # first launches before the capture
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.calls):
                fn()
        for _ in range(WARMUP_REPLAYS):
            g.replay()
        runs[k] = g
    torch.cuda.synchronize()

    def timed(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def plain(fn):
        for _ in range(a.calls):
            fn()
    graph_ms, stream_ms = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(a.rounds):
        for k in legs:
            graph_ms[k].append(timed(runs[k].replay))
        for k, fn in legs.items():
            stream_ms[k].append(timed(lambda fn=fn: plain(fn)))
    result = {"width": W, "height": H, "chroma_format": "4:2:0", "rounds": a.rounds, "calls": a.calls,
              "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "legs": {}, "ratio": {}}
    for k in legs:
        g, s = graph_ms[k], stream_ms[k]
        med = statistics.median(g)
        result["legs"][k] = {**info[k],
                             "graph_ms": {"median": round(med, 4), "min": round(min(g), 4), "max": round(max(g), 4)},
                             "stream_ms": {"median": round(statistics.median(s), 4), "min": round(min(s), 4),
                                           "max": round(max(s), 4)},
                             "ms_per_frame": round(med / info[k]["n_frames"], 4),
                             "hbm_share": round(info[k]["bytes"] / (med * 1e-3) / HBM_PEAK, 4)}
        if k in shares:
            result["legs"][k]["skip_share"] = round(float(shares[k].to(torch.float32).mean()), 3)
    for bd in (8, 10):
        for nf in (1, 16):
            chain = result["legs"]["mc_encode_%dbit_n%d" % (bd, nf)]["graph_ms"]["median"]
            for leg in ("p", "p_weighted", "b"):
                probe = result["legs"]["probe_%s_%dbit_n%d" % (leg, bd, nf)]["graph_ms"]["median"]
                result["ratio"]["probe_%s_over_mc_encode_%dbit_n%d" % (leg, bd, nf)] = round(probe / chain, 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
