"""Time the inter macroblock encode (x264hip_*_mb_encode_inter) on 1080p 4:2:0 frames (120 x 68
MBs), n_frames 1 and 16, 8 and 10 bit, and in the same run, alternating, on the same fenc and pred,
the luma-only two-launch chain it replaces in the frame loop (mb_dct_quant + mb_dequant_idct_add,
transform 4 and transform 8).  The two do different work -- the chain has no chroma, no
decimation, no zigzag, one transform size and one qp's quant row per call -- so their ratio is
recorded, not judged.

Content: a ramp with texture as fenc; pred = fenc plus noise of about one quantiser step of the
macroblock's qp (20..40 + QP_BD_OFFSET), so blocks are decimated, kept and empty side by side; half
the MBs transform 8x8, 10 % skip, 5 % intra.  recon is a plane of its own, so every call does the
same work.

bytes: what one call must move -- fenc and pred read, recon, level, chroma_dc, nnz, cbp, nz and
flags_out written, from the shapes -- and `hbm_share` = bytes / graph time / 8 TB/s.

Method (tools/deblock_time.py's): each leg is captured into a graph of CALLS calls, warmed up, then
ROUNDS interleaved rounds of one replay between two device events: `graph_ms` is the median ms per
call (min, max beside it); `stream_ms` the same number of calls enqueued without a graph.  Writes
one JSON line (and --out FILE).

usage: python tools/mbenc_time.py [--rounds 7] [--calls 3] [--out profiles/mbenc_time.json]"""
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
WARMUP_REPLAYS = 3
HBM_PEAK = 8e12
FLAT = [[16] * 16] * 4 + [[16] * 64] * 4


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
    legs, info = {}, {}
    for bd in (8, 10):
        pdt = np.uint8 if bd == 8 else np.int16
        px, co = (1, 2) if bd == 8 else (2, 4)
        pm = (1 << bd) - 1
        q = x.cqm_init(bd, FLAT)
        vt = np.int16 if bd == 8 else np.int32
        q = [torch.from_numpy(t.view(vt)).cuda() for t in q]
        dq4, dq8 = (torch.from_numpy(t).cuda() for t in x.cqm_dequant(FLAT))
        for nf in (1, 16):
            n = nf * MBW * MBH
            qp_h = (rng.integers(20, 41, n) + 6 * (bd - 8)).astype(np.int8)
            step = 0.625 * 2.0 ** ((qp_h.astype(np.float64) - 6 * (bd - 8)) / 6.0) * (1 << (bd - 8))
            amp = np.repeat(np.repeat(step.reshape(nf, MBH, MBW), 16, 1), 16, 2)
            fy, fc = picture(rng, nf, W, H, bd), picture(rng, nf, W, H // 2, bd)
            py = np.clip(np.rint(fy + rng.normal(0, 1, fy.shape) * amp), 0, pm)
            pc = np.clip(np.rint(fc + rng.normal(0, 0.5, fc.shape) * amp[:, ::2]), 0, pm)
            fy, fc, py, pc = (torch.from_numpy(t.astype(np.int64).astype(pdt)).cuda() for t in (fy, fc, py, pc))
            ry, rc = torch.zeros_like(py), torch.zeros_like(pc)
            r = rng.random((2, n))
            flags_h = ((r[0] < 0.5) * 2 + (r[1] < 0.05) * 1 + ((r[1] >= 0.05) & (r[1] < 0.15)) * 8 + 4).astype(np.uint8)
            qp, flags = torch.from_numpy(qp_h).cuda(), torch.from_numpy(flags_h).cuda()
            qp32 = qp.to(torch.int32)
            outs = {"level": torch.zeros((n, 48, 16), dtype=torch.int16 if bd == 8 else torch.int32, device="cuda"),
                    "chroma_dc": torch.zeros((n, 2, 8), dtype=torch.int16 if bd == 8 else torch.int32, device="cuda"),
                    "nnz": torch.zeros((n, 48), dtype=torch.uint8, device="cuda"),
                    "cbp": torch.zeros(n, dtype=torch.int32, device="cuda"),
                    "nz": torch.zeros(n, dtype=torch.int32, device="cuda"),
                    "flags_out": torch.zeros(n, dtype=torch.uint8, device="cuda")}
            table = x.chroma_qp_table(bd)
            name = "mb_encode_inter_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda fy=fy, fc=fc, py=py, pc=pc, ry=ry, rc=rc, qp=qp, flags=flags, outs=outs, table=table,
                          nf=nf, q=q, dq4=dq4, dq8=dq8: x.mb_encode_inter(
                (fy, 0, W, W * H), (py, 0, W, W * H), MBW, MBH, nf, qp, flags, (q[0], q[1]), dq4, quant8=(q[2], q[3]),
                dequant8_mf=dq8, chroma_format=1, fenc_chroma=(fc, 0, W, W * H // 2), pred_chroma=(pc, 0, W, W * H // 2),
                recon=(ry, 0, W, W * H), recon_chroma=(rc, 0, W, W * H // 2), b_dct_decimate=True, qp_table=table,
                outs=outs))
            pixels = nf * W * H * 3 // 2
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": 1,
                          "bytes": 3 * pixels * px + n * (48 * 16 + 16) * co + n * (48 + 4 + 4 + 1)}
            dct = torch.zeros((n, 256), dtype=torch.int16 if bd == 8 else torch.int32, device="cuda")
            nz = torch.zeros(n, dtype=torch.int32, device="cuda")
            qmid = 30 + 6 * (bd - 8)
            for t in (4, 8):
                mf, bias = (q[0], q[1]) if t == 4 else (q[2], q[3])
                dmf = dq4[1] if t == 4 else dq8[1]
                name = "luma_chain_t%d_%dbit_n%d" % (t, bd, nf)
                legs[name] = (lambda t=t, fy=fy, py=py, ry=ry, mf=mf[1, qmid].contiguous(), bias=bias[1, qmid].contiguous(),
                              dmf=dmf.contiguous(), dct=dct, nz=nz, qp32=qp32, nf=nf: (
                    x.mb_dct_quant(t, fy, 0, W, py, 0, W, MBW, MBH, nf, mf, bias, dct=dct, nz=nz),
                    x.mb_dequant_idct_add(t, dct, MBW, MBH, nf, dmf, qp32, py, 0, W, ry, 0, W)))
                info[name] = {"n_frames": nf, "bit_depth": bd, "launches": 2,
                              "bytes": 4 * nf * W * H * px + 2 * n * 256 * co + 2 * n * 4}

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
    for bd in (8, 10):
        for nf in (1, 16):
            fused = result["legs"]["mb_encode_inter_%dbit_n%d" % (bd, nf)]["graph_ms"]["median"]
            for t in (4, 8):
                chain = result["legs"]["luma_chain_t%d_%dbit_n%d" % (t, bd, nf)]["graph_ms"]["median"]
                result["ratio"]["fused_over_chain_t%d_%dbit_n%d" % (t, bd, nf)] = round(fused / chain, 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
