"""Time the intra mode decision (x264hip_*_mb_analyse_intra) on 1080p 4:2:0 frames (120 x 68 MBs),
n_frames 1 and 16, 8 and 10 bit: an I picture with every macroblock tried (I_4x4 and I_8x8 on,
i_subpel_refine 5).  In the same run and on the same content, alternating, it times
mb_encode_intra fed the flags and modes that analysis decided -- the encode the analysis kernel
ends with, so the difference is what the decision costs -- and deblock_frames, the launch floor of
this execution shape (the same 254 dependent launches).  `ratio` = analyse leg / each of the two.
Recorded, not judged.

Content and method are tools/mbintra_time.py's: a ramp with texture as fenc, qp 20..40 +
QP_BD_OFFSET, recon encoded in place call after call; each leg captured into a graph of CALLS
calls, warmed up, then ROUNDS interleaved rounds of one replay between two device events:
`graph_ms` is the median ms per call (min, max beside it).  Writes one JSON line (and --out FILE).

usage: python tools/mbanalyse_time.py [--rounds 7] [--calls 2] [--out profiles/mbanalyse_time.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import load_package  # noqa: E402
from mbintra_time import FLAT, H, LAUNCHES, MBH, MBW, W, WARMUP_REPLAYS, picture  # noqa: E402

LAMBDA_TAB = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14,
              16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91, 102, 114, 128, 144, 161, 181, 203, 228, 256,
              287, 323, 362)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    x = load_package()
    x.init(0)
    rng = np.random.default_rng(1)
    legs, info = {}, {}
    for bd in (8, 10):
        vt = np.int16 if bd == 8 else np.int32
        cdt = torch.int16 if bd == 8 else torch.int32
        q = [torch.from_numpy(t.view(vt)).cuda() for t in x.cqm_init(bd, FLAT)]
        dq4, dq8 = (torch.from_numpy(t).cuda() for t in x.cqm_dequant(FLAT))
        table = x.chroma_qp_table(bd)
        lam = np.array(LAMBDA_TAB[:52 + 6 * (bd - 8)], np.uint16)
        for nf in (1, 16):
            n = nf * MBW * MBH
            fy, fc = picture(rng, nf, W, H, bd), picture(rng, nf, W, H // 2, bd)
            qp = torch.from_numpy((rng.integers(20, 41, n) + 6 * (bd - 8)).astype(np.int8)).cuda()
            common = dict(quant8=(q[2], q[3]), dequant8_mf=dq8, chroma_format=1, fenc_chroma=(fc, 0, W, W * H // 2),
                          b_dct_decimate=1, qp_table=table)

            def outs():
                return {"level": torch.zeros((n, 48, 16), dtype=cdt, device="cuda"),
                        "chroma_dc": torch.zeros((n, 2, 8), dtype=cdt, device="cuda"),
                        "luma_dc": torch.zeros((n, 16), dtype=cdt, device="cuda"),
                        "nnz": torch.zeros((n, 48), dtype=torch.uint8, device="cuda"),
                        "cbp": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "nz": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "flags_out": torch.zeros(n, dtype=torch.uint8, device="cuda")}
            flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
            tr = torch.ones(n, dtype=torch.uint8, device="cuda")
            pm, cm = torch.zeros((n, 16), dtype=torch.int8, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda")
            ry, rc = fy.clone(), fc.clone()
            o1 = dict(outs(), mb_flags_out=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      cost=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))
            analyse = (lambda fy=fy, ry=ry, rc=rc, nf=nf, qp=qp, flags=flags, tr=tr, pm=pm, cm=cm, q=q, dq4=dq4, o1=o1,
                       common=common, lam=lam: x.mb_analyse_intra(
                (fy, 0, W, W * H), (ry, 0, W, W * H), MBW, MBH, nf, qp, flags, tr, pm, lam, (q[0], q[1]), dq4,
                recon_chroma=(rc, 0, W, W * H // 2), chroma_pred_mode=cm, slice_type=0, i_subpel_refine=5, outs=dict(o1),
                **common))
            analyse()                                       # the decided flags and modes for the encode leg
            torch.cuda.synchronize()
            dflags_i, pm2, cm2 = o1["mb_flags_out"].clone(), pm.clone(), cm.clone()
            kinds = dflags_i.cpu().numpy()
            name = "mb_analyse_intra_%dbit_n%d" % (bd, nf)
            legs[name] = analyse
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": LAUNCHES,
                          "decided": {"i4x4": round(float((kinds == 1).mean()), 4), "i8x8": round(float((kinds == 3).mean()), 4),
                                      "i16x16": round(float((kinds == 17).mean()), 4)}}
            ry2, rc2, o2 = fy.clone(), fc.clone(), outs()
            name = "mb_encode_intra_decided_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda fy=fy, ry2=ry2, rc2=rc2, nf=nf, qp=qp, dflags_i=dflags_i, pm2=pm2, cm2=cm2, q=q, dq4=dq4,
                          o2=o2, common=common: x.mb_encode_intra(
                (fy, 0, W, W * H), (ry2, 0, W, W * H), MBW, MBH, nf, qp, dflags_i, pm2, (q[0], q[1]), dq4,
                recon_chroma=(rc2, 0, W, W * H // 2), chroma_pred_mode=cm2, outs=o2, **common))
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": LAUNCHES}
            # the launch floor: deblock_frames on the same shape (tools/deblock_time.py's inputs)
            luma, nv = fy.clone(), fc.clone()
            r3 = rng.random((3, n))
            dflags_h = ((r3[0] < 0.2) * 1 + (r3[1] < 0.3) * 2 + (r3[2] < 0.15) * 4).astype(np.uint8)
            bs_h = rng.integers(0, 3, (n, 2, 4, 4)).astype(np.uint8)
            bs_h[(dflags_h & 1) != 0, :, 1:] = 3
            dflags, bs = torch.from_numpy(dflags_h).cuda(), torch.from_numpy(bs_h).cuda()
            name = "deblock_frames_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda luma=luma, nv=nv, qp=qp, dflags=dflags, bs=bs, nf=nf, table=table: x.deblock_frames(
                luma, 0, W, MBW, MBH, qp, dflags, bs, chroma=(1, [nv], 0, W), qp_table=table, nframes=nf))
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": LAUNCHES}

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

    graph_ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k in legs:
            graph_ms[k].append(timed(runs[k].replay))
    result = {"width": W, "height": H, "chroma_format": "4:2:0", "rounds": a.rounds, "calls": a.calls,
              "device": torch.cuda.get_device_name(0), "launches_per_call": LAUNCHES, "legs": {}, "ratio": {}}
    for k in legs:
        g = graph_ms[k]
        med = statistics.median(g)
        result["legs"][k] = {**info[k],
                             "graph_ms": {"median": round(med, 4), "min": round(min(g), 4), "max": round(max(g), 4)},
                             "ms_per_frame": round(med / info[k]["n_frames"], 4),
                             "us_per_launch": round(med * 1e3 / LAUNCHES, 3)}
    for k in legs:
        if k.startswith("mb_analyse_intra"):
            bd_nf = "_".join(k.rsplit("_", 2)[-2:])                  # "<depth>bit_n<frames>"
            med = result["legs"][k]["graph_ms"]["median"]
            for other, tag in (("mb_encode_intra_decided_", "_over_encode"), ("deblock_frames_", "_over_deblock")):
                result["ratio"][k + tag] = round(med / result["legs"][other + bd_nf]["graph_ms"]["median"], 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
