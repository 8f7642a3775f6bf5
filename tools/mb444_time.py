"""Time the 4:4:4 macroblock encodes (x264hip_*_mb_encode_inter_444 / _intra_444) on 1080p frames
(120 x 68 MBs), n_frames 1 and 16, 8 and 10 bit: the inter entry on a P-like picture (no intra
macroblock, half transform 8), the intra entry on all I_16x16, all I_4x4 and all I_8x8.  In the
same run, alternating, it times the existing 4:2:0 entries on the same luma, the same qp, flags and
modes -- the yardstick: `ratio` = 4:4:4 leg / 4:2:0 leg -- and, for the intra legs, deblock_frames
on the same shape (the same 254 dependent launches: the launch floor).  4:4:4 codes 768 samples a
macroblock, 4:2:0 384.  Recorded, not judged.

Content: a ramp with texture per plane as fenc; inter: pred = fenc + noise of about one quantiser
step; qp 20..40 + QP_BD_OFFSET; intra modes as tools/mbintra_time.py draws them.  recon is encoded in
place for the intra legs and apart for the inter legs, so every call does the same work.

Method (tools/mbenc_time.py's): each leg is captured into a graph of CALLS calls, warmed up, then
ROUNDS interleaved rounds of one replay between two device events: `graph_ms` is the median ms per
call (min, max beside it).  Writes one JSON line (and --out FILE).

usage: python tools/mb444_time.py [--rounds 7] [--calls 2] [--out profiles/mb444_time.json]"""
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
from mbintra_time import modes, picture  # noqa: E402

W, H = 1920, 1088
MBW, MBH = W // 16, H // 16
LAUNCHES = MBW + 2 * (MBH - 1)
WARMUP_REPLAYS = 2
FLAT = [[16] * 16] * 4 + [[16] * 64] * 4
INTRA, T8, D16, I16 = 1, 2, 4, 16


def noisy(rng, t, qp_h, nf, h, bd):
    """t + noise of about a quantiser step of each macroblock's qp (4:2:0 chroma: h = H / 2)"""
    step = 0.625 * 2.0 ** ((qp_h.astype(np.float64) - 6 * (bd - 8)) / 6.0) * (1 << (bd - 8))
    s = np.repeat(np.repeat(step.reshape(nf, MBH, MBW), h // MBH, 1), 16, 2)
    a = t.cpu().numpy().astype(np.int64) & ((1 << 16) - 1)
    a = np.clip(np.rint(a + rng.normal(0, 1, a.shape) * s), 0, (1 << bd) - 1)
    return torch.from_numpy(a.astype(np.uint8 if bd == 8 else np.int16)).cuda()


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
        q = [torch.from_numpy(t.view(vt)).cuda() for t in x.cqm_init444(bd, FLAT)]
        dq4, dq8 = (torch.from_numpy(t).cuda() for t in x.cqm_dequant444(FLAT))
        table = x.chroma_qp_table(bd)
        for nf in (1, 16):
            n = nf * MBW * MBH
            fy, fu, fv = (picture(rng, nf, W, H, bd) for _ in range(3))
            fc = picture(rng, nf, W, H // 2, bd)                # the NV12 plane of the 4:2:0 legs
            qp_h = (rng.integers(20, 41, n) + 6 * (bd - 8)).astype(np.int8)
            qp = torch.from_numpy(qp_h).cuda()
            L, C = W * H, W * H // 2

            def outs444():
                return {"level": torch.zeros((n, 48, 16), dtype=cdt, device="cuda"),
                        "luma_dc": torch.zeros((n, 3, 16), dtype=cdt, device="cuda"),
                        "nnz": torch.zeros((n, 48), dtype=torch.uint8, device="cuda"),
                        "cbp": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "nz": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "flags_out": torch.zeros(n, dtype=torch.uint8, device="cuda")}

            def outs420():
                o = outs444()
                o["luma_dc"] = torch.zeros((n, 16), dtype=cdt, device="cuda")
                o["chroma_dc"] = torch.zeros((n, 2, 8), dtype=cdt, device="cuda")
                return o
            t444 = dict(quant8=(q[2], q[3]), dequant8_mf=dq8, b_dct_decimate=1, qp_table=table)
            t420 = dict(quant8=(q[2], q[3]), dequant8_mf=dq8[:2].contiguous(), chroma_format=1, fenc_chroma=(fc, 0, W, C),
                        b_dct_decimate=1, qp_table=table)
            fenc444 = ((fy, 0, W, L), ([fu, fv], 0, W, L))
            tag = "%dbit_n%d" % (bd, nf)
            meta = {"n_frames": nf, "bit_depth": bd}

            # ---- inter: a P-like picture, recon apart
            r = rng.random((2, n))
            flags = torch.from_numpy((np.where(r[0] < 0.5, T8, 0) + np.where(r[1] < 0.5, D16, 0)).astype(np.uint8)).cuda()
            py, pu, pv = (noisy(rng, t, qp_h, nf, H, bd) for t in (fy, fu, fv))
            pc = noisy(rng, fc, qp_h, nf, H // 2, bd)
            pred444 = ((py, 0, W, L), ([pu, pv], 0, W, L))
            rec444 = ((torch.zeros_like(py), 0, W, L), ([torch.zeros_like(pu), torch.zeros_like(pv)], 0, W, L))
            o4, o2 = outs444(), outs420()
            legs["inter_444_" + tag] = (lambda fenc444=fenc444, pred444=pred444, rec444=rec444, nf=nf, qp=qp, flags=flags, q=q,
                                        dq4=dq4, o4=o4, t444=t444: x.mb_encode_inter_444(
                fenc444, pred444, MBW, MBH, nf, qp, flags, (q[0], q[1]), dq4, recon=rec444, outs=o4, **t444))
            ry, rc = torch.zeros_like(py), torch.zeros_like(pc)
            legs["inter_420_" + tag] = (lambda fy=fy, py=py, pc=pc, ry=ry, rc=rc, nf=nf, qp=qp, flags=flags, q=q, dq4=dq4, o2=o2,
                                        t420=t420: x.mb_encode_inter(
                (fy, 0, W, L), (py, 0, W, L), MBW, MBH, nf, qp, flags, (q[0], q[1]), dq4, pred_chroma=(pc, 0, W, C),
                recon=(ry, 0, W, L), recon_chroma=(rc, 0, W, C), outs={k: v for k, v in o2.items() if k != "luma_dc"}, **t420))
            info["inter_444_" + tag] = {**meta, "launches": 1}
            info["inter_420_" + tag] = {**meta, "launches": 1}

            # ---- intra: the three kinds, recon in place
            for leg, kind in (("i16x16", 2), ("i4x4", 0), ("i8x8", 1)):
                kinds = np.full(n, kind)
                flags = torch.from_numpy(np.full(n, INTRA + (0, T8, I16)[kind], np.uint8)).cuda()
                pm, cm = modes(rng, nf, kinds)
                rec444 = ((fy.clone(), 0, W, L), ([fu.clone(), fv.clone()], 0, W, L))
                o4, o2 = outs444(), outs420()
                name = "intra_444_%s_%s" % (leg, tag)
                legs[name] = (lambda fenc444=fenc444, rec444=rec444, nf=nf, qp=qp, flags=flags, pm=pm, q=q, dq4=dq4, o4=o4,
                              t444=t444: x.mb_encode_intra_444(fenc444, rec444, MBW, MBH, nf, qp, flags, pm, (q[0], q[1]), dq4,
                                                               outs=o4, **t444))
                info[name] = {**meta, "launches": LAUNCHES}
                ry, rc = fy.clone(), fc.clone()
                name = "intra_420_%s_%s" % (leg, tag)
                legs[name] = (lambda fy=fy, ry=ry, rc=rc, nf=nf, qp=qp, flags=flags, pm=pm, cm=cm, q=q, dq4=dq4, o2=o2,
                              t420=t420: x.mb_encode_intra((fy, 0, W, L), (ry, 0, W, L), MBW, MBH, nf, qp, flags, pm, (q[0], q[1]),
                                                           dq4, recon_chroma=(rc, 0, W, C), chroma_pred_mode=cm, outs=o2, **t420))
                info[name] = {**meta, "launches": LAUNCHES}
            # the launch floor: deblock_frames on the same shape (tools/deblock_time.py's inputs)
            luma, nv = fy.clone(), fc.clone()
            r3 = rng.random((3, n))
            dflags_h = ((r3[0] < 0.2) * 1 + (r3[1] < 0.3) * 2 + (r3[2] < 0.15) * 4).astype(np.uint8)
            bs_h = rng.integers(0, 3, (n, 2, 4, 4)).astype(np.uint8)
            bs_h[(dflags_h & 1) != 0, :, 1:] = 3
            dflags, bs = torch.from_numpy(dflags_h).cuda(), torch.from_numpy(bs_h).cuda()
            legs["deblock_frames_" + tag] = (lambda luma=luma, nv=nv, qp=qp, dflags=dflags, bs=bs, nf=nf, table=table:
                                             x.deblock_frames(luma, 0, W, MBW, MBH, qp, dflags, bs, chroma=(1, [nv], 0, W),
                                                              qp_table=table, nframes=nf))
            info["deblock_frames_" + tag] = {**meta, "launches": LAUNCHES}

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
    result = {"width": W, "height": H, "rounds": a.rounds, "calls": a.calls, "device": torch.cuda.get_device_name(0),
              "launches_per_intra_call": LAUNCHES, "legs": {}, "ratio": {}}
    for k in legs:
        g = graph_ms[k]
        med = statistics.median(g)
        result["legs"][k] = {**info[k],
                             "graph_ms": {"median": round(med, 4), "min": round(min(g), 4), "max": round(max(g), 4)},
                             "ms_per_frame": round(med / info[k]["n_frames"], 4),
                             "us_per_launch": round(med * 1e3 / info[k]["launches"], 3)}
    med = lambda k: result["legs"][k]["graph_ms"]["median"]
    for k in legs:
        if "_444_" in k:
            result["ratio"][k + "_over_420"] = round(med(k) / med(k.replace("_444_", "_420_")), 3)
        if k.startswith("intra_"):
            result["ratio"][k + "_over_deblock"] = round(med(k) / med("deblock_frames_" + "_".join(k.rsplit("_", 2)[-2:])), 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
