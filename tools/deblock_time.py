"""Time the deblocking filter (x264hip_*_deblock_frames) and x264hip_deblock_strength on 1080p
4:2:0 frames (120 x 68 MBs: 254 dependent launches a call), n_frames 1 and 16, 8 and 10 bit.

Content: a ramp with a random offset per 4x4 block and +-1 of noise (blocking the filter acts
on); per MB a random qp in 30..51, 20 % intra, 30 % transform 8x8, 15 % with flag bit 2; bs random
in {0, 1, 2}, 3 inside intra MBs.  The filter works in place, so every call after the first filters
an already filtered picture: the launches, the loads and the stores are the same, fewer lines
pass the filters' thresholds.

Method: each leg is captured into a graph of CALLS calls, warmed up, then ROUNDS interleaved
rounds of one replay between two device events: `graph_ms` is the median ms per call (min, max
beside it).  `stream_ms` is the same number of calls enqueued on the stream without a graph,
between two events: what a caller that does not capture pays, the host's launch cost included
where it is the slower side.  ms_per_frame = graph_ms / n_frames.  Writes one JSON line (and
--out FILE).

usage: python tools/deblock_time.py [--rounds 7] [--calls 3] [--out profiles/deblock_time.json]"""
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


def picture(rng, nf, w, h, bd):
    y, x = np.mgrid[0:h, 0:w]
    ramp = 48 + abs(((x + y) >> 2) % 320 - 160)
    off = rng.integers(-5, 6, (nf, h // 4, w // 4))
    pic = ramp + np.repeat(np.repeat(off, 4, 1), 4, 2) + rng.integers(-1, 2, (nf, h, w))
    return (np.clip(pic, 0, 255) << (bd - 8)).astype(np.uint8 if bd == 8 else np.int16)


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
        for nf in (1, 16):
            n = nf * MBW * MBH
            luma = torch.from_numpy(picture(rng, nf, W, H, bd)).cuda()
            nv = torch.from_numpy(picture(rng, nf, W, H // 2, bd)).cuda()
            qp = torch.from_numpy(rng.integers(30, 52, n).astype(np.int8)).cuda()
            r = rng.random((3, n))
            flags_h = ((r[0] < 0.2) * 1 + (r[1] < 0.3) * 2 + (r[2] < 0.15) * 4).astype(np.uint8)
            bs_h = rng.integers(0, 3, (n, 2, 4, 4)).astype(np.uint8)
            bs_h[(flags_h & 1) != 0, :, 1:] = 3
            flags, bs = torch.from_numpy(flags_h).cuda(), torch.from_numpy(bs_h).cuda()
            table = x.chroma_qp_table(bd)
            name = "deblock_frames_%dbit_n%d" % (bd, nf)
            legs[name] = (lambda luma=luma, nv=nv, qp=qp, flags=flags, bs=bs, table=table, nf=nf: x.deblock_frames(
                luma, 0, W, MBW, MBH, qp, flags, bs, chroma=(1, [nv], 0, W), qp_table=table, nframes=nf))
            px = 1 if bd == 8 else 2
            info[name] = {"n_frames": nf, "bit_depth": bd, "launches": MBW + 2 * (MBH - 1),
                          "bytes_picture": nf * W * H * 3 // 2 * px}
    for nf in (1, 16):
        n = nf * MBW * MBH
        nz = torch.from_numpy((rng.integers(0, 1 << 16, n) & rng.integers(0, 1 << 16, n)).astype(np.int32)).cuda()
        flags = torch.from_numpy(((rng.random(n) < 0.2) * 1 + (rng.random(n) < 0.3) * 2).astype(np.uint8)).cuda()
        mv = torch.from_numpy(rng.integers(-6, 7, (nf, 4 * MBH, 4 * MBW, 2)).astype(np.int16)).cuda()
        ref = torch.from_numpy((rng.random((nf, 2 * MBH, 2 * MBW)) < 0.15).astype(np.int8)).cuda()
        out = torch.empty((n, 2, 4, 4), dtype=torch.uint8, device="cuda")
        name = "deblock_strength_n%d" % nf
        legs[name] = (lambda nz=nz, flags=flags, mv=mv, ref=ref, out=out, nf=nf: x.deblock_strength(
            nz, flags, mv, ref, MBW, MBH, nf, bs=out))
        info[name] = {"n_frames": nf, "launches": 1}

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
              "device": torch.cuda.get_device_name(0), "legs": {}}
    for k in legs:
        g, s = graph_ms[k], stream_ms[k]
        med = statistics.median(g)
        result["legs"][k] = {**info[k],
                             "graph_ms": {"median": round(med, 4), "min": round(min(g), 4), "max": round(max(g), 4)},
                             "stream_ms": {"median": round(statistics.median(s), 4), "min": round(min(s), 4),
                                           "max": round(max(s), 4)},
                             "ms_per_frame": round(med / info[k]["n_frames"], 4),
                             "us_per_launch": round(1e3 * med / info[k]["launches"], 3)}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
