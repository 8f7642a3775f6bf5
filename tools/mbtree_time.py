"""Time the MB-tree entries (x264hip_mbtree_propagate with 1 and 3 steps, x264hip_mbtree_finish)
at 1080p (120x68 MBs) and 2160p (240x135 MBs) against what a caller pays today to run MB-tree on
the host: the device-to-host copies of i_intra_cost, lowres_costs and the two mv planes of the
same frames into pinned memory.

Method: every leg warmed up (WARMUP_CALLS calls), then ROUNDS interleaved rounds; in a round each
leg is timed twice:
  * "stream_us": CALLS calls enqueued back to back between two device events (the cost on a
    stream that is kept busy, launch gaps included);
  * "sync_us":   the host clock around one call and a stream synchronise (the latency a caller
    sees who waits for the result), median of SYNC_CALLS.
Reported: the median over the rounds and the spread (min, max).  Prints one JSON line.

usage: python tools/mbtree_time.py [--rounds 7] [--calls 200]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SYNC_CALLS = 30
WARMUP_CALLS = 500


def inputs(x, w, h, nsteps, seed):
    """nsteps B-frame steps sharing two destination planes, lookahead-like values"""
    n = w * h
    g = torch.Generator(device="cpu").manual_seed(seed)

    def u16(lo, hi, *shape):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.int16).cuda()
    dst = [u16(0, 4000, n), u16(0, 4000, n)]
    frames = []
    for _ in range(nsteps):
        intra = u16(200, 9000, n)
        costs = (torch.randint(1, 4, (n,), generator=g, dtype=torch.int32) * 16384
                 + torch.randint(0, 6000, (n,), generator=g, dtype=torch.int32)).to(torch.int16).cuda()
        mvs = [torch.randint(-96, 97, (n, 2), generator=g, dtype=torch.int32).to(torch.int16).cuda() for _ in range(2)]
        frames.append(dict(intra=intra, costs=costs, mvs=mvs, invq=u16(100, 700, n)))
    steps = [x.mbtree_step(f["intra"], f["costs"], f["mvs"][0], dst[0], 0.00195, f["mvs"][1], dst[1], f["invq"],
                           None, 43) for f in frames]
    return dst, frames, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    x = load_package()
    x.init(0)
    result = {"rounds": a.rounds, "calls": a.calls, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name, (w, h) in (("1080p", (120, 68)), ("2160p", (240, 135))):
        n = w * h
        dst, frames, steps3 = inputs(x, w, h, 3, n)
        aq = torch.zeros(n, dtype=torch.float32, device="cuda")
        qp = torch.empty_like(aq)
        pinned = [{k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in
                   (("intra", f["intra"]), ("costs", f["costs"]), ("mv0", f["mvs"][0]), ("mv1", f["mvs"][1]))}
                  for f in frames]

        def copies(k):
            for f, p in zip(frames[:k], pinned[:k]):
                p["intra"].copy_(f["intra"], non_blocking=True)
                p["costs"].copy_(f["costs"], non_blocking=True)
                p["mv0"].copy_(f["mvs"][0], non_blocking=True)
                p["mv1"].copy_(f["mvs"][1], non_blocking=True)

        legs = {
            "propagate_1": lambda: x.mbtree_propagate(steps3[:1], w, h),
            "propagate_3": lambda: x.mbtree_propagate(steps3, w, h),
            "finish": lambda: x.mbtree_finish(frames[0]["intra"], dst[0], aq, 512, 0.0, 2.0, frames[0]["invq"], qp),
            "copies_1": lambda: copies(1),
            "copies_3": lambda: copies(3),
        }
        for fn in legs.values():
            for _ in range(WARMUP_CALLS):
                fn()
        torch.cuda.synchronize()
        samples = {k: {"stream_us": [], "sync_us": []} for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                samples[k]["stream_us"].append(e0.elapsed_time(e1) * 1000 / a.calls)
                lat = []
                for _ in range(SYNC_CALLS):
                    t = time.perf_counter()
                    fn()
                    torch.cuda.current_stream().synchronize()
                    lat.append((time.perf_counter() - t) * 1e6)
                samples[k]["sync_us"].append(statistics.median(lat))
        out = {}
        for k, s in samples.items():
            out[k] = {m: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                      for m, v in s.items()}
        for k, c in (("propagate_1", "copies_1"), ("propagate_3", "copies_3")):
            out[k]["ratio_to_copies"] = {m: round(out[k][m]["median"] / out[c][m]["median"], 3)
                                         for m in ("stream_us", "sync_us")}
        out["copy_bytes_per_frame"] = int(sum(np.prod(p.shape) * p.element_size() for p in pinned[0].values()))
        result["sizes"][name] = out
    print(json.dumps(result))


if __name__ == "__main__":
    main()
