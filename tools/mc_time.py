"""Time batched motion compensation (x264hip_*_mb_mc) on 16 1080p 4:2:0 8-bit frames of
synth.make_subpel_sequence content (frame k predicted from frame k - 1, hpel planes from
x264hip's hpel_filter), in three cases:
  * p16x16:  every 16x16 block, list 0 (mode == NULL: the fast path);
  * p8x8:    every 8x8 block, list 0;
  * b16x16:  every 16x16 block bipred (list 0 = the previous frame, list 1 = the one before it),
against, in the same run, mb_dct_quant (4x4 transform) on the same frames -- the stage this
feeds -- and what a caller pays today instead: the device-to-host copy of the search's output
(int32 [n, 4] per block) plus the host-to-device upload of the luma and chroma prediction planes
from pinned memory (the host's own x264_mb_mc time is not counted).

Method: every kernel leg captured into a graph of CALLS calls (the copies: CALLS calls enqueued back
to back), warmed up, then ROUNDS interleaved rounds of one replay between two device events;
reported: the median ms per call and the spread (min, max).  bytes_* are the bytes the algorithm
needs (computed from the shapes and the phases of the vectors: one or two planes per list for
luma, one extra row and column for chroma); gb_per_s is their sum over the median time.  Writes
one JSON line (and --out FILE).

usage: python tools/mc_time.py [--rounds 9] [--calls 20] [--out profiles/mc_time.json]
       rocprofv3 --pmc COUNTERS... -d DIR -- python tools/mc_time.py --kernels-only 5     (counters:
       a run of its own, nothing timed)"""
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

W, H, NF = 1920, 1088, 16
WARMUP_REPLAYS = 5


def block_list(bw, bh, seed):
    """pos / par of every bw x bh block of frames 0..NF-1: vectors around the sequence's motion
    (13, 10) quarter pixels per frame with +-6 of spread, clipped to analyse.c's limits"""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(0, H, bh), np.arange(0, W, bw), indexing="ij")
    n1 = xs.size
    pos = np.stack([np.repeat(np.arange(NF), n1), np.tile(xs.ravel(), NF), np.tile(ys.ravel(), NF)], 1).astype(np.int32)
    n = len(pos)
    mbx, mby = pos[:, 1] // 16, pos[:, 2] // 16
    mbw, mbh = W // 16, H // 16
    lim = np.stack([4 * (-16 * mbx - 24), 4 * (-16 * mby - 24), 4 * (16 * (mbw - mbx - 1) + 24),
                    4 * (16 * (mbh - mby - 1) + 24)], 1)
    mv0 = np.array([13, 10]) + rng.integers(-6, 7, (n, 2))
    mv1 = np.array([26, 20]) + rng.integers(-6, 7, (n, 2))
    par = np.concatenate([mv0, mv1, lim], 1).astype(np.int16)
    return pos, par


def luma_read_bytes(par, cols, bw, bh):
    """bytes get_ref needs of the hpel planes: one plane at a full / half-pel phase, two otherwise"""
    mvx = np.clip(par[:, cols[0]].astype(np.int64), par[:, 4], par[:, 6])
    mvy = np.clip(par[:, cols[1]].astype(np.int64), par[:, 5], par[:, 7])
    idx = ((mvy & 3) << 2) + (mvx & 3)
    return int((1 + ((idx & 5) != 0)).sum()) * bw * bh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N",
                    help="run each kernel leg N times, untimed and without graphs (for a rocprofv3 --pmc run)")
    a = ap.parse_args()
    x = load_package()
    x.init(0)
    from x264hip import synth
    luma, stride, origin, nv, cs, co = synth.make_subpel_sequence(NF + 2, W, H, 8)
    dl, dn = torch.from_numpy(luma).cuda(), torch.from_numpy(nv).cuda()
    hp = x.hpel_filter(dl, origin, stride, W, H)
    planes = [dl] + list(hp)
    # frame k = 2 .. NF+1 is predicted from k - 1 (list 0) and k - 2 (list 1): views of one stack
    l0, l1 = [p[1:NF + 1] for p in planes], [p[0:NF] for p in planes]
    c0, c1 = [dn[1:NF + 1]], [dn[0:NF]]
    fenc = dl[2:NF + 2]
    pred = torch.zeros_like(dl[:NF])
    pred_c = [torch.zeros_like(dn[:NF])]
    outs = (pred, origin, stride, pred_c, co, cs)
    mbw, mbh = W // 16, H // 16
    flat = [16] * 64
    q4m, q4b, _, _ = x.cqm_init(8, [flat] * 8)
    mf, bias = torch.from_numpy(q4m[1, 26].copy()).cuda(), torch.from_numpy(q4b[1, 26].copy()).cuda()
    dct = torch.empty((NF * mbw * mbh, 256), dtype=torch.int16, device="cuda")
    nz = torch.empty(NF * mbw * mbh, dtype=torch.int32, device="cuda")

    cases, legs, info = {}, {}, {}
    for name, i_pixel, bi in (("p16x16", 0, False), ("p8x8", 3, False), ("b16x16", 0, True)):
        bw, bh = x.PIXEL_SIZES[i_pixel]
        pos, par = block_list(bw, bh, 5 + i_pixel)
        n = len(pos)
        dpos, dpar = torch.from_numpy(pos).cuda(), torch.from_numpy(par).cuda()
        mode = torch.full((n,), 3 | (32 << 8), dtype=torch.int32, device="cuda") if bi else None
        cases[name] = (i_pixel, dpos, dpar, mode)
        legs[name] = (lambda i_pixel=i_pixel, dpos=dpos, dpar=dpar, mode=mode: x.mb_mc(
            l0, l1 if mode is not None else None, origin, stride, i_pixel, dpos, dpar, mode,
            chroma=(1, c0, c1 if mode is not None else None, co, cs), outs=outs))
        lists = 2 if bi else 1
        rd = luma_read_bytes(par, (0, 1), bw, bh) + (luma_read_bytes(par, (2, 3), bw, bh) if bi else 0)
        rd += lists * n * 2 * (bw // 2 + 1) * (bh // 2 + 1)              # mc_chroma's rows and columns, U and V
        rd += n * (12 + 16 + (4 if bi else 0))                           # pos, par, mode
        wr = n * (bw * bh + 2 * (bw // 2) * (bh // 2))
        info[name] = {"blocks": n, "bytes_read": rd, "bytes_written": wr}
        # what this call replaces: the search's out to the host, the prediction planes back
        host_out = torch.empty((n, 4), dtype=torch.int32).pin_memory()
        dev_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        host_pred, host_pc = torch.empty(pred.shape, dtype=pred.dtype).pin_memory(), \
            torch.empty(pred_c[0].shape, dtype=pred.dtype).pin_memory()

        def copies(host_out=host_out, dev_out=dev_out, host_pred=host_pred, host_pc=host_pc):
            host_out.copy_(dev_out, non_blocking=True)
            pred.copy_(host_pred, non_blocking=True)
            pred_c[0].copy_(host_pc, non_blocking=True)
        legs["copies_" + name] = copies
        info["copies_" + name] = {"bytes_d2h": n * 16, "bytes_h2d": pred.numel() + pred_c[0].numel()}
    legs["mb_dct_quant"] = lambda: x.mb_dct_quant(4, fenc, origin, stride, pred, origin, stride, mbw, mbh, NF, mf, bias,
                                                  dct=dct, nz=nz)
    info["mb_dct_quant"] = {"bytes_read": 2 * NF * W * H, "bytes_written": NF * W * H * 2 + NF * mbw * mbh * 4}

    if a.kernels_only:
        for k, fn in legs.items():
            if not k.startswith("copies_"):
                for _ in range(a.kernels_only):
                    fn()
        torch.cuda.synchronize()
        return
    # the kernels as graphs of `calls` calls; the copies (pinned host memory on one side) as the same
    # number of calls enqueued back to back on the stream
    runs = {}
    side = torch.cuda.Stream()
    for k, fn in legs.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # first launches before the capture
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if k.startswith("copies_"):
            def run(fn=fn):
                for _ in range(a.calls):
                    fn()
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(a.calls):
                    fn()
            run = g.replay
        for _ in range(WARMUP_REPLAYS):
            run()
        runs[k] = run
    torch.cuda.synchronize()
    samples = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            samples[k].append(e0.elapsed_time(e1) / a.calls)
    result = {"frames": NF, "width": W, "height": H, "rounds": a.rounds, "calls": a.calls,
              "device": torch.cuda.get_device_name(0), "legs": {}}
    for k, v in samples.items():
        med = statistics.median(v)
        leg = {"ms": {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4)}, **info[k]}
        moved = sum(val for key, val in info[k].items() if key.startswith("bytes_"))
        leg["gb_per_s"] = round(moved / (med * 1e-3) / 1e9, 1)
        result["legs"][k] = leg
    for name in cases:
        m = result["legs"][name]["ms"]["median"]
        result["legs"][name]["ratio_to_mb_dct_quant"] = round(m / result["legs"]["mb_dct_quant"]["ms"]["median"], 3)
        result["legs"][name]["ratio_to_copies"] = round(m / result["legs"]["copies_" + name]["ms"]["median"], 4)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
