"""Time the intra macroblock encode (x264hip_*_mb_encode_intra) on 1080p 4:2:0 frames (120 x 68
MBs), n_frames 1 and 16, 8 and 10 bit: all I_16x16, all I_4x4, all I_8x8, and a P-like mix with
5 % intra macroblocks (of the three kinds) after an inter call.  In the same run, alternating, it
times deblock_frames on the same shape: the same 254 dependent launches, one per macroblock
anti-diagonal, so that leg is the launch floor of this execution shape.  `us_per_launch` = graph
time / 254 per leg, `ratio` = leg / deblock leg of the same bit depth and n_frames.  Recorded, not
judged.

Content: a ramp with texture as fenc; qp 20..40 + QP_BD_OFFSET; with both neighbours every mode of
the macroblock's kind is drawn, at the picture's first row and column the modes that need no more
than what is there.  recon is encoded in place, call after call: every call does the same work.

Method (tools/mbenc_time.py's): each leg is captured into a graph of CALLS calls, warmed up, then
ROUNDS interleaved rounds of one replay between two device events: `graph_ms` is the median ms per
call (min, max beside it).  Writes one JSON line (and --out FILE).

usage: python tools/mbintra_time.py [--rounds 7] [--calls 2] [--out profiles/mbintra_time.json]"""
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
LAUNCHES = MBW + 2 * (MBH - 1)
WARMUP_REPLAYS = 2
FLAT = [[16] * 16] * 4 + [[16] * 64] * 4
INTRA, T8, I16 = 1, 2, 16


def picture(rng, nf, w, h, bd):
    y, x = np.mgrid[0:h, 0:w]
    ramp = 48 + abs(((x + y) >> 2) % 320 - 160) + 20 * np.sin(x / 9.0) * np.cos(y / 7.0)
    pic = np.clip(np.rint(ramp[None] + rng.normal(0, 3, (nf, h, w))), 0, 255) * (1 << (bd - 8))
    return torch.from_numpy(pic.astype(np.int64).astype(np.uint8 if bd == 8 else np.int16)).cuda()


def modes(rng, nf, kinds):
    """pred_mode [n, 16] and chroma_pred_mode [n], valid at every position; kinds [n]: 0 I_4x4,
    1 I_8x8, 2 I_16x16"""
    n = nf * MBW * MBH
    mx, my = np.tile(np.arange(MBW), nf * MBH), np.tile(np.repeat(np.arange(MBH), MBW), nf)
    top, left = (my > 0)[:, None], (mx > 0)[:, None]
    luma = np.where(top & left, rng.integers(0, 9, (n, 16)), np.where(top, rng.choice([0, 10], (n, 16)),
                    np.where(left, rng.choice([1, 9], (n, 16)), 11)))
    l16 = np.where(top & left, rng.integers(0, 4, (n, 1)), np.where(top, rng.choice([0, 5], (n, 1)),
                   np.where(left, rng.choice([1, 4], (n, 1)), 6)))
    luma[kinds == 2, 0] = l16[kinds == 2, 0]
    chroma = np.where(top & left, rng.integers(0, 4, (n, 1)), np.where(top, rng.choice([2, 5], (n, 1)),
                      np.where(left, rng.choice([1, 4], (n, 1)), 6)))[:, 0]
    return (torch.from_numpy(luma.astype(np.int8)).cuda(), torch.from_numpy(chroma.astype(np.int8)).cuda())


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
        for nf in (1, 16):
            n = nf * MBW * MBH
            fy, fc = picture(rng, nf, W, H, bd), picture(rng, nf, W, H // 2, bd)
            qp_h = (rng.integers(20, 41, n) + 6 * (bd - 8)).astype(np.int8)
            qp = torch.from_numpy(qp_h).cuda()
            common = dict(quant8=(q[2], q[3]), dequant8_mf=dq8, chroma_format=1, fenc_chroma=(fc, 0, W, W * H // 2),
                          b_dct_decimate=1, qp_table=table)
            r = rng.random(n)
            mixed = rng.integers(0, 3, n)
            for leg, kinds, intra in (("i16x16", np.full(n, 2), np.ones(n, bool)), ("i4x4", np.full(n, 0), np.ones(n, bool)),
                                      ("i8x8", np.full(n, 1), np.ones(n, bool)), ("p_mix_5pct", mixed, r < 0.05)):
                flags_h = np.where(intra, INTRA + np.array([0, T8, I16])[kinds], np.where(r < 0.5, T8, 0) + 4)
                flags = torch.from_numpy(flags_h.astype(np.uint8)).cuda()
                pm, cm = modes(rng, nf, kinds)
                ry, rc = fy.clone(), fc.clone()
                recon, recon_c = (ry, 0, W, W * H), (rc, 0, W, W * H // 2)
                outs = {"level": torch.zeros((n, 48, 16), dtype=cdt, device="cuda"),
                        "chroma_dc": torch.zeros((n, 2, 8), dtype=cdt, device="cuda"),
                        "luma_dc": torch.zeros((n, 16), dtype=cdt, device="cuda"),
                        "nnz": torch.zeros((n, 48), dtype=torch.uint8, device="cuda"),
                        "cbp": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "nz": torch.zeros(n, dtype=torch.int32, device="cuda"),
                        "flags_out": torch.zeros(n, dtype=torch.uint8, device="cuda")}
                if not intra.all():                         # the inter macroblocks, once, before the timed calls
                    x.mb_encode_inter((fy, 0, W, W * H), recon, MBW, MBH, nf, qp, flags, (q[0], q[1]), dq4, pred_chroma=recon_c,
                                      outs={k: v for k, v in outs.items() if k != "luma_dc"}, **common)
                name = "mb_encode_intra_%s_%dbit_n%d" % (leg, bd, nf)
                legs[name] = (lambda fy=fy, recon=recon, recon_c=recon_c, nf=nf, qp=qp, flags=flags, pm=pm, cm=cm, q=q, dq4=dq4,
                              outs=outs, common=common: x.mb_encode_intra(
                    (fy, 0, W, W * H), recon, MBW, MBH, nf, qp, flags, pm, (q[0], q[1]), dq4, recon_chroma=recon_c,
                    chroma_pred_mode=cm, outs=outs, **common))
                info[name] = {"n_frames": nf, "bit_depth": bd, "launches": LAUNCHES, "intra_share": round(float(intra.mean()), 4)}
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
        if k.startswith("mb_encode_intra"):
            bd_nf = "_".join(k.rsplit("_", 2)[-2:])                  # "<depth>bit_n<frames>"
            floor = result["legs"]["deblock_frames_" + bd_nf]["graph_ms"]["median"]
            result["ratio"][k + "_over_deblock"] = round(result["legs"][k]["graph_ms"]["median"] / floor, 3)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
