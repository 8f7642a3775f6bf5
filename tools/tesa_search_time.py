"""Time x264hip_*_me_search_ref_tesa against the calls a caller had before it.

Workload: bench.py's search legs' (rates_refine's 16 1080p 4:2:0 pairs, search_params' mvp / mvc),
me_range 16, subme 7 with chroma ME, every 16x16 and every 8x8 partition.  Legs, alternating in one
process, device events around ITERS calls after a warm-up round, ROUNDS rounds:
  tesa     the new call (predictor stage with SATD, window, refine with fpelcmp = SATD)
  hex      me_search_ref HEX on the same inputs (a proxy for predictor stage + refine)
  esa      me_search_ref ESA (every candidate of the same window scored)
  me_tesa  16x16 only: the window stage alone by me_tesa's in-scan SAD kernel
           (X264HIP_TESA_VARIANT=1) around the rounded mvp
Prints one line per leg: ms per call, min .. max over the rounds.  The 16x16 yardstick is hex +
me_tesa: the two calls TESA needed before.  Usage: python tools/tesa_search_time.py [rounds]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

ITERS = 3


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    x = load_package()
    x.init(0)
    from x264hip import synth
    W, H, F, me_range, subme = 1920, 1088, 16, 16, 7
    mbw, mbh = W // 16, H // 16
    luma, stride, origin, nv, cs, co = synth.make_subpel_sequence(F + 1, W, H, 8)
    dev, nvd = torch.from_numpy(luma).cuda(), torch.from_numpy(nv).cuda()
    fstride = luma[0].size
    planes = [dev[:-1]] + list(x.hpel_filter(dev[:-1], origin, stride, W, H))
    ext = x.refine_ext(1, 1, 0, fenc_chroma=[nvd[1:]], fenc_chroma_origin=co, fenc_chroma_stride=cs,
                       ref_chroma=[nvd[:-1]], ref_chroma_origin=co, ref_chroma_stride=cs)
    _, _, cm, span = bench.tesa_params(mbw, mbh, F, me_range)
    cm_d = torch.from_numpy(cm.view(np.int16)).cuda()
    integ = x.frame_integral(dev[:-1], origin, stride, H, sub8x8=True)
    integ1 = x.frame_integral(dev[:-1], origin, stride, H)
    legs = []
    for i_pixel in (0, 3):
        pos, par, mvc = bench.search_params(mbw, mbh, F, i_pixel)
        n = len(pos)
        pos_d, par_d, mvc_d = (torch.from_numpy(v).cuda() for v in (pos, par, mvc))
        out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        ne = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        scan = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        kw = dict(out=out, fenc_frame_stride=fstride, ref_frame_stride=fstride, ext=ext)

        def tesa(i_pixel=i_pixel, pos_d=pos_d, par_d=par_d, mvc_d=mvc_d, kw=kw, ne=ne, scan=scan):
            x.me_search_ref_tesa(dev[1:], origin, stride, dev[:-1], planes, origin, stride, integ, i_pixel, subme,
                                 me_range, pos_d, par_d, mvc_d, (cm_d, span), nevals=ne, scan=scan, **kw)

        def ref(me, i_pixel=i_pixel, pos_d=pos_d, par_d=par_d, mvc_d=mvc_d, kw=kw):
            x.me_search_ref(dev[1:], origin, stride, dev[:-1], planes, origin, stride, i_pixel, me, subme, me_range,
                            pos_d, par_d, mvc_d, (cm_d, span), **kw)

        sz = "16x16" if i_pixel == 0 else "8x8"
        legs += [(f"{sz} tesa", tesa, n, (ne, scan)), (f"{sz} hex", lambda ref=ref: ref(1), n, None),
                 (f"{sz} esa", lambda ref=ref: ref(3), n, None)]
        if i_pixel == 0:
            tpar = np.zeros((n, 8), np.int16)
            tpar[:, 0] = np.clip((par[:, 0] + 2) >> 2, par[:, 2], par[:, 4])
            tpar[:, 1] = np.clip((par[:, 1] + 2) >> 2, par[:, 3], par[:, 5])
            tpar[:, 2:4], tpar[:, 4:8] = par[:, 0:2], par[:, 2:6]
            tpar_d = torch.from_numpy(tpar).cuda()
            init_d = torch.full((n,), 1 << 30, dtype=torch.int32, device="cuda")
            tout = torch.empty((n, 4), dtype=torch.int32, device="cuda")

            def me_tesa():
                x.me_tesa(dev[1:], origin, stride, dev[:-1], origin, stride, integ1, mbw, mbh, F, me_range, tpar_d,
                          init_d, (cm_d, span), satd=True, out=tout, fenc_frame_stride=fstride,
                          ref_frame_stride=fstride)
            legs.append(("16x16 me_tesa", me_tesa, n, None))
    x.set_variant("X264HIP_TESA_VARIANT", 1)
    ms = {name: [] for name, *_ in legs}
    for r in range(rounds + 1):                       # round 0 warms up
        for name, fn, n, _ in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ITERS):
                fn()
            e1.record()
            e1.synchronize()
            if r:
                ms[name].append(e0.elapsed_time(e1) / ITERS)
    print(f"1080p x {F} pairs, me_range {me_range}, subme {subme}, chroma ME; {rounds} rounds of {ITERS} calls; "
          f"ms per call: median (min .. max)")
    for name, fn, n, cnt in legs:
        v = sorted(ms[name])
        line = f"{name:14s} {v[len(v) // 2]:8.3f} ({v[0]:.3f} .. {v[-1]:.3f})  {n} partitions"
        if cnt is not None:
            ne, scan = (t.cpu().numpy().astype(np.int64) for t in cnt)
            line += (f"; per partition: {(ne[:, 0] & 0xFFFF).mean():.2f} fpelcmp, {(ne[:, 0] >> 16).mean():.2f} get_ref, "
                     f"{scan[:, 0].mean():.1f} scan SADs, {scan[:, 1].mean():.1f} listed")
        print(line)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(f"16x16: tesa {med['16x16 tesa']:.3f} ms vs hex + me_tesa {med['16x16 hex'] + med['16x16 me_tesa']:.3f} ms")


if __name__ == "__main__":
    main()
