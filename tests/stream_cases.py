"""Stream-order checks of the device entries: what tests/test_gpu_streams.py runs and
tests/test_cpu_streams.py keeps complete.  No GPU code at import.

The rows are tests/test_gpu_footprint.py's (one per stream-taking entry: setup / call over a byte
arena), each at its first case, 8 and 10 bit; mb_mc, which has no row there, gets MBMC below.  The
expected bytes of a run are the same row's on the null stream, synchronised -- the footprint and
parity suites hold that run to the oracle.

A run `behind a delay` (side_run): the arena's device copy starts as THIRD_FILL in every byte,
and on the stream under test, without a host wait in between, go a delay kernel, the upload of
the arena from pinned memory, the row's call and the copy back.  A step of the entry that runs
on another stream meets the fill, not the inputs (or is overwritten by the upload), and an event
recorded right after the delay that has not completed when the call returns shows that the call
did not wait for the stream -- and that the inputs had not landed when it was enqueued.
"""
import functools
import os
import re
import types

import numpy as np

import footprint as fp
from test_gpu_footprint import EXCLUDED, ROWS, T, pdt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITDEPTHS = (8, 10)
THIRD_FILL = 0x3C               # neither of footprint.FILLS
assert THIRD_FILL not in fp.FILLS

# torch.cuda._sleep's argument for the delay kernel: 49.97 ms on an MI355X; tests/test_gpu_streams.py
# has the measurements behind it
DELAY_CYCLES = 120_000_000

# ------------------------------------------------------------------ the rows
# entries that take a stream and run behind no delay, with test_gpu_footprint.EXCLUDED's reason:
# the two that own no kernel of the library's, the two that have no device buffer, and the twins
# that are their _ex form with defaults (capi_entries.inc)
NOT_RUN = {name: EXCLUDED[name] for name in ("forward_ref", "upload", "stream_destroy", "lowres_status",
                                             "lowres_inter_cost", "lowres_bidir_cost")}

# entries that may wait for the stream: the header line that says so
WAITS = {"weights_analyse": "x264hip.h, weights_analyse: \"Synchronous: every candidate of a plane is scored in one "
                            "batch on the stream and the host replays the reference's search over the costs\""}

# two entries that share library state, in flight on two streams at once: (row, row, what they share)
PAIRS = [("ssd_plane_batch", "ssd_nv12_batch", "the SSD accumulator ring"),
         ("me_tesa", "me_search_ref_tesa", "the scratch pool"),
         ("ssim_wxh", "me_analyse_p16x16", "the scratch pool"),
         ("mbtree_propagate", "weight_cost_batch", "the scratch pool"),
         ("lowres_inter_cost_ex", "lowres_bidir_cost_ex", "the lookahead status word; wavefront kernels")]
PAIR_ROUNDS = 4


# ------------------------------------------------------------------ mb_mc: one call mixing the lists
MC_W, MC_H, MC_NF, MC_PIXEL = 96, 64, 2, 3


@functools.lru_cache(maxsize=None)
def _mc_ref(bd, seed):
    import mc_cases as mcc
    return mcc.make_ref(bd, MC_W, MC_H, 1, MC_NF, seed)


def _mbmc_setup(ar, bd):
    import mc_cases as mcc
    r0, r1 = _mc_ref(bd, 1), _mc_ref(bd, 2)
    pos = mcc.block_positions(MC_W, MC_H, MC_NF, MC_PIXEL)
    n = len(pos)
    par = mcc.make_par(pos, mcc.phase_mvs(pos, MC_W, MC_H, 8), mcc.phase_mvs(pos, MC_W, MC_H, 9, base=3), MC_W, MC_H)
    lists = np.arange(n) % 3 + 1                                   # list 0, list 1, both
    mode = (lists | (np.array([32, 24, 44, -8, 72])[np.arange(n) % 5] << 8)).astype(np.int32)

    def planes(prefix, arrays):
        return [ar.list("%s%d" % (prefix, k), a.shape, pdt(bd), a) for k, a in enumerate(arrays)]
    return types.SimpleNamespace(
        bd=bd, n=n, origin=r0.origin, stride=r0.stride, corigin=r0.corigin, cs=r0.cs,
        l0=planes("l0_", r0.luma), l1=planes("l1_", r1.luma), c0=planes("c0_", r0.chroma), c1=planes("c1_", r1.chroma),
        pos=ar.list("pos", (n, 3), np.int32, pos), par=ar.list("par", (n, 8), np.int16, par),
        mode=ar.list("mode", n, np.int32, mode), pred=ar.list("pred", r0.luma[0].shape, pdt(bd)),
        pred_c=ar.list("pred_c", r0.chroma[0].shape, pdt(bd)))


def _mbmc_call(hip, c, dev, tight):
    def ts(bufs):
        return [T(b, dev) for b in bufs]
    hip.mb_mc(ts(c.l0), ts(c.l1), c.origin, c.stride, MC_PIXEL, T(c.pos, dev), T(c.par, dev), T(c.mode, dev),
              chroma=(1, ts(c.c0), ts(c.c1), c.corigin, c.cs),
              outs=(T(c.pred, dev), c.origin, c.stride, [T(c.pred_c, dev)], c.corigin, c.cs))


# (a namespace, not a footprint Row: a Row would join test_gpu_footprint's ROWS and its test ids)
MBMC = types.SimpleNamespace(name="mb_mc", entries=("mb_mc",), cases=[("96x64x2-p3", {})], setup=_mbmc_setup,
                             call=_mbmc_call, variants=[], variant_case=lambda bd, case: True)


def rows():
    """name -> row of everything that runs behind the delay"""
    out = {r.name: r for r in ROWS}
    out[MBMC.name] = MBMC
    return out


def case_of(row):
    """the row's smallest case: its first"""
    return row.cases[0][1]


# ------------------------------------------------------------------ the header's word on waiting
def header_comment(entry):
    """the comment in front of `entry`'s prototype in include/"""
    for header in ("x264hip.h", "x264hip_mc.h", "x264hip_mbtree.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        m = re.search(r"\bint\s+x264hip_(?:##BD##_|8_|10_)?%s\s*\(" % re.escape(entry), text)
        if m:
            end = text.rfind("*/", 0, m.start())
            return text[text.rfind("/*", 0, end):end]
    raise KeyError(entry)


# ------------------------------------------------------------------ runs
class Prepared:
    """one row at one bit depth: its buffers, the arena's bytes in pinned memory, and the bytes a
    null-stream run leaves, each computed once and never modified"""

    def __init__(self, row, bd):
        import torch
        ar = fp.Arena(fp.FILLS[0])
        self.row, self.bd = row, bd
        self.c = row.setup(ar, bd, **case_of(row))
        self.c.check = False                     # the lookahead wrappers: no lowres_status() behind the launch
        self.pinned = torch.from_numpy(ar.bytes().copy()).pin_memory()
        self.nbytes, self.bufs = ar.used, ar.bufs
        self.want = None

    def fresh(self):
        """(device arena holding THIRD_FILL, pinned buffer for the result)"""
        import torch
        return (torch.full((self.nbytes,), THIRD_FILL, dtype=torch.uint8, device="cuda"),
                torch.zeros(self.nbytes, dtype=torch.uint8).pin_memory())


_PREPARED = {}


def prepared(name, bd):
    if (name, bd) not in _PREPARED:
        _PREPARED[name, bd] = Prepared(rows()[name], bd)
    return _PREPARED[name, bd]


FAULTS = ("illegal memory access", "hipErrorIllegalAddress", "unspecified launch failure", "hipErrorLaunchFailure")


def guarded(fn):
    """fn(); a GPU fault (FAULTS in the error's text) ends the session: nothing more runs on this
    device.  Any other error -- a bad argument, a lookahead "timed out" report -- fails the test only."""
    import pytest
    try:
        return fn()
    except RuntimeError as e:
        if any(f in str(e) for f in FAULTS):
            pytest.exit("GPU fault: %s" % e, returncode=3)
        raise


def null_run(hip, p):
    """the bytes of the arena after the row's call on the null stream, synchronised (the current
    stream must be the default one)"""
    import torch
    if p.want is None:
        def go():
            dev = p.pinned.cuda()
            p.row.call(hip, p.c, dev, False)
            torch.cuda.synchronize()
            return dev.cpu().numpy()
        p.want = guarded(go)
    return p.want


def enqueue(hip, p, stream, dev, back):
    """upload, call, copy back on `stream`, no host wait"""
    import torch
    with torch.cuda.stream(stream):
        dev.copy_(p.pinned, non_blocking=True)
        p.row.call(hip, p.c, dev, False)
        back.copy_(dev, non_blocking=True)


def side_run(hip, p, stream, cycles=DELAY_CYCLES):
    """the row behind a delay on `stream`: (bytes after, whether the delay had ended when the call
    returned)"""
    import torch
    dev, back = p.fresh()
    torch.cuda.synchronize()

    def go():
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
            ev = torch.cuda.Event()
            ev.record(stream)
            dev.copy_(p.pinned, non_blocking=True)
            p.row.call(hip, p.c, dev, False)
            ended = ev.query()
            back.copy_(dev, non_blocking=True)
        stream.synchronize()
        return ended
    ended = guarded(go)
    return back.numpy(), ended


def differing(p, got, want):
    """where two runs of a row differ, by buffer: a message, or None"""
    if np.array_equal(got, want):
        return None
    at = np.flatnonzero(got != want)
    names = [b.name for b in p.bufs if ((at >= b.start) & (at < b.start + b.nbytes)).any()]
    return "%s, %d bit: %d byte(s) differ from the null-stream run, first at arena offset %d, in %s" % (
        p.row.name, p.bd, at.size, at[0], names or "no buffer")


# ------------------------------------------------------------------ the SSD ring's wrap
SSD_RING = 65536                 # pixel.hip's ring: slots of launches in flight, taken from a running counter
WRAP_FRAMES, WRAP_W, WRAP_H = 33000, 16, 4       # two such calls take 66000 slots: one of them straddles the end
SSD_LIMIT = 1 << 48              # "a frame's SSD below 2^48": the plane path's packed accumulator


@functools.lru_cache(maxsize=None)
def wrap_case(bd, nv12):
    """the calls of one wrap run: [(pix1, pix2 [n, 4, 16], expected int64 [n] or [n, 2])] -- two of
    WRAP_FRAMES frames on different pictures, then an ordinary one of 2 frames.  nv12: 8 chroma
    pairs per row, U in the even columns.  The sums are numpy's, in int64."""
    rs = np.random.default_rng(bd + nv12)
    out = []
    for n in (WRAP_FRAMES, WRAP_FRAMES, 2):
        a, b = (rs.integers(0, 1 << bd, (n, WRAP_H, WRAP_W)).astype(pdt(bd)) for _ in range(2))
        d = (a.astype(np.int64) - b.astype(np.int64)) ** 2
        want = np.stack([d[:, :, 0::2].sum((1, 2)), d[:, :, 1::2].sum((1, 2))], 1) if nv12 else d.sum((1, 2))
        out.append((a, b, want))
    return out
