"""Stream order of the device entries: "asynchronous on `stream`, no host synchronisation"
(include/x264hip.h, x264hip_mc.h, x264hip_mbtree.h) on streams other than the null stream, which
is where every other GPU test runs.  tests/stream_cases.py has the method and the tables; the rows
are tests/test_gpu_footprint.py's, each at its first case, 8 and 10 bit, and the expected bytes
are the same row's on the null stream.

1. behind a delay -- every row on a fresh stream behind a delay kernel and the upload of its
   inputs: an internal launch, memset, gather or scratch free on another stream meets the fill
   the arena held before, and the bytes differ.
2. no host wait -- in the same test: the delay has not ended when the call returns.  Only the
   entries the header calls synchronous are exempt (stream_cases.WAITS).
3. two streams in flight -- the pairs that share library state (stream_cases.PAIRS), four rounds
   each on two streams released by one delay.  Overlap is likely, not certain: this leg can miss
   a fault, it cannot report one falsely.
4. the SSD ring's wrap -- on a side stream, two ssd_plane_batch (ssd_nv12_batch) calls of 33000
   frames of 16x4 pixels take 66000 of the ring's 65536 slots, so one range straddles the ring's
   end; then an ordinary call of 2 frames.  Every sum against numpy's in int64.

The delay is torch.cuda._sleep(stream_cases.DELAY_CYCLES), 120,000,000 cycles.  Measured on an
MI355X: the slowest row takes the host 0.145 ms for the arena's upload plus its call on a side
stream after one warm-up call (me_search_ref_tesa at 8 bit, a 434 KB arena; every other row is
quicker), and the delay kernel runs 49.97 ms between two timing events (three runs: 49.965 to
49.973 ms; 2.4 cycles per ns).  That is some 340 times the host's time, where 10 times was asked
for, to cover first-touch page faults and a loaded host, and a fifth of the 250 ms a test may
spend on it.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu


def _behind_delay(hip, name, bd, stream):
    """legs 1 and 2 of one row on `stream`"""
    p = sc.prepared(name, bd)
    want = sc.null_run(hip, p)
    got, ended = sc.side_run(hip, p, stream)
    assert sc.differing(p, got, want) is None, sc.differing(p, got, want)
    # (after the bytes: a delay that had ended proves nothing about them either way)
    if any(e in sc.WAITS for e in p.row.entries):
        return
    assert not ended, ("%s: the delay kernel in front of the call had ended when the call returned -- the call "
                       "waited for the stream (or took longer on the host than the delay)" % name)


# ------------------------------------------------------------------ 1, 2. every row behind a delay
@pytest.mark.parametrize("bd", sc.BITDEPTHS)
@pytest.mark.parametrize("name", sorted(sc.rows()))
def test_behind_delay(hip, name, bd):
    _behind_delay(hip, name, bd, torch.cuda.Stream())


# ------------------------------------------------------------------ 3. two streams in flight together
@pytest.mark.parametrize("bd", sc.BITDEPTHS)
@pytest.mark.parametrize("a,b", [p[:2] for p in sc.PAIRS], ids=["%s+%s" % p[:2] for p in sc.PAIRS])
def test_two_streams(hip, a, b, bd):
    ps = [sc.prepared(n, bd) for n in (a, b)]
    wants = [sc.null_run(hip, p) for p in ps]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [[p.fresh() for _ in range(sc.PAIR_ROUNDS)] for p in ps]
    torch.cuda.synchronize()

    def go():
        with torch.cuda.stream(streams[0]):
            torch.cuda._sleep(sc.DELAY_CYCLES)
            ev = torch.cuda.Event()
            ev.record(streams[0])
        streams[1].wait_event(ev)
        for r in range(sc.PAIR_ROUNDS):
            for p, st, bf in zip(ps, streams, bufs):
                sc.enqueue(hip, p, st, *bf[r])
        if a.startswith("lowres_"):
            for st in streams:
                with torch.cuda.stream(st):
                    hip.lowres_status()                  # waits for the stream; raises on a wavefront timeout
        for st in streams:
            st.synchronize()
    sc.guarded(go)
    for p, want, bf in zip(ps, wants, bufs):
        for r in range(sc.PAIR_ROUNDS):
            msg = sc.differing(p, bf[r][1].numpy(), want)
            assert msg is None, "round %d: %s" % (r, msg)


# ------------------------------------------------------------------ 4. the SSD ring's wrap
@pytest.mark.parametrize("bd", sc.BITDEPTHS)
@pytest.mark.parametrize("nv12", [0, 1], ids=["plane", "nv12"])
def test_ssd_ring_wrap(hip, nv12, bd):
    calls = sc.wrap_case(bd, nv12)
    fn = hip.ssd_nv12_batch if nv12 else hip.ssd_plane_batch
    dev = [[torch.from_numpy(x.view(np.int16) if bd == 10 else x).cuda() for x in (a, b)] for a, b, _ in calls]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def go():
        with torch.cuda.stream(side):
            outs = [fn(a, 0, sc.WRAP_W, b, 0, sc.WRAP_W, sc.WRAP_W // 2 if nv12 else sc.WRAP_W, sc.WRAP_H, a.shape[0])
                    for a, b in dev]
        side.synchronize()
        return [o.cpu().numpy() for o in outs]
    for k, (got, (_, _, want)) in enumerate(zip(sc.guarded(go), calls)):
        bad = np.argwhere(got != want)
        assert not len(bad), "call %d: %d of %d sums differ, first at %s" % (k, len(bad), want.size, bad[0])
