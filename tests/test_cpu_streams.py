"""The tables of tests/stream_cases.py without a GPU: every stream-taking entry of the ctypes table
runs behind the delay of tests/test_gpu_streams.py or is named with a reason, only entries the
header calls synchronous may wait, the pairs that run on two streams exist, and the sums of the
ring-wrap case are the oracle's and stay in range."""
import numpy as np

import stream_cases as sc
from test_cpu_footprint import _stream_entries
from test_gpu_footprint import EXCLUDED, ROWS


def test_every_stream_entry_runs_behind_the_delay_or_has_a_reason():
    entries = _stream_entries()
    run = {e for row in sc.rows().values() for e in row.entries}
    assert "mb_mc" in run and not run & set(sc.NOT_RUN)
    missing = [e for e in entries if e not in run and e not in sc.NOT_RUN]
    assert not missing, "stream entries neither run behind the delay nor named: %s" % missing
    stale = [e for e in list(run) + list(sc.NOT_RUN) if e not in entries]
    assert not stale, "rows or reasons for entries the ctypes table does not have: %s" % stale
    # the reasons are the footprint suite's: no kernel of the library's, no device buffer, an _ex twin
    assert set(sc.NOT_RUN) == {"forward_ref", "upload", "stream_destroy", "lowres_status", "lowres_inter_cost",
                               "lowres_bidir_cost"}
    assert all(sc.NOT_RUN[e] == EXCLUDED[e] for e in sc.NOT_RUN)
    for twin in ("lowres_inter_cost", "lowres_bidir_cost"):
        assert twin + "_ex" in run and "_ex" in sc.NOT_RUN[twin]
    # every row has a first case to run
    assert all(row.cases and isinstance(sc.case_of(row), dict) for row in sc.rows().values())


def test_only_entries_the_header_calls_synchronous_may_wait():
    entries = _stream_entries()
    for e, why in sc.WAITS.items():
        assert e in entries and "Synchronous" in sc.header_comment(e), e
        assert "Synchronous" in why
    # and the header calls no other entry so: what it says is what the no-wait leg pins
    said = [e for e in entries if e not in sc.NOT_RUN and e not in sc.WAITS and "Synchronous" in sc.header_comment(e)]
    assert not said, "the header calls these synchronous, the suite holds them to no host wait: %s" % said
    assert "Asynchronous" in sc.header_comment("lowres_inter_cost")


def test_pairs_exist():
    names = {r.name for r in ROWS}
    for a, b, shared in sc.PAIRS:
        assert a in names and b in names and a != b and shared
    assert len(sc.PAIRS) == 5 and sc.PAIR_ROUNDS == 4


def test_ring_wrap_sums_in_range(oracle):
    """ssd_plane_batch / ssd_nv12_batch: "uint64 results"; the plane path packs a frame's SSD below
    2^48 (pixel.hip), a launch takes one ring slot per frame and at most the ring.  The numpy sums
    are the oracle's on the first and last frames of every call."""
    assert sc.WRAP_FRAMES <= 65535 < sc.SSD_RING < 2 * sc.WRAP_FRAMES      # one launch fits, two wrap
    for bd in sc.BITDEPTHS:
        assert sc.WRAP_W * sc.WRAP_H * ((1 << bd) - 1) ** 2 < sc.SSD_LIMIT
        for nv12 in (0, 1):
            calls = sc.wrap_case(bd, nv12)
            assert [len(a) for a, _, _ in calls] == [sc.WRAP_FRAMES, sc.WRAP_FRAMES, 2]
            for a, b, want in calls:
                assert want.dtype == np.int64 and want.shape == ((len(a), 2) if nv12 else (len(a),))
                assert 0 <= want.min() and want.max() < sc.SSD_LIMIT and want.any()
                assert a.shape[1:] == (sc.WRAP_H, sc.WRAP_W) and a.nbytes <= 5 << 20
                for f in (0, 1, len(a) - 1):
                    args = (bd, a[f].ravel(), 0, sc.WRAP_W, b[f].ravel(), 0, sc.WRAP_W)
                    if nv12:
                        assert oracle.ssd_nv12(*args, sc.WRAP_W // 2, sc.WRAP_H) == tuple(int(v) for v in want[f])
                    else:
                        assert oracle.ssd_wxh(*args, sc.WRAP_W, sc.WRAP_H) == int(want[f])
            assert not np.array_equal(calls[0][2], calls[1][2])             # a stale result of call 1 would show
