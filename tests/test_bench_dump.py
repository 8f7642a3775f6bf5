"""CPU: bench.py's --dump-outputs helpers (the sample of a large output is fixed, the .npy files
are float32 / float64 and hold the integers exactly, the byte limit holds) and the --full /
--dump-outputs options of its parser."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    try:
        import bench as b
    finally:
        sys.path.remove(ROOT)
    return b


def test_sample_rows_fixed(bench):
    assert np.array_equal(bench.sample_rows(10, 10), np.arange(10))
    a, b = bench.sample_rows(100000, 777), bench.sample_rows(100000, 777)
    assert np.array_equal(a, b)                         # the same rows in every run
    assert a.size == 777 and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 100000


def test_dump_outputs_exact(bench, tmp_path):
    u16 = np.array([[0, 1, 65280, 65535]], np.uint16)
    i32 = np.array([-(1 << 31), -1, (1 << 24) + 1, (1 << 31) - 1], np.int32)
    bench.dump_outputs(str(tmp_path / "d"), 0, {"a": u16, "b": i32})
    bench.dump_outputs(str(tmp_path / "d"), 1, {"a": u16})
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "a.rank1.npy", "b.npy"]
    a, b = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert a.dtype == np.float32 and b.dtype == np.float64
    assert np.array_equal(a.astype(np.uint16), u16) and np.array_equal(b.astype(np.int32), i32)


def test_dump_outputs_limit(bench, tmp_path):
    assert bench.DUMP_LIMIT < 64 * 1000 * 1000
    big = np.zeros(bench.DUMP_LIMIT // 4 + 1, np.uint8)  # float32: 4 bytes each, one over the limit
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "d"), 0, {"big": big})
    assert not os.path.exists(tmp_path / "d" / "big.npy")


def test_parser_options(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 3 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"
