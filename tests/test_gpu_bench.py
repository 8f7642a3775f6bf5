"""bench.py's one-line JSON contract on the GPU (short run: 2 timed steps, --full without the
side rates, a 0.3-s CPU sample): the keys the driver and the judge read, their types and the
consistency of the roofline record with the line's own numbers; a plain run's line and its
--dump-outputs files."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1",
                        "--frames", "8", "--no-extra", "--cpu-seconds", "0.3"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "u8"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-6)
    assert 0 < rf["frac"] < 1
    # value = candidates per step / step time; launch_ms <= ms_per_step
    cands = d["config"]["frames_per_step_per_gpu"] * d["config"]["mbs_per_frame"] * d["config"]["candidates_per_mb"]
    assert d["value"] == pytest.approx(cands / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert rf["launch_ms"] <= d["ms_per_step"] * 1.001
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path, oracle):
    """A plain run (no --full) times the headline only: no side rates, no cpu_baseline; and
    --dump-outputs writes the last step's SAD tables, here every MB of a 2-pair 96x48 run,
    equal to the oracle's full search of the same seeded frames."""
    import numpy as np
    from conftest import load_package
    load_package()
    from x264hip import synth
    w, h, rng, f = 96, 48, 8, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--frames", str(f), "--width", str(w), "--height", str(h), "--range", str(rng),
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert "extra" not in d and "cpu_baseline" not in d
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["me_table.npy", "me_table_mb_index.npy"]
    got = np.load(tmp_path / "out" / "me_table.npy")
    idx = np.load(tmp_path / "out" / "me_table_mb_index.npy")
    mbw, mbh = w // 16, h // 16
    assert got.dtype == np.float32 and idx.dtype == np.float64
    assert np.array_equal(idx, np.arange(f * mbw * mbh))
    planes, stride, origin = synth.make_sequence(f + 1, w, h, 8)
    want = np.stack([oracle.me_search_full(8, planes[k + 1].ravel(), origin, stride, planes[k].ravel(), origin,
                                           stride, mbw, mbh, rng) for k in range(f)])
    assert np.array_equal(got, want.reshape(got.shape).astype(np.float32))


@pytest.mark.gpu
def test_bench_two_ranks_gloo():
    """The N-rank path the driver's scaling run uses:
    bench.py --gpus 2 starts its own two ranks (a fresh child process; this process is never
    exec'd), both on the box's one GPU over gloo, and rank 0 prints one line whose value is the
    two ranks' candidates over the max-over-ranks step time."""
    import time
    env = dict(os.environ, X264HIP_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--frames", "2", "--no-extra",
                        "--no-cpu", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    c = d["config"]
    assert d["n_gpus"] == 2 and c["world_size"] == 2 and c["rank_devices"] == [0, 0]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["ms_per_step"] * d["steps"] * 1e-3 < wall
    cands = 2 * c["frames_per_step_per_gpu"] * c["mbs_per_frame"] * c["candidates_per_mb"]
    assert d["value"] == pytest.approx(cands / (d["ms_per_step"] * 1e-3), rel=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_2160p_workload(gpus):
    """bench.py --workload 2160p (configs[3]: a 2160p frame per GPU per step, full search + refine +
    DCT/quant, H2D in the timed region): one line, config.workload = configs[3], value = the ranks'
    candidates per step over the step time; with --gpus 2 the two ranks share the box's GPU over
    gloo (the path the driver's 8-GPU scaling run takes over RCCL)."""
    env = dict(os.environ, X264HIP_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "2160p", "--gpus", str(gpus),
                        "--full", "--steps", "3", "--warmup", "2", "--cpu-seconds", "0.3"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    c = d["config"]
    assert c["workload"].startswith("configs[3]") and d["n_gpus"] == gpus and c["world_size"] == gpus
    assert c["candidates_per_mb"] > c["table_candidates_per_mb"] and c["mbs_per_frame"] == 240 * 135
    cands = gpus * c["frames_per_step_per_gpu"] * c["mbs_per_frame"] * c["candidates_per_mb"]
    assert d["value"] == pytest.approx(cands / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert 0 < d["roofline"]["frac"] < 1
    assert ("cpu_baseline" in d) == (gpus == 1)
