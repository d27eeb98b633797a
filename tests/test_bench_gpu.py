"""bench.py's contract on the GPU: one JSON line with the driver's keys, at
N=1 (C1, the smallest config) and through the N>1 sharded path (2 ranks on
cuda:0 with the gloo exchange: the measured-cost partition, side-stream band
sweep, max-over-ranks timing and slowest-shard roofline all run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_single_gpu_c1():
    p = subprocess.run([sys.executable, "bench.py", "--config", "c1", "--steps", "5", "--warmup", "1", "--full", "--no-cpu"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _json_line(p.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["value"] > 0
    assert d["config"]["workload"] == "single-chrom-40kb-5000-bins" and d["config"]["resolution_bp"] == 40000
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["achieved"] > 0


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the line holds the headline figure only (no roofline, no
    CPU baseline, no extra passes); --dump-outputs writes the bias the timed
    iterations left, float64, the same from run to run (seeded inputs) and
    the oracle's bias after the same warmup + steps iterations."""
    import numpy as np
    got = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "c1", "--steps", "4", "--warmup",
                            "2", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        line = _json_line(p.stdout)
        assert (KEYS - {"roofline"}) <= set(line)
        assert not {"roofline", "cpu_baseline", "vs_cpu_baseline", "tad_scan"} & set(line)
        assert line["steps"] == 4 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(1000.0 / line["ms_per_step"])
        assert sorted(os.listdir(d)) == ["bias.npy"]
        got.append(np.load(d / "bias.npy"))
    assert got[0].dtype == np.float64 and got[0].shape == (5000,)
    np.testing.assert_array_equal(got[0], got[1])
    # every one of the 6 iterations ran (tol 0): the oracle's bias after as many
    sys.path.insert(0, ROOT)
    import bench
    from hichap_master_amd import ice
    from oracle import ice_ref
    sizes, kw, _, _, _ = bench.config("c1")
    m = ice.ContactMatrix.synthetic(sizes, **kw)
    b1, b2, c = m.export_upper()
    m.close()
    n = int(sizes[0])
    bias, (f1, f2, fc) = ice_ref.ice_filters(b1, b2, c, n, np.array([0, n], dtype=np.int64))
    ice_ref._iterate(bias, f1, f2, fc, n, 0, n, 0.0, 6)
    # fp64 sums in another order: ~1e-13 relative after 6 sweeps; 1e-9 as smoke() asks of the weights
    np.testing.assert_allclose(got[0], bias, rtol=1e-9, atol=0)


def test_bench_two_ranks_sharded_path():
    env = dict(os.environ, HH_DEVICE="0", HH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--standalone",
           "--local-addr", "127.0.0.1", "bench.py", "--gpus", "2", "--nnz", "2e8", "--steps", "3", "--warmup", "1", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    d = _json_line(p.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert "sharded x2" in d["config"]["parallelism"]
    assert 0 < d["roofline"]["shard_nnz_upper"] < d["config"]["nnz_upper"]


def test_bench_gpus_flag_launches_ranks_itself():
    """``bench.py --gpus 2`` with no launcher starts its
    own two ranks (here both on cuda:0 with the gloo exchange, HH_DEVICE) and
    reports n_gpus 2 from the sharded path."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HH_DEVICE="0", HH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--nnz", "2e8", "--steps", "3", "--warmup", "1", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    d = _json_line(p.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert "sharded x2" in d["config"]["parallelism"]


def test_bench_gpus_flag_refuses_missing_devices():
    """More GPUs asked than the box has: non-zero exit and no JSON line, not a
    one-GPU number labelled n_gpus N."""
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HH_DEVICE")}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", str(n), "--config", "c1", "--steps", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "visible GPUs" in p.stderr
