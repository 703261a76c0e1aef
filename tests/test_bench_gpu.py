"""bench.py end to end on the GPU box: the JSON contract (plain and --full), the outputs of the last timed step, and
`--gpus 2` started as ONE process (it must re-execute itself as 2 ranks; on this single-GPU box the ranks share the GPU
through the gloo backend hook — the driver's 8-GPU launch is the same code with backend nccl = RCCL and one GPU per rank)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2",
                        "--no-cpu-baseline"] + extra, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


def test_bench_json_contract_single_gpu():
    d = _run(["--batch", "2", "--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert "workload" in d["config"]


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline fields only, and --dump-outputs writes what the last timed step returned: the depth maps of
    the seeded input batch, bit for bit what one plain forward of the same panoramas returns."""
    d = _run(["--batch", "2", "--dump-outputs", str(tmp_path)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "panoramas/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    for k in ("value_long", "pipelining", "host_fed", "batch1", "roofline", "roofline_resample", "configs", "cpu_baseline"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["depth.npy"]
    got = np.load(tmp_path / "depth.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1, 512, 1024) and np.isfinite(got).all()
    import torch
    sys.path.insert(0, ROOT)
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    rgb = torch.rand((2, 3, 512, 1024), generator=torch.Generator(device="cpu").manual_seed(1234))     # bench.py's rank-0 input
    net = spherical_fusion(4, 18, (128, 128), (80.0, 80.0)).cuda(0)
    net.load_state_dict(make_state_dict(42, 18, False))
    want = net(rgb.cuda(0), confidence=True).cpu().numpy()
    assert np.array_equal(got, want)


def test_bench_gpus_2_spawns_two_ranks(tmp_path):
    d = _run(["--gpus", "2", "--batch", "2", "--full", "--dump-outputs", str(tmp_path)], {"OMNI_BENCH_DIST_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4
    assert abs(d["value"] - 4 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    got = np.load(tmp_path / "depth.npy")                          # both ranks' panoramas, rank 0's first
    assert got.shape == (4, 1, 512, 1024) and np.isfinite(got).all() and not np.array_equal(got[:2], got[2:])


def test_bench_rejects_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stdout + r.stderr)


def test_bench_under_launcher_one_rank_rccl():
    """The driver's launch form with N = 1: torch.distributed.run starts one rank, the process group is RCCL (backend nccl), and the
    barrier + MAX all-reduce of the timing protocol run on the device — the same calls the 8-GPU launch makes."""
    sys.path.insert(0, ROOT)
    from omnifusion_amd import dist
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "OMNI_BENCH_DIST_BACKEND"):
        env.pop(k, None)
    cmd = dist.launch_command(os.path.join(ROOT, "bench.py"), ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2", "--no-cpu-baseline"], 1)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0
