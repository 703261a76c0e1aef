"""GPU, two ranks: ops.sync_batch_norm, sync_batchnorm.convert_model and dist.sync_gradients under the launcher.  ONE launch
of tests/_syncbn_rank_probe.py — two ranks over gloo that share the GPU, as in test_bench_gpu.py — covers (a) the operator against float64
on the concatenated batch, (b) a residual block's training step, (c) the whole model's training-mode forward and (d) the world-1 paths;
the probe exits non-zero at its first failure and writes what it measured, which the tests below assert on.  A second, single process
without a launcher runs (d) where no process group exists at all.

(c): every batch normalisation's updated running mean and variance against tests/_train_model_ref.py at bs = 2 in float64 on the device's
own patches; the gate is test_train_model_gpu.py's, max(8 . e32, 3e-5)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "_syncbn_rank_probe.py")
CONV_GATE = 3e-5
_OUT = {}


def _env():
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    return env


@functools.lru_cache(maxsize=None)
def launch(tmp):
    """the one two-rank launch -> [rank 0's results, rank 1's]"""
    from omnifusion_amd import dist
    out = os.path.join(tmp, "probe.json")
    r = subprocess.run(dist.launch_command(PROBE, ["gpu", out], 2), env=_env(), capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _OUT["path"] = out
    return [json.load(open(f"{out}.{rank}")) for rank in range(2)]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    return launch(str(tmp_path_factory.mktemp("syncbn_ranks")))


def test_operator_on_two_ranks_vs_float64(ranks):
    for rank, info in enumerate(ranks):
        assert info["rank"] == rank and info["world"] == 2
        for name in ("odd105", "offset"):
            keys = [k for k in info if k.startswith(f"a.{name}.") and not k.endswith("buffers_equal")]
            assert len(keys) == (7 if name == "odd105" else 6), keys               # y, dx, dw, db, (dres,) rm, rv
            for k in keys:
                e, gate = info[k]
                print(f"syncbn ranks [{rank}] {k}: normalised error {e:.3e}  gate {gate:.3e}")
                assert e <= gate, (rank, k, e, gate)
            assert info[f"a.{name}.buffers_equal"] is True


def test_residual_block_step_on_two_ranks(ranks):
    for rank, info in enumerate(ranks):
        grads = [k for k in info if k.startswith("b.grad.")]
        assert sorted(grads) == sorted(f"b.grad.{k}" for k in ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "x"))
        for k in grads + [k for k in info if k.startswith("b.after.") and not k.endswith("num_batches_tracked")]:
            e, gate = info[k]
            print(f"syncbn ranks [{rank}] {k}: normalised error {e:.3e}  gate {gate:.1e}")
            assert gate == CONV_GATE and e <= gate, (rank, k, e)
        assert info["b.after.bn1.num_batches_tracked"] == 1 and info["b.after.bn2.num_batches_tracked"] == 1
        assert info["b.state_equal"] is True                                    # parameters and buffers after the step: the same bits on both ranks


def test_whole_model_forward_on_two_ranks(ranks):
    import _train_model_ref as ref
    from omnifusion_amd.model import trainable
    from omnifusion_amd.weights import make_state_dict
    for info in ranks:
        assert info["c.buffers_equal"] is True and info["c.tracked"] == [1] and info["c.buffers"] > 100
    saved = torch.load(_OUT["path"] + ".model.pt")
    nrows, N, P = 3, 10, 128
    points_in = trainable.spherical_fusion(nrows, N, (P, P), (80, 80)).point_input("cpu")
    results = {}
    for dtype in (torch.float64, torch.float32):
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in make_state_dict(42, N).items()}
        stats = {}
        with torch.no_grad():
            pf = ref.mlp_points(sd, points_in.to(dtype), True, 0.0, stats)       # [N, ...]: not synchronised, as on one device
            ref.network(sd, saved["patches"].to(dtype).reshape(2 * N, 3, P, P), pf, 2, N, True, 0.0, stats)
        results[dtype] = stats
    r64, r32 = results[torch.float64], results[torch.float32]
    assert sorted(saved["stats"]) == sorted(r64)
    worst = (0.0, None)
    for k, want in r64.items():
        gate = max(8.0 * nerr(r32[k], want), CONV_GATE)
        e = nerr(saved["stats"][k], want)
        worst = max(worst, (e / gate, k))
        assert torch.isfinite(saved["stats"][k]).all() and e <= gate, f"{k}: {e:.3e} > {gate:.3e}"
    print(f"syncbn ranks (c): {len(r64)} running buffers at bs = 2, largest error / gate {worst[0]:.3f} ({worst[1]})")


def nerr(got, want):
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def test_world_one_paths(ranks, tmp_path):
    for info in ranks:
        assert info["d.eval"] is True and info["d.train0"] is True             # eval mode; a one-rank group under the launcher
    out = str(tmp_path / "one.json")
    r = subprocess.run([sys.executable, PROBE, "gpu1", out], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    info = json.load(open(out + ".0"))
    assert info["world"] == 1 and info["d.eval"] is True and info["d.train0"] is True
