"""GPU, two ranks: optim.AdamW(flat_grads=True) under the launcher.  ONE launch of tests/_optim_rank_probe.py — two ranks
over gloo that share the GPU, the form of test_syncbn_ranks_gpu.py: a residual block with SyncBatchNorm2d takes two training steps, each
rank on its half of the batch.  opt.sync_gradients() — one all_reduce of the gradient arena — must leave the bits dist.sync_gradients
leaves on clones of the same gradients, and parameters, moments, the gradient norm and the step count must have the same bits on both
ranks after each step.  The probe exits non-zero at its first failure and writes what it measured."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "_optim_rank_probe.py")


def test_flat_gradients_on_two_ranks(tmp_path):
    from omnifusion_amd import dist
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    out = str(tmp_path / "probe.json")
    r = subprocess.run(dist.launch_command(PROBE, [out], 2), env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [json.load(open(f"{out}.{rank}")) for rank in range(2)]
    for rank, info in enumerate(ranks):
        assert info["rank"] == rank and info["world"] == 2 and info["steps"] == 2
        for step in range(2):
            assert info[f"{step}.local_differs"] is True                        # the ranks saw different halves of the batch
            assert info[f"{step}.sync_bits"] is True and info[f"{step}.sync_changed"] is True
            assert info[f"{step}.finite"] is True and info[f"{step}.state_equal"] is True
            assert info[f"{step}.grad_norm"] == ranks[0][f"{step}.grad_norm"] > 0.0
