"""The synchronised batch normalisation's split calls (csrc/omni_batchnorm.hip omni_syncbn_*) against the fused calls they
were cut from, at the output shapes of the network's convolutions, B = 8 panoramas x 18 patches (M = 144: tools/batchnorm_bench.py's shapes).

    python tools/syncbn_bench.py [--m 144] [--iters 20] [--rounds 5] [--only 0,3] [--no-gather] [--out profiles/r29a_syncbn.json]

Per layer, in ONE process and one run, the library alone on buffers allocated once, every gradient asked for, world = 1 (the record is the
call's own):
    fused_fwd   omni_batchnorm_fwd_f32 (stats + finish + apply)          split_fwd   omni_syncbn_stats_f32 + omni_syncbn_fwd_apply_f32
    fused_bwd   omni_batchnorm_bwd_f32 (reduce + finish + apply)         split_bwd   omni_syncbn_bwd_reduce_f32 + omni_syncbn_bwd_apply_f32
Device events around `iters` back-to-back calls; the four are INTERLEAVED — round k times all four before round k + 1 — and the median of
the rounds is reported with their range, so a drift of the clock falls on both sides.  The split form moves the same bytes per element
(fwd 16 B, bwd 28 B); it adds one C-sized launch to the forward and none to the backward.  What the collective between the two halves
costs is measured apart on a ONE-rank RCCL group under the launcher, host time per call over `iters` calls between synchronisations:
dist.all_gather_records of 2 C + 1 doubles — at world 1 the identity by contract, so this is the cost of the call where nothing is
exchanged — and the torch.distributed.all_gather_into_tensor it issues when world > 1, on the same record (`collective`: the stream
ordering and the launch of a real RCCL collective; no link is crossed).
There is no GPU -> the tool fails; it never falls back.  A multi-GPU training step is timed only where more than one GPU is present."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from omnifusion_amd import _lib, build, dist  # noqa: E402
from batchnorm_bench import CFGS  # noqa: E402

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
GATHER_C = (32, 64, 128, 256, 512)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                                   # microseconds per call


def gather_rank(a):
    """under the launcher: the latency of all_gather_records on the group dist.init() creates (RCCL)"""
    rank, _, world, dev = dist.init()
    rows = []
    for C in GATHER_C:
        rec = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
        out = torch.empty(world * (2 * C + 1), dtype=torch.float64, device=dev)
        row = {"C": C, "doubles": 2 * C + 1}
        for key, fn in (("all_gather_records", lambda: dist.all_gather_records(rec)),
                        ("collective", lambda: torch.distributed.all_gather_into_tensor(out, rec))):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            per = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                per.append((time.perf_counter() - t0) / a.iters * 1e6)
            row[key] = {"us_median": round(statistics.median(per), 2), "us_min": round(min(per), 2), "us_max": round(max(per), 2)}
        rows.append(row)
    if rank == 0:
        print("GATHER " + json.dumps({"backend": torch.distributed.get_backend(), "world": world, "rows": rows}), flush=True)
    dist.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=144)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--gather-rank", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join("profiles", "r29a_syncbn.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("syncbn_bench needs an MI355X: nothing is measured without one")
    if a.gather_rank:
        return gather_rank(a)
    lib = _lib.load()
    dev = "cuda"
    S = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cfgs = [CFGS[int(i)] for i in a.only.split(",")] if a.only else CFGS
    M = a.m
    rows_out = []
    for name, H, W, C1, C2, C, k, s, pad in cfgs:
        Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        rows = M * Ho * Wo
        xn, resn, gn = (torch.randn(M, Ho, Wo, C, device=dev) for _ in range(3))
        wd, bd = 1 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbytes = lib.omni_batchnorm_workspace_bytes(rows, C)
        assert nbytes > 0, (rows, C)
        ws = torch.empty(nbytes // 4, device=dev)
        y, dx, dres = torch.empty_like(xn), torch.empty_like(xn), torch.empty_like(xn)
        saved, dgamma, dbeta = torch.empty(2, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        rec, rec2 = torch.empty(1, 2 * C + 1, dtype=torch.float64, device=dev), torch.empty(1, 2 * C + 1, dtype=torch.float64, device=dev)

        def ok(rc):
            assert rc == 0, lib.omni_last_error()

        def fused_fwd():
            ok(lib.omni_batchnorm_fwd_f32(P(xn), P(resn), P(wd), P(bd), P(rm), P(rv), P(y), P(saved), rows, C, 1, 0.1, 1e-5, 1, P(ws), nbytes, S()))

        def split_fwd():
            ok(lib.omni_syncbn_stats_f32(P(xn), P(rec), rows, C, P(ws), nbytes, S()))
            ok(lib.omni_syncbn_fwd_apply_f32(P(xn), P(resn), P(wd), P(bd), P(rec), 1, P(rm), P(rv), P(y), P(saved), rows, C, 0.1, 1e-5, 1, S()))

        def fused_bwd():
            ok(lib.omni_batchnorm_bwd_f32(P(gn), P(xn), P(y), P(wd), P(saved), P(dx), P(dres), P(dgamma), P(dbeta), rows, C, 1, 1, P(ws), nbytes, S()))

        def split_bwd():
            ok(lib.omni_syncbn_bwd_reduce_f32(P(gn), P(xn), P(y), P(saved), P(dres), P(rec2), P(dgamma), P(dbeta), rows, C, 1, P(ws), nbytes, S()))
            ok(lib.omni_syncbn_bwd_apply_f32(P(dres), None, P(xn), P(wd), P(saved), P(rec2), 1, P(dx), None, rows, C, 1, S()))

        fns = {"fused_fwd": fused_fwd, "split_fwd": split_fwd, "fused_bwd": fused_bwd, "split_bwd": split_bwd}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {key: [] for key in fns}
        for _ in range(a.rounds):
            for key, fn in fns.items():
                t[key].append(window(fn, a.iters))
        med = {key: statistics.median(v) for key, v in t.items()}
        row = {"layer": name, "M": M, "H": Ho, "W": Wo, "C": C, "rows": rows, "MiB": round(rows * C * 4 / 2 ** 20, 2),
               "us": {key: round(v, 2) for key, v in med.items()},
               "us_range": {key: [round(min(v), 2), round(max(v), 2)] for key, v in t.items()},
               "split_over_fused_fwd": round(med["split_fwd"] / med["fused_fwd"], 3),
               "split_over_fused_bwd": round(med["split_bwd"] / med["fused_bwd"], 3)}
        rows_out.append(row)
        print("%-10s %7.1f MiB | fwd fused %8.2f us  split %8.2f us (%5.3fx) | bwd fused %8.2f us  split %8.2f us (%5.3fx)"
              % (name, row["MiB"], med["fused_fwd"], med["split_fwd"], row["split_over_fused_fwd"], med["fused_bwd"], med["split_bwd"],
                 row["split_over_fused_bwd"]), flush=True)
    gather = "not measured (--no-gather)"
    if not a.no_gather:
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
            env.pop(key, None)
        cmd = dist.launch_command(os.path.abspath(__file__), ["--gather-rank", "--iters", str(a.iters), "--rounds", str(a.rounds)], 1)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("GATHER ")]
        if r.returncode != 0 or not lines:
            raise SystemExit("the all_gather_records run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        gather = json.loads(lines[-1][len("GATHER "):])
        for g in gather["rows"]:
            print("one-rank %s group, %4d doubles: all_gather_records (identity) %7.2f us | all_gather_into_tensor %8.2f us (%.2f - %.2f)"
                  % (gather["backend"], g["doubles"], g["all_gather_records"]["us_median"], g["collective"]["us_median"],
                     g["collective"]["us_min"], g["collective"]["us_max"]))
    out = {"tool": "tools/syncbn_bench.py", "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "M": M,
           "iters": a.iters, "rounds": a.rounds,
           "timing": "device events around `iters` calls, the four forms interleaved per round, median and range of the rounds",
           "rows": rows_out, "all_gather_records": gather,
           "multi_gpu_training_step": "not measured" if torch.cuda.device_count() < 2 else "not measured by this tool"}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
