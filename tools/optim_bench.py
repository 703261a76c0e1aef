"""The optimiser step on one MI355X (omnifusion_amd/optim.py, csrc/omni_optim.hip) over the single-pass model's 222 parameter
tensors (42 477 842 elements, make_state_dict(42, 18)), a gradient of every parameter present.

    python tools/optim_bench.py [--iters 10] [--repeats 7] [--train-iters 3] [--train-repeats 3] [--no-train] [--out profiles/r30a_optim.json]

Table 1, the step alone.  In ONE process and one run, the windows of all rows alternating (row A, row B, ..., row A, ...), each window
`iters` back-to-back steps between two device events after a warm-up; per row the median window with the smallest and the largest, and
`host_s`, the wall time the Python calls of a window took to ENQUEUE (no synchronisation inside).  Every row owns TWO independent sets of
parameters, gradients and state and alternates between them, so that a step never finds the arenas it needs in the 256-MiB memory-side
cache because the previous step of the same row left them there (one set is 680 MB: p, g, m, v).
    ours_pointers / ours_flat [_clip]          optim.AdamW in both gradient modes, without and with max_grad_norm=0.5
    torch_foreach / torch_fused [_clip]        torch.optim.AdamW(foreach=True | fused=True), without and with clip_grad_norm_(params, 0.5)
    graph_*                                    the same step replayed from a captured graph: ours in flat mode (pointer mode cannot be
                                               captured), torch's with capturable=True; a row whose capture fails records the error
    kernel_grad_sqnorm / _prepare / _apply     the three launches alone, through the C entry points
    floor_s                                    32 B per element (AdamW 28, the norm's second read of g 4) at 8 TB/s
Table 2, the whole training step (forward, backward, optimiser) at tools/train_bench.py's configuration (8 panoramas of 512 x 1024,
nrows 4): torch.optim.AdamW + clip_grad_norm_, and optim.AdamW(max_grad_norm=0.5) in each gradient mode; the windows alternate.  The
flat mode adds one in-place add per parameter to the backward where autograd otherwise adopts the gradient tensor; this table says what
that costs against what the step saves.
There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash; DESIGN §29 and the README quote them.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omnifusion_amd import _lib, build, optim  # noqa: E402
from omnifusion_amd.model import trainable  # noqa: E402
from omnifusion_amd.weights import make_state_dict  # noqa: E402

DEV = "cuda:0"
NROWS, N, P, H, W, FOV = 4, 18, 128, 512, 1024, (80, 80)
HBM = 8e12
ROTATE = 2
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def windows(fns, iters, repeats, warm=3):
    """fns: {row: callable}; the rows' windows alternate -> {row: median / min / max of the windows, host enqueue time}"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            host[k].append((time.perf_counter() - t0) / iters)
            torch.cuda.synchronize()
            dev[k].append(e0.elapsed_time(e1) / iters * 1e-3)
    return {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "windows_s": v, "host_s": statistics.median(host[k])}
            for k, v in dev.items()}


def rotating(steps):
    state = {"k": 0}

    def fn():
        steps[state["k"] % len(steps)]()
        state["k"] += 1
    return fn


_GRADS = []


def tensors(sd, gen):
    """one set: the model's parameter tensors with their shapes and a gradient of each (the same values in every set)"""
    params = [torch.nn.Parameter(v.clone().to(DEV)) for k, v in sd.items() if k.rsplit(".", 1)[-1] not in _BUFFERS]
    if not _GRADS:
        _GRADS.extend(1e-3 * torch.randn(p.shape, generator=gen) for p in params)
    return params, [g.to(DEV) for g in _GRADS]


def ours_set(sd, gen, flat, clip):
    params, grads = tensors(sd, gen)
    opt = optim.AdamW(params, flat_grads=flat, max_grad_norm=0.5 if clip else None, **HYPER)
    for p, g in zip(params, grads):
        if flat:
            p.grad.copy_(g)
        else:
            p.grad = g
    return opt, params


def torch_set(sd, gen, clip, **kw):
    params, grads = tensors(sd, gen)
    opt = torch.optim.AdamW(params, **HYPER, **kw)
    for p, g in zip(params, grads):
        p.grad = g

    def step():
        if clip:
            torch.nn.utils.clip_grad_norm_(params, 0.5, foreach=True)
        opt.step()
    return step, params


def captured(step):
    """warm up on a side stream, capture one step, return the replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    return graph.replay


def step_table(sd, a):
    gen = torch.Generator().manual_seed(0)
    fns, failed, keep = {}, {}, []
    for flat in (False, True):
        for clip in (False, True):
            sets = [ours_set(sd, gen, flat, clip) for _ in range(ROTATE)]
            keep.append(sets)
            name = f"ours_{'flat' if flat else 'pointers'}{'_clip' if clip else ''}"
            fns[name] = rotating([o.step for o, _ in sets])
            if flat:
                fns["graph_" + name] = rotating([captured(o.step) for o, _ in sets])
    for kind in ("foreach", "fused"):
        for clip in (False, True):
            sets = [torch_set(sd, gen, clip, **{kind: True}) for _ in range(ROTATE)]
            keep.append(sets)
            name = f"torch_{kind}{'_clip' if clip else ''}"
            fns[name] = rotating([s for s, _ in sets])
            try:
                csets = [torch_set(sd, gen, clip, capturable=True, **{kind: True}) for _ in range(ROTATE)]
                keep.append(csets)
                fns["graph_" + name] = rotating([captured(s) for s, _ in csets])
            except Exception as e:                                              # recorded, not hidden: the row says why it is missing
                failed["graph_" + name] = f"{type(e).__name__}: {e}"[:300]
    # the three launches alone
    L = _lib.load()
    sets = [ours_set(sd, gen, True, True)[0] for _ in range(ROTATE)]
    keep.append(sets)
    call = lambda fn, args: (lambda: _lib.check(fn(*args, None), "optim_bench"))
    fns["kernel_grad_sqnorm"] = rotating([call(L.omni_adamw_grad_sqnorm_f32, o._args_norm) for o in sets])
    fns["kernel_prepare"] = rotating([call(L.omni_adamw_prepare_f32, o._args_prep) for o in sets])
    fns["kernel_apply"] = rotating([call(L.omni_adamw_apply_f32, o._args_apply) for o in sets])
    rows = windows(fns, a.iters, a.repeats)
    for k, why in failed.items():
        rows[k] = {"failed": why}
    o = sets[0]
    return rows, {"tensors": len(o._params), "elements": sum(p.numel() for p in o._params), "arena_floats": o._total, "chunks": o._nchunk,
                  "tensors_below_4096": sum(p.numel() < 4096 for p in o._params)}


def train_table(sd, a):
    gen = torch.Generator().manual_seed(0)
    bs = a.bs
    rgb = torch.rand(bs, 3, H, W, generator=gen).to(DEV)
    g = torch.randn(bs, 1, H, W, generator=gen).to(DEV)

    def model():
        m = trainable.spherical_fusion(NROWS, N, (P, P), FOV)
        m.load_state_dict(sd)
        return m.to(DEV)

    def loop(net, opt, clip):
        def step():
            opt.zero_grad()
            (net(rgb, confidence=True) * g).sum().backward()
            if clip:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
            opt.step()
        return step

    fns = {}
    net = model()
    fns["train_torch_adamw_clip"] = loop(net, torch.optim.AdamW(net.parameters(), **HYPER), True)
    for flat in (False, True):
        net = model()
        fns[f"train_ours_{'flat' if flat else 'pointers'}_clip"] = loop(net, optim.AdamW(net.parameters(), flat_grads=flat, max_grad_norm=0.5, **HYPER), False)
    net = model()

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        (net(rgb, confidence=True) * g).sum().backward()
    fns["train_fwd_bwd_only"] = fwd_bwd
    return windows(fns, a.train_iters, a.train_repeats, warm=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--train-iters", type=int, default=3)
    ap.add_argument("--train-repeats", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30a_optim.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs an MI355X"
    sd = make_state_dict(42, N)
    rows, shape = step_table(sd, a)
    floor = shape["elements"] * 32 / HBM
    kernels = sum(rows[k]["median_s"] for k in ("kernel_grad_sqnorm", "kernel_prepare", "kernel_apply"))
    result = {"tool": "tools/optim_bench.py", "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(), "torch": torch.__version__,
              "iters": a.iters, "repeats": a.repeats, "rotating_sets": ROTATE, "timing": "device events; the windows of all rows alternate",
              **shape, "floor_s": floor, "kernels_s": kernels, "kernels_over_floor": kernels / floor, "rows": rows}
    med = lambda k: rows[k].get("median_s")
    result["torch_foreach_clip_over_ours_pointers_clip"] = med("torch_foreach_clip") / med("ours_pointers_clip")
    result["torch_fused_clip_over_ours_pointers_clip"] = med("torch_fused_clip") / med("ours_pointers_clip")
    if not a.no_train:
        torch.cuda.empty_cache()
        train = train_table(sd, a)
        result["train"] = {"panoramas": a.bs, "erp": [H, W], "nrows": NROWS, "iters": a.train_iters, "repeats": a.train_repeats, "rows": train}
        t = train["train_torch_adamw_clip"]["median_s"]
        result["train"]["ours_pointers_over_torch"] = train["train_ours_pointers_clip"]["median_s"] / t
        result["train"]["ours_flat_over_torch"] = train["train_ours_flat_clip"]["median_s"] / t
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
