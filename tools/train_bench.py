"""One training step of the trainable spherical_fusion (omnifusion_amd/model/trainable.py) on one MI355X, at 8 panoramas of
512 x 1024, nrows 4 (M = 144 patches of 128 x 128), random weights make_state_dict(42, 18).

    python tools/train_bench.py [--bs 8] [--iters 5] [--repeats 3] [--precision f16x3|f16x1|both] [--out profiles/r21a_train_step.json]

In ONE process and one run, each row timed with device events around `iters` back-to-back calls after a warm-up of the same calls; the
median of `repeats` windows with the smallest and the largest beside it:
    train_fwd_bwd        net(rgb) -> sum(depth . g) -> backward, the trainable model in training mode
    torch_fwd_bwd        the same network from torch's own operators (tests/_train_model_ref.py: F.conv2d, F.batch_norm, ...) in float32 on
                         channels-last tensors on the same GPU, blended by the differentiable pers2equi and a torch division
    inference_fwd        the inference spherical_fusion (f16x3) forward under no_grad
    heads_fwd            omni_depth_heads_fwd_f32 alone (p and q written), on buffers allocated once
    heads_bwd_data       omni_depth_heads_bwd_f32 with dx only: the planar pre-pass and the data-gradient kernel
    heads_bwd_weight     the same with dw and dbias only: the pre-pass, the weight-gradient kernel and its finish
    torch_heads_fwd / torch_heads_fwd_bwd    F.conv2d at Cout = 2 (+ ReLU, sigmoid, product) and its autograd, channels-last
    torch_pieces         the pieces of the trainable model that torch operators run, fwd + bwd, at their shapes: mlp_points, layer1 +
                         point_feat, the token reshape and layer4 + tokens; `torch_pieces_share` is their sum over train_fwd_bwd
    floor                302 MB (the [144,128,128,32] tensor once) at 8 TB/s per heads kernel
    peak_memory          torch.cuda.max_memory_allocated over one training step of either model
--precision f16x1 builds the trainable model with precision="f16x1" (DESIGN.md §27).  --precision both times ONLY the training step, of
two models that differ in the mode alone, with the windows alternating f16x3, f16x1, f16x3, ... in one process: per mode the median, the
smallest and the largest window and the peak memory, their ratio, and whether the f16x1 median lies below the smallest f16x3 window.
There is no GPU -> the tool fails; it never falls back.  Writes the rows with the library's source hash; DESIGN §23 and the README quote them.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _train_model_ref as ref  # noqa: E402
from omnifusion_amd import _lib, build  # noqa: E402
from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches  # noqa: E402
from omnifusion_amd.equi_pers.pers2equi_v3 import pers2equi  # noqa: E402
from omnifusion_amd.model import trainable  # noqa: E402
from omnifusion_amd.model.spherical_model import spherical_fusion as inference_fusion  # noqa: E402
from omnifusion_amd.weights import make_state_dict  # noqa: E402

DEV = "cuda:0"
NROWS, N, P, H, W, FOV = 4, 18, 128, 512, 1024, (80, 80)
HBM = 8e12
_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
PTR = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
cl = lambda t: t.contiguous(memory_format=torch.channels_last)


def timed(fn, iters, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e-3)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}


def timed_interleaved(fns, iters, repeats, warm=2):
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1) / iters * 1e-3)
    return [{"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "windows_s": v} for v in out]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="f16x3", choices=("f16x3", "f16x1", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21a_train_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench needs an MI355X"
    bs, M = a.bs, a.bs * N
    gen = torch.Generator().manual_seed(0)
    rgb = torch.rand(bs, 3, H, W, generator=gen).to(DEV)
    g = torch.randn(bs, 1, H, W, generator=gen).to(DEV)
    sd = make_state_dict(42, N)
    rows = {}

    def model(precision):
        m = trainable.spherical_fusion(NROWS, N, (P, P), FOV, precision=precision)
        m.load_state_dict(sd)
        return m.to(DEV)

    def step_of(m):
        def step():
            for p in m.parameters():
                p.grad = None
            (m(rgb, confidence=True) * g).sum().backward()
        return step

    if a.precision == "both":
        modes = ("f16x3", "f16x1")
        steps = [step_of(model(m)) for m in modes]
        for m, t, st in zip(modes, timed_interleaved(steps, a.iters, a.repeats), steps):
            rows["train_fwd_bwd_" + m] = t
            t["peak_memory_bytes"] = peak(st)
        r3, r1 = rows["train_fwd_bwd_f16x3"], rows["train_fwd_bwd_f16x1"]
        result = {"tool": "tools/train_bench.py", "precision": "both", "device": torch.cuda.get_device_name(0),
                  "source_hash": build.source_hash(), "panoramas": bs, "erp": [H, W], "nrows": NROWS, "patches": M, "iters": a.iters,
                  "repeats": a.repeats, "timing": "device events; the windows of the two modes alternate", "rows": rows,
                  "f16x1_over_f16x3": r1["median_s"] / r3["median_s"],
                  "f16x1_median_below_f16x3_min": r1["median_s"] < r3["min_s"],
                  "peak_memory_f16x1_over_f16x3": r1["peak_memory_bytes"] / r3["peak_memory_bytes"]}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return

    net = model(a.precision)
    train_step = step_of(net)
    rows["train_fwd_bwd"] = timed(train_step, a.iters, a.repeats)
    rows["train_fwd_bwd"]["peak_memory_bytes"] = peak(train_step)

    # the same network from torch's own operators, float32, channels-last
    tsd = {k: v.to(DEV) for k, v in sd.items()}
    names = [k for k in tsd if k.rsplit(".", 1)[-1] not in _BUFFERS]
    for k in names:
        tsd[k].requires_grad_(True)
    pin = net.point_input(DEV)

    def torch_step():
        for k in names:
            tsd[k].grad = None
        patches = cl(equi2pers_patches(rgb, FOV, NROWS, (P, P), layout=_lib.LAYOUT_BNCHW).reshape(M, 3, P, P))
        pf = ref.mlp_points(tsd, pin, True)
        pred, weight = ref.network(tsd, patches, pf, bs, N, True)
        av, cv = (pred * weight).reshape(bs, N, 1, P, P), weight.reshape(bs, N, 1, P, P)
        A = pers2equi(av, FOV, NROWS, (P, P), (H, W), None, _lib.LAYOUT_BNCHW)
        C = pers2equi(cv, FOV, NROWS, (P, P), (H, W), None, _lib.LAYOUT_BNCHW)
        ((A / (C + 1e-8 * (C <= 1e-8).float())) * g).sum().backward()
    rows["torch_fwd_bwd"] = timed(torch_step, a.iters, a.repeats)
    rows["torch_fwd_bwd"]["peak_memory_bytes"] = peak(torch_step)
    for k in names:
        tsd[k].grad = None

    inf = inference_fusion(NROWS, N, (P, P), FOV, precision="f16x3")
    inf.load_state_dict(sd)
    inf = inf.to(DEV).eval()
    with torch.no_grad():
        rows["inference_fwd"] = timed(lambda: inf(rgb, confidence=True), 4 * a.iters, a.repeats)

    # the heads alone
    lib = _lib.load()
    st = None
    x = torch.randn(M, P, P, 32, device=DEV)
    w = torch.randn(2, 9, 32, device=DEV) / 17.0
    bias = torch.tensor([1.0, 0.0], device=DEV)
    planes = [torch.empty(M, P, P, device=DEV) for _ in range(4)]
    ga, gc = torch.randn(M, P, P, device=DEV), torch.randn(M, P, P, device=DEV)
    dx, dw, db = torch.empty_like(x), torch.empty(2, 9, 32, device=DEV), torch.empty(2, device=DEV)
    nb = lib.omni_depth_heads_bwd_workspace_bytes(M, P, P)
    ws = torch.empty(nb // 4, device=DEV)
    ok = lambda rc: _lib.check(rc, "heads")
    fwd = lambda: ok(lib.omni_depth_heads_fwd_f32(PTR(x), PTR(w), PTR(bias), *(PTR(t) for t in planes), M, P, P, 1, st))
    bwd = lambda dx_, dw_, db_: ok(lib.omni_depth_heads_bwd_f32(PTR(ga), PTR(gc), PTR(planes[2]), PTR(planes[3]), PTR(x), PTR(w), PTR(dx_), PTR(dw_),
                                                                PTR(db_), M, P, P, 1, PTR(ws), nb, st))
    hi = 20 * a.iters
    rows["heads_fwd"] = timed(fwd, hi, a.repeats)
    rows["heads_bwd_data"] = timed(lambda: bwd(dx, None, None), hi, a.repeats)
    rows["heads_bwd_weight"] = timed(lambda: bwd(None, dw, db), hi, a.repeats)
    rows["heads_bwd_all"] = timed(lambda: bwd(dx, dw, db), hi, a.repeats)
    xt = x.permute(0, 3, 1, 2).requires_grad_(True)                            # channels-last [M,32,P,P]
    wt = w.reshape(2, 3, 3, 32).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bt = bias.clone().requires_grad_(True)
    g2 = torch.randn(M, 2, P, P, device=DEV)

    def torch_heads(backward):
        y = F.conv2d(xt, wt, bt, padding=1)
        s = torch.sigmoid(y[:, 1:])
        out = torch.cat([F.relu(y[:, :1]) * s, s], 1)
        if backward:
            torch.autograd.grad(out, [xt, wt, bt], g2)
    with torch.no_grad():
        rows["torch_heads_fwd"] = timed(lambda: torch_heads(False), hi, a.repeats)
    rows["torch_heads_fwd_bwd"] = timed(lambda: torch_heads(True), hi, a.repeats)
    del x, xt, dx, planes, ga, gc, ws, g2

    # the pieces of the trainable model that torch operators run, forward + backward, at their shapes
    l1 = cl(torch.randn(M, 64, P // 4, P // 4, device=DEV)).requires_grad_(True)
    l4 = cl(torch.randn(M, 512, P // 32, P // 32, device=DEV)).requires_grad_(True)
    d4 = cl(torch.randn(M, 32, P // 32, P // 32, device=DEV)).requires_grad_(True)
    tk = torch.randn(bs, N, 512, device=DEV, requires_grad=True)

    def pieces():
        pf = cl(net.mlp_points(pin))
        y1 = (l1.reshape(bs, N, 64, P // 4, P // 4) + pf[None]).reshape(l1.shape)
        t = d4.reshape(bs, N, 512)
        y4 = l4 + tk.reshape(M, 512, 1, 1)
        torch.autograd.grad([y1, t, y4], [l1, d4, l4, tk] + [p for p in net.mlp_points.parameters()],
                            [torch.ones_like(y1), torch.ones_like(t), torch.ones_like(y4)])
    rows["torch_pieces"] = timed(pieces, hi, a.repeats)

    floor = M * P * P * 32 * 4 / HBM
    result = {
        "tool": "tools/train_bench.py", "precision": a.precision, "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash(),
        "panoramas": bs, "erp": [H, W], "nrows": NROWS, "patches": M, "iters": a.iters, "repeats": a.repeats,
        "rows": rows, "heads_floor_s": floor,
        "train_over_torch": rows["train_fwd_bwd"]["median_s"] / rows["torch_fwd_bwd"]["median_s"],
        "train_over_inference": rows["train_fwd_bwd"]["median_s"] / rows["inference_fwd"]["median_s"],
        "heads_over_floor": {k: rows[k]["median_s"] / floor for k in ("heads_fwd", "heads_bwd_data", "heads_bwd_weight")},
        "torch_pieces_share": rows["torch_pieces"]["median_s"] / rows["train_fwd_bwd"]["median_s"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
