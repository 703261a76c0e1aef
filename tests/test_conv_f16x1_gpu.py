"""GPU: ops.conv2d(..., precision="f16x1") — one fp16 matrix instruction per product block, forward, data gradient and weight gradient
(csrc/omni_conv.hip, csrc/omni_conv_bwd.hip).  Every buffer the operator allocates is filled with NaN first.

1. Exact integers: every input an integer in [-3, 3], so every product and partial sum is exact in fp16 x fp16 -> fp32 (K <= 9 . 160,
   |dZ . 2^7| <= 384, sums < 2^24): the output and all gradients are torch.equal to float64 autograd, and to the f16x3 run.  No tolerance:
   indexing, taps, parities, the two sources, chunking and the scale.
2. The rounding model (tests/_conv_f16x1_ref.py) on random inputs: float64 sums over hi16 operands, for the backward hi16(dZ 2^s) 2^-s.
   Two halfs multiply exactly in fp32, so what remains is fp32 accumulation: the gate is the project's CONV_GATE, 3e-5 . max(1, rms).
   Each case also asserts that the UNROUNDED float64 result lies outside that gate for everything that is a sum of products (the output,
   dX, dX2, dW) — otherwise it could not tell f16x1 from f16x3 — and prints that distance.
   ReLU masks: the operator masks with its own output, the model with the float64 pre-activation; `reference` asserts that no model
   pre-activation behind a ReLU lies within ZMARGIN = 1e-4 of 0.  For the cases without a residual the seed is chosen so (from the CPU
   model alone); 327 680 random pre-activations (rows10240) cannot all miss that band for any seed, so where the case has a residual,
   `inputs` moves the residual of the few elements inside twice the band by 1/64, which takes them out of it.
3. grad_out . 2^-30 and . 2^13 give every gradient . 2^n bit for bit.
4. A NaN in grad_out, and one in x, reach exactly the float64 reference's elements.
5. A frozen input or weight is not computed and the others keep their bits; two runs give equal bits; conv_wgrad_rows = 32 stays within
   the gate and repeatable; one capture-and-replay of forward + backward equals eager bit for bit.
6. An omitted keyword and precision="f16x3" give the same bits.

Distances of the f16x1 results from the unrounded float64, measured on an MI355X: DESIGN.md §27."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _conv_f16x1_ref as r16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 3e-5                                                                     # CONV_GATE
ZMARGIN = 1e-4
NAN = float("nan")

#        M   H   W  C1  C2  Cout k  s  p  act    res          (the small shapes of test_conv_bwd_gpu.py)
CASES = {
    "plain":      (2, 8, 8, 32, 0, 32, 3, 1, 1, "none", False),
    "odd105":     (3, 5, 7, 32, 0, 64, 3, 1, 1, "relu", True),       # 105 rows: not a multiple of any tile
    "s2even":     (2, 8, 8, 64, 0, 32, 3, 2, 1, "relu", False),
    "s2odd":      (2, 7, 9, 32, 0, 32, 3, 2, 1, "none", False),      # Ho x Wo = 4 x 5
    "ds1x1":      (2, 8, 8, 32, 0, 64, 1, 2, 0, "none", False),      # the down-sample branch: three quarters of dX are zeros
    "concat":     (2, 6, 6, 32, 96, 64, 3, 1, 1, "relu", False),     # unequal halves, two gradient tensors
    "c96_160":    (2, 4, 4, 96, 0, 160, 3, 1, 1, "none", False),     # multiples of 32 but not of 64
    "linear":     (18, 1, 1, 512, 0, 2048, 1, 1, 0, "none", False),  # fewer rows than one MFMA tile
    "rows10240":  (40, 16, 16, 32, 0, 32, 3, 1, 1, "relu", True),    # many wgrad chunks, many blocks
    # two more, for the forward's halo-tile kernel (3x3, stride 1, W % 32 == 0, H % 4 == 0), which none of the shapes above reaches
    "halo64":     (2, 8, 32, 32, 32, 64, 3, 1, 1, "relu", True),     # 64-channel column tiles, two sources
    "halo96":     (1, 4, 64, 64, 0, 96, 3, 1, 1, "none", False),     # 32-channel column tiles: the weight loader's last pass is partial
}
SEEDS = {"plain": 0, "odd105": 1, "s2even": 2, "s2odd": 3, "ds1x1": 4, "concat": 5, "c96_160": 6, "linear": 7, "rows10240": 8, "halo64": 9,
         "halo96": 10}
KINDS = ("x", "x2", "w", "b", "res")
PRODUCTS = ("x", "x2", "w")                                                     # the gradients that are sums of rounded products


def conf(name):
    _, _, _, _, _, _, _, s, p, act, _ = CASES[name]
    return s, p, act


def shapes(name):
    M, H, W, C1, C2, Cout, k, s, p, act, has_res = CASES[name]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return {"x": (M, C1, H, W), "x2": (M, C2, H, W) if C2 else None, "w": (Cout, C1 + C2, k, k), "b": (Cout,),
            "res": (M, Cout, Ho, Wo) if has_res else None, "g": (M, Cout, Ho, Wo)}


@functools.lru_cache(maxsize=None)
def inputs(name):
    s, p, act = conf(name)
    gen = torch.Generator().manual_seed(SEEDS[name])
    sh = shapes(name)
    d = {k: (torch.randn(*v, generator=gen) if v is not None else None) for k, v in sh.items()}
    d["w"] = d["w"] / math.sqrt(sh["w"][1] * sh["w"][2] * sh["w"][3])
    if act == "relu" and d["res"] is not None:                                 # (module docstring, 2)
        z, _ = r16.model64(d, s, p, act, d["g"])
        d["res"] = torch.where(z.abs() < 2 * ZMARGIN, d["res"] + 1.0 / 64, d["res"])
    return d


@functools.lru_cache(maxsize=None)
def int_inputs(name):
    gen = torch.Generator().manual_seed(100 + SEEDS[name])
    return {k: (torch.randint(-3, 4, v, generator=gen).float() if v is not None else None) for k, v in shapes(name).items()}


def torch64(d, s, p, act, g):
    """unrounded float64 autograd on the CPU -> (output, pre-activation, {kind: gradient})"""
    leaf = {k: (v.double().requires_grad_(True) if v is not None else None) for k, v in d.items() if k in KINDS}
    xin = leaf["x"] if leaf["x2"] is None else torch.cat([leaf["x"], leaf["x2"]], 1)
    z = F.conv2d(xin, leaf["w"], leaf["b"], s, p)
    if leaf["res"] is not None:
        z = z + leaf["res"]
    y = F.relu(z) if act == "relu" else z
    y.backward(g.double())
    return y.detach(), z.detach(), {k: (v.grad if v is not None else None) for k, v in leaf.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (inputs, the model's pre-activation and gradients, the unrounded float64 output and gradients)"""
    d = inputs(name)
    s, p, act = conf(name)
    z, grads = r16.model64(d, s, p, act, d["g"])
    if act == "relu":
        assert z.abs().min().item() >= ZMARGIN, f"{name}: a model pre-activation within {ZMARGIN} of 0 behind a ReLU (pick another seed)"
    y64, _, g64 = torch64(d, s, p, act, d["g"])
    return d, z, grads, y64, g64


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def leaves(d, frozen=()):
    return {k: (None if d[k] is None else (d[k].to(DEV) if k == "b" else cl(d[k])).requires_grad_(k not in frozen)) for k in KINDS}


def run(name, d=None, g=None, frozen=(), **kw):
    """ops.conv2d + backward on the device -> {kind: gradient on the CPU, NCHW; "y": the output}; kw: precision (default "f16x1")"""
    from omnifusion_amd import ops
    s, p, act = conf(name)
    d = d or reference(name)[0]
    g = d["g"] if g is None else g
    kw = kw if "default" in kw else {"precision": "f16x1", **kw}
    kw.pop("default", None)
    leaf = leaves(d, frozen)
    y = ops.conv2d(leaf["x"], leaf["w"], leaf["b"], x2=leaf["x2"], res=leaf["res"], stride=s, padding=p, act=act, **kw)
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[2] * y.shape[3] == 1
    y.backward(cl(g))
    out = {k: (v.grad.cpu().contiguous() if v is not None and v.grad is not None else None) for k, v in leaf.items()}
    out["y"] = y.detach().cpu().contiguous()
    return out


def nerr(got, want):
    """the gate's left side over its right side without the 3e-5: max|g - g64| / max(1, rms(g64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def check_gate(name, got, want, what=""):
    for k in KINDS:
        assert (got[k] is None) == (want[k] is None), (name, k)
        if want[k] is None:
            continue
        assert got[k].shape == want[k].shape and not torch.isnan(got[k]).any(), f"{name}{what}: NaN (an unwritten element) in the gradient of {k}"
        e = nerr(got[k], want[k])
        print(f"conv_f16x1 {name}{what} d{k}: normalised error against the rounding model {e:.3e}")
        assert e <= GATE, f"{name}{what}: gradient of {k}: {e:.3e} > {GATE}"


def same_bits(a, b, keys=KINDS + ("y",)):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("name", list(CASES))
def test_exact_integers(name):
    d = int_inputs(name)
    s, p, act = conf(name)
    y64, _, g64 = torch64(d, s, p, act, d["g"])
    got, x3 = run(name, d=d), run(name, d=d, precision="f16x3")
    assert torch.equal(got["y"].double(), y64), f"{name}: output"
    for k in KINDS:
        assert (got[k] is None) == (g64[k] is None), (name, k)
        if g64[k] is not None:
            assert torch.equal(got[k].double(), g64[k]), f"{name}: gradient of {k} is not the exact integer result"
    assert same_bits(got, x3), f"{name}: f16x1 and f16x3 differ on exact integers"
    if name == "ds1x1":                                                       # stored zeros, not untouched memory
        dx = got["x"]
        assert (dx[:, :, 1::2, :] == 0).all() and (dx[:, :, :, 1::2] == 0).all() and (dx[:, :, ::2, ::2] != 0).any()


@pytest.mark.parametrize("name", list(CASES))
def test_rounding_model_and_repeatable(name):
    d, z, want, y64, g64 = reference(name)
    got = run(name)
    ywant = F.relu(z) if conf(name)[2] == "relu" else z
    e = nerr(got["y"], ywant)
    print(f"conv_f16x1 {name} output: normalised error against the rounding model {e:.3e}")
    assert not torch.isnan(got["y"]).any() and e <= GATE, f"{name}: output {e:.3e} > {GATE}"
    check_gate(name, got, want)
    far = {"y": nerr(got["y"], y64)}
    far.update({k: nerr(got[k], g64[k]) for k in PRODUCTS if g64[k] is not None})
    print(f"conv_f16x1 {name}: distance to the UNROUNDED float64: " + "  ".join(f"{k} {v:.3e}" for k, v in far.items()))
    for k, v in far.items():
        assert v > GATE, f"{name}: {k} lies within the gate of the unrounded result ({v:.3e}): the case cannot tell the modes apart"
    assert same_bits(got, run(name)), f"{name}: two runs differ"


@pytest.mark.parametrize("name", ["plain", "s2even"])
@pytest.mark.parametrize("exp", [-30, 13])
def test_scaling(name, exp):
    d = reference(name)[0]
    base = run(name)
    f = 2.0 ** exp
    got = run(name, g=d["g"] * f)
    for k in KINDS:
        if base[k] is not None:
            assert torch.equal(got[k], base[k] * f), f"{name}: gradient of {k} at grad_out * 2^{exp}"


def test_nan_in_grad_out_stays_local():
    """One NaN in grad_out behind an active ReLU (stride 2, 3x3): dX is NaN exactly where float64's is — a tap that does not apply is not
    read — and dW and the bias gradient exactly in the rows of that output channel."""
    name = "s2even"
    d, z = reference(name)[:2]
    s, p, act = conf(name)
    m, oy, ox = 1, 2, 3
    co = int((z[m, :, oy, ox] > 0.1).nonzero()[0])                             # an unambiguously active element of that pixel
    g = d["g"].clone()
    g[m, co, oy, ox] = NAN
    _, _, want = torch64(d, s, p, act, g)
    got = run(name, g=g)
    assert torch.equal(torch.isnan(got["x"]), torch.isnan(want["x"])) and 0 < torch.isnan(got["x"]).sum() < got["x"].numel()
    assert torch.equal(torch.isnan(got["w"]), torch.isnan(want["w"])) and torch.equal(torch.isnan(got["b"]), torch.isnan(want["b"]))
    rows = torch.zeros(CASES[name][5], dtype=torch.bool)
    rows[co] = True
    assert torch.equal(torch.isnan(got["w"]).flatten(1).all(1), rows) and torch.equal(torch.isnan(got["b"]), rows)
    assert not torch.isnan(got["y"]).any()


def test_nan_in_x_stays_local():
    """One NaN in x (stride 2, odd sizes, no activation): the output and dW are NaN exactly where float64's are — the taps that reach that
    pixel, in that input channel — and dX, which does not depend on x, nowhere."""
    name = "s2odd"
    d = reference(name)[0]
    s, p, act = conf(name)
    x = d["x"].clone()
    x[1, 7, 3, 4] = NAN
    dn = dict(d, x=x)
    y64, _, want = torch64(dn, s, p, act, d["g"])
    got = run(name, d=dn)
    assert torch.equal(torch.isnan(got["y"]), torch.isnan(y64)) and 0 < torch.isnan(got["y"]).sum() < got["y"].numel()
    assert torch.equal(torch.isnan(got["w"]), torch.isnan(want["w"])) and 0 < torch.isnan(got["w"]).sum() < got["w"].numel()
    assert torch.isnan(got["w"]).sum(0).flatten().count_nonzero() == torch.isnan(got["w"])[0].sum()      # the same taps for every output channel
    assert not torch.isnan(got["x"]).any() and not torch.isnan(want["x"]).any() and not torch.isnan(got["b"]).any()


def test_selective_backward():
    for name in ("plain", "concat"):
        full = run(name)
        no_x = run(name, frozen=("x", "x2"))
        assert no_x["x"] is None and no_x["x2"] is None and torch.equal(no_x["w"], full["w"]) and torch.equal(no_x["b"], full["b"])
        no_w = run(name, frozen=("w", "b"))
        assert no_w["w"] is None and no_w["b"] is None and torch.equal(no_w["x"], full["x"])
        if full["x2"] is not None:
            assert torch.equal(no_w["x2"], full["x2"])
            only_x2 = run(name, frozen=("x", "w", "b"))
            assert only_x2["x"] is None and torch.equal(only_x2["x2"], full["x2"])


def test_wgrad_chunk_length():
    """10 240 rows at the smallest legal chunk (32 rows: 320 chunks): within the gate, repeatable, and only dW differs from the plan's"""
    from omnifusion_amd import _lib
    want = reference("rows10240")[2]
    assert _lib.get_option("conv_wgrad_rows") == 0
    try:
        _lib.set_option("conv_wgrad_rows", 32)
        small = run("rows10240")
        check_gate("rows10240", small, want, " [32-row chunks]")
        assert same_bits(small, run("rows10240"))
    finally:
        _lib.set_option("conv_wgrad_rows", 0)
    dflt = run("rows10240")
    for k in ("x", "b", "res", "y"):
        assert torch.equal(small[k], dflt[k])


def test_capture_and_replay_equals_eager():
    from omnifusion_amd import ops
    name = "odd105"
    d = reference(name)[0]
    s, p, act = conf(name)
    eager = run(name)
    leaf = leaves(d)
    g = cl(d["g"])
    live = [k for k in KINDS if leaf[k] is not None]

    def step():
        y = ops.conv2d(leaf["x"], leaf["w"], leaf["b"], x2=leaf["x2"], res=leaf["res"], stride=s, padding=p, act=act, precision="f16x1")
        return (y.detach(),) + torch.autograd.grad(y, [leaf[k] for k in live], g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                 # warm-up: allocator pools
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for k, t in zip(["y"] + live, outs):
        assert torch.equal(t.cpu().contiguous(), eager[k]), k


def test_default_is_f16x3():
    for name in ("odd105", "concat"):
        assert same_bits(run(name, default=True), run(name, precision="f16x3")), name
        assert not same_bits(run(name, precision="f16x1"), run(name, precision="f16x3"), keys=("y", "x", "w")), name
