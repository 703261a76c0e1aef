"""GPU: the backward of the convolution (omnifusion_amd.ops.conv2d, csrc/omni_conv_bwd.hip) against float64 torch autograd on the CPU,

    F.relu(F.conv2d(cat(x, x2), w, b, stride, padding) + res)        against a random grad_out,

inputs as in test_conv2d_vs_torch: randn, weights divided by sqrt(K).  Gate on every gradient (x, x2, weight, bias, res):
max|g - g64| <= 3e-5 * max(1, rms(g64)) — the forward's f16x3 gate of tests/test_model_gpu.py, normalised so that it means the same at unit
scale.  Every buffer the operator allocates is filled with NaN first (ops._empty), so an element no kernel writes shows.

The ReLU cases: the operator masks with ITS forward's output (fp32, off by up to 3.7e-6 from float64), the reference with the float64 one, so
an input whose float64 pre-activation lies within that error of 0 would compare two different masks.  The seeds below are chosen, from the
float64 reference alone, so that no pre-activation lies within ZMARGIN = 1e-5 of 0; `reference` asserts it."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 3e-5
ZMARGIN = 1e-5
NAN = float("nan")

#        M   H   W  C1  C2  Cout k  s  p  act    res
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
    "rows16641":  (1, 129, 129, 32, 0, 32, 3, 1, 1, "relu", True),   # 261 epilogue blocks of 64 rows: the finish kernel's threads 0 .. 4 add two partials
}
SEEDS = {"plain": 0, "odd105": 1, "s2even": 2, "s2odd": 3, "ds1x1": 4, "concat": 5, "c96_160": 6, "linear": 7, "rows10240": 448, "rows16641": 19}
KINDS = ("x", "x2", "w", "b", "res")


def inputs(name):
    M, H, W, C1, C2, Cout, k, s, p, act, has_res = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    d = {"x": rn(M, C1, H, W), "x2": rn(M, C2, H, W) if C2 else None, "w": rn(Cout, C1 + C2, k, k) / math.sqrt(k * k * (C1 + C2)),
         "b": rn(Cout), "res": rn(M, Cout, Ho, Wo) if has_res else None, "g": rn(M, Cout, Ho, Wo)}
    return d


def torch64(d, s, p, act, g):
    """float64 autograd on the CPU -> (pre-activation, {kind: gradient})"""
    leaf = {k: (v.double().requires_grad_(True) if v is not None else None) for k, v in d.items() if k in KINDS}
    xin = leaf["x"] if leaf["x2"] is None else torch.cat([leaf["x"], leaf["x2"]], 1)
    z = F.conv2d(xin, leaf["w"], leaf["b"], s, p)
    if leaf["res"] is not None:
        z = z + leaf["res"]
    y = F.relu(z) if act == "relu" else z
    y.backward(g.double())
    return z.detach(), {k: (v.grad if v is not None else None) for k, v in leaf.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    d = inputs(name)
    _, _, _, _, _, _, _, s, p, act, _ = CASES[name]
    z, grads = torch64(d, s, p, act, d["g"])
    if act == "relu":
        assert z.abs().min().item() >= ZMARGIN, f"{name}: a float64 pre-activation within {ZMARGIN} of 0 (pick another seed)"
    return d, z, grads


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def run(name, d=None, g=None, frozen=()):
    """ops.conv2d + backward on the device -> {kind: gradient on the CPU, NCHW}"""
    from omnifusion_amd import ops
    _, _, _, _, _, _, _, s, p, act, _ = CASES[name]
    d = d or reference(name)[0]
    g = d["g"] if g is None else g
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    leaf = {k: (None if d[k] is None else (d[k].to(DEV) if k == "b" else cl(d[k])).requires_grad_(k not in frozen)) for k in KINDS}
    y = ops.conv2d(leaf["x"], leaf["w"], leaf["b"], x2=leaf["x2"], res=leaf["res"], stride=s, padding=p, act=act)
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[2] * y.shape[3] == 1
    y.backward(cl(g))
    return {k: (v.grad.cpu().contiguous() if v is not None and v.grad is not None else None) for k, v in leaf.items()}


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
        print(f"conv_bwd {name}{what} d{k}: normalised error {e:.3e}")
        assert e <= GATE, f"{name}{what}: gradient of {k}: {e:.3e} > {GATE}"


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in KINDS)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_vs_float64_and_repeatable(name):
    want = reference(name)[2]
    got = run(name)
    check_gate(name, got, want)
    assert same_bits(got, run(name)), f"{name}: two runs differ"
    if name == "ds1x1":                                                       # stored zeros, not untouched memory
        dx = got["x"]
        assert (dx[:, :, 1::2, :] == 0).all() and (dx[:, :, :, 1::2] == 0).all() and (dx[:, :, ::2, ::2] != 0).any()


def test_forward_matches_float64():
    """The forward through ops.conv2d (weights split on the device) under the forward's own gate, 3e-5 absolute at unit scale."""
    from omnifusion_amd import ops
    for name in ("odd105", "concat", "ds1x1"):
        d, z, _ = reference(name)
        _, _, _, _, _, _, _, s, p, act, _ = CASES[name]
        f = lambda t: None if t is None else t.to(DEV)
        with torch.no_grad():
            y = ops.conv2d(f(d["x"]), f(d["w"]), f(d["b"]), x2=f(d["x2"]), res=f(d["res"]), stride=s, padding=p, act=act).cpu()
        want = F.relu(z) if act == "relu" else z
        e = (y.double() - want).abs().max().item()
        print(f"conv_bwd forward {name}: max error {e:.3e}")
        assert e <= GATE


def test_wgrad_chunk_length():
    """10 240 rows at the smallest legal chunk (32 rows: 320 chunks) and at the library's plan: both meet the gate, each is repeatable."""
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
    check_gate("rows10240", dflt, want, " [planned chunks]")
    assert same_bits(dflt, run("rows10240"))
    for k in ("x", "b", "res"):                                               # the chunk length reaches dW only
        assert torch.equal(small[k], dflt[k])


@pytest.mark.parametrize("name", ["plain", "s2even"])
@pytest.mark.parametrize("exp", [-30, 13])
def test_scaled_split(name, exp):
    """grad_out * 2^n gives every gradient * 2^n bit for bit: the gradient is scaled by a power of two of its own before it is split into
    halfs.  A backward that splits the raw gradient loses the 2^-30 run (hi = 0 everywhere, 11 bits or fewer in lo)."""
    d = reference(name)[0]
    base = run(name)
    f = 2.0 ** exp
    got = run(name, g=d["g"] * f)
    for k in KINDS:
        if base[k] is not None:
            assert torch.equal(got[k], base[k] * f), f"{name}: gradient of {k} at grad_out * 2^{exp}"


def test_nan_stays_local():
    """One NaN in grad_out behind an active ReLU (stride 2, 3x3): dX is NaN exactly where float64's is — a tap that does not apply is not
    read — and dW and the bias gradient exactly in the rows of that output channel."""
    name = "s2even"
    d, z, _ = reference(name)
    _, _, _, _, _, _, _, s, p, act, _ = CASES[name]
    m, co, oy, ox = 1, 5, 2, 3
    if z[m, co, oy, ox] < 0.1:                                                # an unambiguously active element of that pixel
        co = int((z[m, :, oy, ox] > 0.1).nonzero()[0])
    g = d["g"].clone()
    g[m, co, oy, ox] = NAN
    _, want = torch64(d, s, p, act, g)
    got = run(name, g=g)
    assert torch.equal(torch.isnan(got["x"]), torch.isnan(want["x"])) and 0 < torch.isnan(got["x"]).sum() < got["x"].numel()
    rows = torch.zeros(CASES[name][5], dtype=torch.bool)
    rows[co] = True
    assert torch.equal(torch.isnan(got["w"]).flatten(1).all(1), rows) and torch.equal(torch.isnan(got["w"]).flatten(1).any(1), rows)
    assert torch.equal(torch.isnan(got["b"]), rows)
    assert torch.equal(torch.isnan(want["w"]).flatten(1).all(1), rows)         # (the reference agrees)


def test_selective_backward():
    """Only what autograd asks for is computed, and what is computed has the bits of the full backward."""
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


def berhu64(pred, gt, mask, weights):
    """calculate_berhu_loss restated with torch operators (any dtype): the threshold is a constant of the backward"""
    bs = pred.shape[0]
    diff = gt - pred
    ad = diff.abs()
    c = (ad.max() / 5).detach()
    loss = torch.where(ad <= c, ad, (diff ** 2 + c ** 2) / (2 * c)).reshape(bs, -1)
    m, w = mask.reshape(bs, -1), weights.reshape(bs, -1)
    return ((loss * m * w).sum(1) / m.sum(1)).mean()


CHAIN_SEED = 11


def test_a_layer_can_be_fine_tuned():
    """conv (relu) -> conv with residual (relu) -> 1x1 conv -> channel mean -> BerHu loss -> backward(): every parameter gradient against the
    float64 torch chain, under the same gate."""
    from omnifusion_amd import ops
    from omnifusion_amd.supervision.direct import calculate_berhu_loss
    gen = torch.Generator().manual_seed(CHAIN_SEED)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    M, C, H, W = 2, 32, 8, 8
    x = rn(M, C, H, W)
    par = {"w1": rn(C, C, 3, 3) / math.sqrt(9 * C), "b1": rn(C), "w2": rn(C, C, 3, 3) / math.sqrt(9 * C), "b2": rn(C),
           "w3": rn(C, C, 1, 1) / math.sqrt(C), "b3": rn(C)}
    gt = rn(M, 1, H, W) + 2.0
    mask = (torch.rand(M, 1, H, W, generator=gen) < 0.8).float()
    weights = torch.rand(M, 1, H, W, generator=gen) + 0.5

    p64 = {k: v.double().requires_grad_(True) for k, v in par.items()}
    z1 = F.conv2d(x.double(), p64["w1"], p64["b1"], 1, 1)
    h1 = F.relu(z1)
    z2 = F.conv2d(h1, p64["w2"], p64["b2"], 1, 1) + h1
    h3 = F.conv2d(F.relu(z2), p64["w3"], p64["b3"])
    loss64 = berhu64(h3.mean(1, keepdim=True), gt.double(), mask.double(), weights.double())
    loss64.backward()
    assert min(z1.abs().min().item(), z2.abs().min().item()) >= ZMARGIN       # (module docstring)

    pg = {k: v.to(DEV).requires_grad_(True) for k, v in par.items()}
    a1 = ops.conv2d(x.to(DEV), pg["w1"], pg["b1"], padding=1, act="relu")
    a2 = ops.conv2d(a1, pg["w2"], pg["b2"], res=a1, padding=1, act="relu")
    a3 = ops.conv2d(a2, pg["w3"], pg["b3"])
    loss = calculate_berhu_loss(a3.mean(1, keepdim=True), gt.to(DEV), mask.to(DEV), weights.to(DEV))
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= GATE * max(1.0, abs(loss64.item()))
    for k in par:
        got, want = pg[k].grad.cpu(), p64[k].grad
        assert got.shape == want.shape and not torch.isnan(got).any()
        e = nerr(got, want)
        print(f"conv_bwd chain d{k}: normalised error {e:.3e}  (rms of the float64 gradient {want.pow(2).mean().sqrt().item():.3e})")
        assert e <= GATE, f"chain: gradient of {k}: {e:.3e}"
