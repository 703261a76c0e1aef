"""GPU: batch normalisation with its backward (omnifusion_amd.ops.batch_norm / BatchNorm2d / convert, csrc/omni_batchnorm.hip) against
float64 torch autograd on the CPU,

    F.relu(F.batch_norm(x, running_mean, running_var, w, b, training, momentum, eps) + res)        against a random grad_out,

inputs randn, w = 1 + 0.1 randn, b = 0.1 randn, running buffers random (so that the (1 - momentum) term shows).  Every buffer the operator
allocates is filled with NaN first (ops._empty), so an element no kernel writes shows.  Device tensors are channels-last.

The gate comes from the reference side alone: for each case and each tensor kind, e32 = max|v32 - v64| / max(1, rms(v64)) of torch's OWN
float32 CPU evaluation of the same expression against the float64 one; the device result must satisfy err <= 8 . max(e32, 5e-7).  The factor
8 covers a different summation order and the fp32 rounding of the saved mean, the floor keeps a case where torch happens to be exact from
demanding exactness.  Every measured error is printed.

The ReLU cases: the operator masks with ITS forward's output, the reference with the float64 one, so the seeds are chosen, from the float64
reference alone, so that no pre-activation lies within ZMARGIN = 1e-5 of 0; `reference` asserts it.

Largest errors measured on an MI355X over all cases of this file (err / e32 of that case): see DESIGN.md §20."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 5e-7
ZMARGIN = 1e-5
CONV_GATE = 3e-5                                                                # tests/test_conv_bwd_gpu.py: the f16x3 products' gate
NAN = float("nan")

#        M   H    W    C   act    res
CASES = {
    "plain":      (2, 8, 8, 32, "none", False),
    "odd105":     (3, 5, 7, 32, "relu", True),          # 105 rows: a multiple of no slab
    "c4":         (2, 3, 3, 4, "relu", False),          # the narrowest channel count: 256 row lanes
    "c16":        (2, 4, 4, 16, "relu", False),         # mlp_points
    "c96":        (2, 4, 4, 96, "none", True),          # 24 quads in a column group of 32
    "rows18":     (18, 1, 1, 512, "none", False),       # fewer rows than channels, two column groups
    "rows2":      (2, 1, 1, 32, "none", False),         # n = 2, the smallest legal batch
    "rows10240":  (40, 16, 16, 32, "relu", True),       # many slabs, many partials
    "offset":     (4, 8, 8, 32, "none", False),         # x = randn . (c even ? 1 : 0.1) + 100 . (c mod 4)
    "rows131200": (5, 164, 160, 32, "none", False),     # 513 slabs: the finish kernels' threads take more than one partial
}
EXTRA = {"one": (1, 1, 1, 32, "relu", True)}            # rows == 1: eval mode only
# configurations: (training, momentum, eps, affine)
TRAIN, REF101, REF101_PLAIN, EVAL = (True, 0.1, 1e-5, True), (True, 0.99, 1e-6, True), (True, 0.99, 1e-6, False), (False, 0.1, 1e-5, True)
SEEDS = {("rows10240", TRAIN): 5}                       # (case, configuration) -> seed, where 0 leaves a pre-activation within ZMARGIN of 0
DEFAULT_SEED = 0
KINDS = ("x", "w", "b", "res")                          # the differentiable inputs
OUTS = ("y", "x", "w", "b", "res", "rm", "rv")          # what is compared: the output, the four gradients, the updated running buffers


def inputs(name, cfg=TRAIN):
    M, H, W, C, act, has_res = (CASES | EXTRA)[name]
    gen = torch.Generator().manual_seed(SEEDS.get((name, cfg), DEFAULT_SEED))
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    x = rn(M, C, H, W)
    if name == "offset":
        c = torch.arange(C)
        x = x * torch.where(c % 2 == 0, 1.0, 0.1).view(1, C, 1, 1) + (100.0 * (c % 4)).view(1, C, 1, 1)
    return {"x": x, "w": 1 + 0.1 * rn(C), "b": 0.1 * rn(C), "res": rn(M, C, H, W) if has_res else None, "g": rn(M, C, H, W),
            "rm": 0.5 * rn(C), "rv": 0.5 + torch.rand(C, generator=gen)}


def torch_cpu(d, act, cfg, dtype, g=None):
    """torch autograd on the CPU in `dtype` -> {z: the pre-activation, y, the gradients by kind, rm, rv: the buffers afterwards}"""
    training, momentum, eps, affine = cfg
    leaf = {k: (d[k].to(dtype, copy=True).requires_grad_(True) if d[k] is not None and (affine or k not in "wb") else None) for k in KINDS}
    rm, rv = d["rm"].to(dtype).clone(), d["rv"].to(dtype).clone()
    z = F.batch_norm(leaf["x"], rm, rv, leaf["w"], leaf["b"], training, momentum, eps)
    if leaf["res"] is not None:
        z = z + leaf["res"]
    y = F.relu(z) if act == "relu" else z
    y.backward((d["g"] if g is None else g).to(dtype))
    out = {k: (v.grad if v is not None else None) for k, v in leaf.items()}
    out.update(z=z.detach(), y=y.detach(), rm=rm, rv=rv)
    return out


def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


@functools.lru_cache(maxsize=None)
def reference(name, cfg=TRAIN):
    """(inputs, float64 results, {kind: the gate's right side})"""
    d = inputs(name, cfg)
    act = (CASES | EXTRA)[name][4]
    r64, r32 = torch_cpu(d, act, cfg, torch.float64), torch_cpu(d, act, cfg, torch.float32)
    if act == "relu":
        assert r64["z"].abs().min().item() >= ZMARGIN, f"{name} {cfg}: a float64 pre-activation within {ZMARGIN} of 0 (pick another seed)"
    gate = {k: FACTOR * max(nerr(r32[k], r64[k]), FLOOR) for k in OUTS if r64[k] is not None}
    return d, r64, gate


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def run(name, cfg=TRAIN, d=None, g=None, frozen=(), nchw=False):
    """ops.batch_norm + backward on the device -> {y, the gradients by kind, rm, rv}, on the CPU"""
    from omnifusion_amd import ops
    training, momentum, eps, affine = cfg
    act = (CASES | EXTRA)[name][4]
    d = d or reference(name, cfg)[0]
    g = d["g"] if g is None else g
    put = (lambda t: t.to(DEV).contiguous()) if nchw else cl
    leaf = {k: (None if d[k] is None or (k in "wb" and not affine) else (d[k].to(DEV) if k in "wb" else put(d[k])).requires_grad_(k not in frozen))
            for k in KINDS}
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    y = ops.batch_norm(leaf["x"], leaf["w"], leaf["b"], rm, rv, res=leaf["res"], training=training, momentum=momentum, eps=eps, act=act)
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[2] * y.shape[3] == 1
    if any(v is not None and v.requires_grad for v in leaf.values()):
        y.backward(put(g))
    out = {k: (v.grad.cpu().contiguous() if v is not None and v.grad is not None else None) for k, v in leaf.items()}
    out.update(y=y.detach().cpu().contiguous(), rm=rm.cpu(), rv=rv.cpu())
    return out


def check_gate(name, cfg, got, what=""):
    _, want, gate = reference(name, cfg)
    for k in OUTS:
        assert (got[k] is None) == (want[k] is None), (name, k)
        if want[k] is None:
            continue
        assert got[k].shape == want[k].shape and not torch.isnan(got[k]).any(), f"{name}{what}: NaN (an unwritten element) in {k}"
        e = nerr(got[k], want[k])
        print(f"batchnorm {name}{what} {'' if k in ('y', 'rm', 'rv') else 'd'}{k}: normalised error {e:.3e}  gate {gate[k]:.3e} (e32 {gate[k] / FACTOR:.3e})")
        assert e <= gate[k], f"{name}{what}: {k}: {e:.3e} > {gate[k]:.3e}"


def same_bits(a, b, kinds=OUTS):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in kinds)


def masked(name, cfg, g):
    """the residual's gradient: grad_out behind the float64 reference's ReLU mask"""
    _, want, _ = reference(name, cfg)
    return torch.where(want["z"] > 0, g, torch.zeros_like(g)) if (CASES | EXTRA)[name][4] == "relu" else g


@pytest.mark.parametrize("name", list(CASES))
def test_training_vs_float64_and_repeatable(name):
    d, want, _ = reference(name)
    got = run(name)
    check_gate(name, TRAIN, got)
    if d["res"] is not None:
        assert torch.equal(got["res"], masked(name, TRAIN, d["g"]))              # exact: a select
    n = d["x"].numel() // d["x"].shape[1]
    unbiased = 0.9 * d["rv"].double() + 0.1 * d["x"].double().var((0, 2, 3), unbiased=True)
    biased = 0.9 * d["rv"].double() + 0.1 * d["x"].double().var((0, 2, 3), unbiased=False)
    assert nerr(want["rv"], unbiased) < 1e-12                                   # (the reference's running_var IS the unbiased one)
    if n <= 128:                                                                # the two differ by var / n: visible against the gate at small n
        assert nerr(got["rv"], unbiased) < nerr(got["rv"], biased)
    assert same_bits(got, run(name)), f"{name}: two runs differ"


@pytest.mark.parametrize("cfg", [REF101, REF101_PLAIN], ids=["affine", "no_affine"])
@pytest.mark.parametrize("name", ["plain", "odd105"])
def test_reference_transformer_settings(name, cfg):
    """momentum = 0.99, eps = 1e-6 (the reference's transformer BatchNorm2d), with and without weight and bias"""
    got = run(name, cfg)
    check_gate(name, cfg, got, f" [momentum 0.99, eps 1e-6, affine {cfg[3]}]")
    if not cfg[3]:
        assert got["w"] is None and got["b"] is None


@pytest.mark.parametrize("name", ["plain", "odd105", "c16"])
def test_eval_mode(name):
    d, want, _ = reference(name, EVAL)
    got = run(name, EVAL)
    check_gate(name, EVAL, got, " [eval]")
    assert torch.equal(got["rm"], d["rm"]) and torch.equal(got["rv"], d["rv"])   # bit-unchanged
    dz = masked(name, EVAL, d["g"]).double()
    dx = (d["w"].double() / (d["rv"].double() + 1e-5).sqrt()).view(1, -1, 1, 1) * dz       # dx = gamma . invstd . dZ
    assert nerr(got["x"], dx) <= reference(name, EVAL)[2]["x"]
    if d["res"] is not None:
        assert torch.equal(got["res"], dz.float())


def test_only_requested_gradients(monkeypatch):
    from omnifusion_amd import ops
    for name, cfg in (("odd105", TRAIN), ("c96", TRAIN), ("odd105", EVAL)):
        full = run(name, cfg)
        no_x = run(name, cfg, frozen=("x",))
        assert no_x["x"] is None and same_bits(no_x, full, ("y", "w", "b", "res", "rm", "rv"))
        no_wb = run(name, cfg, frozen=("w", "b"))
        assert no_wb["w"] is None and no_wb["b"] is None and same_bits(no_wb, full, ("y", "x", "res", "rm", "rv"))
        no_res = run(name, cfg, frozen=("res",))
        assert no_res["res"] is None and same_bits(no_res, full, ("y", "x", "w", "b", "rm", "rv"))
        only_res = run(name, cfg, frozen=("x", "w", "b"))
        assert only_res["x"] is None and only_res["w"] is None and torch.equal(only_res["res"], full["res"])
    # eval mode with a frozen affine pair: no reduction pass.  The reduction pass is the only user of the workspace and the library rejects
    # a reduction without one, so a backward that asks for no workspace and succeeds has launched none.
    asked = []
    real = ops._bn_workspace
    monkeypatch.setattr(ops, "_bn_workspace", lambda *a: (asked.append(a[1:3]), real(*a))[1])
    full = run("odd105", EVAL)
    assert len(asked) == 1                                                      # the backward's; the eval-mode forward needs none
    del asked[:]
    got = run("odd105", EVAL, frozen=("w", "b"))
    assert asked == [] and same_bits(got, full, ("y", "x", "res"))
    got = run("odd105", TRAIN, frozen=("w", "b"))                              # training: the two sums are needed for dx whatever is frozen
    assert len(asked) == 2


def test_nan_stays_local():
    d, _, _ = reference("plain")
    x = d["x"].clone()
    x[1, 3, 2, 2] = NAN
    got = run("plain", d=dict(d, x=x))
    ch3 = torch.zeros(32, dtype=torch.bool)
    ch3[3] = True
    per_channel = lambda t: (torch.isnan(t).flatten(2).all(2).all(0), torch.isnan(t).flatten(2).any(2).any(0))
    for k in ("y", "x"):
        every, some = per_channel(got[k])
        assert torch.equal(every, ch3) and torch.equal(some, ch3), k             # channel 3, all of it, and nothing else
    assert torch.equal(torch.isnan(got["w"]), ch3) and not torch.isnan(got["b"]).any()
    assert torch.equal(torch.isnan(got["rm"]), ch3) and torch.equal(torch.isnan(got["rv"]), ch3)
    # a NaN in grad_out behind an inactive ReLU changes no gradient
    d, want, _ = reference("odd105")
    idx = (want["z"] < -0.1).nonzero()[0].tolist()
    g = d["g"].clone()
    g[tuple(idx)] = NAN
    assert same_bits(run("odd105", g=g), run("odd105"))


def test_one_value_per_channel():
    from omnifusion_amd import ops
    x = torch.randn(1, 32, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.batch_norm(x, training=True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.BatchNorm2d(32).to(DEV)(x)
    got = run("one", EVAL)
    check_gate("one", EVAL, got, " [eval]")


def test_nchw_input_gives_the_same_values():
    for name in ("odd105", "c96"):
        assert same_bits(run(name, nchw=True), run(name))


# ------------------------------------------------------------------------------------------------ a residual block on the device
BLOCK_SEED = 2                                          # the first whose float64 pre-activations and L1 differences all keep ZMARGIN from 0


class TorchBlock(torch.nn.Module):
    """conv -> BN -> ReLU -> conv -> BN -> + identity -> ReLU with torch's layers"""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
        self.conv2, self.bn2 = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)

    def forward(self, x):
        self.z1 = self.bn1(self.conv1(x))
        self.z2 = self.bn2(self.conv2(F.relu(self.z1))) + x
        return F.relu(self.z2)


class FusedBlock(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from omnifusion_amd import ops
        self.conv1, self.bn1 = ops.Conv2d(64, 64, 3, padding=1, bias=False), ops.BatchNorm2d(64, act="relu")
        self.conv2, self.bn2 = ops.Conv2d(64, 64, 3, padding=1, bias=False), ops.BatchNorm2d(64, act="relu")

    def forward(self, x):
        return self.bn2(self.conv2(self.bn1(self.conv1(x))), res=x)


def block_state(gen):
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    sd = {}
    for i in (1, 2):
        sd[f"conv{i}.weight"] = rn(64, 64, 3, 3) / 24.0                         # 1 / sqrt(9 . 64)
        sd[f"bn{i}.weight"], sd[f"bn{i}.bias"] = 1 + 0.1 * rn(64), 0.1 * rn(64)
        sd[f"bn{i}.running_mean"], sd[f"bn{i}.running_var"] = 0.5 * rn(64), 0.5 + torch.rand(64, generator=gen)
        sd[f"bn{i}.num_batches_tracked"] = torch.tensor(0)
    return sd


def block_step(block, x, target, lr=0.1):
    """forward, loss = sum |mean_c(out) - target|, backward, one SGD step -> (dx, {name: grad}), the block's state advanced"""
    x = x.clone().requires_grad_(True)
    opt = torch.optim.SGD(block.parameters(), lr=lr)
    diff = block(x).mean(1, keepdim=True) - target
    diff.abs().sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in block.named_parameters()}
    opt.step()
    return x.grad, grads, diff.detach()


def test_a_residual_block_trains_on_the_device():
    from omnifusion_amd import ops
    gen = torch.Generator().manual_seed(BLOCK_SEED)
    sd = block_state(gen)
    x, target = torch.randn(4, 64, 8, 8, generator=gen), torch.randn(4, 1, 8, 8, generator=gen)

    ref = TorchBlock().double()
    ref.load_state_dict(sd)
    dx64, g64, diff64 = block_step(ref, x.double(), target.double())
    assert min(ref.z1.abs().min().item(), ref.z2.abs().min().item(), diff64.abs().min().item()) >= ZMARGIN      # (module docstring)

    fused = FusedBlock()
    fused.load_state_dict(sd)
    converted, names = ops.convert(TorchBlock())
    assert names == ["conv1", "bn1", "conv2", "bn2"]
    converted.load_state_dict(sd)
    for what, block in (("fused", fused), ("converted", converted)):
        block.to(DEV)
        dx, grads, _ = block_step(block, cl(x), cl(target))
        got = dict(grads, x=dx)
        for k, want in dict(g64, x=dx64).items():
            assert not torch.isnan(got[k]).any(), (what, k)
            e = nerr(got[k].cpu(), want)
            print(f"batchnorm block [{what}] d{k}: normalised error {e:.3e}  (rms of the float64 gradient {want.pow(2).mean().sqrt().item():.3e})")
            assert e <= CONV_GATE, f"{what}: gradient of {k}: {e:.3e}"
        after, after64 = block.state_dict(), ref.state_dict()                   # one SGD step and one batch of statistics later
        for k, want in after64.items():
            if k.endswith("num_batches_tracked"):
                assert after[k].item() == want.item() == 1, (what, k)
            else:
                e = nerr(after[k].cpu(), want)
                print(f"batchnorm block [{what}] {k} after the step: normalised error {e:.3e}")
                assert e <= CONV_GATE, f"{what}: {k} after the step: {e:.3e}"


def test_graph_capture():
    """plain, forward + backward inside torch.cuda.graph: each replay equals an eager call on the same contents bit for bit, and the running
    buffers advance once per replay."""
    from omnifusion_amd import ops
    d, _, _ = reference("plain")
    gen = torch.Generator().manual_seed(77)
    w, b = d["w"].to(DEV).requires_grad_(True), d["b"].to(DEV).requires_grad_(True)
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    xs, gs = cl(d["x"]).requires_grad_(True), cl(d["g"])

    def step(x, g, rm, rv):
        y = ops.batch_norm(x, w, b, rm, rv, training=True, momentum=0.1, eps=1e-5, act="none")
        return (y,) + torch.autograd.grad(y, (x, w, b), g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(xs, gs, rm, rv)                                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    rm.copy_(d["rm"])
    rv.copy_(d["rv"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(xs, gs, rm, rv)
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), d["rm"]) and torch.equal(rv.cpu(), d["rv"])   # capturing runs nothing
    rm_e, rv_e = d["rm"].to(DEV), d["rv"].to(DEV)
    for i in range(2):
        x_new, g_new = torch.randn(d["x"].shape, generator=gen) + i, torch.randn(d["g"].shape, generator=gen)
        with torch.no_grad():
            xs.copy_(x_new)
            gs.copy_(g_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(cl(x_new).requires_grad_(True), cl(g_new), rm_e, rv_e)
        for got, want in zip(outs, eager):
            assert not torch.isnan(got).any() and torch.equal(got, want), f"replay {i}"
        assert torch.equal(rm, rm_e) and torch.equal(rv, rv_e), f"replay {i}: the running buffers"
    assert not torch.equal(rm.cpu(), d["rm"])
