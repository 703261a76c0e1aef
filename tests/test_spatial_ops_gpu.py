"""GPU: the stem convolution, the 3x3/2 max-pool and the 2x bilinear up-sampling in training mode (omnifusion_amd.ops.stem_conv2d /
max_pool2d / upsample_bilinear2x and their modules, csrc/omni_stem_conv.hip, omni_maxpool_bwd.hip, omni_upsample_bwd.hip)
against float64 torch autograd on the CPU over the same float32 inputs, backward from a random grad_out.  Inputs come from a seeded
torch.Generator, the stem's weights are divided by sqrt(147).  Every buffer the operators allocate is filled with NaN first (ops._empty),
so an element no kernel writes shows.

The gate comes from the reference side alone, as in test_batchnorm_gpu.py: per case and per tensor, e32 = max|v32 - v64| / max(1, rms(v64))
of torch's OWN float32 CPU evaluation against the float64 one; the device must satisfy err <= 8 . max(e32, 5e-7).  The factor 8 covers a
different summation order, the floor keeps a case where torch is exact from demanding exactness.  Every measured error is printed.

The stage test masks (ReLU) and selects (pool) with the device's own forward, the reference with the float64 one, so its seed is chosen,
from the float64 reference alone, so that no pre-activation lies within MARGIN = 1e-5 of 0 and every pool window's greatest value leads
the values at the other positions by MARGIN (or the whole window is exactly 0); `stage_reference` asserts both.

Largest ratios of error to gate measured on an MI355X: see DESIGN.md §22."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 5e-7
MARGIN = 1e-5
CONV_GATE = 3e-5                                                                # tests/test_conv_bwd_gpu.py: the f16x3 products' gate
NAN = float("nan")

#             M   H   W
STEM_CASES = {
    "plain":   (2, 16, 16),
    "odd":     (3, 7, 9),           # odd sizes, partial tiles
    "small":   (2, 3, 3),           # a map smaller than the filter
    "one":     (2, 1, 1),           # one output, almost all padding
    "wide":    (1, 6, 70),          # wide and flat: more than one tile along W only
    "rows10240": (40, 32, 32),      # 160 tiles = 40 chunks of 4: the finish kernel's 16 chunk lanes each add two or three partials
}
#             M  H  W  C
POOL_CASES = {"plain": (2, 8, 8, 32), "odd": (3, 7, 9, 8), "pixel": (2, 1, 1, 4), "rows2": (2, 2, 5, 4), "row": (2, 1, 6, 64)}
UP_CASES = {"pixel": (2, 1, 1, 4), "row": (2, 1, 5, 4), "two": (2, 2, 2, 32), "odd": (3, 3, 7, 8), "plain": (2, 8, 8, 64)}


def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def gates(r32, r64):
    return {k: FACTOR * max(nerr(r32[k], r64[k]), FLOOR) for k in r64 if r64[k] is not None}


def check_gate(what, got, want, gate):
    for k, w in want.items():
        assert (got[k] is None) == (w is None), (what, k)
        if w is None:
            continue
        assert got[k].shape == w.shape and not torch.isnan(got[k]).any(), f"{what}: NaN (an unwritten element) or a wrong shape in {k}"
        e = nerr(got[k], w)
        print(f"spatial {what} {k}: normalised error {e:.3e}  gate {gate[k]:.3e} (e32 {gate[k] / FACTOR:.3e})  ratio {e / gate[k]:.3f}")
        assert e <= gate[k], f"{what}: {k}: {e:.3e} > {gate[k]:.3e}"


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def grad_of(t):
    return t.grad.cpu().contiguous() if t is not None and t.grad is not None else None


# ------------------------------------------------------------------------------------------------ stem
def stem_torch(d, bias, dtype):
    w = d["w"].to(dtype, copy=True).requires_grad_(True)
    b = d["b"].to(dtype, copy=True).requires_grad_(True) if bias else None
    y = F.conv2d(d["x"].to(dtype), w, b, stride=2, padding=3)
    y.backward(d["g"].to(dtype))
    return {"y": y.detach(), "dw": w.grad, "db": b.grad if bias else None}


@functools.lru_cache(maxsize=None)
def stem_reference(name, bias):
    M, H, W = STEM_CASES[name]
    gen = torch.Generator().manual_seed(0)
    d = {"x": torch.randn(M, 3, H, W, generator=gen), "w": torch.randn(64, 3, 7, 7, generator=gen) / math.sqrt(147.0),
         "b": 0.1 * torch.randn(64, generator=gen), "g": torch.randn(M, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=gen)}
    r64 = stem_torch(d, bias, torch.float64)
    return d, r64, gates(stem_torch(d, bias, torch.float32), r64)


def stem_run(d, bias, frozen=(), x_cl=False, g_nchw=False):
    from omnifusion_amd import ops
    x = cl(d["x"]) if x_cl else d["x"].to(DEV)
    w = d["w"].to(DEV).requires_grad_("w" not in frozen)
    b = d["b"].to(DEV).requires_grad_("b" not in frozen) if bias else None
    y = ops.stem_conv2d(x, w, b)
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[2] * y.shape[3] == 1
    if y.requires_grad:
        y.backward(d["g"].to(DEV).contiguous() if g_nchw else cl(d["g"]))
    return {"y": y.detach().cpu().contiguous(), "dw": grad_of(w), "db": grad_of(b)}


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", list(STEM_CASES))
def test_stem_against_float64(name, bias):
    d, want, gate = stem_reference(name, bias)
    check_gate(f"stem {name}{' +bias' if bias else ''}", stem_run(d, bias), want, gate)


def test_stem_reads_the_weights_as_omni_stem_f32_does():
    """relu(stem_conv2d) against the library's inference stem (folded bn + ReLU baked in) on a 16-multiple square case, at the conv gate."""
    from omnifusion_amd import _lib, ops
    d, _, _ = stem_reference("plain", True)
    M, H, W = STEM_CASES["plain"]
    x, w, b = d["x"].to(DEV), d["w"].to(DEV), d["b"].to(DEV)
    y = F.relu(ops.stem_conv2d(x, w, b)).permute(0, 2, 3, 1).contiguous()
    wk = w.permute(2, 3, 1, 0).contiguous()                                     # [147][64], k = (ky*7+kx)*3+c
    ref = torch.full((M, H // 2, W // 2, 64), NAN, device=DEV)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().omni_stem_f32(_lib.ptr(x), _lib.ptr(wk), _lib.ptr(b), _lib.ptr(ref), M, H, _lib.stream_of(x)), "stem")
    e = nerr(y.cpu(), ref.cpu())
    print(f"spatial stem relu(y) against omni_stem_f32: normalised error {e:.3e}  gate {CONV_GATE:.1e}")
    assert not torch.isnan(ref).any() and (ref > 0).any() and e <= CONV_GATE


# ------------------------------------------------------------------------------------------------ max-pool
def pool_torch(d, dtype):
    x = d["x"].to(dtype, copy=True).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(d["g"].to(dtype))
    return {"y": y.detach(), "dx": x.grad}


@functools.lru_cache(maxsize=None)
def pool_reference(name, relu):
    M, H, W, C = POOL_CASES[name]
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(M, C, H, W, generator=gen)
    if relu:
        x = F.relu(x)                                                           # about half the elements exactly 0, as behind bn1 + ReLU
    d = {"x": x, "g": torch.randn(M, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=gen)}
    r64 = pool_torch(d, torch.float64)
    if relu and name == "odd":
        assert (r64["y"] == 0).any(), "no all-zero window: the tie rule would go untested"
    return d, r64, gates(pool_torch(d, torch.float32), r64)


def pool_run(d, nchw=False):
    from omnifusion_amd import ops
    put = (lambda t: t.to(DEV).contiguous()) if nchw else cl
    x = put(d["x"]).requires_grad_(True)
    y = ops.max_pool2d(x)
    y.backward(put(d["g"]))
    return {"y": y.detach().cpu().contiguous(), "dx": grad_of(x)}


@pytest.mark.parametrize("relu", [False, True], ids=["randn", "relu"])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_against_float64(name, relu):
    d, want, gate = pool_reference(name, relu)
    got = pool_run(d)
    assert torch.equal(got["y"], F.max_pool2d(d["x"], 3, 2, 1)), "the forward must give torch's float32 bits"
    check_gate(f"pool {name}{' relu' if relu else ''}", got, want, gate)


def test_pool_all_zero_map_sends_the_gradient_to_the_first_tap():
    g = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).expand(1, 4, 2, 2).contiguous()
    got = pool_run({"x": torch.zeros(1, 4, 4, 4), "g": g})
    want = torch.zeros(4, 4)
    want[:2, :2] = g[0, 0]
    assert torch.equal(got["y"], torch.zeros(1, 4, 2, 2))
    assert torch.equal(got["dx"], want.expand(1, 4, 4, 4)), got["dx"][0, 0]
    assert torch.equal(pool_torch({"x": torch.zeros(1, 4, 4, 4), "g": g}, torch.float32)["dx"], want.expand(1, 4, 4, 4))   # torch's rule indeed


def test_pool_drops_a_nan():
    """the forward's fmaxf drops a NaN, the backward sends a window's gradient to its first greatest NON-NaN element."""
    x = torch.zeros(1, 4, 4, 4)
    x[0, :, 1, 1] = NAN
    x[0, :, 0, 1] = 2.0
    g = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).expand(1, 4, 2, 2).contiguous()
    got = pool_run({"x": x, "g": g})
    assert torch.equal(got["y"], torch.tensor([[2.0, 2.0], [0.0, 0.0]]).expand(1, 4, 2, 2))
    want = torch.zeros(4, 4)
    want[0, 1], want[1, 0], want[1, 2] = 1.0 + 2.0, 3.0, 4.0                  # windows (0,0) and (0,1): the 2; (1,0), (1,1): their first zero
    assert torch.equal(got["dx"], want.expand(1, 4, 4, 4)), got["dx"][0, 0]


# ------------------------------------------------------------------------------------------------ up-sampling
def up_torch(d, dtype):
    x = d["x"].to(dtype, copy=True).requires_grad_(True)
    y = F.interpolate(x, size=(2 * x.shape[2], 2 * x.shape[3]), mode="bilinear", align_corners=False)
    y.backward(d["g"].to(dtype))
    return {"y": y.detach(), "dx": x.grad}


@functools.lru_cache(maxsize=None)
def up_reference(name):
    M, H, W, C = UP_CASES[name]
    gen = torch.Generator().manual_seed(0)
    d = {"x": torch.randn(M, C, H, W, generator=gen), "g": torch.randn(M, C, 2 * H, 2 * W, generator=gen)}
    r64 = up_torch(d, torch.float64)
    return d, r64, gates(up_torch(d, torch.float32), r64)


def up_run(d, nchw=False):
    from omnifusion_amd import ops
    put = (lambda t: t.to(DEV).contiguous()) if nchw else cl
    x = put(d["x"]).requires_grad_(True)
    y = ops.upsample_bilinear2x(x)
    y.backward(put(d["g"]))
    return {"y": y.detach().cpu().contiguous(), "dx": grad_of(x)}


@pytest.mark.parametrize("name", list(UP_CASES))
def test_upsample_against_float64(name):
    d, want, gate = up_reference(name)
    check_gate(f"upsample {name}", up_run(d), want, gate)
    ones = up_run({"x": d["x"], "g": torch.ones_like(d["g"])})["dx"]
    assert torch.equal(ones, torch.full_like(ones, 4.0)), "every input element carries total weight 4"


# ------------------------------------------------------------------------------------------------ properties
def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert not torch.isnan(a[k]).any() and torch.equal(a[k], b[k]), k


def test_two_runs_give_the_same_bits():
    for bias in (False, True):
        same_bits(stem_run(stem_reference("rows10240", bias)[0], bias), stem_run(stem_reference("rows10240", bias)[0], bias))
    same_bits(stem_run(stem_reference("odd", True)[0], True), stem_run(stem_reference("odd", True)[0], True))
    same_bits(pool_run(pool_reference("odd", True)[0]), pool_run(pool_reference("odd", True)[0]))
    same_bits(up_run(up_reference("odd")[0]), up_run(up_reference("odd")[0]))


def test_batch_equals_items_one_at_a_time():
    for run, d in ((pool_run, pool_reference("odd", True)[0]), (pool_run, pool_reference("rows2", False)[0]), (up_run, up_reference("odd")[0]),
                   (up_run, up_reference("row")[0])):
        whole = run(d)
        for m in range(d["x"].shape[0]):
            item = run({k: v[m:m + 1] for k, v in d.items()})
            for k in whole:
                assert torch.equal(whole[k][m:m + 1], item[k]), (run.__name__, m, k)


def test_memory_formats_give_the_same_bits():
    d = stem_reference("odd", True)[0]
    same_bits(stem_run(d, True), stem_run(d, True, x_cl=True, g_nchw=True))
    same_bits(pool_run(pool_reference("odd", True)[0]), pool_run(pool_reference("odd", True)[0], nchw=True))
    same_bits(up_run(up_reference("odd")[0]), up_run(up_reference("odd")[0], nchw=True))


def test_only_the_requested_gradients_are_computed(monkeypatch):
    from omnifusion_amd import _lib, ops
    d, want, gate = stem_reference("odd", True)
    full = stem_run(d, True)
    log = []
    monkeypatch.setattr(_lib, "CALL_LOG", log)
    # a frozen weight behind a trainable batch normalisation: the stem's output needs no gradient, its backward never runs
    w = d["w"].to(DEV)
    gamma = torch.ones(64, device=DEV, requires_grad=True)
    y = ops.batch_norm(ops.stem_conv2d(d["x"].to(DEV), w), gamma, training=True, act="relu")
    y.backward(torch.ones_like(y))
    assert w.grad is None and gamma.grad is not None and not torch.isnan(gamma.grad).any()
    assert "stem_conv2d" in log and "batch_norm_bwd" in log and "stem_conv2d_bwd_weight" not in log
    # a frozen weight with a trainable bias: no dw, the same db
    got = stem_run(d, True, frozen=("w",))
    assert got["dw"] is None and torch.equal(got["db"], full["db"])
    got = stem_run(d, True, frozen=("b",))
    assert got["db"] is None and torch.equal(got["dw"], full["dw"])
    assert log.count("stem_conv2d_bwd_weight") == 2
    # the pool and the up-sampling behind a frozen input launch no backward
    del log[:]
    a = cl(pool_reference("odd", True)[0]["x"])
    s = torch.ones(1, device=DEV, requires_grad=True)
    (ops.max_pool2d(a) * s).sum().backward()
    (ops.upsample_bilinear2x(a) * s).sum().backward()
    assert "max_pool2d" in log and "upsample_bilinear2x" in log and "max_pool2d_bwd" not in log and "upsample_bilinear2x_bwd" not in log


# ------------------------------------------------------------------------------------------------ one stage of the network
STAGE_SEED = 1
STAGE_LR = 0.1
STAGE_PARAMS = ("w1", "gamma", "beta", "w2", "b2")


def stage_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    return {"x": rn(2, 3, 16, 16), "w1": rn(64, 3, 7, 7) / math.sqrt(147.0), "gamma": 1 + 0.1 * rn(64), "beta": 0.1 * rn(64),
            "w2": rn(64, 64, 3, 3) / math.sqrt(576.0), "b2": 0.1 * rn(64), "g": rn(2, 64, 8, 8)}


def stage_margins(d):
    """(the smallest |pre-activation|, the smallest lead of a pool window's winner over the other positions) of the float64 stage"""
    x, w1, gamma, beta = (d[k].double() for k in ("x", "w1", "gamma", "beta"))
    z = F.batch_norm(F.conv2d(x, w1, None, stride=2, padding=3), None, None, gamma, beta, True, 0.1, 1e-5)
    a = F.relu(z)
    win = F.unfold(F.pad(a, (1, 1, 1, 1), value=-math.inf), 3, stride=2).view(a.shape[0], a.shape[1], 9, -1)
    top = win.sort(dim=2, descending=True).values
    lead = top[:, :, 0] - top[:, :, 1]
    lead = torch.where(top[:, :, 0] == 0, torch.full_like(lead, math.inf), lead)    # a window of exact zeros: any rule but torch's would show
    return z.abs().min().item(), lead.min().item()


def stage_torch(d, dtype):
    p = {k: d[k].to(dtype, copy=True).requires_grad_(True) for k in STAGE_PARAMS}
    a = F.conv2d(d["x"].to(dtype), p["w1"], None, stride=2, padding=3)
    a = F.relu(F.batch_norm(a, None, None, p["gamma"], p["beta"], True, 0.1, 1e-5))
    a = F.conv2d(F.max_pool2d(a, 3, 2, 1), p["w2"], p["b2"], padding=1)
    y = F.interpolate(a, size=(8, 8), mode="bilinear", align_corners=False)
    y.backward(d["g"].to(dtype))
    out = {k: v.grad for k, v in p.items()}
    out.update(y=y.detach(), w1_after=(p["w1"] - STAGE_LR * p["w1"].grad).detach())
    return out


@functools.lru_cache(maxsize=None)
def stage_reference():
    d = stage_inputs(STAGE_SEED)
    zmin, lead = stage_margins(d)
    assert zmin >= MARGIN, f"a float64 pre-activation within {MARGIN} of 0 ({zmin:.2e}): pick another seed"
    assert lead >= MARGIN, f"a pool window whose winner leads by less than {MARGIN} ({lead:.2e}): pick another seed"
    return d, stage_torch(d, torch.float64)


def stage_device(p, x, g):
    """the functional stage on the device -> (y, the gradients in STAGE_PARAMS order)"""
    from omnifusion_amd import ops
    a = ops.batch_norm(ops.stem_conv2d(x, p["w1"]), p["gamma"], p["beta"], training=True, momentum=0.1, eps=1e-5, act="relu")
    y = ops.upsample_bilinear2x(ops.conv2d(ops.max_pool2d(a), p["w2"], p["b2"], padding=1))
    return (y,) + torch.autograd.grad(y, [p[k] for k in STAGE_PARAMS], g)


def stage_params(d):
    return {k: d[k].to(DEV).requires_grad_(True) for k in STAGE_PARAMS}


def test_stage_against_float64():
    d, want = stage_reference()
    p = stage_params(d)
    outs = stage_device(p, d["x"].to(DEV), cl(d["g"]))
    got = dict(zip(("y",) + STAGE_PARAMS, outs))
    with torch.no_grad():
        got["w1_after"] = p["w1"] - STAGE_LR * got["w1"]                       # one SGD step of the stem's weight
    for k, w in want.items():
        assert not torch.isnan(got[k]).any(), k
        e = nerr(got[k].cpu(), w)
        print(f"spatial stage {k}: normalised error {e:.3e}  gate {CONV_GATE:.1e}  ratio {e / CONV_GATE:.3f}")
        assert e <= CONV_GATE, f"stage: {k}: {e:.3e}"


def test_stage_graph_capture_and_convert():
    """The stage captured in torch.cuda.graph and replayed twice equals the eager run bit for bit, and convert(model, spatial=True) of the
    equivalent nn.Sequential gives the functional form's bits."""
    from omnifusion_amd import ops
    d, _ = stage_reference()
    p = stage_params(d)
    gen = torch.Generator().manual_seed(77)
    xs, gs = d["x"].to(DEV), cl(d["g"])
    # Nothing of an autograd graph built on the default stream may be alive while the capture runs (the warm-up's results are dropped,
    # the eager runs come after it): the engine would make that stream wait for the capturing one, which breaks the capture.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stage_device(p, xs, gs)                                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = stage_device(p, xs, gs)
    torch.cuda.synchronize()
    eager = None
    for i in range(2):
        x_new, g_new = (d["x"], d["g"]) if i == 0 else (torch.randn(d["x"].shape, generator=gen), torch.randn(d["g"].shape, generator=gen))
        with torch.no_grad():
            xs.copy_(x_new)
            gs.copy_(g_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = tuple(t.detach() for t in stage_device(p, x_new.to(DEV), cl(g_new)))
        for got, want in zip(outs, eager):
            assert not torch.isnan(got).any() and torch.equal(got, want), f"replay {i}"
        if i == 0:
            first = eager
    eager, x, g = first, d["x"].to(DEV), cl(d["g"])

    nn = torch.nn
    model = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1),
                          nn.Conv2d(64, 64, 3, padding=1), ops.UpsampleBilinear2x())
    with torch.no_grad():
        for layer, names in ((model[0], ("w1",)), (model[1], ("gamma", "beta")), (model[4], ("w2", "b2"))):
            for param, k in zip((layer.weight, layer.bias), names):
                param.copy_(d[k])
    model, names = ops.convert(model.to(DEV).train(), spatial=True)
    assert names == ["0", "1", "3", "4"]
    y = model(x)
    grads = torch.autograd.grad(y, [model[0].weight, model[1].weight, model[1].bias, model[4].weight, model[4].bias], g)
    for k, got, want in zip(("y",) + STAGE_PARAMS, (y,) + grads, eager):
        assert not torch.isnan(got).any() and torch.equal(got, want), k
