"""GPU: the 1x1 convolutions of the point-feature MLPs (omnifusion_amd.ops.point_conv / PointConv2d, csrc/omni_point_conv.hip)
against float64 torch autograd on the CPU — F.conv2d over x repeated M / Mx times and multiplied by the scale — over the same seeded
float32 inputs, backward from a random grad_y.  x, scale and grad_y are standard normal, the weight is divided by sqrt(Cin).  Every buffer
the operator allocates is filled with NaN first (ops._empty), so an element no kernel writes shows.

The gate comes from the reference side alone, the project's standing one: per case and per tensor, e32 = max|v32 - v64| / max(1, rms(v64))
of torch's OWN float32 CPU evaluation against the float64 one; the device must satisfy err <= 8 . max(e32, 5e-7).  Every measured ratio is
printed; the largest are in DESIGN.md §25.

    (Mx, M, Cin -> Cout, h, w)
    (1, 1, 3 -> 16, 1, 1)               the smallest
    (2, 6, 3 -> 16, 3, 5) with scale    x broadcast over three repeats; 90 rows: one full 64-row tile and a partial one
    (10, 10, 5 -> 16, 4, 4)             the 5-channel form
    (3, 3, 16 -> 64, 7, 9)              dx; 189 rows
    (2, 36, 3 -> 16, 32, 32) with scale 36864 rows in chunks of 320: 116 partials, the last of 64 rows (the plan is printed)"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 5e-7
NAN = float("nan")

#           Mx  M  Cin Cout h   w  scale
CASES = {
    "one":    (1, 1, 3, 16, 1, 1, False),
    "repeat": (2, 6, 3, 16, 3, 5, True),
    "five":   (10, 10, 5, 16, 4, 4, False),
    "wide":   (3, 3, 16, 64, 7, 9, False),
    "chunks": (2, 36, 3, 16, 32, 32, True),
}
GRADS = ("dw", "dscale", "dx")


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def nerr(got, want):
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


@functools.lru_cache(maxsize=None)
def inputs(name):
    Mx, M, cin, cout, h, w, scaled = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 1)
    return {"x": torch.randn(Mx, cin, h, w, generator=gen), "w": torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5,
            "scale": torch.randn(M, 1, h, w, generator=gen) if scaled else None, "gy": torch.randn(M, cout, h, w, generator=gen)}


def torch_run(name, dtype):
    """F.conv2d and its autograd on the CPU in `dtype` -> y, dw, dscale (scaled cases), dx (the 16 -> 64 form)"""
    Mx, M, cin, cout, h, w, scaled = CASES[name]
    d = inputs(name)
    x, wt = d["x"].to(dtype).clone().requires_grad_(cin == 16), d["w"].to(dtype).clone().requires_grad_(True)      # (clone: float32 -> float32 is no copy)
    s = d["scale"].to(dtype).clone().requires_grad_(True) if scaled else None
    xin = x.repeat(M // Mx, 1, 1, 1)                                           # item m reads x[m mod Mx]
    y = F.conv2d(xin * s if scaled else xin, wt)
    y.backward(d["gy"].to(dtype))
    return {"y": y.detach(), "dw": wt.grad, "dscale": s.grad if scaled else None, "dx": x.grad if cin == 16 else None}


@functools.lru_cache(maxsize=None)
def reference(name):
    want, r32 = torch_run(name, torch.float64), torch_run(name, torch.float32)
    gate = {k: FACTOR * max(nerr(r32[k], v), FLOOR) for k, v in want.items() if v is not None}
    return want, gate


def device_tensors(name, need_w=True, need_s=True, need_x=True):
    Mx, M, cin, cout, h, w, scaled = CASES[name]
    d = inputs(name)
    x = d["x"].to(DEV)
    if cin == 16:
        x = x.contiguous(memory_format=torch.channels_last).requires_grad_(need_x)
    return {"x": x, "w": d["w"].to(DEV).requires_grad_(need_w), "scale": d["scale"].to(DEV).requires_grad_(need_s) if scaled else None,
            "gy": d["gy"].to(DEV)}


def run(name, **need):
    from omnifusion_amd import ops
    v = device_tensors(name, **need)
    y = ops.point_conv(v["x"], v["w"], scale=v["scale"])
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[1] == 1 or y.shape[2] * y.shape[3] == 1
    if y.requires_grad:
        y.backward(v["gy"])
    cpu = lambda t: None if t is None else t.detach().cpu().contiguous()
    return {"y": cpu(y), "dw": cpu(v["w"].grad), "dscale": cpu(v["scale"].grad) if v["scale"] is not None else None,
            "dx": cpu(v["x"].grad) if v["x"].requires_grad else None}


@functools.lru_cache(maxsize=None)
def device_result(name):
    return run(name)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_against_float64(name):
    from omnifusion_amd import _lib
    Mx, M, cin, cout, h, w, scaled = CASES[name]
    want, gate = reference(name)
    got = device_result(name)
    nbytes = _lib.load().omni_point_conv_bwd_workspace_bytes(M, h * w, cin, cout)
    nchunk = nbytes // (4 * cin * cout)
    per = 64 * max(5, -(-(-(-M * h * w // 1024)) // 64))
    print(f"point_conv {name}: {M * h * w} rows, plan: {nchunk} partial(s) of {per} rows (the last of {M * h * w - (nchunk - 1) * per})")
    assert nchunk == -(-M * h * w // per)
    if name == "chunks":
        assert nchunk >= 3 and (M * h * w) % per
    for k, v in want.items():
        g = got[k]
        if v is None:
            assert g is None, k
            continue
        assert g is not None and g.shape == v.shape and not torch.isnan(g).any(), f"{name}: NaN (an unwritten element) or a wrong shape in {k}"
        e = nerr(g, v)
        print(f"point_conv {name} {k}: normalised error {e:.3e}  gate {gate[k]:.3e} (e32 {gate[k] / FACTOR:.3e})  ratio {e / gate[k]:.3f}")
        assert e <= gate[k], f"{name}: {k}: {e:.3e} > {gate[k]:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_give_the_same_bits(name):
    a, b = device_result(name), run(name)
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), f"{name}: {k}"


@pytest.mark.parametrize("name", ["repeat", "wide", "chunks"])
def test_frozen_inputs_get_none_and_leave_the_other_bits_alone(name):
    full = device_result(name)
    live = [k for k in GRADS if full[k] is not None]
    flag = {"dw": "need_w", "dscale": "need_s", "dx": "need_x"}
    for frozen in live:
        got = run(name, **{flag[frozen]: False})
        assert got[frozen] is None and torch.equal(got["y"], full["y"])
        for k in live:
            if k != frozen:
                assert torch.equal(got[k], full[k]), f"{name}: {k} with {frozen} frozen"
    got = run(name, need_w=False, need_s=False, need_x=False)                   # nothing pending: no graph, the same forward
    assert all(got[k] is None for k in GRADS) and torch.equal(got["y"], full["y"])


@pytest.mark.parametrize("name", ["repeat", "chunks"])
def test_dscale_of_the_items_one_at_a_time_equals_the_batched_bits(name):
    """item m alone: x[m mod Mx] with scale[m] — dscale (and y) of an item are functions of that item"""
    from omnifusion_amd import ops
    Mx, M, cin, cout, h, w, _ = CASES[name]
    d, full = inputs(name), device_result(name)
    wt = d["w"].to(DEV)
    for m in sorted({0, 1, Mx, M - 1}):
        s = d["scale"][m:m + 1].to(DEV).requires_grad_(True)
        y = ops.point_conv(d["x"][m % Mx:m % Mx + 1].to(DEV), wt, scale=s)
        y.backward(d["gy"][m:m + 1].to(DEV))
        assert torch.equal(s.grad.cpu(), full["dscale"][m:m + 1]) and torch.equal(y.detach().cpu().contiguous(), full["y"][m:m + 1]), m


def test_dx_of_an_item_does_not_depend_on_the_batch():
    from omnifusion_amd import ops
    d, full = inputs("wide"), device_result("wide")
    x = d["x"][1:2].to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.point_conv(x, d["w"].to(DEV))
    y.backward(d["gy"][1:2].to(DEV))
    assert torch.equal(x.grad.cpu().contiguous(), full["dx"][1:2]) and torch.equal(y.detach().cpu().contiguous(), full["y"][1:2])


def test_the_layer_and_a_planar_16_channel_input():
    """ops.PointConv2d on the module path, and a planar x for the 16 -> 64 form (converted, the same bits)"""
    from omnifusion_amd import ops
    d, full = inputs("wide"), device_result("wide")
    layer = ops.PointConv2d(16, 64, kernel_size=1, stride=1, padding=0, bias=False).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(d["w"])
    x = d["x"].to(DEV).requires_grad_(True)                                    # planar storage
    y = layer(x)
    y.backward(d["gy"].to(DEV))
    assert torch.equal(y.detach().cpu().contiguous(), full["y"]) and torch.equal(layer.weight.grad.cpu(), full["dw"])
    assert torch.equal(x.grad.cpu().contiguous(), full["dx"])


@pytest.mark.parametrize("name", ["repeat", "wide"])
def test_graph_capture_replays_the_eager_bits(name):
    from omnifusion_amd import ops
    eager = device_result(name)
    v = device_tensors(name)
    wrt = [(k, v[t]) for k, t in (("dw", "w"), ("dscale", "scale"), ("dx", "x")) if v[t] is not None and v[t].requires_grad]

    def step():
        y = ops.point_conv(v["x"], v["w"], scale=v["scale"])
        return (y.detach(),) + tuple(torch.autograd.grad(y, [t for _, t in wrt], v["gy"]))

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
    for k, t in zip(("y",) + tuple(k for k, _ in wrt), outs):
        assert torch.equal(t.cpu().contiguous(), eager[k]), k
