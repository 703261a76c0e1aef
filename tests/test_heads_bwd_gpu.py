"""GPU: the two depth heads in training mode (omnifusion_amd.ops.depth_heads / DepthHeads, csrc/omni_heads_bwd.hip) against
float64 torch autograd on the CPU (F.conv2d, relu, sigmoid, the product) over the same seeded float32 inputs, backward from a random
grad_a and grad_c.  x is standard normal, the weights are divided by sqrt(288), the biases are 0.1 . randn.  Every buffer the operator
allocates is filled with NaN first (ops._empty), so an element no kernel writes shows.

The gate comes from the reference side alone, as in test_spatial_ops_gpu.py: per case and per tensor, e32 = max|v32 - v64| / max(1, rms(v64))
of torch's OWN float32 CPU evaluation against the float64 one; the device must satisfy err <= 8 . max(e32, 5e-7).  Every measured ratio is
printed.

The device masks (ReLU) with its own float32 p, the reference with the float64 one, so the seed of each case is the first one, judged from
the float64 reference alone, at which no |p| < MARGIN = 1e-5; `reference` asserts it.

A gradient that autograd leaves undefined on the reference side (pred's parameters when only grad_c flows) is compared as zero.

Largest ratios of error to gate measured on an MI355X: see DESIGN.md §23."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 8.0, 5e-7
MARGIN = 1e-5
NAN = float("nan")

#          M   H   W
CASES = {
    "one":       (2, 1, 1),         # all padding
    "odd":       (3, 7, 9),         # odd, partial tiles
    "tile":      (2, 16, 16),       # exactly one tile
    "wide":      (1, 6, 70),        # more than one tile along W only
    "past":      (2, 17, 33),       # one pixel past a tile edge in both axes
    "rows40960": (40, 32, 32),      # 160 tiles = 40 chunks of 4: the finish kernel's 16 lanes each add two or three partials
}
#         confidence, grad_a, grad_c
MODES = {"conf-both": (True, True, True), "conf-a": (True, True, False), "conf-c": (True, False, True), "plain-a": (False, True, False)}
PARAMS = ("x", "wp", "bp", "wc", "bc")


def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def heads_torch(d, mode, dtype):
    conf, use_a, use_c = MODES[mode]
    v = {k: d[k].to(dtype, copy=True).requires_grad_(True) for k in PARAMS}
    p = F.conv2d(v["x"], v["wp"], v["bp"], padding=1)
    s = torch.sigmoid(F.conv2d(v["x"], v["wc"], v["bc"], padding=1))
    a = F.relu(p) * s if conf else F.relu(p)
    loss = (a * d["ga"].to(dtype)).sum() * float(use_a) + (s * d["gc"].to(dtype)).sum() * float(use_c)
    grads = torch.autograd.grad(loss, [v[k] for k in PARAMS], allow_unused=True)
    out = {"a": a.detach(), "c": s.detach() if conf else None, "p": p.detach()}
    out.update({"d" + k: (g if g is not None else torch.zeros_like(v[k])) for k, g in zip(PARAMS, grads)})
    return out


def inputs(name, seed):
    M, H, W = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(M, 32, H, W, generator=gen), "wp": torch.randn(1, 32, 3, 3, generator=gen) / math.sqrt(288.0),
            "bp": 0.1 * torch.randn(1, generator=gen), "wc": torch.randn(1, 32, 3, 3, generator=gen) / math.sqrt(288.0),
            "bc": 0.1 * torch.randn(1, generator=gen), "ga": torch.randn(M, 1, H, W, generator=gen), "gc": torch.randn(M, 1, H, W, generator=gen)}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """the first seed, judged from the float64 pre-activation alone, at which no |p| < MARGIN"""
    for seed in range(64):
        d = inputs(name, seed)
        p = F.conv2d(d["x"].double(), d["wp"].double(), d["bp"].double(), padding=1)
        if p.abs().min().item() >= MARGIN:
            return d
    raise AssertionError(f"{name}: no seed below 64 keeps every |p| >= {MARGIN}")


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    d = case_inputs(name)
    r64 = heads_torch(d, mode, torch.float64)
    assert r64["p"].abs().min().item() >= MARGIN, "a pre-activation within MARGIN of 0: the ReLU masks of float32 and float64 could differ"
    r32 = heads_torch(d, mode, torch.float32)
    keys = [k for k in r64 if k != "p" and r64[k] is not None]
    return d, {k: r64[k] for k in keys}, {k: FACTOR * max(nerr(r32[k], r64[k]), FLOOR) for k in keys}


def run(d, mode, frozen=(), x_nchw=False, items=None):
    from omnifusion_amd import ops
    conf, use_a, use_c = MODES[mode]
    sl = slice(None) if items is None else items
    x = d["x"][sl]
    v = {"x": (x.to(DEV).contiguous() if x_nchw else cl(x)).requires_grad_("x" not in frozen)}
    v.update({k: d[k].to(DEV).requires_grad_(k not in frozen) for k in PARAMS[1:]})
    a, c = ops.depth_heads(v["x"], v["wp"], v["bp"], v["wc"], v["bc"], confidence=conf)
    assert (c is None) == (not conf) and a.shape == (x.shape[0], 1) + tuple(x.shape[2:])
    outs, gs = [], []
    if use_a:
        outs.append(a); gs.append(d["ga"][sl].to(DEV))
    if use_c:
        outs.append(c); gs.append(d["gc"][sl].to(DEV))
    torch.autograd.backward(outs, gs)
    out = {"a": a.detach().cpu(), "c": c.detach().cpu() if conf else None}
    out.update({"d" + k: (v[k].grad.cpu().contiguous() if v[k].grad is not None else None) for k in PARAMS})
    return out


def zero_if_none(got, like):
    return got if got is not None else torch.zeros(like.shape)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_heads_against_float64(name, mode):
    d, want, gate = reference(name, mode)
    got = run(d, mode)
    for k, w in want.items():
        g = zero_if_none(got[k], w) if k.startswith("d") else got[k]
        assert g.shape == w.shape and not torch.isnan(g).any(), f"{name} {mode}: NaN (an unwritten element) or a wrong shape in {k}"
        e = nerr(g, w)
        print(f"heads {name} {mode} {k}: normalised error {e:.3e}  gate {gate[k]:.3e} (e32 {gate[k] / FACTOR:.3e})  ratio {e / gate[k]:.3f}")
        assert e <= gate[k], f"{name} {mode}: {k}: {e:.3e} > {gate[k]:.3e}"


def test_planar_x_gives_the_bits_of_channels_last():
    d, _, _ = reference("past", "conf-both")
    a, b = run(d, "conf-both"), run(d, "conf-both", x_nchw=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("frozen", [("x",), ("wp",), ("bp",), ("wc",), ("bc",), ("wp", "bp", "wc", "bc")], ids=lambda f: "+".join(f))
def test_frozen_inputs_get_no_gradient(frozen):
    d, _, _ = reference("past", "conf-both")
    full, part = run(d, "conf-both"), run(d, "conf-both", frozen=frozen)
    for k in PARAMS:
        if k in frozen:
            assert part["d" + k] is None, k
        else:
            assert torch.equal(part["d" + k], full["d" + k]), k
    assert torch.equal(part["a"], full["a"]) and torch.equal(part["c"], full["c"])


def test_no_grad_and_plain_mode_outputs():
    from omnifusion_amd import ops
    d, want, gate = reference("odd", "plain-a")
    v = {k: (cl(d[k]) if k == "x" else d[k].to(DEV)) for k in PARAMS}
    with torch.no_grad():
        a, c = ops.depth_heads(v["x"], v["wp"], v["bp"], v["wc"], v["bc"], confidence=False)
    assert c is None and not a.requires_grad and nerr(a.cpu(), want["a"]) <= gate["a"]
    assert torch.equal(a.cpu(), run(d, "plain-a")["a"])


def test_two_runs_are_bit_equal():
    d, _, _ = reference("rows40960", "conf-both")
    a, b = run(d, "conf-both"), run(d, "conf-both")
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_items_alone_give_the_batched_dx():
    d, _, _ = reference("past", "conf-both")
    full = run(d, "conf-both")
    for i in (0, 1):
        one = run(d, "conf-both", items=slice(i, i + 1))
        assert torch.equal(one["dx"], full["dx"][i:i + 1]), i
        assert torch.equal(one["a"], full["a"][i:i + 1]) and torch.equal(one["c"], full["c"][i:i + 1])


@pytest.mark.parametrize("conf", [True, False], ids=["conf", "plain"])
def test_forward_agrees_with_omni_heads_f32(conf):
    from omnifusion_amd import _lib
    mode = "conf-both" if conf else "plain-a"
    d, want, gate = reference("tile", mode)
    M, H, W = CASES["tile"]
    got = run(d, mode)
    x = d["x"].to(DEV).permute(0, 2, 3, 1).contiguous()
    w = torch.cat([d["wp"], d["wc"]]).permute(0, 2, 3, 1).reshape(2, 9, 32).contiguous().to(DEV)
    ra, rc = torch.full((M, 1, H, W), NAN, device=DEV), torch.full((M, 1, H, W), NAN, device=DEV)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().omni_heads_f32(_lib.ptr(x), _lib.ptr(w), d["bp"].item(), d["bc"].item(), _lib.ptr(ra), _lib.ptr(rc), M, H,
                                              int(conf), _lib.stream_of(x)), "heads")
    for k, r in (("a", ra), ("c", rc)):
        if want.get(k) is None:
            continue
        e, e64 = nerr(got[k], r.cpu()), nerr(r.cpu(), want[k])
        print(f"heads tile {mode} {k} against omni_heads_f32: {e:.3e}  (omni_heads_f32 against float64 {e64:.3e})  gate {gate[k]:.3e}")
        assert not torch.isnan(r).any() and e <= gate[k]


def test_graph_capture_replays_the_eager_bits():
    from omnifusion_amd import ops
    d, _, _ = reference("past", "conf-both")
    eager = run(d, "conf-both")
    v = {"x": cl(d["x"]).requires_grad_(True)}
    v.update({k: d[k].to(DEV).requires_grad_(True) for k in PARAMS[1:]})
    ga, gc = d["ga"].to(DEV), d["gc"].to(DEV)

    def step():
        a, c = ops.depth_heads(v["x"], v["wp"], v["bp"], v["wc"], v["bc"], confidence=True)
        grads = torch.autograd.grad([a, c], [v[k] for k in PARAMS], [ga, gc])
        return (a.detach(), c.detach()) + tuple(grads)

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
    for k, t in zip(("a", "c") + tuple("d" + k for k in PARAMS), outs):
        assert torch.equal(t.cpu().contiguous(), eager[k]), k


def test_rejections_come_before_any_launch():
    from omnifusion_amd import ops
    d = case_inputs("odd")
    v = {k: d[k].to(DEV) for k in PARAMS}
    args = lambda **kw: [kw.get(k, v[k]) for k in PARAMS]
    with pytest.raises(ValueError, match="no CPU path"):
        ops.depth_heads(*args(x=d["x"]))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.depth_heads(*args(bp=d["bp"]))
    with pytest.raises(ValueError, match="float32"):
        ops.depth_heads(*args(x=v["x"].half()))
    with pytest.raises(ValueError, match="float32"):
        ops.depth_heads(*args(wc=v["wc"].double()))
    with pytest.raises(ValueError, match=r"\[M,32,H,W\]"):
        ops.depth_heads(*args(x=v["x"][:, :16]))
    with pytest.raises(ValueError, match=r"\[M,32,H,W\]"):
        ops.depth_heads(*args(x=v["x"][0]))
    with pytest.raises(ValueError, match=r"w_pred must be \[1,32,3,3\]"):
        ops.depth_heads(*args(wp=v["wp"][..., :1]))
    with pytest.raises(ValueError, match=r"w_conf must be \[1,32,3,3\]"):
        ops.depth_heads(*args(wc=torch.cat([v["wc"], v["wc"]])))
    with pytest.raises(ValueError, match=r"b_conf must be \[1\]"):
        ops.depth_heads(*args(bc=v["bc"][0]))


def test_module_holds_the_reference_names():
    from omnifusion_amd import ops
    d, want, gate = reference("odd", "conf-both")
    m = ops.DepthHeads().to(DEV)
    assert list(m.state_dict()) == ["pred.weight", "pred.bias", "weight_pred.weight", "weight_pred.bias"]
    assert tuple(m.pred.weight.shape) == (1, 32, 3, 3) and tuple(m.weight_pred.bias.shape) == (1,)
    m.load_state_dict({"pred.weight": d["wp"], "pred.bias": d["bp"], "weight_pred.weight": d["wc"], "weight_pred.bias": d["bc"]})
    a, c = m(cl(d["x"]))
    torch.autograd.backward([a, c], [d["ga"].to(DEV), d["gc"].to(DEV)])
    assert nerr(a.detach().cpu(), want["a"]) <= gate["a"] and nerr(m.pred.weight.grad.cpu(), want["dwp"]) <= gate["dwp"]
    assert nerr(m.weight_pred.bias.grad.cpu(), want["dbc"]) <= gate["dbc"]
    a2, c2 = m(cl(d["x"]), confidence=False)
    assert c2 is None and torch.equal(a2.detach().cpu(), run(d, "plain-a")["a"])
