"""GPU: the transformer's training operators (omnifusion_amd.ops.layer_norm / gelu / attention / linear, TransformerBlock,
TransformerCascade; csrc/omni_transformer_bwd.hip) against float64 torch autograd on the CPU of the restatements in
tests/_transformer_cases.py.

Every buffer the operators allocate is filled with NaN first (ops._empty); the C-level calls write into buffers with NaN rows behind the last
valid row, which must come back untouched.

The gate of the three fp32 operators comes from the reference side alone: err = max|v - v64| / max(1, rms(v64)); e32 is the same error of
torch's own float32 CPU run of the restatement; the device must satisfy err <= 8 . max(e32, 5e-7).  The linear layers carry the f16x3
products' gate 3e-5 (tests/test_conv_bwd_gpu.py), a chain of both max(3e-5, 8 . e32) per tensor.  Every measured error is printed; the largest
ratios measured on an MI355X are in DESIGN.md §21."""
import ctypes
import functools
import math

import pytest
import torch

import _transformer_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FACTOR, FLOOR = 8.0, 5e-7
CONV_GATE = 3e-5
NAN = float("nan")
OK, INVALID, UNSUPPORTED = 0, 1, 3
PAD = 3                                               # NaN rows behind every output of a C-level call
LN_SLAB_ROWS, FINISH_THREADS = 8, 256                 # include/omnifusion.h: rows per slab of the dgamma / dbeta partials; the finish block


@pytest.fixture(autouse=True)
def nan_filled_buffers(monkeypatch):
    from omnifusion_amd import ops
    monkeypatch.setattr(ops, "_empty", lambda size, **kw: torch.full(size if isinstance(size, tuple) else (size,), NAN, **kw))


def _lib():
    from omnifusion_amd import _lib as L
    return L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return t.to(DEV).contiguous() if t is not None else None


def _out(rows, cols):
    return torch.full((rows + PAD, cols), NAN, device=DEV)


def _untouched(buf, rows):
    assert torch.isnan(buf[rows:]).all(), "rows past the end were written"


def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.detach().cpu().double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


WORST = {}


def check(what, kind, got, want64, want32=None, gate=None):
    """prints the measured error and holds it to FACTOR . max(e32, FLOOR), or to `gate` where one is given"""
    got = got.detach().cpu()
    assert got.shape == want64.shape, (what, kind, got.shape, want64.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN (an unwritten element) in {kind}"
    e = nerr(got, want64)
    if gate is None:
        e32 = nerr(want32, want64)
        gate = FACTOR * max(e32, FLOOR)
    WORST[kind] = max(WORST.get(kind, 0.0), e / gate)
    print(f"transformer_bwd {what} {kind}: normalised error {e:.3e}  gate {gate:.3e}  ratio {e / gate:.3f}  (largest so far for {kind}: {WORST[kind]:.3f})")
    assert e <= gate, f"{what}: {kind}: {e:.3e} > {gate:.3e}"


# ------------------------------------------------------------------------------------------------------------------ layer norm
LN_ROWS = (1, 3, 4, 5, 37, 144)
LN_C = (512, 4, 100, 1024)
LN_KINDS = ("unit", "offset", "small")


def ln_case(rows, C, eps, kind):
    """x [rows, C], weight, bias, grad_y.  C = 512: tc.ln_case itself; other widths: the same three kinds"""
    g = tc.gen("ln_bwd", rows, C, eps, kind)
    if C == 512:
        x, w, b = tc.ln_case(rows, eps, kind)
    else:
        x = torch.randn((rows, C), generator=g)
        x = x + 100.0 if kind == "offset" else x * 3e-3 if kind == "small" else x
        w, b = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    return x, w, b, torch.randn((rows, C), generator=g)


def ln_torch(x, w, b, gy, eps, affine, dtype):
    """-> y, dx, dgamma, dbeta of tc.layernorm in `dtype` on the CPU (the last two None without affine)"""
    xl = x.to(dtype, copy=True).requires_grad_(True)
    wl = w.to(dtype, copy=True).requires_grad_(True) if affine else torch.ones_like(w, dtype=dtype)
    bl = b.to(dtype, copy=True).requires_grad_(True) if affine else torch.zeros_like(b, dtype=dtype)
    y = tc.layernorm(xl, wl, bl, eps, dtype)
    y.backward(gy.to(dtype))
    return y.detach(), xl.grad, wl.grad if affine else None, bl.grad if affine else None


def ln_device(x, w, b, gy, eps, affine, want=(True, True, True)):
    """the two C-level calls with NaN rows behind every output -> y, dx, dgamma, dbeta (None where not wanted)"""
    lib = _lib()
    rows, C = x.shape
    X, G, W, B = _dev(x), _dev(gy), _dev(w) if affine else None, _dev(b) if affine else None
    y = _out(rows, C)
    assert lib.omni_layernorm_fwd_f32(_p(X), _p(W), _p(B), _p(y), rows, C, eps, _stream()) == OK, lib.omni_last_error()
    _untouched(y, rows)
    dx = _out(rows, C) if want[0] else None
    dg = torch.full((1 + PAD, C), NAN, device=DEV) if want[1] else None
    db = torch.full((1 + PAD, C), NAN, device=DEV) if want[2] else None
    nbytes = lib.omni_layernorm_bwd_workspace_bytes(rows, C)
    ws = torch.full((nbytes // 4 + 4 * PAD,), NAN, device=DEV)
    rc = lib.omni_layernorm_bwd_f32(_p(G), _p(X), _p(W), _p(dx), _p(dg), _p(db), rows, C, eps, _p(ws), nbytes, _stream())
    assert rc == OK, lib.omni_last_error()
    _untouched(ws, nbytes // 4)
    for t, r in ((dx, rows), (dg, 1), (db, 1)):
        if t is not None:
            _untouched(t, r)
    return y[:rows], dx[:rows] if want[0] else None, dg[0] if want[1] else None, db[0] if want[2] else None


@pytest.mark.parametrize("C", LN_C)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_against_float64(rows, C):
    lib = _lib()
    for eps in tc.LN_EPS:
        for kind in LN_KINDS:
            x, w, b, gy = ln_case(rows, C, eps, kind)
            for affine in (True, False):
                what = f"layer_norm rows {rows} C {C} eps {eps} {kind} affine {affine}"
                r64, r32 = ln_torch(x, w, b, gy, eps, affine, F64), ln_torch(x, w, b, gy, eps, affine, F32)
                got = ln_device(x, w, b, gy, eps, affine, (True, affine, affine))
                for name, g, a, c in zip(("ln_y", "ln_dx", "ln_dgamma", "ln_dbeta"), got, r64, r32):
                    assert (g is None) == (a is None)
                    if a is not None:
                        check(what, name, g, a, c)
                if C == 512 and affine:                                          # the engine's kernel: the same bits
                    y512, X, W, B = _out(rows, 512), _dev(x), _dev(w), _dev(b)
                    assert lib.omni_layernorm512_f32(_p(X), _p(W), _p(B), _p(y512), rows, ctypes.c_float(eps), _stream()) == OK
                    assert torch.equal(got[0], y512[:rows]), what
                again = ln_device(x, w, b, gy, eps, affine, (True, affine, affine))
                assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(got, again)), f"{what}: two runs differ"


def test_layernorm_many_slabs():
    """enough rows that every thread of the finish kernel adds more than one slab partial"""
    lib = _lib()
    C, eps = 100, 1e-5
    rows = 2 * FINISH_THREADS * LN_SLAB_ROWS + 5
    nslab = (lib.omni_layernorm_bwd_workspace_bytes(rows, C) - rows * 8) // (2 * C * 8)
    assert nslab >= 2 * FINISH_THREADS and math.ceil(rows / LN_SLAB_ROWS) == nslab        # the plan's own figures
    x, w, b, gy = ln_case(rows, C, eps, "unit")
    r64, r32 = ln_torch(x, w, b, gy, eps, True, F64), ln_torch(x, w, b, gy, eps, True, F32)
    got = ln_device(x, w, b, gy, eps, True)
    for name, g, a, c in zip(("ln_y", "ln_dx", "ln_dgamma", "ln_dbeta"), got, r64, r32):
        check(f"layer_norm rows {rows} C {C}", name, g, a, c)
    assert all(torch.equal(p, q) for p, q in zip(got, ln_device(x, w, b, gy, eps, True)))


def _ln_ops(x, w, b, gy, eps, frozen=()):
    from omnifusion_amd import ops
    leaf = {k: (_dev(t).requires_grad_(k not in frozen) if t is not None else None) for k, t in (("x", x), ("w", w), ("b", b))}
    y = ops.layer_norm(leaf["x"], leaf["w"], leaf["b"], eps)
    if any(t is not None and t.requires_grad for t in leaf.values()):
        y.backward(_dev(gy))
    return {"y": y.detach(), **{k: (t.grad if t is not None else None) for k, t in leaf.items()}}


@pytest.mark.parametrize("rows,C", [(37, 512), (5, 100), (144, 1024)])
def test_layernorm_op_only_requested_gradients(rows, C):
    from omnifusion_amd import ops
    x, w, b, gy = ln_case(rows, C, 1e-5, "unit")
    full = _ln_ops(x, w, b, gy, 1e-5)
    ref = ln_device(x, w, b, gy, 1e-5, True)
    for k, r in zip(("y", "x", "w", "b"), ref):
        assert torch.equal(full[k], r), k                                       # the operator is the two C calls
    no_x = _ln_ops(x, w, b, gy, 1e-5, frozen=("x",))
    assert no_x["x"] is None and all(torch.equal(no_x[k], full[k]) for k in ("y", "w", "b"))
    no_wb = _ln_ops(x, w, b, gy, 1e-5, frozen=("w", "b"))
    assert no_wb["w"] is None and no_wb["b"] is None and torch.equal(no_wb["x"], full["x"]) and torch.equal(no_wb["y"], full["y"])
    only_b = _ln_ops(x, w, b, gy, 1e-5, frozen=("x", "w"))
    assert only_b["x"] is None and only_b["w"] is None and torch.equal(only_b["b"], full["b"])
    plain = _ln_ops(x, None, None, gy, 1e-5)
    assert plain["w"] is None and plain["b"] is None and not torch.isnan(plain["x"]).any()
    x3 = _dev(x).reshape(1, rows, C).requires_grad_(True)                       # leading axes and the module
    layer = ops.LayerNorm(C, eps=1e-5).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(_dev(w)); layer.bias.copy_(_dev(b))
    y3 = layer(x3)
    y3.backward(_dev(gy).reshape(1, rows, C))
    assert y3.shape == (1, rows, C) and torch.equal(y3[0], full["y"]) and torch.equal(x3.grad[0], full["x"])
    assert torch.equal(layer.weight.grad, full["w"]) and torch.equal(layer.bias.grad, full["b"])


# ------------------------------------------------------------------------------------------------------------------ attention
ATT_SHAPES = [(1, 1), (3, 3), (2, 10), (1, 18), (2, 26), (1, 46), (2, 63), (1, 64)]
ATT_KINDS = ("unit", "sharp")
ATT_GRADS = (1.0, 1e-6)


def att_case(B, N, kind, gscale):
    qkv = tc.attention_case(B, N, kind)
    go = gscale * torch.randn((B * N, 512), generator=tc.gen("att_bwd", B, N, kind, gscale))
    return qkv[:, :512].contiguous(), qkv[:, 512:].contiguous(), go


def att_torch(q, kv, go, B, N, dtype):
    ql, kvl = q.to(dtype, copy=True).requires_grad_(True), kv.to(dtype, copy=True).requires_grad_(True)
    out = tc.attention_q_kv(ql, kvl, B, N, dtype)
    out.backward(go.to(dtype))
    return out.detach(), ql.grad, kvl.grad[:, :512], kvl.grad[:, 512:]


def att_device(Q, KV, GO, B, N, want=(True, True)):
    """the C-level backward on device tensors -> dq, dkv (None where not wanted)"""
    lib = _lib()
    M = B * N
    dq, dkv = _out(M, 512) if want[0] else None, _out(M, 1024) if want[1] else None
    nbytes = lib.omni_attention_bwd_workspace_bytes(B, N)
    assert nbytes == 2 * B * 4 * N * N * 4
    ws = torch.full((nbytes // 4 + 4 * PAD,), NAN, device=DEV)
    rc = lib.omni_attention_bwd_f32(_p(Q), _p(KV), _p(GO), _p(dq), _p(dkv), B, N, _p(ws), nbytes, _stream())
    assert rc == OK, lib.omni_last_error()
    _untouched(ws, nbytes // 4)
    if want[0]:
        _untouched(dq, M)
    if want[1]:
        _untouched(dkv, M)
        assert not torch.isnan(ws[:nbytes // 4]).any()                          # every probability row was written
    return dq[:M] if want[0] else None, dkv[:M] if want[1] else None


@pytest.mark.parametrize("B,N", ATT_SHAPES)
def test_attention_backward_against_float64(B, N):
    from omnifusion_amd import ops
    lib = _lib()
    M = B * N
    for kind in ATT_KINDS:
        for gscale in ATT_GRADS:
            what = f"attention B {B} N {N} {kind} grad {gscale}"
            q, kv, go = att_case(B, N, kind, gscale)
            r64, r32 = att_torch(q, kv, go, B, N, F64), att_torch(q, kv, go, B, N, F32)
            Q, KV, GO = _dev(q), _dev(kv), _dev(go)
            dq, dkv = att_device(Q, KV, GO, B, N)
            for name, g, i in (("att_dq", dq, 1), ("att_dk", dkv[:, :512], 2), ("att_dv", dkv[:, 512:], 3)):
                check(what, name, g, r64[i], r32[i])
            # the operator: the engine's forward, the same backward
            ql, kvl = Q.clone().requires_grad_(True), KV.clone().requires_grad_(True)
            out = ops.attention(ql, kvl, B)
            direct = _out(M, 512)
            assert lib.omni_attention_f32(_p(Q), _p(KV), _p(direct), B, N, _stream()) == OK, lib.omni_last_error()
            assert torch.equal(out.detach(), direct[:M]), what
            check(what, "att_out", out, r64[0], r32[0])
            out.backward(GO)
            assert torch.equal(ql.grad, dq) and torch.equal(kvl.grad, dkv), f"{what}: the operator is the C call"
            # repeatable, and one gradient alone has the bits it has beside the other
            dq2, dkv2 = att_device(Q, KV, GO, B, N)
            assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2), f"{what}: two runs differ"
            assert torch.equal(att_device(Q, KV, GO, B, N, (True, False))[0], dq)
            assert torch.equal(att_device(Q, KV, GO, B, N, (False, True))[1], dkv)
            # batch-split invariance: the items one at a time
            if B > 1:
                for i in range(B):
                    s = slice(i * N, (i + 1) * N)
                    dqi, dkvi = att_device(Q[s].contiguous(), KV[s].contiguous(), GO[s].contiguous(), 1, N)
                    assert torch.equal(dqi, dq[s]) and torch.equal(dkvi, dkv[s]), f"{what}: item {i} alone differs"


def test_attention_frozen_inputs_and_65_tokens():
    from omnifusion_amd import ops
    lib = _lib()
    B, N = 2, 10
    q, kv, go = att_case(B, N, "unit", 1.0)
    Q, KV, GO = _dev(q), _dev(kv), _dev(go)
    dq, dkv = att_device(Q, KV, GO, B, N)
    for fq, fkv in ((True, False), (False, True)):
        ql, kvl = Q.clone().requires_grad_(not fq), KV.clone().requires_grad_(not fkv)
        ops.attention(ql, kvl, B).backward(GO)
        assert (ql.grad is None) == fq and (kvl.grad is None) == fkv
        assert fq or torch.equal(ql.grad, dq)
        assert fkv or torch.equal(kvl.grad, dkv)
    x65, kv65 = torch.zeros((65, 512), device=DEV), torch.zeros((65, 1024), device=DEV)
    with pytest.raises(ValueError, match="at most 64 tokens"):
        ops.attention(x65, kv65, 1)
    o, o2 = _out(65, 512), _out(65, 1024)
    ws = torch.full((2 * 4 * 65 * 65,), NAN, device=DEV)
    assert lib.omni_attention_bwd_f32(_p(x65), _p(kv65), _p(x65), _p(o), _p(o2), 1, 65, _p(ws), ws.numel() * 4, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    _untouched(o, 0); _untouched(o2, 0)
    assert torch.isnan(ws).all()


# ------------------------------------------------------------------------------------------------------------------ GELU
def gelu_case(n):
    g = tc.gen("gelu", n)
    x = torch.rand(n, generator=g) * 24.0 - 12.0
    special = [0.0, -0.0, 1e-40, -12.0, 12.0, -1e-40, 11.75, -5.5]                # +-0, a denormal, the ends of the range
    x[:min(n, len(special))] = torch.tensor(special[:min(n, len(special))])
    return x, torch.randn(n, generator=g)


def gelu_torch(x, gy, dtype):
    xl = x.to(dtype, copy=True).requires_grad_(True)
    y = tc.activation(xl, 2)
    y.backward(gy.to(dtype))
    return y.detach(), xl.grad


@pytest.mark.parametrize("n", [4, 1028, 18 * 2048])
def test_gelu_against_float64(n):
    from omnifusion_amd import ops
    lib = _lib()
    x, gy = gelu_case(n)
    assert 0.0 < x[2].item() < 2.0 ** -126 and (n < 8 or (x.min().item() == -12.0 and x.max().item() == 12.0))
    r64, r32 = gelu_torch(x, gy, F64), gelu_torch(x, gy, F32)
    X, G = _dev(x), _dev(gy)
    y, dx = torch.full((n + 4 * PAD,), NAN, device=DEV), torch.full((n + 4 * PAD,), NAN, device=DEV)
    assert lib.omni_gelu_fwd_f32(_p(X), _p(y), n, _stream()) == OK, lib.omni_last_error()
    assert lib.omni_gelu_bwd_f32(_p(G), _p(X), _p(dx), n, _stream()) == OK, lib.omni_last_error()
    _untouched(y, n); _untouched(dx, n)
    check(f"gelu n {n}", "gelu_y", y[:n], r64[0], r32[0])
    check(f"gelu n {n}", "gelu_dx", dx[:n], r64[1], r32[1])
    xl = X.clone().reshape(-1, 4).requires_grad_(True)                           # the operator and the module: the same two calls
    yo = ops.GELU()(xl)
    yo.backward(G.reshape(-1, 4))
    assert torch.equal(yo.detach().reshape(-1), y[:n]) and torch.equal(xl.grad.reshape(-1), dx[:n])
    # a NaN in x: a NaN at exactly that element of dx (and of y)
    at = n // 2 + 1 if n > 4 else 3
    xn = x.clone()
    xn[at] = NAN
    xl = _dev(xn).requires_grad_(True)
    yn = ops.gelu(xl)
    yn.backward(G)
    only = torch.zeros(n, dtype=torch.bool, device=DEV)
    only[at] = True
    assert torch.equal(torch.isnan(xl.grad), only) and torch.equal(torch.isnan(yn.detach()), only)
    keep = ~only
    assert torch.equal(xl.grad[keep], dx[:n][keep])


def test_gelu_is_the_fused_epilogue():
    """ops.gelu on the pre-activations of one LayerNorm + Linear case against the rows GEMM's fused act = GELU epilogue on the same
    pre-activations: the same expression, so at most the last bit may differ; the count of differing elements is printed."""
    from omnifusion_amd import ops
    from omnifusion_amd.model._engine import split_weights_f16x3
    lib = _lib()
    rows, N = 18, 2048
    x, g, b, w, bias, _ = tc.lng_case(rows, N)
    w16 = split_weights_f16x3(w).to(DEV)
    w16r = torch.empty_like(w16)
    assert lib.omni_gemm_rows_pack(_p(w16), _p(w16r), N, 512, _stream()) == OK, lib.omni_last_error()
    X, G, Bt, Bi = _dev(x), _dev(g), _dev(b), _dev(bias)
    pre, fused = _out(rows, N), _out(rows, N)
    eps = ctypes.c_float(tc.LNG_EPS)
    for dst, act in ((pre, 0), (fused, 2)):
        rc = lib.omni_gemm_rows_ln_sh_f16x3(_p(X), _p(G), _p(Bt), eps, _p(w16r), _p(Bi), None, _p(dst), 0, rows, N, act, _stream())
        assert rc == OK, lib.omni_last_error()
    mine = ops.gelu(pre[:rows].contiguous())
    diff = (mine - fused[:rows]).abs()
    ulp = 2.0 ** -23 * fused[:rows].abs().clamp_min(2.0 ** -126)
    print(f"transformer_bwd gelu vs fused epilogue: {int((diff > 0).sum())} of {diff.numel()} elements differ, "
          f"largest difference {float((diff / ulp).max()):.2f} ulp-class units")
    assert (diff <= ulp).all()


# ------------------------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("rows,K,out", [(18, 512, 2048), (144, 2048, 512)])
def test_linear_is_the_convolution(rows, K, out):
    from omnifusion_amd import ops
    g = tc.gen("linear_bwd", rows, K, out)
    r = lambda *s: torch.randn(s, generator=g)
    d = {"x": r(rows, K), "w": r(out, K) / math.sqrt(K), "b": r(out), "res": r(rows, out)}
    gy = r(rows, out)
    l64 = {k: v.double().requires_grad_(True) for k, v in d.items()}
    y64 = tc.linear(l64["x"], l64["w"], l64["b"], l64["res"], 0, F64)
    y64.backward(gy.double())
    leaf = {k: _dev(v).requires_grad_(True) for k, v in d.items()}
    y = ops.linear(leaf["x"], leaf["w"], leaf["b"], leaf["res"])
    assert y.shape == (rows, out)
    y.backward(_dev(gy))
    what = f"linear {rows} x {K} -> {out}"
    check(what, "linear_y", y, y64.detach(), gate=CONV_GATE)
    for k in d:
        check(what, "linear_d" + k, leaf[k].grad, l64[k].grad, gate=CONV_GATE)
    layer = ops.Linear(K, out).to(DEV)                                          # the module, with leading axes
    with torch.no_grad():
        layer.weight.copy_(leaf["w"]); layer.bias.copy_(leaf["b"])
    y3 = layer(leaf["x"].detach().reshape(1, rows, K), res=leaf["res"].detach().reshape(1, rows, out))
    assert y3.shape == (1, rows, out) and torch.equal(y3[0], y.detach())


# ------------------------------------------------------------------------------------------------------------------ the block and the cascade
def cascade_keys(depth):
    return ["pos_emb"] + [f"layer.{i}.{n}" for i in range(depth) for n in
                          ("norm1.weight", "norm1.bias", "attn.q.weight", "attn.kv.weight", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
                           "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")] + \
        ["encoder_norm.weight", "encoder_norm.bias"]


def cascade_inputs(bs, N, depth):
    """weights (tc.state_dict's transformer.* entries of the first `depth` blocks), tokens [bs, N, 512] (those of tc.whole_case at unit
    scale), and the fixed random projection of the loss"""
    sd = {k: tc.state_dict(N)["transformer." + k] for k in cascade_keys(depth)}
    d = tc.whole_case(N, bs, 1.0).reshape(bs * N, 16, 32)
    tok = tc.token_pack(d, torch.zeros((N, 512)), bs, N, F32).reshape(bs, N, 512)
    proj = torch.randn((bs, N, 512), generator=tc.gen("cascade_proj", bs, N, depth))
    return sd, tok, proj


def restate(sd, tok, depth, dtype):
    """tc.transformer with `depth` blocks, from tc's pieces -> [bs, N, 512]"""
    bs, N, _ = tok.shape
    x = (tok + sd["pos_emb"]).reshape(bs * N, 512)
    for i in range(depth):
        W = lambda n: sd[f"layer.{i}.{n}"]
        y = tc.layernorm(x, W("norm1.weight"), W("norm1.bias"), 1e-5, dtype)
        a = tc.attention_q_kv(tc.linear(y, W("attn.q.weight"), None, None, 0, dtype), tc.linear(y, W("attn.kv.weight"), None, None, 0, dtype), bs, N, dtype)
        x = tc.linear(a, W("attn.proj.weight"), W("attn.proj.bias"), x, 0, dtype)
        h = tc.ln_linear(x, W("norm2.weight"), W("norm2.bias"), 1e-5, W("mlp.fc1.weight"), W("mlp.fc1.bias"), None, 2, dtype)
        x = tc.linear(h, W("mlp.fc2.weight"), W("mlp.fc2.bias"), x, 0, dtype)
    return tc.layernorm(x, sd["encoder_norm.weight"], sd["encoder_norm.bias"], 1e-6, dtype).reshape(bs, N, 512)


@functools.lru_cache(maxsize=None)
def cascade_reference(bs, N, depth, dtype):
    """-> output, {name: gradient} with "tok" among the names, of the restatement in `dtype` on the CPU"""
    sd, tok, proj = cascade_inputs(bs, N, depth)
    leaf = {k: v.to(dtype, copy=True).requires_grad_(True) for k, v in sd.items()}
    t = tok.to(dtype, copy=True).requires_grad_(True)
    out = restate(leaf, t, depth, dtype)
    (out * proj.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in leaf.items()}
    grads["tok"] = t.grad
    return out.detach(), grads


def cascade_device(bs, N, depth):
    from omnifusion_amd import ops
    sd, tok, proj = cascade_inputs(bs, N, depth)
    net = ops.TransformerCascade(512, N, depth=depth).to(DEV)
    net.load_state_dict(sd, strict=True)
    t = _dev(tok).requires_grad_(True)
    out = net(t)
    (out * _dev(proj)).sum().backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads["tok"] = t.grad
    return net, out.detach(), grads


def check_cascade(bs, N, depth):
    want, g64 = cascade_reference(bs, N, depth, F64)
    w32, g32 = cascade_reference(bs, N, depth, F32)
    net, out, grads = cascade_device(bs, N, depth)
    what = f"cascade bs {bs} N {N} depth {depth}"
    assert out.shape == (bs, N, 512) and set(grads) == set(g64)
    check(what, "cascade_out", out, want, gate=max(CONV_GATE, FACTOR * nerr(w32, want)))
    for k in g64:
        kind = "cascade_d" + (k if k in ("tok", "pos_emb") else k.split(".", 2)[-1] if k.startswith("layer.") else k)
        check(f"{what} {k}", kind, grads[k], g64[k], gate=max(CONV_GATE, FACTOR * nerr(g32[k], g64[k])))
    return net, out


@pytest.mark.parametrize("bs,N", [(2, 18), (1, 10)])
def test_cascade_of_two_blocks_against_float64(bs, N):
    check_cascade(bs, N, 2)


def test_cascade_of_six_blocks_against_float64_and_the_engine():
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.weights import make_state_dict
    bs, N = 1, 18
    sd, tok, _ = cascade_inputs(bs, N, 6)
    full = {"transformer." + k: v.double() for k, v in sd.items()}
    mine = restate({k: v.double() for k, v in sd.items()}, tok.double(), 6, F64).reshape(bs * N, 512)
    assert float((mine - tc.transformer(full, tok, F64)).abs().max()) < 1e-12    # the restatement above IS tc's (sums in another order)
    _, out = check_cascade(bs, N, 6)
    # forward only: Engine.transformer on the same weights and tokens, within tc's gate of the case
    net = spherical_fusion(4, N, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(tc.WHOLE_SEED, N, False))
    net._sync_packed(torch.device(DEV))
    eng = net._eng.transformer(_dev(tc.whole_case(N, bs, 1.0)), bs)
    key = ("whole", N, bs, 1.0)
    diff = float((out.reshape(bs * N, 512) - eng).abs().max())
    print(f"transformer_bwd cascade vs Engine.transformer: max difference {diff:.3e} = {diff / tc.GAPS[key]:.2f} x Y, gate {tc.gate(key):.3e}")
    assert diff <= tc.gate(key)
    tc.report(key, "ops", float((out.reshape(bs * N, 512).cpu().double() - tc.whole_run(N, bs, 1.0, F64)).abs().max()))


def test_one_sgd_step():
    """lr 1e-2 on the two-block cascade: every parameter after the step within 1e-6 of the float64 step"""
    bs, N, depth, lr = 2, 18, 2, 1e-2
    sd, tok, proj = cascade_inputs(bs, N, depth)
    _, g64 = cascade_reference(bs, N, depth, F64)
    from omnifusion_amd import ops
    net = ops.TransformerCascade(512, N, depth=depth).to(DEV)
    net.load_state_dict(sd, strict=True)
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    opt.zero_grad()
    (net(_dev(tok)) * _dev(proj)).sum().backward()
    opt.step()
    worst = 0.0
    for k, p in net.named_parameters():
        want = sd[k].double() - lr * g64[k]
        e = float((p.detach().cpu().double() - want).abs().max())
        worst = max(worst, e)
        assert not torch.equal(p.detach().cpu(), sd[k]), f"{k} did not move"
        assert e <= 1e-6, f"{k}: {e:.3e} from the float64 step"
    print(f"transformer_bwd sgd step: largest distance from the float64 step {worst:.3e}")


def test_block_in_a_graph():
    """forward + backward of one TransformerBlock inside torch.cuda.graph (the default hardware queues): each of two replays on new contents
    equals an eager call bit for bit"""
    from omnifusion_amd import ops
    bs, N = 2, 18
    sd, tok, _ = cascade_inputs(bs, N, 1)
    blk = ops.TransformerBlock(512, 4).to(DEV)
    blk.load_state_dict({k[len("layer.0."):]: v for k, v in sd.items() if k.startswith("layer.0.")}, strict=True)
    params = list(blk.parameters())
    gen = tc.gen("block_graph")
    xs = _dev(tok.reshape(bs * N, 512)).requires_grad_(True)
    gs = torch.randn((bs * N, 512), generator=gen).to(DEV)

    def step(x, g):
        y = blk(x, bs)
        return (y,) + torch.autograd.grad(y, [x] + params, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(xs, gs)                                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(xs, gs)
    torch.cuda.synchronize()
    for i in range(2):
        x_new, g_new = torch.randn((bs * N, 512), generator=gen), torch.randn((bs * N, 512), generator=gen)
        with torch.no_grad():
            xs.copy_(x_new)
            gs.copy_(g_new)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(_dev(x_new).requires_grad_(True), _dev(g_new))
        assert len(outs) == len(eager) == 2 + len(params)
        for got, want in zip(outs, eager):
            assert not torch.isnan(got).any() and torch.equal(got, want), f"replay {i}"
