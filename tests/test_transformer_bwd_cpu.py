"""CPU: the boundary of the transformer's training operators (omnifusion_amd.ops.layer_norm / gelu / attention / linear and the modules
LayerNorm, GELU, Linear, TransformerBlock, TransformerCascade; csrc/omni_transformer_bwd.hip) — the names exist and are bound, the
workspace queries, the C-level rejections that return before a device is touched, the ValueErrors of the Python layer on CPU tensors, and
the reference's state-dict names."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omnifusion.h")
UNIT = os.path.join(ROOT, "omnifusion_amd", "csrc", "omni_transformer_bwd.hip")
NEW_SYMBOLS = ("omni_layernorm_bwd_workspace_bytes", "omni_layernorm_fwd_f32", "omni_layernorm_bwd_f32", "omni_attention_bwd_workspace_bytes",
               "omni_attention_bwd_f32", "omni_gelu_fwd_f32", "omni_gelu_bwd_f32")


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


def test_symbols_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(HEADER).read()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_layernorm_bwd_workspace_bytes.restype is ctypes.c_size_t and L.omni_attention_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.omni_layernorm_fwd_f32.argtypes) == 8 and len(L.omni_layernorm_bwd_f32.argtypes) == 12
    assert len(L.omni_attention_bwd_f32.argtypes) == 10
    assert len(L.omni_gelu_fwd_f32.argtypes) == 4 and len(L.omni_gelu_bwd_f32.argtypes) == 5


def test_no_getenv_no_guarded_kernel_name_and_no_second_attention_forward_in_the_unit():
    from omnifusion_amd import isa
    src = open(UNIT).read() + open(os.path.join(os.path.dirname(UNIT), "omni_partials.h")).read()       # (the finish order the unit includes)
    assert "getenv" not in src and "hipMalloc" not in src and "Synchronize" not in src
    kernels = re.findall(r"void\s+(\w+_kernel)\s*\(", src)
    assert {"ln_fwd_kernel", "ln_bwd_row_kernel", "ln_bwd_reduce_kernel", "ln_bwd_finish_kernel", "attention_bwd_rows_kernel",
            "attention_bwd_keys_kernel", "gelu_fwd_kernel", "gelu_bwd_kernel"} == set(kernels)
    for k in kernels:
        assert not any(g in k for g in isa.COUNTED + isa.HOT), k


def test_workspace_queries():
    from omnifusion_amd import _lib
    L = _lib.load()
    q = L.omni_layernorm_bwd_workspace_bytes
    for bad in ((0, 512), (-3, 512), (18, 0), (18, -4), (18, 6), (18, 1028), (18, 1023), (1 << 31, 512)):
        assert q(*bad) == 0, bad

    def want(rows, C):                                                          # include/omnifusion.h
        slab = max(8, -(-rows // 1024))
        nslab = -(-rows // slab)
        return (nslab * 2 * C * 8 + rows * 8 + 15) // 16 * 16

    for rows, C in ((1, 4), (18, 512), (144, 512), (368, 512), (37, 100), (5, 1024), (4101, 4), (8192, 512), (8193, 512), (100000, 32)):
        assert q(rows, C) == want(rows, C), (rows, C)
    a = L.omni_attention_bwd_workspace_bytes
    for bad in ((0, 18), (-1, 18), (1, 0), (1, 65), (1, -2), (1 << 30, 64)):
        assert a(*bad) == 0, bad
    for B, N in ((1, 1), (1, 18), (8, 18), (8, 46), (8, 64), (3, 3)):
        assert a(B, N) == 2 * B * 4 * N * N * 4, (B, N)
    assert a(8, 64) == 1 << 20


def test_c_boundary_rejects_before_touching_a_device():
    """Every rejection of the header.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    big = 1 << 30
    err = L.omni_last_error

    #   x gamma beta y | rows C eps | stream
    def f(x=p, gamma=p, beta=p, y=p, rows=18, C=512, eps=1e-5):
        return L.omni_layernorm_fwd_f32(x, gamma, beta, y, rows, C, eps, z)

    assert f(x=z) == INV and b"null" in err()
    assert f(y=z) == INV
    for C in (0, -4, 6, 510):
        assert f(C=C) == INV and b"multiple of 4" in err(), C
    assert f(C=1028) == UNS and b"1024" in err()
    assert f(rows=0) == INV and f(rows=-1) == INV
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        assert f(eps=eps) == INV and b"eps" in err(), eps
    assert f(rows=1 << 31) == UNS and b"32-bit" in err()

    #   grad_y x gamma dx dgamma dbeta | rows C eps | ws ws_bytes stream
    def b(g=p, x=p, gamma=p, dx=p, dgamma=p, dbeta=p, rows=18, C=512, eps=1e-5, ws=p, nb=big):
        return L.omni_layernorm_bwd_f32(g, x, gamma, dx, dgamma, dbeta, rows, C, eps, ws, nb, z)

    assert b(g=z) == INV and b"null" in err()
    assert b(x=z) == INV
    assert b(dx=z, dgamma=z, dbeta=z) == INV and b"no gradient requested" in err()
    for C in (0, 6, 30):
        assert b(C=C) == INV and b"multiple of 4" in err(), C
    assert b(C=1028) == UNS
    assert b(rows=0) == INV
    assert b(eps=0.0) == INV and b"eps" in err()
    assert b(nb=16) == INV and b"workspace" in err()
    assert b(ws=z) == INV and b"workspace" in err()
    assert b(nb=L.omni_layernorm_bwd_workspace_bytes(18, 512) - 1) == INV and b"workspace" in err()
    assert b(dx=z, ws=z) == INV                                                  # the parameters' sums need it even without dx
    assert b(rows=1 << 31) == UNS

    #   q kv grad_out dq dkv | B N | ws ws_bytes stream
    def a(q=p, kv=p, go=p, dq=p, dkv=p, B=1, N=18, ws=p, nb=big):
        return L.omni_attention_bwd_f32(q, kv, go, dq, dkv, B, N, ws, nb, z)

    assert a(N=65) == UNS and b"64 tokens" in err()
    assert a(N=0) == INV and a(B=0) == INV and a(B=-1) == INV
    assert a(q=z) == INV and b"null" in err()
    assert a(kv=z) == INV and a(go=z) == INV
    assert a(dq=z, dkv=z) == INV and b"no gradient requested" in err()
    assert a(nb=16) == INV and b"workspace" in err()
    assert a(ws=z) == INV and b"workspace" in err()
    assert a(B=8, N=64, nb=(1 << 20) - 1) == INV and b"workspace" in err()

    assert L.omni_gelu_fwd_f32(p, p, 6, z) == INV and b"multiple of 4" in err()
    assert L.omni_gelu_fwd_f32(p, p, 0, z) == INV and L.omni_gelu_fwd_f32(p, p, -4, z) == INV
    assert L.omni_gelu_fwd_f32(z, p, 8, z) == INV and b"null" in err()
    assert L.omni_gelu_fwd_f32(p, z, 8, z) == INV
    assert L.omni_gelu_bwd_f32(p, p, p, 1030, z) == INV and b"multiple of 4" in err()
    assert L.omni_gelu_bwd_f32(p, p, p, 0, z) == INV
    for k in range(3):
        args = [p, p, p]
        args[k] = z
        assert L.omni_gelu_bwd_f32(*args, 8, z) == INV and b"null" in err()


def test_python_errors_of_the_functions():
    from omnifusion_amd import ops
    x = torch.rand(18, 512)
    X = dev(x)
    v = lambda n=512: dev(torch.rand(n))
    # layer_norm
    with pytest.raises(ValueError, match="x must be a tensor on an MI355X device; there is no CPU path"):
        ops.layer_norm(x)
    with pytest.raises(ValueError, match="must be a tensor"):
        ops.layer_norm(x.numpy())
    with pytest.raises(ValueError, match="weight must be a tensor on an MI355X device"):
        ops.layer_norm(X, torch.rand(512))
    with pytest.raises(ValueError, match="float32"):
        ops.layer_norm(dev(x.double()))
    with pytest.raises(ValueError, match="bias must be float32"):
        ops.layer_norm(X, v(), dev(torch.rand(512).half()))
    with pytest.raises(ValueError, match="non-empty"):
        ops.layer_norm(dev(torch.rand(0, 512)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.layer_norm(dev(torch.rand(3, 6)))
    with pytest.raises(ValueError, match="at most 1024"):
        ops.layer_norm(dev(torch.rand(3, 1028)))
    with pytest.raises(ValueError, match=r"weight must be \[C\]"):
        ops.layer_norm(X, v(256))
    with pytest.raises(ValueError, match=r"bias must be \[C\]"):
        ops.layer_norm(X, v(), v(4))
    for eps in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="eps must be a positive finite number"):
            ops.layer_norm(X, eps=eps)
    # gelu
    with pytest.raises(ValueError, match="no CPU path"):
        ops.gelu(x)
    with pytest.raises(ValueError, match="float32"):
        ops.gelu(dev(x.half()))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.gelu(dev(torch.rand(3, 2)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.gelu(dev(torch.rand(0, 4)))
    # attention
    q, kv = dev(torch.rand(36, 512)), dev(torch.rand(36, 1024))
    with pytest.raises(ValueError, match="q must be a tensor on an MI355X device"):
        ops.attention(torch.rand(36, 512), kv, 2)
    with pytest.raises(ValueError, match="kv must be float32"):
        ops.attention(q, dev(torch.rand(36, 1024).double()), 2)
    with pytest.raises(ValueError, match="model width is 512"):
        ops.attention(dev(torch.rand(36, 256)), dev(torch.rand(36, 512)), 2)
    with pytest.raises(ValueError, match="model width is 512"):
        ops.attention(q, dev(torch.rand(36, 1536)), 2)
    with pytest.raises(ValueError, match="non-empty"):
        ops.attention(dev(torch.rand(2, 18, 512)), kv, 2)
    with pytest.raises(ValueError, match="same B.N rows"):
        ops.attention(q, dev(torch.rand(18, 1024)), 2)
    with pytest.raises(ValueError, match="multiple of batch"):
        ops.attention(q, kv, 5)
    with pytest.raises(ValueError, match="at most 64 tokens"):
        ops.attention(dev(torch.rand(65, 512)), dev(torch.rand(65, 1024)), 1)
    for batch in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="batch must be a positive int"):
            ops.attention(q, kv, batch)
    # linear
    w, bias = dev(torch.rand(2048, 512)), dev(torch.rand(2048))
    with pytest.raises(ValueError, match="x must be a tensor on an MI355X device"):
        ops.linear(x, w)
    with pytest.raises(ValueError, match="weight must be float32"):
        ops.linear(X, dev(torch.rand(2048, 512).double()))
    with pytest.raises(ValueError, match=r"\[rows, K\]"):
        ops.linear(dev(torch.rand(2, 9, 512)), w)
    with pytest.raises(ValueError, match="res must have the result's shape"):
        ops.linear(X, w, bias, dev(torch.rand(18, 512)))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.linear(dev(torch.rand(18, 48)), dev(torch.rand(64, 48)))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.linear(X, dev(torch.rand(40, 512)))
    with pytest.raises(ValueError, match="input channels"):
        ops.linear(X, dev(torch.rand(64, 256)))
    with pytest.raises(ValueError, match="bias must be"):
        ops.linear(X, w, dev(torch.rand(512)))


def test_python_errors_of_the_modules():
    from omnifusion_amd import ops
    with pytest.raises(ValueError, match="one normalised axis"):
        ops.LayerNorm((18, 512))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.LayerNorm(6)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.LayerNorm(1028)
    with pytest.raises(ValueError, match="eps"):
        ops.LayerNorm(512, eps=0.0)
    for kw in ({"dim": 256}, {"num_heads": 8}, {"dim": 1024, "num_heads": 8}):
        with pytest.raises(ValueError, match="width 512 with 4 heads"):
            ops.TransformerBlock(**kw)
    with pytest.raises(ValueError, match="width 512 with 4 heads"):
        ops.TransformerCascade(256, 18)
    with pytest.raises(ValueError, match="width 512 with 4 heads"):
        ops.TransformerCascade(512, 18, num_heads=2)
    for n in (0, 65, 18.0):
        with pytest.raises(ValueError, match="1 to 64 patches"):
            ops.TransformerCascade(512, n)
    with pytest.raises(ValueError, match="depth >= 1"):
        ops.TransformerCascade(512, 18, depth=0)
    x = torch.rand(2, 18, 512)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.LayerNorm(512)(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.GELU()(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.Linear(512, 512)(x)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.TransformerBlock()(x.reshape(36, 512), 2)
    net = ops.TransformerCascade(512, 18, depth=1)
    with pytest.raises(ValueError, match="no CPU path"):
        net(x)
    for bad in (torch.rand(2, 10, 512), torch.rand(36, 512), torch.rand(2, 18, 256)):
        with pytest.raises(ValueError, match=r"x must be \[bs, 18, 512\]"):
            net(dev(bad))


def test_modules_carry_the_torch_layers_state_dicts():
    from omnifusion_amd import ops
    nn = torch.nn
    assert issubclass(ops.LayerNorm, nn.LayerNorm) and issubclass(ops.Linear, nn.Linear)
    ln = ops.LayerNorm(512, eps=1e-6)
    assert ln.eps == 1e-6 and ln.normalized_shape == (512,) and list(ln.state_dict()) == list(nn.LayerNorm(512).state_dict())
    plain = ops.LayerNorm(100, elementwise_affine=False)
    assert plain.weight is None and plain.bias is None and list(plain.state_dict()) == []
    assert list(ops.Linear(512, 2048).state_dict()) == ["weight", "bias"] and list(ops.Linear(512, 512, bias=False).state_dict()) == ["weight"]
    assert list(ops.GELU().state_dict()) == []
    blk = ops.TransformerBlock(512, 4)
    assert sorted(blk.state_dict()) == sorted(["norm1.weight", "norm1.bias", "attn.q.weight", "attn.kv.weight", "attn.proj.weight", "attn.proj.bias",
                                               "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"])
    assert blk.norm1.eps == 1e-5 and blk.norm2.eps == 1e-5
    assert tuple(blk.attn.kv.weight.shape) == (1024, 512) and tuple(blk.mlp.fc1.weight.shape) == (2048, 512)


@pytest.mark.parametrize("N", [18, 10])
def test_cascade_loads_the_transformer_slice_of_the_reference_state_dict(N):
    from omnifusion_amd import ops
    from omnifusion_amd.weights import make_state_dict
    sd = make_state_dict(42, N, False)
    part = {k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")}
    assert len(part) == 1 + 6 * 12 + 2
    net = ops.TransformerCascade(512, N)
    assert set(net.state_dict()) == set(part)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in part.items()}
    res = net.load_state_dict(part, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(net.pos_emb.data, part["pos_emb"]) and torch.equal(net.layer[5].mlp.fc2.bias.data, part["layer.5.mlp.fc2.bias"])
    assert net.encoder_norm.eps == 1e-6 and len(net.layer) == 6 and all(p.requires_grad for p in net.parameters())
    assert len(ops.TransformerCascade(512, N, depth=2).layer) == 2
    with pytest.raises(RuntimeError):
        ops.TransformerCascade(512, N + 1).load_state_dict(part, strict=True)   # pos_emb of another patch count
