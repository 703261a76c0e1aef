"""The transformer between layer4 and the decoder, operator by operator: plain torch restatements, an emulation of the split-half
format, the seeded cases of tests/test_transformer_cpu.py and tests/test_transformer_gpu.py, and their yardsticks.

Every restatement takes a `dtype` and is run twice, in float64 (the reference of the GPU tests) and in float32.  Y, the yardstick of a
case, is max |float32 run - float64 run| of its restatement on the case's inputs (GAPS, measured on the CPU; test_transformer_cpu.py
recomputes the table and holds it to the stored figures).  The gate of every float64 comparison on the device is FACTOR * Y with
FACTOR = 4: the 22-bit split-half format against fp32's 24 bits, another summation order, the dropped lo * lo term.  MEASURED holds the
ratios error / Y the MI355X gave when the gates were written.

Layouts (include/omnifusion.h): d [M, HW, C] -> token m, dim c * HW + hw; q | k | v at columns 0 / 512 / 1024 of [B * N, 1536]; four heads of
128; weights [out, in] as nn.Linear keeps them.
"""
import math
import zlib

import torch
import torch.nn.functional as F

FACTOR = 4.0
HEADS, HEAD_DIM = 4, 128
SCALE = HEAD_DIM ** -0.5


def gen(*key):
    """one seeded generator per case key (crc32 of its repr: stable across runs and machines)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the split-half format (csrc/omni_sh.h)
def sh_split(x):
    """float32 -> (hi, lo) halfs: hi = fp16(x), 0 below the fp16 normal range 2^-14; lo = fp16((x - hi) * 2048); |x| saturates at 65504."""
    x = x.to(torch.float32).clamp(-65504.0, 65504.0)
    hi = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x).half()
    lo = ((x - hi.float()) * 2048.0).half()
    return hi, lo


def sh_value(x, dtype=torch.float64):
    """what a split-half tensor holds of x: hi + lo * 2^-11, exactly (in `dtype`)"""
    hi, lo = sh_split(x)
    return hi.to(dtype) + lo.to(dtype) / 2048.0


# ------------------------------------------------------------------ restatements
def attention(q, k, v, B, N, dtype, fault=None):
    """softmax(q k^T / sqrt(128)) v per batch item and head: q, k, v [B * N, 512] -> [B * N, 512] (model/blocks.py:52-62).
    fault: None | "fp16_out" | "uniform_query" | "no_scale" | "kv_of_item0"."""
    sp = lambda t: t.to(dtype).reshape(B, N, HEADS, HEAD_DIM).permute(0, 2, 1, 3)
    q, k, v = sp(q), sp(k), sp(v)
    if fault == "kv_of_item0" and B > 1:
        k, v = k.clone(), v.clone()
        k[1], v[1] = k[0], v[0]
    logits = q @ k.transpose(-2, -1)
    if fault != "no_scale":
        logits = logits * SCALE
    p = torch.softmax(logits, -1)
    if fault == "uniform_query":                     # the last query of head 1 of the last item averages its values
        p = p.clone()
        p[B - 1, 1, N - 1] = 1.0 / N
    out = (p @ v).permute(0, 2, 1, 3).reshape(B * N, HEADS * HEAD_DIM)
    if fault == "fp16_out":                          # the lo half of the split-half store lost
        out = out.half().to(dtype)
    return out


def attention_qkv(qkv, B, N, dtype, fault=None):
    """the same from a fused q | k | v projection [B * N, 1536]"""
    return attention(qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:], B, N, dtype, fault)


def attention_q_kv(q, kv, B, N, dtype, fault=None):
    """... and from separate q [B * N, 512] and k | v [B * N, 1024]"""
    return attention(q, kv[:, :512], kv[:, 512:], B, N, dtype, fault)


def token_pack(d, pos, bs, N, dtype, fault=None):
    """d [bs * N, HW, C], pos [N, C * HW] -> tok [bs * N, C * HW]: tok[m, c * HW + hw] = d[m, hw, c] + pos[m % N] (spherical_model.py:264,181).
    fault: "pos_row" (pos[m]: rows past the table read as 0) | "dim_order" (hw * C + c)."""
    M, HW, C = d.shape
    d, pos = d.to(dtype), pos.to(dtype)
    t = d.reshape(M, HW * C) if fault == "dim_order" else d.permute(0, 2, 1).reshape(M, C * HW)
    if fault == "pos_row":
        p = torch.cat([pos, torch.zeros((M - N, C * HW), dtype=dtype)], 0)
    else:
        p = pos.repeat(bs, 1)
    return t + p


def mlp_points(xyz, depth, w1, b1, w2, b2, Mo, N, dtype):
    """xyz [N, 3, HW] (* depth [Mo, HW]) -> relu(W2 relu(W1 x + b1) + b2) as [Mo, HW, 64]; row m reads patch m % N."""
    x = xyz.to(dtype)[torch.arange(Mo) % N].permute(0, 2, 1)                     # [Mo, HW, 3]
    if depth is not None:
        x = x * depth.to(dtype)[:, :, None]
    h = torch.relu(x @ w1.to(dtype).T + b1.to(dtype))
    return torch.relu(h @ w2.to(dtype).T + b2.to(dtype))


def layernorm(x, g, b, eps, dtype):
    """nn.LayerNorm(512): biased variance, eps inside the root"""
    x = x.to(dtype)
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    return c / torch.sqrt(var + eps) * g.to(dtype) + b.to(dtype)


def parts_sum(parts, bias, res, dtype, drop=None):
    """sum_s parts[s] + bias + res in that order ([S, rows, 512]; bias, res optional); drop: a slice left out"""
    t = None
    for s in range(parts.shape[0]):
        if s == drop:
            continue
        t = parts[s].to(dtype) if t is None else t + parts[s].to(dtype)
    if bias is not None:
        t = t + bias.to(dtype)
    if res is not None:
        t = t + res.to(dtype)
    return t


def parts_layernorm(parts, bias, res, g, b, eps, dtype, drop=None):
    """-> (tok, LayerNorm(tok)): the second pass of a K-sliced fc2 with the LayerNorm that follows (blocks.py:83-88)"""
    t = parts_sum(parts, bias, res, dtype, drop)
    return t, layernorm(t, g, b, eps, dtype)


def activation(x, act):
    return torch.relu(x) if act == 1 else 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5))) if act == 2 else x


def linear(x, w, bias, res, act, dtype):
    y = x.to(dtype) @ w.to(dtype).T
    if bias is not None:
        y = y + bias.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return activation(y, act)


def ln_linear(x, g, b, eps, w, bias, res, act, dtype):
    """act(LayerNorm(x) W^T + bias + res): act 0 none, 1 ReLU, 2 GELU (erf)"""
    return linear(layernorm(x, g, b, eps, dtype), w, bias, res, act, dtype)


def transformer(sd, tok, dtype, fault=None):
    """The six pre-LN blocks and encoder_norm over tok [bs, N, 512] (pos_emb added here), restating oracle/model_ref._transformer
    (spherical_model.py:180-187, blocks.py:33-89) -> [bs * N, 512].  fault: an attention fault (in block 2) | "no_fc2_bias" (block 2) |
    "enc_eps" (encoder_norm at 1e-3)."""
    bs, N, _ = tok.shape
    W = lambda k: sd[k].to(dtype)
    x = (tok.to(dtype) + W("transformer.pos_emb")).reshape(bs * N, 512)
    for i in range(6):
        p = f"transformer.layer.{i}."
        hit = fault if i == 2 else None
        y = layernorm(x, W(p + "norm1.weight"), W(p + "norm1.bias"), 1e-5, dtype)
        q, kv = y @ W(p + "attn.q.weight").T, y @ W(p + "attn.kv.weight").T
        a = attention_q_kv(q, kv, bs, N, dtype, hit if hit in ("fp16_out", "uniform_query", "no_scale", "kv_of_item0") else None)
        x = x + a @ W(p + "attn.proj.weight").T + W(p + "attn.proj.bias")
        h = ln_linear(x, W(p + "norm2.weight"), W(p + "norm2.bias"), 1e-5, W(p + "mlp.fc1.weight"), W(p + "mlp.fc1.bias"), None, 2, dtype)
        x = linear(h, W(p + "mlp.fc2.weight"), None if hit == "no_fc2_bias" else W(p + "mlp.fc2.bias"), x, 0, dtype)
    return layernorm(x, W("transformer.encoder_norm.weight"), W("transformer.encoder_norm.bias"), 1e-3 if fault == "enc_eps" else 1e-6, dtype)


def gap(fn):
    """Y of a case: max |float32 run - float64 run| of restatement fn(dtype) (a tensor or a tuple of tensors: the largest)"""
    a, b = fn(torch.float64), fn(torch.float32)
    if not isinstance(a, tuple):
        a, b = (a,), (b,)
    return max(float((x - y.double()).abs().max()) for x, y in zip(a, b))


# ------------------------------------------------------------------ cases
ATT_SHAPES = [(1, 1), (3, 3), (2, 10), (1, 18), (2, 26), (1, 46), (1, 61), (2, 63), (1, 64)]      # (B, N); the kernel groups queries in fours
ATT_KINDS = ("unit", "sharp", "tiny")


def attention_case(B, N, kind):
    """qkv [B * N, 1536].  unit: all three at unit scale (logits of unit scale: a softmax with many live terms); sharp: q * 30 (logits beyond
    +-100: the subtraction of the maximum is needed); tiny: v * 1e-5 (results below 2^-14: the hi half of a split-half store is flushed)."""
    qkv = torch.randn((B * N, 1536), generator=gen("att", B, N, kind))
    if kind == "sharp":
        qkv[:, :512] *= 30.0
    if kind == "tiny":
        qkv[:, 1024:] *= 1e-5
    return qkv


PACK_SHAPES = [(1, 18, 16, 32), (3, 10, 16, 32), (2, 46, 16, 32), (1, 3, 5, 7)]                  # (bs, N, HW, C); the last: 105 elements


def pack_case(bs, N, HW, C):
    g = gen("pack", bs, N, HW, C)
    return torch.randn((bs * N, HW, C), generator=g), torch.randn((N, C * HW), generator=g)       # pos at unit scale: a wrong row shows


MLP_SHAPES = [(Mo, N, HW, dep) for N in (10, 18) for Mo in (N, 2 * N) for HW in (1024, 100) for dep in (False, True)]


def mlp_case(Mo, N, HW, dep):
    """-> xyz (unit rays), depth (0.3 .. 8 with exact zeros, or None), w1 [16,3], b1, w2 [64,16], b2"""
    g = gen("mlp", Mo, N, HW, dep)
    xyz = F.normalize(torch.randn((N, 3, HW), generator=g), dim=1)
    depth = None
    if dep:
        depth = 0.3 + 7.7 * torch.rand((Mo, HW), generator=g)
        depth[torch.rand((Mo, HW), generator=g) < 0.05] = 0.0
        depth[Mo - 1, HW - 1] = 0.0
    r = lambda *s: torch.randn(s, generator=g)
    return xyz, depth, r(16, 3) * 0.8, r(16) * 0.3, r(64, 16) * 0.35, r(64) * 0.3


MLP_ENGINE = ("mlp_points1", "mlp_points2")        # Engine.mlp_points of an iterative engine (nrows 4, 18 patches of 32 x 32 points)


def mlp_engine_case(name):
    """-> xyz [18, 3, 32, 32] unit rays, depth [36, 1, 32, 32] with exact zeros (mlp_points2) or None, Mo"""
    g = gen("mlp_engine", name)
    xyz = F.normalize(torch.randn((18, 3, 32, 32), generator=g), dim=1)
    if name == "mlp_points1":
        return xyz, None, 18
    depth = 0.3 + 7.7 * torch.rand((36, 1, 32, 32), generator=g)
    depth[torch.rand((36, 1, 32, 32), generator=g) < 0.05] = 0.0
    return xyz, depth, 36


def mlp_engine_ref(name, dtype):
    """oracle/model_ref._mlp_points (conv, eval-mode BatchNorm, ReLU, twice: the BatchNorm NOT folded) on the case -> NHWC [Mo, 32, 32, 64]"""
    from oracle import model_ref
    from omnifusion_amd.weights import make_state_dict
    sd = {k: v.to(dtype) for k, v in make_state_dict(WHOLE_SEED, 18, True).items() if k.startswith(name) and v.is_floating_point()}
    xyz, depth, Mo = mlp_engine_case(name)
    x = xyz.to(dtype).repeat(Mo // 18, 1, 1, 1)
    if depth is not None:
        x = x * depth.to(dtype)
    return model_ref._mlp_points(sd, name, x).permute(0, 2, 3, 1).contiguous()


LN_ROWS = (1, 3, 4, 5, 18, 37)                      # four rows per block
LN_EPS = (1e-5, 1e-6)
LN_KINDS = ("unit", "offset", "small", "const")


def ln_case(rows, eps, kind):
    """-> x [rows, 512], weight, bias.  unit; offset: mean 100, std 1; small: std 3e-3 (variance ~ eps: eps matters); const: every row one
    value with a short significand (the mean is exact, x - mean is 0 and the result is the LayerNorm bias exactly)."""
    g = gen("ln", rows, eps, kind)
    x = torch.randn((rows, 512), generator=g)
    if kind == "offset":
        x = x + 100.0
    elif kind == "small":
        x = x * 3e-3
    elif kind == "const":
        # quarters: the wave's sum of 512 equal values (pairs, 6 c among them, then a butterfly) is exact only if 3 c needs no rounding
        x = (torch.round(x[:, :1] * 12.0) / 4.0 + 0.25).expand(rows, 512).contiguous()
    return x, 0.5 + torch.rand(512, generator=g), torch.randn(512, generator=g)


PARTS_N = (1, 2, 4, 8)
PARTS_ROWS = (1, 18, 32, 50)
PARTS_EPS = 1e-5


def parts_case(nparts, rows, has_bias, has_res):
    """-> parts [nparts, rows, 512] (their sum at unit scale), bias or None, res or None, LayerNorm weight, bias"""
    g = gen("parts", nparts, rows, has_bias, has_res)
    parts = torch.randn((nparts, rows, 512), generator=g) / math.sqrt(nparts)
    bias = torch.randn(512, generator=g) if has_bias else None
    res = torch.randn((rows, 512), generator=g) if has_res else None
    return parts, bias, res, 0.5 + torch.rand(512, generator=g), torch.randn(512, generator=g)


GEMM_ROWS = (1, 7, 8, 9, 18, 31, 32)                # 8 waves: the boundary at 8 | 9 rows; at most 32 rows
LNG_N = (512, 1536, 2048)
LNG_OPTIONS = [(act, has_bias, has_res) for act in (0, 2) for has_bias in (False, True) for has_res in (False, True)]
LNG_EPS = 1e-5


def lng_case(rows, N):
    """-> x [rows, 512], LayerNorm weight / bias, w [N, 512] (unit-scale products), bias [N], res [rows, N]; the options pick among the last two"""
    g = gen("lng", rows, N)
    r = lambda *s: torch.randn(s, generator=g)
    return r(rows, 512), 0.5 + torch.rand(512, generator=g), r(512), r(N, 512) / math.sqrt(512.0), r(N), r(rows, N)


SLICES = (1, 2, 4)


def slices_case(rows):
    """fc2 of a lone panorama: x [rows, 2048], w [512, 2048], bias [512]"""
    g = gen("slices", rows)
    r = lambda *s: torch.randn(s, generator=g)
    return r(rows, 2048), r(512, 2048) / math.sqrt(2048.0), r(512)


def lnparts_case(nparts, rows):
    """-> parts, pbias, pres, LayerNorm weight / bias, w [1536, 512]: the next block's norm1 + qkv on fc2's K slices"""
    g = gen("lnparts", nparts, rows)
    r = lambda *s: torch.randn(s, generator=g)
    return r(nparts, rows, 512) / math.sqrt(nparts), r(512), r(rows, 512), 0.5 + torch.rand(512, generator=g), r(512), r(1536, 512) / math.sqrt(512.0)


WHOLE_SHAPES = [(4, 18, 1), (4, 18, 2), (4, 18, 8), (3, 10, 1), (3, 10, 3), (5, 26, 1), (6, 46, 1)]       # (nrows, N, bs)
WHOLE_STD = (10.0, 1.0)                             # 10: the scale of the model's own tokens
WHOLE_SEED = 42


def whole_case(N, bs, std):
    """d [bs * N, 4, 4, 32] fp32: the `down` projection the transformer starts from"""
    return std * torch.randn((bs * N, 4, 4, 32), generator=gen("whole", N, bs, std))


_SD = {}


def state_dict(N):
    from omnifusion_amd.weights import make_state_dict
    if N not in _SD:
        _SD[N] = make_state_dict(WHOLE_SEED, N, False)
    return _SD[N]


def whole_run(N, bs, std, dtype, fault=None):
    """the restatement of Engine.transformer on a case -> [bs * N, 512]"""
    d = whole_case(N, bs, std).reshape(bs * N, 16, 32)
    tok = token_pack(d, torch.zeros((N, 512)), bs, N, dtype).reshape(bs, N, 512)
    return transformer(state_dict(N), tok, dtype, fault)


# ------------------------------------------------------------------ the yardsticks, by case
def measure(key):
    """Y of case `key` (the keys of GAPS)"""
    kind, a = key[0], key[1:]
    if kind == "att":
        qkv = attention_case(*a)
        return gap(lambda t: attention_qkv(qkv, a[0], a[1], t))
    if kind == "pack":
        d, pos = pack_case(*a)
        return gap(lambda t: token_pack(d, pos, a[0], a[1], t))
    if kind == "mlp":
        c = mlp_case(*a)
        return gap(lambda t: mlp_points(*c, a[0], a[1], t))
    if kind == "mlp_engine":
        return gap(lambda t: mlp_engine_ref(a[0], t))
    if kind == "ln":
        x, g, b = ln_case(*a)
        return gap(lambda t: layernorm(x, g, b, a[1], t))
    if kind == "parts":
        c = parts_case(*a)
        return gap(lambda t: parts_layernorm(*c, PARTS_EPS, t))
    if kind == "lng":
        rows, N, act, has_bias, has_res = a
        x, g, b, w, bias, res = lng_case(rows, N)
        return gap(lambda t: ln_linear(x, g, b, LNG_EPS, w, bias if has_bias else None, res if has_res else None, act, t))
    if kind == "slices":
        x, w, bias = slices_case(*a)
        return gap(lambda t: linear(x, w, bias, None, 0, t))
    if kind == "whole":
        return gap(lambda t: whole_run(*a, t))
    raise KeyError(key)


def all_keys():
    keys = [("att", B, N, k) for B, N in ATT_SHAPES for k in ATT_KINDS]
    keys += [("pack",) + s for s in PACK_SHAPES]
    keys += [("mlp",) + s for s in MLP_SHAPES]
    keys += [("mlp_engine", n) for n in MLP_ENGINE]
    keys += [("ln", r, e, k) for r in LN_ROWS for e in LN_EPS for k in LN_KINDS if k != "const"]
    keys += [("parts", n, r, hb, hr) for n in PARTS_N for r in PARTS_ROWS for hb in (False, True) for hr in (False, True)]
    keys += [("lng", r, n) + o for r in GEMM_ROWS for n in LNG_N for o in LNG_OPTIONS]
    keys += [("slices", r) for r in GEMM_ROWS]
    keys += [("whole", N, bs, std) for _, N, bs in WHOLE_SHAPES for std in WHOLE_STD]
    return keys


def format_bound(key, ref):
    """Two attention results are finer in fp32 than a split-half tensor can hold them, so their SPLIT-HALF gate is the format's own bound
    (the bounds test_sh_elementwise_ops_match_f32 sets for the format) where FACTOR * Y lies below it:
    one token — the softmax is 1, the result is v bit for bit and Y = 0, while hi + lo * 2^-11 keeps 22 bits: 2^-22 * max |result|;
    the tiny kind — below 2^-14 hi is flushed and lo = fp16(x * 2048) keeps 11 bits of x, against Y ~ 1e-12: 2^-11 * max |result| (results of
    3e-5: 1.5e-8, half of what a store of fp16(x) alone would lose there, 2^-25)."""
    if key[0] == "att" and key[3] == "tiny":
        return 2.0 ** -11 * float(ref.abs().max())
    if key[0] == "att" and key[2] == 1:
        return 2.0 ** -22 * float(ref.abs().max())
    return 0.0


def gate(key, what=None, ref=None):
    """the bound on max |kernel - float64| of case `key`; `what`: the kernel variant ("sh": a split-half result, which needs `ref`, the float64 result)"""
    g = RAISED.get((key, what), RAISED.get((key[0], what), FACTOR)) * GAPS[key]
    return max(g, format_bound(key, ref)) if what == "sh" else g


def report(key, what, err, ref=None):
    """prints the measured ratio error / Y (the figures of MEASURED) and holds it to the gate"""
    y, bound = GAPS[key], gate(key, what, ref)
    print(f"RATIO {key!r} {what}: error {err:.3e} = {err / y if y else float('inf'):.2f} x Y ({y:.3e}), gate {bound:.3e}")
    assert err <= bound, (key, what, err, y, err / y if y else None)


# factors other than FACTOR, each with the arithmetic that explains it: (case key or its family, kernel variant) -> factor
RAISED = {}

# Y per case, measured by test_transformer_cpu.py's measure() on the CPU
GAPS = {
    ('att', 1, 1, 'unit'): 0.00e+00, ('att', 1, 1, 'sharp'): 0.00e+00, ('att', 1, 1, 'tiny'): 0.00e+00, ('att', 3, 3, 'unit'): 4.29e-07,
    ('att', 3, 3, 'sharp'): 5.42e-06, ('att', 3, 3, 'tiny'): 5.09e-12, ('att', 2, 10, 'unit'): 6.98e-07, ('att', 2, 10, 'sharp'): 8.41e-06,
    ('att', 2, 10, 'tiny'): 9.06e-12, ('att', 1, 18, 'unit'): 6.17e-07, ('att', 1, 18, 'sharp'): 1.50e-05, ('att', 1, 18, 'tiny'): 9.62e-12,
    ('att', 2, 26, 'unit'): 7.06e-07, ('att', 2, 26, 'sharp'): 4.36e-05, ('att', 2, 26, 'tiny'): 1.02e-11, ('att', 1, 46, 'unit'): 8.26e-07,
    ('att', 1, 46, 'sharp'): 2.86e-05, ('att', 1, 46, 'tiny'): 1.09e-11, ('att', 1, 61, 'unit'): 7.29e-07, ('att', 1, 61, 'sharp'): 3.08e-05,
    ('att', 1, 61, 'tiny'): 7.10e-12, ('att', 2, 63, 'unit'): 1.09e-06, ('att', 2, 63, 'sharp'): 4.51e-05, ('att', 2, 63, 'tiny'): 7.44e-12,
    ('att', 1, 64, 'unit'): 7.44e-07, ('att', 1, 64, 'sharp'): 3.44e-05, ('att', 1, 64, 'tiny'): 1.15e-11,
    ('pack', 1, 18, 16, 32): 2.38e-07, ('pack', 3, 10, 16, 32): 2.38e-07, ('pack', 2, 46, 16, 32): 2.38e-07, ('pack', 1, 3, 5, 7): 2.38e-07,
    ('mlp', 10, 10, 1024, False): 8.93e-07, ('mlp', 10, 10, 1024, True): 3.15e-06, ('mlp', 10, 10, 100, False): 5.72e-07,
    ('mlp', 10, 10, 100, True): 3.08e-06, ('mlp', 20, 10, 1024, False): 5.29e-07, ('mlp', 20, 10, 1024, True): 3.72e-06,
    ('mlp', 20, 10, 100, False): 5.85e-07, ('mlp', 20, 10, 100, True): 4.54e-06, ('mlp', 18, 18, 1024, False): 5.76e-07,
    ('mlp', 18, 18, 1024, True): 5.33e-06, ('mlp', 18, 18, 100, False): 6.26e-07, ('mlp', 18, 18, 100, True): 2.66e-06,
    ('mlp', 36, 18, 1024, False): 6.06e-07, ('mlp', 36, 18, 1024, True): 6.01e-06, ('mlp', 36, 18, 100, False): 5.43e-07,
    ('mlp', 36, 18, 100, True): 7.41e-06,
    ('mlp_engine', 'mlp_points1'): 5.43e-07, ('mlp_engine', 'mlp_points2'): 5.28e-06,
    ('ln', 1, 1e-05, 'unit'): 2.51e-07, ('ln', 1, 1e-05, 'offset'): 1.39e-05, ('ln', 1, 1e-05, 'small'): 4.71e-07, ('ln', 1, 1e-06, 'unit'): 4.78e-07,
    ('ln', 1, 1e-06, 'offset'): 4.45e-06, ('ln', 1, 1e-06, 'small'): 3.35e-07, ('ln', 3, 1e-05, 'unit'): 5.14e-07,
    ('ln', 3, 1e-05, 'offset'): 5.51e-06, ('ln', 3, 1e-05, 'small'): 3.21e-07, ('ln', 3, 1e-06, 'unit'): 4.92e-07,
    ('ln', 3, 1e-06, 'offset'): 1.39e-05, ('ln', 3, 1e-06, 'small'): 4.40e-07, ('ln', 4, 1e-05, 'unit'): 4.09e-07,
    ('ln', 4, 1e-05, 'offset'): 1.10e-05, ('ln', 4, 1e-05, 'small'): 3.11e-07, ('ln', 4, 1e-06, 'unit'): 5.17e-07,
    ('ln', 4, 1e-06, 'offset'): 1.44e-05, ('ln', 4, 1e-06, 'small'): 3.39e-07, ('ln', 5, 1e-05, 'unit'): 5.78e-07,
    ('ln', 5, 1e-05, 'offset'): 1.16e-05, ('ln', 5, 1e-05, 'small'): 4.59e-07, ('ln', 5, 1e-06, 'unit'): 4.45e-07,
    ('ln', 5, 1e-06, 'offset'): 8.64e-06, ('ln', 5, 1e-06, 'small'): 4.61e-07, ('ln', 18, 1e-05, 'unit'): 7.69e-07,
    ('ln', 18, 1e-05, 'offset'): 1.28e-05, ('ln', 18, 1e-05, 'small'): 3.72e-07, ('ln', 18, 1e-06, 'unit'): 6.62e-07,
    ('ln', 18, 1e-06, 'offset'): 1.11e-05, ('ln', 18, 1e-06, 'small'): 4.53e-07, ('ln', 37, 1e-05, 'unit'): 6.55e-07,
    ('ln', 37, 1e-05, 'offset'): 1.48e-05, ('ln', 37, 1e-05, 'small'): 5.07e-07, ('ln', 37, 1e-06, 'unit'): 5.40e-07,
    ('ln', 37, 1e-06, 'offset'): 1.57e-05, ('ln', 37, 1e-06, 'small'): 5.13e-07,
    ('parts', 1, 1, False, False): 4.92e-07, ('parts', 1, 1, False, True): 2.79e-07, ('parts', 1, 1, True, False): 2.78e-07,
    ('parts', 1, 1, True, True): 4.20e-07, ('parts', 1, 18, False, False): 5.84e-07, ('parts', 1, 18, False, True): 5.43e-07,
    ('parts', 1, 18, True, False): 6.18e-07, ('parts', 1, 18, True, True): 5.31e-07, ('parts', 1, 32, False, False): 6.79e-07,
    ('parts', 1, 32, False, True): 6.08e-07, ('parts', 1, 32, True, False): 5.75e-07, ('parts', 1, 32, True, True): 8.39e-07,
    ('parts', 1, 50, False, False): 8.00e-07, ('parts', 1, 50, False, True): 7.80e-07, ('parts', 1, 50, True, False): 7.04e-07,
    ('parts', 1, 50, True, True): 7.26e-07, ('parts', 2, 1, False, False): 4.77e-07, ('parts', 2, 1, False, True): 3.73e-07,
    ('parts', 2, 1, True, False): 3.40e-07, ('parts', 2, 1, True, True): 4.59e-07, ('parts', 2, 18, False, False): 6.20e-07,
    ('parts', 2, 18, False, True): 6.42e-07, ('parts', 2, 18, True, False): 6.66e-07, ('parts', 2, 18, True, True): 7.67e-07,
    ('parts', 2, 32, False, False): 6.16e-07, ('parts', 2, 32, False, True): 6.12e-07, ('parts', 2, 32, True, False): 6.00e-07,
    ('parts', 2, 32, True, True): 6.34e-07, ('parts', 2, 50, False, False): 7.05e-07, ('parts', 2, 50, False, True): 7.84e-07,
    ('parts', 2, 50, True, False): 7.73e-07, ('parts', 2, 50, True, True): 1.02e-06, ('parts', 4, 1, False, False): 3.93e-07,
    ('parts', 4, 1, False, True): 5.35e-07, ('parts', 4, 1, True, False): 2.87e-07, ('parts', 4, 1, True, True): 3.87e-07,
    ('parts', 4, 18, False, False): 7.50e-07, ('parts', 4, 18, False, True): 7.79e-07, ('parts', 4, 18, True, False): 5.89e-07,
    ('parts', 4, 18, True, True): 6.72e-07, ('parts', 4, 32, False, False): 6.53e-07, ('parts', 4, 32, False, True): 7.51e-07,
    ('parts', 4, 32, True, False): 8.25e-07, ('parts', 4, 32, True, True): 8.08e-07, ('parts', 4, 50, False, False): 7.23e-07,
    ('parts', 4, 50, False, True): 7.50e-07, ('parts', 4, 50, True, False): 9.90e-07, ('parts', 4, 50, True, True): 6.83e-07,
    ('parts', 8, 1, False, False): 5.91e-07, ('parts', 8, 1, False, True): 2.95e-07, ('parts', 8, 1, True, False): 7.48e-07,
    ('parts', 8, 1, True, True): 3.87e-07, ('parts', 8, 18, False, False): 9.59e-07, ('parts', 8, 18, False, True): 7.32e-07,
    ('parts', 8, 18, True, False): 6.22e-07, ('parts', 8, 18, True, True): 6.77e-07, ('parts', 8, 32, False, False): 8.70e-07,
    ('parts', 8, 32, False, True): 6.59e-07, ('parts', 8, 32, True, False): 8.41e-07, ('parts', 8, 32, True, True): 8.53e-07,
    ('parts', 8, 50, False, False): 8.28e-07, ('parts', 8, 50, False, True): 8.12e-07, ('parts', 8, 50, True, False): 7.56e-07,
    ('parts', 8, 50, True, True): 7.59e-07,
    ('lng', 1, 512, 0, False, False): 7.74e-07, ('lng', 1, 512, 0, False, True): 9.68e-07, ('lng', 1, 512, 0, True, False): 7.75e-07,
    ('lng', 1, 512, 0, True, True): 7.44e-07, ('lng', 1, 512, 2, False, False): 8.45e-07, ('lng', 1, 512, 2, False, True): 9.70e-07,
    ('lng', 1, 512, 2, True, False): 9.40e-07, ('lng', 1, 512, 2, True, True): 6.24e-07, ('lng', 1, 1536, 0, False, False): 8.77e-07,
    ('lng', 1, 1536, 0, False, True): 7.07e-07, ('lng', 1, 1536, 0, True, False): 1.03e-06, ('lng', 1, 1536, 0, True, True): 9.45e-07,
    ('lng', 1, 1536, 2, False, False): 7.23e-07, ('lng', 1, 1536, 2, False, True): 1.07e-06, ('lng', 1, 1536, 2, True, False): 8.58e-07,
    ('lng', 1, 1536, 2, True, True): 9.45e-07, ('lng', 1, 2048, 0, False, False): 7.79e-07, ('lng', 1, 2048, 0, False, True): 8.99e-07,
    ('lng', 1, 2048, 0, True, False): 9.21e-07, ('lng', 1, 2048, 0, True, True): 9.21e-07, ('lng', 1, 2048, 2, False, False): 7.46e-07,
    ('lng', 1, 2048, 2, False, True): 8.86e-07, ('lng', 1, 2048, 2, True, False): 7.38e-07, ('lng', 1, 2048, 2, True, True): 8.00e-07,
    ('lng', 7, 512, 0, False, False): 8.23e-07, ('lng', 7, 512, 0, False, True): 8.97e-07, ('lng', 7, 512, 0, True, False): 9.42e-07,
    ('lng', 7, 512, 0, True, True): 1.05e-06, ('lng', 7, 512, 2, False, False): 7.97e-07, ('lng', 7, 512, 2, False, True): 9.11e-07,
    ('lng', 7, 512, 2, True, False): 7.34e-07, ('lng', 7, 512, 2, True, True): 8.61e-07, ('lng', 7, 1536, 0, False, False): 8.34e-07,
    ('lng', 7, 1536, 0, False, True): 8.34e-07, ('lng', 7, 1536, 0, True, False): 8.34e-07, ('lng', 7, 1536, 0, True, True): 8.34e-07,
    ('lng', 7, 1536, 2, False, False): 9.66e-07, ('lng', 7, 1536, 2, False, True): 9.81e-07, ('lng', 7, 1536, 2, True, False): 8.97e-07,
    ('lng', 7, 1536, 2, True, True): 8.64e-07, ('lng', 7, 2048, 0, False, False): 9.43e-07, ('lng', 7, 2048, 0, False, True): 1.00e-06,
    ('lng', 7, 2048, 0, True, False): 9.43e-07, ('lng', 7, 2048, 0, True, True): 1.05e-06, ('lng', 7, 2048, 2, False, False): 1.02e-06,
    ('lng', 7, 2048, 2, False, True): 1.08e-06, ('lng', 7, 2048, 2, True, False): 1.02e-06, ('lng', 7, 2048, 2, True, True): 1.18e-06,
    ('lng', 8, 512, 0, False, False): 7.54e-07, ('lng', 8, 512, 0, False, True): 8.44e-07, ('lng', 8, 512, 0, True, False): 7.96e-07,
    ('lng', 8, 512, 0, True, True): 8.56e-07, ('lng', 8, 512, 2, False, False): 7.58e-07, ('lng', 8, 512, 2, False, True): 8.04e-07,
    ('lng', 8, 512, 2, True, False): 9.14e-07, ('lng', 8, 512, 2, True, True): 9.38e-07, ('lng', 8, 1536, 0, False, False): 7.77e-07,
    ('lng', 8, 1536, 0, False, True): 8.16e-07, ('lng', 8, 1536, 0, True, False): 8.95e-07, ('lng', 8, 1536, 0, True, True): 8.96e-07,
    ('lng', 8, 1536, 2, False, False): 8.73e-07, ('lng', 8, 1536, 2, False, True): 8.24e-07, ('lng', 8, 1536, 2, True, False): 8.83e-07,
    ('lng', 8, 1536, 2, True, True): 9.25e-07, ('lng', 8, 2048, 0, False, False): 9.19e-07, ('lng', 8, 2048, 0, False, True): 1.04e-06,
    ('lng', 8, 2048, 0, True, False): 1.01e-06, ('lng', 8, 2048, 0, True, True): 1.02e-06, ('lng', 8, 2048, 2, False, False): 9.56e-07,
    ('lng', 8, 2048, 2, False, True): 1.12e-06, ('lng', 8, 2048, 2, True, False): 1.03e-06, ('lng', 8, 2048, 2, True, True): 1.23e-06,
    ('lng', 9, 512, 0, False, False): 7.35e-07, ('lng', 9, 512, 0, False, True): 7.15e-07, ('lng', 9, 512, 0, True, False): 8.13e-07,
    ('lng', 9, 512, 0, True, True): 8.13e-07, ('lng', 9, 512, 2, False, False): 8.02e-07, ('lng', 9, 512, 2, False, True): 7.95e-07,
    ('lng', 9, 512, 2, True, False): 9.01e-07, ('lng', 9, 512, 2, True, True): 9.50e-07, ('lng', 9, 1536, 0, False, False): 9.18e-07,
    ('lng', 9, 1536, 0, False, True): 9.18e-07, ('lng', 9, 1536, 0, True, False): 9.18e-07, ('lng', 9, 1536, 0, True, True): 9.18e-07,
    ('lng', 9, 1536, 2, False, False): 9.96e-07, ('lng', 9, 1536, 2, False, True): 9.88e-07, ('lng', 9, 1536, 2, True, False): 9.18e-07,
    ('lng', 9, 1536, 2, True, True): 9.14e-07, ('lng', 9, 2048, 0, False, False): 8.54e-07, ('lng', 9, 2048, 0, False, True): 1.03e-06,
    ('lng', 9, 2048, 0, True, False): 9.97e-07, ('lng', 9, 2048, 0, True, True): 1.03e-06, ('lng', 9, 2048, 2, False, False): 9.74e-07,
    ('lng', 9, 2048, 2, False, True): 1.02e-06, ('lng', 9, 2048, 2, True, False): 1.02e-06, ('lng', 9, 2048, 2, True, True): 9.97e-07,
    ('lng', 18, 512, 0, False, False): 2.63e-06, ('lng', 18, 512, 0, False, True): 2.68e-06, ('lng', 18, 512, 0, True, False): 2.68e-06,
    ('lng', 18, 512, 0, True, True): 2.73e-06, ('lng', 18, 512, 2, False, False): 2.23e-06, ('lng', 18, 512, 2, False, True): 2.48e-06,
    ('lng', 18, 512, 2, True, False): 2.34e-06, ('lng', 18, 512, 2, True, True): 2.20e-06, ('lng', 18, 1536, 0, False, False): 2.91e-06,
    ('lng', 18, 1536, 0, False, True): 3.00e-06, ('lng', 18, 1536, 0, True, False): 2.99e-06, ('lng', 18, 1536, 0, True, True): 3.11e-06,
    ('lng', 18, 1536, 2, False, False): 2.76e-06, ('lng', 18, 1536, 2, False, True): 2.88e-06, ('lng', 18, 1536, 2, True, False): 3.21e-06,
    ('lng', 18, 1536, 2, True, True): 2.95e-06, ('lng', 18, 2048, 0, False, False): 2.61e-06, ('lng', 18, 2048, 0, False, True): 2.56e-06,
    ('lng', 18, 2048, 0, True, False): 2.51e-06, ('lng', 18, 2048, 0, True, True): 2.56e-06, ('lng', 18, 2048, 2, False, False): 2.58e-06,
    ('lng', 18, 2048, 2, False, True): 2.66e-06, ('lng', 18, 2048, 2, True, False): 2.77e-06, ('lng', 18, 2048, 2, True, True): 2.82e-06,
    ('lng', 31, 512, 0, False, False): 2.94e-06, ('lng', 31, 512, 0, False, True): 2.94e-06, ('lng', 31, 512, 0, True, False): 2.94e-06,
    ('lng', 31, 512, 0, True, True): 2.94e-06, ('lng', 31, 512, 2, False, False): 2.53e-06, ('lng', 31, 512, 2, False, True): 2.88e-06,
    ('lng', 31, 512, 2, True, False): 2.35e-06, ('lng', 31, 512, 2, True, True): 2.45e-06, ('lng', 31, 1536, 0, False, False): 2.67e-06,
    ('lng', 31, 1536, 0, False, True): 2.64e-06, ('lng', 31, 1536, 0, True, False): 2.61e-06, ('lng', 31, 1536, 0, True, True): 2.61e-06,
    ('lng', 31, 1536, 2, False, False): 2.79e-06, ('lng', 31, 1536, 2, False, True): 2.71e-06, ('lng', 31, 1536, 2, True, False): 2.82e-06,
    ('lng', 31, 1536, 2, True, True): 2.61e-06, ('lng', 31, 2048, 0, False, False): 3.14e-06, ('lng', 31, 2048, 0, False, True): 3.23e-06,
    ('lng', 31, 2048, 0, True, False): 3.37e-06, ('lng', 31, 2048, 0, True, True): 3.46e-06, ('lng', 31, 2048, 2, False, False): 3.07e-06,
    ('lng', 31, 2048, 2, False, True): 3.22e-06, ('lng', 31, 2048, 2, True, False): 3.29e-06, ('lng', 31, 2048, 2, True, True): 3.65e-06,
    ('lng', 32, 512, 0, False, False): 2.68e-06, ('lng', 32, 512, 0, False, True): 2.74e-06, ('lng', 32, 512, 0, True, False): 2.62e-06,
    ('lng', 32, 512, 0, True, True): 2.68e-06, ('lng', 32, 512, 2, False, False): 2.40e-06, ('lng', 32, 512, 2, False, True): 2.50e-06,
    ('lng', 32, 512, 2, True, False): 2.32e-06, ('lng', 32, 512, 2, True, True): 2.18e-06, ('lng', 32, 1536, 0, False, False): 3.33e-06,
    ('lng', 32, 1536, 0, False, True): 3.39e-06, ('lng', 32, 1536, 0, True, False): 3.33e-06, ('lng', 32, 1536, 0, True, True): 3.33e-06,
    ('lng', 32, 1536, 2, False, False): 3.60e-06, ('lng', 32, 1536, 2, False, True): 3.80e-06, ('lng', 32, 1536, 2, True, False): 3.45e-06,
    ('lng', 32, 1536, 2, True, True): 3.39e-06, ('lng', 32, 2048, 0, False, False): 2.93e-06, ('lng', 32, 2048, 0, False, True): 2.99e-06,
    ('lng', 32, 2048, 0, True, False): 3.05e-06, ('lng', 32, 2048, 0, True, True): 2.99e-06, ('lng', 32, 2048, 2, False, False): 2.90e-06,
    ('lng', 32, 2048, 2, False, True): 2.98e-06, ('lng', 32, 2048, 2, True, False): 3.28e-06, ('lng', 32, 2048, 2, True, True): 3.35e-06,
    ('slices', 1): 6.53e-07, ('slices', 7): 8.36e-07, ('slices', 8): 7.99e-07, ('slices', 9): 9.56e-07, ('slices', 18): 1.85e-06,
    ('slices', 31): 1.85e-06, ('slices', 32): 1.66e-06,
    ('whole', 18, 1, 10.0): 1.03e-06, ('whole', 18, 1, 1.0): 2.79e-06, ('whole', 18, 2, 10.0): 1.24e-06, ('whole', 18, 2, 1.0): 2.40e-06,
    ('whole', 18, 8, 10.0): 1.49e-06, ('whole', 18, 8, 1.0): 2.46e-06, ('whole', 10, 1, 10.0): 9.96e-07, ('whole', 10, 1, 1.0): 1.75e-06,
    ('whole', 10, 3, 10.0): 1.68e-06, ('whole', 10, 3, 1.0): 2.49e-06, ('whole', 26, 1, 10.0): 1.70e-06, ('whole', 26, 1, 1.0): 2.53e-06,
    ('whole', 46, 1, 10.0): 1.25e-06, ('whole', 46, 1, 1.0): 2.18e-06,
}

# error / Y per case and kernel variant on an MI355X (the RATIO lines of test_transformer_gpu.py); the error itself where Y = 0 (one token).
# The split-half attention of the tiny kind is held to format_bound, not to Y.
MEASURED = {
    ('att', 1, 1, 'unit'): {'f32': 0, 'sh': 2.38e-07}, ('att', 1, 1, 'sharp'): {'f32': 0, 'sh': 2.38e-07},
    ('att', 1, 1, 'tiny'): {'f32': 0, 'sh': 7.32e-09}, ('att', 3, 3, 'unit'): {'f32': 1.06, 'sh': 1.15}, ('att', 3, 3, 'sharp'): {'f32': 1, 'sh': 1},
    ('att', 3, 3, 'tiny'): {'f32': 1.13, 'sh': 1.9e+03}, ('att', 2, 10, 'unit'): {'f32': 0.93, 'sh': 0.93},
    ('att', 2, 10, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 2, 10, 'tiny'): {'f32': 0.97, 'sh': 749}, ('att', 1, 18, 'unit'): {'f32': 1.19, 'sh': 1.19},
    ('att', 1, 18, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 1, 18, 'tiny'): {'f32': 1, 'sh': 689}, ('att', 2, 26, 'unit'): {'f32': 1, 'sh': 1},
    ('att', 2, 26, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 2, 26, 'tiny'): {'f32': 1.09, 'sh': 650}, ('att', 1, 46, 'unit'): {'f32': 1, 'sh': 1.14},
    ('att', 1, 46, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 1, 46, 'tiny'): {'f32': 1, 'sh': 340}, ('att', 1, 61, 'unit'): {'f32': 0.94, 'sh': 1.02},
    ('att', 1, 61, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 1, 61, 'tiny'): {'f32': 1, 'sh': 503}, ('att', 2, 63, 'unit'): {'f32': 1, 'sh': 1},
    ('att', 2, 63, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 2, 63, 'tiny'): {'f32': 1, 'sh': 498}, ('att', 1, 64, 'unit'): {'f32': 1.32, 'sh': 1.32},
    ('att', 1, 64, 'sharp'): {'f32': 1, 'sh': 1}, ('att', 1, 64, 'tiny'): {'f32': 1, 'sh': 322},
    ('mlp', 10, 10, 1024, False): {'f32': 1.29}, ('mlp', 10, 10, 1024, True): {'f32': 0.83}, ('mlp', 10, 10, 100, False): {'f32': 0.91},
    ('mlp', 10, 10, 100, True): {'f32': 1.26}, ('mlp', 20, 10, 1024, False): {'f32': 1.01}, ('mlp', 20, 10, 1024, True): {'f32': 0.98},
    ('mlp', 20, 10, 100, False): {'f32': 0.98}, ('mlp', 20, 10, 100, True): {'f32': 1.12}, ('mlp', 18, 18, 1024, False): {'f32': 1.2},
    ('mlp', 18, 18, 1024, True): {'f32': 1.25}, ('mlp', 18, 18, 100, False): {'f32': 1.06}, ('mlp', 18, 18, 100, True): {'f32': 0.95},
    ('mlp', 36, 18, 1024, False): {'f32': 0.98}, ('mlp', 36, 18, 1024, True): {'f32': 0.74}, ('mlp', 36, 18, 100, False): {'f32': 0.98},
    ('mlp', 36, 18, 100, True): {'f32': 1.02},
    ('mlp_engine', 'mlp_points1'): {'f32': 0.97}, ('mlp_engine', 'mlp_points2'): {'f32': 0.82},
    ('ln', 1, 1e-05, 'unit'): {'f32': 1.45, 'sh': 1.45}, ('ln', 1, 1e-05, 'offset'): {'f32': 0.7, 'sh': 0.7},
    ('ln', 1, 1e-05, 'small'): {'f32': 1, 'sh': 1}, ('ln', 1, 1e-06, 'unit'): {'f32': 1, 'sh': 1},
    ('ln', 1, 1e-06, 'offset'): {'f32': 1.63, 'sh': 1.63}, ('ln', 1, 1e-06, 'small'): {'f32': 1.04, 'sh': 1.95},
    ('ln', 3, 1e-05, 'unit'): {'f32': 0.92, 'sh': 1.78}, ('ln', 3, 1e-05, 'offset'): {'f32': 1.36, 'sh': 1.34},
    ('ln', 3, 1e-05, 'small'): {'f32': 1, 'sh': 1.14}, ('ln', 3, 1e-06, 'unit'): {'f32': 1.4, 'sh': 1.4},
    ('ln', 3, 1e-06, 'offset'): {'f32': 0.79, 'sh': 0.79}, ('ln', 3, 1e-06, 'small'): {'f32': 1.54, 'sh': 2.05},
    ('ln', 4, 1e-05, 'unit'): {'f32': 1.39, 'sh': 1.39}, ('ln', 4, 1e-05, 'offset'): {'f32': 1, 'sh': 1},
    ('ln', 4, 1e-05, 'small'): {'f32': 1.91, 'sh': 1.91}, ('ln', 4, 1e-06, 'unit'): {'f32': 0.87, 'sh': 1.79},
    ('ln', 4, 1e-06, 'offset'): {'f32': 0.35, 'sh': 0.37}, ('ln', 4, 1e-06, 'small'): {'f32': 1, 'sh': 1.47},
    ('ln', 5, 1e-05, 'unit'): {'f32': 1.18, 'sh': 1.18}, ('ln', 5, 1e-05, 'offset'): {'f32': 0.38, 'sh': 0.39},
    ('ln', 5, 1e-05, 'small'): {'f32': 1, 'sh': 1}, ('ln', 5, 1e-06, 'unit'): {'f32': 1.27, 'sh': 1.42},
    ('ln', 5, 1e-06, 'offset'): {'f32': 1.73, 'sh': 1.73}, ('ln', 5, 1e-06, 'small'): {'f32': 0.89, 'sh': 1.51},
    ('ln', 18, 1e-05, 'unit'): {'f32': 0.89, 'sh': 1.51}, ('ln', 18, 1e-05, 'offset'): {'f32': 0.95, 'sh': 0.97},
    ('ln', 18, 1e-05, 'small'): {'f32': 1.02, 'sh': 1.91}, ('ln', 18, 1e-06, 'unit'): {'f32': 1.12, 'sh': 1.24},
    ('ln', 18, 1e-06, 'offset'): {'f32': 0.8, 'sh': 0.82}, ('ln', 18, 1e-06, 'small'): {'f32': 1.54, 'sh': 1.54},
    ('ln', 37, 1e-05, 'unit'): {'f32': 1.16, 'sh': 1.35}, ('ln', 37, 1e-05, 'offset'): {'f32': 0.82, 'sh': 0.82},
    ('ln', 37, 1e-05, 'small'): {'f32': 1.14, 'sh': 1.4}, ('ln', 37, 1e-06, 'unit'): {'f32': 1.64, 'sh': 2.08},
    ('ln', 37, 1e-06, 'offset'): {'f32': 0.74, 'sh': 0.74}, ('ln', 37, 1e-06, 'small'): {'f32': 1.15, 'sh': 1.76},
    ('parts', 1, 1, False, False): {'f32': 0.65, 'sh': 0.87}, ('parts', 1, 1, False, True): {'f32': 1.2, 'sh': 2.51},
    ('parts', 1, 1, True, False): {'f32': 2.07, 'sh': 2.42}, ('parts', 1, 1, True, True): {'f32': 0.92, 'sh': 0.94},
    ('parts', 1, 18, False, False): {'f32': 0.87, 'sh': 1.28}, ('parts', 1, 18, False, True): {'f32': 0.91, 'sh': 1.3},
    ('parts', 1, 18, True, False): {'f32': 1.34, 'sh': 1.77}, ('parts', 1, 18, True, True): {'f32': 1.36, 'sh': 1.36},
    ('parts', 1, 32, False, False): {'f32': 1.1, 'sh': 1.13}, ('parts', 1, 32, False, True): {'f32': 1.01, 'sh': 1.38},
    ('parts', 1, 32, True, False): {'f32': 1.44, 'sh': 1.71}, ('parts', 1, 32, True, True): {'f32': 0.82, 'sh': 0.93},
    ('parts', 1, 50, False, False): {'f32': 0.9, 'sh': 1.36}, ('parts', 1, 50, False, True): {'f32': 1.05, 'sh': 1.42},
    ('parts', 1, 50, True, False): {'f32': 1.11, 'sh': 1.26}, ('parts', 1, 50, True, True): {'f32': 1.12, 'sh': 1.6},
    ('parts', 2, 1, False, False): {'f32': 1.5, 'sh': 1.5}, ('parts', 2, 1, False, True): {'f32': 1, 'sh': 1.29},
    ('parts', 2, 1, True, False): {'f32': 1.31, 'sh': 1.44}, ('parts', 2, 1, True, True): {'f32': 1, 'sh': 1.29},
    ('parts', 2, 18, False, False): {'f32': 1.34, 'sh': 1.34}, ('parts', 2, 18, False, True): {'f32': 1.18, 'sh': 1.18},
    ('parts', 2, 18, True, False): {'f32': 0.97, 'sh': 1.29}, ('parts', 2, 18, True, True): {'f32': 1, 'sh': 1.57},
    ('parts', 2, 32, False, False): {'f32': 1.2, 'sh': 1.31}, ('parts', 2, 32, False, True): {'f32': 1.25, 'sh': 1.7},
    ('parts', 2, 32, True, False): {'f32': 1.3, 'sh': 1.71}, ('parts', 2, 32, True, True): {'f32': 1.16, 'sh': 1.32},
    ('parts', 2, 50, False, False): {'f32': 1.25, 'sh': 1.86}, ('parts', 2, 50, False, True): {'f32': 1, 'sh': 1.13},
    ('parts', 2, 50, True, False): {'f32': 1, 'sh': 1.18}, ('parts', 2, 50, True, True): {'f32': 0.92, 'sh': 0.92},
    ('parts', 4, 1, False, False): {'f32': 1.48, 'sh': 1.48}, ('parts', 4, 1, False, True): {'f32': 1, 'sh': 1},
    ('parts', 4, 1, True, False): {'f32': 1.99, 'sh': 1.99}, ('parts', 4, 1, True, True): {'f32': 1.33, 'sh': 1.33},
    ('parts', 4, 18, False, False): {'f32': 1, 'sh': 1.25}, ('parts', 4, 18, False, True): {'f32': 1, 'sh': 1.1},
    ('parts', 4, 18, True, False): {'f32': 1.05, 'sh': 1.77}, ('parts', 4, 18, True, True): {'f32': 0.91, 'sh': 1.47},
    ('parts', 4, 32, False, False): {'f32': 1.58, 'sh': 1.58}, ('parts', 4, 32, False, True): {'f32': 1, 'sh': 1.26},
    ('parts', 4, 32, True, False): {'f32': 1.29, 'sh': 1.29}, ('parts', 4, 32, True, True): {'f32': 1.03, 'sh': 1.19},
    ('parts', 4, 50, False, False): {'f32': 1.14, 'sh': 1.14}, ('parts', 4, 50, False, True): {'f32': 1.29, 'sh': 1.29},
    ('parts', 4, 50, True, False): {'f32': 0.65, 'sh': 1}, ('parts', 4, 50, True, True): {'f32': 1.09, 'sh': 1.46},
    ('parts', 8, 1, False, False): {'f32': 1, 'sh': 1.23}, ('parts', 8, 1, False, True): {'f32': 0.99, 'sh': 1.87},
    ('parts', 8, 1, True, False): {'f32': 1, 'sh': 1}, ('parts', 8, 1, True, True): {'f32': 1.42, 'sh': 1.42},
    ('parts', 8, 18, False, False): {'f32': 0.99, 'sh': 1.1}, ('parts', 8, 18, False, True): {'f32': 0.93, 'sh': 1.17},
    ('parts', 8, 18, True, False): {'f32': 0.94, 'sh': 1.17}, ('parts', 8, 18, True, True): {'f32': 1.15, 'sh': 1.68},
    ('parts', 8, 32, False, False): {'f32': 0.9, 'sh': 0.97}, ('parts', 8, 32, False, True): {'f32': 0.97, 'sh': 1.41},
    ('parts', 8, 32, True, False): {'f32': 1.11, 'sh': 1.11}, ('parts', 8, 32, True, True): {'f32': 1, 'sh': 1.14},
    ('parts', 8, 50, False, False): {'f32': 1.13, 'sh': 1.15}, ('parts', 8, 50, False, True): {'f32': 1.15, 'sh': 1.15},
    ('parts', 8, 50, True, False): {'f32': 1, 'sh': 1.23}, ('parts', 8, 50, True, True): {'f32': 1.33, 'sh': 1.33},
    ('lng', 1, 512, 0, False, False): {'f32': 0.88, 'sh': 0.91}, ('lng', 1, 512, 0, False, True): {'f32': 0.7, 'sh': 0.7},
    ('lng', 1, 512, 0, True, False): {'f32': 0.89, 'sh': 0.89}, ('lng', 1, 512, 0, True, True): {'f32': 1.19, 'sh': 1.21},
    ('lng', 1, 512, 2, False, False): {'f32': 0.86, 'sh': 0.86}, ('lng', 1, 512, 2, False, True): {'f32': 0.58, 'sh': 0.8},
    ('lng', 1, 512, 2, True, False): {'f32': 0.73, 'sh': 0.82}, ('lng', 1, 512, 2, True, True): {'f32': 1.02, 'sh': 1.47},
    ('lng', 1, 1536, 0, False, False): {'f32': 0.75, 'sh': 0.88}, ('lng', 1, 1536, 0, False, True): {'f32': 0.93, 'sh': 1.32},
    ('lng', 1, 1536, 0, True, False): {'f32': 0.85, 'sh': 0.85}, ('lng', 1, 1536, 0, True, True): {'f32': 0.97, 'sh': 0.97},
    ('lng', 1, 1536, 2, False, False): {'f32': 1.09, 'sh': 1.42}, ('lng', 1, 1536, 2, False, True): {'f32': 0.61, 'sh': 0.8},
    ('lng', 1, 1536, 2, True, False): {'f32': 0.74, 'sh': 0.95}, ('lng', 1, 1536, 2, True, True): {'f32': 0.81, 'sh': 0.81},
    ('lng', 1, 2048, 0, False, False): {'f32': 0.68, 'sh': 0.81}, ('lng', 1, 2048, 0, False, True): {'f32': 0.79, 'sh': 1.21},
    ('lng', 1, 2048, 0, True, False): {'f32': 0.66, 'sh': 0.94}, ('lng', 1, 2048, 0, True, True): {'f32': 0.83, 'sh': 1.14},
    ('lng', 1, 2048, 2, False, False): {'f32': 0.89, 'sh': 1}, ('lng', 1, 2048, 2, False, True): {'f32': 0.76, 'sh': 1.07},
    ('lng', 1, 2048, 2, True, False): {'f32': 1.03, 'sh': 1.44}, ('lng', 1, 2048, 2, True, True): {'f32': 0.98, 'sh': 1.11},
    ('lng', 7, 512, 0, False, False): {'f32': 1.16, 'sh': 1.16}, ('lng', 7, 512, 0, False, True): {'f32': 0.86, 'sh': 1.02},
    ('lng', 7, 512, 0, True, False): {'f32': 1.01, 'sh': 1.51}, ('lng', 7, 512, 0, True, True): {'f32': 1.01, 'sh': 1.16},
    ('lng', 7, 512, 2, False, False): {'f32': 1.31, 'sh': 1.68}, ('lng', 7, 512, 2, False, True): {'f32': 1.05, 'sh': 1.27},
    ('lng', 7, 512, 2, True, False): {'f32': 1.4, 'sh': 1.47}, ('lng', 7, 512, 2, True, True): {'f32': 0.93, 'sh': 1.35},
    ('lng', 7, 1536, 0, False, False): {'f32': 1.1, 'sh': 1.25}, ('lng', 7, 1536, 0, False, True): {'f32': 1.1, 'sh': 1.53},
    ('lng', 7, 1536, 0, True, False): {'f32': 1.1, 'sh': 1.13}, ('lng', 7, 1536, 0, True, True): {'f32': 1.32, 'sh': 1.45},
    ('lng', 7, 1536, 2, False, False): {'f32': 0.98, 'sh': 1.11}, ('lng', 7, 1536, 2, False, True): {'f32': 1, 'sh': 1.49},
    ('lng', 7, 1536, 2, True, False): {'f32': 1.18, 'sh': 1.18}, ('lng', 7, 1536, 2, True, True): {'f32': 1.53, 'sh': 1.53},
    ('lng', 7, 2048, 0, False, False): {'f32': 0.85, 'sh': 1.03}, ('lng', 7, 2048, 0, False, True): {'f32': 0.86, 'sh': 1.09},
    ('lng', 7, 2048, 0, True, False): {'f32': 0.91, 'sh': 1.29}, ('lng', 7, 2048, 0, True, True): {'f32': 1, 'sh': 1.04},
    ('lng', 7, 2048, 2, False, False): {'f32': 0.84, 'sh': 1.1}, ('lng', 7, 2048, 2, False, True): {'f32': 0.84, 'sh': 0.84},
    ('lng', 7, 2048, 2, True, False): {'f32': 0.99, 'sh': 1.1}, ('lng', 7, 2048, 2, True, True): {'f32': 1.03, 'sh': 1.05},
    ('lng', 8, 512, 0, False, False): {'f32': 0.97, 'sh': 1.59}, ('lng', 8, 512, 0, False, True): {'f32': 0.98, 'sh': 1.35},
    ('lng', 8, 512, 0, True, False): {'f32': 1.1, 'sh': 1.27}, ('lng', 8, 512, 0, True, True): {'f32': 1.09, 'sh': 1.09},
    ('lng', 8, 512, 2, False, False): {'f32': 1.19, 'sh': 1.53}, ('lng', 8, 512, 2, False, True): {'f32': 1.14, 'sh': 1.68},
    ('lng', 8, 512, 2, True, False): {'f32': 1.37, 'sh': 1.37}, ('lng', 8, 512, 2, True, True): {'f32': 0.98, 'sh': 0.98},
    ('lng', 8, 1536, 0, False, False): {'f32': 1.18, 'sh': 1.18}, ('lng', 8, 1536, 0, False, True): {'f32': 1.18, 'sh': 1.41},
    ('lng', 8, 1536, 0, True, False): {'f32': 1.03, 'sh': 1.41}, ('lng', 8, 1536, 0, True, True): {'f32': 1.09, 'sh': 1.62},
    ('lng', 8, 1536, 2, False, False): {'f32': 1.05, 'sh': 1.19}, ('lng', 8, 1536, 2, False, True): {'f32': 1.11, 'sh': 1.35},
    ('lng', 8, 1536, 2, True, False): {'f32': 1.27, 'sh': 1.27}, ('lng', 8, 1536, 2, True, True): {'f32': 1.17, 'sh': 1.69},
    ('lng', 8, 2048, 0, False, False): {'f32': 0.86, 'sh': 1.16}, ('lng', 8, 2048, 0, False, True): {'f32': 0.88, 'sh': 1},
    ('lng', 8, 2048, 0, True, False): {'f32': 0.95, 'sh': 1.31}, ('lng', 8, 2048, 0, True, True): {'f32': 0.93, 'sh': 1.28},
    ('lng', 8, 2048, 2, False, False): {'f32': 0.98, 'sh': 1.23}, ('lng', 8, 2048, 2, False, True): {'f32': 0.99, 'sh': 1.14},
    ('lng', 8, 2048, 2, True, False): {'f32': 1.04, 'sh': 1.5}, ('lng', 8, 2048, 2, True, True): {'f32': 0.96, 'sh': 1.14},
    ('lng', 9, 512, 0, False, False): {'f32': 1.26, 'sh': 1.26}, ('lng', 9, 512, 0, False, True): {'f32': 1.19, 'sh': 1.19},
    ('lng', 9, 512, 0, True, False): {'f32': 1.13, 'sh': 1.13}, ('lng', 9, 512, 0, True, True): {'f32': 0.92, 'sh': 1.05},
    ('lng', 9, 512, 2, False, False): {'f32': 1.18, 'sh': 1.18}, ('lng', 9, 512, 2, False, True): {'f32': 1.18, 'sh': 1.26},
    ('lng', 9, 512, 2, True, False): {'f32': 1.16, 'sh': 1.16}, ('lng', 9, 512, 2, True, True): {'f32': 0.8, 'sh': 1.12},
    ('lng', 9, 1536, 0, False, False): {'f32': 0.94, 'sh': 1.01}, ('lng', 9, 1536, 0, False, True): {'f32': 0.97, 'sh': 1.25},
    ('lng', 9, 1536, 0, True, False): {'f32': 1.01, 'sh': 1.09}, ('lng', 9, 1536, 0, True, True): {'f32': 1.01, 'sh': 1.3},
    ('lng', 9, 1536, 2, False, False): {'f32': 0.92, 'sh': 1.1}, ('lng', 9, 1536, 2, False, True): {'f32': 1.01, 'sh': 1.49},
    ('lng', 9, 1536, 2, True, False): {'f32': 0.98, 'sh': 1.29}, ('lng', 9, 1536, 2, True, True): {'f32': 0.96, 'sh': 1.28},
    ('lng', 9, 2048, 0, False, False): {'f32': 1.1, 'sh': 1.42}, ('lng', 9, 2048, 0, False, True): {'f32': 0.91, 'sh': 1.01},
    ('lng', 9, 2048, 0, True, False): {'f32': 1.11, 'sh': 1.11}, ('lng', 9, 2048, 0, True, True): {'f32': 1.02, 'sh': 1.07},
    ('lng', 9, 2048, 2, False, False): {'f32': 0.91, 'sh': 1.19}, ('lng', 9, 2048, 2, False, True): {'f32': 0.96, 'sh': 1.06},
    ('lng', 9, 2048, 2, True, False): {'f32': 1.08, 'sh': 1.08}, ('lng', 9, 2048, 2, True, True): {'f32': 1.1, 'sh': 1.58},
    ('lng', 18, 512, 0, False, False): {'f32': 0.29, 'sh': 0.38}, ('lng', 18, 512, 0, False, True): {'f32': 0.33, 'sh': 0.49},
    ('lng', 18, 512, 0, True, False): {'f32': 0.3, 'sh': 0.44}, ('lng', 18, 512, 0, True, True): {'f32': 0.32, 'sh': 0.42},
    ('lng', 18, 512, 2, False, False): {'f32': 0.41, 'sh': 0.44}, ('lng', 18, 512, 2, False, True): {'f32': 0.45, 'sh': 0.45},
    ('lng', 18, 512, 2, True, False): {'f32': 0.36, 'sh': 0.55}, ('lng', 18, 512, 2, True, True): {'f32': 0.43, 'sh': 0.58},
    ('lng', 18, 1536, 0, False, False): {'f32': 0.3, 'sh': 0.34}, ('lng', 18, 1536, 0, False, True): {'f32': 0.33, 'sh': 0.35},
    ('lng', 18, 1536, 0, True, False): {'f32': 0.3, 'sh': 0.38}, ('lng', 18, 1536, 0, True, True): {'f32': 0.31, 'sh': 0.46},
    ('lng', 18, 1536, 2, False, False): {'f32': 0.33, 'sh': 0.41}, ('lng', 18, 1536, 2, False, True): {'f32': 0.36, 'sh': 0.38},
    ('lng', 18, 1536, 2, True, False): {'f32': 0.3, 'sh': 0.36}, ('lng', 18, 1536, 2, True, True): {'f32': 0.37, 'sh': 0.42},
    ('lng', 18, 2048, 0, False, False): {'f32': 0.36, 'sh': 0.36}, ('lng', 18, 2048, 0, False, True): {'f32': 0.36, 'sh': 0.44},
    ('lng', 18, 2048, 0, True, False): {'f32': 0.38, 'sh': 0.4}, ('lng', 18, 2048, 0, True, True): {'f32': 0.4, 'sh': 0.57},
    ('lng', 18, 2048, 2, False, False): {'f32': 0.35, 'sh': 0.36}, ('lng', 18, 2048, 2, False, True): {'f32': 0.41, 'sh': 0.5},
    ('lng', 18, 2048, 2, True, False): {'f32': 0.34, 'sh': 0.4}, ('lng', 18, 2048, 2, True, True): {'f32': 0.42, 'sh': 0.59},
    ('lng', 31, 512, 0, False, False): {'f32': 0.29, 'sh': 0.45}, ('lng', 31, 512, 0, False, True): {'f32': 0.29, 'sh': 0.33},
    ('lng', 31, 512, 0, True, False): {'f32': 0.34, 'sh': 0.34}, ('lng', 31, 512, 0, True, True): {'f32': 0.32, 'sh': 0.53},
    ('lng', 31, 512, 2, False, False): {'f32': 0.33, 'sh': 0.45}, ('lng', 31, 512, 2, False, True): {'f32': 0.36, 'sh': 0.52},
    ('lng', 31, 512, 2, True, False): {'f32': 0.48, 'sh': 0.48}, ('lng', 31, 512, 2, True, True): {'f32': 0.49, 'sh': 0.64},
    ('lng', 31, 1536, 0, False, False): {'f32': 0.37, 'sh': 0.41}, ('lng', 31, 1536, 0, False, True): {'f32': 0.37, 'sh': 0.4},
    ('lng', 31, 1536, 0, True, False): {'f32': 0.47, 'sh': 0.47}, ('lng', 31, 1536, 0, True, True): {'f32': 0.39, 'sh': 0.51},
    ('lng', 31, 1536, 2, False, False): {'f32': 0.36, 'sh': 0.53}, ('lng', 31, 1536, 2, False, True): {'f32': 0.41, 'sh': 0.49},
    ('lng', 31, 1536, 2, True, False): {'f32': 0.43, 'sh': 0.46}, ('lng', 31, 1536, 2, True, True): {'f32': 0.47, 'sh': 0.55},
    ('lng', 31, 2048, 0, False, False): {'f32': 0.32, 'sh': 0.47}, ('lng', 31, 2048, 0, False, True): {'f32': 0.33, 'sh': 0.35},
    ('lng', 31, 2048, 0, True, False): {'f32': 0.31, 'sh': 0.37}, ('lng', 31, 2048, 0, True, True): {'f32': 0.34, 'sh': 0.48},
    ('lng', 31, 2048, 2, False, False): {'f32': 0.27, 'sh': 0.37}, ('lng', 31, 2048, 2, False, True): {'f32': 0.34, 'sh': 0.37},
    ('lng', 31, 2048, 2, True, False): {'f32': 0.33, 'sh': 0.41}, ('lng', 31, 2048, 2, True, True): {'f32': 0.35, 'sh': 0.43},
    ('lng', 32, 512, 0, False, False): {'f32': 0.33, 'sh': 0.41}, ('lng', 32, 512, 0, False, True): {'f32': 0.32, 'sh': 0.39},
    ('lng', 32, 512, 0, True, False): {'f32': 0.39, 'sh': 0.42}, ('lng', 32, 512, 0, True, True): {'f32': 0.38, 'sh': 0.41},
    ('lng', 32, 512, 2, False, False): {'f32': 0.39, 'sh': 0.39}, ('lng', 32, 512, 2, False, True): {'f32': 0.35, 'sh': 0.41},
    ('lng', 32, 512, 2, True, False): {'f32': 0.4, 'sh': 0.49}, ('lng', 32, 512, 2, True, True): {'f32': 0.49, 'sh': 0.64},
    ('lng', 32, 1536, 0, False, False): {'f32': 0.28, 'sh': 0.34}, ('lng', 32, 1536, 0, False, True): {'f32': 0.28, 'sh': 0.33},
    ('lng', 32, 1536, 0, True, False): {'f32': 0.3, 'sh': 0.38}, ('lng', 32, 1536, 0, True, True): {'f32': 0.37, 'sh': 0.38},
    ('lng', 32, 1536, 2, False, False): {'f32': 0.26, 'sh': 0.3}, ('lng', 32, 1536, 2, False, True): {'f32': 0.3, 'sh': 0.33},
    ('lng', 32, 1536, 2, True, False): {'f32': 0.32, 'sh': 0.42}, ('lng', 32, 1536, 2, True, True): {'f32': 0.36, 'sh': 0.4},
    ('lng', 32, 2048, 0, False, False): {'f32': 0.44, 'sh': 0.44}, ('lng', 32, 2048, 0, False, True): {'f32': 0.47, 'sh': 0.49},
    ('lng', 32, 2048, 0, True, False): {'f32': 0.46, 'sh': 0.46}, ('lng', 32, 2048, 0, True, True): {'f32': 0.51, 'sh': 0.41},
    ('lng', 32, 2048, 2, False, False): {'f32': 0.41, 'sh': 0.52}, ('lng', 32, 2048, 2, False, True): {'f32': 0.39, 'sh': 0.49},
    ('lng', 32, 2048, 2, True, False): {'f32': 0.37, 'sh': 0.44}, ('lng', 32, 2048, 2, True, True): {'f32': 0.42, 'sh': 0.56},
    ('slices', 1): {'1 slices': 0.78, '2 slices': 0.67, '4 slices': 0.67}, ('slices', 7): {'1 slices': 0.7, '2 slices': 0.59, '4 slices': 0.6},
    ('slices', 8): {'1 slices': 1.18, '2 slices': 0.69, '4 slices': 0.65}, ('slices', 9): {'1 slices': 0.91, '2 slices': 0.5, '4 slices': 0.5},
    ('slices', 18): {'1 slices': 0.4, '2 slices': 0.35, '4 slices': 0.35}, ('slices', 31): {'1 slices': 0.39, '2 slices': 0.34, '4 slices': 0.4},
    ('slices', 32): {'1 slices': 0.38, '2 slices': 0.54, '4 slices': 0.35},
    ('whole', 18, 1, 10.0): {'f16x3': 1.01, 'fc2_slices=1': 1.01, 'fc2_slices=2': 0.99, 'fuse_ln=False': 1.01, 'rows_gemm=False': 1.01, 'latency_plan=False': 1.01, 'fp32': 0.99},
    ('whole', 18, 1, 1.0): {'f16x3': 0.54, 'fc2_slices=1': 0.48, 'fc2_slices=2': 0.53, 'fuse_ln=False': 0.48, 'rows_gemm=False': 0.58, 'latency_plan=False': 0.58, 'fp32': 0.6},
    ('whole', 18, 2, 10.0): {'f16x3': 1, 'fp32': 1}, ('whole', 18, 2, 1.0): {'f16x3': 0.66, 'fp32': 0.92}, ('whole', 18, 8, 10.0): {'f16x3': 0.9},
    ('whole', 18, 8, 1.0): {'f16x3': 0.68}, ('whole', 10, 1, 10.0): {'f16x3': 0.85}, ('whole', 10, 1, 1.0): {'f16x3': 0.75},
    ('whole', 10, 3, 10.0): {'f16x3': 0.67}, ('whole', 10, 3, 1.0): {'f16x3': 0.71}, ('whole', 26, 1, 10.0): {'f16x3': 0.52},
    ('whole', 26, 1, 1.0): {'f16x3': 0.59}, ('whole', 46, 1, 10.0): {'f16x3': 0.7}, ('whole', 46, 1, 1.0): {'f16x3': 0.74},
}
