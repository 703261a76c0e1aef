"""GPU: the transformer between layer4 and the decoder, operator by operator, against the float64 restatements of
tests/_transformer_cases.py — the attention kernels, the token pack, mlp_points, the LayerNorm family, the rows GEMMs of a lone panorama
and Engine.transformer as a whole, at the row counts where the kernels take another path (the groups of four queries, the 8-wave boundary,
the limit of 32 rows, four rows per LayerNorm block).

Gate of every float64 comparison: FACTOR * Y of the case (_transformer_cases.gate); bit-equality claims have no tolerance.  Every output
buffer carries NaN-filled rows after its last valid row, which must come back untouched.  Each comparison prints its ratio error / Y
(the RATIO lines; _transformer_cases.MEASURED keeps them)."""
import ctypes

import pytest
import torch

import _transformer_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
OK, INVALID, UNSUPPORTED = 0, 1, 3
PAD = 3                                               # NaN rows behind every output


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
    return torch.full((rows + PAD, cols), float("nan"), device=DEV)


_NAN = torch.full((1,), float("nan")).view(torch.int32).item()


def _untouched(buf, rows):
    """the rows behind the last valid one still hold the fill pattern (compared as bits: the buffer may be a split-half tensor)"""
    assert (buf[rows:].view(torch.int32) == _NAN).all(), "rows past the end were written"


def _f32(lib, t, rows, sh=True):
    """the first `rows` rows of a result as fp32 (decoded from split-half if `sh`)"""
    if not sh:
        return t[:rows]
    o = torch.empty_like(t[:rows])
    assert lib.omni_sh_to_f32(_p(t), _p(o), ctypes.c_size_t(o.numel()), _stream()) == OK
    return o


def _to_sh(lib, x):
    y = torch.empty_like(x)
    assert lib.omni_sh_from_f32(_p(x), _p(y), ctypes.c_size_t(x.numel()), _stream()) == OK
    return y


def _err(got, ref):
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rows_weights(lib, w):
    """w [N, K] -> the fragment-ordered f16x3 operand of the rows GEMMs, and the tile kernel's"""
    from omnifusion_amd.model._engine import split_weights_f16x3
    w16 = split_weights_f16x3(w).to(DEV)
    w16r = torch.empty_like(w16)
    assert lib.omni_gemm_rows_pack(_p(w16), _p(w16r), w.shape[0], w.shape[1], _stream()) == OK, lib.omni_last_error()
    return w16r, w16


# ------------------------------------------------------------------ attention
@pytest.mark.parametrize("kind", tc.ATT_KINDS)
@pytest.mark.parametrize("B,N", tc.ATT_SHAPES)
def test_attention_against_float64(B, N, kind):
    lib = _lib()
    key, M = ("att", B, N, kind), B * N
    qkv = tc.attention_case(B, N, kind)
    ref = tc.attention_qkv(qkv, B, N, F64)
    QKV = _dev(qkv)
    Q, KV = QKV[:, :512].contiguous(), QKV[:, 512:].contiguous()
    o_sh, o_32 = _out(M, 512), _out(M, 512)
    assert lib.omni_attention_qkv_sh(_p(QKV), _p(o_sh), B, N, _stream()) == OK, lib.omni_last_error()
    assert lib.omni_attention_f32(_p(Q), _p(KV), _p(o_32), B, N, _stream()) == OK, lib.omni_last_error()
    a_sh, a_32 = _f32(lib, o_sh, M), _f32(lib, o_32, M, sh=False)
    _untouched(o_sh, M); _untouched(o_32, M)
    tc.report(key, "f32", _err(a_32, ref))
    tc.report(key, "sh", _err(a_sh, ref), ref)
    # the split-half store against the fp32 store of the same kernel: the format's bound (test_sh_elementwise_ops_match_f32)
    bound = 2.0 ** -25 if kind == "tiny" else 2.0 ** -22 * float(a_32.abs().max())
    assert float((a_sh - a_32).abs().max()) <= bound
    if kind == "tiny":
        assert float(ref.abs().max()) < 2.0 ** -14                  # every hi half is flushed ...
        hi = o_sh[:M].view(torch.float16).reshape(M, 16, 2, 32)[:, :, 0]
        assert (hi == 0).all()                                       # ... and the value lives in lo alone
    if kind == "sharp" and N >= 18:                                  # the logits do leave +-100
        q, k = (t.double().reshape(B, N, 4, 128).transpose(1, 2) for t in (qkv[:, :512], qkv[:, 512:1024]))
        assert float((q @ k.transpose(-2, -1)).abs().max()) * tc.SCALE > 100.0


def test_attention_refuses_65_tokens():
    lib = _lib()
    x, o = torch.zeros((65, 1536), device=DEV), _out(65, 512)
    assert lib.omni_attention_qkv_sh(_p(x), _p(o), 1, 65, _stream()) == UNSUPPORTED
    assert lib.omni_attention_f32(_p(x), _p(x), _p(o), 1, 65, _stream()) == UNSUPPORTED
    _untouched(o, 0)


# ------------------------------------------------------------------ token pack
@pytest.mark.parametrize("bs,N,HW,C", tc.PACK_SHAPES)
def test_token_pack_is_one_fp32_add(bs, N, HW, C):
    lib = _lib()
    d, pos = tc.pack_case(bs, N, HW, C)
    M = bs * N
    tok, D, POS = _out(M, HW * C), _dev(d), _dev(pos)
    assert lib.omni_token_pack_f32(_p(D), _p(POS), _p(tok), M, N, HW, C, _stream()) == OK, lib.omni_last_error()
    assert torch.equal(tok[:M].cpu(), tc.token_pack(d, pos, bs, N, torch.float32))
    _untouched(tok, M)


# ------------------------------------------------------------------ mlp_points
@pytest.mark.parametrize("Mo,N,HW,dep", tc.MLP_SHAPES)
def test_mlp_points_against_float64(Mo, N, HW, dep):
    lib = _lib()
    c = tc.mlp_case(Mo, N, HW, dep)
    xyz, depth, w1, b1, w2, b2 = c
    if dep:
        assert (depth == 0).any() and depth[Mo - 1, HW - 1] == 0
    out = _out(Mo * HW, 64)
    XYZ, D, W1, B1, W2, B2 = (_dev(t) for t in c)                     # (held: a pointer outlives no temporary)
    rc = lib.omni_mlp_points_f32(_p(XYZ), _p(D), _p(W1), _p(B1), _p(W2), _p(B2), _p(out), Mo, N, HW, _stream())
    assert rc == OK, lib.omni_last_error()
    tc.report(("mlp", Mo, N, HW, dep), "f32", _err(out[:Mo * HW], tc.mlp_points(*c, Mo, N, F64).reshape(Mo * HW, 64)))
    _untouched(out, Mo * HW)


_ENGINES = {}


def _engine(nrows, N, iterative=False, precision=None):
    """the packed engine of a model with the seeded weights, one per process and configuration"""
    k = (nrows, N, iterative, precision)
    if k not in _ENGINES:
        from omnifusion_amd.model.spherical_model import spherical_fusion
        from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
        from omnifusion_amd.weights import make_state_dict
        net = (spherical_fusion_it if iterative else spherical_fusion)(nrows, N, (128, 128), (80, 80), precision=precision).cuda()
        net.load_state_dict(make_state_dict(tc.WHOLE_SEED, N, iterative))
        net._sync_packed(torch.device(DEV))
        _ENGINES[k] = (net, net._eng)
    return _ENGINES[k][1]


@pytest.mark.parametrize("name", tc.MLP_ENGINE)
def test_engine_mlp_points_folds_the_batchnorms(name):
    """Engine.mlp_points of an iterative engine (weights folded by Engine.pack) against the oracle's conv -> BatchNorm -> ReLU in float64"""
    eng = _engine(4, 18, iterative=True)
    xyz, depth, Mo = tc.mlp_engine_case(name)
    out = eng.mlp_points(name, _dev(xyz), _dev(depth), Mo)
    assert out.shape == (Mo, 32, 32, 64)
    tc.report(("mlp_engine", name), "f32", _err(out, tc.mlp_engine_ref(name, F64)))


# ------------------------------------------------------------------ LayerNorm family
@pytest.mark.parametrize("eps", tc.LN_EPS)
@pytest.mark.parametrize("rows", tc.LN_ROWS)
def test_layernorm_against_float64(rows, eps):
    lib = _lib()
    for kind in tc.LN_KINDS:
        x, g, b = tc.ln_case(rows, eps, kind)
        X, G, B = _dev(x), _dev(g), _dev(b)
        y32, ysh = _out(rows, 512), _out(rows, 512)
        assert lib.omni_layernorm512_f32(_p(X), _p(G), _p(B), _p(y32), rows, ctypes.c_float(eps), _stream()) == OK, lib.omni_last_error()
        assert lib.omni_layernorm512_sh(_p(X), _p(G), _p(B), _p(ysh), rows, ctypes.c_float(eps), _stream()) == OK, lib.omni_last_error()
        a32, ash = _f32(lib, y32, rows, sh=False), _f32(lib, ysh, rows)
        _untouched(y32, rows); _untouched(ysh, rows)
        if kind == "const":                                          # x - mean is 0 exactly: the result is the bias, whatever eps
            assert torch.equal(a32.cpu(), b.expand(rows, 512))
            assert torch.equal(ash.cpu(), tc.sh_value(b).float().expand(rows, 512))
            continue
        ref = tc.layernorm(x, g, b, eps, F64)
        tc.report(("ln", rows, eps, kind), "f32", _err(a32, ref))
        tc.report(("ln", rows, eps, kind), "sh", _err(ash, ref), ref)


@pytest.mark.parametrize("rows", tc.PARTS_ROWS)
@pytest.mark.parametrize("nparts", tc.PARTS_N)
def test_splitk_reduce_ln512(nparts, rows):
    """tok: the fp32 sum in the documented order (slices, then bias, then residual), bit for bit; y: the bits of omni_layernorm512_sh / _f32 on
    that tok, and the float64 LayerNorm of the float64 sum within the gate."""
    lib = _lib()
    for has_bias in (False, True):
        for has_res in (False, True):
            key = ("parts", nparts, rows, has_bias, has_res)
            parts, bias, res, g, b = tc.parts_case(nparts, rows, has_bias, has_res)
            P, Bi, R, G, Bt = _dev(parts), _dev(bias), _dev(res), _dev(g), _dev(b)
            want_tok = tc.parts_sum(parts, bias, res, torch.float32)
            _, ref = tc.parts_layernorm(parts, bias, res, g, b, tc.PARTS_EPS, F64)
            for fmt in (0, 1):
                tok, y, y2 = _out(rows, 512), _out(rows, 512), _out(rows, 512)
                rc = lib.omni_splitk_reduce_ln512(_p(P), nparts, _p(Bi), _p(R), _p(tok), _p(G), _p(Bt), ctypes.c_float(tc.PARTS_EPS), _p(y), fmt, rows, _stream())
                assert rc == OK, lib.omni_last_error()
                assert torch.equal(tok[:rows].cpu(), want_tok), (key, fmt)
                ln = lib.omni_layernorm512_sh if fmt else lib.omni_layernorm512_f32
                assert ln(_p(tok), _p(G), _p(Bt), _p(y2), rows, ctypes.c_float(tc.PARTS_EPS), _stream()) == OK
                assert _same_bits(y[:rows], y2[:rows]), (key, fmt)
                _untouched(tok, rows); _untouched(y, rows)
                tc.report(key, "sh" if fmt else "f32", _err(_f32(lib, y, rows, sh=bool(fmt)), ref), ref)


# ------------------------------------------------------------------ the rows GEMMs of a lone panorama
@pytest.mark.parametrize("N", tc.LNG_N)
@pytest.mark.parametrize("rows", tc.GEMM_ROWS)
def test_gemm_rows_ln_is_the_two_calls_and_float64(rows, N):
    """omni_gemm_rows_ln_sh_f16x3: the bits of omni_layernorm512_sh + omni_gemm_rows_sh_f16x3 (as include/omnifusion.h promises), and the float64
    LayerNorm + Linear within the gate; bias, residual, GELU and a split-half result in every combination."""
    lib = _lib()
    x, g, b, w, bias, res = tc.lng_case(rows, N)
    X, G, Bt, Bi, R = _dev(x), _dev(g), _dev(b), _dev(bias), _dev(res)
    W16R, _ = _rows_weights(lib, w)
    xs = _out(rows, 512)
    assert lib.omni_layernorm512_sh(_p(X), _p(G), _p(Bt), _p(xs), rows, ctypes.c_float(tc.LNG_EPS), _stream()) == OK
    for act, has_bias, has_res in tc.LNG_OPTIONS:
        ref = tc.ln_linear(x, g, b, tc.LNG_EPS, w, bias if has_bias else None, res if has_res else None, act, F64)
        bp, rp = _p(Bi) if has_bias else None, _p(R) if has_res else None
        for fmt in (0, 1):
            one, two = _out(rows, N), _out(rows, N)
            rc = lib.omni_gemm_rows_ln_sh_f16x3(_p(X), _p(G), _p(Bt), ctypes.c_float(tc.LNG_EPS), _p(W16R), bp, rp, _p(one), fmt, rows, N, act, _stream())
            assert rc == OK, lib.omni_last_error()
            assert lib.omni_gemm_rows_sh_f16x3(_p(xs), _p(W16R), bp, rp, _p(two), fmt, rows, 512, N, act, _stream()) == OK, lib.omni_last_error()
            assert _same_bits(one[:rows], two[:rows]), (act, has_bias, has_res, fmt)
            _untouched(one, rows); _untouched(two, rows)
            tc.report(("lng", rows, N, act, has_bias, has_res), "sh" if fmt else "f32", _err(_f32(lib, one, rows, sh=bool(fmt)), ref), ref)
    o = _out(33, N)
    assert lib.omni_gemm_rows_ln_sh_f16x3(_p(X), _p(G), _p(Bt), ctypes.c_float(tc.LNG_EPS), _p(W16R), None, None, _p(o), 0, 33, N, 0, _stream()) == INVALID
    _untouched(o, 0)


@pytest.mark.parametrize("rows", tc.GEMM_ROWS)
def test_gemm_rows_slices(rows):
    """fc2 in K slices: the slices' sum + bias against float64 and against the unsliced rows GEMM (1e-5: the rows-vs-tile figure of test_gemm_rows_vs_torch)"""
    lib = _lib()
    x, w, bias = tc.slices_case(rows)
    ref = tc.linear(x, w, bias, None, 0, F64)
    XS, Bi = _to_sh(lib, _dev(x)), _dev(bias)
    W16R, _ = _rows_weights(lib, w)
    whole = _out(rows, 512)
    assert lib.omni_gemm_rows_sh_f16x3(_p(XS), _p(W16R), _p(Bi), None, _p(whole), 0, rows, 2048, 512, 0, _stream()) == OK, lib.omni_last_error()
    _untouched(whole, rows)
    for S in tc.SLICES:
        parts = _out(S * rows, 512)
        assert lib.omni_gemm_rows_slices_sh_f16x3(_p(XS), _p(W16R), _p(parts), rows, 2048, 512, S, _stream()) == OK, lib.omni_last_error()
        _untouched(parts, S * rows)
        total = parts[:rows].clone()
        for s in range(1, S):
            total += parts[s * rows:(s + 1) * rows]
        total += Bi
        tc.report(("slices", rows), f"{S} slices", _err(total, ref))
        assert float((total - whole[:rows]).abs().max()) < 1e-5
    parts = _out(4 * rows, 512)
    assert lib.omni_gemm_rows_slices_sh_f16x3(_p(XS), _p(W16R), _p(parts), rows, 2048, 512, 3, _stream()) == UNSUPPORTED
    assert lib.omni_gemm_rows_slices_sh_f16x3(_p(XS), _p(W16R), _p(parts), rows, 512, 512, 1, _stream()) == UNSUPPORTED
    _untouched(parts, 0)


@pytest.mark.parametrize("rows", tc.GEMM_ROWS)
@pytest.mark.parametrize("nparts", tc.PARTS_N)
def test_gemm_rows_ln_parts(nparts, rows):
    """norm1 + qkv on a token matrix that still is K slices: xout is the ordered fp32 sum bit for bit, dst the bits of omni_gemm_rows_ln_sh_f16x3 on it"""
    lib = _lib()
    parts, pbias, pres, g, b, w = tc.lnparts_case(nparts, rows)
    P, G, Bt = _dev(parts), _dev(g), _dev(b)
    W16R, _ = _rows_weights(lib, w)
    eps = ctypes.c_float(1e-5)
    for has_bias, has_res, fmt in ((True, True, 0), (False, False, 1), (True, False, 0), (False, True, 1)):
        bi, rs = pbias if has_bias else None, pres if has_res else None
        Bi, Rs = _dev(bi), _dev(rs)
        xout, dst, two = _out(rows, 512), _out(rows, 1536), _out(rows, 1536)
        rc = lib.omni_gemm_rows_ln_parts_sh_f16x3(_p(P), nparts, _p(Bi), _p(Rs), _p(xout), _p(G), _p(Bt), eps, _p(W16R), None, _p(dst), fmt, rows, 1536, 0, _stream())
        assert rc == OK, lib.omni_last_error()
        assert torch.equal(xout[:rows].cpu(), tc.parts_sum(parts, bi, rs, torch.float32)), (has_bias, has_res)
        assert lib.omni_gemm_rows_ln_sh_f16x3(_p(xout), _p(G), _p(Bt), eps, _p(W16R), None, None, _p(two), fmt, rows, 1536, 0, _stream()) == OK, lib.omni_last_error()
        assert _same_bits(dst[:rows], two[:rows]), (has_bias, has_res, fmt)
        _untouched(xout, rows); _untouched(dst, rows)
    xout, dst = _out(rows, 512), _out(rows, 1536)
    P9 = torch.zeros((9, rows, 512), device=DEV)
    assert lib.omni_gemm_rows_ln_parts_sh_f16x3(_p(P9), 9, None, None, _p(xout), _p(G), _p(Bt), eps, _p(W16R), None, _p(dst), 0, rows, 1536, 0, _stream()) == INVALID
    _untouched(xout, 0); _untouched(dst, 0)


# ------------------------------------------------------------------ Engine.transformer
def _whole(nrows, N, bs, std, what, precision=None):
    eng = _engine(nrows, N, precision=precision)
    got = eng.transformer(_dev(tc.whole_case(N, bs, std)), bs)
    assert got.shape == (bs * N, 512) and got.dtype == torch.float32
    tc.report(("whole", N, bs, std), what, _err(got, tc.whole_run(N, bs, std, F64)))
    return got


@pytest.mark.parametrize("std", tc.WHOLE_STD)
@pytest.mark.parametrize("nrows,N,bs", tc.WHOLE_SHAPES)
def test_transformer_against_float64(nrows, N, bs, std):
    _whole(nrows, N, bs, std, "f16x3")


@pytest.mark.parametrize("std", tc.WHOLE_STD)
@pytest.mark.parametrize("switch,value", [("fc2_slices", 1), ("fc2_slices", 2), ("fuse_ln", False), ("rows_gemm", False), ("latency_plan", False)])
def test_transformer_of_a_lone_panorama_under_every_switch(switch, value, std):
    from omnifusion_amd.model._engine import Engine
    default = getattr(Engine, switch)
    try:
        setattr(Engine, switch, value)
        _whole(4, 18, 1, std, f"{switch}={value}")
    finally:
        setattr(Engine, switch, default)


@pytest.mark.parametrize("std", tc.WHOLE_STD)
@pytest.mark.parametrize("bs", [1, 2])
def test_transformer_fp32_precision(bs, std):
    _whole(4, 18, bs, std, "fp32", precision="fp32")
