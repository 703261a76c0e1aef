"""CPU: the reference side of tests/test_glue_float64_gpu.py — the host model of the split-half format against the same format built by another route
and its two error bounds, the float64 restatements of tests/_glue_cases.py against stock torch, the arithmetic of the case tables — and the
argument checks of the csrc/omni_net.hip entry points, which refuse before any launch (no device is touched)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _glue_cases as gc

F64 = torch.float64


# ------------------------------------------------------------------ the SH host model
def test_sh_model_is_the_weight_split_built_by_another_route():
    """split_weights_f16x3 writes the same format with torch's half conversion; [Cout][K/32][2][32] is the layout of a [Cout, K] SH tensor"""
    from omnifusion_amd.model._engine import split_weights_f16x3
    w = torch.randn((64, 192), generator=gc.gen("weights")) * torch.logspace(-7, 4, 192)[None, :]          # from far below 2^-14 to 1e4
    w[0, :4] = torch.tensor([2.0 ** -14, -2.0 ** -14, float(np.nextafter(np.float32(2.0 ** -14), np.float32(0))), 0.0])
    w16 = split_weights_f16x3(w)
    assert gc.same_bits(gc.sh_pack(w), w16.reshape(64, 192 * 2).view(torch.float32))
    hi, lo = w16[:, :, 0, :].reshape(64, 192), w16[:, :, 1, :].reshape(64, 192)
    assert torch.equal(gc.sh_unpack(gc.sh_pack(w)), torch.addcmul(hi.float(), lo.float(), torch.tensor(2.0 ** -11)))
    assert (hi[0, :4] == torch.tensor([2.0 ** -14, -2.0 ** -14, 0.0, 0.0]).half()).all()                  # the threshold is |x| < 2^-14


def test_sh_model_layout_saturation_and_fixed_point():
    x = torch.arange(64, dtype=torch.float32).reshape(1, 64) + 0.5 + 2.0 ** -13
    h = gc.sh_pack(x).numpy().view(np.float16).reshape(2, 2, 32)                                         # [group][hi | lo][32]
    assert (h[:, 0].astype(np.float32).reshape(-1) == np.float16(x.numpy().reshape(-1))).all()
    assert h[0, 1, 1] == np.float16((1.5 + 2.0 ** -13 - float(np.float16(1.5 + 2.0 ** -13))) * 2048.0) and h[0, 1, 1] != 0
    inf = np.float32(np.inf)
    v = gc.sh_join(*gc.sh_split(np.array([inf, -inf, 7e4, -7e4, 65504.0, 65519.996, np.nan], np.float32)))
    assert v[:6].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, 65504.0] and np.isnan(v[6])
    # a store of a stored value changes no byte (what the pool, the adds and the identity up-sampling rely on)
    p, val = gc.sh_canonical(torch.randn((4096, 32), generator=gc.gen("fixed point")) * 3.0)
    assert gc.same_bits(gc.sh_pack(val), p) and torch.equal(gc.sh_unpack(p), val)
    # ... which split(x) alone does not promise: hi odd, lo rounds up to half an ulp of hi, the joined value is a tie
    t = torch.full((1, 32), float(np.float32(1.0 + 2.0 ** -10 + 2.0 ** -11 - 2.0 ** -23)))
    assert not gc.same_bits(gc.sh_pack(gc.sh_unpack(gc.sh_pack(t))), gc.sh_pack(t))
    assert torch.equal(gc.sh_unpack(gc.sh_pack(gc.sh_unpack(gc.sh_pack(t)))), gc.sh_unpack(gc.sh_pack(t)))


def test_sh_sweep_holds_what_it_says():
    x = gc.sh_sweep()
    assert len(x) % 32 == 0 and len(x) >= 256 * 2 * (5 + gc.SWEEP_MANTISSAS)
    b = x.view(np.uint32)
    assert set(((b >> 23) & 0xFF).tolist()) == set(range(256)) and set((b >> 31).tolist()) == {0, 1}
    for m in (0, 1, 0x7FFFFF, 0x1000, 0x3000):
        assert (((b & 0x7FFFFF) == m).sum()) >= 512
    normal, den, nan = gc.sweep_classes(x)
    assert normal.sum() > 500000 and den.sum() > 2000 and nan.sum() > 2000
    for v in (2.0 ** -14, -2.0 ** -14, 65504.0, 65520.0, np.inf, -np.inf, float(np.finfo(np.float32).max)):
        assert (x == np.float32(v)).any(), v
    assert (np.signbit(x) & (x == 0)).any()


def test_sh_bounds():
    """Q and A of the other sections, from the model alone.  Q: x in [2^-14, 2^-13) leaves a remainder below 2^-25, which lo holds as an fp16
    denormal of spacing 2^-24 / 2048: an error of up to 2^-36 on 2^-14, 2^-22; two binades up lo is normal and the error 2^-23 of x.  A: below 2^-14
    hi = 0 and lo = fp16(2048 x) keeps eleven bits: half an ulp of [2^-4, 2^-3) over 2048 = 2^-26, attained at a tie."""
    q, a = gc.sh_bounds()
    print(f"GLUE sh format: Q = {q:.6e} = 2^{math.log2(q):.4f} (largest relative error on [2^-14, 65504]); A = {a:.6e} = 2^{math.log2(a):.4f} (largest absolute error below 2^-14)")
    assert 2.0 ** -22 * (1 - 2.0 ** -9) < q <= 2.0 ** -22
    assert a == 2.0 ** -26
    # the sweep's own values stay inside both, and fp32 denormals inside 2^-36 (the device may flush them)
    x = gc.sh_sweep()
    normal, den, nan = gc.sweep_classes(x)
    v = gc.sh_join(*gc.sh_split(x)).astype(np.float64)
    big = normal & (np.abs(x) >= 2.0 ** -14) & (np.abs(x) <= 65504.0)
    small = normal & (np.abs(x) < 2.0 ** -14)
    assert (np.abs(v[big] - x[big]) <= q * np.abs(x[big])).all() and (np.abs(v[small] - x[small]) <= a).all()
    assert (np.abs(v[den] - x[den]) <= 2.0 ** -36).all() and np.isnan(v[nan]).all()
    # value-only faults of the format move the model's own numbers: the threshold doubled ...
    q2, _ = gc.sh_bounds(2.0 ** -13)
    assert q2 > 64 * q
    x = np.float32(1.5 * 2.0 ** -14)
    assert not np.array_equal(gc.sh_split(np.array([x]), np.float32(2.0 ** -13))[0], gc.sh_split(np.array([x]))[0])


# ------------------------------------------------------------------ the restatements against stock torch
@pytest.mark.parametrize("M,P", gc.STEM_F32_CASES + gc.STEM_MM_CASES[:3])
def test_stem_restatement(M, P):
    x, w, b = gc.stem_case(M, P)
    assert (gc.stem(x, w, b, F64) - gc.stem_reference(M, P)[0]).abs().max().item() < 1e-12
    assert float(w.std()) < 1.2 / math.sqrt(147.0)
    # both weight layouts come from the one [64, 3, 7, 7] tensor
    wt = gc.stem_weights_f32(w)
    assert wt.shape == (147, 64) and wt[(2 * 7 + 5) * 3 + 1, 9] == w[9, 1, 2, 5]
    W16 = gc.stem_weights_f16x3(w)
    we = (W16[:, :, 0, :].double() + W16[:, :, 1, :].double() * 2.0 ** -11).reshape(64, 192)
    assert abs(float(we[9, (1 * 7 + 2) * 8 + 5]) - float(w[9, 1, 2, 5])) <= gc.sh_bounds()[0] * abs(float(w[9, 1, 2, 5])) + 2.0 ** -26
    assert (we[:, 168:] == 0).all() and (we[:, 7:168:8] == 0).all()
    # the bias matters at the gate: dropping it moves the reference by far more
    ref = gc.stem_reference(M, P)[0]
    assert gc.nerr(gc.stem(x, w, None, F64), ref) > 100 * max(gc.gate(gc.stem_reference(M, P)[1], ref, sh=True), gc.CONV_GATE)


@pytest.mark.parametrize("kind", gc.POOL_KINDS)
@pytest.mark.parametrize("M,H,W,C", gc.POOL_CASES)
def test_pool_restatement(M, H, W, C, kind):
    _, v = gc.pool_case(M, H, W, C, kind)
    clean = torch.where(torch.isnan(v), torch.full_like(v, -math.inf), v)
    assert torch.equal(gc.maxpool(v, F64), gc.maxpool_stock(clean, F64))
    assert torch.equal(gc.maxpool(v, torch.float32), gc.maxpool_stock(clean, torch.float32))
    assert not torch.isnan(gc.maxpool(v, F64)).any() and torch.isfinite(gc.maxpool(v, F64)).all()
    if kind == "negative":
        assert float(gc.maxpool(v, F64).max()) <= -1.0
        # an initial value or a padding of 0 would win every window of this map
        assert (gc.maxpool(v, F64, pad_value=0.0) != gc.maxpool(v, F64)).any()


def test_pool_cases_reach_every_border_and_the_special_values():
    sides = set()
    for M, H, W, C in gc.POOL_CASES:
        s = gc.pool_padded_sides(H, W)
        sides |= s
        _, v = gc.pool_case(M, H, W, C, "negative")
        y, y0 = gc.maxpool(v, F64), gc.maxpool(v, F64, pad_value=0.0)
        Ho, Wo = y.shape[1:3]
        rows = {"top": y0[:, 0], "left": y0[:, :, 0], "bottom": y0[:, Ho - 1], "right": y0[:, :, Wo - 1]}
        for side in s:                                               # there, zero padding does win
            assert (rows[side] == 0).all() and (y < 0).all(), (M, H, W, C, side)
    assert sides == {"top", "left", "bottom", "right"}
    assert gc.pool_padded_sides(7, 9) == {"top", "left", "bottom", "right"} and gc.pool_padded_sides(8, 8) == {"top", "left"}
    v = gc.pool_case(*gc.POOL_EXTREME, "randn")[1]
    assert float(v.max()) == 65504.0 and float(v.min()) == -65504.0
    v = gc.pool_case(*gc.POOL_NAN, "randn")[1]
    assert int(torch.isnan(v).sum()) == 1
    assert torch.isnan(gc.maxpool_stock(v, F64)).sum() >= 2          # torch propagates it: the restatement's rule is the kernel's, d43


@pytest.mark.parametrize("M,H,W,C,Ho,Wo", gc.UP_SH_CASES + gc.UP_F32_CASES)
def test_upsample_restatement(M, H, W, C, Ho, Wo):
    _, v = gc.up_case(M, H, W, C, C % 32 == 0)
    assert (gc.upsample(v, Ho, Wo, F64) - gc.upsample_stock(v, Ho, Wo, F64)).abs().max().item() < 1e-12
    if (Ho, Wo) == (H, W) or (M, H, W, C) in gc.UP_IDENTITY_CASES:
        assert torch.equal(gc.upsample(v, H, W, F64), v.double())


@pytest.mark.parametrize("M,P,conf", gc.HEADS_CASES[:3])
def test_heads_restatement(M, P, conf):
    for sharp in (False, True):
        x, w, bp, bw = gc.heads_case(M, P, sharp)
        a, c, z = gc.heads(x, w, bp, bw, conf, F64)
        a0, c0 = gc.heads_stock(x, w, bp, bw, conf, F64)
        assert (a - a0).abs().max().item() < 1e-12 and (c - c0).abs().max().item() < 1e-12
        if sharp:                                                    # beyond +-89 expf overflows float32: the sigmoid must still give 0 and 1
            assert float(z[..., 1].max()) > 95 and float(z[..., 1].min()) < -95
            assert float(c.max()) == 1.0 and float(c.min()) < 1e-40


def test_adds_restatement():
    for M, HW, C in gc.ADD_HW_CASES + gc.ADD_SH_CASES:
        x, y = gc.add_case("hw", (M, HW, C), (M, C))
        want = torch.stack([x[m] + y[m].expand(HW, C) for m in range(M)])
        assert torch.equal(gc.add_hw(x, y), want)
    for total, period in gc.ADD_PERIOD_CASES:
        x, y = gc.add_case("period", (total,), (period,))
        want = torch.tensor([x[i] + y[i % period] for i in range(0, total, 97)])
        assert torch.equal(gc.add_period(x, y)[::97], want)
    for M, HW, C in gc.ADD_SH_CASES:
        assert add_sh_quads(M, HW, C) > 0
    assert any(add_sh_quads(*c) % 256 for c in gc.ADD_SH_CASES) and {c[2] for c in gc.ADD_SH_CASES} == {32, 96}


def add_sh_quads(M, HW, C):
    return M * HW * C // 4


# ------------------------------------------------------------------ the arithmetic of the case tables
def test_stated_tile_counts_follow_from_the_tables():
    L = gc.stem_launch
    assert [L(M, P)["split"] for M, P in gc.STEM_MM_CASES] == [1, 2, 1, 2, 1, 1]
    assert L(3, 96)["tps"] == 3 and L(3, 96)["tpb"] == 3 and L(70, 64)["strips"] == 280
    a = L(301, 32)
    assert (a["ntiles"], a["tpb"], a["blocks"], a["last"]) == (602, 3, 201, 2) and a["tps"] == 1
    assert 2 * 3 % 2 == 0 and 3 % 2 != 0                            # two tiles an image, three a block: every second block straddles two images
    b = L(131, 64)
    assert (b["ntiles"], b["tpb"], b["blocks"], b["last"]) == (1048, 5, 210, 3) and b["tps"] == 2 and b["strips"] == 524
    assert 5 % b["tps"] != 0 and 5 % (b["tps"] * 4) != 0            # five tiles a block: not whole strips (2 tiles), not whole images (8 tiles)
    for M, P in gc.STEM_MM_CASES:                                    # on any CU count every tile belongs to exactly one block
        for ncu in (1, 64, 256, 304, 4096):
            c = L(M, P, ncu)
            assert (c["blocks"] - 1) * c["tpb"] < c["ntiles"] <= c["blocks"] * c["tpb"] and 1 <= c["last"] <= c["tpb"]
    assert gc.heads_tiles(49, 64) == (784, 768, 16) and gc.heads_tiles(2, 8) == (2, 2, 0)
    assert [P % 16 for _, P, _ in gc.HEADS_CASES] == [8, 8, 8, 0]
    assert max(M * (P // 2) ** 2 * 64 * 4 for M, P in gc.STEM_MM_CASES) == 131 * 32 * 32 * 64 * 4 < 35e6


# ------------------------------------------------------------------ refusals: OMNI_ERR_INVALID before any launch
def test_net_entry_points_refuse_bad_arguments():
    """Null tensors, dimensions below 1, C % 4, period 0, token counts below 1.  The non-null pointers below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z, INV = ctypes.c_void_p(4096), None, _lib.OMNI_ERR_INVALID
    f = ctypes.c_float(0.0)

    def refused(fn, *args, word=None):
        assert fn(*args, z) == INV, (fn.__name__, args)
        assert word is None or word in L.omni_last_error(), (fn.__name__, args, L.omni_last_error())

    def sweep(fn, ptrs, dims, optional=(), tail=()):
        """every pointer null in turn (but the optional ones), every dimension 0 and -1 in turn"""
        for i in range(len(ptrs)):
            if i not in optional:
                refused(fn, *[z if j == i else p for j in range(len(ptrs))], *dims, *tail, word=b"null")
        for i in range(len(dims)):
            for bad in (0, -1):
                refused(fn, *ptrs, *[bad if j == i else d for j, d in enumerate(dims)], *tail)

    P4, P2, P3 = (p,) * 4, (p,) * 2, (p,) * 3
    sweep(L.omni_stem_f32, P4, (2, 32))
    sweep(L.omni_stem_sh, P4, (2, 32))
    for fn, C in ((L.omni_maxpool3x3s2_f32, 8), (L.omni_maxpool3x3s2_sh, 32)):
        sweep(fn, P2, (2, 8, 8, C))
    for fn, C in ((L.omni_upsample_bilinear_f32, 8), (L.omni_upsample_bilinear_sh, 32)):
        sweep(fn, P2, (2, 8, 8, C, 16, 16))
    for C in (6, 2, 33, 7):                                          # C / 4 channels quads would leave channels unwritten
        refused(L.omni_maxpool3x3s2_f32, p, p, 2, 8, 8, C, word=b"multiple of 4")
        refused(L.omni_upsample_bilinear_f32, p, p, 2, 8, 8, C, 16, 16, word=b"multiple of 4")
    for C in (8, 48):
        refused(L.omni_maxpool3x3s2_sh, p, p, 2, 8, 8, C)
        refused(L.omni_upsample_bilinear_sh, p, p, 2, 8, 8, C, 16, 16)
        refused(L.omni_add_hw_sh, p, p, 2, 8, C)
    sweep(L.omni_add_hw_f32, P2, (2, 8, 8))
    sweep(L.omni_add_hw_sh, P2, (2, 8, 32))
    for fn in (L.omni_add_period_f32, L.omni_add_period_sh):
        refused(fn, z, p, 64, 32, word=b"null")
        refused(fn, p, z, 64, 32, word=b"null")
        refused(fn, p, p, 64, 0, word=b"period")                     # i % period
        refused(fn, p, p, 0, 32)
    for total, period in ((64, 16), (48, 32), (64, 33), (40, 8)):
        refused(L.omni_add_period_sh, p, p, total, period, word=b"32")
    for fn in (L.omni_layernorm512_f32, L.omni_layernorm512_sh):
        for i in range(4):
            refused(fn, *[z if j == i else p for j in range(4)], 5, f, word=b"null")
        refused(fn, p, p, p, p, 0, f)
        refused(fn, p, p, p, p, -3, f)
    sweep(L.omni_attention_qkv_sh, P2, (2, 18))
    sweep(L.omni_attention_f32, P3, (2, 18))
    sweep(L.omni_token_pack_f32, P3, (36, 18, 16, 32))
    for x, w, oa in ((z, p, p), (p, z, p), (p, p, z)):               # out_c may be null
        refused(L.omni_heads_f32, x, w, f, f, oa, p, 2, 16, 1, word=b"null")
    for M, P in ((0, 16), (2, 0), (-1, 16), (2, -16)):
        refused(L.omni_heads_f32, p, p, f, f, p, p, M, P, 1)
    sweep(L.omni_mlp_points_f32, (p,) * 7, (36, 18, 100), optional=(1,))          # depth may be null
    # what refuses keeps refusing with the right code
    assert L.omni_stem_f32(p, p, p, p, 2, 24, z) == INV and L.omni_attention_f32(p, p, p, 1, 65, z) == _lib.OMNI_ERR_UNSUPPORTED
