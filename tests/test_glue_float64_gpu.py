"""GPU: the stem (four launch forms of the matrix-core kernels, the fp32 kernel), the 3x3/2 max-pool, bilinear up-sampling, the four broadcast adds, the
heads and the split-half conversions against tests/_glue_cases.py — bit for bit with the host model of the SH format where the operator is exact,
under the gate of tests/test_spatial_ops_gpu.py (from the reference side alone) where it rounds.  Every output buffer is filled with NaN before the
call and a NaN in a result fails, except where a test states its own expectation (the SH sweep, the pool's dropped NaN).  Every comparison prints its
error, its gate and their ratio (the GLUE lines); DESIGN.md §22b keeps the largest ratio per operator as measured on an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import _glue_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
OK = 0
NAN = float("nan")


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return t.to(DEV).contiguous()


def _out(*shape):
    return torch.full(shape, NAN, device=DEV)


def _n(t):
    return ctypes.c_size_t(t.numel())


def _overflow(lib, reset=True):
    flag = ctypes.c_int(0)
    assert lib.omni_sh_overflow(ctypes.byref(flag), 1 if reset else 0) == OK, lib.omni_last_error()
    return flag.value


class _Options:
    """library options for the duration of a block, put back in a finally"""
    def __init__(self, L, **kv):
        self.L, self.kv, self.old = L, kv, {}

    def __enter__(self):
        for k in self.kv:
            self.old[k] = self.L.get_option(k)
        try:
            for k, v in self.kv.items():
                self.L.set_option(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.L.set_option(k, v)


# ------------------------------------------------------------------ 1. the SH format
def test_sh_conversions_are_the_host_model_bit_for_bit():
    L, lib = _lib()
    x = gc.sh_sweep()
    normal, den, nan = gc.sweep_classes(x)
    hi, lo = gc.sh_split(x.reshape(-1, 32))
    want_bytes = np.stack([hi, lo], 1).reshape(-1).view(np.uint16)               # [group][hi | lo][32]
    want_vals = gc.sh_join(hi, lo).reshape(-1)
    X = _dev(torch.from_numpy(x))
    S = _out(len(x))
    _overflow(lib)
    assert lib.omni_sh_from_f32(_p(X), _p(S), _n(X), _stream()) == OK, lib.omni_last_error()
    assert _overflow(lib) == 1 and _overflow(lib) == 0                           # the sweep holds values beyond 65504; read and cleared
    got_bytes = S.cpu().numpy().view(np.uint16)
    # the model's bytes, uploaded: omni_sh_to_f32 is checked on them, not on what omni_sh_from_f32 wrote
    V = _out(len(x))
    assert lib.omni_sh_to_f32(_p(_dev(torch.from_numpy(want_bytes.view(np.float32).copy()))), _p(V), _n(V), _stream()) == OK, lib.omni_last_error()
    got_vals = V.cpu().numpy()
    V2 = _out(len(x))
    assert lib.omni_sh_to_f32(_p(S), _p(V2), _n(V2), _stream()) == OK
    round_trip = V2.cpu().numpy()
    el = lambda m: np.stack([m.reshape(-1, 32), m.reshape(-1, 32)], 1).reshape(-1)   # an element mask -> a mask over the halfs
    bad = (el(normal) & (got_bytes != want_bytes)).reshape(-1, 2, 32).any(1).reshape(-1)
    assert not bad.any(), f"omni_sh_from_f32: {bad.sum()} elements differ from the host model, the first at inputs {x[np.nonzero(bad)[0][:4]]}"
    bad = normal & (got_vals.view(np.uint32) != want_vals.view(np.uint32))
    assert not bad.any(), f"omni_sh_to_f32: {bad.sum()} values differ from the host model, first at input {x[np.nonzero(bad)[0][:4]]}"
    assert (np.abs(round_trip[den].astype(np.float64) - x[den]) <= 2.0 ** -36).all()          # fp32 denormals: flushed or not, inside the bound
    assert np.isnan(round_trip[nan]).all() and np.isnan(got_vals[nan]).all()                 # NaN stays NaN
    assert not np.isnan(round_trip[~nan]).any()
    q, a = gc.sh_bounds()
    big = normal & (np.abs(x) >= 2.0 ** -14) & (np.abs(x) <= 65504.0)
    small = normal & (np.abs(x) < 2.0 ** -14)
    rel = float((np.abs(round_trip[big].astype(np.float64) - x[big]) / np.abs(x[big])).max())
    ab = float(np.abs(round_trip[small].astype(np.float64) - x[small]).max())
    print(f"GLUE sh round trip: largest relative error {rel:.4e} (Q {q:.4e}), largest absolute error below 2^-14 {ab:.4e} (A {a:.4e}); "
          f"{int(den.sum())} fp32 denormals within 2^-36")
    assert rel <= q and ab <= a


def test_sh_overflow_flag_is_raised_by_values_beyond_65504_alone():
    L, lib = _lib()
    _overflow(lib)
    nxt = float(np.nextafter(np.float32(65504.0), np.float32(np.inf)))

    def raised(values):
        x = torch.zeros(64)
        x[5:5 + len(values)] = torch.tensor(values)
        X, S = _dev(x), _out(64)
        assert _overflow(lib) == 0
        assert lib.omni_sh_from_f32(_p(X), _p(S), _n(X), _stream()) == OK
        r = _overflow(lib, reset=False)
        assert _overflow(lib) == r and _overflow(lib) == 0                       # sticky until read with reset, then clear
        return r

    assert raised([65504.0, -65504.0, 1.0]) == 0
    assert raised([NAN, 65504.0]) == 0
    assert raised([float(np.nextafter(np.float32(65504.0), np.float32(0.0))), -3.0e4]) == 0
    for v in (nxt, -nxt, 65519.996, 65520.0, -65520.0, float(np.finfo(np.float32).max), float("inf"), float("-inf")):
        assert raised([1.0, v]) == 1, v
    assert raised([NAN, nxt]) == 1


# ------------------------------------------------------------------ 2. exact operators
@pytest.mark.parametrize("kind", gc.POOL_KINDS)
@pytest.mark.parametrize("M,H,W,C", gc.POOL_CASES)
def test_maxpool_sh_bit_for_bit(M, H, W, C, kind):
    """F.max_pool2d of the joined input, re-split by the host model; a NaN is dropped, +-65504 pass through, no padding wins"""
    L, lib = _lib()
    packed, vals = gc.pool_case(M, H, W, C, kind)
    want = gc.maxpool(vals, F32)
    Ho, Wo = want.shape[1:3]
    _overflow(lib)
    out = _out(M, Ho, Wo, C)
    assert lib.omni_maxpool3x3s2_sh(_p(_dev(packed)), _p(out), M, H, W, C, _stream()) == OK, lib.omni_last_error()
    got = out.cpu()
    assert not torch.isnan(gc.sh_unpack(got)).any()
    assert gc.same_bits(got, gc.sh_pack(want)), (gc.sh_unpack(got) - want).abs().max()
    assert _overflow(lib) == 0
    if kind == "negative":
        assert float(gc.sh_unpack(got).max()) <= -1.0
    if (M, H, W, C) == gc.POOL_EXTREME and kind == "randn":
        assert float(gc.sh_unpack(got).max()) == 65504.0
    # the fp32 kernel gives the same values
    out32 = _out(M, Ho, Wo, C)
    assert lib.omni_maxpool3x3s2_f32(_p(_dev(vals)), _p(out32), M, H, W, C, _stream()) == OK, lib.omni_last_error()
    assert torch.equal(out32.cpu(), want)


@pytest.mark.parametrize("M,HW,C", gc.ADD_HW_CASES)
def test_add_hw_f32_is_one_fp32_add(M, HW, C):
    L, lib = _lib()
    x, y = gc.add_case("hw", (M, HW, C), (M, C))
    X = torch.cat([_dev(x).reshape(-1), _out(7)])                                # NaN behind the end: must stay
    assert lib.omni_add_hw_f32(_p(X), _p(_dev(y)), M, HW, C, _stream()) == OK, lib.omni_last_error()
    assert torch.equal(X[:x.numel()].cpu().reshape(x.shape), gc.add_hw(x, y)) and torch.isnan(X[x.numel():]).all()


@pytest.mark.parametrize("total,period", gc.ADD_PERIOD_CASES)
def test_add_period_f32_is_one_fp32_add(total, period):
    L, lib = _lib()
    x, y = gc.add_case("period", (total,), (period,))
    X = torch.cat([_dev(x), _out(7)])
    assert lib.omni_add_period_f32(_p(X), _p(_dev(y)), ctypes.c_size_t(total), ctypes.c_size_t(period), _stream()) == OK, lib.omni_last_error()
    assert torch.equal(X[:total].cpu(), gc.add_period(x, y)) and torch.isnan(X[total:]).all()


@pytest.mark.parametrize("M,HW,C", gc.ADD_SH_CASES)
def test_adds_sh_bit_for_bit(M, HW, C):
    """split(join(x) + y) of the host model"""
    L, lib = _lib()
    x, y = gc.add_case("hw", (M, HW, C), (M, C))
    packed, vals = gc.sh_canonical(x)
    X = torch.cat([_dev(packed).reshape(-1), _out(32)])
    assert lib.omni_add_hw_sh(_p(X), _p(_dev(y)), M, HW, C, _stream()) == OK, lib.omni_last_error()
    assert gc.same_bits(X[:x.numel()].cpu().reshape(x.shape), gc.sh_pack(gc.add_hw(vals, y))) and torch.isnan(X[x.numel():]).all()
    total = M * HW * C
    for period in gc.add_sh_periods(M, HW, C):
        _, y = gc.add_case("period sh", (total,), (period,))
        X = torch.cat([_dev(packed).reshape(-1), _out(32)])
        assert lib.omni_add_period_sh(_p(X), _p(_dev(y)), ctypes.c_size_t(total), ctypes.c_size_t(period), _stream()) == OK, lib.omni_last_error()
        want = gc.sh_pack(gc.add_period(vals.reshape(-1), y).reshape(x.shape))
        assert gc.same_bits(X[:total].cpu().reshape(x.shape), want) and torch.isnan(X[total:]).all(), period


@pytest.mark.parametrize("M,H,W,C", gc.UP_IDENTITY_CASES)
def test_upsample_sh_to_the_same_size_copies_the_bytes(M, H, W, C):
    L, lib = _lib()
    packed, _ = gc.up_case(M, H, W, C, True)
    out = _out(M, H, W, C)
    assert lib.omni_upsample_bilinear_sh(_p(_dev(packed)), _p(out), M, H, W, C, H, W, _stream()) == OK, lib.omni_last_error()
    assert gc.same_bits(out.cpu(), packed)


# ------------------------------------------------------------------ 3. operators under a gate
@pytest.mark.parametrize("M,P", gc.STEM_F32_CASES)
def test_stem_fp32_kernel_against_float64(M, P):
    L, lib = _lib()
    x, w, b = gc.stem_case(M, P)
    ref, r32 = gc.stem_reference(M, P)
    X, WT, B = _dev(x), _dev(gc.stem_weights_f32(w)), _dev(b)
    o32, osh = _out(M, P // 2, P // 2, 64), _out(M, P // 2, P // 2, 64)
    assert lib.omni_stem_f32(_p(X), _p(WT), _p(B), _p(o32), M, P, _stream()) == OK, lib.omni_last_error()
    assert lib.omni_stem_sh(_p(X), _p(WT), _p(B), _p(osh), M, P, _stream()) == OK, lib.omni_last_error()
    gc.report("stem_f32", (M, P), o32.cpu(), ref, gc.gate(r32, ref))
    gc.report("stem_sh", (M, P), gc.sh_unpack(osh.cpu()), ref, gc.gate(r32, ref, sh=True))
    assert gc.same_bits(osh.cpu(), gc.sh_pack(o32.cpu()))                       # the SH kernel stores the fp32 kernel's sums


@pytest.mark.parametrize("M,P", gc.STEM_MM_CASES)
def test_stem_matrix_core_launch_forms_against_float64(M, P):
    """omni_stem_sh_f16x3 at CONV_GATE, omni_stem_sh_f16x1 under test_stem_f16x1's check, with conv_stem_pc in {1, 0} (and conv_epi_lds = 0 for the
    first two cases): every form gives the same bits.  The last two cases are sized for 256 CUs (tests/_glue_cases.py); the count is printed."""
    L, lib = _lib()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"GLUE stem {(M, P)}: {ncu} CUs; on them {gc.stem_launch(M, P, ncu)}; on 256 {gc.stem_launch(M, P)}")
    x, w, b = gc.stem_case(M, P)
    ref, _ = gc.stem_reference(M, P)
    W16c = gc.stem_weights_f16x3(w)
    X, W16, B = _dev(x), _dev(W16c), _dev(b)
    x1_refs = gc.stem_f16x1_refs(x, b, W16c)
    epis = (1, 0) if (M, P) in gc.STEM_MM_NO_EPI_LDS else (1,)
    first = {}
    for epi in epis:
        for pc in (1, 0):
            with _Options(L, conv_stem_pc=pc, conv_epi_lds=epi):
                for name, fn in (("f16x3", lib.omni_stem_sh_f16x3), ("f16x1", lib.omni_stem_sh_f16x1)):
                    out = _out(M, P // 2, P // 2, 64)
                    assert fn(_p(X), _p(W16), _p(B), _p(out), M, P, _stream()) == OK, lib.omni_last_error()
                    got = out.cpu()
                    val = gc.sh_unpack(got)
                    what = f"{(M, P)} pc={pc} epi_lds={epi}"
                    if name == "f16x3":
                        gc.report("stem_f16x3", what, val, ref, gc.CONV_GATE)
                    else:
                        assert not torch.isnan(val).any(), what
                        e = gc.f16x1_check(val, *x1_refs, what)
                        print(f"GLUE stem_f16x1 {what}: error {e:.3e} of sum |a||w|  gate {gc.X1_REL:.1e}  ratio {e / gc.X1_REL:.3f}")
                    if name in first:
                        assert gc.same_bits(got, first[name]), f"{name} {what}: other bits than pc=1 epi_lds=1"
                    else:
                        first[name] = got
    assert not gc.same_bits(first["f16x3"], first["f16x1"])


@pytest.mark.parametrize("M,H,W,C,Ho,Wo", gc.UP_SH_CASES)
def test_upsample_sh_against_float64(M, H, W, C, Ho, Wo):
    L, lib = _lib()
    packed, vals = gc.up_case(M, H, W, C, True)
    ref = gc.upsample(vals, Ho, Wo, F64)
    g = gc.gate(gc.upsample_stock(vals, Ho, Wo, F32), ref, sh=True)
    out = _out(M, Ho, Wo, C)
    assert lib.omni_upsample_bilinear_sh(_p(_dev(packed)), _p(out), M, H, W, C, Ho, Wo, _stream()) == OK, lib.omni_last_error()
    gc.report("upsample_sh", (M, H, W, C, Ho, Wo), gc.sh_unpack(out.cpu()), ref, g)


@pytest.mark.parametrize("M,H,W,C,Ho,Wo", gc.UP_F32_CASES)
def test_upsample_f32_against_float64(M, H, W, C, Ho, Wo):
    L, lib = _lib()
    x, _ = gc.up_case(M, H, W, C, False)
    ref = gc.upsample(x, Ho, Wo, F64)
    out = _out(M, Ho, Wo, C)
    assert lib.omni_upsample_bilinear_f32(_p(_dev(x)), _p(out), M, H, W, C, Ho, Wo, _stream()) == OK, lib.omni_last_error()
    gc.report("upsample_f32", (M, H, W, C, Ho, Wo), out.cpu(), ref, gc.gate(gc.upsample_stock(x, Ho, Wo, F32), ref))


def _heads_run(lib, x, w, bp, bw, conf, with_c=True):
    M, P = x.shape[0], x.shape[1]
    oa, oc = _out(M, P, P), (_out(M, P, P) if with_c else None)
    assert lib.omni_heads_f32(_p(_dev(x)), _p(_dev(w)), ctypes.c_float(bp), ctypes.c_float(bw), _p(oa), _p(oc), M, P, conf, _stream()) == OK, lib.omni_last_error()
    return oa.cpu(), (oc.cpu() if with_c else None)


@pytest.mark.parametrize("M,P,conf", gc.HEADS_CASES)
def test_heads_against_float64(M, P, conf):
    L, lib = _lib()
    print(f"GLUE heads {(M, P)}: (tiles, blocks, second tiles) = {gc.heads_tiles(M, P)}")
    x, w, bp, bw = gc.heads_case(M, P)
    a64, c64, _ = gc.heads(x, w, bp, bw, conf, F64)
    a32, c32 = gc.heads_stock(x, w, bp, bw, conf, F32)
    oa, oc = _heads_run(lib, x, w, bp, bw, conf)
    gc.report("heads", f"{(M, P, conf)} a", oa, a64, gc.gate(a32, a64))
    gc.report("heads", f"{(M, P, conf)} c", oc, c64, gc.gate(c32, c64))
    if (M, P, conf) == gc.HEADS_NO_CONF_PLANE:
        oa2, none = _heads_run(lib, x, w, bp, bw, conf, with_c=False)
        assert none is None and torch.equal(oa2, oa)
        oa1, _ = _heads_run(lib, x, w, bp, bw, 1)                                # the other setting of `confidence` on the same input
        a64c = gc.heads(x, w, bp, bw, 1, F64)[0]
        gc.report("heads", f"{(M, P, 1)} a", oa1, a64c, gc.gate(gc.heads_stock(x, w, bp, bw, 1, F32)[0], a64c))
    if (M, P, conf) == gc.HEADS_SHARP:
        x, w, bp, bw = gc.heads_case(M, P, sharp=True)
        a64, c64, z = gc.heads(x, w, bp, bw, conf, F64)
        a32, c32 = gc.heads_stock(x, w, bp, bw, conf, F32)
        oa, oc = _heads_run(lib, x, w, bp, bw, conf)
        gc.report("heads", f"{(M, P, conf)} sharp a", oa, a64, gc.gate(a32, a64))
        gc.report("heads", f"{(M, P, conf)} sharp c", oc, c64, gc.gate(c32, c64))
        assert torch.isfinite(oa).all() and float(oc.min()) == 0.0 and float(oc.max()) == 1.0
        assert (oc[z[..., 1] < -95.0] == 0).all() and (oc[z[..., 1] > 95.0] == 1).all()
