"""GPU: equi2pers / pers2equi, the fused confidence blend and both backwards against the float64 restatement of tests/_resample_cases.py
(pinned on the CPU by tests/test_resample_restatement_cpu.py), every kernel path.

The comparison is split where the conditioning changes:

  (a) coordinates    the kernel's uv / xyz (omni_equi2pers_aux) within 4 * max(e32, 16 * 2^-24 * scale) of float64, in pixels; NaN where float64's is
  (b) the blend      at the kernel's OWN coordinates every sample within 5 * 2^-24 * max|img| of the float64 blend, whichever kernel sampled it
  (c) pers2equi      within 4 * max(e32, 16 * 2^-24 * max|pers|) of float64 -- of one of the 2 or 4 float64 results with the masks of a pixel's one or
                     two near entries flipped, where it has any; more than two: skipped (finite, inside the input's range); uncovered: exactly 0
  (d) backwards      against the float64 transposes, equi2pers at the kernel's coordinates, pers2equi with the gradient zeroed at near pixels

`e32` is the distance of the float32 restatement from the float64 one for the same quantity; nothing in a gate comes from a kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _resample_cases as rc
from _util import rng_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FOV_H, FOV_W = rc.FOV


def _L():
    from omnifusion_amd import _lib
    return _lib


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bc(planes):
    return {1: (1, 1), 2: (2, 1), 3: (1, 3), 7: (7, 1)}[planes]


def _with_options(fn, **opts):
    """fn() under the given options on fresh geometry handles; the options are put back and the handles dropped whatever happens"""
    L = _L()
    lib = L.load()
    before = {k: L.get_option(k) for k in opts}
    try:
        for k, v in opts.items(): L.set_option(k, v)
        lib.omni_geometry_cache_clear()
        out = fn().clone()
        torch.cuda.synchronize()
        return out
    finally:
        for k, v in before.items(): L.set_option(k, v)
        lib.omni_geometry_cache_clear()


def _planar_to_ref(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _ref_to_planar(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------- (a) coordinates
@functools.lru_cache(maxsize=None)
def _kernel_coords(name):
    """omni_equi2pers_aux into NaN-filled buffers -> dict(u, v natural [N,ph,pw] float32, xyz, ix, iy float32 as every sampler must use them)"""
    L = _L()
    case = rc.e2p_case(name)
    (ph, pw), (H, W), N = case["patch"], case["erp_size"], case["N"]
    xyz = torch.full((N, 3, ph, pw), NAN, device=DEV)
    uv = torch.full((N, 2, ph, pw), float("inf"), device=DEV)                # (NaN is a legitimate value of v: q4)
    with torch.cuda.device(DEV):
        L.check(L.load().omni_equi2pers_aux(L.ptr(xyz), L.ptr(uv), ph, pw, case["nrows"], FOV_H, FOV_W, L.stream_of(uv)), "equi2pers_aux")
    torch.cuda.synchronize()
    uv = uv.cpu()
    assert not bool(torch.isinf(uv).any())
    u, v = rc.unscramble(uv[:, 0]).numpy(), rc.unscramble(uv[:, 1]).numpy()
    ix, iy = rc.sampling_coords_f32(u, v, H, W)
    return dict(u=u, v=v, xyz=xyz.cpu().numpy(), ix=ix, iy=iy)


@pytest.mark.parametrize("name", list(rc.E2P_CASES))
def test_coordinates(name):
    case = rc.e2p_case(name)
    H, W = case["erp_size"]
    k = _kernel_coords(name)
    c64 = case["c64"]
    np.testing.assert_array_equal(np.isnan(k["v"]), torch.isnan(c64["v"]).numpy())
    assert not np.isnan(k["u"]).any()
    np.testing.assert_array_equal(np.isnan(k["xyz"]), torch.isnan(rc.xyz_of(c64["lon"], c64["lat"])).numpy())
    assert int(np.isnan(k["v"]).sum()) == (case["N"] if name == "n6_odd" else 0)
    e32 = rc.e2p_coord_e32(case)
    err = rc.e2p_coord_errors(c64, k["u"], k["v"], k["xyz"], H, W)
    for q, scale in (("x", W), ("y", H), ("xyz", 1)):
        print(f"COORD {name} {q}: e32 {e32[q]:.3e}  kernel {err[q]:.3e}  gate {rc.gate(e32[q], scale):.3e}")
    for q, scale in (("x", W), ("y", H), ("xyz", 1)):
        assert err[q] <= rc.gate(e32[q], scale), (q, err[q], rc.gate(e32[q], scale))


# ---------------------------------------------------------------------------------------------------------------- (b) the blend
def _explicit_handle(x, case, layout):
    """omni_equi2pers_g on a handle of its own, into a NaN-filled buffer"""
    L = _L()
    lib = L.load()
    (ph, pw), (H, W), N = case["patch"], case["erp_size"], case["N"]
    B, C = x.shape[:2]
    out = torch.full((B, N, C, ph, pw) if layout == L.LAYOUT_BNCHW else (B, C, ph, pw, N), NAN, dtype=x.dtype, device=DEV)
    handle = ctypes.c_void_p()
    with torch.cuda.device(DEV):
        L.check(lib.omni_geometry_create(ctypes.byref(handle), case["nrows"], FOV_H, FOV_W, ph, pw, H, W, L.stream_of(x)), "geometry_create")
        try:
            L.check(lib.omni_equi2pers_g(handle, L.ptr(x), L.ptr(out), L.dtype_code(x), B, C, layout, L.stream_of(x)), "equi2pers_g")
        finally:
            torch.cuda.synchronize()
            lib.omni_geometry_destroy(handle)
    return out


def _e2p_paths(x, case):
    """(name, result [B,C,ph,pw,N]) of every way to the samplers"""
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers, equi2pers_patches
    L = _L()
    nrows, patch = case["nrows"], case["patch"]
    planar = lambda: equi2pers_patches(x, rc.FOV, nrows, patch, layout=L.LAYOUT_BNCHW)
    ref = lambda: equi2pers_patches(x, rc.FOV, nrows, patch)
    yield "planar", _planar_to_ref(_with_options(planar))
    yield "reference layout", _with_options(ref)
    yield "planar, e2p_gather=1", _planar_to_ref(_with_options(planar, e2p_gather=1))
    yield "reference layout, e2p_gather=1", _with_options(ref, e2p_gather=1)
    yield "reference layout, e2p_ref_lds=0", _with_options(ref, e2p_ref_lds=0)
    yield "omni_equi2pers_g planar", _planar_to_ref(_explicit_handle(x, case, L.LAYOUT_BNCHW))
    yield "omni_equi2pers_g reference layout", _explicit_handle(x, case, L.LAYOUT_BCHWN)
    yield "equi2pers()", equi2pers(x, rc.FOV, nrows, patch)[0]


@pytest.mark.parametrize("name,planes", [(n, p) for n, c in rc.E2P_CASES.items() for p in c[3]])
def test_blend_at_the_kernels_coordinates(name, planes):
    case = rc.e2p_case(name)
    H, W = case["erp_size"]
    k = _kernel_coords(name)
    B, C = _bc(planes)
    x = rng_uniform(901, (B, C, H, W))
    want = rc.equi2pers(x, coords=(k["ix"], k["iy"]))
    tol = 5 * rc.U24 * float(x.max())
    errs = [(path, float((got.cpu().to(rc.F64) - want).abs().max())) for path, got in _e2p_paths(t(x), case)]
    for path, d in errs:
        print(f"BLEND {name} B*C={planes} {path}: {d / (rc.U24 * float(x.max())):.2f} units of 2^-24 (gate 5)")
    for path, d in errs:
        assert d <= tol, (path, d, tol)


def test_blend_fp16_storage():
    """image values in [0, 8) rounded to fp16 first: half an fp16 ulp of the result on top of the fp32 gate"""
    case = rc.e2p_case(rc.E2P_FP16)
    H, W = case["erp_size"]
    k = _kernel_coords(rc.E2P_FP16)
    x = (rng_uniform(902, (1, 3, H, W)) * np.float32(8.0)).astype(np.float16)
    want = rc.equi2pers(x.astype(np.float32), coords=(k["ix"], k["iy"]))
    gate = 2.0 ** -11 * want.abs() + 2.0 ** -25 + 5 * rc.U24 * 8
    errs = []
    for path, got in _e2p_paths(t(x), case):
        assert got.dtype == torch.float16
        errs.append((path, float(((got.cpu().to(rc.F64) - want).abs() - gate).max()), float((got.cpu().to(rc.F64) - want).abs().max())))
    for path, excess, d in errs:
        print(f"BLEND fp16 {path}: max |d| {d:.3e}, largest |d| - gate {excess:.3e} (gate 2^-11 |want| + 2^-25 + {5 * rc.U24 * 8:.3e})")
    for path, excess, d in errs:
        assert excess <= 0, (path, excess)


# ---------------------------------------------------------------------------------------------------------------- (c) pers2equi
def _p2e_paths(run_planar, run_ref):
    """run_planar() / run_ref(): the operator on the planar / the N-innermost tensor -> [(name, result)] of every kernel form and layout route"""
    import omnifusion_amd.equi_pers.pers2equi_v3 as mod
    out = [("default", _with_options(run_planar)),
           ("p2e_walk=2", _with_options(run_planar, p2e_walk=2)),
           ("p2e_walk=0 p2e_gather=2", _with_options(run_planar, p2e_walk=0, p2e_gather=2)),
           ("p2e_gather=1", _with_options(run_planar, p2e_gather=1)),
           ("p2e_walk=2 p2e_tile8=0", _with_options(run_planar, p2e_walk=2, p2e_tile8=0)),
           ("p2e_tile8=0", _with_options(run_planar, p2e_tile8=0))]
    if run_ref is not None:
        floor, via = mod.VIA_PLANAR_MIN, mod.VIA_PLANAR
        try:
            mod.VIA_PLANAR_MIN = 0
            out.append(("pers2equi() via planar", _with_options(run_ref)))
            mod.VIA_PLANAR = False
            out.append(("pers2equi() N-innermost kernel", _with_options(run_ref)))
        finally:
            mod.VIA_PLANAR, mod.VIA_PLANAR_MIN = via, floor
    return out


@pytest.mark.parametrize("name,planes", [(n, p) for n, c in rc.P2E_CASES.items() for p in c[3]])
def test_pers2equi(name, planes):
    from omnifusion_amd.equi_pers.pers2equi_v3 import pers2equi
    L = _L()
    case = rc.p2e_case(name)
    nrows, patch, size = case["nrows"], case["patch"], case["erp_size"]
    x = rc.p2e_inputs(case, planes, 911).reshape(*_bc(planes), *patch, case["N"])
    xt = torch.from_numpy(x)
    want, e32 = rc.p2e_references(case, lambda tab, f: rc.pers2equi(xt, tab, f))
    tol = rc.gate(e32, float(x.max()))
    print(f"P2E {name} B*C={planes}: e32 {e32:.3e}  gate {tol:.3e}")
    ref, planar = t(x), _ref_to_planar(t(x))
    paths = _p2e_paths(lambda: pers2equi(planar, rc.FOV, nrows, patch, size, None, layout=L.LAYOUT_BNCHW),
                       lambda: pers2equi(ref, rc.FOV, nrows, patch, size, "f64"))
    for path, got in paths:
        rc.check_p2e(got.cpu(), want, case, tol, float(x.min()), float(x.max()), f"P2E {name} B*C={planes} {path}")


def test_pers2equi_fp16_storage():
    from omnifusion_amd.equi_pers.pers2equi_v3 import pers2equi
    L = _L()
    case = rc.p2e_case(rc.P2E_FP16)
    nrows, patch, size = case["nrows"], case["patch"], case["erp_size"]
    x = rc.p2e_inputs(case, 3, 912, hi=8.0, fp16=True).reshape(1, 3, *patch, case["N"])
    xt = torch.from_numpy(x)
    want, e32 = rc.p2e_references(case, lambda tab, f: rc.pers2equi(xt, tab, f))
    tol = rc.gate(e32, float(x.max()))
    print(f"P2E fp16 {rc.P2E_FP16}: e32 {e32:.3e}  fp32 part of the gate {tol:.3e}")
    ref, planar = t(x).half(), _ref_to_planar(t(x)).half()
    assert torch.equal(ref.float().cpu(), xt)
    paths = _p2e_paths(lambda: pers2equi(planar, rc.FOV, nrows, patch, size, None, layout=L.LAYOUT_BNCHW),
                       lambda: pers2equi(ref, rc.FOV, nrows, patch, size, "f64"))
    for path, got in paths:
        assert got.dtype == torch.float16
        rc.check_p2e(got.cpu(), want, case, tol, float(x.min()), float(x.max()), f"P2E fp16 {path}", rel=2.0 ** -11, floor=2.0 ** -25)


@pytest.mark.parametrize("name", ["n4_p16", "n3_p32", "n6_p32", "n3_rect"])
def test_confidence_blend(name):
    """conf in [0.25, 1), depth in [0, 8): a well-conditioned quotient.  The nrows = 3 cases take the 1e-8 branch at their uncovered pixels: exactly 0."""
    from omnifusion_amd.equi_pers.pers2equi_v3 import pers2equi_conf
    L = _L()
    case = rc.p2e_case(name)
    nrows, patch, size = case["nrows"], case["patch"], case["erp_size"]
    B = 2
    conf = np.float32(0.25) + np.float32(0.75) * rc.p2e_inputs(case, B, 913)
    depth = rc.p2e_inputs(case, B, 914, hi=8.0)
    pred_w = depth * conf
    ct, pt = torch.from_numpy(conf), torch.from_numpy(pred_w)
    want, e32 = rc.p2e_references(case, lambda tab, f: rc.conf_blend(pt, ct, tab, f))
    tol = rc.gate(e32, float(want[0].abs().max()))
    q = pred_w.astype(np.float64) / conf
    print(f"CONF {name}: e32 {e32:.3e}  gate {tol:.3e}")
    if nrows == 3:
        assert bool(case["uncovered"].any())
    pl = lambda a: _ref_to_planar(t(a))
    a, b = pl(pred_w), pl(conf)
    paths = _p2e_paths(lambda: pers2equi_conf(a, b, rc.FOV, nrows, patch, size, layout=L.LAYOUT_BNCHW), None)
    for path, got in paths:
        rc.check_p2e(got.cpu(), want, case, tol, float(q.min()), float(q.max()), f"CONF {name} {path}")
    got = pers2equi_conf(t(pred_w), t(conf), rc.FOV, nrows, patch, size)
    rc.check_p2e(got.cpu(), want, case, tol, float(q.min()), float(q.max()), f"CONF {name} N-innermost")


# ---------------------------------------------------------------------------------------------------------------- (d) backwards
@pytest.mark.parametrize("name", list(rc.E2P_CASES))
def test_equi2pers_backward(name):
    """The float64 transpose at the kernel's own coordinates, so the weights are exact.  The q4 NaN sample reads row 0 in the forward and its gradient goes
    to row 0 here: the transpose of the forward as it is (dropping it would break <J x, y> = <x, J^T y>)."""
    L = _L()
    lib = L.load()
    case = rc.e2p_case(name)
    (ph, pw), (H, W), N = case["patch"], case["erp_size"], case["N"]
    k = _kernel_coords(name)
    B, C = _bc(case["planes"][-1])
    gp = rng_uniform(921, (B, C, ph, pw, N))
    coords = (k["ix"], k["iy"])
    want = rc.equi2pers_bwd(gp, (H, W), coords=coords)
    e32 = float((rc.equi2pers_bwd(gp, (H, W), coords=coords, dtype=rc.F32).to(rc.F64) - want).abs().max())
    mass = float(rc.equi2pers_bwd(np.abs(gp), (H, W), coords=coords).max())
    tol = rc.gate(e32, mass)
    for layout, g in ((L.LAYOUT_BCHWN, t(gp)), (L.LAYOUT_BNCHW, _ref_to_planar(t(gp)))):
        out = torch.full((B, C, H, W), NAN, device=DEV)
        with torch.cuda.device(DEV):
            L.check(lib.omni_equi2pers_bwd(L.ptr(g), L.ptr(out), L.F32, B, C, H, W, ph, pw, case["nrows"], FOV_H, FOV_W, layout, L.stream_of(g)), "equi2pers_bwd")
        torch.cuda.synchronize()
        d = float((out.cpu().to(rc.F64) - want).abs().max())
        print(f"E2P BWD {name} layout {layout}: e32 {e32:.3e}  kernel {d:.3e}  gate {tol:.3e}  (largest sum of |terms| {mass:.1f})")
        assert bool(torch.isfinite(out).all()) and d <= tol, (layout, d, tol)
    # ... and through autograd of the drop-in
    from omnifusion_amd.equi_pers.equi2pers_v3 import equi2pers_patches
    erp = torch.zeros((B, C, H, W), device=DEV, requires_grad=True)
    (equi2pers_patches(erp, rc.FOV, case["nrows"], (ph, pw)) * t(gp)).sum().backward()
    assert float((erp.grad.cpu().to(rc.F64) - want).abs().max()) <= tol


@pytest.mark.parametrize("name", list(rc.P2E_CASES))
def test_pers2equi_backward(name):
    """grad_erp is zero at every pixel that has a near entry: a mask flip cannot reach the result"""
    L = _L()
    lib = L.load()
    case = rc.p2e_case(name)
    nrows, (ph, pw), (H, W), N = case["nrows"], case["patch"], case["erp_size"], case["N"]
    B, C = _bc(case["planes"][-1])
    ge = rng_uniform(922, (B, C, H, W))
    ge[:, :, (case["count"] > 0).numpy()] = 0
    want = rc.pers2equi_bwd(ge, case["t64"], nrows)
    e32 = float((rc.pers2equi_bwd(ge, case["t32"], nrows).to(rc.F64) - want).abs().max())
    mass = float(rc.pers2equi_bwd(np.abs(ge), case["t64"], nrows).max())
    tol = rc.gate(e32, mass)
    g = t(ge)
    for layout in (L.LAYOUT_BCHWN, L.LAYOUT_BNCHW):
        out = torch.full((B, C, ph, pw, N) if layout == L.LAYOUT_BCHWN else (B, N, C, ph, pw), NAN, device=DEV)
        with torch.cuda.device(DEV):
            L.check(lib.omni_pers2equi_bwd(L.ptr(g), L.ptr(out), L.F32, B, C, ph, pw, H, W, nrows, FOV_H, FOV_W, layout, L.stream_of(g)), "pers2equi_bwd")
        torch.cuda.synchronize()
        got = out if layout == L.LAYOUT_BCHWN else _planar_to_ref(out)
        d = float((got.cpu().to(rc.F64) - want).abs().max())
        print(f"P2E BWD {name} layout {layout}: e32 {e32:.3e}  kernel {d:.3e}  gate {tol:.3e}  (largest sum of |terms| {mass:.1f})")
        assert bool(torch.isfinite(out).all()) and d <= tol, (layout, d, tol)
    from omnifusion_amd.equi_pers.pers2equi_v3 import pers2equi
    pers = torch.zeros((B, C, ph, pw, N), device=DEV, requires_grad=True)
    (pers2equi(pers, rc.FOV, nrows, (ph, pw), (H, W), "f64") * g).sum().backward()
    assert float((pers.grad.cpu().to(rc.F64) - want).abs().max()) <= tol
