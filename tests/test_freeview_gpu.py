"""Free-view sampling on the device (csrc/omni_freeview.hip) against the reference's float64 results (goldens G16a-d, tools/gen_golden_freeview.py).

Gates: equi2pers max |d| <= 1e-3 with no outliers (the project's parity gate of the resample operators for inputs in [0,1); this direction
has no step predicate).  pers2equi: a mask element may differ from the reference's float64 mask only where flip_allowed() says a float32
evaluation can land on the other side of a strict comparison; the number of such flips is pinned per case in FLIPS (and capped at 1 per
10 000 elements for a, b, d); where the masks agree max |d| <= 1e-3; where our mask is 0 the output is exactly 0; nothing is non-finite."""
import numpy as np
import pytest
import torch

import _freeview_cases as fc

pytestmark = pytest.mark.gpu

TOL = 1e-3
# mask elements that differ from the reference's float64 mask, measured on MI355X when the gate was written (the kernels are deterministic
# and the inputs seeded: a constant of the kernel arithmetic).  The reference's own float32 run: 0 in every case, G16c included.
FLIPS = {"G16a": 0, "G16b": 0, "G16c": 0, "G16d": 0}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _angles(c):
    return torch.from_numpy(c["theta"]), torch.from_numpy(c["phi"])


@pytest.fixture(scope="module")
def ops():
    from omnifusion_amd.equi_pers import cubemap_views, views_to_erp
    from omnifusion_amd.equi_pers.equi2pers_torch import equi2pers, equi2pers_planar
    from omnifusion_amd.equi_pers.pers2equi_torch import pers2equi
    import types
    return types.SimpleNamespace(equi2pers=equi2pers, equi2pers_planar=equi2pers_planar, pers2equi=pers2equi, views_to_erp=views_to_erp,
                                 cubemap_views=cubemap_views)


@pytest.mark.parametrize("name", fc.NAMES)
def test_equi2pers_against_reference(ops, name):
    c, g = fc.case(name), fc.load(name)
    theta, phi = _angles(c)
    B, C, _, _ = c["erp"].shape
    N, h, w = len(c["theta"]), c["h"], c["w"]
    got = ops.equi2pers(_dev(c["erp"]), c["hfov"], c["wfov"], theta, phi, h, w)
    assert got.shape == (B, C, h, N * w) and got.dtype == torch.float32
    d = np.abs(got.cpu().numpy().astype(np.float64) - g["e2p"])
    print(f"{name} equi2pers max |d| = {d.max():.3e} (reference float32 run: {float(g['ref32_e2p_max']):.3e})")
    assert np.isfinite(d).all() and d.max() <= TOL
    planar = ops.equi2pers_planar(_dev(c["erp"]), c["hfov"], c["wfov"], theta, phi, h, w)
    assert planar.shape == (B, N, C, h, w)
    assert torch.equal(planar.permute(0, 2, 3, 1, 4).reshape(B, C, h, N * w), got)      # both layouts: the same samples


@pytest.mark.parametrize("name", fc.NAMES)
def test_pers2equi_against_reference(ops, name):
    c, g = fc.case(name), fc.load(name)
    theta, phi = _angles(c)
    erp, mask = ops.pers2equi(_dev(c["pers"]), c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])
    assert erp.shape == g["p2e"].shape and mask.shape == g["mask"].shape
    assert str(mask.dtype) == "torch." + str(g["mask_dtype"])
    erp, mask = erp.cpu().numpy(), mask.cpu().numpy()
    assert np.isfinite(erp).all()
    assert set(np.unique(mask).tolist()) <= {0, 1}
    flipped = mask != g["mask"]
    n = int(flipped.sum())
    print(f"{name} pers2equi mask flips = {n} of {mask.size} (reference float32 run: {int(g['ref32_mask_flips'])})")
    allowed = fc.flip_allowed(c["theta"], c["phi"], c["hfov"], c["wfov"], c["H"], c["W"])
    assert not (flipped & ~allowed).any(), f"{int((flipped & ~allowed).sum())} mask elements flipped away from every frustum bound"
    assert n <= FLIPS[name]
    if name != "G16c":
        assert n <= fc.FLIP_CAP * mask.size
    agree = np.broadcast_to(~flipped, erp.shape)
    d = np.abs(erp.astype(np.float64) - g["p2e"])[agree]
    print(f"{name} pers2equi max |d| = {d.max():.3e} (reference float32 run: {float(g['ref32_p2e_max']):.3e})")
    assert d.max() <= TOL
    assert (erp[np.broadcast_to(mask == 0, erp.shape)] == 0).all()


@pytest.mark.parametrize("name", fc.NAMES)
def test_views_to_erp_is_the_masked_mean_of_pers2equi(ops, name):
    c = fc.case(name)
    theta, phi = _angles(c)
    N, C, h, w = c["pers"].shape
    views = torch.stack([_dev(c["pers"]), _dev(fc.rng_uniform(1790, c["pers"].shape))])          # [2,N,C,h,w]
    erp, count = ops.views_to_erp(views, c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])
    assert erp.shape == (2, C, c["H"], c["W"]) and count.shape == (1, 1, c["H"], c["W"]) and count.dtype == torch.uint8
    assert bool(torch.isfinite(erp).all())
    for b in range(2):
        e, m = ops.pers2equi(views[b], c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])
        want, cnt = fc.merge(e, m)
        assert torch.equal(count[0].to(torch.int64), cnt)
        d = float((erp[b] - want).abs().max())
        assert d <= 1e-6, d
        alone, count1 = ops.views_to_erp(views[b:b + 1], c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])
        assert torch.equal(alone[0], erp[b]) and torch.equal(count1, count)


def test_cube_round_trip(ops):
    """ERP -> six 64 x 64 cube faces -> views_to_erp on a smooth panorama: every pixel is covered, and away from the image border the
    result is as close to the input as the float64 restatement's own round trip (two bilinear resamplings), plus 1e-3."""
    H, W, P = 64, 128, 64
    img = fc.smooth_pattern(3, H, W)
    theta, phi = ops.cubemap_views()
    faces = ops.equi2pers_planar(_dev(img), 90, 90, theta, phi, P, P)
    erp, count = ops.views_to_erp(faces, 90, 90, theta, phi, H, W)
    assert int(count.min()) >= 1
    r = fc.equi2pers(img, 90, 90, theta.numpy(), phi.numpy(), P, P)                                 # [1,3,P,6P]
    r = r.reshape(3, P, 6, P).permute(2, 0, 1, 3)
    want, cnt = fc.merge(*fc.pers2equi(r, 90, 90, theta.numpy(), phi.numpy(), H, W))
    assert int(cnt.min()) >= 1
    inner = (slice(None), slice(2, H - 2), slice(2, W - 2))
    ref_err = float(np.abs(want.numpy() - img[0])[inner].max())
    err = float(np.abs(erp[0].cpu().numpy().astype(np.float64) - img[0])[inner].max())
    print(f"round trip: interior error {err:.3e} (float64 restatement {ref_err:.3e})")
    assert err <= ref_err + 1e-3


def _three_ops(ops, c):
    theta, phi = _angles(c)
    erp, pers = _dev(c["erp"]), _dev(c["pers"])
    views = pers[None].contiguous()
    return [lambda: ops.equi2pers(erp, c["hfov"], c["wfov"], theta, phi, c["h"], c["w"]),
            lambda: ops.pers2equi(pers, c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])[0],
            lambda: ops.views_to_erp(views, c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])[0]]


def test_deterministic_and_capturable(ops):
    for call in _three_ops(ops, fc.case("G16a")):
        a = call()
        assert torch.equal(a, call())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()                                                      # warm-up on a side stream: the rotation table is uploaded here
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = call()
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


def test_error_paths_launch_nothing(ops):
    from omnifusion_amd import _lib, util
    c = fc.case("G16a")
    theta, phi = _angles(c)
    erp, pers = _dev(c["erp"]), _dev(c["pers"])
    args = (c["hfov"], c["wfov"])
    _lib.CALL_LOG = log = []
    try:
        for bad in (erp.double(), erp.half(), erp.cpu(), erp[0]):
            with pytest.raises(ValueError):
                ops.equi2pers(bad, *args, theta, phi, c["h"], c["w"])
        for bad in (pers.double(), pers.cpu(), pers[:3]):
            with pytest.raises(ValueError):
                ops.pers2equi(bad, *args, theta, phi, c["H"], c["W"])
        with pytest.raises(ValueError):
            ops.views_to_erp(pers[None].cpu(), *args, theta, phi, c["H"], c["W"])
        with pytest.raises(ValueError):
            ops.views_to_erp(pers[None, :2], *args, theta, phi, c["H"], c["W"])
        for call in (lambda: ops.equi2pers(erp, *args, theta, phi[:3], c["h"], c["w"]),
                     lambda: ops.pers2equi(pers, *args, theta[:2], phi, c["H"], c["W"]),
                     lambda: ops.views_to_erp(pers[None], *args, theta, phi[:1], c["H"], c["W"]),
                     lambda: ops.equi2pers(erp, 0.0, 90.0, theta, phi, c["h"], c["w"]),
                     lambda: ops.equi2pers(erp, 60.0, 180.0, theta, phi, c["h"], c["w"]),
                     lambda: ops.equi2pers(erp, *args, theta, phi, 1, c["w"])):
            with pytest.raises(ValueError):
                call()
        for call in (lambda: ops.equi2pers(erp.clone().requires_grad_(True), *args, theta, phi, c["h"], c["w"]),
                     lambda: ops.pers2equi(pers.clone().requires_grad_(True), *args, theta, phi, c["H"], c["W"]),
                     lambda: ops.views_to_erp(pers[None].clone().requires_grad_(True), *args, theta, phi, c["H"], c["W"]),
                     lambda: util.transform_equi(erp.clone().requires_grad_(True), theta, phi, c["h"], c["w"], 2, *args)):
            with pytest.raises(NotImplementedError):
                call()
        launches = [w for w in log if "rotations" not in w]
        assert launches == [], launches
    finally:
        _lib.CALL_LOG = None


def test_util_transforms_mirror_the_reference_shapes(ops):
    from omnifusion_amd import util
    c = fc.case("G16a")
    theta, phi = _angles(c)
    B, C, _, _ = c["erp"].shape
    N = len(c["theta"])
    pers = util.transform_equi(_dev(c["erp"]), theta, phi, c["h"], c["w"], 2, c["hfov"], c["wfov"])
    assert pers.shape == (B * 2, C, c["h"], N * c["w"])
    one = ops.equi2pers(_dev(c["erp"]), c["hfov"], c["wfov"], theta, phi, c["h"], c["w"])
    assert torch.equal(pers[0::2], one) and torch.equal(pers[1::2], one)
    equi, mask = util.transform_pers(_dev(c["pers"]), theta, phi, c["H"], c["W"], c["hfov"], c["wfov"])
    e, m = ops.pers2equi(_dev(c["pers"]), c["hfov"], c["wfov"], theta, phi, c["H"], c["W"])
    assert torch.equal(equi, e) and mask.shape == (N, 1, 1, c["H"], c["W"]) and torch.equal(mask[:, 0], m)
