"""The backwards of free-view sampling on the device (csrc/omni_freeview_bwd.hip, equi_pers/differentiable.py) against the reference's
float64 autograd (goldens G17a-d, tools/gen_golden_freeview_bwd.py) and, where no golden exists, against the float64 restatement of
tests/_freeview_bwd_cases.py (pinned on the CPU by tests/test_freeview_bwd_cpu.py).

Gate (DESIGN §11's, for gradients): an element is an outlier if |d| > 1e-4 x the largest reference gradient of its tensor; the number
of outliers allowed per case is what the reference's OWN float32 autograd shows against its float64 run (GRAD_OUTLIERS, measured on the
CPU by the generator and stored in the goldens: 0 everywhere; worst relative deviation 1.8e-5)."""
import types

import numpy as np
import pytest
import torch

import _freeview_bwd_cases as bc
import _freeview_cases as fc

pytestmark = pytest.mark.gpu

#                 d/d equi_img, d/d pers_img: elements over the gate in the reference's own float32 autograd (tools/gen_golden_freeview_bwd.py)
GRAD_OUTLIERS = {"G17a": (0, 0), "G17b": (0, 0), "G17c": (0, 0), "G17d": (0, 0)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)


def _args(c):
    return c["hfov"], c["wfov"], torch.from_numpy(c["theta"]), torch.from_numpy(c["phi"])


@pytest.fixture(scope="module")
def fv():
    from omnifusion_amd.equi_pers import differentiable
    return differentiable


def _grad(fn, x, G):
    """d (fn(x) * G).sum() / dx through autograd"""
    x = x.clone().requires_grad_(True)
    out = fn(x)
    out = out[0] if isinstance(out, tuple) else out
    (out * G).sum().backward()
    return x.grad


def _outliers(got, want, what):
    want = np.asarray(want, np.float64)
    d = np.abs(got.cpu().numpy().astype(np.float64) - want)
    top = np.abs(want).max()
    n = int((d > bc.GATE * top).sum())
    print(f"{what}: max |d| / max |grad| = {d.max() / top:.3e}, {n} of {d.size} over the gate")
    assert np.isfinite(d).all()
    return n


def _custom(seed, B, C, H, W, h, w, theta=fc.CUBE_THETA, phi=fc.CUBE_PHI, fov=90.0):
    N = len(theta)
    u = lambda k, shape: (fc.rng_uniform(seed + k, shape) * 2 - 1).astype(np.float32)
    return dict(erp=u(0, (B, C, H, W)), views=u(1, (B, N, C, h, w)), g_e2p=u(2, (B, C, h, N * w)), g_p2e=u(3, (N, C, H, W)), g_merge=u(4, (B, C, H, W)),
                theta=np.asarray(theta, np.float32), phi=np.asarray(phi, np.float32), hfov=fov, wfov=fov, h=h, w=w, H=H, W=W)


def _golden_case(name, B=2):
    """A G17 case as _custom's dict; views / g_merge: B items for views_to_erp (item 0 = the case's own pers)"""
    c = dict(bc.case(name))
    c["g_e2p"], c["g_p2e"] = bc.upstream(name)
    k = bc.NAMES.index(name)
    c["views"] = np.stack([c["pers"]] + [fc.rng_uniform(1752 + 10 * k + b, c["pers"].shape) for b in range(1, B)])
    c["g_merge"] = (fc.rng_uniform(1757 + 10 * k, (B, c["pers"].shape[1], c["H"], c["W"])) * 2 - 1).astype(np.float32)
    return c


# ---------------------------------------------------------------------------------------------------------------- 1. parity (goldens)
@pytest.mark.parametrize("name", bc.NAMES)
def test_equi2pers_backward_against_reference_autograd(fv, name):
    c, g = bc.case(name), bc.load(name)
    G = _dev(bc.upstream(name)[0])
    N = len(c["theta"])
    got = _grad(lambda x: fv.equi2pers(x, *_args(c), c["h"], c["w"]), _dev(c["erp"]), G)
    assert got.shape == c["erp"].shape and got.dtype == torch.float32
    assert _outliers(got, g["grad_erp"], name + " d/d equi_img") <= GRAD_OUTLIERS[name][0]
    planar = _grad(lambda x: fv.equi2pers_planar(x, *_args(c), c["h"], c["w"]), _dev(c["erp"]), bc.planar(G, N))
    assert torch.equal(planar, got)                                       # both layouts: the same gradient bits


@pytest.mark.parametrize("name", bc.NAMES)
def test_pers2equi_backward_against_reference_autograd(fv, name):
    c, g = bc.case(name), bc.load(name)
    G = _dev(bc.upstream(name)[1])
    got = _grad(lambda x: fv.pers2equi(x, *_args(c), c["H"], c["W"]), _dev(c["pers"]), G)
    assert got.shape == c["pers"].shape and got.dtype == torch.float32
    assert _outliers(got, g["grad_pers"], name + " d/d pers_img") <= GRAD_OUTLIERS[name][1]


# ---------------------------------------------------------------------------------------------------------------- 2. views_to_erp
@pytest.mark.parametrize("name", ("G17a", "G17c"))
def test_views_to_erp_backward_against_restatement(fv, name):
    c = _golden_case(name)
    x = _dev(c["views"]).requires_grad_(True)
    erp, count = fv.views_to_erp(x, *_args(c), c["H"], c["W"])
    assert erp.requires_grad and not count.requires_grad and count.dtype == torch.uint8
    (erp * _dev(c["g_merge"])).sum().backward()
    ref = _t64(c["views"]).requires_grad_(True)
    want, wcount = bc.views_to_erp(ref, c["hfov"], c["wfov"], c["theta"], c["phi"], c["H"], c["W"])
    (want * _t64(c["g_merge"])).sum().backward()
    assert torch.equal(count[0].cpu().to(torch.int64), wcount)
    assert x.grad.shape == x.shape
    assert _outliers(x.grad, ref.grad.numpy(), name + " views_to_erp d/d pers") <= max(GRAD_OUTLIERS[name])
    _, mask = fv.pers2equi(_dev(c["pers"]).requires_grad_(True), *_args(c), c["H"], c["W"])
    assert not mask.requires_grad and mask.dtype == torch.int64


# ---------------------------------------------------------------------------------------------------------------- 3. adjoint identity
def _three(fv, c):
    """[(name, f, x, G)]: the three operators on the case's inputs with their upstream gradients (device tensors)"""
    a = _args(c)
    N = len(c["theta"])
    views = _dev(c["views"])
    return [("equi2pers", lambda x: fv.equi2pers(x, *a, c["h"], c["w"]), _dev(c["erp"]), _dev(c["g_e2p"])),
            ("equi2pers_planar", lambda x: fv.equi2pers_planar(x, *a, c["h"], c["w"]), _dev(c["erp"]), bc.planar(_dev(c["g_e2p"]), N)),
            ("pers2equi", lambda x: fv.pers2equi(x, *a, c["H"], c["W"])[0], views[0].contiguous(), _dev(c["g_p2e"])),
            ("views_to_erp", lambda x: fv.views_to_erp(x, *a, c["H"], c["W"])[0], views, _dev(c["g_merge"]))]


@pytest.mark.parametrize("name", bc.NAMES)
def test_adjoint_identity_with_the_forward(fv, name):
    """sum f(x) G == sum x f^T(G) with the library's OWN forward, in float64: forward and backward share their taps.  Both sides carry a
    few fp32 roundings per element (6e-8 each): 1e-5 of sum |f(x) G| leaves two orders of margin."""
    for what, f, x, G in _three(fv, _golden_case(name)):
        with torch.no_grad():
            y = f(x)
        gx = _grad(f, x, G)
        lhs = float((y.double() * G.double()).sum())
        rhs = float((x.double() * gx.double()).sum())
        scale = float((y.double() * G.double()).abs().sum())
        print(f"{name} {what}: <f(x), G> = {lhs:.9e}, <x, fT(G)> = {rhs:.9e}, |d| / sum|.| = {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= 1e-5 * scale


# ---------------------------------------------------------------------------------------------------------------- 4. determinism
def _dense():
    return _custom(1800, 2, 3, 64, 128, 8, 8)             # a 64 x 128 panorama into 8 x 8 cube faces: hundreds of sources per view pixel


def _sparse():
    return _custom(1810, 2, 2, 16, 32, 32, 32)            # a 16 x 32 panorama into 32 x 32 faces: most view pixels receive nothing


def _mixed():
    return _custom(1820, 1, 2, 96, 192, 32, 32)           # a 96 x 192 panorama (18 432 pixels: three LDS windows) from 32 x 32 faces


LDS_WINDOW = 6144        # int64 words a block of the scatter kernel may sum in LDS (FVB_WIN, csrc/omni_freeview_bwd.hip)


def _e2p_tile_boxes(c):
    """The bounding boxes (pixels) of the on-image corners of every source tile of equi2pers^T, from the restatement's float64
    coordinates, with the kernel's tile rule: 16 groups of four pixels x 16 rows, narrower and taller for rows shorter than 64 pixels."""
    h, w, H, W = c["h"], c["w"], c["H"], c["W"]
    ix, iy = (t.numpy() for t in bc.pixel_coordinates(bc.e2p_grid(c["hfov"], c["wfov"], c["theta"], c["phi"], h, w, H, W), H, W))
    groups, tg = -(-w // 4), 1
    while tg < 16 and tg < groups:
        tg *= 2
    tr, tw = 256 // tg, 4 * tg
    boxes = []
    for v in range(len(c["theta"])):
        for r0 in range(0, h, tr):
            for c0 in range(0, w, tw):
                x0 = np.floor(ix[r0:r0 + tr, v * w + c0:v * w + min(c0 + tw, w)]).astype(np.int64)
                y0 = np.floor(iy[r0:r0 + tr, v * w + c0:v * w + min(c0 + tw, w)]).astype(np.int64)
                xs, ys = [], []
                for dy in (0, 1):
                    for dx in (0, 1):
                        ok = (x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H)
                        xs.append((x0 + dx)[ok])
                        ys.append((y0 + dy)[ok])
                xs, ys = np.concatenate(xs), np.concatenate(ys)
                if xs.size:
                    boxes.append(int((xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)))
    return boxes


def test_cases_take_both_scatter_paths():
    """fv_bwd_lds 0 against 1 compares two paths only if the LDS path is taken with the option on.  In the dense, sparse and G17a
    cases a view is smaller than the LDS window (the target of pers2equi^T and views_to_erp^T) and so is every tile box of equi2pers^T,
    so EVERY block sums in LDS; in the mixed case the tiles of equi2pers^T
    fall on both sides (a face across the +-180 degree seam spans the panorama's width), well away from the threshold."""
    for c in (_dense(), _sparse(), _golden_case("G17a")):
        assert c["h"] * c["w"] <= LDS_WINDOW and max(_e2p_tile_boxes(c)) <= 0.8 * LDS_WINDOW
    boxes = _e2p_tile_boxes(_mixed())
    print("mixed case: equi2pers^T tile boxes", sorted(boxes))
    assert min(boxes) <= 0.8 * LDS_WINDOW and max(boxes) >= 1.2 * LDS_WINDOW


def _launches(c):
    """The three backward launches on the case's upstream gradients (no autograd: capturable as they are)."""
    from omnifusion_amd import _lib
    from omnifusion_amd.equi_pers import _freeview
    a = (float(c["hfov"]), float(c["wfov"]), torch.from_numpy(c["theta"]), torch.from_numpy(c["phi"]))
    B, N, C, h, w = c["views"].shape
    ge, gp, gm = _dev(c["g_e2p"]), _dev(c["g_p2e"]), _dev(c["g_merge"])
    return [lambda: _freeview.launch_equi2pers_bwd(ge, c["erp"].shape, *a, h, w, _lib.LAYOUT_BCHNW),
            lambda: _freeview.launch_pers2equi_bwd(gp, (N, C, h, w), *a, c["H"], c["W"]),
            lambda: _freeview.launch_views_to_erp_bwd(gm, (B, N, C, h, w), *a, c["H"], c["W"])]


def test_dense_case_has_targets_with_many_contributions():
    """The point of _dense(): view pixels that take more than 64 contributions each (so the LDS sums and the global sums meet on the
    same targets many times).  From the restatement's float64 coordinates."""
    c = _dense()
    grid, mask = bc.p2e_grid(c["hfov"], c["wfov"], c["theta"], c["phi"], c["h"], c["w"], c["H"], c["W"])
    ix, iy = bc.pixel_coordinates(grid, c["h"], c["w"])
    most = max(int(bc.contributions(ix[v].numpy(), iy[v].numpy(), mask[v, 0].numpy(), c["h"], c["w"]).max()) for v in range(len(c["theta"])))
    print("dense case: most contributions to one view pixel:", most)
    assert most > 64


@pytest.mark.parametrize("make", (_dense, _sparse, _mixed, lambda: _golden_case("G17a")), ids=("dense", "sparse", "mixed", "G17a"))
def test_deterministic_capturable_and_path_independent(fv, make):
    from omnifusion_amd import _lib
    c = make()
    assert _lib.get_option("fv_bwd_lds") == 1
    for call in _launches(c):
        a = call()
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, call())
        _lib.set_option("fv_bwd_lds", 0)
        try:
            assert torch.equal(a, call())                                  # global atomics only: the same integer sums
        finally:
            _lib.set_option("fv_bwd_lds", 1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = call()
        for _ in range(2):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


@pytest.mark.parametrize("make", (_dense, _sparse, lambda: _golden_case("G17a")), ids=("dense", "sparse", "G17a"))
def test_batch_equals_its_items(fv, make):
    c = make()
    hfov, wfov, theta, phi = _args(c)
    B = c["erp"].shape[0]
    N = len(c["theta"])
    erp, views = _dev(c["erp"]), _dev(c["views"])
    ge, gp, gm = _dev(c["g_e2p"]), _dev(c["g_p2e"]), _dev(c["g_merge"])
    e2p = lambda x: fv.equi2pers(x, hfov, wfov, theta, phi, c["h"], c["w"])
    merge = lambda x: fv.views_to_erp(x, hfov, wfov, theta, phi, c["H"], c["W"])
    full_e, full_m = _grad(e2p, erp, ge), _grad(merge, views, gm)
    for b in range(B):
        assert torch.equal(_grad(e2p, erp[b:b + 1], ge[b:b + 1])[0], full_e[b])
        assert torch.equal(_grad(merge, views[b:b + 1], gm[b:b + 1])[0], full_m[b])
    pers = views[0].contiguous()
    full_p = _grad(lambda x: fv.pers2equi(x, hfov, wfov, theta, phi, c["H"], c["W"]), pers, gp)
    for n in range(N):
        one = _grad(lambda x: fv.pers2equi(x, hfov, wfov, theta[n:n + 1], phi[n:n + 1], c["H"], c["W"]), pers[n:n + 1], gp[n:n + 1])
        assert torch.equal(one[0], full_p[n])


# ---------------------------------------------------------------------------------------------------------------- 5. non-finite upstream values
def _poison(G, sites):
    """-> a copy of G with inf at the first site and NaN at the second (sites: index tuples)"""
    bad = G.copy()
    bad[sites[0]] = np.inf
    bad[sites[1]] = np.nan
    return bad


def _check_nonfinite(f, x, G, Gbad, want_grad):
    fin, got = _grad(f, x, _dev(G)), _grad(f, x, _dev(Gbad))
    assert bool(torch.isfinite(fin).all())
    bad = ~torch.isfinite(got)
    want = ~torch.isfinite(want_grad)
    assert int(want.sum()) >= 4
    assert torch.equal(bad.cpu(), want), (int(bad.sum()), int(want.sum()))
    assert torch.equal(got[~bad], fin[~bad])                             # every other element: the finite run's bits


def test_nonfinite_upstream_reaches_exactly_its_targets(fv):
    c = _golden_case("G17a")
    a, a64 = _args(c), (c["hfov"], c["wfov"], c["theta"], c["phi"])
    B, C, H, W = c["erp"].shape
    N, h, w = len(c["theta"]), c["h"], c["w"]
    # equi2pers: two covered view pixels whose float64 coordinates sit inside a pixel cell (the same corners in float32)
    ix, iy = (t.numpy() for t in bc.pixel_coordinates(bc.e2p_grid(*a64, h, w, H, W), H, W))
    ok = np.argwhere(bc.interior_sources(ix, iy, np.ones_like(ix), H, W))
    sites = [(0, 1, int(ok[0][0]), int(ok[0][1])), (1, 0, int(ok[-1][0]), int(ok[-1][1]))]
    Gbad = _poison(c["g_e2p"], sites)
    ref = _t64(c["erp"]).requires_grad_(True)
    (bc.equi2pers(ref, *a64, h, w) * _t64(Gbad)).sum().backward()
    _check_nonfinite(lambda x: fv.equi2pers(x, *a, h, w), _dev(c["erp"]), c["g_e2p"], Gbad, ref.grad)
    # pers2equi: two ERP pixels inside their view's mask
    grid, mask = bc.p2e_grid(*a64, h, w, H, W)
    px, py = (t.numpy() for t in bc.pixel_coordinates(grid, h, w))
    inner = bc.interior_sources(px, py, mask[:, 0].numpy(), h, w)
    ok0, ok2 = np.argwhere(inner[0]), np.argwhere(inner[2])
    sites = [(0, 2, int(ok0[0][0]), int(ok0[0][1])), (2, 0, int(ok2[-1][0]), int(ok2[-1][1]))]
    Gbad = _poison(c["g_p2e"], sites)
    ref = _t64(c["pers"]).requires_grad_(True)
    (bc.pers2equi(ref, *a64, H, W)[0] * _t64(Gbad)).sum().backward()
    p2e = lambda x: fv.pers2equi(x, *a, H, W)
    _check_nonfinite(p2e, _dev(c["pers"]), c["g_p2e"], Gbad, ref.grad)
    # ... and one OUTSIDE the mask reaches nothing (the reference: NaN at pixel (0, 0) of the view)
    r, s = (int(v) for v in np.argwhere(mask[1, 0].numpy() == 0)[0])
    Gout = c["g_p2e"].copy()
    Gout[1, :, r, s] = np.inf
    got = _grad(p2e, _dev(c["pers"]), _dev(Gout))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, _grad(p2e, _dev(c["pers"]), _dev(c["g_p2e"])))
    # views_to_erp: two ERP pixels that are inside a pixel cell of every view that covers them
    m = mask[:, 0].numpy().astype(bool)
    ok = np.argwhere((inner | ~m).all(0) & m.any(0))
    sites = [(0, 1, int(ok[0][0]), int(ok[0][1])), (1, 2, int(ok[-1][0]), int(ok[-1][1]))]
    Gbad = _poison(c["g_merge"], sites)
    ref = _t64(c["views"]).requires_grad_(True)
    (bc.views_to_erp(ref, *a64, H, W)[0] * _t64(Gbad)).sum().backward()
    _check_nonfinite(lambda x: fv.views_to_erp(x, *a, H, W), _dev(c["views"]), c["g_merge"], Gbad, ref.grad)


# ---------------------------------------------------------------------------------------------------------------- 6. interface
def test_interface(fv):
    from omnifusion_amd.equi_pers import views_to_erp
    from omnifusion_amd.equi_pers.equi2pers_torch import equi2pers, equi2pers_planar
    from omnifusion_amd.equi_pers.pers2equi_torch import pers2equi
    c = _golden_case("G17a")
    hfov, wfov, theta, phi = _args(c)
    erp, pers, views = _dev(c["erp"]), _dev(c["pers"]), _dev(c["views"])
    h, w, H, W = c["h"], c["w"], c["H"], c["W"]
    # without grad: the plain mirrors' bits, and nothing to back-propagate
    for plain, diff, x, size in ((equi2pers, fv.equi2pers, erp, (h, w)), (equi2pers_planar, fv.equi2pers_planar, erp, (h, w)),
                                 (pers2equi, fv.pers2equi, pers, (H, W)), (views_to_erp, fv.views_to_erp, views, (H, W))):
        want, got = plain(x, hfov, wfov, theta, phi, *size), diff(x, hfov, wfov, theta, phi, *size)
        with_grad = diff(x.clone().requires_grad_(True), hfov, wfov, theta, phi, *size)
        with torch.no_grad():
            quiet = diff(x.clone().requires_grad_(True), hfov, wfov, theta, phi, *size)
        for a, b, g, q in zip(*(v if isinstance(v, tuple) else (v,) for v in (want, got, with_grad, quiet))):
            assert torch.equal(a, b) and torch.equal(a, g) and torch.equal(a, q) and a.dtype == g.dtype
            assert not b.requires_grad and not q.requires_grad
        first = with_grad[0] if isinstance(with_grad, tuple) else with_grad
        assert first.requires_grad
    # only inputs that require grad get one; the angles never do
    x = erp.clone().requires_grad_(True)
    scale = torch.ones((), device="cuda", requires_grad=True)
    (fv.equi2pers(x, hfov, wfov, theta, phi, h, w) * scale).sum().backward()
    assert x.grad is not None and scale.grad is not None and theta.grad is None
    for call in (lambda: fv.equi2pers(x, hfov, wfov, theta.clone().requires_grad_(True), phi, h, w),
                 lambda: fv.pers2equi(pers.clone().requires_grad_(True), hfov, wfov, theta, phi.clone().requires_grad_(True), H, W),
                 lambda: fv.views_to_erp(views, hfov, wfov, theta.clone().requires_grad_(True), phi, H, W)):
        with pytest.raises(NotImplementedError):
            call()
    # the same argument errors as the plain mirrors
    for call in (lambda: fv.equi2pers(x.double(), hfov, wfov, theta, phi, h, w), lambda: fv.equi2pers(x, hfov, 180.0, theta, phi, h, w),
                 lambda: fv.equi2pers(x, hfov, wfov, theta, phi[:2], h, w), lambda: fv.equi2pers(x.cpu(), hfov, wfov, theta, phi, h, w),
                 lambda: fv.pers2equi(pers[:3].clone().requires_grad_(True), hfov, wfov, theta, phi, H, W),
                 lambda: fv.views_to_erp(views[:, :2].clone().requires_grad_(True), hfov, wfov, theta, phi, H, W)):
        with pytest.raises(ValueError):
            call()
    # no double backward
    y = erp.clone().requires_grad_(True)
    out = fv.equi2pers(y, hfov, wfov, theta, phi, h, w)
    (gy,) = torch.autograd.grad(out.sum(), y, create_graph=True)
    with pytest.raises(RuntimeError):
        gy.sum().backward()
    # a chain: erp -> views -> torch ops -> merged panorama -> loss
    z = erp.clone().requires_grad_(True)
    faces = fv.equi2pers_planar(z, hfov, wfov, theta, phi, h, w)                      # [B,N,C,h,w]
    merged, count = fv.views_to_erp(torch.tanh(faces) * 2.0, hfov, wfov, theta, phi, H, W)
    (merged - z).abs().sum().backward()
    assert z.grad.shape == z.shape and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
