"""GPU: the Chamfer term (supervision.chamfer, util.chamfer_distance_with_batch; csrc/omni_chamfer.hip) against the fixtures G21a-e — the
reference's own chamfer_distance_with_batch in float64 on the CPU with its autograd gradients (tools/gen_golden_chamfer.py) — and its
bitwise properties: the lowest index wins a tie, repeated runs, batch splits, the M-split path against the unsplit walk, mask dtypes,
NaN and empty-target conventions, and depth_chamfer against the same call on points formed by hand."""
import functools

import numpy as np
import pytest
import torch

import _chamfer_cases as cc
from _util import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def t(a, **kw):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, **kw)


def run(c, p1=None, p2=None, mask1="case", mask2="case", grads=True):
    """-> dict(loss: 0-d float32 array, dist, idx, g1, g2: arrays) of one forward (and backward) on the case's clouds or on p1 / p2."""
    from omnifusion_amd.supervision import chamfer_distance, nearest_neighbours
    a, b = t(c["p1"] if p1 is None else p1).requires_grad_(grads), t(c["p2"] if p2 is None else p2).requires_grad_(grads)
    m1, m2 = (t(c["mask1"]) if isinstance(mask1, str) else mask1), (t(c["mask2"]) if isinstance(mask2, str) else mask2)
    dist, idx = nearest_neighbours(a, b, m1, m2)
    loss = chamfer_distance(a, b, m1, m2)
    out = dict(loss=loss.detach().cpu().numpy(), dist=dist.detach().cpu().numpy(), idx=idx.cpu().numpy())
    assert out["idx"].dtype == np.int32 and out["dist"].dtype == np.float32 and out["loss"].dtype == np.float32 and out["loss"].shape == ()
    if grads:
        loss.backward()
        out.update(g1=a.grad.cpu().numpy(), g2=b.grad.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def result(name):
    return run(cc.case(name))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint8)


def same_bits(a, b, keys=("loss", "dist", "idx", "g1", "g2")):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys if k in a and k in b)


def loss_gate(g):
    return max(1e-6 * abs(float(g["loss"])), 4 * float(g["ref32_loss_err"]))


@pytest.mark.parametrize("name", cc.NAMES)
def test_parity_with_reference(name):
    """idx exactly; dist within max(1e-5, 4 x the reference's float32 error); the loss within max(1e-6 |golden|, 4 x its float32 error) — a
    float32 scalar of size 2600 has an ulp of 2.4e-4; both gradients within max(1e-5, 4 x its float32 error) of the largest reference
    gradient; the gradient exactly 0 at the planted duplicates and at masked points."""
    c, g, r = cc.case(name), golden(name + "_chamfer"), result(name)
    assert np.array_equal(r["idx"], g["idx"])
    d_err, d_tol = np.abs(r["dist"].astype(np.float64) - g["dist"]).max(), max(1e-5, 4 * float(g["ref32_dist_err"]))
    l_err, l_tol = abs(float(r["loss"]) - float(g["loss"])), loss_gate(g)
    g_tol = max(1e-5, 4 * float(g["ref32_grad_max"]))
    e1, e2 = cc.rel_error(r["g1"], g["grad_p1"]).max(), cc.rel_error(r["g2"], g["grad_p2"]).max()
    print(f"{name}: dist {d_err:.2e} / {d_tol:.1e}, loss {l_err:.2e} / {l_tol:.1e}, grad_p1 {e1:.2e} grad_p2 {e2:.2e} / {g_tol:.1e}")
    assert d_err <= d_tol and l_err <= l_tol and e1 <= g_tol and e2 <= g_tol
    for b, i, j in c["dup"]:
        assert r["dist"][b, i] == 0.0 and r["idx"][b, i] == j and not r["g1"][b, i].any()
    if c["mask1"] is not None:
        assert not r["g1"][~c["mask1"]].any() and not r["g2"][~c["mask2"]].any() and not r["dist"][~c["mask1"]].any()
        assert (r["idx"][~c["mask1"]] == -1).all()
    if c["dup"]:                                                               # a duplicate sends nothing to its original either
        only = {}
        for b, i, j in c["dup"]:
            only[(b, j)] = [q for q in np.flatnonzero(g["idx"][b] == j) if q != i]
        for (b, j), others in only.items():
            if not others:
                assert not r["g2"][b, j].any()


def test_with_batch_is_the_sum_reduction():
    from omnifusion_amd.supervision import chamfer_distance
    from omnifusion_amd.util import chamfer_distance_with_batch
    c = cc.case("G21a")
    a, b = t(c["p1"]), t(c["p2"])
    x, y, z = chamfer_distance_with_batch(a, b), chamfer_distance(a, b, reduction="sum"), chamfer_distance_with_batch(a, b, debug=True)
    assert x.dtype == torch.float32 and x.dim() == 0 and x.is_cuda
    assert np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy())) and np.array_equal(bits(x.cpu().numpy()), bits(z.cpu().numpy()))
    assert np.array_equal(bits(x.cpu().numpy()), bits(result("G21a")["loss"]))
    p = t(c["p1"]).requires_grad_(True)
    chamfer_distance_with_batch(p, b).backward()
    assert np.array_equal(bits(p.grad.cpu().numpy()), bits(result("G21a")["g1"]))


def test_bidirectional_and_mean():
    from omnifusion_amd.supervision import chamfer_distance
    c, g = cc.case("G21e"), golden("G21e_chamfer")
    a, b, m1, m2 = t(c["p1"]), t(c["p2"]), t(c["mask1"]), t(c["mask2"])
    fwd, back = chamfer_distance(a, b, m1, m2), chamfer_distance(b, a, m2, m1)
    both = chamfer_distance(a, b, m1, m2, bidirectional=True)
    assert abs(float(both) - (float(fwd) + float(back))) <= loss_gate(g)
    swapped = dict(c, p1=c["p2"], p2=c["p1"], mask1=c["mask2"], mask2=c["mask1"])
    want = cc.run_restatement(c, torch.float64)["loss"] + cc.run_restatement(swapped, torch.float64)["loss"]
    assert abs(float(both) - want) <= 2 * loss_gate(g)
    n1, n2 = int(c["mask1"].sum()), int(c["mask2"].sum())
    mean = chamfer_distance(a, b, m1, m2, reduction="mean")
    assert abs(float(mean) - float(fwd) / n1) <= 2e-7 * abs(float(mean))
    mean2 = chamfer_distance(a, b, m1, m2, bidirectional=True, reduction="mean")
    assert abs(float(mean2) - (float(fwd) / n1 + float(back) / n2)) <= 4e-7 * abs(float(mean2))
    c3 = cc.case("G21c")                                                       # without masks: every point is a valid query
    s, m = chamfer_distance(t(c3["p1"]), t(c3["p2"])), chamfer_distance(t(c3["p1"]), t(c3["p2"]), reduction="mean")
    assert abs(float(m) - float(s) / (3 * 1000)) <= 2e-7 * abs(float(m))


@pytest.mark.parametrize("name", ["G21a", "G21d"])
def test_lowest_index_wins_a_tie(name):
    """Copies of targets that ARE nearest neighbours, appended at higher indices (G21a: a third tile; G21d: a later chunk of the split
    path): idx never names a copy, and dist and the loss keep their bits."""
    c, r = cc.case(name), result(name)
    B, N, M, D = cc.SHAPES[name]
    ncopy = 40
    copies = np.stack([c["p2"][b, r["idx"][b, :ncopy]] for b in range(B)])
    tied = run(c, p2=np.concatenate([c["p2"], copies], axis=1), grads=False)
    assert tied["idx"].max() < M and np.array_equal(tied["idx"], r["idx"])
    assert same_bits(tied, r, ("loss", "dist"))
    # ... and placed BEFORE the originals, the copies win
    first = run(c, p2=np.concatenate([copies, c["p2"]], axis=1), grads=False)
    for b in range(B):
        q = np.arange(ncopy)
        assert np.array_equal(first["idx"][b, q], np.array([int(np.flatnonzero(r["idx"][b, :ncopy] == j)[0]) for j in r["idx"][b, :ncopy]]))
    assert same_bits(first, r, ("loss", "dist"))


@pytest.mark.parametrize("name", ["G21a", "G21e"])
def test_bitwise_reproducible_and_batch_split_invariant(name):
    c, r = cc.case(name), result(name)
    for _ in range(2):
        assert same_bits(run(c), r)
    for b in range(cc.SHAPES[name][0]):
        one = run(dict(c, p1=c["p1"][b:b + 1], p2=c["p2"][b:b + 1], mask1=None if c["mask1"] is None else c["mask1"][b:b + 1],
                       mask2=None if c["mask2"] is None else c["mask2"][b:b + 1]))
        for k in ("dist", "idx", "g1", "g2"):
            assert np.array_equal(bits(one[k][0]), bits(r[k][b])), (k, b)


@pytest.mark.parametrize("name", ["G21d", "G21c"])
def test_split_path_has_the_bits_of_the_unsplit_walk(name):
    """G21d (65 queries, 4099 targets: 17 tiles in 17 chunks and a merge) and G21c (never split) with option chamfer_split = 0."""
    from omnifusion_amd import _lib
    c, r = cc.case(name), result(name)
    assert _lib.get_option("chamfer_split") == 1
    _lib.set_option("chamfer_split", 0)
    try:
        off = run(c)
    finally:
        _lib.set_option("chamfer_split", 1)
    assert same_bits(off, r)


def test_directional_derivative():
    """(L(x + h v) - L(x - h v)) / 2h of the float64 restatement against <grad, v> of the device's gradients on G21a, both clouds moving, v
    along the gradient, h = 3e-3; tolerance: twice the residual the same check leaves on the reference's float32 run (recorded in the
    fixture).  The same residual with the device's own float32 loss is printed beside it and held to the same tolerance."""
    c, g, r = cc.case("G21a"), golden("G21a_chamfer"), result("G21a")
    v1, v2 = cc.direction("G21a")
    n1 = c["p1"].size
    x, v = np.concatenate([c["p1"].ravel(), c["p2"].ravel()]), np.concatenate([v1.ravel(), v2.ravel()])
    grad = np.concatenate([r["g1"].ravel(), r["g2"].ravel()]).astype(np.float64)
    split = lambda y: (y[:n1].reshape(c["p1"].shape), y[n1:].reshape(c["p2"].shape))
    res64, fd64, dot = cc.directional_residual(lambda y: cc.restatement_loss(c, torch.float64, *split(y)), grad, x, v, cc.DIRECTION_H)
    res32, fd32, _ = cc.directional_residual(lambda y: float(run(c, *split(y), grads=False)["loss"]), grad, x, v, cc.DIRECTION_H)
    tol = 2 * float(g["ref32_direction_residual"])
    print(f"finite difference {fd64:.8e} (float64 restatement) {fd32:.8e} (device), <grad, v> {dot:.8e}, residuals {res64:.3e} {res32:.3e}, tolerance {tol:.3e}")
    assert res64 <= tol and res32 <= tol, (res64, res32, fd64, fd32, dot)


def test_mask_dtypes_give_the_same_bits():
    c, r = cc.case("G21e"), result("G21e")
    for conv in (lambda m: t(m), lambda m: t(m).to(torch.uint8), lambda m: t(m).to(torch.float32) * 2.5, lambda m: t(m).double()):
        assert same_bits(run(c, mask1=conv(c["mask1"]), mask2=conv(c["mask2"])), r)


def test_nan_at_a_masked_point_changes_nothing():
    c, r = cc.case("G21e"), result("G21e")
    p1, p2 = c["p1"].copy(), c["p2"].copy()
    p1[0, np.flatnonzero(~c["mask1"][0])[3], 1] = np.nan
    p2[1, np.flatnonzero(~c["mask2"][1])[5], 0] = np.nan
    p2[0, np.flatnonzero(~c["mask2"][0])[0]] = np.nan
    assert same_bits(run(c, p1=p1, p2=p2), r)


def test_nan_at_a_valid_point_poisons_its_item_only():
    from omnifusion_amd.supervision import chamfer_distance
    c, r = cc.case("G21a"), result("G21a")
    p2 = c["p2"].copy()
    p2[0, 300, 1] = np.nan                                                     # a target of item 0, in its second tile
    bad = run(c, p2=p2, grads=False)
    assert np.isnan(bad["loss"]) and np.isnan(bad["dist"][0]).all() and (bad["idx"][0] == -1).all()
    assert np.array_equal(bits(bad["dist"][1]), bits(r["dist"][1])) and np.array_equal(bad["idx"][1], r["idx"][1])
    items = [chamfer_distance(t(c["p1"][b:b + 1]), t(p2[b:b + 1])) for b in range(2)]
    assert bool(torch.isnan(items[0])) and bool(torch.isfinite(items[1]))
    p1 = c["p1"].copy()
    p1[1, 7, 2] = np.nan                                                       # a query: its own distance only
    bad = run(c, p1=p1, grads=False)
    keep = np.ones(300, bool)
    keep[7] = False
    assert np.isnan(bad["loss"]) and np.isnan(bad["dist"][1, 7]) and bad["idx"][1, 7] == -1
    assert np.array_equal(bits(bad["dist"][1, keep]), bits(r["dist"][1, keep])) and np.array_equal(bits(bad["dist"][0]), bits(r["dist"][0]))
    # the split path carries both flags through its merge
    d = cc.case("G21d")
    p2 = d["p2"].copy()
    p2[1, 4000, 0] = np.nan
    bad = run(d, p2=p2, grads=False)
    assert np.isnan(bad["dist"][1]).all() and np.array_equal(bits(bad["dist"][0]), bits(result("G21d")["dist"][0]))
    p1 = d["p1"].copy()
    p1[0, 64, 0] = np.nan
    bad = run(d, p1=p1, grads=False)
    assert np.isnan(bad["dist"][0, 64]) and np.array_equal(bits(bad["dist"][0, :64]), bits(result("G21d")["dist"][0, :64]))


def test_item_without_a_valid_target():
    c, r = cc.case("G21e"), result("G21e")
    mask2 = c["mask2"].copy()
    mask2[1] = False
    e = run(c, mask2=t(mask2))
    v = c["mask1"][1]
    assert np.isposinf(e["dist"][1, v]).all() and not e["dist"][1, ~v].any() and (e["idx"][1] == -1).all() and np.isposinf(e["loss"])
    assert not e["g1"][1].any() and not e["g2"][1].any()
    for k in ("dist", "idx", "g1", "g2"):
        assert np.array_equal(bits(e[k][0]), bits(r[k][0])), k


def test_distance_map_is_differentiable_and_only_requested_gradients_are_computed():
    """sum(w dist) through nearest_neighbours: grad_p1[i] = w_i u_i, grad_p2 its negated scatter, against the float64 restatement."""
    from omnifusion_amd.supervision import chamfer_distance, nearest_neighbours
    c, g = cc.case("G21a"), golden("G21a_chamfer")
    B, N, M, D = cc.SHAPES["G21a"]
    w = 0.25 + 3.0 * np.random.default_rng(5).random((B, N))
    a, b = t(c["p1"]).requires_grad_(True), t(c["p2"]).requires_grad_(True)
    dist, idx = nearest_neighbours(a, b)
    assert not idx.requires_grad and dist.requires_grad
    (dist * t(w, dtype=torch.float32)).sum().backward()
    want1 = g["grad_p1"] * w[..., None]
    want2 = np.zeros_like(g["grad_p2"])
    for bb in range(B):
        np.add.at(want2[bb], g["idx"][bb], -want1[bb])
    assert cc.rel_error(a.grad.cpu().numpy(), want1).max() <= 1e-5 and cc.rel_error(b.grad.cpu().numpy(), want2).max() <= 1e-5
    a2, b2 = t(c["p1"]).requires_grad_(True), t(c["p2"])
    chamfer_distance(a2, b2).backward()
    assert b2.grad is None and np.array_equal(bits(a2.grad.cpu().numpy()), bits(result("G21a")["g1"]))
    a3, b3 = t(c["p1"]), t(c["p2"]).requires_grad_(True)
    chamfer_distance(a3, b3).backward()
    assert a3.grad is None and np.array_equal(bits(b3.grad.cpu().numpy()), bits(result("G21a")["g2"]))
    # the upstream gradient is a device scalar: it scales both gradients
    a4, b4 = t(c["p1"]).requires_grad_(True), t(c["p2"]).requires_grad_(True)
    (chamfer_distance(a4, b4) * 0.5).backward()
    assert np.array_equal(a4.grad.cpu().numpy(), 0.5 * result("G21a")["g1"]) and np.abs(b4.grad.cpu().numpy() - 0.5 * result("G21a")["g2"]).max() <= 1e-6


def test_depth_chamfer():
    from omnifusion_amd.spherical.grid import spherical_grid_of
    from omnifusion_amd.supervision import chamfer_distance, depth_chamfer
    B, H, W = 2, 8, 16
    rng = np.random.default_rng(11)
    pred, gt = 1.0 + 2.0 * rng.random((B, 1, H, W), dtype=np.float32), 1.0 + 2.0 * rng.random((B, 1, H, W), dtype=np.float32)
    mask = rng.random((B, 1, H, W)) < 0.8
    sg = spherical_grid_of(H, W, device=DEV)
    p, th = sg[0, 0], sg[0, 1]
    rays = torch.stack((-(torch.cos(p) * torch.cos(th)), torch.sin(th), torch.sin(p) * torch.cos(th)), dim=-1)      # [H,W,3], unit
    assert float((rays.norm(dim=-1) - 1).abs().max()) <= 1e-6
    for stride in (1, 2):
        x = t(pred).requires_grad_(True)
        loss = depth_chamfer(x, t(gt), t(mask), stride=stride)
        r = rays[::stride, ::stride]
        pts = lambda d: (r.unsqueeze(0) * t(d)[:, 0, ::stride, ::stride].unsqueeze(-1)).reshape(B, -1, 3)
        m = t(mask)[:, 0, ::stride, ::stride].reshape(B, -1)
        want = chamfer_distance(pts(pred), pts(gt), m, m)
        assert loss.dim() == 0 and abs(float(loss.detach()) - float(want)) <= 1e-6 * abs(float(want))
        loss.backward()
        gr = x.grad.cpu().numpy()
        used = np.zeros_like(mask)
        used[:, :, ::stride, ::stride] = mask[:, :, ::stride, ::stride]
        assert np.isfinite(gr).all() and not gr[~used].any() and np.abs(gr[used]).max() > 0
    for md in (t(mask).to(torch.uint8), t(mask).float()):
        assert float(depth_chamfer(t(pred), t(gt), md)) == float(depth_chamfer(t(pred), t(gt), t(mask)))
