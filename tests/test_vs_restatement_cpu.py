"""CPU: the float64 restatement of view synthesis (tests/_vs_restatement.py) is the reference's arithmetic — proved against the
fixtures G14a-e, G15a-e and G16a-c under the gates their GPU tests apply, and, where the reference checkout is present, against the
reference's own functions at every case of tests/_vs_shape_cases.py — and those cases reach what they are there for: the
restatement's own float32 run stays inside the gates of tests/test_vs_shapes_gpu.py (GAPS), and the splat tiles lie where the
case table says with respect to the LDS window."""
import numpy as np
import pytest
import torch

import _dibr_cases as dc
import _vs_cases as vc
import _vs_restatement as rs
import _vs_shape_cases as sc
from _util import assert_close_outliers, golden
from oracle import ref_loader

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")


# ------------------------------------------------------------------ the restatement against the fixtures
@pytest.mark.parametrize("name", dc.NAMES)
def test_restatement_against_forward_fixtures(name):
    """G14a-e hold the reference's float32 run.  The restatement's float32 run is that run bit for bit (same operations, same scatter
    order); its float64 run passes the gate of test_dibr_gpu.py at every element where float32 and float64 take the same discrete
    steps: the 2 / 1 / 1 elements of G14c / d / e over 1e-4 are exactly elements where the restatement's own two precisions part by as
    much (a corner weight or a floor on the other side of its step in float32), none over 1e-2 — a property of the fixture's precision."""
    c, g = dc.case(name), golden(name + "_dibr")
    r32, r64 = sc.run_dibr(c, torch.float32, grad=False), sc.run_dibr(c, torch.float64, grad=False)
    assert np.array_equal(r32["recon"], g["recon"])
    d = np.abs(r64["recon"] - g["recon"])
    own = np.abs(r64["recon"] - r32["recon"].astype(np.float64))
    tol = 1e-3 if name == "G14e" else 1e-4
    print(f"{name}: float64 max |d| {d.max():.3e}, over {tol}: {int((d > tol).sum())}")
    assert ((d > tol) <= (own > tol)).all() and (d > tol).sum() <= 2 and d.max() <= 1e-2
    if name == "G14e":
        assert_close_outliers(r64["recon"], g["recon"], tol=1e-3, max_tol=1e-1, frac=1e-3, what=name)
    if "mask" in r64:
        assert np.array_equal(r64["mask"].astype(np.uint8), g["mask"]) and np.array_equal(r32["mask"], r64["mask"])


@pytest.mark.parametrize("name", vc.DIBR_NAMES)
def test_restatement_against_gradient_fixtures(name):
    """The gate of test_dibr_bwd_gpu.py (share over 1e-4 <= 2e-4, none over 1e-2, GRAD_OUTLIERS) with both sides in float64: in fact
    no element over 1e-6 (the fixtures are float64 results stored as float32), NaN exactly where the fixture has NaN."""
    c, g = vc.dibr_case(name), golden(name + "_dibr_bwd")
    r = sc.run_dibr(c, torch.float64)
    for k in vc.dibr_grad_names(c):
        mine, want = r["grad_" + k], g["grad_" + k]
        assert np.array_equal(np.isfinite(mine), np.isfinite(want)), (name, k)
        e = vc.rel_error(mine, want)
        print(f"{name} {k}: max {e.max():.3e}")
        assert e.max() <= 1e-6, (name, k, float(e.max()))
    if c["kind"] != "render":
        assert np.array_equal(~np.isfinite(r["grad_depth"]), c["depth"] == 0)


def _separable_ssim(x, y, window, std, mode):
    """The SSIM map by the kernel's route — rows, then columns, float64, zeros beyond the image — in plain numpy loops over the taps."""
    r = window // 2
    w = rs.window_1d(window, std, torch.float64).numpy() if mode == "gaussian" else np.full(window, 1.0 / window)

    def win(z):
        zp = np.pad(z, ((0, 0), (0, 0), (r, r), (r, r)))
        rows = sum(w[k] * zp[..., :, k:k + z.shape[-1]] for k in range(window))
        return sum(w[k] * rows[..., k:k + z.shape[-2], :] for k in range(window))
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    if mode == "box":
        inner = np.zeros_like(s)
        inner[..., r:s.shape[-2] - r, r:s.shape[-1] - r] = s[..., r:s.shape[-2] - r, r:s.shape[-1] - r]
        return inner
    return s


@pytest.mark.parametrize("name", vc.PHOTO_NAMES)
def test_restatement_against_photometric_fixtures(name):
    """The gates of test_photometric_gpu.py: loss within 2e-6, gradient within 1e-4 of the largest at every element, SSIM map within
    2e-6 of a second float64 evaluation (here the kernel's separable route in numpy).  Measured: 1e-9, 3.4e-7, 1e-15."""
    c, g = vc.photo_case(name), golden(name + "_photometric")
    r = sc.run_photo(c, torch.float64)
    e = vc.rel_error(r["grad"], g["grad"])
    print(f"{name}: loss |d| {abs(r['loss'] - float(g['loss'])):.2e}, grad max rel {e.max():.2e}")
    assert abs(r["loss"] - float(g["loss"])) <= 2e-6 and e.max() <= 1e-4
    assert abs(r["dssim_min"] - float(g["dssim_min"])) <= 2e-6 and abs(r["dssim_max"] - float(g["dssim_max"])) <= 2e-6
    m = c["mask"].astype(np.float64)
    want = _separable_ssim(c["pred"] * m, c["gt"] * m, c["window"], c["std"], c["mode"])
    assert np.abs(r["ssim"] - want).max() <= 2e-6


@pytest.mark.parametrize("name", sc.PHOTO_NAMES)
def test_ssim_map_two_routes_at_the_new_cases(name):
    c = sc.photo_case(name)
    m = c["mask"].astype(np.float64)
    want = _separable_ssim(c["pred"] * m, c["gt"] * m, c["window"], c["std"], c["mode"])
    assert np.abs(sc.reference64(name)["ssim"] - want).max() <= 1e-12


# ------------------------------------------------------------------ the restatement against the reference at the new cases
def _finite_coords(c):
    """The reference's render is undefined for a non-finite coordinate (an out-of-range scatter index): for the
    reference's run such a source aims far off the image instead, where every corner is gated out — dropped, as the kernel drops it."""
    if c["kind"] != "render":
        return c
    bad = ~np.isfinite(c["coords"]).all(axis=1, keepdims=True)
    return dict(c, coords=np.where(bad, np.float32(-100.5), c["coords"]))


@needs_reference
@pytest.mark.parametrize("name", sc.DIBR_NAMES)
def test_restatement_against_reference_dibr(name):
    c = sc.dibr_case(name)
    cf = _finite_coords(c)
    recon, mask = dc.run_reference(cf)
    r32 = sc.run_dibr(c, torch.float32, grad=False)
    assert np.array_equal(r32["recon"], recon)                               # float32: the reference's run bit for bit
    if mask is not None:
        assert np.array_equal(r32["mask"], mask)
    want = vc.reference_dibr_grads(cf, torch.float64)
    ref = sc.reference64(name)
    for k in vc.dibr_grad_names(c):
        assert np.array_equal(np.isfinite(ref["grad_" + k]), np.isfinite(want[k])), (name, k)
        e = sc.rel_error(name, k, want[k], ref)
        print(f"{name} {k}: max {e.max():.3e}")
        assert e.max() <= 1e-9, (name, k, float(e.max()))


@needs_reference
@pytest.mark.parametrize("name,alpha", [(n, 0.85) for n in sc.PHOTO_NAMES] + [("P6", 0.0), ("P6", 1.0)])
def test_restatement_against_reference_photometric(name, alpha):
    """The reference multiplies the 1-D Gaussian into its 2-D window in float32 (one more rounding, 6e-8 of every weight); the kernel
    and the restatement widen the 1-D float32 values and multiply in float64.  With the window built the reference's way the
    restatement is the reference to 1e-9; the kernel's way moves the loss by at most 2e-7 and the gradient by at most 4e-6 of its
    largest (P4, whose narrow window amplifies it; the others 1e-10 and 5e-8) — far inside the gates, 2e-6 and 1e-4."""
    c = sc.photo_case(name, alpha)
    loss, p, hmin, hmax = vc.reference_photo(c, torch.float64)
    loss.backward()
    top = np.abs(p.grad.numpy()).max()
    for as_reference, tl, tg in ((True, 1e-9, 1e-9), (False, 2e-7, 4e-6)):
        r = sc.run_photo(c, torch.float64, window_2d_float32=True) if as_reference else sc.reference64(name, alpha)
        dl, dg = abs(float(loss.detach()) - r["loss"]), np.abs(p.grad.numpy() - r["grad"]).max() / top
        print(f"{name} alpha {alpha} window as the reference {as_reference}: loss |d| {dl:.2e}, grad max rel {dg:.2e}")
        assert dl <= tl and dg <= tg
        if as_reference:
            assert abs(hmin - r["dssim_min"]) <= 1e-9 and abs(hmax - r["dssim_max"]) <= 1e-9


@needs_reference
def test_empty_mask_item_is_nan_in_the_reference_too():
    c = sc.p6_with_empty_item()
    assert np.isnan(float(vc.reference_photo(c, torch.float64)[0].detach())) and np.isnan(sc.run_photo(c, torch.float64, grad=False)["loss"])


# ------------------------------------------------------------------ the restatement alone under the gates of the GPU tests
def measure_dibr(name):
    """-> the GAPS row of a DIBR / render case: quantity -> (largest error, elements over the ceiling's tolerance, elements)."""
    c, a = sc.dibr_case(name), sc.reference64(name)
    b = sc.run_dibr(c, torch.float32)
    d = np.abs(a["recon"] - b["recon"])
    row = {"recon": (float(d.max()), int((d > sc.CEILING["recon"][0]).sum()), d.size)}
    if "mask" in a:
        row["mask"] = (int((a["mask"] != b["mask"]).sum()), 0, a["mask"].size)
    for k in vc.dibr_grad_names(c):
        e = sc.rel_error(name, k, b["grad_" + k], a)
        row["grad_" + k] = (float(e.max()), int((e > sc.CEILING["grad"][0]).sum()), e.size)
    return row


def measure_photo(name, alpha):
    c, a = sc.photo_case(name, alpha), sc.reference64(name, alpha)
    b = sc.run_photo(c, torch.float32)
    top = np.abs(a["grad"]).max()
    e = np.abs(b["grad"] - a["grad"]) / top
    d = np.abs(a["ssim"] - b["ssim"])
    return {"loss": (abs(a["loss"] - b["loss"]), 0, 1), "grad": (float(e.max()), int((e > sc.CEILING["pgrad"][0]).sum()), e.size),
            "ssim": (float(d.max()), int((d > sc.CEILING["ssim"][0]).sum()), d.size)}


def _check_row(key, row, kinds):
    """The measured row against the committed one (within a factor 1.5 both ways: another libm or BLAS may move the last bits of a
    float32 run, not its size), and the conditions: no more than 1e-3 of a tensor's elements outside a gate, none beyond its bound."""
    want = sc.GAPS[key]
    assert sorted(row) == sorted(want), key
    for q, (gap, over, n) in row.items():
        wgap, wover, wn = want[q]
        print(f"{key} {q}: measured ({gap:.2e}, {over}, {n}), committed ({wgap:.2e}, {wover}, {wn})")
        assert n == wn and over <= wover, (key, q)
        assert gap <= 1.5 * wgap and wgap <= 1.5 * gap + 1e-12, (key, q, gap, wgap)
        if q == "mask":
            assert gap == 0, (key, "mask flips between float32 and float64")
            continue
        if kinds[q] is None:                                                # recorded only (the SSIM map: see the test's docstring)
            continue
        tol, share, max_tol = sc.CEILING[kinds[q]]
        assert over <= min(share, 1e-3) * n and gap <= max_tol, (key, q, gap, over, n)


@pytest.mark.parametrize("name", sc.DIBR_NAMES)
def test_float32_restatement_stays_inside_the_gates_dibr(name):
    _check_row(name, measure_dibr(name), dict(recon="recon", mask="mask", grad_img="grad", grad_depth="grad", grad_coords="grad"))


@pytest.mark.parametrize("name,alpha", [(n, 0.85) for n in sc.PHOTO_NAMES] + [("P6", 0.0), ("P6", 1.0)])
def test_float32_restatement_stays_inside_the_gates_photometric(name, alpha):
    """Loss and gradient: inside the gates.  The SSIM map is recorded only: its gate (2e-6, test_ssim_map_against_torch) is a gate
    between two float64 evaluations — the kernel's window sums are float64 because float32 sums leave 1e-4 in sigma^2 against C2
    (DESIGN.md §11), which is what the float32 restatement shows here (up to 2e-4) — so it is never tightened below its ceiling.
    (1 - ssim) / 2 stays inside [0, 1): the clamp's upper step is not reached, and 0 only where pred == gt over a whole window."""
    _check_row((name, alpha), measure_photo(name, alpha), dict(loss="loss", grad="pgrad", ssim=None))
    ref = sc.reference64(name, alpha)
    assert 0.0 <= ref["dssim_min"] and ref["dssim_max"] <= 0.5 + 1e-12            # 0.5: the zero border ring of the 'box' map


# ------------------------------------------------------------------ structure: the cases reach what they are there for
def test_splat_tiles_lie_where_the_case_table_says():
    """box * (C + 1) of every splat tile against DIBR_WIN = 6144, from the restatement's float64 coordinates.

    R3 (integer shift, C = 5): the tile whose 16 x 64 sources all stay on the image fills the window exactly, 1024 * 6 = 6144 (the
    others lose the 3 columns / 2 rows that leave the image).  R3h (shift + 0.5): the same tile is 17 * 65 * 6 = 6630 words — over
    the window, by 1.08: at 2 x 5 x 32 x 128 no shift can reach 1.2 x, and the coordinates are exact in float32 (x.5), so no margin for
    round-off is needed.  R5 (noise): every tile more than 1.2 x over.  V1 (C = 2), R4 (C = 8) and Hz2 (C = 3) have tiles on both
    sides.  R1 (2 x 2 x 20 x 72) cannot: its whole image is 1440 * 3 = 4320 words, so every tile sums in LDS."""
    words = {n: sc.tile_words(sc.dibr_case(n)) for n in sc.DIBR_NAMES}
    w = lambda n: [t[3] for t in words[n]]
    for n in sc.DIBR_NAMES:
        print(n, sorted(w(n))[:3], "...", sorted(w(n))[-3:])
    interior = lambda n: [t[3] for t in words[n] if (t[1], t[2]) == (1, 0)]                 # rows 16 .. 31, columns 0 .. 63: shifted by (3, -2), all on the image
    assert interior("R3") == [sc.DIBR_WIN] * 2 and max(w("R3")) == sc.DIBR_WIN
    assert interior("R3h") == [17 * 65 * 6] * 2 and 17 * 65 * 6 > sc.DIBR_WIN
    assert min(w("R5")) > 1.2 * sc.DIBR_WIN
    for n in ("V1", "R4", "Hz2"):
        assert min(w(n)) <= 0.8 * sc.DIBR_WIN and max(w(n)) > sc.DIBR_WIN, (n, min(w(n)), max(w(n)))
    assert max(w("Hz2")) > 1.2 * sc.DIBR_WIN
    assert max(w("R1")) <= sc.DIBR_WIN and max(w("R2")) <= sc.DIBR_WIN and max(w("V2")) <= sc.DIBR_WIN and max(w("Hz1")) <= sc.DIBR_WIN


def test_r5_has_crowded_targets_and_its_edge_sources():
    c = sc.dibr_case("R5")
    n = sc.contributions(c)
    print("R5: most contributions to one target", int(n.max()))
    assert n.max() > 16
    co = c["coords"][0, :, 0, :2 * sc.R5_EDGE_SOURCES:2]
    H, W = c["img"].shape[-2:]
    assert (~np.isfinite(co)).any(axis=0).sum() == 5
    for val in (-1.0, 0.0, W - 1.0):
        assert (co[0] == val).any()
    for val in (-1.0, 0.0, H - 1.0):
        assert (co[1] == val).any()
    assert (co[0] > W).any() and (co[1] > H).any() and (co[0] < -1).any()
    # what the kernel documents: a source at exactly -1 keeps no corner (its in-image corner has weight 0), one at 0 or W - 1 keeps one
    alive = sum(a[0, 0, :2 * sc.R5_EDGE_SOURCES:2].astype(int) for a, _, _ in sc.survivors(sc.target_coordinates(c), H, W))
    assert alive[0] == 0 and alive[8] == 0 and alive[7] == 1 and alive[6] == 1 and (alive[9:] == 0).all()


def test_hz2_wraps_inside_the_image():
    """Sources whose column plus displacement is >= 512 (u + 512 >= 1024 before the fmod) land on columns below W - 512 = 32; and
    Hz1's negative u wraps to beyond W = 72, off the image."""
    c = sc.dibr_case("Hz2")
    H, W = c["img"].shape[-2:]
    u = sc.target_coordinates(c)[0, 0]
    src = np.broadcast_to(np.arange(W)[None, :], (H, W))
    folded = (src >= 512) & (u < W - 512)
    print("Hz2: sources folded by the literal 512:", int(folded.sum()))
    assert folded.sum() >= 0.5 * H * (W - 512) and (u < 512).all()
    c1 = sc.dibr_case("Hz1")
    u1 = sc.target_coordinates(c1)[0, 0]
    assert (u1 > c1["img"].shape[-1]).sum() > 0
