"""CPU: the float64 yardstick of equi2pers / pers2equi (tests/_resample_cases.py) is proved before any kernel is held to it.

  * the restatement, in float32 and in float64 mode, against the reference's own goldens at the gates tests/test_oracle_golden.py and
    tests/test_backward_oracle.py use for the C oracle;
  * the C oracle against it on the cases of tests/test_resample_float64_gpu.py, through the SAME comparison rules the kernels get there (the oracle
    stands in for a kernel: its masks equal float64's outside the near entries, its blend at its own coordinates is within 5 * 2^-24);
  * the conditions those rules rest on, from float64 alone: few skipped pixels; and `e32`, the distance of the float32 restatement from the float64
    one, from which the GPU gates are computed, printed for every case and quantity."""
import json
import os

import numpy as np
import pytest
import torch

import _resample_cases as rc
from oracle import c_oracle as co
from _util import GOLDEN, assert_close_outliers, golden, rng_uniform

DTYPES = [rc.F32, rc.F64]
ids = lambda d: str(d).split(".")[-1]


# ---------------------------------------------------------------------------------------------------------------- the reference's own goldens
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ["G1_equi2pers_n4", "G2_equi2pers_n6", "G2b_equi2pers_n3", "G2b_equi2pers_n5", "G2c_equi2pers_rect"])
def test_equi2pers_golden(name, dtype):
    g = golden(name)
    fov = tuple(float(v) for v in g["fov"]); P = tuple(int(v) for v in g["patch"]); nrows = int(g["nrows"])
    c = rc.e2p_coords(nrows, fov, P, g["erp"].shape[2:], dtype)
    pers = rc.equi2pers(g["erp"], fov, nrows, P, dtype=dtype)
    assert pers.dtype == dtype and pers.shape == g["pers"].shape
    assert_close_outliers(pers.numpy(), g["pers"], tol=1e-3, max_tol=2e-2, frac=2e-5, what=name)
    np.testing.assert_allclose(rc.xyz_of(c["lon"], c["lat"]).numpy(), g["xyz"], atol=1e-4)
    np.testing.assert_allclose(rc.uv_strip(c["u"], c["v"]).numpy(), g["uv"], atol=1e-4)
    np.testing.assert_array_equal(rc.patch_centers(nrows, 0)[2].numpy(), g["center_p"])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ["G2d_equi2pers_odd", "G2d_equi2pers_odd2"])
def test_equi2pers_odd_patch_quirk(name, dtype):
    """q4: the NaN of the centre sample sits where the reference's does, and that sample reads row 0"""
    g = golden(name)
    P = tuple(int(v) for v in g["patch"]); nrows = int(g["nrows"])
    c = rc.e2p_coords(nrows, (80, 80), P, g["erp"].shape[2:], dtype)
    xyz = rc.xyz_of(c["lon"], c["lat"]).numpy()
    np.testing.assert_array_equal(np.isnan(xyz), np.isnan(g["xyz"]))
    np.testing.assert_allclose(np.nan_to_num(xyz), np.nan_to_num(g["xyz"]), atol=1e-4)
    assert_close_outliers(rc.equi2pers(g["erp"], (80, 80), nrows, P, dtype=dtype).numpy(), g["pers"], tol=1e-3, max_tol=2e-2, frac=1e-3, what=name)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", ["G3_pers2equi_n4", "G3b_pers2equi_n3", "G3b_pers2equi_n5", "G4_pers2equi_n6", "G4b_pers2equi_fov"])
def test_pers2equi_golden(name, dtype):
    g = golden(name)
    fov = tuple(float(v) for v in g["fov"]); P = g["pers"].shape[2]
    tab = rc.p2e_tables(int(g["nrows"]), fov, (P, P), tuple(int(v) for v in g["erp_size"]), dtype)
    erp = rc.pers2equi(g["pers"], tab)
    assert erp.dtype == dtype
    np.testing.assert_allclose(erp.numpy(), g["erp"], atol=2e-4, rtol=0)
    if "n3" in name:
        assert (g["erp"] == 0).sum() > 0 and (erp.numpy()[g["erp"] == 0] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("nrows", [3, 4, 5, 6])
def test_pers2equi_tables_golden(nrows, dtype):
    """G5: the predicates themselves.  Masks differ from the reference's only at near entries of the float64 tables; where both are valid the clamped taps
    are the reference's."""
    g = golden(f"G5_tables_n{nrows}")
    P = int(g["patch"]); size = tuple(int(v) for v in g["erp_size"])
    tab = rc.p2e_tables(nrows, (80, 80), (P, P), size, dtype)
    near = rc.near_entries(rc.p2e_tables(nrows, (80, 80), (P, P), size, rc.F64)).numpy()
    diff = tab["mask"].numpy() != (g["mask"] == 1)
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    x0, x1, y0, y1 = (t.long().numpy() for t in rc._clamped_taps(tab["X"], tab["Y"], P, P))
    both = tab["mask"].numpy() & (g["mask"] == 1)
    # a floor may differ only where the coordinate is within 1e-3 px of an integer (the gate of tests/test_oracle_golden.py for these tables)
    on_cell_edge = {k: ((t - torch.round(t)).abs() < 1e-3).numpy() for k, t in (("x", tab["X"]), ("y", tab["Y"]))}
    for mine, k in ((x0, "x0"), (x1, "x1"), (y0, "y0"), (y1, "y1")):
        diff = (mine != g[k]) & both
        assert not (diff & ~on_cell_edge[k[0]]).any(), k
        assert diff.mean() < 1e-2, k


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_backward_goldens(dtype):
    """G10 / G11: gradients of the reference functions by its own autograd"""
    for name in ("G10_e2p_bwd", "G10b_e2p_bwd_n6"):
        g = golden(name)
        H, W, nrows, P, B, C = (int(v) for v in g["meta"])
        got = rc.equi2pers_bwd(g["grad_pers"], (H, W), (80, 80), nrows, dtype=dtype)
        assert_close_outliers(got.numpy(), g["grad_erp"], tol=2e-4, max_tol=2e-3, frac=1e-4, what=name)
    for name in ("G11_p2e_bwd", "G11b_p2e_bwd_n6"):
        g = golden(name)
        H, W, nrows, P, B, C = (int(v) for v in g["meta"])
        got = rc.pers2equi_bwd(g["grad_erp"], rc.p2e_tables(nrows, (80, 80), (P, P), (H, W), dtype), nrows)
        assert_close_outliers(got.numpy(), g["grad_pers"], tol=2e-4, max_tol=2e-3, frac=1e-4, what=name)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_known_answer_subsamples(dtype):
    """G8: the strided sub-samples of the reference's outputs at 512x1024 -> 18 x 256^2 and 1024x2048 -> 46 x 256^2 (pers2equi evaluated on the
    sub-sampled rows and columns only: every pixel is independent)"""
    g = golden("G8_config1")
    c = rc.e2p_coords(4, (80, 80), (256, 256), (512, 1024), dtype)
    pers = rc.equi2pers(rng_uniform(100, (1, 3, 512, 1024)), (80, 80), 4, (256, 256), dtype=dtype, coords=(c["ix"], c["iy"])).numpy()
    ka = json.load(open(os.path.join(GOLDEN, "G8_config1.json")))
    assert abs(pers.astype(np.float64).sum() - ka["pers_sum"]) < 0.5
    assert_close_outliers(pers[:, :, ::8, ::8, :], g["pers_sub"], tol=1e-3, max_tol=2e-2, frac=5e-5)
    np.testing.assert_allclose(rc.xyz_of(c["lon"], c["lat"]).numpy()[:, :, ::8, ::8], g["xyz_sub"], atol=1e-4)
    np.testing.assert_allclose(rc.uv_strip(c["u"], c["v"]).numpy()[:, :, ::8, ::8], g["uv_sub"], atol=1e-4)
    pin = rng_uniform(101, (1, 1, 256, 256, 18))
    sub = rc.p2e_tables(4, (80, 80), (256, 256), (512, 1024), dtype, rows=np.arange(0, 512, 4), cols=np.arange(0, 1024, 4))
    np.testing.assert_allclose(rc.pers2equi(pin, sub).numpy(), g["erp_sub"], atol=2e-4)
    rows = rc.p2e_tables(4, (80, 80), (256, 256), (512, 1024), dtype, rows=np.array([0, 1, 255, 256, 510, 511]))
    np.testing.assert_allclose(rc.pers2equi(pin, rows).numpy(), g["erp_rows"], atol=2e-4)
    g3 = golden("G8_config3")
    p3 = rc.equi2pers(rng_uniform(102, (1, 1, 1024, 2048)), (80, 80), 6, (256, 256), dtype=dtype).numpy()
    assert_close_outliers(p3[:, :, ::8, ::8, :], g3["pers_sub"], tol=1e-3, max_tol=2e-2, frac=1e-4)
    sub = rc.p2e_tables(6, (80, 80), (256, 256), (1024, 2048), dtype, rows=np.arange(0, 1024, 8), cols=np.arange(0, 2048, 8))
    np.testing.assert_allclose(rc.pers2equi(rng_uniform(103, (1, 1, 256, 256, 46)), sub).numpy(), g3["erp_sub"], atol=2e-4)


def test_scramble_is_a_permutation_and_centres_are_the_oracles():
    nat = torch.arange(10 * 3 * 7, dtype=rc.F64).reshape(10, 3, 7)
    scr = rc.scramble(nat)
    assert torch.equal(rc.unscramble(scr), nat) and not torch.equal(scr, nat)
    for b, h, a in ((0, 0, 0), (3, 2, 5), (9, 1, 6)):          # uv[b, h, a] = strip[h, a*N + b], strip[h, n*pw + w] = nat[n, h, w]
        s = a * 10 + b
        assert scr[b, h, a] == nat[s // 7, h, s % 7]
    for nrows in (3, 4, 5, 6):
        for which in (0, 1):
            for mine, theirs in zip(rc.patch_centers(nrows, which), co.patch_centers(nrows, which)):
                np.testing.assert_array_equal(mine.numpy(), theirs)
    assert abs(np.degrees(float(rc.patch_centers(3, 1)[1][0])) + 59.6) < 1e-4 and abs(np.degrees(float(rc.patch_centers(3, 0)[1][0])) + 60) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- the C oracle as the kernel
@pytest.mark.parametrize("name", list(rc.E2P_CASES))
def test_equi2pers_oracle_through_the_gpu_rules(name):
    """(a) the oracle's coordinates within 4 * max(e32, 16 * 2^-24 * scale) of float64, NaN where float64's is; (b) its blend within 5 * 2^-24 of the
    float64 blend at its own coordinates; its backward within the gate of the float64 transpose at those coordinates."""
    case = rc.e2p_case(name)
    nrows, patch, (H, W) = case["nrows"], case["patch"], case["erp_size"]
    x = rng_uniform(801, (case["planes"][-1], 1, H, W))
    ref, rxyz, ruv, _ = co.equi2pers(x, rc.FOV, nrows, patch)
    u, v = (rc.unscramble(torch.from_numpy(ruv[:, k])).numpy() for k in (0, 1))
    e32 = rc.e2p_coord_e32(case)
    err = rc.e2p_coord_errors(case["c64"], u, v, rxyz, H, W)
    for k, scale in (("x", W), ("y", H), ("xyz", 1)):
        print(f"{name} {k}: e32 {e32[k]:.3e}  oracle {err[k]:.3e}  gate {rc.gate(e32[k], scale):.3e}")
        assert err[k] <= rc.gate(e32[k], scale), k
    np.testing.assert_array_equal(np.isnan(v), torch.isnan(case["c64"]["v"]).numpy())
    np.testing.assert_array_equal(np.isnan(rxyz), torch.isnan(rc.xyz_of(case["c64"]["lon"], case["c64"]["lat"])).numpy())
    assert int(np.isnan(v).sum()) == (case["N"] if name == "n6_odd" else 0)
    coords = rc.sampling_coords_f32(u, v, H, W)
    want = rc.equi2pers(x, rc.FOV, nrows, patch, coords=coords).numpy()
    units = np.abs(ref - want).max() / (rc.U24 * x.max())
    print(f"{name} blend at the oracle's coordinates: {units:.2f} units of 2^-24 (gate 5)")
    assert units <= 5.0
    gp = rng_uniform(802, ref.shape)
    want = rc.equi2pers_bwd(gp, (H, W), coords=coords)
    b32 = rc.equi2pers_bwd(gp, (H, W), coords=coords, dtype=rc.F32).to(rc.F64)
    mass = float(rc.equi2pers_bwd(np.abs(gp), (H, W), coords=coords).max())
    e32b = float((b32 - want).abs().max())
    got = float((torch.from_numpy(co.equi2pers_bwd(gp, rc.FOV, nrows, (H, W))).to(rc.F64) - want).abs().max())
    print(f"{name} backward: e32 {e32b:.3e}  oracle {got:.3e}  gate {rc.gate(e32b, mass):.3e}  (largest sum of |terms| {mass:.1f})")
    assert got <= rc.gate(e32b, mass)
    if name == "n6_odd":
        # The q4 NaN sample: the forward reads row 0 there (the clip sends the NaN to 0), and the transpose puts its gradient into row 0.  A backward that
        # dropped the sample instead (what the kernels' comments once said) is NOT what the oracle computes, and is not the transpose of the forward:
        nan = torch.from_numpy(np.isnan(v))
        dropped = rc.equi2pers_bwd(gp, (H, W), coords=coords, drop=nan)
        assert float((torch.from_numpy(co.equi2pers_bwd(gp, rc.FOV, nrows, (H, W))).to(rc.F64) - dropped).abs().max()) > 0.1
        y = torch.from_numpy(gp).to(rc.F64)
        lhs = float((rc.equi2pers(x, coords=coords) * y).sum())
        assert abs(lhs - float((torch.from_numpy(x).to(rc.F64) * want).sum())) <= 1e-9 * abs(lhs)
        assert abs(lhs - float((torch.from_numpy(x).to(rc.F64) * dropped).sum())) > 1e-6 * abs(lhs)


@pytest.mark.parametrize("name", list(rc.P2E_CASES))
def test_pers2equi_oracle_through_the_gpu_rules(name):
    """(c) masks equal float64's outside the near entries; the blend and the confidence blend through the flip rule; (d) the backward with the gradient
    zeroed at pixels that have a near entry.  Skipped pixels stay within the two pole rows + 0.1 % of the image."""
    case = rc.p2e_case(name)
    nrows, patch, (H, W) = case["nrows"], case["patch"], case["erp_size"]
    tab = co.pers2equi_tables(rc.FOV, nrows, patch, (H, W))
    near = case["near"].numpy()
    for what, m in (("oracle", tab["mask"] > 0), ("float32", case["t32"]["mask"].numpy())):
        diff = m != case["t64"]["mask"].numpy()
        assert not (diff & ~near).any(), f"{what}: {int((diff & ~near).sum())} mask entries differ from float64 away from every bound"
    skipped = int((case["count"] > 2).sum())
    print(f"{name}: {int(near.sum())} near entries in {int((case['count'] > 0).sum())} pixels, {skipped} skipped, {int(case['uncovered'].sum())} uncovered")
    assert skipped <= 2 * W + 1e-3 * H * W
    assert bool(case["uncovered"].any()) == (nrows == 3)
    x = rc.p2e_inputs(case, case["planes"][-1], 811)
    xt = torch.from_numpy(x)
    want, e32 = rc.p2e_references(case, lambda t, f: rc.pers2equi(xt, t, f))
    assert all(bool(torch.isfinite(w).all()) for w in want)
    print(f"{name} blend: e32 {e32:.3e}")
    rc.check_p2e(co.pers2equi(x, rc.FOV, nrows, patch, (H, W)), want, case, rc.gate(e32, float(x.max())), float(x.min()), float(x.max()), name)
    conf = 0.25 + 0.75 * rc.p2e_inputs(case, 2, 812)
    depth = rc.p2e_inputs(case, 2, 813, hi=8.0)
    pw_ = depth * conf
    ct, pt = torch.from_numpy(conf), torch.from_numpy(pw_)
    want, e32 = rc.p2e_references(case, lambda t, f: rc.conf_blend(pt, ct, t, f))
    q = pw_.astype(np.float64) / conf
    print(f"{name} confidence blend: e32 {e32:.3e}")
    rc.check_p2e(co.pers2equi_conf(pw_, conf, rc.FOV, nrows, patch, (H, W)), want, case, rc.gate(e32, float(want[0].abs().max())), float(q.min()), float(q.max()),
                 name + " conf")
    ge = rng_uniform(814, (2, 1, H, W))
    ge[:, :, (case["count"] > 0).numpy()] = 0
    wantb = rc.pers2equi_bwd(ge, case["t64"], nrows)
    e32b = float((rc.pers2equi_bwd(ge, case["t32"], nrows).to(rc.F64) - wantb).abs().max())
    mass = float(rc.pers2equi_bwd(np.abs(ge), case["t64"], nrows).max())
    got = float((torch.from_numpy(co.pers2equi_bwd(ge, rc.FOV, nrows, patch)).to(rc.F64) - wantb).abs().max())
    print(f"{name} backward: e32 {e32b:.3e}  oracle {got:.3e}  gate {rc.gate(e32b, mass):.3e}  (largest sum of |terms| {mass:.1f})")
    assert got <= rc.gate(e32b, mass)


def test_flip_rule_accepts_a_flip_only_at_a_near_entry():
    """The rule itself, on the case with near entries: a result computed with a near entry's mask inverted passes (and is counted), the same change at an
    entry that is not near fails, and so does a planted error of four gates at a pixel without near entries."""
    case = rc.p2e_case("n4_p64")
    x = torch.from_numpy(rc.p2e_inputs(case, 1, 821))
    want, e32 = rc.p2e_references(case, lambda t, f: rc.pers2equi(x, t, f))
    tol = rc.gate(e32, 1.0)
    assert int(((case["count"] == 1) | (case["count"] == 2)).sum()) > 0
    assert float((want[1] - want[0]).abs().max()) > 100 * tol           # a flip is far outside the gate
    assert rc.check_p2e(want[1], want, case, tol, 0.0, 1.0, "flip at near entries")[1] > 0
    far = torch.zeros_like(case["near"])
    n, i, j = np.argwhere((case["t64"]["mask"] & (case["count"] == 0)[None]).numpy())[1000]
    far[n, i, j] = True
    with pytest.raises(AssertionError):
        rc.check_p2e(rc.pers2equi(x, case["t64"], far), want, case, tol, 0.0, 1.0, "flip elsewhere")
    bad = want[0].clone(); bad[0, 0, i, j] += 4 * tol
    with pytest.raises(AssertionError):
        rc.check_p2e(bad, want, case, tol, 0.0, 1.0, "planted error")
