"""CPU: the yardstick of tests/_eval_cases.py (masked median, depth metrics, BerHu, preprocessing, point cloud) is proved before any kernel is
held to it.

  * the restatements against the reference's own goldens (G9, G12, G13) at the gates the existing tests use, and against oracle/metrics_ref.py and
    oracle/io_ref.py on the random cases; `lower_median` against torch.median on every median case, NaN and empty included;
  * the conditions the cases rest on, from the restatements alone: every tie case does what its name says (radix buckets counted in numpy), no
    random metrics element sits within 2^-20 of a delta threshold, the planted block separates a float32 from a float64 compare, the BerHu
    maxima are where the case names put them, the planted rounding ties are ties, and the fractional preprocess case meets the caps of
    test_preprocess_vs_restatement_INTER_AREA_UNPINNED from the reference alone."""
import numpy as np
import pytest
import torch

import _eval_cases as ec
from _util import golden
from oracle import io_ref, metrics_ref

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------- the reference's own goldens
def test_metrics_restatement_golden_G9():
    g = golden("G9_eval_metrics")
    scale = F32(ec.lower_median(g["gt"], g["mask"])) / F32(ec.lower_median(g["pred"], g["mask"]))
    r = ec.metrics(g["pred"], g["gt"], g["mask"], scale)
    np.testing.assert_allclose(r["scaled"].reshape(g["scaled"].shape), g["scaled"], rtol=1e-6)
    np.testing.assert_allclose(r["vals"], g["metrics"], rtol=2e-5)
    assert r["N"] == int(g["N"]) and r["N_log"] < r["N"]


def test_berhu_restatement_golden_G12():
    g = golden("G12_berhu")
    r = ec.berhu(g["pred"], g["gt"], g["mask"], g["weights"])
    assert abs(r["loss"] - float(g["loss"])) <= 2e-6
    assert np.abs(r["grad"] - g["grad"]).max() <= 1e-8
    assert r["grad"][1, 0, 3, 5] == 0.0                                      # exact hit: sign(0) = 0


def test_pointcloud_restatement_golden_G13():
    g = golden("G13_pointcloud")
    assert np.abs(ec.pointcloud64(g["depth"]) - g["pts"]).max() <= 2e-6
    assert np.array_equal(io_ref.pointcloud(g["depth"], g["rgb"])[1], g["col"])


# ---------------------------------------------------------------------------------------------------------------- against the oracle restatements
@pytest.mark.parametrize("n", ec.METRIC_SIZES)
def test_metrics_agree_with_metrics_ref(n):
    pred, gt, mask, scale = ec.metrics_case(n)
    r = ec.metrics(pred, gt, mask, scale)
    scaled, ref, N = metrics_ref.compute_eval_metrics(pred, gt, mask)
    assert np.array_equal(scaled, r["scaled"]) and N == r["N"]
    np.testing.assert_allclose(r["vals"], ref, rtol=1e-10)                   # float64 both; the inliers agree because no ratio is near a threshold
    assert r["counts"] == r["counts64"]


@pytest.mark.parametrize("B,per", ec.BERHU_SIZES[1:])
def test_berhu_agrees_with_io_ref(B, per):
    pred, gt, mask, wt = ec.berhu_case(B, per)
    r = ec.berhu(pred, gt, mask, wt)
    loss, grad = io_ref.berhu_loss(pred, gt, mask, wt)                       # float32 values, float64 sums
    assert abs(r["loss"] - float(loss)) <= 1e-6 * r["loss"]
    assert np.abs(r["grad"] - grad).max() <= 4 * ec.U24 * np.abs(r["grad"]).max()


@pytest.mark.parametrize("fy,fx", ec.PREP_INT_SCALES)
def test_integer_scales_agree_with_io_ref(fy, fx):
    fr, dz, (H, W) = ec.prep_int_case(fy, fx)
    assert np.array_equal(ec.prep_rgb_int(fr, H, W), io_ref.preprocess_rgb(fr, H, W))
    d, m = ec.prep_depth_int(dz, H, W)
    rd, rm = io_ref.preprocess_depth(dz, H, W)
    assert np.array_equal(m, rm) and np.abs(d - rd).max() <= ec.DEPTH_CAP


def test_equal_size_agrees_with_io_ref():
    for name in ("quad", "byte", "b2", "levels"):
        fr = ec.prep_same_case(name)
        assert np.array_equal(ec.prep_rgb_int(fr, *fr.shape[1:3]), io_ref.preprocess_rgb(fr, *fr.shape[1:3]))
    assert sorted(ec.prep_same_case("levels")[0, :, :, 1].ravel().tolist()) == list(range(256))
    assert ec.prep_same_case("quad")[0, :, :, 0].size % 4 == 0 and ec.prep_same_case("byte")[0, :, :, 0].size % 4 != 0
    d, m = ec.prep_depth_int(ec.DEPTH_CODES, 1, ec.DEPTH_CODES.shape[2])
    rd, rm = io_ref.preprocess_depth(ec.DEPTH_CODES, 1, ec.DEPTH_CODES.shape[2])
    assert m.ravel().tolist() == [0, 0, 1, 1, 0, 0, 1] and np.array_equal(m, rm) and np.array_equal(d, rd)
    assert (d[m == 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the median
@pytest.mark.parametrize("name", ec.MEDIAN_CASES)
def test_lower_median_is_torch_median(name):
    x, mask = ec.median_case(name)
    sel = torch.from_numpy(x.copy())[torch.from_numpy(mask.copy()) > 0]
    want = sel.median() if sel.numel() else torch.tensor(float("nan"))      # torch refuses an empty median; the device entry answers NaN
    assert ec.same_median(ec.lower_median(x, mask), want.item()), name
    assert np.isnan(ec.lower_median(x, mask)) == (name in ("nan_pos_selected", "nan_neg_selected", "empty"))


def test_torch_median_of_a_selection_with_nan_is_nan():
    assert torch.isnan(torch.tensor([1.0, float("nan"), 3.0, -2.0, 0.5]).median())
    assert torch.isnan(torch.from_numpy(ec.f32_bits([0x3F800000, 0xFFC00000, 0x40000000])).median())


def test_median_sizes_are_the_launch_edges():
    """256 threads per block, 2048 blocks at most: one ragged block, one full, one more; the cap reached with 257 threads taking a second step; every
    thread taking three steps but the last"""
    cap = 2048 * 256
    assert ec.MEDIAN_SIZES == (1, 2, 255, 256, 257, cap + 257, 3 * cap - 1)
    for n in ec.MEDIAN_SIZES:
        x, mask = ec.median_case(f"n{n}")
        assert x.size == n and 0.6 * n <= (mask > 0).sum() and (n < 255 or (mask > 0).sum() <= 0.8 * n)


def test_median_tie_cases_do_what_their_names_say():
    sel = lambda name: (lambda x, m: x[m > 0])(*ec.median_case(name))
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)
    for name in ("equal_pos", "equal_neg"):
        assert np.unique(sel(name)).size == 1 and sel(name).size > 2000
    s = sel("equal_neg"); assert s[0] < 0 and ec.median_case("equal_neg")[0].size % 2 == 0
    s = sel("u16_codes")
    assert ec.median_case("u16_codes")[0].size == 70001 and np.unique(s).size == 37
    assert np.array_equal(s, (np.rint(s.astype(F64) / 128 * 65535).astype(F32) / F32(65535) * F32(128)).astype(F32))      # u16 codes, scaled
    b = bits(sel("low_byte")); assert np.unique(b >> 8).size == 1 and np.unique(b & 255).size > 200
    b = bits(sel("top_byte")); assert np.unique(b & 0xFFFFFF).size == 1 and np.unique(b >> 24).size > 200 and np.isfinite(sel("top_byte")).all()
    s = np.sort(sel("denormal_middle")); n = s.size
    assert n % 2 == 0 and bits(s[n // 2 - 1: n // 2 + 1]).tolist() == [0x80000001, 0x00000001]
    b = bits(sel("zeros")); assert set(b.tolist()) == {0, 0x80000000} and (b == 0).sum() > 1000 and (b != 0).sum() > 1000
    for name, fin in (("inf_finite_median", True), ("inf_median", False), ("neg_inf_median", False)):
        s = sel(name)
        assert np.isinf(s).any() and np.isfinite(ec.lower_median(*ec.median_case(name))) == fin
    assert ec.lower_median(*ec.median_case("inf_median")) == np.inf and ec.lower_median(*ec.median_case("neg_inf_median")) == -np.inf


@pytest.mark.parametrize("name", ec.MEDIAN_BUCKET)
def test_rank_element_on_a_bucket_edge(name):
    """counted in numpy: in the pass named, the rank element is the LAST key of its bucket with keys of the same prefix in the buckets above, or the
    FIRST of its bucket with keys of the same prefix below: a select that is off by one at either edge lands in the neighbouring bucket"""
    p, which = int(name[4]), name[6:]
    x, mask = ec.median_case(name)
    idx, size, below, above = ec.radix_rank_position(x, mask, p)
    assert size >= 1000
    if which == "last":
        assert idx == size - 1 and above >= 1000
    else:
        assert idx == 0 and below >= 1000
    assert np.isfinite(x).all()


def test_median_mask_and_nan_cases():
    x, mask = ec.median_case("mask_values")
    assert np.isnan(mask).any() and (mask == 0.25).any() and (mask == 2.0).any() and (mask < 0).any() and np.signbit(mask[mask == 0]).any()
    x, mask = ec.median_case("nan_masked_out")
    assert np.isnan(x[mask == 0]).all() and not np.isnan(x[mask > 0]).any() and (mask == 0).sum() > 1000
    for name, sign in (("nan_pos_selected", False), ("nan_neg_selected", True)):
        x, mask = ec.median_case(name)
        k = np.flatnonzero(np.isnan(x))
        assert k.size == 1 and mask[k[0]] > 0 and bool(np.signbit(x[k[0]])) == sign
    assert (ec.median_case("empty")[1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the metrics cases
def test_no_random_ratio_near_a_threshold():
    """outside the planted block no element's float64 ratio lies within 2^-20 relative of 1.25, 1.5625 or 1.953125 (the seeds of METRIC_SEEDS were
    searched for this): the float32 inlier decision of every random element is beyond doubt, so the counts are exact expectations"""
    for n in ec.METRIC_SIZES:
        pred, gt, mask, scale = ec.metrics_case(n)
        r = ec.metrics(pred, gt, mask, scale)
        assert ec.near_threshold(r["ratio64"]) == 0, n
        assert n < 64 or r["N_log"] < r["N"]
    assert ec.METRIC_SIZES[1] % 256 == 1 and ec.METRIC_SIZES[2] % 256 and ec.METRIC_SIZES[3] == 2048 * 256 + 257


def test_planted_block_sits_on_the_thresholds():
    p, g, mask = ec.metrics_planted()
    r = ec.metrics(p, g, mask)
    sel = mask > 0
    with np.errstate(all="ignore"):
        r32 = np.maximum(p[sel] / g[sel], g[sel] / p[sel])
    for t in ec.THRESHOLDS:
        assert (r32 == F32(t)).sum() >= 5 and (r32 == np.nextafter(F32(t), F32(0))).sum() >= 1 and (r32 == np.nextafter(F32(t), F32(2))).sum() >= 1
    assert r["counts"] != r["counts64"]                                      # a float64 compare counts another element
    assert r["counts"][0] == int((r32 < F32(1.25)).sum()) < int((r32 <= F32(1.25)).sum())
    assert r["N"] == int(sel.sum()) == p.size - 2 and r["N"] - r["N_log"] == 5      # 0, -1, 1e-7 and the two denormals; nextafter(1e-7) stays
    assert np.isfinite(r["vals"]).all()


def test_other_metrics_cases():
    r = ec.metrics(*ec.metrics_other("empty"))
    assert r["N"] == 0 and r["N_log"] == 0 and np.isnan(r["vals"]).all()
    r = ec.metrics(*ec.metrics_other("no_log"))
    assert r["N"] > 500 and r["N_log"] == 0 and np.isnan(r["vals"][3]) and np.isfinite(np.delete(r["vals"], 3)).all()
    pred, gt, mask = ec.metrics_other("mask_values")
    r = ec.metrics(pred, gt, mask)
    assert r["N"] == int(((mask == 0.5) | (mask == 2.0)).sum()) and (mask == 0.5).sum() > 100 and (mask == 2.0).sum() > 100


# ---------------------------------------------------------------------------------------------------------------- the BerHu cases
def test_berhu_sizes_are_the_launch_edges():
    assert ec.BERHU_SIZES == ((1, 1), (3, 255), (3, 257), (2, 77100), (2, 270000))
    assert 77100 > 256 * 256 and 77100 % 256 and 2 * 77100 < 2048 * 256 < 2 * 270000


@pytest.mark.parametrize("B,per", ec.BERHU_LARGE)
def test_berhu_maximum_is_where_the_case_puts_it(B, per):
    base = ec.berhu(*ec.berhu_case(B, per))
    assert float(base["c"]) < 2.0
    for placement in ec.BERHU_PLACEMENTS:
        if placement == "beyond_cap" and B * per <= 2048 * 256:
            continue
        pred, gt, mask, wt = ec.berhu_case(B, per, placement)
        r = ec.berhu(pred, gt, mask, wt)
        j = int(np.abs(r["d"]).argmax())
        assert r["c"] == F32(8.0) and np.abs(r["d"]).ravel()[j] == F32(ec.PLANTED_MAX)
        assert (np.abs(r["d"]).ravel() == F32(ec.PLANTED_MAX)).sum() == 1
        assert {"last": j == B * per - 1, "beyond_cap": j > 2048 * 256, "masked_out": mask.ravel()[j] == 0, "item1": j // per == 1}[placement]
        if placement == "masked_out":
            assert np.abs(r["d"])[mask > 0].max() < 8.0                       # a maximum over the masked elements alone would be far smaller
        assert np.abs(r["grad"][0]).max() > 0 and np.isfinite(r["grad"]).all()


def test_berhu_planted_and_other_cases():
    B, per = 3, 257
    pred, gt, mask, wt = ec.berhu_case(B, per, None, "planted")
    r = ec.berhu(pred, gt, mask, wt)
    up = np.nextafter(F32(1), F32(2))
    assert r["c"] == F32(1.0) and r["d"][0, 0, 0, 3:10].tolist() == [5.0, 1.0, -1.0, up, -up, 0.0, np.nextafter(F32(1), F32(0))]
    scale = -(1.0 / B) * wt.astype(F64)[0, 0, 0, 3:10] / r["counts"][0]      # mask 1 there
    np.testing.assert_allclose(r["grad"][0, 0, 0, 3:10] / scale, [5.0, 1.0, -1.0, float(up), -float(up), 0.0, 1.0], rtol=1e-15)
    assert set(np.unique(mask).tolist()) == {0.0, 0.5, 1.0} and wt.min() >= 0.5 and wt.max() <= 2.0
    pred, gt, mask, wt = ec.berhu_case(B, per, None, "equal")
    r = ec.berhu(pred, gt, mask, wt)
    assert r["c"] == 0 and r["loss"] == 0.0 and (r["grad"] == 0).all()
    pred, gt, mask, wt = ec.berhu_case(B, per, None, "empty_item")
    r = ec.berhu(pred, gt, mask, wt)
    assert np.isnan(r["loss"]) and r["counts"][1] == 0 and np.isfinite(r["grad"][[0, 2]]).all() and np.isnan(r["grad"][1]).all()


# ---------------------------------------------------------------------------------------------------------------- the preprocess cases
def test_planted_rounding_ties():
    """2 x 2: the planted sums are 4k + 2, where half up and half to even part ways for even k; 4 x 4: 16k + 8 with k odd and even; one axis: 2k + 1"""
    half_even = lambda S, area: (lambda q, r: q + (2 * r > area) + ((2 * r == area) & (q % 2 == 1)))(*np.divmod(S, area))
    for fy, fx in ((2, 2), (4, 4), (1, 2), (2, 1)):
        fr, dz, (H, W) = ec.prep_int_case(fy, fx)
        S, _, _ = ec._box_sums(fr, H, W)
        area = fy * fx
        tie = (S[0, :2] % area) == area // 2
        assert tie.all()
        k = S[0, :2] // area
        assert (k % 2 == 0).sum() > 20 and (k % 2 == 1).sum() > 20
        got = ec.prep_rgb_bytes_int(fr, H, W).astype(np.int64)
        if area == 4:
            assert np.array_equal(got, (S + 2) >> 2) and (got != half_even(S, 4)).sum() > 20
        else:
            assert np.array_equal(got, half_even(S, area)) and (got[0, :2] == k + (k % 2)).all()
        Sd, _, _ = ec._box_sums(dz, H, W)
        assert ((Sd[0, :2] % area) == area // 2).all()
    fr, dz, (H, W) = ec.prep_int_case(3, 3)
    assert H * W % 256 and H * W > 256 and fr.shape[1:3] == (3 * H, 3 * W)


def test_fractional_case_meets_the_caps_from_the_reference_alone():
    """(70,140) -> (30,60): 7 / 3 is no float32 number, so the kernel's float32 `d * scale` and OpenCV's double part ways in the last bit.  io_ref's
    tables evaluated in float32, and io_ref's own output, against the float64 evaluation: at most one uint8 step, differing share <= 1e-3, mask
    flips <= 1e-3, depth within 1e-4 where the mask agrees: the caps of test_preprocess_vs_restatement_INTER_AREA_UNPINNED, which the GPU test reuses."""
    fr, dz = ec.fractional_case()
    (Hs, Ws), (H, W) = ec.FRACTIONAL
    assert fr.shape[1:3] == (Hs, Ws) and Hs % H and Ws % W and float(F32(Hs / H)) != Hs / H
    rgb64, d64, m64 = ec.preprocess_tab(fr, dz, H, W, F64)
    rgb32, d32, m32 = ec.preprocess_tab(fr, dz, H, W, F32)
    for what, rgb, d, m in (("float32 tables", rgb32, d32, m32), ("io_ref", io_ref.preprocess_rgb(fr, H, W)) + io_ref.preprocess_depth(dz, H, W)):
        e = np.abs(rgb - rgb64)
        flip = m != m64
        derr = np.abs(d - d64)[~flip].max()
        print(f"{what}: rgb max {e.max():.3e} share {(e > 1e-6).mean():.2e}; mask flips {flip.mean():.2e}; depth max {derr:.3e}")
        assert e.max() <= ec.RGB_STEP_CAP and (e > 1e-6).mean() <= ec.SHARE_CAP
        assert flip.mean() <= ec.FLIP_CAP and derr <= ec.DEPTH_CAP


# ---------------------------------------------------------------------------------------------------------------- the point cloud case
def test_pointcloud_case():
    depth, rgb = ec.pointcloud_case()
    B, _, H, W = depth.shape
    assert (B, H, W) == (3, 5, 7) and depth.min() == 0 and depth.max() == 8 and B * H * W % 256
    pts, col = io_ref.pointcloud(depth, rgb)
    assert np.abs(ec.pointcloud64(depth) - pts).max() <= 2e-6
    flat = rgb.ravel()
    assert np.array_equal(flat[:256], np.arange(256, dtype=F32) / F32(255)) and flat[256] == F32(-0.1) and flat[257] == F32(1.2)
    lev = (flat[:256] * 255).astype(np.uint8).astype(int)
    assert np.abs(lev - np.arange(256)).max() <= 1                           # numpy truncates: a level whose product falls below k gives k - 1
    print("levels that numpy's float32 product truncates to k - 1:", np.flatnonzero(lev != np.arange(256)).tolist())
