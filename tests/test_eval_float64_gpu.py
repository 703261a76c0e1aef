"""GPU: the masked median and the depth metrics (csrc/omni_eval.hip through omnifusion_amd/eval.py) against the restatements of
tests/_eval_cases.py (pinned on the CPU by tests/test_eval_cases_cpu.py), at the sizes where the launch arithmetic changes and on the ties,
bucket edges, NaNs and thresholds that decide real medians and inlier counts.

  median    equal to the restatement (both NaN where it is NaN), whatever the 260-word workspace held before, and again on a second call
  metrics   the scaled prediction bit-equal over the whole array; N, N_log and the three inlier counts exact, decided in float32 as the reference
            decides them; abs_rel, sq_rel, rms_sq_lin within 3, 4, 3 * 2^-24 relative of float64 (every term is non-negative and carries that many
            float32 roundings, the sums are in double, one final cast); rms_sq_log within the case's own bound (`_eval_cases.metrics`: logf at one
            ulp, the subtraction's rounding)

Nothing in a gate comes from a kernel."""
import ctypes

import numpy as np
import pytest
import torch

import _eval_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
REL = (3 * ec.U24, 4 * ec.U24, 3 * ec.U24)
NAMES = ("abs_rel", "sq_rel", "rms_sq_lin", "rms_sq_log", "d1", "d2", "d3")


def _L():
    from omnifusion_amd import _lib
    return _lib


def t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # a copy: the cases are read-only


def ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def _median_raw(x, mask, fill):
    """omni_masked_median_f32 on a workspace of 260 words pre-filled with the byte `fill`"""
    L = _L()
    ws = torch.full((260 * 4,), fill, dtype=torch.uint8, device=DEV)
    out = torch.full((1,), 123.0, dtype=torch.float32, device=DEV)
    L.check(L.load().omni_masked_median_f32(ptr(x), ptr(mask), x.numel(), ptr(ws), ptr(out), L.stream_of(x)), "masked_median")
    return out.cpu().numpy()[0]


# ---------------------------------------------------------------------------------------------------------------- median
@pytest.mark.parametrize("name", ec.MEDIAN_CASES)
def test_median_equals_the_restatement(name):
    from omnifusion_amd.eval import masked_median
    x, mask = ec.median_case(name)
    want = ec.lower_median(x, mask)
    xd, md = t(x), t(mask)
    got = [masked_median(xd, md).cpu().numpy()[0], _median_raw(xd, md, 0xFF), _median_raw(xd, md, 0xFF), masked_median(xd, md).cpu().numpy()[0]]
    print(f"{name}: n {x.size} selected {int((mask > 0).sum())} median {want!r} kernel {got[0]!r}")
    for g in got:
        assert ec.same_median(g, want), (name, g, want)
        assert g.view(np.uint32) == got[0].view(np.uint32) or np.isnan(g)           # the same bits on every call


# ---------------------------------------------------------------------------------------------------------------- metrics
def _metrics_raw(pred, gt, mask, num=None, den=None, fill=float("nan")):
    """omni_depth_metrics_f32 on a fresh copy of the prediction and a workspace pre-filled with `fill` -> (out[9] float32, scaled prediction)"""
    L = _L()
    p, g, m = t(pred).clone(), t(gt), t(mask)
    ws = torch.full((2048 * 9,), fill, dtype=torch.float64, device=DEV)
    out = torch.full((9,), -7.0, dtype=torch.float32, device=DEV)
    nd = [None if v is None else t(np.array([v], F32)) for v in (num, den)]
    L.check(L.load().omni_depth_metrics_f32(ptr(p), ptr(g), ptr(m), ptr(nd[0]), ptr(nd[1]), p.numel(), ptr(ws), ptr(out), L.stream_of(p)),
            "depth_metrics")
    return out.cpu().numpy(), p.cpu().numpy()


def _hold(what, out, scaled, r):
    """the gates of the module docstring; prints the measured error beside its bound for every quantity"""
    assert np.array_equal(scaled.view(np.uint32), r["scaled"].view(np.uint32)), f"{what}: scaled prediction"
    N, NL = r["N"], r["N_log"]
    assert out[7] == N and out[8] == NL, (what, out[7:], N, NL)
    if N == 0:
        assert np.isnan(out[:7]).all(), (what, out)
        return
    for k in range(3):
        ref = r["vals"][k]
        err = abs(float(out[k]) - ref) / ref if ref else abs(float(out[k]))
        print(f"{what}: {NAMES[k]} {out[k]:.9g} float64 {ref:.12g} relative error {err:.2e} bound {REL[k]:.2e}")
        assert err <= REL[k], (what, NAMES[k], err)
    if NL == 0:
        assert np.isnan(out[3]), (what, out[3])
    else:
        err = abs(float(out[3]) - r["vals"][3])
        print(f"{what}: rms_sq_log {out[3]:.9g} float64 {r['vals'][3]:.12g} error {err:.2e} bound {r['log_bound']:.2e}")
        assert err <= r["log_bound"], (what, err, r["log_bound"])
    for k in range(3):
        cnt = r["counts"][k]
        print(f"{what}: {NAMES[4 + k]} {out[4 + k]:.9g} count {round(float(out[4 + k]) * N)} float32 restatement {cnt} (a float64 compare: {r['counts64'][k]}) of {N}")
        assert round(float(out[4 + k]) * N) == cnt and out[4 + k] == F32(cnt / N), (what, NAMES[4 + k], out[4 + k], cnt, N)


@pytest.mark.parametrize("n", ec.METRIC_SIZES)
def test_metrics_at_the_launch_edges(n):
    """n = 1, 257 (a second block of one thread), 16 384 + 37 (ragged last block), 2048 * 256 + 257 (the block cap binds, 257 threads wrap): scaled by
    median(gt) / median(pred) handed over as device scalars.  A workspace full of NaN or of 1e300 and a repeat on a fresh copy: the same bits."""
    pred, gt, mask, scale = ec.metrics_case(n)
    num, den = ec.lower_median(gt, mask), ec.lower_median(pred, mask)
    r = ec.metrics(pred, gt, mask, scale)
    out, scaled = _metrics_raw(pred, gt, mask, num, den)
    _hold(f"n {n}", out, scaled, r)
    out2, scaled2 = _metrics_raw(pred, gt, mask, num, den, fill=1e300)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(scaled.view(np.uint32), scaled2.view(np.uint32))


def test_metrics_planted_block_decides_in_float32():
    """ratios exactly on 1.25, 1.5625 and 1.953125 (not inliers: `<`), their float32 neighbours, a pair whose float32 quotient is 1.25 while the
    float64 one is below it (an inlier for a float64 compare only), divisors that are no power of two, and predictions of 0, -1, 1e-7 and denormals,
    which the log mask drops (N_log = N - 5).  Both scale pointers NULL: the prediction comes back untouched."""
    pred, gt, mask = ec.metrics_planted()
    r = ec.metrics(pred, gt, mask)
    assert r["counts"] != r["counts64"]
    out, scaled = _metrics_raw(pred, gt, mask)
    _hold("planted", out, scaled, r)
    assert np.array_equal(scaled.view(np.uint32), pred.view(np.uint32))


def test_metrics_empty_mask_no_log_and_mask_values():
    """empty mask: seven NaNs, N = N_log = 0; every selected prediction <= 1e-7: N > 0, N_log = 0 and only rms_sq_log is NaN; mask values 0.5 and 2.0
    count as one element each, 0 and -0.5 as none"""
    for name in ("empty", "no_log", "mask_values"):
        pred, gt, mask = ec.metrics_other(name)
        r = ec.metrics(pred, gt, mask)
        out, scaled = _metrics_raw(pred, gt, mask)
        _hold(name, out, scaled, r)
        if name == "empty":
            assert np.isnan(out[:7]).all() and out[7] == 0 and out[8] == 0
        if name == "no_log":
            assert out[7] > 0 and out[8] == 0 and np.isnan(out[3]) and np.isfinite(np.delete(out[:7], 3)).all()


def test_compute_eval_metrics_end_to_end_at_the_block_cap():
    """compute_eval_metrics on the 524 545-element case: both medians, the float32 scale and the metrics in one call, the prediction scaled in place"""
    from omnifusion_amd.eval import compute_eval_metrics
    pred, gt, mask, scale = ec.metrics_case(ec.METRIC_SIZES[-1])
    r = ec.metrics(pred, gt, mask, scale)
    p = t(pred).clone().reshape(1, 1, 1, -1)
    out = compute_eval_metrics(p, t(gt).reshape(p.shape), t(mask).reshape(p.shape)).cpu().numpy()
    _hold("end to end", out, p.cpu().numpy().ravel(), r)


def test_compute_eval_metrics_reports_nan_for_a_prediction_with_nan():
    """a prediction that overflowed somewhere: torch.median of the selection is NaN, the reference scales by it, its four error metrics are NaN and
    its inlier ratios 0 (NaN < t is false); so here.  A NaN at a masked-out element changes nothing but that element."""
    from omnifusion_amd.eval import compute_eval_metrics
    pred, gt, mask, scale = ec.metrics_case(16384 + 37)
    bad = pred.copy()
    bad[np.flatnonzero(mask > 0)[777]] = np.nan
    p = t(bad).clone()
    out = compute_eval_metrics(p, t(gt), t(mask)).cpu().numpy()
    assert np.isnan(out[:4]).all() and (out[4:7] == 0).all() and out[7] == (mask > 0).sum() and out[8] == 0 and torch.isnan(p).all()
    bad = pred.copy()
    j = int(np.flatnonzero(mask == 0)[5])
    bad[j] = np.nan
    p = t(bad).clone()
    out = compute_eval_metrics(p, t(gt), t(mask)).cpu().numpy()
    r = ec.metrics(pred, gt, mask, scale)
    got = p.cpu().numpy()
    assert np.isnan(got[j]) and np.array_equal(np.delete(got, j).view(np.uint32), np.delete(r["scaled"], j).view(np.uint32))
    assert np.array_equal(out[4:], np.array([c / r["N"] for c in r["counts"]] + [r["N"], r["N_log"]], F32))
