"""Eval metrics, BerHu, input preprocessing and the point cloud against float64: the restatements and the seeded case tables that
tests/test_eval_cases_cpu.py (the yardstick itself, and the conditions the cases rest on), tests/test_eval_float64_gpu.py, tests/test_io_float64_gpu.py
and the BerHu tests of tests/test_losses_gpu.py share.  Written from the header comments of csrc/omni_eval.hip, omni_losses.hip, omni_io.hip and
omni_area.h.  Test infrastructure, CPU only (numpy; torch nowhere): the CPU test pins it against the reference's own goldens (G9, G12, G13) first.

Every restatement takes the float32 arrays the kernel gets.  What a kernel decides in float32 (an inlier, the BerHu branch, the depth mask) is
decided here on the same float32 values; what it sums is summed here in float64.  The sizes are chosen for the launch arithmetic of the kernels
(256 threads per block; 2048 blocks at most for the median, the metrics and the BerHu maximum; 256 blocks per item for the BerHu sum), not for
the workload."""
import functools

import numpy as np

from oracle import io_ref

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24                       # half an fp32 ulp of 1
NAN32 = np.float32("nan")
THRESHOLDS = (1.25, 1.5625, 1.953125)  # 1.25 ** k, all exact in float32


def f32_bits(bits):
    return np.asarray(bits, np.uint32).view(F32)


# ================================================================================================================ masked median
def lower_median(x, mask):
    """x[mask > 0].median() as torch.median defines it: the element of rank (n - 1) // 2 of the sorted selection, NaN for an empty selection and
    for one that holds a NaN.  The result equals any other correct one under `==` (-0.0 == +0.0: the order of the two zeros is not defined)."""
    x = np.asarray(x, F32).ravel()
    sel = x[np.asarray(mask, F32).ravel() > 0]
    if sel.size == 0 or np.isnan(sel).any():
        return NAN32
    return np.sort(sel)[(sel.size - 1) // 2]


def same_median(a, b):
    """both NaN, or equal (for everything but the two zeros that is bit equality)"""
    a, b = F32(a), F32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def radix_key(x):
    """the order-preserving key of the float bits that the radix select of csrc/omni_eval.hip sorts by"""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _key_to_f32(k):
    k = np.asarray(k, np.uint64).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def radix_rank_position(x, mask, p):
    """Where the rank element sits in pass p (0: the top byte) of an 8-bit radix select over the selection's keys:
    -> (index in its bucket, bucket size, keys of the same prefix below the bucket, keys of the same prefix above it)."""
    x = np.asarray(x, F32).ravel()
    ks = np.sort(radix_key(x[np.asarray(mask, F32).ravel() > 0])).astype(np.uint64)
    r = (ks.size - 1) // 2
    shift = 24 - 8 * p
    top = int(ks[r]) >> shift
    lo, hi = np.searchsorted(ks, np.uint64(top << shift)), np.searchsorted(ks, np.uint64((top + 1) << shift))
    ptop = top >> 8
    plo, phi = np.searchsorted(ks, np.uint64(ptop << (shift + 8))), np.searchsorted(ks, np.uint64((ptop + 1) << (shift + 8)))
    return int(r - lo), int(hi - lo), int(lo - plo), int(phi - hi)


MEDIAN_SIZES = (1, 2, 255, 256, 257, 2048 * 256 + 257, 3 * 2048 * 256 - 1)
MEDIAN_BUCKET = tuple(f"pass{p}_{w}" for p in range(4) for w in ("last", "first"))
MEDIAN_TIES = ("equal_pos", "equal_neg", "u16_codes", "low_byte", "top_byte", "denormal_middle", "zeros", "inf_finite_median", "inf_median",
               "neg_inf_median") + MEDIAN_BUCKET
MEDIAN_MASKS = ("mask_values", "nan_masked_out", "nan_pos_selected", "nan_neg_selected", "empty")
MEDIAN_CASES = tuple(f"n{n}" for n in MEDIAN_SIZES) + MEDIAN_TIES + MEDIAN_MASKS


def _bucket_case(p, which, rng):
    """the rank element is the last of its bucket in pass p (1001 keys in bucket a, 1000 in a + 1) or the first of the next (1000 and 1001);
    500 keys of another prefix on either side leave it there"""
    shift = 24 - 8 * p
    base = (0xBF801200 & (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF) if p else 0
    a = 0x40 if p else 0xBF
    na, nb = (1001, 1000) if which == "last" else (1000, 1001)
    low = lambda n: rng.integers(0, 1 << shift, n, dtype=np.uint64) if shift else np.zeros(n, np.uint64)
    keys = [np.uint64(base | (a << shift)) | low(na), np.uint64(base | ((a + 1) << shift)) | low(nb)]
    if p:
        keys += [np.uint64(0xBE000000) | rng.integers(0, 1 << 24, 500, dtype=np.uint64), np.uint64(0xC0000000) | rng.integers(0, 1 << 24, 500, dtype=np.uint64)]
    x = _key_to_f32(np.concatenate(keys))
    junk = (rng.standard_normal(300) * 5).astype(F32)
    x, mask = np.concatenate([x, junk]), np.concatenate([np.ones(x.size, F32), np.zeros(300, F32)])
    perm = rng.permutation(x.size)
    return x[perm], mask[perm]


@functools.lru_cache(maxsize=None)
def median_case(name):
    """-> (x, mask), float32, read-only"""
    rng = np.random.default_rng([77, MEDIAN_CASES.index(name)])
    ones = lambda x: np.ones(x.size, F32)
    if name[0] == "n" and name[1:].isdigit():
        n = int(name[1:])
        x = (rng.standard_normal(n) * 5).astype(F32)
        mask = (rng.random(n) < 0.7).astype(F32)
        mask[0] = 1.0
    elif name in ("equal_pos", "equal_neg"):
        x = np.full(3001 if name == "equal_pos" else 3000, 2.5 if name == "equal_pos" else -2.5, F32)
        mask = (rng.random(x.size) < 0.7).astype(F32)
    elif name == "u16_codes":
        codes = rng.choice(np.arange(1, 65536), 37, replace=False)
        x = (codes[rng.integers(0, 37, 70001)].astype(F32) / F32(65535) * F32(128)).astype(F32)
        mask = (rng.random(x.size) < 0.8).astype(F32)
    elif name == "low_byte":
        x = f32_bits(np.uint32(0x40490F00) | rng.integers(0, 256, 4001).astype(np.uint32)); mask = ones(x)
    elif name == "top_byte":
        x = f32_bits((rng.integers(0, 256, 4000).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)); mask = ones(x)
    elif name == "denormal_middle":
        x = np.concatenate([-1 - rng.random(999), 1 + rng.random(999)]).astype(F32)
        x = np.concatenate([x, f32_bits([0x80000001, 0x00000001])]); mask = ones(x)
        x = x[rng.permutation(x.size)]
    elif name == "zeros":
        x = np.concatenate([np.full(1500, -0.0, F32), np.zeros(1501, F32)])[rng.permutation(3001)]; mask = ones(x)
    elif name in ("inf_finite_median", "inf_median", "neg_inf_median"):
        npos, nneg, nfin = {"inf_finite_median": (5, 7, 2001), "inf_median": (1200, 300, 500), "neg_inf_median": (0, 1200, 800)}[name]
        x = np.concatenate([np.full(npos, np.inf), np.full(nneg, -np.inf), rng.standard_normal(nfin) * 5]).astype(F32)
        x = x[rng.permutation(x.size)]; mask = ones(x)
    elif name in MEDIAN_BUCKET:
        x, mask = _bucket_case(int(name[4]), name[6:], rng)
    elif name == "mask_values":
        x = (rng.standard_normal(4099) * 5).astype(F32)
        mask = np.array([0.25, 2.0, -1.0, -0.0, np.nan, 0.0, 1.0], F32)[rng.integers(0, 7, x.size)]
    elif name in ("nan_masked_out", "nan_pos_selected", "nan_neg_selected"):
        x = (rng.standard_normal(4099) * 5).astype(F32)
        mask = (rng.random(x.size) < 0.7).astype(F32)
        if name == "nan_masked_out":
            x[mask == 0] = f32_bits([0x7FC00000, 0xFFC00000])[rng.integers(0, 2, int((mask == 0).sum()))]
        else:
            x[np.flatnonzero(mask > 0)[1234]] = f32_bits(0x7FC00000 if name == "nan_pos_selected" else 0xFFC00000)
    elif name == "empty":
        x = (rng.standard_normal(4096) * 5).astype(F32); mask = np.zeros(4096, F32)
    else:
        raise KeyError(name)
    x, mask = np.ascontiguousarray(x, F32), np.ascontiguousarray(mask, F32)
    x.setflags(write=False); mask.setflags(write=False)
    return x, mask


# ================================================================================================================ depth metrics
def metrics(pred, gt, mask, scale=None):
    """The seven depth metrics over mask > 0 at the float32 values pred * float32(scale) (scale None: pred itself).
    -> dict: scaled (float32, every element), vals (float64[7]: abs_rel, sq_rel, rms_sq_lin, rms_sq_log, d1, d2, d3), counts (the three inlier
    counts, decided in float32), counts64 (the same decided in float64), N, N_log, log_bound (the bound on the float32 rms_sq_log, below)."""
    pred, gt = np.asarray(pred, F32).ravel(), np.asarray(gt, F32).ravel()
    m = np.asarray(mask, F32).ravel() > 0
    scaled = pred if scale is None else pred * F32(scale)                     # one correctly rounded float32 multiply
    assert scaled.dtype == F32
    p32, g32 = scaled[m], gt[m]
    p, g = p32.astype(F64), g32.astype(F64)
    N = int(m.sum())
    with np.errstate(all="ignore"):
        r32 = np.maximum(p32 / g32, g32 / p32)
        r64 = np.maximum(p / g, g / p)
        counts = [int((r32 < F32(t)).sum()) for t in THRESHOLDS]
        counts64 = [int((r64 < t).sum()) for t in THRESHOLDS]
        ml = (p32 > F32(1e-7)) & (g32 > F32(1e-7))
        NL = int(ml.sum())
        lp, lg = np.log(p[ml]), np.log(g[ml])
        l = lp - lg
        # logf within one ulp (2^-23 relative) of each logarithm, the subtraction's rounding 2^-24 |l|: together below delta; the product's
        # rounding and the final cast fit into the quarter of delta that is left
        delta = 2.0 ** -22 * (np.abs(lp) + np.abs(lg))
        nan = float("nan")
        vals = [np.sum(np.abs(p - g) / g) / N, np.sum((p - g) ** 2 / g) / N, np.sum((p - g) ** 2) / N] if N else [nan] * 3
        vals.append(np.sum(l * l) / NL if NL else nan)
        vals += [c / N for c in counts] if N else [nan] * 3
        log_bound = float(np.sum(2 * np.abs(l) * delta + delta * delta) / NL) if NL else nan
    return dict(scaled=scaled, vals=np.array(vals, F64), counts=counts, counts64=counts64, N=N, N_log=NL, log_bound=log_bound, ratio64=r64)


METRIC_SIZES = (1, 257, 16384 + 37, 2048 * 256 + 257)
METRIC_SEEDS = {1: 0, 257: 0, 16384 + 37: 0, 2048 * 256 + 257: 9}            # reseeded until no ratio lies within 2^-20 of a threshold
NEAR = 2.0 ** -20


def _depth_like(seed, n):
    """the data of G9: gt in [0.1, 8), the prediction off by a factor in 1.7 * [0.7, 1.4), a few zero predictions, a mask that keeps 0.8"""
    rng = np.random.default_rng([9, n, seed])
    gt = rng.uniform(0.1, 8.0, n).astype(F32)
    pred = (gt * rng.uniform(0.7, 1.4, n) * 1.7).astype(F32)
    if n > 64:
        pred[rng.integers(0, n, 5)] = 0.0
    mask = (rng.random(n) < 0.8).astype(F32)
    mask[0] = 1.0
    return pred, gt, mask


def near_threshold(ratio64):
    """how many float64 ratios lie within 2^-20 relative of a threshold"""
    r = ratio64[np.isfinite(ratio64)]
    return int(sum((np.abs(r - t) <= NEAR * t).sum() for t in THRESHOLDS))


@functools.lru_cache(maxsize=None)
def metrics_case(n, seed=None):
    """-> (pred, gt, mask, scale) with scale = median(gt) / median(pred) over the mask, one float32 division"""
    pred, gt, mask = _depth_like(METRIC_SEEDS[n] if seed is None else seed, n)
    scale = F32(lower_median(gt, mask)) / F32(lower_median(pred, mask))
    for a in (pred, gt, mask): a.setflags(write=False)
    return pred, gt, mask, scale


def _around(v):
    v = F32(v)
    return [np.nextafter(v, F32(0)), v, np.nextafter(v, F32(np.inf))]


@functools.lru_cache(maxsize=None)
def metrics_planted():
    """(pred, gt, mask), no scaling: ratios exactly on the three thresholds with their float32 neighbours on either side, one pair whose float32
    quotient is the threshold while the float64 one is below it, and predictions that the log mask drops."""
    g, p = [], []
    for gg, pp in ((4, 5), (1, 1.5625), (1, 1.953125), (1, 1)):                               # p / g on a threshold (and on 1): neighbours of p
        for v in _around(pp): g.append(gg); p.append(v)
    for gg, pp in ((5, 4), (1.953125, 1)):                                      # g / p on a threshold: neighbours of p
        for v in _around(pp): g.append(gg); p.append(v)
    for gg in (3, 7, 11, 13):                                                   # divisors that are no power of two
        for t in THRESHOLDS: g.append(gg); p.append(F32(gg) * F32(t))
    g.append(np.nextafter(F32(4), F32(np.inf))); p.append(np.nextafter(F32(5), F32(np.inf)))       # 1.25 (1 - 2.4e-8): float32 says 1.25
    for pp in (0.0, -1.0, F32(1e-7), np.nextafter(F32(1e-7), F32(1)), f32_bits(0x00000003), f32_bits(0x00400000)):
        g.append(1.0); p.append(pp)
    g, p = np.array(g, F32), np.array(p, F32)
    mask = np.ones(g.size, F32)
    g, p, mask = np.concatenate([g, [2.0, 2.0]]).astype(F32), np.concatenate([p, [2.5, 0.0]]).astype(F32), np.concatenate([mask, [0.0, -1.0]]).astype(F32)
    for a in (p, g, mask): a.setflags(write=False)
    return p, g, mask


@functools.lru_cache(maxsize=None)
def metrics_other(name):
    """-> (pred, gt, mask): 'empty' mask; 'no_log' (every selected prediction <= 1e-7: N > 0, N_log = 0); 'mask_values' (0.5 and 2.0 count once)"""
    pred, gt, mask = (a.copy() for a in _depth_like(1, 1000))
    rng = np.random.default_rng(31)
    if name == "empty":
        mask[:] = 0
    elif name == "no_log":
        pred[mask > 0] = np.array([0.0, 1e-7, -2.0, 1e-30], F32)[rng.integers(0, 4, int((mask > 0).sum()))]
    elif name == "mask_values":
        mask = np.array([0.5, 2.0, 0.0, -0.5], F32)[rng.integers(0, 4, mask.size)]
    else:
        raise KeyError(name)
    for a in (pred, gt, mask): a.setflags(write=False)
    return pred, gt, mask


# ================================================================================================================ BerHu
def berhu(pred, gt, mask, weights, grad_out=1.0):
    """calculate_berhu_loss: d = float32(gt - pred), c = float32(max |d|) / float32(5) in float32 (csrc/omni_losses.hip), the branch |d| <= c
    decided on those float32 values; values, sums and the gradient w.r.t. pred in float64.  Where c = 0 (pred == gt everywhere) every element
    takes the |d| branch: loss 0, gradient 0 (the reference evaluates (d^2 + c^2) / (2 c) there and returns NaN).
    -> dict: loss (float64), grad (float64, pred's shape), c (float32), counts (float64[B]: the mask sums), d (float32)"""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    B = pred.shape[0]
    d = gt - pred
    ad = np.abs(d)
    c = F32(ad.max()) / F32(5)
    assert d.dtype == F32 and c.dtype == F32
    leq = ad <= c
    d64, c64 = d.astype(F64), F64(c)
    m, w = np.asarray(mask, F32).astype(F64).reshape(B, -1), np.asarray(weights, F32).astype(F64).reshape(B, -1)
    with np.errstate(all="ignore"):
        val = np.where(leq, np.abs(d64), (d64 * d64 + c64 * c64) / (2 * c64)).reshape(B, -1)
        counts = m.sum(1)
        loss = np.mean((val * m * w).sum(1) / counts)
        dl = np.where(leq, np.sign(d64), d64 / c64).reshape(B, -1)
        grad = -(F64(grad_out) / B) * (m * w / counts[:, None]) * dl
    return dict(loss=float(loss), grad=grad.reshape(pred.shape), c=c, counts=counts, d=d)


BERHU_SIZES = ((1, 1), (3, 255), (3, 257), (2, 77100), (2, 270000))
BERHU_LARGE = ((2, 77100), (2, 270000))
BERHU_PLACEMENTS = ("last", "beyond_cap", "masked_out", "item1")
PLANTED_MAX = 40.0                                                               # the planted maximum of |gt - pred|: c = 8 exactly


@functools.lru_cache(maxsize=None)
def berhu_case(B, per, placement=None, other=None):
    """-> (pred, gt, mask, weights) [B, 1, 1, per] float32: gt in [0, 8), pred = gt + N(0, 1), masks in {0, 0.5, 1}, weights in [0.5, 2].
    placement: |gt - pred| = 40 planted in the last element / an element beyond index 524 288 / a masked-out element / item 1.
    other: 'planted' (max 5 -> c = 1; |d| = 1 and nextafter(1, 2) with both signs; d = 0), 'equal' (pred == gt), 'empty_item' (item 1 unmasked)."""
    rng = np.random.default_rng([12, B, per])
    gt = rng.uniform(0, 8, (B, per)).astype(F32)
    pred = (gt + rng.standard_normal((B, per))).astype(F32)
    mask = np.array([0.0, 0.5, 1.0], F32)[rng.integers(0, 3, (B, per))]
    wt = rng.uniform(0.5, 2, (B, per)).astype(F32)
    if per > 1:
        mask[:, 0] = 1.0
    else:
        mask[:] = 1.0
    if placement is not None:
        n = B * per
        j = {"last": n - 1, "beyond_cap": 2048 * 256 + 4321, "masked_out": int(np.flatnonzero(mask.ravel() == 0)[len(mask.ravel()) // 7]),
             "item1": per + per // 3}[placement]
        assert j < n, (placement, B, per)
        pred.ravel()[j] = 1.0; gt.ravel()[j] = 1.0 + PLANTED_MAX
        if placement != "masked_out":
            mask.ravel()[j] = 1.0
    if other == "planted":
        assert per >= 16
        dv = np.array([5.0, 1.0, -1.0, np.nextafter(F32(1), F32(2)), -np.nextafter(F32(1), F32(2)), 0.0, np.nextafter(F32(1), F32(0))], F32)
        np.clip(pred, gt - 4.5, gt + 4.5, out=pred)
        for b in range(B):
            pred[b, 3:3 + dv.size] = 0.0; gt[b, 3:3 + dv.size] = dv; mask[b, 3:3 + dv.size] = 1.0      # gt - 0: d is dv to the bit
    elif other == "equal":
        pred = gt.copy()
    elif other == "empty_item":
        mask[1] = 0.0
    elif other is not None:
        raise KeyError(other)
    out = tuple(np.ascontiguousarray(a.reshape(B, 1, 1, per)) for a in (pred, gt, mask, wt))
    for a in out: a.setflags(write=False)
    return out


# ================================================================================================================ preprocessing
def _box_sums(frames, H, W):
    f = np.asarray(frames)
    B, Hs, Ws = f.shape[:3]
    assert Hs % H == 0 and Ws % W == 0, "integer scales only"
    fy, fx = Hs // H, Ws // W
    return f.reshape((B, H, fy, W, fx) + f.shape[3:]).astype(np.int64).sum((2, 4)), fy, fx


def prep_rgb_bytes_int(frames_u8, H, W):
    """[B,Hs,Ws,3] uint8 -> the bytes of cv2.INTER_AREA at an integer scale [B,H,W,3], in exact integer arithmetic: the box sum S over fy x fx
    source pixels; 2 x 2: floor(S / 4 + 1 / 2) (OpenCV's fast path rounds half up); every other scale: S / area rounded half to even."""
    S, fy, fx = _box_sums(frames_u8, H, W)
    area = fy * fx
    if fy == 2 and fx == 2:
        return ((S + 2) >> 2).astype(np.uint8)
    q, r = np.divmod(S, area)
    return (q + (2 * r > area) + ((2 * r == area) & (q % 2 == 1))).astype(np.uint8)


def prep_rgb_int(frames_u8, H, W):
    """-> [B,3,H,W] float32: float32(byte) / float32(255)"""
    return (prep_rgb_bytes_int(frames_u8, H, W).astype(F32) / F32(255)).transpose(0, 3, 1, 2)


def prep_depth_int(frames_u16, H, W, min_depth=0.1, max_depth=8.0):
    """[B,Hs,Ws] uint16 -> (depth [B,1,H,W] float32, mask uint8): the float32 sequence of prep_depth_kernel at an integer scale written out.  The
    box sum is an integer below 2^24 (exact in float32, in any order); then acc * (inv_x * inv_y) with inv = 1 / scale (equal size: no product),
    / 65535, * 128, each one float32 operation; mask = v <= 8 and v > 0.1 (float32 thresholds); depth = 0 where the mask is."""
    S, fy, fx = _box_sums(frames_u16, H, W)
    assert int(S.max()) < 1 << 24
    v = S.astype(F32)
    if fy * fx > 1:
        v = v * ((F32(1) / F32(fx)) * (F32(1) / F32(fy)))
    v = v / F32(65535) * F32(128)
    assert v.dtype == F32
    m = (v <= F32(max_depth)) & (v > F32(min_depth))
    return np.where(m, v, F32(0))[:, None], m.astype(np.uint8)[:, None]


def inter_area_tab(img, H, W, dtype):
    """oracle/io_ref.py's INTER_AREA tables evaluated in `dtype` (weights and sums), no rounding back: [Hs,Ws(,C)] -> [H,W(,C)] of dtype"""
    x = np.asarray(img).astype(dtype)
    if x.ndim == 2:
        x = x[..., None]
    Hs, Ws, C = x.shape
    tmp = np.zeros((Hs, W, C), dtype)
    for d, e in enumerate(io_ref._area_tab(W, Ws)):
        for s, w in e:
            tmp[:, d] += x[:, s] * dtype(w)
    out = np.zeros((H, W, C), dtype)
    for d, e in enumerate(io_ref._area_tab(H, Hs)):
        for s, w in e:
            out[d] += tmp[s] * dtype(w)
    return out[..., 0] if np.asarray(img).ndim == 2 else out


FRACTIONAL = ((70, 140), (30, 60))                                               # scale 7 / 3 in both axes
RGB_STEP_CAP, SHARE_CAP, FLIP_CAP, DEPTH_CAP = 1.0 / 255 + 1e-6, 1e-3, 1e-3, 1e-4  # the caps of test_preprocess_vs_restatement_INTER_AREA_UNPINNED


@functools.lru_cache(maxsize=None)
def fractional_case():
    rng = np.random.default_rng(70)
    src = FRACTIONAL[0]
    fr = rng.integers(0, 256, (2,) + src + (3,), dtype=np.uint8)
    dz = rng.integers(0, 6000, (2,) + src, dtype=np.uint16)
    fr.setflags(write=False); dz.setflags(write=False)
    return fr, dz


def preprocess_tab(fr, dz, H, W, dtype):
    """preprocess_rgb / preprocess_depth of oracle/io_ref.py with the tables evaluated in `dtype`: -> (rgb [B,3,H,W], depth [B,1,H,W], mask)"""
    rgb = np.stack([np.clip(np.rint(inter_area_tab(f, H, W, dtype)), 0, 255).astype(F32).transpose(2, 0, 1) / F32(255) for f in fr])
    d = np.stack([(inter_area_tab(f, H, W, dtype).astype(F32) / F32(65535) * F32(128))[None] for f in dz])
    m = (d <= F32(8.0)) & (d > F32(0.1))
    return rgb, d * m, m.astype(np.uint8)


PREP_INT_SCALES = ((2, 2), (4, 4), (3, 3), (1, 2), (2, 1))                       # (fy, fx)


@functools.lru_cache(maxsize=None)
def prep_int_case(fy, fx):
    """-> (frames uint8 [2,Hs,Ws,3], depth uint16 [2,Hs,Ws], (H, W)).  H x W = 9 x 31 (279 pixels per item: two blocks, ragged).  2 x 2: the first
    rows hold box sums 4k + 2 (the half that OpenCV's fast path rounds up, k odd and even); 4 x 4: sums 16k + 8; 1 x 2 and 2 x 1: sums 2k + 1."""
    H, W = 9, 31
    rng = np.random.default_rng([55, fy, fx])
    Hs, Ws = H * fy, W * fx
    fr = rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)
    dz = rng.integers(0, 6000, (2, Hs, Ws), dtype=np.uint16)
    area = fy * fx
    if area % 2 == 0:
        for i in range(2 * W):                                                   # two destination rows of planted ties
            y, x = (i // W) * fy, (i % W) * fx
            for a, top in ((fr, 255), (dz, 6000)):
                k = int(rng.integers(0, top - 1))
                blk = np.full((fy, fx), k, np.int64)
                blk.ravel()[: area // 2] += 1                                    # S = area * k + area / 2
                if a is fr:
                    a[0, y:y + fy, x:x + fx, :] = blk[..., None]
                else:
                    a[0, y:y + fy, x:x + fx] = blk
    fr.setflags(write=False); dz.setflags(write=False)
    return fr, dz, (H, W)


@functools.lru_cache(maxsize=None)
def prep_same_case(name):
    """equal-size frames uint8 [B,H,W,3]: 'quad' (6,10), 'byte' (5,7), 'b2' (B = 2, 6 x 10), 'levels' (16 x 16: every byte level in every channel)"""
    rng = np.random.default_rng([56, ("quad", "byte", "b2", "levels").index(name)])
    if name == "levels":
        fr = np.stack([rng.permutation(256) for _ in range(3)], -1).astype(np.uint8).reshape(1, 16, 16, 3)
    else:
        B, H, W = {"quad": (1, 6, 10), "byte": (1, 5, 7), "b2": (2, 6, 10)}[name]
        fr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    fr.setflags(write=False)
    return fr


DEPTH_CODES = np.array([[[0, 51, 52, 4095, 4096, 65535, 1000]]], np.uint16)       # (0.1, 8]: 51 and 4096 are out, 52 and 4095 are in


# ================================================================================================================ point cloud
@functools.lru_cache(maxsize=None)
def pointcloud_case():
    """depth [3,1,5,7] in [0, 8] (0 and 8 included); rgb [3,3,5,7] holding every k / 255 once, then -0.1 and 1.2, then random values in [0, 1)"""
    rng = np.random.default_rng(13)
    depth = rng.uniform(0, 8, (3, 1, 5, 7)).astype(F32)
    depth.ravel()[[0, 104]] = (0.0, 8.0)
    rgb = rng.random(3 * 3 * 5 * 7).astype(F32)
    rgb[:256] = np.arange(256, dtype=F32) / F32(255)
    rgb[256:258] = (-0.1, 1.2)
    rgb = rgb.reshape(3, 3, 5, 7)
    depth.setflags(write=False); rgb.setflags(write=False)
    return depth, rgb


def pointcloud64(depth):
    """the rays at the float32-rounded u, v (coords2uv stores them to float32) evaluated in float64, times the float32 depth: [B,H*W,3] float64"""
    B, _, h, w = depth.shape
    xs, ys = np.meshgrid(np.arange(w) + 1, np.arange(h) + 1)
    u = ((xs - (w / 2 + 0.5)) / w * 2 * np.pi).astype(F32).astype(F64).ravel()
    v = (-(ys - (h / 2 + 0.5)) / h * np.pi).astype(F32).astype(F64).ravel()
    xyz = np.stack([np.cos(v) * np.sin(u), np.cos(v) * np.cos(u), np.sin(v)], -1)
    return xyz[None] * np.asarray(depth, F32).astype(F64).reshape(B, h * w, 1)
