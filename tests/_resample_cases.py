"""equi2pers / pers2equi against float64: the case table, a plain torch-CPU restatement of both operators in a chosen dtype, and the comparison
rules that tests/test_resample_restatement_cpu.py (the C oracle standing in for a kernel) and tests/test_resample_float64_gpu.py (the HIP kernels)
share.  Written from DESIGN.md section 4, the header comments of csrc/omni_equi2pers.hip, omni_e2p_common.h and omni_p2e_common.h, and the line
citations of oracle/omni_oracle.c.  Test infrastructure: the CPU test pins it against the reference's own goldens first.

What makes the float64 mode meaningful: the CONSTANTS are the reference's fp32 values, widened -- the patch centres (a float32 tensor made from the
float64 preset arithmetic), the torch.linspace(..., dtype=float32) nodes, FOV / 360 and FOV / 180 as float32, pi and pi / 2 cast to float32 -- and
only the arithmetic after them runs in `dtype`.  The float64 result is then the exact value of the function the reference rounds its way through,
and the float32 mode is one more fp32 evaluation of it, whose distance from float64 (`e32`) sizes every gate."""
import functools
import math

import numpy as np
import torch

from _util import rng_uniform

F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24                       # half an fp32 ulp of 1
NPATCH = {3: 10, 4: 18, 5: 26, 6: 46}
FOV = (80.0, 80.0)

#            nrows  patch      ERP        B*C
E2P_CASES = {
    "n4_p32":   (4, (32, 32), (64, 128), (1, 7)),       # one tile per patch; seam-straddling polar patches; ring stages
    "n3_rect":  (3, (24, 40), (100, 333), (3,)),        # rectangular, ragged tiles; row pitch no multiple of 4: every tile takes the gather path
    "n6_odd":   (6, (33, 33), (128, 256), (2,)),        # odd patch: q4 NaN centre; pole tiles next to box tiles
    "n5_p64":   (5, (64, 64), (256, 512), (3,)),        # several tiles per patch; the fp16 case
}
P2E_CASES = {
    "n4_p16":   (4, (16, 16), (64, 128), (1, 7)),
    "n3_p32":   (3, (32, 32), (64, 128), (2,)),         # uncovered pixels; pole rows
    "n6_p32":   (6, (32, 32), (128, 256), (1,)),        # the one-plane walk form
    "n5_ragged": (5, (32, 32), (100, 333), (3,)),       # ragged ERP width
    "n3_rect":  (3, (24, 40), (100, 333), (2,)),        # rectangular: the height / width swap
    "n4_p64":   (4, (64, 64), (256, 512), (3,)),        # the fp16 case
}
E2P_FP16, P2E_FP16 = "n5_p64", "n4_p64"
NEAR_DELTA, NEAR_EPS = 1e-5, 1e-6


def _pair(t):
    return tuple(t) if isinstance(t, (tuple, list)) else (t, t)


def _c(value, dtype):
    """a constant the reference holds in fp32, widened"""
    return torch.tensor(value, dtype=F32).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- patch centres
_PRESET = {4: ((3, 6, 6, 3), (-67.5, -22.5, 22.5, 67.5)),
           6: ((3, 8, 12, 12, 8, 3), (-75.2, -45.93, -15.72, 15.72, 45.93, 75.2)),
           5: ((3, 6, 8, 6, 3), (-72.2, -36.1, 0, 36.1, 72.2))}


def patch_centers(nrows, which=0):
    """-> (lam0 [N], phi1 [N], center_p [N,2]), float32 tensors.  which: 0 the equi2pers table, 1 the pers2equi table (nrows = 3: +-60 against +-59.6).
    The angles of the presets are combined in Python floats, cast to float32, and everything after the cast is float32 arithmetic."""
    if nrows == 3:
        cols, phis = (3, 4, 3), ((-60, 0, 60), (-59.6, 0, 59.6))[which]
    else:
        cols, phis = _PRESET[nrows]
    deg = []
    for n, phi in zip(cols, phis):
        step = 360.0 / n
        deg += [(j * step + step / 2, phi) for j in range(n)]
    c = torch.tensor(deg, dtype=torch.float64).to(F32)
    cx = c[:, 0] / 360.0
    cy = (c[:, 1] + 90.0) / 180.0
    center_p = torch.stack([cx * 2.0 - 1.0, cy * 2.0 - 1.0], -1)
    return center_p[:, 0] * _c(math.pi, F32), center_p[:, 1] * _c(math.pi * 0.5, F32), center_p


# ---------------------------------------------------------------------------------------------------------------- equi2pers
def e2p_coords(nrows, fov, patch, erp_size, dtype=F64):
    """Natural [N, ph, pw] arrays of the inverse gnomonic grid: lon (unwrapped), lat, u (wrapped once each way), v, and the sampling coordinates ix, iy
    of bilinear / border / align_corners=True.  Quirk q4: where x == y == 0 (the centre sample when both patch dimensions are odd) lat is 0/0 = NaN;
    the clip sends the NaN row coordinate to 0, so the sample reads row 0 (iy = 0 here), and v stays NaN."""
    ph, pw = _pair(patch); fov_h, fov_w = _pair(fov); H, W = _pair(erp_size)
    lam, phi, _ = patch_centers(nrows, 0)
    lam = lam.to(dtype)[:, None, None]; phi = phi.to(dtype)[:, None, None]
    PI, PI_2 = _c(math.pi, dtype), _c(math.pi * 0.5, dtype)
    fovx = (torch.tensor(fov_w, dtype=F32) / 360.0).to(dtype)
    fovy = (torch.tensor(fov_h, dtype=F32) / 180.0).to(dtype)
    sx = torch.linspace(0, 1, pw, dtype=F32).to(dtype)[None, None, :]
    sy = torch.linspace(0, 1, ph, dtype=F32).to(dtype)[None, :, None]
    x = ((sx * 2 - 1) * PI) * fovx
    y = ((sy * 2 - 1) * PI_2) * fovy
    rou = torch.sqrt(x * x + y * y)
    c = torch.atan(rou)
    sin_c, cos_c = torch.sin(c), torch.cos(c)
    sp, cp = torch.sin(phi), torch.cos(phi)
    lat = torch.asin(cos_c * sp + (y * sin_c * cp) / rou)
    lon = lam + torch.atan2(x * sin_c, rou * cp * cos_c - y * sp * sin_c)
    v = lat / PI_2
    u = lon / PI
    u = torch.where(u > 1, u - 2, u)
    u = torch.where(u < -1, u + 2, u)
    ix, iy = sampling_coords(u, v, H, W)
    return dict(lon=lon.expand_as(lat), lat=lat, u=u.expand_as(lat), v=v, ix=ix.expand_as(lat), iy=iy)


def sampling_coords(u, v, H, W):
    """grid_sample's un-normalisation for align_corners=True and its border clip, in the dtype of u, v; a NaN coordinate clips to 0."""
    sx = _c(W - 1, u.dtype) / 2
    sy = _c(H - 1, v.dtype) / 2
    ix = ((u + 1) * sx).clamp(0, W - 1)
    iy = ((v + 1) * sy).clamp(0, H - 1)
    return torch.where(torch.isnan(ix), torch.zeros_like(ix), ix), torch.where(torch.isnan(iy), torch.zeros_like(iy), iy)


def sampling_coords_f32(u, v, H, W):
    """The same from a kernel's own float32 (u, v) in numpy float32 arithmetic: one add, one multiply, the clamp.  -> float32 arrays"""
    u = np.asarray(u, np.float32); v = np.asarray(v, np.float32)
    one = np.float32(1.0)
    ix = (u + one) * (np.float32(W - 1) / np.float32(2.0))
    iy = (v + one) * (np.float32(H - 1) / np.float32(2.0))
    with np.errstate(invalid="ignore"):
        ix = np.minimum(np.float32(W - 1), np.maximum(ix, np.float32(0.0)))
        iy = np.minimum(np.float32(H - 1), np.maximum(iy, np.float32(0.0)))
    ix = np.where(np.isnan(ix), np.float32(0.0), ix).astype(np.float32)
    iy = np.where(np.isnan(iy), np.float32(0.0), iy).astype(np.float32)
    return ix, iy


def xyz_of(lon, lat):
    """[N, 3, ph, pw] unit rays from the UNWRAPPED longitude; NaN wherever lat is (q4)"""
    cl = torch.cos(lat)
    return torch.stack([cl * torch.sin(lon), cl * torch.cos(lon), torch.sin(lat)], 1)


def scramble(nat):
    """The reference lays the N grids side by side in a [ph, N*pw] strip and reads that strip back as [ph, pw, N]:
    uv[b, h, a] = strip[h, a*N + b], strip[h, n*pw + w] = nat[n, h, w].  nat [N, ph, pw] -> [N, ph, pw]"""
    N, ph, pw = nat.shape
    return nat.permute(1, 0, 2).reshape(ph, pw, N).permute(2, 0, 1)


def unscramble(scr):
    """inverse of scramble()"""
    N, ph, pw = scr.shape
    return scr.permute(1, 2, 0).reshape(ph, N, pw).permute(1, 0, 2)


def uv_strip(u, v):
    """-> the reference's uv output [N, 2, ph, pw]"""
    return torch.stack([scramble(u), scramble(v)], 1)


def equi2pers(erp, fov=FOV, nrows=4, patch=(16, 16), coords=None, dtype=F64, drop=None):
    """erp [B,C,H,W] -> pers [B,C,ph,pw,N] in `dtype`: bilinear sampling with border clipping.  Taps outside the image are skipped (a clipped coordinate
    is integral there, so their weight is 0 anyway).  coords=(ix, iy): blend at the [N,ph,pw] sampling coordinates given (a kernel's own) instead of the
    restatement's.  drop: [N,ph,pw] bool, samples whose weights are zeroed (only to show what a backward that dropped the q4 NaN sample would give)."""
    erp = (erp if isinstance(erp, torch.Tensor) else torch.as_tensor(np.asarray(erp))).to(dtype)
    B, C, H, W = erp.shape
    if coords is None:
        k = e2p_coords(nrows, fov, patch, (H, W), dtype)
        ix, iy = k["ix"], k["iy"]
    else:
        ix, iy = (torch.as_tensor(np.asarray(t)).to(dtype) for t in coords)
    x0f, y0f = torch.floor(ix), torch.floor(iy)
    tw, tn = ix - x0f, iy - y0f
    te, ts = 1 - tw, 1 - tn
    x0, y0 = x0f.long(), y0f.long()
    inx, iny = (x0 + 1 < W).to(dtype), (y0 + 1 < H).to(dtype)
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    keep = 1.0 if drop is None else (~drop).to(dtype)
    out = (erp[:, :, y0, x0] * (ts * te * keep) + erp[:, :, y0, x1] * (ts * tw * inx * keep)
           + erp[:, :, y1, x0] * (tn * te * iny * keep) + erp[:, :, y1, x1] * (tn * tw * inx * iny * keep))
    return out.permute(0, 1, 3, 4, 2)


def equi2pers_bwd(grad_pers, erp_size, fov=FOV, nrows=4, coords=None, dtype=F64, drop=None):
    """The transpose by autograd of the restatement: grad_pers [B,C,ph,pw,N] -> grad_erp [B,C,H,W]"""
    g = torch.as_tensor(grad_pers).to(dtype)
    B, C, ph, pw, N = g.shape
    H, W = _pair(erp_size)
    erp = torch.zeros((B, C, H, W), dtype=dtype, requires_grad=True)
    out = equi2pers(erp, fov, nrows, (ph, pw), coords=coords, dtype=dtype, drop=drop)
    (out * g).sum().backward()
    return erp.grad


# ---------------------------------------------------------------------------------------------------------------- pers2equi
def p2e_tables(nrows, fov, patch, erp_size, dtype=F64, rows=None, cols=None):
    """The per-(patch, pixel) geometry of pers2equi, [N, H, W] each: cos_c, X, Y (with the reference's swap: X is scaled by the patch HEIGHT and tested
    against the WIDTH, Y the other way round), the validity mask, and the taps clamped to the patch after the floor (a NaN clamps to 0).
    rows / cols: index arrays of the ERP rows / columns wanted (the goldens of the large configurations are strided sub-samples)."""
    ph, pw = _pair(patch); fov_h, fov_w = _pair(fov); H, W = _pair(erp_size)
    lam, phi, _ = patch_centers(nrows, 1)
    lam = lam.to(dtype)[:, None, None]; phi = phi.to(dtype)[:, None, None]
    PI, PI_2 = _c(math.pi, dtype), _c(math.pi * 0.5, dtype)
    fovx = (torch.tensor(fov_w, dtype=F32) / 360.0).to(dtype)
    fovy = (torch.tensor(fov_h, dtype=F32) / 180.0).to(dtype)
    lat = torch.linspace(-math.pi * 0.5, math.pi * 0.5, H, dtype=F32).to(dtype)
    lon = torch.linspace(-math.pi, math.pi, W, dtype=F32).to(dtype)
    if rows is not None: lat = lat[torch.as_tensor(rows)]
    if cols is not None: lon = lon[torch.as_tensor(cols)]
    lat = lat[None, :, None]; lon = lon[None, None, :]
    d = lon - lam
    sp, cp, sl, cl, cd = torch.sin(phi), torch.cos(phi), torch.sin(lat), torch.cos(lat), torch.cos(d)
    cos_c = sp * sl + cp * cl * cd
    nx = (cl * torch.sin(d)) / cos_c
    ny = (cp * sl - sp * cl * cd) / cos_c
    nx = nx / fovx / PI
    ny = ny / fovy / PI_2
    X = (nx + 1) * 0.5 * ph               # (sic) height
    Y = (ny + 1) * 0.5 * pw               # (sic) width
    mask = (X < pw) & (X > 0) & (Y < ph) & (Y > 0) & (cos_c > 0)
    return dict(cos_c=cos_c, X=X, Y=Y, mask=mask, ph=ph, pw=pw, dtype=dtype)


def _clamped_taps(X, Y, ph, pw):
    def cl(t, hi):
        t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
        return t.clamp(0, hi)
    fx, fy = torch.floor(X), torch.floor(Y)
    return cl(fx, pw - 1), cl(fx + 1, pw - 1), cl(fy, ph - 1), cl(fy + 1, ph - 1)


def p2e_weights(tab, flipped=None):
    """-> (x0, x1, y0, y1 [N,H,W] int64, mask [N,H,W] bool, w [N,H,W,4]): the weights of taps (y0,x0), (y1,x0), (y0,x1), (y1,x1) built from the CLAMPED
    taps, multiplied by the mask, zeroed unless > 1e-5, L1-normalised over all N * 4 of a pixel with the floor 1e-12.

    flipped [N,H,W] bool: entries whose mask is inverted -- what another evaluation of the geometry gives when a coordinate that float64 puts within
    round-off of a validity bound lands on the other side of it.  An entry switched ON gets the coordinate such an evaluation has: X or Y, where it
    lies outside its bound, is put ON the bound (X = 0 gives the full weight of column 0, as a coordinate just inside does; inverting the mask alone
    would keep the clamped taps of the outside, whose weights are ~0)."""
    X, Y, mask, ph, pw = tab["X"], tab["Y"], tab["mask"], tab["ph"], tab["pw"]
    if flipped is not None:
        on = flipped & ~mask
        X = torch.where(on, X.clamp(0, pw), X)
        Y = torch.where(on, Y.clamp(0, ph), Y)
        mask = mask ^ flipped
    x0f, x1f, y0f, y1f = _clamped_taps(X, Y, ph, pw)
    m = mask.to(X.dtype)
    w = torch.stack([(x1f - X) * (y1f - Y) * m, (x1f - X) * (Y - y0f) * m, (X - x0f) * (y1f - Y) * m, (X - x0f) * (Y - y0f) * m], -1)
    w = torch.where(w > _c(1e-5, w.dtype), w, w * 0)
    denom = torch.maximum(w.abs().sum((0, 3)), _c(1e-12, w.dtype))
    return x0f.long(), x1f.long(), y0f.long(), y1f.long(), mask, w / denom[None, :, :, None]


def pers2equi(pers, tab, flipped=None):
    """pers [B,C,ph,pw,N] -> erp [B,C,H,W] in the dtype of the tables: the four gathers of every patch times the mask, times the normalised weights,
    summed over the patches."""
    dtype = tab["dtype"]
    pers = pers.to(dtype) if isinstance(pers, torch.Tensor) else torch.as_tensor(np.asarray(pers)).to(dtype)
    B, C, ph, pw, N = pers.shape
    x0, x1, y0, y1, mask, w = p2e_weights(tab, flipped)
    img = pers.permute(0, 1, 4, 2, 3).reshape(B, C, N * ph * pw)
    base = (torch.arange(N) * (ph * pw))[:, None, None]
    m = mask.to(dtype)
    out = 0
    for k, (yy, xx) in enumerate(((y0, x0), (y1, x0), (y0, x1), (y1, x1))):
        out = out + ((img[:, :, base + yy * pw + xx] * m) * w[..., k]).sum(2)
    return out


def pers2equi_bwd(grad_erp, tab, nrows):
    """The transpose by autograd of the restatement: grad_erp [B,C,H,W] -> grad_pers [B,C,ph,pw,N]"""
    g = torch.as_tensor(grad_erp).to(tab["dtype"])
    pers = torch.zeros((g.shape[0], g.shape[1], tab["ph"], tab["pw"], NPATCH[nrows]), dtype=tab["dtype"], requires_grad=True)
    (pers2equi(pers, tab) * g).sum().backward()
    return pers.grad


def conf_blend(pred_w, conf, tab, flipped=None):
    """P(pred_w) / (P(conf) + 1e-8 * [P(conf) <= 1e-8])"""
    a, b = pers2equi(pred_w, tab, flipped), pers2equi(conf, tab, flipped)
    tiny = _c(1e-8, b.dtype)
    return a / (b + tiny * (b <= tiny).to(b.dtype))


def near_entries(tab64, delta=NEAR_DELTA, eps=NEAR_EPS):
    """[N,H,W] bool: the entries whose validity mask an fp32 evaluation may legitimately flip, from float64 alone -- X or Y within delta * P of 0 or of
    its bound while the other conditions hold loosely, or |cos_c| < eps with X, Y loosely in range.  P is the larger patch dimension: X is scaled by the
    height and bounded by the width, Y the other way round, so one tolerance serves both."""
    X, Y, cc, ph, pw = tab64["X"], tab64["Y"], tab64["cos_c"], tab64["ph"], tab64["pw"]
    t = delta * max(ph, pw)
    x_in = (X > -t) & (X < pw + t)
    y_in = (Y > -t) & (Y < ph + t)
    x_edge = (X.abs() < t) | ((X - pw).abs() < t)
    y_edge = (Y.abs() < t) | ((Y - ph).abs() < t)
    return ((x_edge | y_edge) & x_in & y_in & (cc > -eps)) | ((cc.abs() < eps) & x_in & y_in)


def flip_variants(near):
    """Per pixel the near entries are ordered by patch; variant v (0..3) flips the first if v & 1 and the second if v & 2.
    -> (count [H,W] of near entries per pixel, [flipped masks of variants 1, 2, 3])"""
    order = near.cumsum(0)
    first, second = near & (order == 1), near & (order == 2)
    return near.sum(0), [first, second, first | second]


@functools.lru_cache(maxsize=None)
def p2e_case(name):
    """Everything float64 and float32 say about one pers2equi case, computed once: tables, near entries, flip variants."""
    nrows, patch, erp_size, planes = P2E_CASES[name]
    t64 = p2e_tables(nrows, FOV, patch, erp_size, F64)
    t32 = p2e_tables(nrows, FOV, patch, erp_size, F32)
    near = near_entries(t64)
    count, variants = flip_variants(near)
    return dict(name=name, nrows=nrows, patch=patch, erp_size=erp_size, planes=planes, N=NPATCH[nrows], t64=t64, t32=t32, near=near, count=count,
                variants=variants, uncovered=~t64["mask"].any(0) & (count == 0))


@functools.lru_cache(maxsize=None)
def e2p_case(name):
    nrows, patch, erp_size, planes = E2P_CASES[name]
    c64 = e2p_coords(nrows, FOV, patch, erp_size, F64)
    c32 = e2p_coords(nrows, FOV, patch, erp_size, F32)
    return dict(name=name, nrows=nrows, patch=patch, erp_size=erp_size, planes=planes, N=NPATCH[nrows], c64=c64, c32=c32)


def _nanmax(t):
    t = t[~torch.isnan(t)]
    return float(t.abs().max()) if t.numel() else 0.0


def e2p_coord_errors(c64, u, v, xyz, H, W):
    """Pixel error of (u, v) [N,ph,pw] and error of xyz [N,3,ph,pw] against float64 -> dict(x, y, xyz)"""
    to = lambda t: torch.as_tensor(np.asarray(t)).to(F64)
    return dict(x=_nanmax(to(u) - c64["u"]) * (W - 1) / 2, y=_nanmax(to(v) - c64["v"]) * (H - 1) / 2,
                xyz=_nanmax(to(xyz) - xyz_of(c64["lon"], c64["lat"])))


def e2p_coord_e32(case):
    H, W = case["erp_size"]
    c32 = case["c32"]
    return e2p_coord_errors(case["c64"], c32["u"], c32["v"], xyz_of(c32["lon"], c32["lat"]), H, W)


def gate(e32, scale):
    """4 * max(e32, 16 * 2^-24 * scale): four times the distance of one fp32 evaluation from float64, with a floor of 16 half-ulps of the scale"""
    return 4.0 * max(e32, 16 * U24 * scale)


def p2e_inputs(case, planes, seed, hi=1.0, fp16=False):
    B = planes
    ph, pw = case["patch"]
    x = rng_uniform(seed, (B, 1, ph, pw, case["N"])) * np.float32(hi)
    if fp16:
        x = x.astype(np.float16).astype(np.float32)
    return x


def p2e_references(case, fn):
    """fn(tab, flipped) -> result [B,C,H,W]; -> (float64 results of the 4 flip variants, e32: the float32 restatement's largest distance from float64
    over the pixels without a near entry)"""
    want = [fn(case["t64"], None)] + [fn(case["t64"], f) for f in case["variants"]]
    got32 = fn(case["t32"], None).to(F64)
    clean = case["count"] == 0
    e32 = float((got32 - want[0]).abs()[:, :, clean].max())
    return want, e32


def check_p2e(got, want, case, tol, lo, hi, what, rel=0.0, floor=0.0):
    """The flip rule.  got [B,C,H,W]; want: the 4 float64 variants; a pixel with no near entry must be within the gate of variant 0, one with one or two
    near entries within the gate of ONE variant in all its planes, one with more is skipped: finite and inside [lo, hi].  Uncovered pixels are exactly 0.
    The gate of an element is tol + rel * |want| + floor (rel, floor: half an ulp of fp16 storage).  -> (largest error held to the gate, pixels that
    needed a flipped variant, skipped pixels)"""
    got = torch.as_tensor(np.asarray(got)).to(F64)
    count = case["count"]
    assert got.shape == want[0].shape, (got.shape, want[0].shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    # excess over the gate per variant and pixel (largest over the planes); <= 0 passes
    excess = torch.stack([((got - w).abs() - (tol + rel * w.abs() + floor)).amax((0, 1)) for w in want])
    err = torch.stack([(got - w).abs().amax((0, 1)) for w in want])
    allowed = torch.stack([count <= 2, (count == 1) | (count == 2), count == 2, count == 2])
    best = torch.where(allowed, excess, torch.full_like(excess, float("inf"))).min(0)
    judged = count <= 2
    worst = float(best.values[judged].max())
    held = float(torch.gather(err, 0, best.indices[None])[0][judged].max())
    nflip = int((best.indices[judged] != 0).sum())
    skipped = ~judged
    print(f"{what}: max error {held:.3e} (gate {tol:.3e}{' + fp16 half-ulp' if rel else ''}), {nflip} pixel(s) matched a flipped variant, "
          f"{int(skipped.sum())} skipped")
    assert worst <= 0, f"{what}: a pixel misses every allowed float64 variant by {worst:.3e} over its gate, at {np.argwhere((best.values > 0).numpy() & judged.numpy())[:4].tolist()}"
    if bool(skipped.any()):
        s = got[:, :, skipped]
        assert float(s.min()) >= lo and float(s.max()) <= hi, f"{what}: a skipped pixel leaves [{lo}, {hi}]: {float(s.min())} .. {float(s.max())}"
    if bool(case["uncovered"].any()):
        assert bool((got[:, :, case["uncovered"]] == 0).all()), f"{what}: an uncovered pixel is not exactly 0"
    return held, nflip, int(skipped.sum())
