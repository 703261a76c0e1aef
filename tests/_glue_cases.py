"""The network's oldest kernels — the stem, the 3x3/2 max-pool, bilinear up-sampling, the broadcast adds and the heads of csrc/omni_net.hip, the
matrix-core stem of csrc/omni_conv_halo.hip and the split-half ("SH") conversion of csrc/omni_sh.h — as case tables, float64 restatements and a
host model of the SH format.  numpy / torch on the CPU only; tests/test_glue_cpu.py checks this file against stock torch, tests/test_glue_float64_gpu.py
holds the kernels to it.

Exact operators (pool, adds, the identity up-sampling, the SH conversions) are compared bit for bit with the host model.  The others pass a gate
that comes from the reference side alone (tests/test_spatial_ops_gpu.py): with nerr = max|v - v64| / max(1, rms(v64)) and e32 = nerr of torch's own
float32 CPU evaluation, the device must satisfy nerr <= 8 * max(e32, 5e-7), plus Q * max|v64| / max(1, rms(v64)) where the result is SH (Q: the
format's largest relative error, sh_bounds()); the f16x3 stem passes CONV_GATE, the f16x1 stem the check of tests/test_precision_f16x1_gpu.py
(f16x1_check, stem_f16x1_refs: they live here so that both files apply the same one).
"""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

FACTOR, FLOOR = 8.0, 5e-7                     # tests/test_spatial_ops_gpu.py
CONV_GATE = 3e-5                              # tests/test_conv_bwd_gpu.py: the f16x3 products' gate
X1_REL = 1e-6                                 # tests/test_precision_f16x1_gpu.py: fp32-accumulation gate, relative to sum |a||w| (+ |bias|)
F64 = torch.float64


def gen(*key):
    """one seeded generator per case key (crc32 of its repr: stable across runs and machines)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------ the split-half format, exactly as sh_split4 / sh_join4 / sh_off state it
SH_MAX = np.float32(65504.0)
SH_TINY = np.float32(2.0 ** -14)              # below it hi = 0
SH_SCALE, SH_INV = np.float32(2048.0), np.float32(2.0 ** -11)


def sh_split(x, tiny=SH_TINY):
    """float32 array -> (hi, lo) float16 arrays: |x| saturates at 65504 (+-inf included; NaN compares false and stays), hi = fp16(x) and 0 for
    |x| < 2^-14, lo = fp16((x - hi) * 2048), every step in float32 as the kernel takes it.  `tiny`: the threshold (the tests move it to show
    that they notice)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = np.where(np.abs(x) > SH_MAX, np.copysign(SH_MAX, x), x).astype(np.float32)
        hi = np.where(np.abs(xs) < tiny, np.float32(0.0), xs).astype(np.float16)
        lo = ((xs - hi.astype(np.float32)) * SH_SCALE).astype(np.float16)
    return hi, lo


def sh_join(hi, lo):
    """fma(lo, 2^-11, hi) in float32: lo * 2^-11 is exact (eleven bits times a power of two, never below 2^-35), so the sum's one rounding is the fma's"""
    with np.errstate(invalid="ignore"):
        return (lo.astype(np.float32) * SH_INV + hi.astype(np.float32)).astype(np.float32)


def sh_pack(x, tiny=SH_TINY):
    """float32 tensor [..., C] (C % 32 == 0) -> the SH tensor's bytes as a float32 tensor of the same shape: per 32 channels, 32 hi halfs then 32 lo halfs"""
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.shape[-1] % 32 == 0
    hi, lo = sh_split(x.numpy().reshape(-1, 32), tiny)
    return torch.from_numpy(np.stack([hi, lo], 1).reshape(-1).view(np.float32).copy()).reshape(x.shape)


def sh_unpack(p):
    """the float32 values an SH tensor holds"""
    h = p.contiguous().numpy().reshape(-1).view(np.float16).reshape(-1, 2, 32)
    return torch.from_numpy(sh_join(h[:, 0], h[:, 1]).reshape(-1).copy()).reshape(p.shape)


def sh_canonical(x):
    """-> (bytes, values) of x as an SH STORE of an SH value leaves it.  split(join(split(x))) is a fixed point of bytes; split(x) alone is not quite:
    where lo rounds up to exactly half an ulp of hi and hi is odd, the joined value is a tie that splits as (hi + ulp, -half ulp)."""
    v = sh_unpack(sh_pack(x))
    return sh_pack(v), v


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits(exp, sign, mant):
    return ((np.uint32(sign) << np.uint32(31)) | (np.uint32(exp) << np.uint32(23)) | np.asarray(mant, np.uint32)).astype(np.uint32)


SWEEP_MANTISSAS = 1000


@functools.lru_cache(maxsize=None)
def sh_sweep():
    """float32 bit patterns: every exponent x both signs x a mantissa grid (0, 1, all ones, the fp16 rounding ties — bit 12 alone and with bit 13 —
    and 1,000 seeded mantissas), then the values at which the format changes its behaviour; padded with zeros to a multiple of 32."""
    rng = np.random.RandomState(zlib.crc32(b"sh sweep"))
    mant = np.concatenate([np.array([0, 1, 0x7FFFFF, 0x1000, 0x3000], np.uint32), rng.randint(0, 1 << 23, SWEEP_MANTISSAS).astype(np.uint32)])
    grid = np.concatenate([_bits(e, s, mant) for e in range(256) for s in (0, 1)]).view(np.float32)
    f = np.float32
    up, dn = lambda v: np.nextafter(f(v), f(np.inf)), lambda v: np.nextafter(f(v), f(-np.inf))
    t, m = f(2.0 ** -14), f(65504.0)
    special = np.array([0.0, -0.0, t, -t, up(t), dn(t), up(-t), dn(-t), m, -m, up(m), dn(m), up(-m), dn(-m), 65519.996, -65519.996, 65520.0, -65520.0,
                        np.finfo(f).max, -np.finfo(f).max, np.inf, -np.inf, np.nan], dtype=f)
    x = np.concatenate([grid, special])
    return np.concatenate([x, np.zeros(-len(x) % 32, f)])


def sweep_classes(x):
    """-> (normal or zero, fp32 denormal, NaN) masks of a float32 array"""
    a = np.abs(x)
    nan = np.isnan(x)
    den = (a > 0) & (a < np.finfo(np.float32).tiny)
    return ~nan & ~den, den, nan


def _err_over(exp, mant, tiny=SH_TINY):
    x = _bits(exp, 0, mant).view(np.float32)
    x = x[x <= SH_MAX]
    hi, lo = sh_split(x, tiny)
    e = np.abs(sh_join(hi, lo).astype(np.float64) - x.astype(np.float64))
    return float((e / x.astype(np.float64)).max()), float(e.max())


@functools.lru_cache(maxsize=None)
def sh_bounds(tiny=float(SH_TINY)):
    """-> (Q, A) from the host model alone.  Q: the largest relative error of join(split(x)) over the normal range [2^-14, 65504]; A: the largest
    absolute error for 2^-126 <= x < 2^-14.  The error of x = 2^e (1 + m 2^-23) depends on e and, through hi's rounding, on m: the two binades where
    the bounds are attained (e = -14: lo is an fp16 denormal, spacing 2^-35 of x; e = -15: hi = 0 and lo carries eleven bits of x) are taken
    exhaustively, every other binade on a grid of ten upper x all 8,192 lower mantissa patterns (the thirteen bits hi does not hold)."""
    tiny = np.float32(tiny)
    every = np.arange(1 << 23, dtype=np.uint32)
    rng = np.random.RandomState(zlib.crc32(b"sh bounds"))
    upper = np.concatenate([[0, 1023], rng.randint(0, 1024, 8)]).astype(np.uint32)
    grid = ((upper[:, None] << np.uint32(13)) | np.arange(1 << 13, dtype=np.uint32)[None, :]).reshape(-1)
    q = a = 0.0
    for e in range(-126, 16):
        rel, ab = _err_over(e + 127, every if e in (-14, -15) else grid, tiny)
        if e >= -14:
            q = max(q, rel)
        else:
            a = max(a, ab)
    return q, a


# ------------------------------------------------------------------ the gate
def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def gate(r32, r64, sh=False):
    """FACTOR * max(e32, FLOOR) (+ Q * max|v64| / max(1, rms(v64)) for an SH result)"""
    g = FACTOR * max(nerr(r32, r64), FLOOR)
    if sh:
        g += sh_bounds()[0] * r64.abs().max().item() / max(1.0, r64.double().pow(2).mean().sqrt().item())
    return g


RATIOS = {}                                   # operator -> the largest error / gate the running session has seen (DESIGN.md §22b keeps the MI355X's)


def report(op, what, got, ref, g):
    """prints the error, the gate and their ratio; a NaN (an element no kernel wrote) or a miss fails"""
    assert got.shape == ref.shape, (op, what, got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{op} {what}: NaN in the result (an unwritten element?)"
    e = nerr(got, ref)
    RATIOS[op] = max(RATIOS.get(op, 0.0), e / g)
    print(f"GLUE {op} {what}: normalised error {e:.3e}  gate {g:.3e}  ratio {e / g:.3f}  (largest so far for {op}: {RATIOS[op]:.3f})")
    assert e <= g, f"{op} {what}: {e:.3e} > {g:.3e}"
    return e


# ------------------------------------------------------------------ restatements (float64 is the reference; NHWC as the kernels keep their tensors)
def stem(x, w, b, dtype):
    """relu(conv 7x7, stride 2, padding 3, 3 -> 64): x [M, 3, P, P], w [64, 3, 7, 7] -> [M, P/2, P/2, 64]; as 147 shifted strided slices"""
    x, w = x.to(dtype), w.to(dtype)
    M, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (3, 3, 3, 3))
    y = torch.zeros((M, Ho, Wo, 64), dtype=dtype)
    for ky in range(7):
        for kx in range(7):
            y += torch.einsum("mchw,oc->mhwo", xp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], w[:, :, ky, kx])
    if b is not None:
        y = y + b.to(dtype)
    return torch.relu(y)


def stem_stock(x, w, b, dtype):
    return torch.relu(F.conv2d(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), stride=2, padding=3)).permute(0, 2, 3, 1).contiguous()


def stem_weights_f32(w):
    """[64, 3, 7, 7] -> omni_stem_f32's [147][64], k = (ky * 7 + kx) * 3 + c"""
    return w.permute(2, 3, 1, 0).reshape(147, 64).contiguous()


def stem_weights_f16x3(w):
    """[64, 3, 7, 7] -> omni_stem_sh_f16x3's [64][192] (k = (c * 7 + ky) * 8 + kx; kx = 7 and k >= 168 zero), split"""
    from omnifusion_amd.model._engine import split_weights_f16x3
    wk = torch.zeros(64, 3, 7, 8)
    wk[..., :7] = w
    return split_weights_f16x3(torch.cat([wk.reshape(64, 168), torch.zeros(64, 24)], 1))


def maxpool(x, dtype, pad_value=-math.inf):
    """3x3 / stride 2 / padding 1 over x [M, H, W, C]: the largest of the taps INSIDE the map (the padding never wins), a NaN is dropped
    (fmaxf); as nine shifted strided slices"""
    x = x.to(dtype)
    x = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    M, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((M, H + 2, W + 2, C), pad_value, dtype=dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = torch.full((M, Ho, Wo, C), -math.inf, dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            y = torch.maximum(y, xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    return y


def maxpool_stock(x, dtype):
    return F.max_pool2d(x.to(dtype).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def pool_padded_sides(H, W):
    """the sides of an H x W map at which some 3x3 / 2 / 1 window reaches into the padding"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    s = {"top", "left"}                                              # window 0 starts at row / column -1
    if 2 * (Ho - 1) + 1 >= H:
        s.add("bottom")
    if 2 * (Wo - 1) + 1 >= W:
        s.add("right")
    return s


def upsample(x, Ho, Wo, dtype):
    """bilinear, align_corners=False: x [M, H, W, C] -> [M, Ho, Wo, C]; source index max(H / Ho * (o + 0.5) - 0.5, 0), the far neighbour clamped to the map"""
    x = x.to(dtype)
    M, H, W, C = x.shape

    def axis(n, no):
        f = (torch.arange(no, dtype=dtype) + 0.5) * (n / no) - 0.5
        f = f.clamp(min=0.0)
        i0 = f.floor().long().clamp(max=n - 1)
        return i0, (i0 + 1).clamp(max=n - 1), f - i0.to(dtype)

    y0, y1, ly = axis(H, Ho)
    x0, x1, lx = axis(W, Wo)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def upsample_stock(x, Ho, Wo, dtype):
    return F.interpolate(x.to(dtype).permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


def heads(x, w, bp, bw, conf, dtype):
    """x [M, P, P, 32], w [2][9][32] (pred, then weight_pred; tap = ky * 3 + kx) -> (a, c, z): z [M, P, P, 2] the two 3x3 convolutions + bias,
    c = sigmoid(z1), a = relu(z0) * (c if conf else 1); as nine shifted slices"""
    x, w = x.to(dtype), w.to(dtype)
    M, P = x.shape[0], x.shape[1]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    z = torch.zeros((M, P, P, 2), dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            z += torch.einsum("mhwc,oc->mhwo", xp[:, ky:ky + P, kx:kx + P], w[:, ky * 3 + kx])
    z = z + torch.tensor([bp, bw], dtype=dtype)
    c = torch.sigmoid(z[..., 1])
    return torch.relu(z[..., 0]) * (c if conf else 1.0), c, z


def heads_stock(x, w, bp, bw, conf, dtype):
    k = w.to(dtype).reshape(2, 3, 3, 32).permute(0, 3, 1, 2)
    z = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), k, torch.tensor([bp, bw], dtype=dtype), padding=1)
    c = torch.sigmoid(z[:, 1])
    return torch.relu(z[:, 0]) * (c if conf else 1.0), c


def add_hw(x, y):
    """x [M, HW, C] + y [M, C]: one rounding in x's dtype"""
    return x + y[:, None, :]


def add_period(x, y):
    """x[i] + y[i % period] over the flat tensors"""
    return x + y.repeat(x.numel() // y.numel() + 1)[:x.numel()].reshape(x.shape)


# ------------------------------------------------------------------ the f16x1 check (tests/test_precision_f16x1_gpu.py applies it to every f16x1 kernel)
def f16x1_check(out, ref_hi, ref_exact, scale, what, rel=X1_REL):
    """out within rel * scale of the hi-only reference; the hi-only and exact references at least 3x further apart somewhere"""
    err = ((out.double().cpu() - ref_hi).abs() / scale).max().item()
    gap = ((ref_exact - ref_hi).abs() / scale).max().item()
    assert gap > 3 * rel, (what, "the gate would not tell f16x1 from f16x3 here", gap)
    assert err <= rel, (what, err, gap)
    return err


def stem_f16x1_refs(x, b, W16):
    """-> (ref_hi, ref_exact, scale) of the f16x1 stem, float64 [M, P/2, P/2, 64]: fp16(x) (0 below 2^-14) . hi(W16) and x . (hi + lo 2^-11)(W16), both
    + b and ReLU; scale = sum |a||w| + |b|.  W16: stem_weights_f16x3's tensor (on the CPU)"""
    xh = torch.where(x.abs() < 6.103515625e-05, torch.zeros_like(x), x).half().double()
    wf = W16.double().cpu()
    wh = wf[:, :, 0, :].reshape(64, 192)[:, :168].reshape(64, 3, 7, 8)[..., :7]
    we = (wf[:, :, 0, :] + wf[:, :, 1, :] * 2.0 ** -11).reshape(64, 192)[:, :168].reshape(64, 3, 7, 8)[..., :7]
    conv = lambda x_, w_: F.conv2d(x_, w_, stride=2, padding=3).permute(0, 2, 3, 1)
    ref_hi, ref_ex = F.relu(conv(xh, wh) + b.double()), F.relu(conv(x.double(), we) + b.double())
    return ref_hi, ref_ex, conv(xh.abs(), wh.abs()) + b.double().abs()


# ------------------------------------------------------------------ cases
#              (M, P): omni_stem_f32 / omni_stem_sh, blocks of 8 x 8 outputs
STEM_F32_CASES = [(1, 16),        # one tile
                  (2, 48),        # 3 x 3 tiles, one of them interior
                  (3, 32)]

# omni_stem_sh_f16x3 / _f16x1 (stem_sh_impl): Po = P / 2, strips = M * Po / 8 (8 output rows), tps = Po / 16 tiles a strip, ntiles = strips * tps;
# split = 4 if strips < 256 and Po % 64 == 0, else 2 if strips < 512 and Po % 32 == 0, else 1.  conv_stem_pc = 0: a grid of strips x split.
# conv_stem_pc = 1: blocks of tpb consecutive tiles, tpb = tps / split, or ceil(ntiles / CUs) where split == 1 and ntiles > CUs * tps.
#              (M, P)                what it reaches on 256 CUs (the last two are SIZED for 256 CUs; they must pass on any count)
STEM_MM_CASES = [(1, 32),          # 2 tiles, split 1, tpb 1
                 (2, 64),          # split 2: 8 strips of two tiles
                 (3, 96),          # split 1, three tiles a strip: tpb 3
                 (70, 64),         # split 2 at 280 strips
                 (301, 32),        # 602 strips of one tile: tpb = ceil(602 / 256) = 3, 201 blocks, the last with two tiles; blocks straddle images (2 strips each)
                 (131, 64)]        # 524 strips of two tiles = 1,048 tiles: tpb = ceil(1048 / 256) = 5, 210 blocks, the last with three; blocks straddle strips and images
STEM_MM_NO_EPI_LDS = STEM_MM_CASES[:2]       # ... also with conv_epi_lds = 0


def stem_launch(M, P, ncu=256, pc=True):
    """stem_sh_impl's arithmetic -> dict(split, tps, ntiles, tpb, blocks, last): tiles per block, blocks, tiles of the last block (pc), or the grid (not pc)"""
    Po = P // 2
    strips, tps = M * (Po // 8), Po // 16
    split = 4 if (strips < 256 and Po % 64 == 0) else 2 if (strips < 512 and Po % 32 == 0) else 1
    ntiles = strips * tps
    if not pc:
        return dict(split=split, tps=tps, ntiles=ntiles, grid=(strips, split))
    tpb = tps // split
    if split == 1 and ntiles > ncu * tps:
        tpb = -(-ntiles // ncu)
    blocks = -(-ntiles // tpb)
    return dict(split=split, tps=tps, ntiles=ntiles, tpb=tpb, blocks=blocks, last=ntiles - (blocks - 1) * tpb, strips=strips)


@functools.lru_cache(maxsize=None)
def stem_case(M, P):
    """-> x [M, 3, P, P], w [64, 3, 7, 7] / sqrt(147), b [64]"""
    g = gen("stem", M, P)
    return torch.randn((M, 3, P, P), generator=g), torch.randn((64, 3, 7, 7), generator=g) / math.sqrt(147.0), 0.1 * torch.randn(64, generator=g)


@functools.lru_cache(maxsize=None)
def stem_reference(M, P):
    """-> (float64 reference, e32-side float32 evaluation) of a stem case, computed once and left unchanged"""
    x, w, b = stem_case(M, P)
    return stem_stock(x, w, b, F64), stem_stock(x, w, b, torch.float32)


#              (M, H, W, C)
POOL_CASES = [(2, 1, 1, 32), (2, 2, 5, 32), (3, 7, 9, 64), (1, 1, 6, 96), (2, 8, 8, 32)]
POOL_KINDS = ("randn", "negative")
POOL_EXTREME = (3, 7, 9, 64)                  # its randn map holds +-65504
POOL_NAN = (2, 8, 8, 32)                      # its randn map holds one NaN


@functools.lru_cache(maxsize=None)
def pool_case(M, H, W, C, kind):
    """-> (bytes of the SH input, its float32 values).  negative: -|randn| - 1 everywhere, so zero padding would win every border window"""
    x = torch.randn((M, H, W, C), generator=gen("pool", M, H, W, C, kind))
    if kind == "negative":
        x = -x.abs() - 1.0
    elif (M, H, W, C) == POOL_EXTREME:
        x[0, 3, 4, 0], x[1, 0, 0, 5], x[2, 6, 8, 63], x[2, 6, 7, 63] = 65504.0, -65504.0, 65504.0, -65504.0
    elif (M, H, W, C) == POOL_NAN:
        x[1, 3, 3, 7] = float("nan")
    return sh_canonical(x)


#              omni_add_hw_f32 (M, HW, C)           omni_add_period_f32 (total, period)
ADD_HW_CASES = [(1, 1, 3), (3, 5, 7), (2, 120, 64)]
ADD_PERIOD_CASES = [(37, 5), (64, 64), (3 * 7680 + 5, 7680)]
#              the SH forms (M, HW, C); periods 32, C * HW and the whole tensor.  (2, 5, 32): 80 threads' worth of quads, not a multiple of 256
ADD_SH_CASES = [(2, 5, 32), (3, 7, 96), (4, 8, 32)]


def add_sh_periods(M, HW, C):
    return [32, C * HW, M * HW * C]


def add_case(*key):
    """-> x, y float32 of the given flat sizes: key = (name, x shape, y shape)"""
    g = gen("add", *key)
    return torch.randn(key[1], generator=g), torch.randn(key[2], generator=g)


#              2x (M, H, W, C)
UP2_CASES = [(2, 1, 1, 32), (2, 1, 5, 32), (3, 3, 7, 64), (2, 8, 8, 96)]
#              other ratios (M, H, W, C, Ho, Wo)
UP_RATIO_CASES = [(3, 10, 12, 64, 15, 30), (2, 4, 4, 32, 7, 5), (2, 8, 6, 32, 4, 3)]
UP_SH_CASES = [(M, H, W, C, 2 * H, 2 * W) for M, H, W, C in UP2_CASES] + UP_RATIO_CASES
UP_F32_CASES = [(3, H, W, C, Ho, Wo) for C in (4, 12) for H, W, Ho, Wo in ((10, 12, 15, 30), (3, 7, 6, 14))]
UP_IDENTITY_CASES = [(2, 8, 8, 96), (3, 3, 7, 64)]


@functools.lru_cache(maxsize=None)
def up_case(M, H, W, C, sh):
    x = torch.randn((M, H, W, C), generator=gen("up", M, H, W, C))
    return sh_canonical(x) if sh else (x, x)


#              (M, P, conf): blocks of 16 x 16 pixels, at most 768 of them
HEADS_CASES = [(2, 8, 1),         # smaller than a tile
               (3, 24, 0),        # ragged tiles (2 x 2 of them)
               (2, 40, 1),        # ragged tiles (3 x 3)
               (49, 64, 1)]       # 49 * 4 * 4 = 784 tiles > 768: sixteen blocks take a second tile
HEADS_NO_CONF_PLANE = (3, 24, 0)             # ... also with out_c = NULL
HEADS_SHARP = (2, 40, 1)                     # ... also with the weight head scaled to pre-activations of about +-100


def heads_tiles(M, P):
    """-> (tiles, blocks, blocks that take a second tile)"""
    t = -(-P // 16)
    n = M * t * t
    return n, min(n, 768), max(0, n - 768)


@functools.lru_cache(maxsize=None)
def heads_case(M, P, sharp=False):
    """-> x [M, P, P, 32], w [2][9][32], bp, bw.  sharp: the weight head scaled (from the float64 pre-activation alone) so that it spans +-100"""
    g = gen("heads", M, P)
    x = torch.randn((M, P, P, 32), generator=g)
    w = torch.randn((2, 9, 32), generator=g) / math.sqrt(288.0)
    bp, bw = 0.25, -0.125
    if sharp:
        z = heads(x, w, bp, bw, 1, F64)[2][..., 1] - bw
        w = w.clone()
        w[1] *= 100.0 / min(float(z.max()), -float(z.min()))      # both signs reach 100
    return x, w, bp, bw
