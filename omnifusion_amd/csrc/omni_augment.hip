// omni_augment.hip — the training-time input augmentation of the reference's loaders, folded into the preprocess pass.  gfx950 only.
//
//   flip    np.flip(axis=1) when the coin is 0            dataset_loader_stanford.py:57-60, dataset_loader_360d.py:54-57
//   rotate  np.roll(dx, axis=1), dx a multiple of W/4     :63-67 / :60-64
//   gamma   rgb ** (1/p), p in [1, 2)                     dataset_loader_360d.py:67-71
//   permute rgb[:, :, idx]                                dataset_loader_stanford.py:70-73
//
// flip then roll is ONE column map per item, out[y][x] = in[y][s(x)]:  r = (x - dx) mod W,  s(x) = r  (no flip) | W-1-r (flip);
// colour is out[c] = in[perm[c]] ** g.  Every kernel reads its item's five integers (flip, dx, perm0..2) and its exponent from DEVICE
// memory: nothing is read back, the calls are capturable and a replayed graph picks up new table contents.  dx is reduced modulo W and
// perm modulo 3 in the kernel, so no table content can index outside a frame.  A block belongs to ONE item (block = item * blocks-per-item + j):
// the table entry is wave-uniform and the gamma look-up table is built once per block.
//
//   omni_augment_rgb_u8     omni_preprocess_rgb_u8's arithmetic (omni_area.h) sampled at column s(x), channel perm[c], then gamma
//   omni_augment_depth_u16  omni_preprocess_depth_u16's arithmetic sampled at column s(x)
//   omni_augment_planes     the index map (or its inverse) on planes of 1/2/4/8-byte elements that already live on the device
//
// No atomics, no workspace; every output element is written by one thread from a fixed expression: bitwise reproducible.
#include "omni_internal.h"
#include "omni_area.h"

namespace {

struct AugItem { int flip, dx, p[3]; };

__device__ __forceinline__ int aug_mod(int a, int n) { const int r = a % n; return r < 0 ? r + n : r; }

__device__ __forceinline__ AugItem aug_load(const int* __restrict__ aug, unsigned b, int W)
{
    const int* a = aug + (size_t)b * 5;
    AugItem t;
    t.flip = a[0] != 0;
    t.dx = aug_mod(a[1], W);                                           // any integer, negative included: 0 <= dx < W from here on
#pragma unroll
    for (int c = 0; c < 3; ++c) t.p[c] = aug_mod(a[2 + c], 3);
    return t;
}

// s(x): the source column of destination column x
__device__ __forceinline__ int aug_col(const AugItem& t, int x, int W)
{
    int r = x - t.dx;
    if (r < 0) r += W;
    return t.flip ? W - 1 - r : r;
}

// t(x) = s^-1: where destination column x of the augmented image came from, read backwards (puts a prediction back on the original panorama)
__device__ __forceinline__ int aug_col_inv(const AugItem& t, int x, int W)
{
    const unsigned xp = (unsigned)(t.flip ? W - 1 - x : x), r = xp + (unsigned)t.dx;
    return (int)(r >= (unsigned)W ? r - (unsigned)W : r);
}

// The value entering /255 on the uint8 paths is an integer 0..255, so the whole colour arithmetic is a 256-entry table per item:
// table[k] = k / 255 (no gamma: a null pointer or an exponent of exactly 1 — bit-identical to the plain preprocess) or powf(k / 255, g).
// A block builds it once in LDS, one entry per thread (PX pixels per thread: 1 / PX divisions or powf per pixel instead of 3), and its
// pixels read it.  LUT = false is the direct form (option augment_lut = 0): the same expression per value, the same bits.
template <bool LUT>
__device__ __forceinline__ bool aug_table_setup(float* lut, const float* __restrict__ gamma, unsigned b, float& g)
{
    g = gamma ? gamma[b] : 1.0f;
    const bool on = g != 1.0f;                                          // block-uniform
    if (LUT) {
        const float v = (float)threadIdx.x / 255.0f;
        lut[threadIdx.x] = on ? powf(v, g) : v;
        __syncthreads();
    }
    return on;
}

template <bool LUT>
__device__ __forceinline__ float aug_u8_value(const float* lut, bool on, float g, unsigned k /* 0..255 */)
{
    if (LUT) return lut[k];
    const float v = (float)k / 255.0f;
    return on ? powf(v, g) : v;
}

constexpr int AUG_QUADS = 2;                                           // quads per thread of aug_rgb_same_kernel, 256 apart: 2048 pixels per table
constexpr int AUG_PX = 4;                                              // pixels per thread of aug_rgb_kernel, 256 apart (coalesced)

template <bool LUT>
__global__ __launch_bounds__(256) void aug_rgb_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, const int* __restrict__ aug,
                                                      const float* __restrict__ gamma, int Hs, int Ws, int H, int W, float sy_, float sx_, unsigned bpi)
{
    __shared__ float lut[256];
    const unsigned b = blockIdx.x / bpi;
    float g;
    const bool on = aug_table_setup<LUT>(lut, gamma, b, g);
    const size_t plane = (size_t)H * W;
    const AugItem t = aug_load(aug, b, W);
    const unsigned char* s = src + (size_t)b * Hs * Ws * 3;
    const unsigned sh[3] = {8u * (unsigned)t.p[0], 8u * (unsigned)t.p[1], 8u * (unsigned)t.p[2]};
    for (int j = 0; j < AUG_PX; ++j) {
        const unsigned i = ((blockIdx.x - b * bpi) * AUG_PX + j) * 256u + threadIdx.x;    // 32 bits: H * W < 2^31 (aug_grid)
        if (i >= (unsigned)plane) return;                                                 // (wave-uniform except in the last block of an item)
        const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
        const int xs = aug_col(t, x, W);
        unsigned px = 0;                                                                  // b | g << 8 | r << 16, each 0..255
        if (Hs == H && Ws == W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px |= (unsigned)s[((size_t)y * Ws + xs) * 3 + c] << (8 * c);
        } else {
            const AreaSpan ay = area_span(y, sy_, Hs), ax = area_span(xs, sx_, Ws);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                px |= (unsigned)area_round_u8(area_sample<unsigned char>(s, Hs, Ws, 3, c, ay, ax), Hs == 2 * H && Ws == 2 * W) << (8 * c);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[((size_t)b * 3 + c) * plane + i] = aug_u8_value<LUT>(lut, on, g, (px >> sh[c]) & 255u);
    }
}

// Frames of the network's size, W % 4 == 0: a thread takes AUG_QUADS destination quads, three aligned 16-byte stores each (the stores are
// four times the load bytes).  The four source pixels are 12 contiguous bytes (read backwards under flip) unless the roll's seam falls inside the quad;
// they start at any byte: four aligned dwords around them and a byte funnel shift.  The one quad per row that straddles the seam
// (dx % 4 != 0 only) reads its pixels one by one.  A pixel stays one packed word (b | g << 8 | r << 16): flip is four selects, the channel
// permutation a shift by a scalar, and the table turns the byte into the output value.
template <bool LUT>
__global__ __launch_bounds__(256) void aug_rgb_same_kernel(const unsigned* __restrict__ src, float* __restrict__ dst, const int* __restrict__ aug,
                                                           const float* __restrict__ gamma, int H, int W, unsigned bpi)
{
    __shared__ float lut[256];
    const unsigned b = blockIdx.x / bpi;
    float g;
    const bool on = aug_table_setup<LUT>(lut, gamma, b, g);
    const size_t plane = (size_t)H * W;
    const unsigned wq = (unsigned)W / 4u;
    const AugItem t = aug_load(aug, b, W);
    for (int jq = 0; jq < AUG_QUADS; ++jq) {
        const unsigned q = ((blockIdx.x - b * bpi) * AUG_QUADS + jq) * 256u + threadIdx.x;       // 32 bits: H * W < 2^31 (aug_grid)
        if (q >= (unsigned)(plane / 4)) return;
        const int y = (int)(q / wq), x0 = 4 * (int)(q - (unsigned)y * wq);
        int r0 = x0 - t.dx;
        if (r0 < 0) r0 += W;
        const size_t row = ((size_t)b * plane + (size_t)y * W) * 3;         // byte offset of the source row
        unsigned px[4];                                                    // destination pixels of the quad; bits 24..31 are not used
        if (r0 <= W - 4) {
            const int start = t.flip ? W - 4 - r0 : r0;                     // first of the four source pixels in memory order
            const size_t o = row + (size_t)start * 3;
            const unsigned k = (unsigned)(o & 3);
            const unsigned* p = src + (o >> 2);
            // the fourth dword exists whenever k != 0: o + 12 <= bytes, both bytes and (o - k) + 16 are multiples of 4 and o + 12 is not
            const unsigned a0 = p[0], a1 = p[1], a2 = p[2], a3 = k ? p[3] : 0u;
            const unsigned w0 = __builtin_amdgcn_alignbyte(a1, a0, k), w1 = __builtin_amdgcn_alignbyte(a2, a1, k), w2 = __builtin_amdgcn_alignbyte(a3, a2, k);
            // 12 bytes: b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            const unsigned m0 = w0, m1 = __builtin_amdgcn_alignbyte(w1, w0, 3), m2 = __builtin_amdgcn_alignbyte(w2, w1, 2), m3 = w2 >> 8;
            px[0] = t.flip ? m3 : m0; px[1] = t.flip ? m2 : m1; px[2] = t.flip ? m1 : m2; px[3] = t.flip ? m0 : m3;
        } else {
            const unsigned char* s = reinterpret_cast<const unsigned char*>(src) + row;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned char* sp = s + (size_t)aug_col(t, x0 + j, W) * 3;
                px[j] = (unsigned)sp[0] | (unsigned)sp[1] << 8 | (unsigned)sp[2] << 16;
            }
        }
        float* d = dst + (size_t)b * 3 * plane + (size_t)y * W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned sh = 8u * (unsigned)t.p[c];
            float o4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o4[j] = aug_u8_value<LUT>(lut, on, g, (px[j] >> sh) & 255u);
            *reinterpret_cast<float4*>(d + (size_t)c * plane) = make_float4(o4[0], o4[1], o4[2], o4[3]);
        }
    }
}

__global__ __launch_bounds__(256) void aug_depth_kernel(const unsigned short* __restrict__ src, float* __restrict__ depth, unsigned char* __restrict__ mask,
                                                        const int* __restrict__ aug, int Hs, int Ws, int H, int W, float sy_, float sx_,
                                                        float min_d, float max_d, unsigned bpi)
{
    const unsigned b = blockIdx.x / bpi;
    const size_t plane = (size_t)H * W;
    const unsigned i = (blockIdx.x - b * bpi) * 256u + threadIdx.x;
    if (i >= (unsigned)plane) return;
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
    const AugItem t = aug_load(aug, b, W);
    const int xs = aug_col(t, x, W);
    const unsigned short* s = src + (size_t)b * Hs * Ws;
    float v;
    if (Hs == H && Ws == W) v = (float)s[(size_t)y * Ws + xs];
    else { const AreaSpan ay = area_span(y, sy_, Hs), ax = area_span(xs, sx_, Ws); v = area_sample<unsigned short>(s, Hs, Ws, 1, 0, ay, ax); }
    v = v / 65535.0f * 128.0f;
    const bool m = (v <= max_d) && (v > min_d);                        // elementwise: commutes with the column map
    depth[(size_t)b * plane + i] = m ? v : 0.0f;
    mask[(size_t)b * plane + i] = m ? 1 : 0;
}

// planes [B][C][H][W] of T (raw bytes of the element): dst[b][c][y][x] = src[b][c'][y][col(x)]; gamma (float32 elements only) is powf per value
template <typename T>
__global__ __launch_bounds__(256) void aug_planes_kernel(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ aug,
                                                         const float* __restrict__ gamma, int C, int H, int W, int color, int inverse, unsigned bpi)
{
    const unsigned b = blockIdx.x / bpi;
    const size_t plane = (size_t)H * W, n = plane * C;
    const unsigned i = (blockIdx.x - b * bpi) * 256u + threadIdx.x;     // 32 bits: C * H * W < 2^31 (aug_grid)
    if (i >= (unsigned)n) return;
    const int x = (int)(i % (unsigned)W), c = (int)(i / (unsigned)plane);
    const AugItem t = aug_load(aug, b, W);
    const int xs = inverse ? aug_col_inv(t, x, W) : aug_col(t, x, W);
    const int cs = color ? (c == 0 ? t.p[0] : (c == 1 ? t.p[1] : t.p[2])) : c;                                 // (color implies C == 3; the host clears it for the inverse map)
    T v = src[(size_t)b * n + (size_t)cs * plane + (i - (size_t)c * plane) - x + xs];
    if constexpr (sizeof(T) == 4) {
        if (gamma) {
            const float g = gamma[b];
            if (g != 1.0f) v = __float_as_uint(powf(__uint_as_float(v), g));
        }
    }
    dst[(size_t)b * n + i] = v;
}

// blocks of 256 threads (`per_block` elements each) per item of `per_item` elements; false when the grid would not fit
bool aug_grid(size_t per_item, int B, unsigned& bpi, unsigned& blocks, unsigned per_block = 256)
{
    const size_t per = (per_item + per_block - 1) / per_block, total = per * (size_t)B;
    if (per == 0 || per_item > 0x7fff0000ull || total > 0x7fffffffull) return false;       // (the kernels index inside an item with 32 bits)
    bpi = (unsigned)per; blocks = (unsigned)total;
    return true;
}

}  // namespace

extern "C" int omni_augment_rgb_u8(const unsigned char* src_hwc, float* dst_chw, const int* aug, const float* gamma, int B, int Hs, int Ws, int H, int W,
                                   omni_stream_t stream)
{
    if (!src_hwc || !dst_chw || !aug) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_rgb_u8: null device pointer");
    if (B < 0 || Hs < 1 || Ws < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_rgb_u8: bad shape");
    if (H > Hs || W > Ws) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_rgb_u8: INTER_AREA is a down-scale here (the loader shrinks 4096x2048 scans)");
    if (B == 0) return OMNI_OK;
    const bool lut = omni_options().augment_lut != 0;
    unsigned bpi, blocks;
    if (Hs == H && Ws == W && W % 4 == 0 && (uintptr_t)src_hwc % 4 == 0 && (uintptr_t)dst_chw % 16 == 0) {
        if (!aug_grid((size_t)H * W / 4, B, bpi, blocks, 256 * AUG_QUADS)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_rgb_u8: item or batch too large for one launch");
        if (lut) hipLaunchKernelGGL(aug_rgb_same_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned*)src_hwc, dst_chw, aug, gamma, H, W, bpi);
        else hipLaunchKernelGGL(aug_rgb_same_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned*)src_hwc, dst_chw, aug, gamma, H, W, bpi);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    if (!aug_grid((size_t)H * W, B, bpi, blocks, 256 * AUG_PX)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_rgb_u8: item or batch too large for one launch");
    const float sy = (float)((double)Hs / H), sx = (float)((double)Ws / W);
    if (lut) hipLaunchKernelGGL(aug_rgb_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src_hwc, dst_chw, aug, gamma, Hs, Ws, H, W, sy, sx, bpi);
    else hipLaunchKernelGGL(aug_rgb_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src_hwc, dst_chw, aug, gamma, Hs, Ws, H, W, sy, sx, bpi);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_augment_depth_u16(const unsigned short* src, float* depth, unsigned char* mask, const int* aug, int B, int Hs, int Ws, int H, int W,
                                      float min_depth, float max_depth, omni_stream_t stream)
{
    if (!src || !depth || !mask || !aug) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_depth_u16: null device pointer");
    if (B < 0 || Hs < 1 || Ws < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_depth_u16: bad shape");
    if (H > Hs || W > Ws) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_depth_u16: INTER_AREA is a down-scale here");
    if (B == 0) return OMNI_OK;
    unsigned bpi, blocks;
    if (!aug_grid((size_t)H * W, B, bpi, blocks)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_depth_u16: item or batch too large for one launch");
    hipLaunchKernelGGL(aug_depth_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, depth, mask, aug, Hs, Ws, H, W,
                       (float)((double)Hs / H), (float)((double)Ws / W), min_depth, max_depth, bpi);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_augment_planes(const void* src, void* dst, int elem_bytes, const int* aug, const float* gamma, int B, int C, int H, int W,
                                   int color, int inverse, omni_stream_t stream)
{
    if (!src || !dst || !aug) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: null device pointer");
    if (src == dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: src and dst must differ (the map is not done in place)");
    if (B < 0 || C < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: bad shape");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: elem_bytes must be 1, 2, 4 or 8");
    if (((uintptr_t)src | (uintptr_t)dst) % (unsigned)elem_bytes) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: pointers must be aligned to the element size");
    if (color && C != 3) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: color needs C == 3");
    if (color && gamma && elem_bytes != 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_augment_planes: gamma needs float32 elements");
    if (B == 0) return OMNI_OK;
    if (inverse) color = 0;                                             // the inverse puts predictions back: columns only
    if (!color) gamma = nullptr;
    unsigned bpi, blocks;
    if (!aug_grid((size_t)C * H * W, B, bpi, blocks)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_augment_planes: item or batch too large for one launch");
    const hipStream_t st = (hipStream_t)stream;
    switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(aug_planes_kernel<unsigned char>, dim3(blocks), dim3(256), 0, st, (const unsigned char*)src, (unsigned char*)dst, aug, gamma, C, H, W, color, inverse, bpi); break;
    case 2: hipLaunchKernelGGL(aug_planes_kernel<unsigned short>, dim3(blocks), dim3(256), 0, st, (const unsigned short*)src, (unsigned short*)dst, aug, gamma, C, H, W, color, inverse, bpi); break;
    case 4: hipLaunchKernelGGL(aug_planes_kernel<unsigned>, dim3(blocks), dim3(256), 0, st, (const unsigned*)src, (unsigned*)dst, aug, gamma, C, H, W, color, inverse, bpi); break;
    default: hipLaunchKernelGGL(aug_planes_kernel<unsigned long long>, dim3(blocks), dim3(256), 0, st, (const unsigned long long*)src, (unsigned long long*)dst, aug, gamma, C, H, W, color, inverse, bpi); break;
    }
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
