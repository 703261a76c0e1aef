// omni_e2p_common.h — what the equi2pers units share (omni_equi2pers.hip: entry points and the box kernel; omni_e2p_ref.hip: the reference-layout and
// direct-gather forwards; omni_e2p_tables.hip: the per-geometry tables; omni_equi2pers_bwd.hip: the backward).  Device side: the argument block, the tap /
// sampling-coordinate helpers (forceinline: every kernel evaluates the SAME functions, same bits), what the LDS-DMA box kernels have in common, and ONE kernel
// template, e2p_lds_kernel<TS, BWD> — the library is built without relocatable device code, so each of its instantiations still lives in exactly one .hip:
// <TS, false> in omni_e2p_tables.hip (tile-flag builder and fp32 forward fallback), <TS, true> in omni_equi2pers_bwd.hip.  Host side: fill_args and the
// few launchers that cross units.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include <vector>
#include <algorithm>
#include <utility>
#include "omni_internal.h"
#include "omni_reduce.h"

namespace {

struct E2PArgs {
    const void* erp; void* pers;
    int B, C, H, W, ph, pw;
    float fovx, fovy;          // fov_w/360, fov_h/180  (equi2pers_v3.py:24)
    float stepx, stepy;        // linspace(0,1,P) step (:29)
    float sx_scale, sy_scale;  // (W-1)/2, (H-1)/2  (grid_sample align_corners=True)
    int dbg;                   // tuning hook (OMNI_E2P_DBG): 1 = suppress stores, 2 = suppress box loads
    const float2* ixy;         // per-geometry table of clamped sampling coordinates [N][ph][pw] (e2p_lds_kernel), or null
    long long* trace;          // debug build, OMNI_E2P_DBG bit 16: per-block time stamps (omni_debug_set_trace)
    int store_mode;            // option e2p_store: 0 plain | 1 non-temporal (default)
    int dbg_skip_fb;           // timing experiment only (option e2p_ref_lds = 2)
    PatchTab tab;
};

struct Tap {                    // one bilinear footprint on the ERP, branch-free to fetch
    int r0, r1;                 // element offsets of the two tap rows (see e2p_tap)
    int sel;                    // PAIR: 1 when the 2-wide load was shifted left by one (x0 == W-1)
                                // !PAIR: column step dx (0 when x0+1 is outside)
    float w00, w01, w10, w11;   // ATen's nw, ne, sw, se weights
};

constexpr float PI_F = 3.14159265358979323846f;
constexpr float PI_2_F = 1.57079632679489661923f;

__device__ __forceinline__ float lin01(int idx, int steps, float step)
{
    // torch.linspace(0, 1, steps)[idx] in fp32 (two-sided), equi2pers_v3.py:29
    // (ATen evaluates the upper half as ONE fma: linspace(0,1,15)[7] = 0.49999997, not 0.5)
    return (idx < (steps >> 1)) ? step * (float)idx : fmaf(-step, (float)(steps - 1 - idx), 1.0f);
}

// inverse gnomonic for sample (h, w) of patch n -> unwrapped lon, lat and the pieces xyz needs
__device__ __forceinline__ void e2p_lonlat(const E2PArgs& a, int n, int h, int w,
                                           float& lon, float& lat, float& x, float& q, float& t, float& inv)
{
    const float sw = lin01(w, a.pw, a.stepx), sh = lin01(h, a.ph, a.stepy);
    x = ((sw * 2.0f - 1.0f) * PI_F) * a.fovx;                 // :86-89
    const float y = ((sh * 2.0f - 1.0f) * PI_2_F) * a.fovy;
    const float sp = a.tab.sphi[n], cp = a.tab.cphi[n];
    q = cp - y * sp;
    t = sp + y * cp;
    inv = 1.0f / sqrtf(1.0f + x * x + y * y);
    float sl = t * inv;
    sl = fminf(1.0f, fmaxf(-1.0f, sl));
    lat = asinf(sl);
    lon = a.tab.lam0[n] + atan2f(x, q);
    // Reference quirk q4: at x == y == 0 (the centre sample when BOTH patch dims are odd and their
    // linspace midpoints are exactly 0.5) the reference divides 0/0 at :99 -> lat = NaN while
    // lon = l0 + atan2(0, 0) = l0.  ATen then clips the NaN row coordinate to 0, so that sample reads
    // the top ERP row, and xyz is NaN.  Reproduced, not fixed: it defines parity.
    if (x == 0.0f && y == 0.0f) { lat = __builtin_nanf(""); t = lat; }
}

__device__ __forceinline__ void e2p_uv(float lon, float lat, float& u, float& v)
{
    v = lat / PI_2_F;                                          // :101
    u = lon / PI_F;                                            // :102
    if (u > 1.0f) u -= 2.0f;                                   // :103
    if (u < -1.0f) u += 2.0f;                                  // :104
}

// Footprint of sample (h, w) of patch n.  ATen's grid_sampler skips taps that fall outside the
// image; a clipped coordinate is integral there, so such a tap also has weight exactly 0.  The
// outside tap is therefore ALIASED onto the in-range pixel of the same row/column (never onto a
// pixel ATen would not have read), which keeps every load unconditional and in bounds.
template <bool PAIR>
__device__ __forceinline__ Tap e2p_tap(const E2PArgs& a, int n, int h, int w)
{
    float lon, lat, x, q, t, inv, u, v;
    e2p_lonlat(a, n, h, w, lon, lat, x, q, t, inv);
    e2p_uv(lon, lat, u, v);
    // ATen grid_sampler: unnormalise (align_corners) then clip (border)
    float ix = (u + 1.0f) * a.sx_scale, iy = (v + 1.0f) * a.sy_scale;
    ix = fminf((float)(a.W - 1), fmaxf(ix, 0.0f));
    iy = fminf((float)(a.H - 1), fmaxf(iy, 0.0f));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy, ex = 1.0f - tx, ey = 1.0f - ty;
    Tap p;
    p.w00 = ey * ex; p.w01 = ey * tx; p.w10 = ty * ex; p.w11 = ty * tx;
    const int y1 = min(y0 + 1, a.H - 1);
    if (PAIR) {                                   // 8-byte loads of (xb, xb+1), xb = min(x0, W-2)
        const int xb = min(x0, a.W - 2);
        p.sel = x0 - xb;
        p.r0 = y0 * a.W + xb; p.r1 = y1 * a.W + xb;
    } else {
        p.sel = (x0 + 1 < a.W) ? 1 : 0;
        p.r0 = y0 * a.W + x0; p.r1 = y1 * a.W + x0;
    }
    return p;
}

template <typename T> struct Pair;
template <> struct Pair<float> {
    struct __attribute__((packed, aligned(4))) U { float x, y; };     // 4-byte aligned 8-byte load
    static __device__ __forceinline__ void ld(const float* p, float& x, float& y)
    { const U v = *reinterpret_cast<const U*>(p); x = v.x; y = v.y; }
};
template <> struct Pair<__half> {
    static __device__ __forceinline__ void ld(const __half* p, float& x, float& y)
    { unsigned u; __builtin_memcpy(&u, p, 4); const __half2 h = *reinterpret_cast<const __half2*>(&u);
      x = __low2float(h); y = __high2float(h); }
};

// ATen's bilinear sum nw*w00 + ne*w01 + sw*w10 + se*w11, associated COLUMN-wise — (v00 w00 + v10 w10) + (v01 w01 + v11 w11) — so that a tap
// pair (x0, x0+1) read as one 8-byte value goes through two packed operations (v_pk_mul_f32, v_pk_fma_f32) and one add without
// any register shuffling.  EVERY equi2pers kernel (gather, LDS box, reference layout, fallback) uses this one function: same bits.
__device__ __forceinline__ float e2p_blend(float v00, float v01, float v10, float v11, float w00, float w01, float w10, float w11)
{
    return fmaf(v10, w10, v00 * w00) + fmaf(v11, w11, v01 * w01);
}

template <typename T, bool PAIR>
__device__ __forceinline__ float e2p_fetch(const T* __restrict__ img, const Tap& p)
{
    float v00, v01, v10, v11;
    if (PAIR) {
        float ax, ay, bx, by;
        Pair<T>::ld(img + p.r0, ax, ay);
        Pair<T>::ld(img + p.r1, bx, by);
        v00 = p.sel ? ay : ax; v01 = ay; v10 = p.sel ? by : bx; v11 = by;
    } else {
        v00 = Store<T>::ld(img + p.r0); v01 = Store<T>::ld(img + p.r0 + p.sel);
        v10 = Store<T>::ld(img + p.r1); v11 = Store<T>::ld(img + p.r1 + p.sel);
    }
    return e2p_blend(v00, v01, v10, v11, p.w00, p.w01, p.w10, p.w11);
}

// clamped sampling coordinates of patch sample (n, h, w): the closed-form geometry (two transcendentals per sample) followed
// by grid_sample's align_corners=True scaling and border clamp (equi2pers_v3.py:95-104,111)
__device__ __forceinline__ void e2p_sample_xy(const E2PArgs& a, int n, int h, int w, float& ix, float& iy)
{
    float lon, lat, x, q, tt, inv, u, v;
    e2p_lonlat(a, n, h, w, lon, lat, x, q, tt, inv);
    e2p_uv(lon, lat, u, v);
    ix = (u + 1.0f) * a.sx_scale; iy = (v + 1.0f) * a.sy_scale;
    ix = fminf((float)(a.W - 1), fmaxf(ix, 0.0f));
    iy = fminf((float)(a.H - 1), fmaxf(iy, 0.0f));
}

// ------------------------------------------------------------------ planar output, LDS-staged ERP footprint
// The gather kernel (e2p_planar_kernel, omni_e2p_ref.hip) is bound by the vector L1: a 64-lane gather costs ~27 tag look-ups for ~0.5 KB of
// useful data (profiles/r01a_resample_pmc.txt).  Here a block owns a 32x32 sample tile of one patch, finds the
// bounding box of the tile's bilinear footprint on the ERP (block reduction; columns measured relative to the
// tile's first sample so that a tile straddling the +-pi seam still has a narrow box), streams that box into
// LDS with fully coalesced 16-byte loads (64 useful bytes per L1 access) and takes the four taps of every
// sample from LDS (ds_read2_b32).  The box of plane p+1 is in flight in registers while plane p is computed
// (double-buffered LDS, one barrier per plane).  Tiles whose box does not fit (the pole itself lies inside, or
// the ERP row pitch is not a multiple of 4) fall back to the direct gathers — wave-uniform branch, same taps.
constexpr int E2P_BOXF = 3968;                    // floats per LDS buffer: 2 buffers + 80 B < 32 KiB -> 5 blocks / CU

// Grid: blocks [0, ntiles) own one (patch, tile) each and run the LDS path; a tile that does not fit returns at once
// and is covered by blocks [ntiles, ntiles + nfb*B): one block per (listed tile, batch item), direct gathers, so the
// few pole tiles are spread over B times more blocks instead of serialising B*C planes in one straggler.
// flags_out != nullptr: geometry-setup mode, only records which tiles need the gather path.
// BWD: the transposed operator — a.pers holds g_pers (read), a.erp g_erp (zeroed by the host, accumulated here): every tile
// accumulates its footprint box in LDS (ds_add_f32) and flushes it with coalesced global atomics, 16 bytes per lane
template <int TS, bool BWD = false>               // tile side in samples: 32 (4 samples per thread) or 16 (1)
__global__ __launch_bounds__(256) void e2p_lds_kernel(E2PArgs a, int tiles_x, int tiles_per_patch, int ntiles,
                                                      const int* __restrict__ fb, unsigned char* flags_out)
{
    // ONE __shared__ object: with a second one hipcc waits vmcnt(0) before every ds_read while an LDS-DMA is in flight
    __shared__ __attribute__((aligned(16))) float lds_all[2 * E2P_BOXF + 20];
    float (*box)[E2P_BOXF] = reinterpret_cast<float (*)[E2P_BOXF]>(lds_all);
    int (*red)[4] = reinterpret_cast<int (*)[4]>(lds_all + 2 * E2P_BOXF);
    int& sh_xc = *reinterpret_cast<int*>(lds_all + 2 * E2P_BOXF + 16);
    const bool fb_block = (int)blockIdx.x >= ntiles;
    int fb_b = 0;
    unsigned lb;
    if (fb_block) { const int idx = blockIdx.x - ntiles; lb = fb[idx / a.B]; fb_b = idx % a.B; }
    else lb = omni_xcd_remap(blockIdx.x, ntiles);
    const int n = lb / tiles_per_patch;
    const int tile = lb % tiles_per_patch;
    constexpr int SPT = TS * TS / 256, RSTEP = 256 / TS;        // samples per thread, row step between them
    const int th0 = (tile / tiles_x) * TS, tw0 = (tile % tiles_x) * TS;
    const int t = threadIdx.x, wave = t >> 6;
    const int col = t % TS, rowb = t / TS;
    const int W = a.W, H = a.H;

    // ---- taps of this thread's 4 samples (rows rowb + 8k of the tile, column col)
    int x0[SPT], y0[SPT], y1[SPT], s1[SPT];
    float w00[SPT], w01[SPT], w10[SPT], w11[SPT];
    const int w = min(tw0 + col, a.pw - 1);
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int h = min(th0 + rowb + RSTEP * k, a.ph - 1);
        float ix, iy;
        if (a.ixy) {                                     // configuration constant: evaluated once per geometry handle by the
            const float2 c = a.ixy[((size_t)n * a.ph + h) * a.pw + w];   // same device function (bit-identical), 8 bytes per sample
            ix = c.x; iy = c.y;
        } else {
            e2p_sample_xy(a, n, h, w, ix, iy);
        }
        const float fx = floorf(ix), fy = floorf(iy);
        x0[k] = (int)fx; y0[k] = (int)fy;
        const float tx = ix - fx, ty = iy - fy, ex = 1.0f - tx, ey = 1.0f - ty;
        w00[k] = ey * ex; w01[k] = ey * tx; w10[k] = ty * ex; w11[k] = ty * tx;
        y1[k] = min(y0[k] + 1, H - 1);
        s1[k] = (x0[k] + 1 < W) ? 1 : 0;          // +1 column outside: alias onto x0 (its weight is exactly 0)
    }
    // ---- footprint box: rows [ymin, ymax], columns relative to the tile's first sample (seam-safe)
    if (t == 0) sh_xc = x0[0];
    __syncthreads();
    const int xc = sh_xc, half = W >> 1;
    int dx[SPT];
    int ymin = y0[0], ymax = y1[0];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        int d = x0[k] - xc;
        if (d >= half) d -= W;
        if (d < -half) d += W;
        dx[k] = d;
        ymin = min(ymin, y0[k]); ymax = max(ymax, y1[k]);
    }
    int dmin = dx[0], dmax = dx[0];
#pragma unroll
    for (int k = 1; k < SPT; ++k) { dmin = min(dmin, dx[k]); dmax = max(dmax, dx[k]); }
    ymin = wave_min(ymin); ymax = wave_max(ymax); dmin = wave_min(dmin); dmax = wave_max(dmax);
    if ((t & 63) == 0) { red[wave][0] = ymin; red[wave][1] = ymax; red[wave][2] = dmin; red[wave][3] = dmax; }
    __syncthreads();
    ymin = min(min(red[0][0], red[1][0]), min(red[2][0], red[3][0]));
    ymax = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    dmin = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
    dmax = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
    int xs = xc + dmin;                             // absolute first column of the box (may wrap)
    if (xs < 0) xs += W;
    if (xs >= W) xs -= W;
    const int xs4 = xs & ~3, shift = xs - xs4;
    int bw = (dmax - dmin + 2 + shift + 3) & ~3;             // columns x0..x0+1 of every sample, whole 16-byte chunks
    if (((bw >> 2) & 1) == 0) bw += 4;                       // odd number of 16-byte chunks per row: consecutive box rows start
                                                             // 4, 12, 20, 28 banks apart (polar patches walk the box by rows)
    const int bh = ymax - ymin + 1;
    const int bw4 = bw >> 2, nchunk = bh * bw4;
    const bool fits = ((W & 3) == 0) && (bw <= W) && (bh * bw <= E2P_BOXF);
    const bool full = (th0 + TS <= a.ph) && (tw0 + TS <= a.pw);

    const float* erp = (const float*)a.erp;
    const int plane = a.ph * a.pw;
    const size_t img_plane = (size_t)H * W;
    const size_t out_bstride = (size_t)a.tab.N * a.C * plane;
    // this thread's 4 output elements: e0 + 8k rows
    float* out = (float*)a.pers + (size_t)n * a.C * plane + (size_t)(th0 + rowb) * a.pw + (tw0 + col);
    const int ostep = RSTEP * a.pw;

    if (flags_out) { if (t == 0) flags_out[lb] = (fits && full) ? 0 : 1; return; }
    if (!fb_block && !(fits && full)) return;          // covered by the fallback blocks of this launch
    if (OMNI_DBG(a, 4) && fb_block) return;
    if (OMNI_DBG(a, 8) && !fb_block) return;
    if (fb_block && blockIdx.y > 0) return;            // the fallback blocks walk every plane themselves
    if (!fb_block) {
        int r0[SPT], r1[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int c0 = dx[k] - dmin + shift;
            r0[k] = (y0[k] - ymin) * bw + c0;
            r1[k] = (y1[k] - ymin) * bw + c0;
        }
        // Plane loop for a box of NJ x 256 16-byte chunks at most (NJ is block-uniform).  Threads past the
        // last chunk re-load / re-store the last chunk (identical data, same address): no exec masking.
        // Box fill by LDS-DMA (global_load_lds_dwordx4): a wave's 64 lanes deposit 64 consecutive 16-byte chunks
        // straight into the box (the chunk order IS the LDS order), no VGPR staging and no ds_write issue slots.
        // The DMA of plane p+1 is in flight behind the gathers of plane p; one barrier per plane.  The loop is kept
        // free of per-lane conditions: the scalar unit is shared by the whole CU and ~100 scalar instructions per wave
        // and plane (exec-mask juggling, 64-bit pointer updates) were costing as much as the gathers themselves.
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int lane = t & 63;
        const int nj = (nchunk + 255) >> 8;                          // block-uniform number of chunk columns (1..4)
        int goff[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int qc = min(wave * 64 + 256 * j + lane, nchunk - 1);   // lanes past the end re-fetch the last chunk ...
            const int r = qc / bw4, cx = qc - r * bw4;
            int gx = xs4 + 4 * cx;
            if (gx >= W) gx -= W;
            goff[j] = (ymin + r) * W + gx;
        }
        // ... into their own (unused) slot, which must still lie inside the buffer: slots = E2P_BOXF/4 = 992 < 1024
        const bool tail_ok = (wave * 64 + 256 * 3 + lane) < E2P_BOXF / 4;
        auto dma = [&](const float* img, float* buf) {
            __builtin_amdgcn_global_load_lds((gptr_t)(img + goff[0]), (lptr_t)(buf + (wave * 64) * 4), 16, 0, 0);
            if (nj > 1) __builtin_amdgcn_global_load_lds((gptr_t)(img + goff[1]), (lptr_t)(buf + (wave * 64 + 256) * 4), 16, 0, 0);
            if (nj > 2) __builtin_amdgcn_global_load_lds((gptr_t)(img + goff[2]), (lptr_t)(buf + (wave * 64 + 512) * 4), 16, 0, 0);
            if (nj > 3 && tail_ok) __builtin_amdgcn_global_load_lds((gptr_t)(img + goff[3]), (lptr_t)(buf + (wave * 64 + 768) * 4), 16, 0, 0);
        };
        float* const box0 = &box[0][0];
        if (BWD) {
            // ---- transposed trip per plane: zero my chunks | barrier | 4 x 4 ds_add_f32 | barrier | flush my chunks (global atomics)
            float* gerp = (float*)a.erp;
            const float* src = (const float*)a.pers + (size_t)n * a.C * plane + (size_t)(th0 + rowb) * a.pw + (tw0 + col);
            const size_t bskip = out_bstride - (size_t)a.C * plane;
            int cc = 0;
            const int planes = a.B * a.C;
            const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int p = 0; p < planes; ++p) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int qc = wave * 64 + 256 * j + lane;
                    if (j < nj && qc < nchunk) *reinterpret_cast<float4*>(box0 + qc * 4) = zero4;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    const float g = src[k * ostep];
                    atomicAdd(box0 + r0[k], g * w00[k]);
                    atomicAdd(box0 + r0[k] + s1[k], g * w01[k]);          // s1 == 0: the +1 column is outside and its weight exactly 0
                    atomicAdd(box0 + r1[k], g * w10[k]);
                    atomicAdd(box0 + r1[k] + s1[k], g * w11[k]);
                }
                __syncthreads();
                float* ge = gerp + (size_t)p * img_plane;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int qc = wave * 64 + 256 * j + lane;
                    if (j < nj && qc < nchunk) {
                        const float4 v = *reinterpret_cast<const float4*>(box0 + qc * 4);
                        float* q = ge + goff[j];
                        if (v.x != 0.0f) atomicAdd(q, v.x);
                        if (v.y != 0.0f) atomicAdd(q + 1, v.y);
                        if (v.z != 0.0f) atomicAdd(q + 2, v.z);
                        if (v.w != 0.0f) atomicAdd(q + 3, v.w);
                    }
                }
                src += plane;
                if (++cc == a.C) { cc = 0; src += bskip; }
            }
            return;
        }
        // blockIdx.y owns a contiguous range of the B*C image planes (small launches — few tiles, e.g. 18 patches of
        // 128^2 — are split over the planes so that the chip is filled; the geometry prologue is repeated per range)
        const int planes_all = a.B * a.C;
        const int per = (planes_all + (int)gridDim.y - 1) / (int)gridDim.y;
        const int p_begin = (int)blockIdx.y * per, planes = min(planes_all, p_begin + per);
        if (p_begin >= planes) return;
        const float* img = erp + (size_t)p_begin * img_plane;
        dma(img, box0 + (p_begin & 1) * E2P_BOXF);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float* dst = out + (size_t)(p_begin / a.C) * out_bstride + (size_t)(p_begin % a.C) * plane;
        const size_t bskip = out_bstride - (size_t)a.C * plane;
        int cc = p_begin % a.C;
        for (int p = p_begin; p < planes; ++p) {
            const float* cur = box0 + (p & 1) * E2P_BOXF;
            if (p + 1 < planes) { img += img_plane; dma(img, box0 + ((p + 1) & 1) * E2P_BOXF); }
            float r[SPT];
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const float a0 = cur[r0[k]], a1 = cur[r0[k] + 1];              // one ds_read2_b32 per tap row
                const float b0 = cur[r1[k]], b1 = cur[r1[k] + 1];
                r[k] = e2p_blend(a0, s1[k] ? a1 : a0, b0, s1[k] ? b1 : b0, w00[k], w01[k], w10[k], w11[k]);
            }
#pragma unroll
            for (int k = 0; k < SPT; ++k) dst[k * ostep] = r[k];
            dst += plane;
            if (++cc == a.C) { cc = 0; dst += bskip; }
            // counted wait: the DMA pieces are older than this trip's 4 stores, which may stay in flight across the
            // barrier (a plain __syncthreads() would drain them: its fence waits vmcnt(0) while an LDS-DMA is pending)
            if (SPT == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
            else          asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    } else {
        // direct gathers (same taps): tiles containing a pole, ragged tiles, odd row pitch
        bool ok[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) ok[k] = (th0 + rowb + RSTEP * k < a.ph) && (tw0 + col < a.pw);
        if (BWD) {                                                // direct global atomics for this (tile, batch item)
            float* gerp = (float*)a.erp;
            const float* srcb = (const float*)a.pers + (size_t)n * a.C * plane + (size_t)(th0 + rowb) * a.pw + (tw0 + col)
                              + (size_t)fb_b * out_bstride;
            for (int c = 0; c < a.C; ++c) {
                float* ge = gerp + ((size_t)fb_b * a.C + c) * img_plane;
#pragma unroll
                for (int k = 0; k < SPT; ++k) {
                    if (!ok[k] || !(w00[k] == w00[k])) continue;              // outside a ragged tile (the weights of the q4 sample are finite: its clipped row coordinate is 0)
                    const float g = srcb[(size_t)c * plane + k * ostep];
                    const int g0 = y0[k] * W + x0[k], g1 = y1[k] * W + x0[k];
                    atomicAdd(ge + g0, g * w00[k]); atomicAdd(ge + g0 + s1[k], g * w01[k]);
                    atomicAdd(ge + g1, g * w10[k]); atomicAdd(ge + g1 + s1[k], g * w11[k]);
                }
            }
            return;
        }
        float* dstb = out + (size_t)fb_b * out_bstride;
        for (int c = 0; c < a.C; ++c) {
            const float* img = erp + ((size_t)fb_b * a.C + c) * img_plane;
            float* dst = dstb + (size_t)c * plane;
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int g0 = y0[k] * W + x0[k], g1 = y1[k] * W + x0[k];
                const float v00 = img[g0], v01 = img[g0 + s1[k]], v10 = img[g1], v11 = img[g1 + s1[k]];
                const float r = e2p_blend(v00, v01, v10, v11, w00[k], w01[k], w10[k], w11[k]);
                if (ok[k]) dst[k * ostep] = r;
            }
        }
    }
}

// ------------------------------------------------------------------ one wave per small sample tile: what e2p_box_kernel (omni_equi2pers.hip),
// e2p_ref_kernel (omni_e2p_ref.hip) and the box-table builder e2b_tiles_kernel (omni_e2p_tables.hip) share
constexpr int E2B_NPX = 4;                      // samples per lane of the 8 x 32 tile (the kernels take NPX = 4 | 2 as a template parameter: 8 x 32 | 4 x 32 samples)
constexpr int E2B_NJMAX = 8;                    // 1-KiB DMA pieces per box at most
constexpr int E2B_RING_KB = 12;                 // LDS ring per wave (13 waves per CU by LDS; NJ <= 3: 4 slots, <= 6: 2 slots, else 1)

typedef __amdgpu_buffer_rsrc_t e2b_rsrc_t;
typedef __attribute__((address_space(3))) void* e2b_lptr_t;
__device__ __forceinline__ void e2b_dma16(e2b_rsrc_t rs, unsigned char* lds, unsigned voff, unsigned soff)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (e2b_lptr_t)lds, 16, (int)voff, (int)soff, 0, 0);
}
template <int N> __device__ __forceinline__ void e2b_wait_vm()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <typename T> struct E2BPair;
template <> struct E2BPair<float> {
    static __device__ __forceinline__ void ld(const unsigned char* b, int o, float& x, float& y)
    { const float* p = reinterpret_cast<const float*>(b) + o; x = p[0]; y = p[1]; }
};
template <> struct E2BPair<__half> {
    static __device__ __forceinline__ void ld(const unsigned char* b, int o, float& x, float& y)
    {   // halfs o, o+1: one ds_read2_b32 of the two 32-bit words around them + a byte-align
        const unsigned* p = reinterpret_cast<const unsigned*>(b) + (o >> 1);
        const unsigned w0 = p[0], w1 = p[1];
        const unsigned v = (o & 1) ? __builtin_amdgcn_alignbyte(w1, w0, 2u) : w0;
        const __half2 h = *reinterpret_cast<const __half2*>(&v);
        x = __low2float(h); y = __high2float(h);
    }
};

// clamped sampling coordinate of sample (n, h, w): from the per-geometry table, or evaluated on the fly (same function, same bits)
__device__ __forceinline__ void e2b_xy(const E2PArgs& a, int n, int h, int w, float& ix, float& iy)
{
    if (a.ixy) { const float2 c = a.ixy[((size_t)n * a.ph + h) * a.pw + w]; ix = c.x; iy = c.y; }
    else e2p_sample_xy(a, n, h, w, ix, iy);
}

// table entry of one tile: x = bw4 | bh << 12 | fits << 31 (bw4 = 16-byte chunks per box row, bh = box rows),
//                          y = xs4 | ymin << 16 (first box column, chunk-aligned, the box wraps at the seam; first box row)
// the tile is E2B_TH = 8 rows x E2B_TW = 32 columns of samples, 4 per lane; every lane stores 4 adjacent samples of ONE row: one 16-byte
// (fp16: 8-byte) store per lane and plane.  Two lane -> sample maps (e2p_box_kernel's ROWMAP); for the second one the 4x4 block (4 rows x 4
// columns) held by each quad of lanes is transposed with DPP moves before the store.
constexpr int E2B_TW = 32;                       // (tile height: 2 NPX = 8 or 4 sample rows, a template parameter)

__device__ __forceinline__ float e2b_dpp_xor1(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ float e2b_dpp_xor2(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); }   // quad_perm [2,3,0,1]
// r[k] of lane i (i = lane % 4)  ->  r[k] = what lane k of the quad held in r[i]
__device__ __forceinline__ void e2b_quad_transpose(float (&r)[4], int lane)
{
    const bool o1 = lane & 1, o2 = lane & 2;
#pragma unroll
    for (int q = 0; q < 2; ++q) {                                  // 2x2 blocks: exchange M[2p][2q+1] <-> M[2p+1][2q]
        const float y = e2b_dpp_xor1(o1 ? r[2 * q] : r[2 * q + 1]);
        r[2 * q + 1] = o1 ? r[2 * q + 1] : y;
        r[2 * q] = o1 ? y : r[2 * q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {                                  // off-diagonal 2x2 blocks: M[p][q+2] <-> M[p+2][q]
        const float y = e2b_dpp_xor2(o2 ? r[q] : r[q + 2]);
        r[q + 2] = o2 ? r[q + 2] : y;
        r[q] = o2 ? y : r[q];
    }
}

// the 4 x 32 tile (NPX = 2): lane l holds (row l/32, column l%32) and (row l/32 + 2, same column); after the exchange with lane l ^ 1 an even lane
// holds its first row's columns (c, c+1), an odd lane its second row's columns (c-1, c): two adjacent samples of one row per lane
__device__ __forceinline__ void e2b_pair_transpose(float (&r)[2], int lane)
{
    const bool odd = lane & 1;
    const float y = e2b_dpp_xor1(odd ? r[0] : r[1]);
    r[0] = odd ? y : r[0];
    r[1] = odd ? r[1] : y;
}
__device__ __forceinline__ void e2b_transpose(float (&r)[4], int lane) { e2b_quad_transpose(r, lane); }
__device__ __forceinline__ void e2b_transpose(float (&r)[2], int lane) { e2b_pair_transpose(r, lane); }

void fill_args(E2PArgs& a, const omni_geometry* g, const void* erp, void* pers, int B, int C)
{
    a.erp = erp; a.pers = pers; a.B = B; a.C = C; a.H = g->H; a.W = g->W; a.ph = g->ph; a.pw = g->pw;
    a.fovx = g->fov_w / 360.0f; a.fovy = g->fov_h / 180.0f;
    a.stepx = g->pw > 1 ? 1.0f / (float)(g->pw - 1) : 0.0f;
    a.stepy = g->ph > 1 ? 1.0f / (float)(g->ph - 1) : 0.0f;
    a.sx_scale = (float)(g->W - 1) / 2.0f; a.sy_scale = (float)(g->H - 1) / 2.0f;
    a.tab = g->e2p;
    a.ixy = g->e2p_ixy;
    a.dbg = 0; a.trace = nullptr;
    a.store_mode = omni_options().e2p_store;
#ifdef OMNI_DEBUG_BUILD
    a.dbg_skip_fb = omni_options().e2p_ref_lds == 2;     // (a RESULT-changing timing experiment: the debug build only, like every OMNI_*_DBG bit)
#else
    a.dbg_skip_fb = 0;
#endif
#ifdef OMNI_DEBUG_BUILD
    a.dbg = omni_debug_bits("OMNI_E2P_DBG");
    a.trace = omni_debug_trace_buf();
#endif
}

}  // namespace

// ---- host launchers that cross units (launch_e2p, omni_equi2pers.hip, chooses; the kernels live where they are launched)
int omni_e2p_launch_lds(const omni_geometry* g, const void* erp, void* pers, int B, int C, hipStream_t stream);                  // omni_e2p_tables.hip: e2p_lds_kernel, fp32, layout BNCHW
int omni_e2p_launch_planar(const omni_geometry* g, const void* erp, void* pers, int dtype, int B, int C, hipStream_t stream);    // omni_e2p_ref.hip: e2p_planar_kernel, layout BNCHW
int omni_e2p_launch_ref(const omni_geometry* g, const void* erp, void* pers, int dtype, int B, int C, hipStream_t stream);       // omni_e2p_ref.hip: e2p_ref_kernel / e2p_reflayout_kernel, layout BCHWN
