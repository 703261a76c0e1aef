// omni_up2_tapsum.h — the SEPARABLE TAP SUM that the tap-product kernels share: up2_taps_fused_kernel (omni_conv_up2_taps.hip) and up2_heads_taps_kernel
// (omni_conv_up2_heads_taps.hip).  Device side, forceinline helpers only; tests/test_up2_taps_sep_cpu.py is the specification of this header.
//
// Both kernels compute conv3x3(upsample2x(x)) as nine 1x1 tap products Y_t = W_t . x on the low-resolution map (t = ky*3 + kx) and owe
//   out[q] = sum_t [q + t - 1 inside the up-sampled map] * up2(Y_t)[q + t - 1].
// A tap's fp32 products are parked in an LDS CHUNK, [pixel][32 channels] = 128 B per pixel, the eight 16-byte channel quads of a pixel permuted with
// (pixel >> 1) & 3 (tapsum_park, tapsum_col_off: every read below touches distinct bank groups).  A thread = (low-res column j, channel quad) owns ROWS
// low-resolution rows i: ROWS 2 x 2 output cells (rows 2i, 2i + 1 x columns 2j, 2j + 1) x 4 channels.
// The sum is separable, because both the up-sampling and the tap shift are.  Taps are taken kx-major (tap_at: 0, 3, 6, 1, 4, 7, 2, 5, 8).  Per tap a VERTICAL
// stage on the thread's own column,
//   S[it][ay] (+)= hy[ay + ky] * Y[row i - 1 + r] + ly[ay + ky] * Y[row i + r],               r = (ay + ky) >> 1
// (the column's ROWS + 1 / ROWS + 2 / ROWS + 1 rows are read once per tap); after the three ky taps of a kx a HORIZONTAL stage,
//   out[it][ay][bx] (+)= hx[bx + kx] * S[column j - 1 + c] + lx[bx + kx] * S[column j + c],    c = (bx + kx) >> 1,
// whose neighbour columns live in other threads and come through the chunks, in the chunks' own layout (tapsum_put).  15 FMAs per output element instead of
// the 36 of a tap-by-tap bilinear sum.
// Weights and clamps of up2_tapsum_sh_kernel (omni_net.hip), NOT its order of summation: the same bilinear weights (0.25 / 0.75 are exact, so the tables
// below hold the values its index arithmetic yields), source rows / columns clamped to the map.  A tap outside the up-sampled map gets weight zero instead
// of being skipped.  Every sum is an explicit fmaf in a fixed order: the helpers fix output bits.
// What stays with a kernel: its weight gather, its fragments and who owns them, the barriers around the stages and which chunk receives which ay half.
#pragma once
#include "omni_conv_sh_common.h"

namespace {

// the tap (ky * 3 + kx) processed at step s: kx-major, 0, 3, 6, 1, 4, 7, 2, 5, 8 — the three taps of a column kx follow each other
__host__ __device__ constexpr int tap_at(int s) { return 3 * (s % 3) + s / 3; }

// byte offset of column col in a chunk row, channel quad `quad` (chunk pieces are permuted with (pixel >> 1) & 3; a row starts at an even pixel)
__device__ __forceinline__ int tapsum_col_off(int col, int quad) { return col * 128 + ((quad ^ ((col >> 1) & 3)) * 16); }

// bilinear weights of up-sampled column 2j + u - 1, u = 0 .. 3, on the column pair (c, c + 1), c = u >> 1: (1 - l, l) with l = frac(max(0.5 (p + 0.5) - 0.5, 0)),
// zero where the column is outside the map of WL columns
template <int WL> __device__ __forceinline__ void tapsum_col_weights(int j, float (&hx)[4], float (&lx)[4])
{
    hx[0] = j > 0 ? 0.75f : 0.0f;      lx[0] = j > 0 ? 0.25f : 0.0f;
    hx[1] = j > 0 ? 0.25f : 1.0f;      lx[1] = j > 0 ? 0.75f : 0.0f;
    hx[2] = 0.75f;                     lx[2] = 0.25f;
    hx[3] = j < WL - 1 ? 0.25f : 0.0f; lx[3] = j < WL - 1 ? 0.75f : 0.0f;
}

// the same for the rows of a thread: only its first row can be the map's top (hy0 / ly0[u], u = 0 .. 3), only its last the map's bottom (hyl / lyl: u = 3);
// every other row has the interior weights
struct TapsumRowW { float hy0[4], ly0[4], hyl, lyl; };
__device__ __forceinline__ TapsumRowW tapsum_row_weights(bool top, bool bot)
{
    return {{top ? 0.0f : 0.75f, top ? 1.0f : 0.25f, 0.75f, 0.25f}, {top ? 0.0f : 0.25f, top ? 0.0f : 0.75f, 0.25f, 0.75f}, bot ? 0.0f : 0.25f, bot ? 0.0f : 0.75f};
}

// One fragment's f16x3 products -> chunk: channels 8q + 4h .. + 3 (h = lane >> 5) of the lane's pixel px.  cp = chunk + px * 128, sw = (px >> 1) & 3 (formed by
// the caller, beside its fragment index: up2_heads_taps_kernel has no register to spare for a second copy)
__device__ __forceinline__ void tapsum_park(const f16v& acc1, const f16v& acc, unsigned char* cp, int sw, int h)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f4v v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc_join<false>(acc1[4 * q + e], acc[4 * q + e]);
        *reinterpret_cast<f4v*>(cp + (((2 * q + h) ^ sw) * 16)) = v;
    }
}

// Vertical stage of tap (KY, kx): S (+)= the tap, on the thread's own column (coff1 = tapsum_col_off(j, quad)).  The column is read once: image rows
// i0 - 1 + k, k = 0 .. ROWS + 1 (i0: the thread's first row; KY = 0 / 2 leave the last / first one out), clamped to the map of Hl rows; sbase = image row of
// the chunk's row 0.  Up-sampled row 2i + ay + KY - 1 takes the row pair (it + r, it + r + 1), r = (ay + KY) >> 1.  The first tap of a column group starts S.
template <int ROWS, int KY, int ROW_BYTES>
__device__ __forceinline__ void tapsum_vertical(f4v (&S)[ROWS][2], const unsigned char* chunk, int i0, int sbase, int Hl, int coff1, const TapsumRowW& w)
{
    constexpr int klo = KY >> 1, khi = ROWS + ((KY + 1) >> 1);
    f4v R[ROWS + 2];
#pragma unroll
    for (int k = klo; k <= khi; ++k)
        R[k] = *reinterpret_cast<const f4v*>(chunk + (min(max(i0 - 1 + k, 0), Hl - 1) - sbase) * ROW_BYTES + coff1);
#pragma unroll
    for (int it = 0; it < ROWS; ++it)
#pragma unroll
        for (int ay = 0; ay < 2; ++ay) {
            const int uy = ay + KY, r = uy >> 1;
            // weights of up-sampled row 2i + uy - 1 (the rows between a thread's first and last are never the map's edge)
            const float h = it == 0 ? w.hy0[uy] : it == ROWS - 1 && uy == 3 ? w.hyl : (uy & 1) ? 0.25f : 0.75f;
            const float l = it == 0 ? w.ly0[uy] : it == ROWS - 1 && uy == 3 ? w.lyl : (uy & 1) ? 0.75f : 0.25f;
            f4v v;
            if constexpr (KY != 0) v = S[it][ay];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if constexpr (KY == 0) v[e] = fmaf(l, R[it + r + 1][e], h * R[it + r][e]);
                else v[e] = fmaf(l, R[it + r + 1][e], fmaf(h, R[it + r][e], v[e]));
            asm volatile("" : "+v"(v));                           // pins the sum HERE: the compiler otherwise sinks the arithmetic below later barriers
            S[it][ay] = v;                                        // and spills everything it read from the chunks meanwhile
        }
    __builtin_amdgcn_sched_barrier(0);                            // one tap's column in flight at a time
}

// The thread's vertical sums of half AY -> buf, for its neighbours' horizontal stage: chunk rows rb + it, the thread's own column (one half is 32 KiB)
template <int ROWS, int AY, int ROW_BYTES>
__device__ __forceinline__ void tapsum_put(const f4v (&S)[ROWS][2], unsigned char* buf, int rb, int coff1)
{
#pragma unroll
    for (int it = 0; it < ROWS; ++it) *reinterpret_cast<f4v*>(buf + (rb + it) * ROW_BYTES + coff1) = S[it][AY];
}

// Horizontal stage of column group KX, half AY: out (+)= hx * S[column j - 1 + c] + lx * S[column j + c], c = (bx + KX) >> 1.  The neighbour columns' S are
// read from buf where tapsum_put left them (coffl / coffr = tapsum_col_off of columns max(j - 1, 0) / min(j + 1, WL - 1): conflict-free like the product
// reads); hx / lx = tapsum_col_weights(j).  The first column group starts out.
template <int ROWS, int KX, int AY, int ROW_BYTES>
__device__ __forceinline__ void tapsum_horizontal(f4v (&out)[ROWS][2][2], const f4v (&S)[ROWS][2], const unsigned char* buf, int rb, int coffl, int coffr,
                                                  const float (&hx)[4], const float (&lx)[4])
{
#pragma unroll
    for (int it = 0; it < ROWS; ++it) {
        const unsigned char* rp = buf + (rb + it) * ROW_BYTES;
        const f4v own = S[it][AY];
        f4v left = own, right = own;                              // (only the live one is read: KX = 0 never looks right, KX = 2 never left)
        if (KX <= 1) left = *reinterpret_cast<const f4v*>(rp + coffl);
        if (KX >= 1) right = *reinterpret_cast<const f4v*>(rp + coffr);
#pragma unroll
        for (int bx = 0; bx < 2; ++bx) {
            const int ux = bx + KX, c = ux >> 1;
            const f4v va = c == 0 ? left : own, vb = c == 0 ? own : right;
            f4v o;
            if constexpr (KX != 0) o = out[it][AY][bx];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if constexpr (KX == 0) o[e] = fmaf(lx[ux], vb[e], hx[ux] * va[e]);
                else o[e] = fmaf(lx[ux], vb[e], fmaf(hx[ux], va[e], o[e]));
            asm volatile("" : "+v"(o));                           // (pinned like the vertical sums)
            out[it][AY][bx] = o;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

}  // namespace
