// omni_conv_up2_taps.hip — up2_taps_fused_kernel, up2_taps_walk_kernel (the same sums on eight waves and persistent blocks, further down; option
// conv_up2_taps_walk) and their entry point omni_conv3x3_up2_taps_sh_f16x3: conv3x3(upsample2x(x)) of the 64 -> 64 decoder stages
// (de_conv3_0, de_conv2_0) as nine 1x1 TAP PRODUCTS on the low-resolution map, summed through LDS.  Both operators are linear, so
//   out[q] = bias + sum_t [q + t - 1 inside the 2Hl x 2Wl map] * up2(W_t . x)[q + t - 1]                       (t = ky*3 + kx)
// — a quarter of the matrix instructions of the up-sampling halo kernel (conv3x3_halo_sh_kernel<64, 4, true, 0>), which convolves at full resolution.  The
// two-launch form of the identity (omni_conv2d_sh_f16x3_ws on the tap-major weights + omni_up2_tapsum_sh, Engine.taps_first) moves the fp32 tap products
// through memory: 340 MB for de_conv3_0 at 144 patches.  Here they never leave the CU.
//
// A block owns ROWS low-resolution rows of one image at full width (WL) — 8 rows + one halo row each side at WL = 32 ("bands": 320 pixels; left and right
// need no halo, the clamp of the up-sampling addresses the same column), or a whole 16 x 16 image (256 pixels, no halo) — and 32 output channels:
//   * the block's nine taps of weights (9 x 32 rows x 256 B = 72 KiB, tap-major f16x3 rows as `<key>.taps.w16`) go to LDS by LDS-DMA, once, in processing order;
//     tap t is waited for just before its products (hand-counted s_waitcnt vmcnt);
//   * a wave keeps the SH fragments of its pixels (32-pixel fragments w, w + 4, w + 8; K = 64: hi and lo of four 16-channel chunks) in registers for all nine taps;
//   * per tap: 12 matrix instructions per fragment (the f16x3 three-term product, acc_join) -> the fp32 products of the tap, [pixel][32 channels], parked in
//     one of two LDS chunks (40 KiB) -> ONE barrier -> every thread takes the tap into its sums: thread = (low-res column j, channel quad),
//     eight 2 x 2 output cells (rows 2i, 2i+1 x columns 2j, 2j+1 for eight rows i) x 4 channels = 128 registers;
//   * the tap sum is the SEPARABLE one of omni_up2_tapsum.h (tap order, chunk layout, weight tables, vertical and horizontal stage: all there), ROWS = 8: 64
//     registers for the vertical sums, the column's 9 / 10 / 9 rows read once per tap, two more barriers per kx around the horizontal stage;
//   * outputs leave through act_store4<true> (saturation, sticky range flag).
// Fixed order, no atomics, no dependence on block placement: an image's bits do not depend on M.
// LDS: 72 KiB + 2 x 40 KiB = 152 KiB, one block of four waves per CU with up to 512 registers per lane.
#include <stdint.h>
#include <algorithm>
#include "omni_up2_tapsum.h"

namespace {

struct TapsArgs {
    const void* src;                         // SH [M, Hl, Wl, 64]
    const void* wt;                          // halfs [9 * Cout][2][hi32|lo32], row t*Cout + co
    const float* bias;                       // [Cout] or null
    void* dst;                               // SH [M, 2Hl, 2Wl, Cout]
    int M, Hl, Cout, act;
};

constexpr int TAP_BYTES = 32 * 256;          // one tap of a block's weights: 32 output channels x (2 groups x 128 B)

// s_waitcnt vmcnt(n) for the even counts the tap loop needs (n is a constant after unrolling)
__device__ __forceinline__ void wait_taps_in_flight(int n)
{
    if (n >= 16) wait_vm<16>();
    else if (n == 14) wait_vm<14>();
    else if (n == 12) wait_vm<12>();
    else if (n == 10) wait_vm<10>();
    else if (n == 8) wait_vm<8>();
    else if (n == 6) wait_vm<6>();
    else if (n == 4) wait_vm<4>();
    else if (n == 2) wait_vm<2>();
    else wait_vm<0>();
}

template <int WL, int ROWS, int HALO>
__global__ __launch_bounds__(256, 1) void up2_taps_fused_kernel(TapsArgs a)
{
    static_assert((WL == 32 && ROWS == 8 && HALO == 1) || (WL == 16 && ROWS == 16 && HALO == 0), "bands of 8 rows of 32-wide maps, or whole 16 x 16 maps");
    constexpr int SROWS = ROWS + 2 * HALO, P = SROWS * WL, NF = P / 32, NFW = (NF + 3) / 4;
    constexpr int W_BYTES = 9 * TAP_BYTES, CH_BYTES = P * 128, ROW_BYTES = WL * 128;
    static_assert(P % 32 == 0 && ROWS * WL == 256, "whole fragments; one (column, channel quad) thread per eight rows");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[W_BYTES + 2 * CH_BYTES];
    static_assert(sizeof(lds) <= 160 * 1024, "one block per CU");

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    const int ntn = a.Cout >> 5, nb = a.Hl / ROWS;
    int bid = blockIdx.x;
    const int tile_n = bid % ntn; bid /= ntn;
    const int band = bid % nb; const int m = bid / nb;
    const int r0 = band * ROWS, col0 = tile_n * 32, sbase = r0 - HALO;       // sbase: image row of LDS slot row 0
    const int Hl = a.Hl;

    // The wave's fragments w, w + 4, w + 8.  Ten fragments on four waves: waves 2 and 3 repeat their fragment w + 4 (the same values to the same addresses) while
    // waves 0 and 1 do fragments 8 and 9 — they would wait at the barrier for as long, and the kernel stays ONE basic block: with a branch here the compiler sinks
    // the whole tap sum below the last tap and keeps every value it read from the chunks alive until then (4.5 KB of scratch).
    auto frag = [&](int fi) { const int f = wave + 4 * fi; return f < NF ? f : wave + 4; };
    // ---- the wave's pixel fragments: fragment f = slot pixels 32 f .. 32 f + 31, lane -> pixel lane & 31, 16-byte piece lane >> 5 of every 16-channel chunk
    h8v xh[NFW][4], xl[NFW][4];
#pragma unroll
    for (int fi = 0; fi < NFW; ++fi) {
        const int f = frag(fi);
        {
            const int p = f * 32 + (lane & 31), sr = p / WL, cx = p - sr * WL;
            const int row = min(max(sbase + sr, 0), Hl - 1);     // (the halo row above the first / below the last band is never read by the tap sum)
            const unsigned char* sp = (const unsigned char*)a.src + ((size_t)(m * Hl + row) * WL + cx) * 256 + (lane >> 5) * 16;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                xh[fi][kc] = *reinterpret_cast<const h8v*>(sp + (kc >> 1) * 128 + (kc & 1) * 32);
                xl[fi][kc] = *reinterpret_cast<const h8v*>(sp + (kc >> 1) * 128 + 64 + (kc & 1) * 32);
            }
        }
    }
    // ---- all nine taps of weights, two DMA instructions per wave and tap.  An instruction deposits four 256-byte rows; the 16 pieces of row r are permuted
    // with r & 15 (slot s holds piece s ^ (r & 15)): the fragment reads below (32 rows, one piece each) then touch 16 distinct 16-byte bank groups
    {
        const rsrc_t rsw = make_rsrc(a.wt, (size_t)9 * a.Cout * 256);
#pragma unroll
        for (int s = 0; s < 9; ++s) {                             // in processing order (kx-major); tap tp keeps its place tp * TAP_BYTES
            const int tp = tap_at(s);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = wave + 4 * k, row = 4 * i + (lane >> 4), piece = (lane & 15) ^ (row & 15);
                dma16(rsw, lds + tp * TAP_BYTES + i * 1024, ((tp * a.Cout + col0 + row) * 16 + piece) * 16, 0);
            }
        }
    }
    // weight fragment of row lane & 31: piece K | h (K = 8 group + 4 lo + 2 chunk, h = lane >> 5) sits in slot (K | h) ^ (row & 15) = K ^ (h ^ (row & 15))
    const int wfo = (lane & 31) * 256 + (((lane >> 5) ^ (lane & 15)) * 16);

    // ---- tap sum geometry: thread = (low-res column j, channel quad), rows i = r0 + ib + it, it = 0 .. 7
    const int quad = t & 7, j = (t >> 3) & (WL - 1);
    const int ib = WL == 32 ? 0 : 8 * (wave >> 1);
    int coff[3];                                                  // tapsum_col_off of columns clamp(j - 1 + c), the lane's channel quad
#pragma unroll
    for (int c = 0; c < 3; ++c) coff[c] = tapsum_col_off(min(max(j - 1 + c, 0), WL - 1), quad);
    float hx[4], lx[4];
    tapsum_col_weights<WL>(j, hx, lx);
    // the rows' weights: only a thread's first row can be the map's top, only its eighth the map's bottom (wave-uniform)
    const TapsumRowW wy = tapsum_row_weights(r0 + ib == 0, r0 + ib + 7 == Hl - 1);

    f4v out[8][2][2];                                             // the 2 x 2 output cells of rows i, column j (written, not added to, by the first column group)
    f4v S[8][2];                                                  // the vertical sums of the column group kx in flight: up-sampled rows 2i + ay of low-res column j

    wait_taps_in_flight(16);                                      // my pieces of tap 0 have landed (the pixel fragments were issued before them)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    auto tap = [&]<int s>() {                                     // (a template, called nine times: `#pragma unroll` gives up on a body of this size)
        constexpr int tp = tap_at(s), ky = tp / 3, kx = tp - 3 * ky;
        unsigned char* chunk = lds + W_BYTES + (s & 1) * CH_BYTES;
        // ---- the tap's products of my fragments -> chunk
        {
            const unsigned char* wb = lds + tp * TAP_BYTES;
            h8v wh[4], wl[4];
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const int K = 8 * (kc >> 1) + 2 * (kc & 1);
                wh[kc] = *reinterpret_cast<const h8v*>(wb + (wfo ^ (K * 16)));
                wl[kc] = *reinterpret_cast<const h8v*>(wb + (wfo ^ ((K + 4) * 16)));
            }
#pragma unroll
            for (int fi = 0; fi < NFW; ++fi) {
                const int f = frag(fi);
                {
                    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) {
                        acc  = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[kc], xh[fi][kc], acc, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[kc], xh[fi][kc], acc1, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[kc], xl[fi][kc], acc1, 0, 0, 0);
                    }
                    const int px = f * 32 + (lane & 31);
                    tapsum_park(acc1, acc, chunk + px * 128, (px >> 1) & 3, lane >> 5);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (s < 8) wait_taps_in_flight(2 * (7 - s));              // my pieces of the next tap (step s + 1) have landed
        wait_lds_reads();                                         // my products are in the chunk (and my reads of the weights have returned)
        __builtin_amdgcn_s_barrier();                             // everybody's are; everybody is done reading the OTHER chunk (step s - 1)
        asm volatile("" ::: "memory");
        tapsum_vertical<8, ky, ROW_BYTES>(S, chunk, r0 + ib, sbase, Hl, coff[1], wy);
        // ---- horizontal stage, after the third tap of a column group.  The neighbour columns' S live in other threads (other waves at j % 8 == 0 / 7): one ay
        // half is 32 KiB: ay = 0 goes to the chunk this step did not use, ay = 1 to this step's chunk once everybody has left its vertical stage.
        if constexpr (ky == 2) {
            unsigned char* other = lds + W_BYTES + ((s & 1) ^ 1) * CH_BYTES;
            tapsum_put<8, 0, ROW_BYTES>(S, other, ib, coff[1]);
            wait_lds_reads();                                     // my ay = 0 sums are in `other` (and my reads of this step's products have returned)
            __builtin_amdgcn_s_barrier();                         // everybody's are; everybody has left the vertical stage: this step's chunk is free
            asm volatile("" ::: "memory");
            tapsum_put<8, 1, ROW_BYTES>(S, chunk, ib, coff[1]);
            __builtin_amdgcn_sched_barrier(0);
            tapsum_horizontal<8, kx, 0, ROW_BYTES>(out, S, other, ib, coff[0], coff[2], hx, lx);
            wait_lds_reads();                                     // my ay = 1 sums are in the chunk, my reads of `other` have returned
            __builtin_amdgcn_s_barrier();                         // everybody's: the next step's products may overwrite `other`
            asm volatile("" ::: "memory");
            tapsum_horizontal<8, kx, 1, ROW_BYTES>(out, S, chunk, ib, coff[0], coff[2], hx, lx);   // (the step after next overwrites this chunk, behind the next step's barrier)
        }
    };
    tap.template operator()<0>(); tap.template operator()<1>(); tap.template operator()<2>();
    tap.template operator()<3>(); tap.template operator()<4>(); tap.template operator()<5>();
    tap.template operator()<6>(); tap.template operator()<7>(); tap.template operator()<8>();

    // ---- bias, activation, SH store
    f4v bv = (f4v)(0.0f);
    if (a.bias) bv = *reinterpret_cast<const f4v*>(a.bias + col0 + quad * 4);
    const int Ho = 2 * Hl, Wo = 2 * WL;
#pragma unroll
    for (int it = 0; it < 8; ++it)
#pragma unroll
        for (int ay = 0; ay < 2; ++ay)
#pragma unroll
            for (int bx = 0; bx < 2; ++bx) {
                f4v o = out[it][ay][bx] + bv;
                if (a.act == OMNI_ACT_RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                const int oy = 2 * (r0 + ib + it) + ay, ox = 2 * j + bx;
                act_store4<true>(a.dst, (((size_t)m * Ho + oy) * Wo + ox) * a.Cout + col0 + quad * 4, o);
            }
}

// ---------------------------------------------------------------- up2_taps_walk_kernel: the same sums on eight waves, by a block that walks
// The operations of up2_taps_fused_kernel on every output element, in its order (same fragment products, chunk layout, tap order and helpers of
// omni_up2_tapsum.h, same epilogue: the same bits), in the structure of up2_heads_taps_kernel (omni_conv_up2_heads_taps.hip):
//   * 512 threads, two waves per SIMD at <= 256 registers: one wave's tap sum runs beside the other's matrix instructions;
//   * a UNIT is (image, band of 8 rows + halo — or the whole 16 x 16 image —, 32-channel half).  XCD x (blocks x mod 8) owns one contiguous range of
//     (image, band) pairs, both halves of each: unit u = 2 * pair + half.  Block lb of the XCD's nlb walks u = first + lb, + nlb, ...: with nlb even (every
//     default grid of a launch with more units than blocks) it keeps one channel half for its life and DMAs its nine taps of weights ONCE, in processing
//     order, with counted waits through its first unit.  An odd nlb (option conv_up2_taps_walk_grid, tiny launches) makes the half alternate: the block
//     then fetches the other half's weights between units, behind a full wait;
//   * ten fragments on eight waves (bands): waves 0 and 1 take fragments w and w + 8, the others leave the second fragment's products out behind a
//     wave-uniform branch — no product is computed or parked twice.  Whole images: eight fragments, one per wave;
//   * tap sum: thread = (column j, channel quad, row group g): rows 4 g .. 4 g + 3 of the band, ROWS = 4 (64 + 32 registers).  Only a band's first row
//     can be the map's top and only its last the bottom, so the row weights of a 4-row thread are those the 8-row thread of the parent used;
//   * the next unit's pixel fragments are requested as soon as the ninth tap's products are issued.
struct WalkArgs {
    const void* src;                         // SH [M, Hl, Wl, 64]
    const void* wt;                          // halfs [9 * 64][2][hi32|lo32], row t*64 + co
    const float* bias;                       // [64] or null
    void* dst;                               // SH [M, 2Hl, 2Wl, 64]
    int Hl, act, npairs;                     // npairs = M * bands per image
};

template <int WL>
__global__ __launch_bounds__(512, 1) void up2_taps_walk_kernel(WalkArgs a)
{
    static_assert(WL == 32 || WL == 16, "bands of 8 rows of 32-wide maps, or whole 16 x 16 maps");
    constexpr int BROWS = WL == 32 ? 8 : 16, HALO = WL == 32 ? 1 : 0, ROWS = 4;
    constexpr int SROWS = BROWS + 2 * HALO, P = SROWS * WL, NF = P / 32, NFW = (NF + 7) / 8;
    constexpr int W_BYTES = 9 * TAP_BYTES, CH_BYTES = P * 128, ROW_BYTES = WL * 128;
    static_assert(P % 32 == 0 && BROWS * WL * 8 == 512 * ROWS && NF <= 16, "whole fragments; one (column, channel quad, row group) thread per four rows");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[W_BYTES + 2 * CH_BYTES];
    static_assert(sizeof(lds) <= 160 * 1024 && BROWS * ROW_BYTES <= CH_BYTES, "one block per CU; one ay half of the vertical sums fits a chunk");

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    const int Hl = a.Hl, nb = Hl / BROWS;
    // units of this block: XCD x owns the (image, band) pairs [x per, (x + 1) per), neighbours and both channel halves in one L2
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int per = (a.npairs + 7) >> 3, u_end = 2 * min(a.npairs, (xcd + 1) * per);
    int u = 2 * xcd * per + lb;
    if (u >= u_end) return;
    int half = u & 1;

    // ---- the wave's pixel fragments: fragment f = slot pixels 32 f .. 32 f + 31, lane -> pixel lane & 31, 16-byte piece lane >> 5 of every 16-channel chunk
    auto frag = [&](int fi) { return fi == 0 || wave + 8 >= NF ? wave : wave + 8; };   // (waves 2-7 load their fragment twice and use it once)
    h8v xh[NFW][4], xl[NFW][4];
    auto load_x = [&](int unit) {
        const int pr = unit >> 1, m = pr / nb, sbase = (pr - m * nb) * BROWS - HALO;
#pragma unroll
        for (int fi = 0; fi < NFW; ++fi) {
            const int p = frag(fi) * 32 + (lane & 31), sr = p / WL, cx = p - sr * WL;
            const int row = min(max(sbase + sr, 0), Hl - 1);     // (the halo row above the first / below the last band is never read by the tap sum)
            const unsigned char* sp = (const unsigned char*)a.src + ((size_t)(m * Hl + row) * WL + cx) * 256 + (lane >> 5) * 16;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                xh[fi][kc] = *reinterpret_cast<const h8v*>(sp + (kc >> 1) * 128 + (kc & 1) * 32);
                xl[fi][kc] = *reinterpret_cast<const h8v*>(sp + (kc >> 1) * 128 + 64 + (kc & 1) * 32);
            }
        }
    };
    // ---- nine taps of weights of channel half h, ONE DMA instruction per wave and tap, in processing order (kx-major); tap tp keeps its place
    // tp * TAP_BYTES.  An instruction deposits four 256-byte rows; the 16 pieces of row r are permuted with r & 15 like the parent's
    const rsrc_t rsw = make_rsrc(a.wt, (size_t)9 * 64 * 256);
    auto load_w = [&](int h) {
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            const int tp = tap_at(s), row = 4 * wave + (lane >> 4), piece = (lane & 15) ^ (row & 15);
            dma16(rsw, lds + tp * TAP_BYTES + wave * 1024, ((tp * 64 + h * 32 + row) * 16 + piece) * 16, 0);
        }
    };
    load_x(u);
    load_w(half);
    // weight fragment of row lane & 31: piece K | h (K = 8 group + 4 lo + 2 chunk, h = lane >> 5) sits in slot (K | h) ^ (row & 15) = K ^ (h ^ (row & 15))
    const int wfo = (lane & 31) * 256 + (((lane >> 5) ^ (lane & 15)) * 16);

    // ---- tap sum geometry: thread = (low-res column j, channel quad, row group), rows i = r0 + ib + it, it = 0 .. 3 (ib is wave-uniform)
    const int quad = t & 7, j = (t >> 3) & (WL - 1);
    const int ib = ROWS * (wave / (WL / 8));
    const int coff1 = tapsum_col_off(j, quad);
    bool first = true;                                            // the block's first unit: its weights are still on their way

    wait_vm<8>();                                                 // my piece of tap 0 has landed (the pixel fragments were issued before it)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    for (;;) {
        const int pr = u >> 1, m = pr / nb, band = pr - m * nb;
        const int r0 = band * BROWS, sbase = r0 - HALO;           // sbase: image row of LDS slot row 0
        const int col0 = half * 32;
        const int next = u + nlb;
        // the rows' weights: only a thread's first row can be the map's top, only its fourth the map's bottom (wave-uniform)
        const TapsumRowW wy = tapsum_row_weights(r0 + ib == 0, r0 + ib + ROWS - 1 == Hl - 1);

        f4v out[ROWS][2][2];                                      // the 2 x 2 output cells of rows i, column j (written, not added to, by the first column group)
        f4v S[ROWS][2];                                           // the vertical sums of the column group kx in flight: up-sampled rows 2i + ay of low-res column j

        auto tap = [&]<int s>() {                                 // (a template, called nine times: `#pragma unroll` gives up on a body of this size)
            constexpr int tp = tap_at(s), ky = tp / 3, kx = tp - 3 * ky;
            unsigned char* chunk = lds + W_BYTES + (s & 1) * CH_BYTES;
            // ---- the tap's products of my fragments -> chunk
            {
                const unsigned char* wb = lds + tp * TAP_BYTES;
                // Registers: 64 (out) + 32 (S) + 64 (two fragments) stay; a tap's eight weight fragments at once (32) and the sixteen LDS addresses of the
                // weight reads and the parks, kept across the nine unrolled taps, were 31 more than a wave has.  So the weight fragments come two k chunks
                // at a time (waves 0 and 1 read them again for their second fragment), and every address is formed per tap from a copy of the lane's
                // constants that the compiler cannot see through.
                int ln = lane, wf = wfo;
                asm volatile("" : "+v"(ln), "+v"(wf));
#pragma unroll
                for (int fi = 0; fi < NFW; ++fi) {
                    if (fi == 1 && wave + 8 >= NF) break;         // (wave-uniform: fragments 8 and 9 belong to waves 0 and 1)
                    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
#pragma unroll
                    for (int kh = 0; kh < 2; ++kh) {
                        h8v wh[2], wl[2];
#pragma unroll
                        for (int k2 = 0; k2 < 2; ++k2) {
                            const int K = 8 * kh + 2 * k2;
                            wh[k2] = *reinterpret_cast<const h8v*>(wb + (wf ^ (K * 16)));
                            wl[k2] = *reinterpret_cast<const h8v*>(wb + (wf ^ ((K + 4) * 16)));
                        }
#pragma unroll
                        for (int k2 = 0; k2 < 2; ++k2) {
                            const int kc = 2 * kh + k2;
                            acc  = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[k2], xh[fi][kc], acc, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[k2], xh[fi][kc], acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[k2], xl[fi][kc], acc1, 0, 0, 0);
                        }
                    }
                    const int px = frag(fi) * 32 + (ln & 31);
                    tapsum_park(acc1, acc, chunk + px * 128, (px >> 1) & 3, ln >> 5);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (s < 8) { if (first) wait_vm<7 - s>(); } // my piece of the next tap (step s + 1) has landed: the first unit only
            else load_x(next < u_end ? next : u);                 // the fragments are free: the next unit's (after the last one: its own again, no branch) are on their way
            wait_lds_reads();                                     // my products are in the chunk (and my reads of the weights have returned)
            __builtin_amdgcn_s_barrier();                         // everybody's are; everybody is done reading the OTHER chunk (step s - 1)
            asm volatile("" ::: "memory");
            tapsum_vertical<ROWS, ky, ROW_BYTES>(S, chunk, r0 + ib, sbase, Hl, coff1, wy);
            // ---- horizontal stage, after the third tap of a column group.  The neighbour columns' S live in other threads: one ay half is 32 KiB: ay = 0 goes to
            // the chunk this step did not use, ay = 1 to this step's chunk once everybody has left its vertical stage.
            if constexpr (ky == 2) {
                unsigned char* other = lds + W_BYTES + ((s & 1) ^ 1) * CH_BYTES;
                auto horizontal = [&]<int ay>(const unsigned char* buf) {
                    // the column's constants are formed HERE, from a copy of j the compiler cannot see through (as up2_heads_taps_kernel does): kept across
                    // the unit they cost 10 registers the products' phase does not have
                    int jj = j;
                    asm volatile("" : "+v"(jj));
                    float hx[4], lx[4];
                    tapsum_col_weights<WL>(jj, hx, lx);
                    tapsum_horizontal<ROWS, kx, ay, ROW_BYTES>(out, S, buf, ib, tapsum_col_off(max(jj - 1, 0), quad), tapsum_col_off(min(jj + 1, WL - 1), quad), hx, lx);
                };
                tapsum_put<ROWS, 0, ROW_BYTES>(S, other, ib, coff1);
                wait_lds_reads();                                 // my ay = 0 sums are in `other` (and my reads of this step's products have returned)
                __builtin_amdgcn_s_barrier();                     // everybody's are; everybody has left the vertical stage: this step's chunk is free
                asm volatile("" ::: "memory");
                tapsum_put<ROWS, 1, ROW_BYTES>(S, chunk, ib, coff1);
                __builtin_amdgcn_sched_barrier(0);
                horizontal.template operator()<0>(other);
                wait_lds_reads();                                 // my ay = 1 sums are in the chunk, my reads of `other` have returned
                __builtin_amdgcn_s_barrier();                     // everybody's: the next step's products may overwrite `other`
                asm volatile("" ::: "memory");
                horizontal.template operator()<1>(chunk);         // (the step after next overwrites this chunk, behind the next step's barrier)
            }
        };
        tap.template operator()<0>(); tap.template operator()<1>(); tap.template operator()<2>();
        tap.template operator()<3>(); tap.template operator()<4>(); tap.template operator()<5>();
        tap.template operator()<6>(); tap.template operator()<7>(); tap.template operator()<8>();

        // ---- bias, activation, SH store
        f4v bv = (f4v)(0.0f);
        if (a.bias) bv = *reinterpret_cast<const f4v*>(a.bias + col0 + quad * 4);
        const int Ho = 2 * Hl, Wo = 2 * WL;
#pragma unroll
        for (int it = 0; it < ROWS; ++it)
#pragma unroll
            for (int ay = 0; ay < 2; ++ay)
#pragma unroll
                for (int bx = 0; bx < 2; ++bx) {
                    f4v o = out[it][ay][bx] + bv;
                    if (a.act == OMNI_ACT_RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                    const int oy = 2 * (r0 + ib + it) + ay, ox = 2 * j + bx;
                    act_store4<true>(a.dst, (((size_t)m * Ho + oy) * Wo + ox) * 64 + col0 + quad * 4, o);
                }
        if (next >= u_end) break;
        u = next;
        first = false;
        if ((u & 1) != half) {                                    // (block-uniform; never with an even number of blocks per XCD) the other half's weights: everybody
            half = u & 1;                                         // has left the ninth tap's products, the last reads of the old ones
            load_w(half);
            wait_vm<0>();
        }
        wait_lds_reads();                                         // my reads of the chunks (the last horizontal stage) have returned
        __builtin_amdgcn_s_barrier();                             // everybody's have: the next unit's first products may overwrite them (and everybody's weights have landed)
        asm volatile("" ::: "memory");
    }
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_up2_taps)      // this translation unit's copy of the sticky range flag

// dst = act(conv3x3(pad 1)(bilinear 2x up-sampling of src) + bias) from the nine 1x1 tap products on the low-resolution map, one launch (see the head of this file).
// src SH [M, Hl, Wl, 64]; wt16t: the tap-major f16x3 weights [9 * Cout][64] (row t*Cout + co = W[co][t][:]); dst SH [M, 2Hl, 2Wl, Cout]; fmt: 1 (SH result, f16x3;
// bit 2, the latency plan of a lone panorama, is accepted and ignored: one form for every batch).
extern "C" int omni_conv3x3_up2_taps_sh_f16x3(const void* src, const void* wt16t, const float* bias, void* dst, int fmt,
                                              int M, int Hl, int Wl, int C, int Cout, int act, omni_stream_t stream)
{
    if (!src || !wt16t || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_taps_sh: null pointer");
    if (M <= 0 || Hl <= 0 || Wl <= 0 || C <= 0 || C % 32 || Cout <= 0 || Cout % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_taps_sh: bad shape (channels must be multiples of 32)");
    if ((uintptr_t)src % 16 || (uintptr_t)wt16t % 16 || (uintptr_t)bias % 16 || (uintptr_t)dst % 16) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_taps_sh: tensors must be 16-byte aligned");
    const bool bands = Wl == 32 && Hl % 8 == 0, image = Wl == 16 && Hl == 16;
    if ((fmt & ~4) != 1 || C != 64 || Cout != 64 || !(bands || image) || (act != OMNI_ACT_NONE && act != OMNI_ACT_RELU))
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_up2_taps_sh: serves f16x3 with an SH result, 64 -> 64 channels, Wl = 32 with Hl % 8 == 0 or 16 x 16 maps, no activation or ReLU");
    if ((long long)M * Hl * Wl * 4 >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_up2_taps_sh: tensor too large for 32-bit indices");
    TapsArgs a;
    a.src = src; a.wt = wt16t; a.bias = bias; a.dst = dst; a.M = M; a.Hl = Hl; a.Cout = Cout; a.act = act;
    // option conv_up2_taps_walk: up2_taps_walk_kernel (same bits) for the forms that were faster in flight (WALK_BANDS / WALK_IMAGE below); 2: both forms,
    // 3 / 4: bands / whole images only; 0: the parent kernel
    constexpr bool WALK_BANDS = true, WALK_IMAGE = false;
    const OmniOptions& o = omni_options();
    const int wk = o.conv_up2_taps_walk;
    if (bands ? (wk == 1 && WALK_BANDS) || wk == 2 || wk == 3 : (wk == 1 && WALK_IMAGE) || wk == 2 || wk == 4) {
        WalkArgs k;
        k.src = src; k.wt = wt16t; k.bias = bias; k.dst = dst; k.Hl = Hl; k.act = act; k.npairs = bands ? M * (Hl / 8) : M;
        // one persistent block per CU, a multiple of 8 (one range of units per XCD), or as many as there are units; option conv_up2_taps_walk_grid caps it
        const long long units = 2ll * k.npairs;
        const int cus = std::max(8, omni_num_cus() / 8 * 8);
        long long grid = units < cus ? (units + 7) / 8 * 8 : cus;
        if (o.conv_up2_taps_walk_grid > 0) grid = std::min<long long>(grid, std::max(8, o.conv_up2_taps_walk_grid / 8 * 8));
        if (bands) hipLaunchKernelGGL(up2_taps_walk_kernel<32>, dim3((unsigned)grid), dim3(512), 0, (hipStream_t)stream, k);
        else       hipLaunchKernelGGL(up2_taps_walk_kernel<16>, dim3((unsigned)grid), dim3(512), 0, (hipStream_t)stream, k);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    const unsigned ntn = (unsigned)(Cout / 32);
    if (bands) hipLaunchKernelGGL((up2_taps_fused_kernel<32, 8, 1>), dim3((unsigned)M * (unsigned)(Hl / 8) * ntn), dim3(256), 0, (hipStream_t)stream, a);
    else       hipLaunchKernelGGL((up2_taps_fused_kernel<16, 16, 0>), dim3((unsigned)M * ntn), dim3(256), 0, (hipStream_t)stream, a);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
