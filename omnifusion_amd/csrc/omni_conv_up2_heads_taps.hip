// omni_conv_up2_heads_taps.hip — up2_heads_taps_kernel: de_conv4_0 = relu(conv3x3(upsample2x(x)) + bias), 32 -> 32 channels, 64 x 64 -> 128 x 128, as nine 1x1
// TAP PRODUCTS on the low-resolution map with the first half of the two heads fused — the form of up2_taps_fused_kernel (omni_conv_up2_taps.hip) for the
// launch that conv3x3_up2_g1_kernel<HEADS> (omni_conv_up2.hip) serves.  Both operators are linear, so
//   y[q] = bias + sum_t [q + t - 1 inside the 128 x 128 map] * up2(W_t . x)[q + t - 1]                           (t = ky*3 + kx)
// — 3/8 of the matrix instructions of the convolution at full resolution, and the up-sampled operand (a 6 x 34-pixel halo per 4 x 32 tile, interpolated
// and split again by four producer waves) never exists.  Reached from omni_conv3x3_up2_heads_sh_f16x3 through omni_up2_heads_taps_launch and from nowhere
// else; f16x3 only.
// SHAPE RULE: P == 128 exactly (low-resolution map 64 x 64): a band needs the full low-resolution width, 64 columns, in one block and the height a multiple
// of the band's 4 rows.  Every other P stays on the g1 kernel.
//
// A block (8 waves) walks over BANDS: 4 low-resolution rows of one image at full width + one halo row each side (6 x 64 = 384 pixels = 12 fragments of 32
// pixels; left and right need no halo, the clamp of the up-sampling addresses the same column) and all 32 output channels:
//   * the nine taps of weights (36 KiB) go to LDS by LDS-DMA ONCE per block, gathered tap-major from the [Cout][9][hi32|lo32] rows of `de_conv4_0.w16`
//     (per-lane global offset (co * 9 + tap) * 128 + piece * 16), and are waited for with ONE hand-placed s_waitcnt vmcnt(0) in front of the first barrier;
//   * a wave keeps the SH fragments of its pixels (fragments w and w + 8; K = 32: hi and lo of two 16-channel chunks, 16 registers per fragment) in
//     registers for all nine taps.  Twelve fragments on eight waves: waves 0-3 do two (w and w + 8), waves 4-7 one and leave the second fragment's products
//     out behind a wave-uniform branch (a SIMD holds waves w and w + 4: three fragments each; with the second fragment repeated instead, as
//     up2_taps_fused_kernel does, the launch took 183 us instead of 173 at 144 patches).  The next band's fragments are loaded as soon as the ninth tap's
//     products are issued;
//   * per tap: 6 matrix instructions per fragment (the f16x3 three-term product, acc_join) -> the fp32 products [pixel][32 channels] in one of two LDS
//     chunks (48 KiB) -> ONE barrier -> the SEPARABLE tap sum of up2_taps_fused_kernel: taps kx-major (0, 3, 6, 1, 4, 7, 2, 5, 8), a vertical stage per tap
//     on the thread's own column, a horizontal stage once per kx whose neighbour columns come through the chunk that is not in use (two more barriers per
//     kx).  Thread = (low-res column j, channel quad): four 2 x 2 output cells x 4 channels = 64 accumulator registers + 32 for the vertical stage.  Same
//     weights, clamps, order of summation and chunk piece permutation as there; tests/test_up2_taps_sep_cpu.py is the specification;
//   * heads: bias, ReLU and sh_split4 (range guard, sticky flag) as every SH epilogue; the band's 8 x 128 output pixels are parked in the chunks as SH rows
//     in two halves of 4 rows (64 KiB each) with the 16-byte pieces in FRAGMENT order — piece 2 kc + h of a pixel holds channel quads 4 kc + h and
//     4 kc + 2 + h, the k order in which the g1 kernel's accumulator quads meet `heads.w16f` — so the heads' product of a 32-pixel row segment is four
//     ds_read_b128 and the same six matrix instructions, the three dx terms meet across neighbouring lanes in the order -1, 0, +1, and the 34 partial sums
//     per (tile row, (dy, head)) land in `hr` at the addresses and with the meaning conv3x3_up2_g1_kernel<HEADS> gives them (tile = 4 output rows x 32
//     pixels, HR_PITCH = 36).  heads_finish_kernel runs unchanged.
// Fixed order, no atomics but the sticky flag, no dependence on block placement or on M: an image's bits are the same alone and inside a batch.
// LDS: 36 KiB + 2 x 48 KiB = 132 KiB, one block of eight waves per CU, at most 256 registers per lane, no scratch.
#include <stdint.h>
#include "omni_conv_sh_common.h"

namespace {

constexpr int HR_PITCH = 36;                 // floats per (tile row, (dy, head)) record of `hr`, as in omni_conv_up2.hip (heads_finish_kernel reads it)

struct HeadsTapsArgs {
    const void* src;                         // SH [M, 64, 64, 32]
    const void* wt;                          // halfs [32][9 taps][hi32|lo32]
    const float* bias;                       // [32] or null
    const void* hw16;                        // the heads' weights in fragment order (heads.w16f), 4 KB
    float* hr;                               // the partial sums heads_finish_kernel adds up
    int nbands;                              // M * 16
};

constexpr int WL = 64, HL = 64, ROWS = 4, SROWS = ROWS + 2, NPX = SROWS * WL, NF = NPX / 32;
constexpr int TAP_BYTES = 32 * 128, W_BYTES = 9 * TAP_BYTES, CH_BYTES = NPX * 128, ROW_BYTES = WL * 128;
constexpr int BANDS_PER_IMG = HL / ROWS;

// the tap (ky * 3 + kx) processed at step s: kx-major, 0, 3, 6, 1, 4, 7, 2, 5, 8 — the three taps of a column kx follow each other
__host__ __device__ constexpr int tap_at(int s) { return 3 * (s % 3) + s / 3; }

__global__ __launch_bounds__(512, 1) void up2_heads_taps_kernel(HeadsTapsArgs a)
{
    __shared__ __attribute__((aligned(1024))) unsigned char lds[W_BYTES + 2 * CH_BYTES];
    static_assert(sizeof(lds) <= 160 * 1024 && NF == 12 && 4 * 128 * 128 <= 2 * CH_BYTES, "one block per CU; half a band's SH rows fit the two chunks");

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    // bands of this block: XCD x (blocks x mod 8) owns one contiguous range of bands (neighbours share their halo rows in one L2), its blocks walk it
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int per = (a.nbands + 7) >> 3, b_end = min(a.nbands, (xcd + 1) * per);
    int bandid = xcd * per + lb;
    if (bandid >= b_end) return;

    // ---- all nine taps of weights, once: 36 DMA instructions of 1 KiB (four 256-byte row pairs) over eight waves.  Tap tp sits at tp * TAP_BYTES as 32 rows of
    // 128 B; the 16 pieces of row pair d are permuted with d (slot s holds piece s ^ d, piece = 8 (row & 1) + 4 lo + 2 chunk + k half): conflict-free fragment reads
    {
        const rsrc_t rsw = make_rsrc(a.wt, (size_t)32 * 9 * 128);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int n = wave + 8 * k;
            if (n < 36) {
                const int tp = n >> 2, d = (n & 3) * 4 + (lane >> 4), pw = (lane & 15) ^ d, row = 2 * d + (pw >> 3);
                dma16(rsw, lds + n * 1024, ((row * 9 + tp) * 8 + (pw & 7)) * 16, 0);
            }
        }
    }
    // weight fragment of row lane & 31: piece K | h (K = 4 lo + 2 chunk, h = lane >> 5)
    const int wfo = ((lane & 31) >> 1) * 256 + ((((lane & 1) * 8 + (lane >> 5)) ^ ((lane & 31) >> 1)) * 16);

    // ---- the wave's pixel fragments: fragment f = slot pixels 32 f .. 32 f + 31, lane -> pixel lane & 31, 16-byte piece lane >> 5 of every 16-channel chunk
    auto frag = [&](int fi) { return fi == 0 || wave >= 4 ? wave : wave + 8; };   // (waves 4-7 load their fragment twice and use it once)
    h8v xh[2][2], xl[2][2];
    auto load_x = [&](int bid) {
        const int m = bid / BANDS_PER_IMG, sbase = (bid - m * BANDS_PER_IMG) * ROWS - 1;
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
            const int p = frag(fi) * 32 + (lane & 31), sr = p / WL, cx = p - sr * WL;
            const int row = min(max(sbase + sr, 0), HL - 1);     // (the halo row above the first / below the last band is never read by the tap sum)
            const unsigned char* sp = (const unsigned char*)a.src + ((size_t)(m * HL + row) * WL + cx) * 128 + (lane >> 5) * 16;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                xh[fi][kc] = *reinterpret_cast<const h8v*>(sp + kc * 32);
                xl[fi][kc] = *reinterpret_cast<const h8v*>(sp + 64 + kc * 32);
            }
        }
    };
    load_x(bandid);

    // ---- tap sum geometry: thread = (low-res column j, channel quad), rows i = r0 + it, it = 0 .. 3
    const int quad = t & 7, j = t >> 3;
    // byte offset of column col in a chunk row, the lane's channel quad (chunk pieces are permuted with (pixel >> 1) & 3)
    auto col_off = [&](int col) { return col * 128 + ((quad ^ ((col >> 1) & 3)) * 16); };
    const int coff1 = col_off(j);
    wait_vm<0>();                                                 // my pieces of the weights have landed (and my first pixel fragments)
    __builtin_amdgcn_s_barrier();                                 // everybody's have
    asm volatile("" ::: "memory");

    for (;;) {
        const int m = bandid / BANDS_PER_IMG, band = bandid - m * BANDS_PER_IMG;
        const int r0 = band * ROWS, sbase = r0 - 1;               // sbase: image row of LDS slot row 0
        const int next = bandid + nlb;
        // the rows' weights: only a thread's first row can be the map's top, only its fourth the map's bottom (block-uniform)
        const bool top = r0 == 0, bot = r0 + ROWS - 1 == HL - 1;
        const float hy0[4] = {top ? 0.0f : 0.75f, top ? 1.0f : 0.25f, 0.75f, 0.25f}, ly0[4] = {top ? 0.0f : 0.25f, top ? 0.0f : 0.75f, 0.25f, 0.75f};
        const float hy3 = bot ? 0.0f : 0.25f, ly3 = bot ? 0.0f : 0.75f;

        f4v out[ROWS][2][2];                                      // the 2 x 2 output cells of rows i, column j (written, not added to, by the first column group)
        f4v S[ROWS][2];                                           // the vertical sums of the column group kx in flight: up-sampled rows 2i + ay of low-res column j

        auto tap = [&]<int s>() {                                 // (a template, called nine times: `#pragma unroll` gives up on a body of this size)
            constexpr int tp = tap_at(s), ky = tp / 3, kx = tp - 3 * ky;
            unsigned char* chunk = lds + W_BYTES + (s & 1) * CH_BYTES;
            // ---- the tap's products of my fragments -> chunk
            {
                const unsigned char* wb = lds + tp * TAP_BYTES;
                h8v wh[2], wl[2];
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    wh[kc] = *reinterpret_cast<const h8v*>(wb + (wfo ^ (2 * kc * 16)));
                    wl[kc] = *reinterpret_cast<const h8v*>(wb + (wfo ^ ((2 * kc + 4) * 16)));
                }
#pragma unroll
                for (int fi = 0; fi < 2; ++fi) {
                    if (fi == 1 && wave >= 4) break;              // (wave-uniform: fragments 8-11 belong to waves 0-3)
                    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
#pragma unroll
                    for (int kc = 0; kc < 2; ++kc) {
                        acc  = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[kc], xh[fi][kc], acc, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[kc], xh[fi][kc], acc1, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[kc], xl[fi][kc], acc1, 0, 0, 0);
                    }
                    const int px = frag(fi) * 32 + (lane & 31);
                    unsigned char* cp = chunk + px * 128;
                    const int sw = (px >> 1) & 3;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {                 // channels 8q + 4 (lane >> 5) .. + 3 of pixel px
                        f4v v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc_join<false>(acc1[4 * q + e], acc[4 * q + e]);
                        *reinterpret_cast<f4v*>(cp + (((2 * q + (lane >> 5)) ^ sw) * 16)) = v;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (s == 8) load_x(next < b_end ? next : bandid);   // the fragments are free: the next band's (after the last one: its own again, no branch) are on their way through the tap sum and the heads
            wait_lds_reads();                                     // my products are in the chunk (and my reads of the weights have returned)
            __builtin_amdgcn_s_barrier();                         // everybody's are; everybody is done reading the OTHER chunk (step s - 1)
            asm volatile("" ::: "memory");
            // ---- vertical stage: S (+)= the tap, on my own column.  The thread's column of the chunk is read once: rows r0 - 1 + k, k = 0 .. 5 (5 / 6 / 5 of them
            // for ky = 0 / 1 / 2), clamped to the map; up-sampled row 2i + ay + ky - 1 takes the row pair (it + r, it + r + 1), r = (ay + ky) >> 1
            {
                constexpr int klo = ky >> 1, khi = ROWS + ((ky + 1) >> 1);
                f4v R[ROWS + 2];
#pragma unroll
                for (int k = klo; k <= khi; ++k)
                    R[k] = *reinterpret_cast<const f4v*>(chunk + (min(max(r0 - 1 + k, 0), HL - 1) - sbase) * ROW_BYTES + coff1);
#pragma unroll
                for (int it = 0; it < ROWS; ++it)
#pragma unroll
                    for (int ay = 0; ay < 2; ++ay) {
                        const int uy = ay + ky, r = uy >> 1;
                        // weights of up-sampled row 2i + uy - 1 (rows 1 and 2 of a thread are never the map's edge)
                        const float h = it == 0 ? hy0[uy] : it == ROWS - 1 && uy == 3 ? hy3 : (uy & 1) ? 0.25f : 0.75f;
                        const float l = it == 0 ? ly0[uy] : it == ROWS - 1 && uy == 3 ? ly3 : (uy & 1) ? 0.75f : 0.25f;
                        f4v v;                                    // the first tap of a column group starts S
                        if constexpr (ky != 0) v = S[it][ay];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if constexpr (ky == 0) v[e] = fmaf(l, R[it + r + 1][e], h * R[it + r][e]);
                            else v[e] = fmaf(l, R[it + r + 1][e], fmaf(h, R[it + r][e], v[e]));
                        asm volatile("" : "+v"(v));               // pins the sum HERE: the compiler otherwise sinks the arithmetic below later barriers
                        S[it][ay] = v;
                    }
                __builtin_amdgcn_sched_barrier(0);                // one tap's column in flight at a time
            }
            // ---- horizontal stage, after the third tap of a column group: out (+)= hx * S[column j - 1 + c] + lx * S[column j + c], c = (bx + kx) >> 1.  The
            // neighbour columns' S live in other threads: they are exchanged through the chunks, in the chunks' own layout (row it, coff[]).  One ay half is
            // 32 KiB: ay = 0 goes to the chunk this step did not use, ay = 1 to this step's chunk once everybody has left its vertical stage.
            if constexpr (ky == 2) {
                unsigned char* other = lds + W_BYTES + ((s & 1) ^ 1) * CH_BYTES;
                auto horizontal = [&]<int ay>(const unsigned char* buf) {
                    // The column's constants are formed HERE, from a copy of j the compiler cannot see through: kept across the band they cost 10 registers the
                    // products' phase does not have.  Bilinear weights of up-sampled column 2j + u - 1, u = 0 .. 3, on the column pair (c, c + 1), c = u >> 1:
                    // (1 - l, l) with l = frac(max(0.5 (p + 0.5) - 0.5, 0)), zero where the column is outside the map
                    int jj = j;
                    asm volatile("" : "+v"(jj));
                    const int coff[3] = {col_off(max(jj - 1, 0)), 0, col_off(min(jj + 1, WL - 1))};
                    float hx[4], lx[4];
                    hx[0] = jj > 0 ? 0.75f : 0.0f;      lx[0] = jj > 0 ? 0.25f : 0.0f;
                    hx[1] = jj > 0 ? 0.25f : 1.0f;      lx[1] = jj > 0 ? 0.75f : 0.0f;
                    hx[2] = 0.75f;                      lx[2] = 0.25f;
                    hx[3] = jj < WL - 1 ? 0.25f : 0.0f; lx[3] = jj < WL - 1 ? 0.75f : 0.0f;
#pragma unroll
                    for (int it = 0; it < ROWS; ++it) {
                        const unsigned char* rp = buf + it * ROW_BYTES;
                        const f4v own = S[it][ay];
                        f4v left = own, right = own;              // (only the live one is read: kx = 0 never looks right, kx = 2 never left)
                        if (kx <= 1) left = *reinterpret_cast<const f4v*>(rp + coff[0]);
                        if (kx >= 1) right = *reinterpret_cast<const f4v*>(rp + coff[2]);
#pragma unroll
                        for (int bx = 0; bx < 2; ++bx) {
                            const int ux = bx + kx, c = ux >> 1;
                            const f4v va = c == 0 ? left : own, vb = c == 0 ? own : right;
                            f4v o;                                // the first column group starts out
                            if constexpr (kx != 0) o = out[it][ay][bx];
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if constexpr (kx == 0) o[e] = fmaf(lx[ux], vb[e], hx[ux] * va[e]);
                                else o[e] = fmaf(lx[ux], vb[e], fmaf(hx[ux], va[e], o[e]));
                            asm volatile("" : "+v"(o));           // (pinned like the vertical sums)
                            out[it][ay][bx] = o;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                };
#pragma unroll
                for (int it = 0; it < ROWS; ++it) *reinterpret_cast<f4v*>(other + it * ROW_BYTES + coff1) = S[it][0];
                wait_lds_reads();                                 // my ay = 0 sums are in `other` (and my reads of this step's products have returned)
                __builtin_amdgcn_s_barrier();                     // everybody's are; everybody has left the vertical stage: this step's chunk is free
                asm volatile("" ::: "memory");
#pragma unroll
                for (int it = 0; it < ROWS; ++it) *reinterpret_cast<f4v*>(chunk + it * ROW_BYTES + coff1) = S[it][1];
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

        // ---- the heads' first half, four output rows at a time: bias, ReLU, split -> SH rows in the chunks (pixel p = row * 128 + x of the half: row pair p >> 1
        // of 256 B, its 16 pieces permuted with (p >> 1) & 15 like the weights') -> the product of every 32-pixel row segment with heads.w16f -> hr
        h8v hwf[4];                                               // this lane's weight fragments (row lane & 31, k chunk lane >> 5)
#pragma unroll
        for (int k = 0; k < 4; ++k) hwf[k] = *reinterpret_cast<const h8v*>((const unsigned char*)a.hw16 + k * 1024 + lane * 16);
        unsigned char* park = lds + W_BYTES;
        // where the thread parks its outputs: SH piece 2 kc + h and 8-byte half s of channel quad 4 kc + 2 s + h
        const int pk_piece = 2 * (quad >> 2) + (quad & 1), pk_half = ((quad >> 1) & 1) * 8;
        const f4v bv = a.bias ? *reinterpret_cast<const f4v*>(a.bias + quad * 4) : (f4v)(0.0f);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            wait_lds_reads();                                     // my reads of the chunks (the last horizontal stage / the first half's fragments) have returned
            __builtin_amdgcn_s_barrier();                         // everybody's have: the chunks are free
            asm volatile("" ::: "memory");
#pragma unroll
            for (int itl = 0; itl < 2; ++itl)
#pragma unroll
                for (int ay = 0; ay < 2; ++ay)
#pragma unroll
                    for (int bx = 0; bx < 2; ++bx) {
                        f4v o = out[2 * half + itl][ay][bx] + bv;
                        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
                        h4v hi, lo; sh_split4(o, hi, lo);         // (the split every SH epilogue does: range guard included)
                        const int p = (2 * itl + ay) * 128 + 2 * j + bx, d = p >> 1;
                        unsigned char* pp = park + d * 256 + pk_half;
                        *reinterpret_cast<h4v*>(pp + ((((p & 1) * 8 + pk_piece) ^ (d & 15)) * 16)) = hi;
                        *reinterpret_cast<h4v*>(pp + ((((p & 1) * 8 + pk_piece + 4) ^ (d & 15)) * 16)) = lo;
                    }
            wait_lds_reads();                                     // my SH pieces are parked
            __builtin_amdgcn_s_barrier();                         // everybody's are
            asm volatile("" ::: "memory");
#pragma unroll
            for (int sg = 0; sg < 2; ++sg) {
                const int seg = wave + 8 * sg, row = seg >> 2, sx = seg & 3;   // the wave's segments: output row 8 band + 4 half + row, pixels 32 sx .. + 31
                const int px = lane & 31, h = lane >> 5;
                const int p = row * 128 + sx * 32 + px, d = p >> 1;
                const unsigned char* fp = park + d * 256;
                const int fo = (((p & 1) * 8 + h) ^ (d & 15)) * 16;
                h8v ph[2], pl[2];
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    ph[kc] = *reinterpret_cast<const h8v*>(fp + (fo ^ (2 * kc * 16)));
                    pl[kc] = *reinterpret_cast<const h8v*>(fp + (fo ^ ((2 * kc + 4) * 16)));
                }
                f16v d0 = (f16v)(0.0f), d1 = (f16v)(0.0f);
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    d0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[kc], ph[kc], d0, 0, 0, 0);
                    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[2 + kc], ph[kc], d1, 0, 0, 0);
                    d1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(hwf[kc], pl[kc], d1, 0, 0, 0);
                }
                // rows (reg & 3) + 8 (reg >> 2) + 4 h: register group g = 0..2 is (dy, head) pair g + 3h, its registers 0..2 are dx = -1, 0, +1
                const size_t tile = ((size_t)m * (2 * BANDS_PER_IMG) + 2 * band + half) * 4 + sx;
                float* hp = a.hr + (tile * 4 + row) * (6 * HR_PITCH);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const float tl = fmaf(d1[4 * g], 4.8828125e-4f, d0[4 * g]), tc = fmaf(d1[4 * g + 1], 4.8828125e-4f, d0[4 * g + 1]),
                                tr = fmaf(d1[4 * g + 2], 4.8828125e-4f, d0[4 * g + 2]);
                    // out[q] takes w[dx] . x[q + dx]: its dx = -1 term comes from pixel q - 1, its dx = +1 term from pixel q + 1
                    const float fl = __shfl_up(tl, 1, 32), fr = __shfl_down(tr, 1, 32);
                    const float sum = ((px > 0 ? fl : 0.0f) + tc) + (px < 31 ? fr : 0.0f);
                    float* rowp = hp + (g + 3 * h) * HR_PITCH;
                    rowp[px] = sum;
                    if (px == 0) rowp[32] = tr;                   // pixel -1 of this row (the left neighbour tile's column 31) takes my dx = +1 term
                    if (px == 31) rowp[33] = tl;                  // pixel 32 takes my dx = -1 term
                }
            }
        }
        if (next >= b_end) break;
        bandid = next;
        wait_lds_reads();                                         // my reads of the parked rows have returned
        __builtin_amdgcn_s_barrier();                             // everybody's have: the next band's first products may overwrite them
        asm volatile("" ::: "memory");
    }
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_up2_heads_taps)   // this translation unit's copy of the sticky range flag

// up2_heads_taps_kernel on one persistent block per CU (a multiple of 8: one range of bands per XCD).  src SH [M, 64, 64, 32]; hr: omni_up2_heads_scratch_bytes(M, 128).
int omni_up2_heads_taps_launch(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float* hr, int M, hipStream_t s)
{
    if (!src || !wt16 || !heads_w16f || !hr || M <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_up2_heads_taps_launch: null pointer or no patches");
    if ((uintptr_t)src % 16 || (uintptr_t)wt16 % 16 || (uintptr_t)bias % 16 || (uintptr_t)heads_w16f % 16 || (uintptr_t)hr % 16)
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_up2_heads_taps_launch: tensors must be 16-byte aligned");
    if ((long long)M * HL * WL >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_up2_heads_taps_launch: tensor too large for 32-bit indices");
    HeadsTapsArgs a;
    a.src = src; a.wt = wt16; a.bias = bias; a.hw16 = heads_w16f; a.hr = hr; a.nbands = M * BANDS_PER_IMG;
    const int cus = omni_num_cus() / 8 * 8;
    const unsigned grid = (unsigned)(a.nbands < cus ? (a.nbands + 7) / 8 * 8 : cus);
    hipLaunchKernelGGL(up2_heads_taps_kernel, dim3(grid), dim3(512), 0, s, a);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
