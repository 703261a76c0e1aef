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
//     chunks (48 KiB) -> ONE barrier -> the SEPARABLE tap sum of omni_up2_tapsum.h with ROWS = 4 (the one up2_taps_fused_kernel runs: same tap order, weights,
//     clamps, order of summation and chunk piece permutation), two more barriers per kx around its horizontal stage.  Thread = (low-res column j, channel
//     quad): four 2 x 2 output cells x 4 channels = 64 accumulator registers + 32 for the vertical stage;
//   * heads: bias, ReLU and sh_split4 (range guard, sticky flag) as every SH epilogue; the band's 8 x 128 output pixels are parked in the chunks as SH rows
//     in two halves of 4 rows (64 KiB each) with the 16-byte pieces in FRAGMENT order — piece 2 kc + h of a pixel holds channel quads 4 kc + h and
//     4 kc + 2 + h, the k order in which the g1 kernel's accumulator quads meet `heads.w16f` — so the heads' product of a 32-pixel row segment is four
//     ds_read_b128 and the same six matrix instructions, the three dx terms meet across neighbouring lanes in the order -1, 0, +1, and the 34 partial sums
//     per (tile row, (dy, head)) land in `hr` through the product and the record writer conv3x3_up2_g1_kernel<HEADS> uses (omni_heads_hr.h; tile = 4 output
//     rows x 32 pixels).  heads_finish_kernel runs unchanged.
// Fixed order, no atomics but the sticky flag, no dependence on block placement or on M: an image's bits are the same alone and inside a batch.
// LDS: 36 KiB + 2 x 48 KiB = 132 KiB, one block of eight waves per CU, at most 256 registers per lane, no scratch.
#include <stdint.h>
#include "omni_up2_tapsum.h"
#include "omni_heads_hr.h"

namespace {

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
    const int coff1 = tapsum_col_off(j, quad);
    wait_vm<0>();                                                 // my pieces of the weights have landed (and my first pixel fragments)
    __builtin_amdgcn_s_barrier();                                 // everybody's have
    asm volatile("" ::: "memory");

    for (;;) {
        const int m = bandid / BANDS_PER_IMG, band = bandid - m * BANDS_PER_IMG;
        const int r0 = band * ROWS, sbase = r0 - 1;               // sbase: image row of LDS slot row 0
        const int next = bandid + nlb;
        // the rows' weights: only a thread's first row can be the map's top, only its fourth the map's bottom (block-uniform)
        const TapsumRowW wy = tapsum_row_weights(r0 == 0, r0 + ROWS - 1 == HL - 1);

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
                    tapsum_park(acc1, acc, chunk + px * 128, (px >> 1) & 3, lane >> 5);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (s == 8) load_x(next < b_end ? next : bandid);   // the fragments are free: the next band's (after the last one: its own again, no branch) are on their way through the tap sum and the heads
            wait_lds_reads();                                     // my products are in the chunk (and my reads of the weights have returned)
            __builtin_amdgcn_s_barrier();                         // everybody's are; everybody is done reading the OTHER chunk (step s - 1)
            asm volatile("" ::: "memory");
            tapsum_vertical<ROWS, ky, ROW_BYTES>(S, chunk, r0, sbase, HL, coff1, wy);
            // ---- horizontal stage, after the third tap of a column group.  The neighbour columns' S live in other threads: one ay half is 32 KiB: ay = 0 goes to
            // the chunk this step did not use, ay = 1 to this step's chunk once everybody has left its vertical stage.
            if constexpr (ky == 2) {
                unsigned char* other = lds + W_BYTES + ((s & 1) ^ 1) * CH_BYTES;
                auto horizontal = [&]<int ay>(const unsigned char* buf) {
                    // The column's constants are formed HERE, from a copy of j the compiler cannot see through: kept across the band they cost 10 registers the
                    // products' phase does not have.
                    int jj = j;
                    asm volatile("" : "+v"(jj));
                    float hx[4], lx[4];
                    tapsum_col_weights<WL>(jj, hx, lx);
                    tapsum_horizontal<ROWS, kx, ay, ROW_BYTES>(out, S, buf, 0, tapsum_col_off(max(jj - 1, 0), quad), tapsum_col_off(min(jj + 1, WL - 1), quad), hx, lx);
                };
                tapsum_put<ROWS, 0, ROW_BYTES>(S, other, 0, coff1);
                wait_lds_reads();                                 // my ay = 0 sums are in `other` (and my reads of this step's products have returned)
                __builtin_amdgcn_s_barrier();                     // everybody's are; everybody has left the vertical stage: this step's chunk is free
                asm volatile("" ::: "memory");
                tapsum_put<ROWS, 1, ROW_BYTES>(S, chunk, 0, coff1);
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
                f16v d0, d1;
                heads_product(hwf, ph, pl, d0, d1);
                const size_t tile = ((size_t)m * (2 * BANDS_PER_IMG) + 2 * band + half) * 4 + sx;
                float* hp = a.hr + (tile * 4 + row) * (6 * HR_PITCH);
                OMNI_HEADS_HR_WRITE(d0, d1, hp, px, h)
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
