// omni_conv_pm.hip — the POSITION-MAJOR form of the im2col tile kernel (conv_pm_sh_kernel) for 3x3, stride 1, pad 1 convolutions of 8 x 8 and 4 x 4
// images.  The SH layout, the LDS image and the shared device helpers: omni_conv_sh_common.h; the parent kernel and the kernel choice: omni_conv_sh.hip.
//
// conv_sh_kernel's GEMM rows are in image order: a 128-row tile holds two whole 8 x 8 images (eight 4 x 4 ones), so each of the nine taps is inside the
// image for SOME row of every tile and the K loop walks them all — 16 % (8 x 8) to 31 % (4 x 4) of the (pixel, tap) products multiply the zero padding.
// Here GEMM row r is image r % M at position order[r / M]: all images' pixel (0,0), then all images' pixel (0,1), ... with the positions sorted by border
// class (first / inner / last row, then first / inner / last column).  The rows of a tile then share their live taps, and the tile's K loop issues and
// multiplies only the K-steps of the taps that are inside the image for at least one of its rows.
//
// Same bits as the parent: a skipped K-step's pixel operand is all zeros for every row of the tile, its products are exact zeros and acc + 0 = acc; the
// surviving steps run in increasing ks on every accumulator, the weights are read at the original ks * 128, split-K keeps the parent's boundaries in
// ORIGINAL K-steps (a range without a live tap writes a slab of zeros) and the slabs / outputs are written at the pixel's own index, so the second pass
// (sh_splitk_reduce_kernel) is the parent's.  Everything else — the LDS-DMA pipeline with four loader waves, the counted waits, the ping-pong phases of
// the eight matrix waves, the XCD remap and wt_major, the epilogues' arithmetic — is conv_sh_kernel<128, BN, 4, 2, 3, 4, PP>'s.
// (Not here: a matrix wave skipping the taps that are dead for its own 32 rows only.  Built and measured — a wave-uniform branch per phase — it was 0.7 %
//  SLOWER with three forwards in flight than skipping per tile alone: profiles/EXPERIMENTS.md, r20a.)
#include <string.h>
#include "omni_conv_sh_common.h"

namespace {

// order[s][i]: the i-th position (y * W + x) of a W x W image, W = 4 (s = 0) or 8 (s = 1), sorted by (row class, column class, position)
struct PmTab { unsigned char order[2][64]; };
constexpr PmTab pm_make()
{
    PmTab t{};
    for (int s = 0; s < 2; ++s) {
        const int W = s ? 8 : 4;
        int n = 0;
        for (int rc = 0; rc < 3; ++rc)
            for (int cc = 0; cc < 3; ++cc)
                for (int p = 0; p < W * W; ++p) {
                    const int y = p / W, x = p % W;
                    const int yc = y == 0 ? 0 : (y == W - 1 ? 2 : 1), xc = x == 0 ? 0 : (x == W - 1 ? 2 : 1);
                    if (yc == rc && xc == cc) t.order[s][n++] = (unsigned char)p;
                }
    }
    return t;
}
__constant__ PmTab pm_tab = pm_make();

// bit (ky * 3 + kx): tap (ky, kx) of the 3 x 3 window around (y, x) lies inside the W x W image
__device__ __forceinline__ unsigned pm_mask(int y, int x, int W)
{
    const unsigned xm = (x > 0 ? 1u : 0u) | 2u | (x < W - 1 ? 4u : 0u);
    return (y > 0 ? xm : 0u) | (xm << 3) | (y < W - 1 ? (xm << 6) : 0u);
}

// The LDS epilogue of omni_conv_sh_common.h (epilogue_tile_lds without a post-activation addend) for position-major rows: accumulator column px is GEMM
// row r0 + px, whose pixel is image (r % Mi) at position order[r / Mi].  The same operations on every element in the same order.
template <int NT, bool X1>
__device__ __forceinline__ void pm_epilogue_tile_lds(const f16v (&acc)[NT], const f16v (&acc1)[NT], const ShConvArgs& a, int r0, int nrows,
                                                     const int (&c0)[NT], int lane, float* tile, int Mi, int hw, int ws)
{
    constexpr int PITCH = 32 * NT + 4;
    {
        const int px = lane & 31;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f4v v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[j][4 * q + e], acc[j][4 * q + e]);
                *reinterpret_cast<f4v*>(tile + px * PITCH + 32 * j + 8 * q + 4 * (lane >> 5)) = v;
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // (wave-private tile: the wave's own writes have landed)
    constexpr int TASKS = 32 * NT * 4 / 64;                       // (pixel, group, piece) tasks per lane
    constexpr int HALF = TASKS >= 4 ? TASKS / 2 : TASKS;          // tasks whose loads are in flight together
#pragma unroll
    for (int k0 = 0; k0 < TASKS; k0 += HALF) {
        f4v va[HALF], vb[HALF]; h8v rh[HALF], rl[HALF];
        size_t off[HALF]; bool ok[HALF];
#pragma unroll
        for (int kk = 0; kk < HALF; ++kk) {
            const int task = (k0 + kk) * 64 + lane, px = task / (4 * NT), rem = task - px * (4 * NT), j = rem >> 2, pc = rem & 3;
            ok[kk] = px < nrows;
            va[kk] = *reinterpret_cast<const f4v*>(tile + px * PITCH + 32 * j + 8 * pc);
            vb[kk] = *reinterpret_cast<const f4v*>(tile + px * PITCH + 32 * j + 8 * pc + 4);
            const int r = ok[kk] ? r0 + px : r0, pi = r / Mi;      // (a column past the end: any valid row, never loaded or stored)
            const size_t pixel = (size_t)(r - pi * Mi) * hw + pm_tab.order[ws][pi];
            off[kk] = (pixel * a.Cout + c0[j]) * 4 + 16 * pc;     // byte offset of the hi piece (the lo piece: + 64)
            if (a.bias) { va[kk] += *reinterpret_cast<const f4v*>(a.bias + c0[j] + 8 * pc); vb[kk] += *reinterpret_cast<const f4v*>(a.bias + c0[j] + 8 * pc + 4); }
            if (a.res && ok[kk]) {
                rh[kk] = *reinterpret_cast<const h8v*>((const unsigned char*)a.res + off[kk]);
                rl[kk] = *reinterpret_cast<const h8v*>((const unsigned char*)a.res + off[kk] + 64);
            }
        }
#pragma unroll
        for (int kk = 0; kk < HALF; ++kk) {
            if (!ok[kk]) continue;
            f4v v0 = va[kk], v1 = vb[kk];
            if (a.res) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] += fmaf((float)rl[kk][e], 4.8828125e-4f, (float)rh[kk][e]); v1[e] += fmaf((float)rl[kk][4 + e], 4.8828125e-4f, (float)rh[kk][4 + e]); }
            }
            if (a.act == OMNI_ACT_RELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] = fmaxf(v0[e], 0.f); v1[e] = fmaxf(v1[e], 0.f); }
            } else if (a.act == OMNI_ACT_GELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { v0[e] = 0.5f * v0[e] * (1.0f + erff(v0[e] * 0.70710678118654752440f)); v1[e] = 0.5f * v1[e] * (1.0f + erff(v1[e] * 0.70710678118654752440f)); }
            }
            h4v h0, l0, h1, l1;
            sh_split4(v0, h0, l0); sh_split4(v1, h1, l1);
            h8v oh, ol;
#pragma unroll
            for (int e = 0; e < 4; ++e) { oh[e] = h0[e]; oh[4 + e] = h1[e]; ol[e] = l0[e]; ol[4 + e] = l1[e]; }
            *reinterpret_cast<h8v*>((unsigned char*)a.dst + off[kk]) = oh;
            *reinterpret_cast<h8v*>((unsigned char*)a.dst + off[kk] + 64) = ol;
        }
    }
}

// 128 x BN tile, eight matrix waves (4 x 2, ping-pong) + four loader waves, three stages.  Requires KH = KW = 3, stride 1, pad 1, H = W in {4, 8}.
template <int BN, bool X1>
__global__ __launch_bounds__(768) void conv_pm_sh_kernel(ShConvArgs a)
{
    constexpr int BM = 128, WM = 4, WN = 2, NST = 3, NW = 8, LW = 4, RPP = 8 * LW;
    constexpr int TN = BN / WN / 32;                            // 32x32 tiles per wave along the channels (one along the rows)
    constexpr int APASS = BM / RPP, BPASS = BN / RPP, LPS = APASS + BPASS;
    constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NST * STAGE];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    const int wm = wave / WN, wn = wave % WN;
    const bool loader = wave >= NW;                             // (wave-uniform)
    const int iw = wave - NW;                                   // index among the loader waves (meaningless in a matrix wave)
    const int ntn = a.Cout / BN;
    // (block order: as conv_sh_kernel — XCD remap, wt_major)
    const int ntm = (a.rows + BM - 1) / BM;
    const unsigned lb = a.noxcd ? blockIdx.x : omni_xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = a.wt_major ? (int)(lb % (unsigned)ntm) : (int)(lb / (unsigned)ntn), tile_n = a.wt_major ? (int)(lb / (unsigned)ntm) : (int)(lb % (unsigned)ntn);
    const int row0 = tile_m * BM, col0 = tile_n * BN;
    const int G1 = a.C1 >> 5, G2 = a.C2 >> 5, G = G1 + G2;
    const int ksteps = 9 * G;
    const int Mi = a.M, W = a.W, hw = W * W, ws = W == 8 ? 1 : 0, lw = ws ? 3 : 2;

    // ---- the tile's tap set: the union over the positions its row range touches (scalar code, the same in every wave)
    unsigned tmask = 0;
    {
        const int p_last = (min(row0 + BM, a.rows) - 1) / Mi;
        for (int p = row0 / Mi; p <= p_last; ++p) {
            const int q = pm_tab.order[ws][p];
            tmask |= pm_mask(q >> lw, q & (W - 1), W);
        }
    }
    auto next_live = [&](int tap) { const unsigned m = tmask >> (tap + 1); return m ? tap + 1 + __builtin_ctz(m) : 9; };
    // split-K: the parent's ranges of ORIGINAL K-steps; n = the live steps inside mine
    int ks_begin = 0, ks_end = ksteps;
    if (a.splitk > 1) {
        const int per = (ksteps + a.splitk - 1) / a.splitk;
        ks_begin = (int)blockIdx.y * per; ks_end = min(ksteps, ks_begin + per);
    }
    int n = 0;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
        if ((tmask >> tp) & 1u) n += max(0, min(ks_end, (tp + 1) * G) - max(ks_begin, tp * G));

    // ---- DMA geometry (as conv_sh_kernel): lane i owns slot g' = i & 15 of LDS row pair d, fetches piece g = g' ^ (d & 15)
    const int gs = (lane & 15) ^ ((4 * iw + (lane >> 4)) & 15);
    const int rl = 8 * iw + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
    int pix[APASS];                                              // pixel index of the (possibly padded) window origin
    unsigned vmask[APASS];                                       // bit (ky*3+kx): tap inside the image
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
        const int r = row0 + rl + RPP * i;
        vmask[i] = 0; pix[i] = 0;
        if (loader && r < a.rows) {
            const int pi = r / Mi, m = r - pi * Mi, q = pm_tab.order[ws][pi], y = q >> lw, x = q & (W - 1);
            pix[i] = (m * W + (y - 1)) * W + (x - 1);
            vmask[i] = pm_mask(y, x, W);
        }
    }
    const rsrc_t rs1 = make_rsrc(a.src1, (size_t)a.M * hw * a.C1 * 4);
    const rsrc_t rs2 = make_rsrc(a.src2 ? a.src2 : a.src1, a.src2 ? (size_t)a.M * hw * a.C2 * 4 : 0);
    const rsrc_t rsw = make_rsrc(a.wt, (size_t)a.Cout * ksteps * 128);
    int wbase[BPASS];
#pragma unroll
    for (int i = 0; i < BPASS; ++i) wbase[i] = (col0 + rl + RPP * i) * ksteps * 128 + pc16;

    // ---- issue side.  The K order is (tap, source, 32-channel group) over the LIVE taps; f_ks is the original K-step of the cursor (the weights' offset)
    int f_tap = 0, f_src = 0, f_gl = 0, f_ky = 0, f_kx = 0, f_gn = G1, f_ks = 0;
    int voff[APASS];
    auto refresh = [&]() {
        const int cs4 = (f_src ? a.C2 : a.C1) * 4;
        const int toff = (f_ky * W + f_kx) * cs4 + pc16;
#pragma unroll
        for (int i = 0; i < APASS; ++i)
            // (the range check of a raw buffer access sees the VGPR offset only and the origin of a padded window may lie
            //  before the tensor: the tap term is folded into the VGPR offset)
            voff[i] = ((vmask[i] >> f_tap) & 1u) ? pix[i] * cs4 + toff : (int)0x80000000;
    };
    auto seek = [&]() {                                           // the first live K-step at or behind ks_begin
        f_tap = ks_begin / G; int g = ks_begin - f_tap * G;
        if (f_tap > 8 || !((tmask >> f_tap) & 1u)) { f_tap = f_tap > 8 ? 9 : next_live(f_tap); g = 0; }
        f_ks = f_tap * G + g;
        f_src = g >= G1; f_gl = f_src ? g - G1 : g; f_gn = f_src ? G2 : G1;
        f_ky = f_tap / 3; f_kx = f_tap - f_ky * 3;
        refresh();
    };
    auto issue_a = [&](auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        unsigned char* sb = lds + SLOT * STAGE + iw * 1024;
        const int so = f_gl * 128;
        if (f_src) {
#pragma unroll
            for (int i = 0; i < APASS; ++i) dma16(rs2, sb + i * (1024 * LW), voff[i], so);
        } else {
#pragma unroll
            for (int i = 0; i < APASS; ++i) dma16(rs1, sb + i * (1024 * LW), voff[i], so);
        }
    };
    auto issue_b = [&](auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        unsigned char* sb = lds + SLOT * STAGE + iw * 1024;
#pragma unroll
        for (int i = 0; i < BPASS; ++i) dma16(rsw, sb + A_BYTES + i * (1024 * LW), wbase[i], f_ks * 128);
        ++f_ks;
        if (++f_gl == f_gn) {
            f_gl = 0;
            if (f_src == 0 && G2 > 0) { f_src = 1; f_gn = G2; }
            else {                                                // the next LIVE tap
                const int nt = next_live(f_tap);
                f_ks += (nt - f_tap - 1) * G;
                f_src = 0; f_gn = G1; f_tap = nt; f_ky = nt / 3; f_kx = nt - f_ky * 3;
            }
            refresh();
        }
    };
    auto issue = [&](auto slot_c) { issue_a(slot_c); issue_b(slot_c); };

    f16v acc[1][TN], acc1[1][TN];                                // acc = hi.hi, acc1 = hi.lo + lo.hi (scaled by 2^11)
#pragma unroll
    for (int j = 0; j < TN; ++j) { acc[0][j] = (f16v)(0.0f); acc1[0][j] = (f16v)(0.0f); }

    // fragment offsets (as conv_sh_kernel)
    int foa[4], fob[4];
    {
        const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
            foa[k] = f + wm * (BM / WM) * 128;
            fob[k] = f + A_BYTES + wn * (BN / WN) * 128;
        }
    }

    if (loader) {
        seek();
        [&]<int... S>(std::integer_sequence<int, S...>) {        // prologue: stages 0 .. NST-2 in flight
            ((S < n ? issue(std::integral_constant<int, S>()) : (void)0), ...);
        }(std::make_integer_sequence<int, NST - 1>());
    }
    auto pbarrier = [&]() {                                      // a phase boundary of the ping-pong schedule: nothing moves across it
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // (j: index among the block's n live steps; the schedule is conv_sh_kernel<.., PP>'s with ks_begin = 0, ks_end = n)
    if (loader) {
        auto lstep = [&](int j, auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            if (j + NST - 2 < n) wait_vm<(NST - 2) * LPS>();
            else                 wait_vm<0>();
            pbarrier();                                           // b_{j-1}: stage j has landed for everybody; group B is done with stage j-1
            if (j + NST - 1 < n) issue_a(std::integral_constant<int, (SLOT + NST - 1) % NST>());             // half of the pieces in each phase
            pbarrier();                                           // a_j
            if (j + NST - 1 < n) issue_b(std::integral_constant<int, (SLOT + NST - 1) % NST>());
        };
        int j = 0;
        for (; j + NST - 1 < n; j += NST) {
            [&]<int... S>(std::integer_sequence<int, S...>) { (lstep(j + S, std::integral_constant<int, S>()), ...); }
            (std::make_integer_sequence<int, NST>());
        }
        [&]<int... S>(std::integer_sequence<int, S...>) {
            ((j + S < n ? lstep(j + S, std::integral_constant<int, S>()) : (void)0), ...);
        }(std::make_integer_sequence<int, NST - 1>());
        pbarrier();                                               // b_{n-1}
        if (a.splitk <= 1 && a.dst_sh && !a.res_f32 && !a.post && a.epi_lds) __syncthreads();    // (the barrier in front of the LDS epilogue)
        return;
    }

    {
        const bool grp_b = wave >= NW / 2;                           // (wave-uniform) waves w and w + NW/2 share a SIMD
        h8v ah[2], al[2], bh[2][TN], bl[2][TN];
        auto reads = [&](auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            const unsigned char* sl = lds + SLOT * STAGE;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                ah[kc] = *reinterpret_cast<const h8v*>(sl + foa[kc]);
                if constexpr (!X1) al[kc] = *reinterpret_cast<const h8v*>(sl + foa[2 + kc]);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    bh[kc][j] = *reinterpret_cast<const h8v*>(sl + j * 4096 + fob[kc]);
                    if constexpr (!X1) bl[kc][j] = *reinterpret_cast<const h8v*>(sl + j * 4096 + fob[2 + kc]);
                }
            }
            wait_lds_reads();                                        // the fragments are in registers before the phase ends (the buffer may be refilled two phases later)
        };
        auto mfmas = [&]() {
            if constexpr (OMNI_PP_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], ah[kc], acc[0][j], 0, 0, 0);
                    if constexpr (!X1) {
                        acc1[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[kc][j], ah[kc], acc1[0][j], 0, 0, 0);
                        acc1[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], al[kc], acc1[0][j], 0, 0, 0);
                    }
                }
            if constexpr (OMNI_PP_PRIO) __builtin_amdgcn_s_setprio(0);
        };
        pbarrier();                                                  // b_{-1}: stage 0 has landed
        if (!grp_b) {
            auto stepa = [&](auto slot_c) {
                reads(slot_c);
                pbarrier();                                          // a_j
                mfmas();
                pbarrier();                                          // b_j
            };
            int j = 0;
            for (; j + NST - 1 < n; j += NST) {
                [&]<int... S>(std::integer_sequence<int, S...>) { (stepa(std::integral_constant<int, S>()), ...); }
                (std::make_integer_sequence<int, NST>());
            }
            [&]<int... S>(std::integer_sequence<int, S...>) {
                ((j + S < n ? stepa(std::integral_constant<int, S>()) : (void)0), ...);
            }(std::make_integer_sequence<int, NST - 1>());
        } else {
            auto stepb = [&](auto slot_c) {
                pbarrier();                                          // a_j
                reads(slot_c);
                pbarrier();                                          // b_j
                mfmas();
            };
            int j = 0;
            for (; j + NST - 1 < n; j += NST) {
                [&]<int... S>(std::integer_sequence<int, S...>) { (stepb(std::integral_constant<int, S>()), ...); }
                (std::make_integer_sequence<int, NST>());
            }
            [&]<int... S>(std::integer_sequence<int, S...>) {
                ((j + S < n ? stepb(std::integral_constant<int, S>()) : (void)0), ...);
            }(std::make_integer_sequence<int, NST - 1>());
        }
    }

    // ---- epilogue.  D = W x pixels: column (lane & 31) = GEMM row -> its pixel, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = channel
    if (a.splitk <= 1 && a.dst_sh && !a.res_f32 && !a.post && a.epi_lds) {
        static_assert(NW * 32 * (32 * TN + 4) * 4 <= NST * STAGE, "the transposition tiles must fit the K loop's buffers");
        wait_lds_reads();
        __syncthreads();                                          // every wave is done with the last stage
        float* tile = reinterpret_cast<float*>(lds) + wave * (32 * (32 * TN + 4));
        int c0[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) c0[j] = col0 + wn * (BN / WN) + j * 32;
        const int r0 = row0 + wm * (BM / WM);
        if (r0 < a.rows) pm_epilogue_tile_lds<TN, X1>(acc[0], acc1[0], a, r0, min(32, a.rows - r0), c0, lane, tile, Mi, hw, ws);
        return;
    }
    const int r = row0 + wm * (BM / WM) + (lane & 31);
    if (r >= a.rows) return;
    const int pi = r / Mi;
    const size_t pixel = (size_t)(r - pi * Mi) * hw + pm_tab.order[ws][pi];
    if (a.splitk > 1) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = col0 + wn * (BN / WN) + j * 32 + 8 * q + 4 * (lane >> 5);
                f4v v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[0][j][4 * q + e], acc[0][j][4 * q + e]);
                *reinterpret_cast<f4v*>(a.ws + ((size_t)blockIdx.y * a.rows + pixel) * a.Cout + c) = v;
            }
    } else if constexpr (TN > 1) {
        // twelve waves per block = a 168-register budget: one channel tile at a time
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const f16v ea[1] = {acc[0][j]}, eb[1] = {acc1[0][j]};
            const int cj[1] = {col0 + wn * (BN / WN) + j * 32};
            epilogue_row<1, 2, X1>(ea, eb, a, pixel, cj, lane, a.dst_sh != 0);
        }
    } else {
        const int c0[1] = {col0 + wn * (BN / WN)};
        epilogue_row<1, 4, X1>(acc[0], acc1[0], a, pixel, c0, lane, a.dst_sh != 0);
    }
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_pm)            // this translation unit's copy of the sticky range flag

int omni_conv_pm_launch(const void* args, int bn, bool x1, unsigned grid_x, unsigned grid_y, hipStream_t s)
{
    ShConvArgs a;
    memcpy(&a, args, sizeof(a));
    const dim3 grid(grid_x, grid_y), block(768);
    if (bn == 128 && !x1)     hipLaunchKernelGGL((conv_pm_sh_kernel<128, false>), grid, block, 0, s, a);
    else if (bn == 128)       hipLaunchKernelGGL((conv_pm_sh_kernel<128, true>), grid, block, 0, s, a);
    else if (bn == 64 && !x1) hipLaunchKernelGGL((conv_pm_sh_kernel<64, false>), grid, block, 0, s, a);
    else if (bn == 64)        hipLaunchKernelGGL((conv_pm_sh_kernel<64, true>), grid, block, 0, s, a);
    else OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv_pm_launch: no conv_pm_sh_kernel<" + std::to_string(bn) + ">");      // a programming error, not a user error
    return OMNI_OK;
}
