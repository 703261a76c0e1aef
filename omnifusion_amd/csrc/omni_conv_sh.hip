// omni_conv_sh.hip — the im2col tile kernel of the split-half convolution (conv_sh_kernel), the kernel choice of omni_conv2d_sh_f16x3_ws, the split-K
// reducers and the fp32 <-> SH converters.  The SH layout, the LDS image and the shared device helpers: omni_conv_sh_common.h.  The other kernel families:
// omni_conv_halo.hip (3x3 with halo reuse; the stem), omni_conv_up2.hip (up-sampling + heads), omni_gemm_rows.hip.
// The experimental Winograd path is conv_sh_kernel<.., WINO> (an instantiation of the template below) plus ONE block at the end of this file.
#include "omni_conv_sh_common.h"

namespace {

// NL > 0: NL extra LOADER waves issue every LDS-DMA piece of the block and wait for them; the WM x WN matrix waves never touch vector memory
// inside the K loop (a piece costs the issuing wave 100-185 cycles between matrix instructions: four pieces per K-step against twelve
// matrix instructions of 32).  Same pieces, same LDS image, same K order: same bits.
//
// PP ("ping-pong", round 6; needs loader waves and 8 matrix waves): the two matrix waves of a SIMD (waves w and w + 4: a block's waves go to the four SIMDs
// in turn) run in ANTI-PHASE.  With one barrier per K-step all eight matrix waves start their fragment reads together — nobody has operands, the matrix
// pipes idle ~350 cycles — and then the two waves of a SIMD run their 12 matrix instructions one after the other: 1 150 cycles per step for 768 of
// matrix work (tools/tile_stamps.py, profiles/r05j_halo_stamps.txt).  Here a K-step is TWO phases behind two barriers: in phase a_k group A (waves 0-3)
// issues its 12 matrix instructions of step k while group B (waves 4-7) reads its fragments of step k; in phase b_k B computes step k and A reads step
// k+1.  Every SIMD's matrix pipe has work in every phase, the LDS port serves four waves' reads (48 KiB) under 384 cycles of matrix work.
//      group A:  b_{k-1} | reads(k)  wait | a_k | mfma(k)          | b_k | reads(k+1) ...
//      group B:  b_{k-1} | mfma(k-1)      | a_k | reads(k)   wait  | b_k | mfma(k)    ...
//      loaders:  wait(stage k landed) | b_{k-1} | issue stage k+NST-1 -> the slot of stage k-1 (B's reads of it ended in front of b_{k-1}) | a_k | ...
// Same pieces, same LDS image, same fragments, same order of the matrix instructions on every accumulator: same bits.
//
// WINO (round 6, experimental): the multiply stage AND the output transform of Winograd F(2x2, 3x3).  The "image" is the transformed input V [16 positions][tiles][C]
// (omni_wino_input_sh), a row of the GEMM is a 2 x 2 output TILE, the K order is (position p, 32-channel group) — sixteen taps whose pixel offset is p * tiles —,
// the weights are U_p = (G g G^T)[p] in the ordinary f16x3 split.  A wave (32 tiles x 32 channels: TM = TN = 1) keeps the four outputs of its tiles in registers:
// when a position's last K-step has been issued, M_p = acc + 2^-11 acc1 is folded into Y[i][j] += A^T[i][xi] A^T[j][nu] M_p (coefficients 0 / +1 / -1) and the
// accumulators start the next position from zero — 16 matrix products per four output pixels instead of 36.  splitk divides the POSITIONS.
// (its input transform and entry points: the Winograd block at the end of this file)
__constant__ float wino_coef[16][4] = {                        // [p = 4 xi + nu][o = 2 i + j] = A^T[i][xi] * A^T[j][nu],  A^T = [[1, 1, 1, 0], [0, 1, -1, -1]]
    {1, 0, 0, 0}, {1, 1, 0, 0}, {1, -1, 0, 0}, {0, -1, 0, 0},
    {1, 0, 1, 0}, {1, 1, 1, 1}, {1, -1, 1, -1}, {0, -1, 0, -1},
    {1, 0, -1, 0}, {1, 1, -1, -1}, {1, -1, -1, 1}, {0, -1, 0, 1},
    {0, 0, -1, 0}, {0, 0, -1, -1}, {0, 0, -1, 1}, {0, 0, 0, 1}};
template <int BM, int BN, int WM, int WN, int NST = 3, int NL = 0, bool PP = false, bool WINO = false, bool X1 = false>   // NST stages in flight (the step loop is unrolled by it); X1: f16x1 (acc_join)
__global__ __launch_bounds__(64 * (WM * WN + NL)) void conv_sh_kernel(ShConvArgs a)
{
    static_assert(!(WINO && X1), "Winograd: f16x3 only");
    static_assert(!PP || (NL > 0 && WM * WN == 8 && NST >= 3), "ping-pong: eight matrix waves (two per SIMD) + loader waves, three stages");
    static_assert(!WINO || (PP && BM / WM == 32 && BN / WN == 32), "Winograd: the ping-pong kernel with 32 x 32 wave tiles");
    constexpr int NW = WM * WN, LW = NL > 0 ? NL : NW, RPP = 8 * LW;   // matrix waves; waves that issue DMA; tile rows covered by one DMA pass of the block
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;         // 32x32 tiles per wave (waves WM x WN)
    constexpr int APASS = BM / RPP, BPASS = BN / RPP, LPS = APASS + BPASS;
    static_assert(APASS >= 1 && BPASS >= 1, "a tile side must cover at least one DMA pass");
    constexpr int A_BYTES = BM * 128, STAGE = (BM + BN) * 128;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NST * STAGE];
    // (ablation 32768, tools/tile_stamps.py: s_memtime of matrix wave 0 and of the first loader wave of block 0 around the parts of its first 28 K steps, dumped to a.ws)
    __shared__ long long cst[OMNI_ABL(32768) ? 256 : 1];
    const bool stamped = OMNI_ABL(32768) && blockIdx.x == 0 && blockIdx.y == 0 && a.ws != nullptr && a.splitk <= 1;
    auto cstamp = [&](int k) { if (OMNI_ABL(32768) && stamped && (threadIdx.x & 63) == 0 && k < 256) cst[k] = clock64(); };
    auto cdump = [&]() { if (OMNI_ABL(32768) && stamped && threadIdx.x == 0) for (int i = 0; i < 256; ++i) reinterpret_cast<long long*>(a.ws)[i] = cst[i]; };
    if (threadIdx.x == 0) cstamp(0);

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    const int wm = wave / WN, wn = wave % WN;
    const bool loader = NL > 0 && wave >= NW;                   // (wave-uniform)
    const int iw = NL > 0 ? wave - NW : wave;                   // index among the issuing waves (meaningless in a matrix wave when NL > 0)
    const int ntn = a.Cout / BN;
    // XCD-aware order: hardware block b runs on XCD b % 8; give each XCD a contiguous range of (tile_m, tile_n) so that the
    // blocks sharing an A row tile (and neighbouring pixels) share one L2
    // (wt_major — the WEIGHTS are the larger operand: layer4's 9.4 MB against 4.7 MB of pixels, the transformer's matrices against 144 token
    //  rows — an XCD gets a range of output-channel tiles instead and fetches 1/8 of the weights rather than all of them; same tiles, same bits)
    const int ntm = (a.rows + BM - 1) / BM;
    const unsigned lb = a.noxcd ? blockIdx.x : omni_xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = a.wt_major ? (int)(lb % (unsigned)ntm) : (int)(lb / (unsigned)ntn), tile_n = a.wt_major ? (int)(lb / (unsigned)ntm) : (int)(lb % (unsigned)ntn);
    const int row0 = tile_m * BM, col0 = tile_n * BN;
    const int G1 = a.C1 >> 5, G2 = a.C2 >> 5, G = G1 + G2;
    const int ksteps = a.KH * a.KW * G;

    // ---- DMA geometry: instruction j of a tile covers LDS row pairs 4j .. 4j+3; wave w issues j = w, w+NW, ...  Lane i
    // owns slot g' = i & 15 of pair d = 4j + (i >> 4), i.e. fetches piece g = g' ^ (d & 15) -> row 2d + (g >> 3), 16-byte
    // piece g & 7.  (d & 15 does not depend on the pass, so the lane's piece is fixed and its row advances by 8 NW per pass.)
    const int gs = (lane & 15) ^ ((4 * iw + (lane >> 4)) & 15);
    const int rl = 8 * iw + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
    int pix[APASS];                                              // pixel index of the (possibly padded) window origin
    unsigned vmask[APASS];                                       // bit (ky*KW+kx): tap inside the image
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
        const int r = row0 + rl + RPP * i;
        vmask[i] = 0; pix[i] = 0;
        if constexpr (WINO) {
            if ((NL == 0 || loader) && r < a.rows) { pix[i] = r; vmask[i] = 0xffffu; }      // row = tile; tap p = position: offset p * tiles (a.W), always "inside"
        } else
        if ((NL == 0 || loader) && r < a.rows) {
            const int hw = a.Ho * a.Wo;
            const int m = r / hw, rem = r - m * hw;
            const int oy = (rem / a.Wo) * a.stride - a.pad, ox = (rem % a.Wo) * a.stride - a.pad;
            pix[i] = (m * a.H + oy) * a.W + ox;
            unsigned vm = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    if (ky < a.KH && kx < a.KW && (unsigned)(oy + ky) < (unsigned)a.H && (unsigned)(ox + kx) < (unsigned)a.W)
                        vm |= 1u << (ky * a.KW + kx);
            vmask[i] = vm;
        }
    }
    const rsrc_t rs1 = make_rsrc(a.src1, (size_t)a.M * a.H * a.W * a.C1 * 4);
    const rsrc_t rs2 = make_rsrc(a.src2 ? a.src2 : a.src1, a.src2 ? (size_t)a.M * a.H * a.W * a.C2 * 4 : 0);
    const rsrc_t rsw = make_rsrc(a.wt, (size_t)a.Cout * ksteps * 128);
    int wbase[BPASS];
#pragma unroll
    for (int i = 0; i < BPASS; ++i) wbase[i] = (col0 + rl + RPP * i) * ksteps * 128 + pc16;

    // ---- issue side.  The K order is (tap, source, 32-channel group); everything that depends on the lane is recomputed
    // only when (tap, source) changes — voff[i] = byte offset of this lane's piece for group 0, or out of range for a tap
    // outside the image — so that a K-step costs one scalar offset and LPS DMA instructions, nothing per lane.  (The matrix
    // pipe retires one MFMA per 32 cycles per SIMD, in which a SIMD has 8 issue slots: a loop with ~20 scalar/vector
    // instructions per MFMA, as the first version of this kernel had, is issue-bound at ~30 % of the MFMA rate.)
    int f_tap = 0, f_src = 0, f_gl = 0, f_ky = 0, f_kx = 0, f_gn = G1;
    int voff[APASS];
    auto refresh = [&]() {
        const int cs4 = (f_src ? a.C2 : a.C1) * 4;
        const int toff = (f_ky * a.W + f_kx) * cs4 + pc16;
#pragma unroll
        for (int i = 0; i < APASS; ++i)
            // (the range check of a raw buffer access sees the VGPR offset only and the origin of a padded window may lie
            //  before the tensor: the tap term is folded into the VGPR offset)
            voff[i] = ((vmask[i] >> f_tap) & 1u) ? pix[i] * cs4 + toff : (int)0x80000000;
    };
    auto seek = [&](int ks) {
        f_tap = ks / G; const int g = ks - f_tap * G;
        f_src = g >= G1; f_gl = f_src ? g - G1 : g; f_gn = f_src ? G2 : G1;
        f_ky = f_tap / a.KW; f_kx = f_tap - f_ky * a.KW;
        refresh();
    };
    // (a stage's pieces in two parts — the pixel operand, then the weights and the step to the next (tap, source, group) — so that the ping-pong schedule
    //  can spread them over its two phases: 32 KiB per K-step through the CU's address path take ~500 cycles, more than one phase's 384 of matrix work)
    auto issue_a = [&](auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        unsigned char* sb = lds + SLOT * STAGE + iw * 1024;
        const int so = f_gl * 128;
        if (OMNI_ABL(128)) {}                                  // (ablation: no operand traffic)
        else if (f_src) {
#pragma unroll
            for (int i = 0; i < APASS; ++i) dma16(rs2, sb + i * (1024 * LW), voff[i], so);
        } else {
#pragma unroll
            for (int i = 0; i < APASS; ++i) dma16(rs1, sb + i * (1024 * LW), voff[i], so);
        }
    };
    auto issue_b = [&](int ks, auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        unsigned char* sb = lds + SLOT * STAGE + iw * 1024;
        if (!OMNI_ABL(128)) {
#pragma unroll
            for (int i = 0; i < BPASS; ++i) dma16(rsw, sb + A_BYTES + i * (1024 * LW), wbase[i], ks * 128);
        }
        if (++f_gl == f_gn) {
            f_gl = 0;
            if (f_src == 0 && G2 > 0) { f_src = 1; f_gn = G2; }
            else { f_src = 0; f_gn = G1; ++f_tap; if (++f_kx == a.KW) { f_kx = 0; ++f_ky; } }
            refresh();
        }
    };
    auto issue = [&](int ks, auto slot_c) { issue_a(slot_c); issue_b(ks, slot_c); };

    f16v acc[TM][TN], acc1[TM][TN];                              // acc = hi.hi, acc1 = hi.lo + lo.hi (scaled by 2^11)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) { acc[i][j] = (f16v)(0.0f); acc1[i][j] = (f16v)(0.0f); }

    // fragment offsets: row lane&31 of a 32-row tile, piece p = 2k + (lane>>5): k = 0,1 hi of the two 16-wide k chunks, 2,3 lo;
    // the wave's tile origin is folded in, the stage offset is an immediate of the unrolled step
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

    int ks_begin = 0, ks_end = ksteps;
    if (a.splitk > 1) {
        const int per = (ksteps + a.splitk - 1) / a.splitk;
        ks_begin = (int)blockIdx.y * per; ks_end = min(ksteps, ks_begin + per);
    }
    if (NL == 0 || loader) {
        seek(ks_begin);
        [&]<int... S>(std::integer_sequence<int, S...>) {        // prologue: stages 0 .. NST-2 in flight
            ((ks_begin + S < ks_end ? issue(ks_begin + S, std::integral_constant<int, S>()) : (void)0), ...);
        }(std::make_integer_sequence<int, NST - 1>());
    }
    auto pbarrier = [&]() {                                      // a phase boundary of the ping-pong schedule: nothing moves across it
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    if (loader) {
        if constexpr (PP) {
            auto lstep = [&](int ks, auto slot_c) {
                constexpr int SLOT = decltype(slot_c)::value;
                const int sk_ = 128 + 4 * (ks - ks_begin);
                if (wave == NW && ks - ks_begin < 28) cstamp(sk_);
                if (ks + NST - 2 < ks_end) wait_vm<(NST - 2) * LPS>();
                else                       wait_vm<0>();
                if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 1);
                pbarrier();                                       // b_{k-1}: stage ks has landed for everybody; group B is done with stage ks-1
                if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 2);
                if (ks + NST - 1 < ks_end) issue_a(std::integral_constant<int, (SLOT + NST - 1) % NST>());             // half of the pieces in each phase
                if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 3);
                pbarrier();                                       // a_k
                if (ks + NST - 1 < ks_end) issue_b(ks + NST - 1, std::integral_constant<int, (SLOT + NST - 1) % NST>());
            };
            int ks = ks_begin;
            for (; ks + NST - 1 < ks_end; ks += NST) {
                [&]<int... S>(std::integer_sequence<int, S...>) { (lstep(ks + S, std::integral_constant<int, S>()), ...); }
                (std::make_integer_sequence<int, NST>());
            }
            [&]<int... S>(std::integer_sequence<int, S...>) {
                ((ks + S < ks_end ? lstep(ks + S, std::integral_constant<int, S>()) : (void)0), ...);
            }(std::make_integer_sequence<int, NST - 1>());
            pbarrier();                                           // b_{n-1}
            if (!WINO && a.splitk <= 1 && a.dst_sh && !a.res_f32 && !a.post && a.epi_lds) __syncthreads();    // (the barrier in front of the LDS epilogue)
            return;
        }
        // ---- a loader wave's K loop: my pieces of stage ks have landed -> barrier (everybody's have; the matrix waves are done with stage
        // ks-1) -> the pieces of stage ks+NST-1 into the slot stage ks-1 occupied
        auto lstep = [&](int ks, auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            const int sk_ = 128 + 4 * (ks - ks_begin);
            if (wave == NW && ks - ks_begin < 28) cstamp(sk_);
            if (ks + NST - 2 < ks_end) wait_vm<(NST - 2) * LPS>();
            else                       wait_vm<0>();
            if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 1);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 2);
            if (ks + NST - 1 < ks_end) issue(ks + NST - 1, std::integral_constant<int, (SLOT + NST - 1) % NST>());
            if (wave == NW && ks - ks_begin < 28) cstamp(sk_ + 3);
        };
        int ks = ks_begin;
        for (; ks + NST - 1 < ks_end; ks += NST) {
            [&]<int... S>(std::integer_sequence<int, S...>) { (lstep(ks + S, std::integral_constant<int, S>()), ...); }
            (std::make_integer_sequence<int, NST>());
        }
        [&]<int... S>(std::integer_sequence<int, S...>) {
            ((ks + S < ks_end ? lstep(ks + S, std::integral_constant<int, S>()) : (void)0), ...);
        }(std::make_integer_sequence<int, NST - 1>());
        if (a.splitk <= 1 && a.dst_sh && !a.res_f32 && !a.post && a.epi_lds) __syncthreads();    // (the barrier in front of the LDS epilogue)
        return;
    }

    if constexpr (PP) {
        const bool grp_b = wave >= NW / 2;                           // (wave-uniform) waves w and w + NW/2 share a SIMD
        h8v ah[2][TM], al[2][TM], bh[2][TN], bl[2][TN];
        auto reads = [&](auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            const unsigned char* sl = lds + SLOT * STAGE;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    ah[kc][i] = *reinterpret_cast<const h8v*>(sl + i * 4096 + foa[kc]);
                    if constexpr (!X1) al[kc][i] = *reinterpret_cast<const h8v*>(sl + i * 4096 + foa[2 + kc]);
                }
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
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], ah[kc][i], acc[i][j], 0, 0, 0);
                        if constexpr (!X1) {
                            acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[kc][j], ah[kc][i], acc1[i][j], 0, 0, 0);
                            acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], al[kc][i], acc1[i][j], 0, 0, 0);
                        }
                    }
            if constexpr (OMNI_PP_PRIO) __builtin_amdgcn_s_setprio(0);
        };
        f16v Y[WINO ? 4 : 1];
        int wino_g = 0, wino_p = ks_begin / (G > 0 ? G : 1);        // K-steps issued of the current position; the position
        if constexpr (WINO) {
#pragma unroll
            for (int o = 0; o < 4; ++o) Y[o] = (f16v)(0.0f);
        }
        auto wino_fold = [&]() {                                     // behind a K-step's matrix instructions: the position's last?  fold it into the four outputs
            if constexpr (WINO) {
                if (++wino_g < G) return;
                wino_g = 0;
                f16v m;
#pragma unroll
                for (int e = 0; e < 16; ++e) m[e] = fmaf(acc1[0][0][e], 4.8828125e-4f, acc[0][0][e]);
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const float c = wino_coef[wino_p][o];            // (wave-uniform: a scalar load)
                    if (c != 0.0f) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) Y[o][e] = fmaf(c, m[e], Y[o][e]);
                    }
                }
                acc[0][0] = (f16v)(0.0f); acc1[0][0] = (f16v)(0.0f);
                ++wino_p;
            }
        };
        pbarrier();                                                  // b_{-1}: stage ks_begin has landed
        if (!grp_b) {
            auto stepa = [&](int ks, auto slot_c) {
                if (wave == 0 && ks - ks_begin < 28) cstamp(8 + 4 * (ks - ks_begin));
                reads(slot_c);
                if (wave == 0 && ks - ks_begin < 28) cstamp(11 + 4 * (ks - ks_begin));
                pbarrier();                                          // a_k
                if (wave == 0 && ks - ks_begin < 28) cstamp(9 + 4 * (ks - ks_begin));
                mfmas();
                wino_fold();
                if (wave == 0 && ks - ks_begin < 28) cstamp(10 + 4 * (ks - ks_begin));
                pbarrier();                                          // b_k
            };
            int ks = ks_begin;
            for (; ks + NST - 1 < ks_end; ks += NST) {
                [&]<int... S>(std::integer_sequence<int, S...>) { (stepa(ks + S, std::integral_constant<int, S>()), ...); }
                (std::make_integer_sequence<int, NST>());
            }
            [&]<int... S>(std::integer_sequence<int, S...>) {
                ((ks + S < ks_end ? stepa(ks + S, std::integral_constant<int, S>()) : (void)0), ...);
            }(std::make_integer_sequence<int, NST - 1>());
        } else {
            auto stepb = [&](int ks, auto slot_c) {
                pbarrier();                                          // a_k
                reads(slot_c);
                pbarrier();                                          // b_k
                mfmas();
                wino_fold();
            };
            int ks = ks_begin;
            for (; ks + NST - 1 < ks_end; ks += NST) {
                [&]<int... S>(std::integer_sequence<int, S...>) { (stepb(ks + S, std::integral_constant<int, S>()), ...); }
                (std::make_integer_sequence<int, NST>());
            }
            [&]<int... S>(std::integer_sequence<int, S...>) {
                ((ks + S < ks_end ? stepb(ks + S, std::integral_constant<int, S>()) : (void)0), ...);
            }(std::make_integer_sequence<int, NST - 1>());
        }
        if constexpr (WINO) {
            // ---- the four output pixels of my tile (column lane & 31): tile -> (image, tile row, tile column) -> pixel (2 ty + i, 2 tx + j); per register quad the
            // lane holds four consecutive channels, as in every other epilogue.  splitk > 1 (the positions were divided): raw partial outputs to the workspace,
            // pixel-major like every split-K launch, for sh_splitk_reduce_kernel.
            const int tl = row0 + wm * (BM / WM) + (lane & 31);
            if (tl >= a.rows) return;
            const int per_img = a.wino_th * a.wino_tw, m = tl / per_img, rem = tl - m * per_img, ty = rem / a.wino_tw, tx = rem - ty * a.wino_tw;
            const int cj[1] = {col0 + wn * (BN / WN)};
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const size_t r = ((size_t)m * a.Ho + 2 * ty + (o >> 1)) * a.Wo + 2 * tx + (o & 1);
                if (a.splitk > 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f4v v; v.x = Y[o][4 * q]; v.y = Y[o][4 * q + 1]; v.z = Y[o][4 * q + 2]; v.w = Y[o][4 * q + 3];
                        *reinterpret_cast<f4v*>(a.ws + ((size_t)blockIdx.y * a.wino_pix + r) * a.Cout + cj[0] + 8 * q + 4 * (lane >> 5)) = v;
                    }
                } else {
                    const f16v ea[1] = {Y[o]}, eb[1] = {(f16v)(0.0f)};
                    epilogue_row<1, 2>(ea, eb, a, r, cj, lane, a.dst_sh != 0);
                }
            }
            return;
        }
    }
    auto step = [&](int ks, auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        // my pieces of stage ks have landed when at most the NST-2 younger stages are in flight (near the end fewer were issued:
        // a smaller count only waits longer, 0 is always safe)
        if (NL == 0) {
            if (ks + NST - 2 < ks_end) wait_vm<(NST - 2) * LPS>();
            else                       wait_vm<0>();
        }
        if (wave == 0 && ks - ks_begin < 28) cstamp(8 + 4 * (ks - ks_begin));
        wait_lds_reads();                                        // my fragment reads of stage ks-1 have returned ...
        if (!OMNI_ABL(256)) __builtin_amdgcn_s_barrier();     // ... everybody's pieces have landed; everybody is done reading stage ks-1
        asm volatile("" ::: "memory");
        if (wave == 0 && ks - ks_begin < 28) cstamp(9 + 4 * (ks - ks_begin));
        const unsigned char* sl = lds + SLOT * STAGE;
        h8v ah[2][TM], al[2][TM], bh[2][TN], bl[2][TN];
        if (OMNI_ABL(512)) {                                  // (ablation: no fragment reads)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
                for (int i = 0; i < TM; ++i) { ah[kc][i] = (h8v)((_Float16)1.0f); al[kc][i] = ah[kc][i]; }
#pragma unroll
                for (int j = 0; j < TN; ++j) { bh[kc][j] = (h8v)((_Float16)1.0f); bl[kc][j] = bh[kc][j]; }
            }
        } else
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[kc][i] = *reinterpret_cast<const h8v*>(sl + i * 4096 + foa[kc]);
                if constexpr (!X1) al[kc][i] = *reinterpret_cast<const h8v*>(sl + i * 4096 + foa[2 + kc]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[kc][j] = *reinterpret_cast<const h8v*>(sl + j * 4096 + fob[kc]);
                if constexpr (!X1) bl[kc][j] = *reinterpret_cast<const h8v*>(sl + j * 4096 + fob[2 + kc]);
            }
        }
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (!OMNI_ABL(64) && !OMNI_DBG(a, 64)) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], ah[kc][i], acc[i][j], 0, 0, 0);
                    else { acc[i][j][0] += (float)bh[kc][j][0] * (float)ah[kc][i][0]; }
                    if constexpr (!X1) {
                        if (!OMNI_ABL(16) && !OMNI_DBG(a, 16)) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[kc][j], ah[kc][i], acc1[i][j], 0, 0, 0);   // precision map: weight-lo term
                        if (!OMNI_ABL(32) && !OMNI_DBG(a, 32)) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[kc][j], al[kc][i], acc1[i][j], 0, 0, 0);   // ... activation-lo term
                    }
                }
            if (kc == 0) {                                       // stage ks+NST-1, issued under the first half's matrix work
                __builtin_amdgcn_sched_barrier(0);
                if (NL == 0 && ks + NST - 1 < ks_end) issue(ks + NST - 1, std::integral_constant<int, (SLOT + NST - 1) % NST>());
            }
        }
    };
    if constexpr (!PP) {
        int ks = ks_begin;
        for (; ks + NST - 1 < ks_end; ks += NST) {               // (no early exits inside: they would park the accumulators in VGPRs)
            [&]<int... S>(std::integer_sequence<int, S...>) { (step(ks + S, std::integral_constant<int, S>()), ...); }
            (std::make_integer_sequence<int, NST>());
        }
        [&]<int... S>(std::integer_sequence<int, S...>) {        // remainder: up to NST-1 steps
            ((ks + S < ks_end ? step(ks + S, std::integral_constant<int, S>()) : (void)0), ...);
        }(std::make_integer_sequence<int, NST - 1>());
    }

    if (wave == 0) cstamp(1);                                     // K loop issued
    if (OMNI_ABL(4) || OMNI_DBG(a, 4)) return;
    // ---- epilogue.  D = W x pixels: column (lane & 31) = pixel, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = channel
    if (a.splitk <= 1 && a.dst_sh && !a.res_f32 && !a.post && a.epi_lds) {       // (`post`: only the halo kernel takes it through LDS — the registers it costs would spill here) split-half output: through LDS, 16-byte pieces (epilogue_tile_lds)
        static_assert(NW * 32 * (32 * TN + 4) * 4 <= NST * STAGE, "the transposition tiles must fit the K loop's buffers");
        wait_lds_reads();
        __syncthreads();                                          // every wave is done with the last stage
        float* tile = reinterpret_cast<float*>(lds) + wave * (32 * (32 * TN + 4));
        int c0[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) c0[j] = col0 + wn * (BN / WN) + j * 32;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int r0 = row0 + wm * (BM / WM) + i * 32;
            if (r0 < a.rows) epilogue_tile_lds<TN, false, X1>(acc[i], acc1[i], a, (size_t)r0, min(32, a.rows - r0), c0, lane, tile);
            if (i + 1 < TM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // (the tile is read back before it is written again)
        }
        if (OMNI_ABL(32768)) { if (wave == 0) cstamp(2); __syncthreads(); cdump(); }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = row0 + wm * (BM / WM) + i * 32 + (lane & 31);
        if (r >= a.rows) continue;
        if (a.splitk > 1) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = col0 + wn * (BN / WN) + j * 32 + 8 * q + 4 * (lane >> 5);
                    f4v v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[i][j][4 * q + e], acc[i][j][4 * q + e]);
                    *reinterpret_cast<f4v*>(a.ws + ((size_t)blockIdx.y * a.rows + r) * a.Cout + c) = v;
                }
        } else {
            if constexpr (NL > 0 && TN > 1) {
                // twelve waves per block = a 168-register budget: one channel tile at a time (4 instead of 4 TN bias / residual quads in flight)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const f16v ea[1] = {acc[i][j]}, eb[1] = {acc1[i][j]};
                    const int cj[1] = {col0 + wn * (BN / WN) + j * 32};
                    epilogue_row<1, 2, X1>(ea, eb, a, (size_t)r, cj, lane, a.dst_sh != 0);
                }
            } else {
                int c0[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) c0[j] = col0 + wn * (BN / WN) + j * 32;
                epilogue_row<TN, 4, X1>(acc[i], acc1[i], a, (size_t)r, c0, lane, a.dst_sh != 0);
            }
        }
    }
}

// dst = act(sum_s ws[s] + bias + res): the deterministic second pass of a split-K launch (4 channels per thread)
__global__ __launch_bounds__(256) void sh_splitk_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ bias,
                                                               const void* __restrict__ res, void* __restrict__ dst,
                                                               size_t n4, int Cout, int splitk, size_t slab, int act, int dst_sh, int res_f32)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const size_t o = i * 4;
    f4v v = *reinterpret_cast<const f4v*>(ws + o);
    for (int s = 1; s < splitk; ++s) v += *reinterpret_cast<const f4v*>(ws + (size_t)s * slab + o);
    splitk_finish(v, o, bias, res, dst, Cout, act, dst_sh, res_f32);
}

// The same second pass for the transformer's fc2 (model/blocks.py:83-88: x = x + mlp(norm2(x)), then the next block's norm1 / encoder_norm) with the
// LayerNorm that follows it anyway in the same kernel: tok = sum_s ws[s] + bias + res (fp32, written: it is the next residual) and y = LayerNorm(tok)
// (SH: the next GEMM's operand, or fp32: encoder_norm).  One wave per row of 512; element for element the operations of sh_splitk_reduce_kernel
// followed by layernorm512_kernel (omni_net.hip) in their order: the bits of the two launches.
template <bool SH>
__global__ __launch_bounds__(256) void sh_splitk_reduce_ln512_kernel(const float* __restrict__ ws, const float* __restrict__ bias, const float* __restrict__ res,
                                                                     float* __restrict__ tok, const float* __restrict__ g, const float* __restrict__ b,
                                                                     void* __restrict__ y, int rows, int splitk, size_t slab, float eps)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t o = (size_t)row * 512;
    f4v v0 = *reinterpret_cast<const f4v*>(ws + o + lane * 4), v1 = *reinterpret_cast<const f4v*>(ws + o + 256 + lane * 4);
    for (int s = 1; s < splitk; ++s) {
        v0 += *reinterpret_cast<const f4v*>(ws + (size_t)s * slab + o + lane * 4);
        v1 += *reinterpret_cast<const f4v*>(ws + (size_t)s * slab + o + 256 + lane * 4);
    }
    if (bias) { v0 += *reinterpret_cast<const f4v*>(bias + lane * 4); v1 += *reinterpret_cast<const f4v*>(bias + 256 + lane * 4); }
    if (res) { v0 += *reinterpret_cast<const f4v*>(res + o + lane * 4); v1 += *reinterpret_cast<const f4v*>(res + o + 256 + lane * 4); }
    *reinterpret_cast<f4v*>(tok + o + lane * 4) = v0; *reinterpret_cast<f4v*>(tok + o + 256 + lane * 4) = v1;
    float sum = (v0.x + v0.y) + (v0.z + v0.w) + (v1.x + v1.y) + (v1.z + v1.w);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    const float mean = sum * (1.0f / 512.0f);
    v0 -= mean; v1 -= mean;
    float q = (v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w) + (v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) q += __shfl_xor(q, d);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 512.0f) + eps);
    const f4v g0 = *reinterpret_cast<const f4v*>(g + lane * 4), g1 = *reinterpret_cast<const f4v*>(g + 256 + lane * 4);
    const f4v b0 = *reinterpret_cast<const f4v*>(b + lane * 4), b1 = *reinterpret_cast<const f4v*>(b + 256 + lane * 4);
    act_store4<SH>(y, o + lane * 4, v0 * rstd * g0 + b0);
    act_store4<SH>(y, o + 256 + lane * 4, v1 * rstd * g1 + b1);
}

// fp32 NHWC <-> SH (4 channels per thread)
__global__ __launch_bounds__(256) void sh_from_f32_kernel(const float* __restrict__ src, void* __restrict__ dst, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    h4v hi, lo; sh_split4(*reinterpret_cast<const f4v*>(src + i * 4), hi, lo);
    unsigned char* dp = (unsigned char*)dst + sh_off(i * 4);
    *reinterpret_cast<h4v*>(dp) = hi; *reinterpret_cast<h4v*>(dp + 64) = lo;
}
__global__ __launch_bounds__(256) void sh_to_f32_kernel(const void* __restrict__ src, float* __restrict__ dst, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const unsigned char* sp = (const unsigned char*)src + sh_off(i * 4);
    *reinterpret_cast<f4v*>(dst + i * 4) = sh_join4(*reinterpret_cast<const h4v*>(sp), *reinterpret_cast<const h4v*>(sp + 64));
}

}  // namespace

// out[M,Ho,Wo,Cout] = act(conv(src1 ++ src2, wt16) + bias + res) with SH activations (see the file header).
// src1/src2: SH tensors; fmt bit 0: dst is SH (else fp32 NHWC); fmt bit 1: res is fp32 NHWC (else SH); fmt bit 2: latency form (few images: the im2col
// tile kernel also where the halo kernel for small images would be taken; equal to it up to the K summation order); wt16 as for
// omni_conv2d_nhwc_f16x3_ws.  A plain GEMM is the case H = W = KH = KW = 1 (rows = M).
// Requirements: C1, C2, Cout multiples of 32, kernels up to 3x3.  split-K as in omni_conv2d_nhwc_f32_ws.
// `post` (or null): fp32 [post_elems / Cout][Cout] added after the activation, output row index modulo its row count — layer1 + point_feat
// (model/spherical_model.py:258) inside layer1's last convolution instead of a pass of its own.  Not with split-K.
static int conv2d_sh_impl(const void* src1, const void* src2, const void* wt16, const float* bias,
                          const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                          int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                          const float* post, size_t post_elems, omni_stream_t stream, bool reduce = true);
extern "C" int omni_conv2d_sh_f16x3_ws(const void* src1, const void* src2, const void* wt16, const float* bias,
                                       const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                                       int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                                       omni_stream_t stream)
{
    return conv2d_sh_impl(src1, src2, wt16, bias, res, dst, fmt, M, H, W, C1, C2, Cout, KH, KW, stride, pad, act, splitk, ws, ws_bytes,
                          nullptr, 0, stream);
}
extern "C" int omni_conv2d_sh_f16x3_post_ws(const void* src1, const void* src2, const void* wt16, const float* bias,
                                            const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                                            int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                                            const float* post, size_t post_elems, omni_stream_t stream)
{
    return conv2d_sh_impl(src1, src2, wt16, bias, res, dst, fmt, M, H, W, C1, C2, Cout, KH, KW, stride, pad, act, splitk, ws, ws_bytes,
                          post, post_elems, stream);
}
// A split-K GEMM with 512 output columns (the transformer's fc2) whose second pass also applies the LayerNorm that follows: tok [rows,512] fp32 =
// x . wt16^T + bias + res (res fp32 [rows,512], may alias nothing), y = LayerNorm(tok; ln_g, ln_b, eps) as SH (fmt bit 0) or fp32.  splitk >= 2 (the
// caller's plan); one launch fewer per transformer layer than omni_conv2d_sh_f16x3_ws + omni_layernorm512_*, the same bits.
extern "C" int omni_gemm_sh_f16x3_ln512_ws(const void* x, const void* wt16, const float* bias, const float* res, float* tok, const float* ln_g, const float* ln_b,
                                           float eps, void* y, int fmt, int rows, int K, int splitk, float* ws, size_t ws_bytes, omni_stream_t stream)
{
    if (!x || !wt16 || !tok || !ln_g || !ln_b || !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_sh_f16x3_ln512: null pointer");
    if (rows <= 0 || K <= 0 || K % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_sh_f16x3_ln512: bad shape");
    if (fmt & 8) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_gemm_sh_f16x3_ln512: no f16x1 form (fmt bit 3)");
    const int S = std::min(splitk, K / 32);
    if (S < 2) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_sh_f16x3_ln512: needs a split-K plan (splitk >= 2); an unsplit GEMM writes its result in its own epilogue");
    const int rc = conv2d_sh_impl(x, nullptr, wt16, bias, res, tok, 2, rows, 1, 1, K, 0, 512, 1, 1, 1, 0, OMNI_ACT_NONE, S, ws, ws_bytes, nullptr, 0, stream, false);
    if (rc != OMNI_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (fmt & 1) hipLaunchKernelGGL(sh_splitk_reduce_ln512_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)ws, bias, res, tok, ln_g, ln_b, y, rows, S, (size_t)rows * 512, eps);
    else         hipLaunchKernelGGL(sh_splitk_reduce_ln512_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, s, (const float*)ws, bias, res, tok, ln_g, ln_b, y, rows, S, (size_t)rows * 512, eps);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

constexpr int OMNI_HALO2_MIN_BLOCKS = 256;               // option conv_halo2 = 1: the least number of halo2_sh_kernel blocks a launch must have (a block per CU)

// Which kernel runs a convolution, with which template arguments, on what grid: what conv_sh_plan decides and conv_sh_launch launches (and what
// omni_conv2d_sh_plan reports, field for field in this order, followed by the split-K factor).  A family's unused arguments are 0.
// family: conv_sh_kernel | conv_pm_sh_kernel | conv3x3_halo_sh_kernel | halo2_sh_kernel; bm .. pp: the tile kernel's (position-major, halo: bn); th, iw: halo (halo2: iw)
enum { CONV_SH_TILE = 0, CONV_SH_PM = 1, CONV_SH_HALO = 2, CONV_SH_HALO2 = 3 };
struct ConvShPlan { int family, bm, bn, wm, wn, nst, nl, pp, th, iw; unsigned grid_x, grid_y; int threads; };

// The argument checks of omni_conv2d_sh_f16x3_ws that need no pointer.  Fills the shape of `a`: M .. pad as given, Ho, Wo, rows and splitk (>= 1: the caller's
// factor, at most the K-steps) — all that conv_sh_plan reads of it.
static int conv_sh_ksteps(const ShConvArgs& a) { return a.KH * a.KW * ((a.C1 + a.C2) / 32); }
static int conv_sh_shape(ShConvArgs& a, int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, int splitk, bool has_post)
{
    if (C1 <= 0 || C1 % 32 || C2 < 0 || C2 % 32 || Cout <= 0 || Cout % 32)
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh: channels must be multiples of 32");
    if (M <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || KH > 3 || KW > 3 || stride <= 0 || pad < 0)
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh: bad shape (kernels up to 3x3)");
    a.M = M; a.H = H; a.W = W; a.C1 = C1; a.C2 = C2; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.Ho = (H + 2 * pad - KH) / stride + 1; a.Wo = (W + 2 * pad - KW) / stride + 1;
    const long long rows = (long long)M * a.Ho * a.Wo;
    if (rows <= 0 || rows >= (1ll << 31) || (long long)M * H * W >= (1ll << 31))
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_sh: too many pixels for 32-bit row indices");
    a.rows = (int)rows;
    if ((long long)M * H * W * (C1 > C2 ? C1 : C2) * 4 >= (1ll << 31) || (long long)Cout * conv_sh_ksteps(a) * 128 >= (1ll << 31))
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_sh: an operand of 2 GiB or more (32-bit buffer offsets)");
    a.splitk = std::max(1, std::min(splitk, conv_sh_ksteps(a)));
    if (has_post && a.splitk > 1) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_sh: no post-activation addend with split-K");
    return OMNI_OK;
}

// blocks of a launch of BM x BN tiles: every block-count rule of conv_sh_plan, and the grid of the tile kernels
static long long conv_sh_tiles(const ShConvArgs& p, int bm, int bn) { return (((long long)p.rows + bm - 1) / bm) * (p.Cout / bn); }
static long long conv_sh_blocks(const ShConvArgs& p, int bm, int bn) { return conv_sh_tiles(p, bm, bn) * p.splitk; }

static ConvShPlan tile_plan(const ShConvArgs& p, const OmniOptions& o, int bm, int bn, int wm, int wn, int nst = 3, int nl = 0)
{
    const int pp = nl > 0 && wm * wn == 8 && o.conv_pingpong;    // the SIMD's two matrix waves in anti-phase (same bits)
    return {CONV_SH_TILE, bm, bn, wm, wn, nst, nl, pp, 0, 0, (unsigned)conv_sh_tiles(p, bm, bn), (unsigned)p.splitk, 64 * (wm * wn + nl)};
}
static ConvShPlan pm_plan(const ShConvArgs& p, int bn) { return {CONV_SH_PM, 0, bn, 0, 0, 0, 0, 0, 0, 0, (unsigned)conv_sh_tiles(p, 128, bn), (unsigned)p.splitk, 768}; }
static ConvShPlan halo_plan(int bn, int th, int iw, unsigned grid) { return {CONV_SH_HALO, 0, bn, 0, 0, 0, 0, 0, th, iw, grid, 1, 64 * th}; }

// The kernel choice of omni_conv2d_sh_f16x3_ws: a function of the shape, the caller's fmt bits, whether there is a post-activation addend, and the tuning
// options — nothing else, no HIP call.  The arithmetic mode (fmt bit 3) plays no part: every form has both instantiations (conv_sh_launch).
static ConvShPlan conv_sh_plan(const ShConvArgs& p, int fmt, bool has_post, const OmniOptions& o)
{
    const int H = p.H, W = p.W, M = p.M, Cout = p.Cout, rows = p.rows;
    const bool conv3x3 = p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1;
    // 64 output channels per block on 256-pixel tiles with 64 x 64 wave tiles (omni_conv_halo2.hip): the two 64-channel halo forms below with 0.59x the
    // operand bytes into LDS and 0.56x the fragment reads per matrix instruction — the same bits, so the choice may depend on anything.  Option conv_halo2:
    // 0 never | 1 where the launch has at least OMNI_HALO2_MIN_BLOCKS blocks of the new size | 2 wherever the shape allows (tests) | n > 2: as 1 with n blocks
    // (tuning).  Never for the latency form (fmt bit 2), nor where an option asks for the tile kernels or for 32-channel blocks.
    if (const int h2 = o.conv_halo2; h2 > 0 && p.splitk <= 1 && conv3x3 && Cout % 64 == 0 && rows % 256 == 0 && !(fmt & 4) && !o.conv_nohalo && o.conv_halo_bn != 32) {
        const int iw = (H == 16 && W == 16 && o.conv_img > 0) ? 16 : (W % HT_W == 0 && H % 8 == 0) ? 0 : -1;
        const long long blocks = (long long)(rows / 256) * (Cout / 64);
        if (iw >= 0 && (h2 == 2 || blocks >= (h2 == 1 ? OMNI_HALO2_MIN_BLOCKS : h2))) return {CONV_SH_HALO2, 0, 0, 0, 0, 0, 0, 0, 0, iw, (unsigned)blocks, 1, 256};
    }
    // small square images: the halo kernel over bands of whole image rows (IW > 0) — 16 x 16 (layer2, de_conv1_x: 61.6 -> 49.3 us per layer2
    // convolution at 8 panoramas) by default, 8 x 8 as well with conv_img = 2 (layer3: 52.7 -> 50.9)
    // (the choice must not depend on the number of images: a panorama's bits are the same in every batch size; a caller that runs ONE panorama,
    //  where the launch would be a quarter block per CU, asks for the tile kernel with fmt bit 2)
    if (p.splitk <= 1 && conv3x3 && H == W && (W == 16 || (W == 8 && o.conv_img >= 2)) && rows % 128 == 0 &&
        Cout % 64 == 0 && !(fmt & 4) && o.conv_img > 0 && !o.conv_nohalo) {
        const int bn = o.conv_halo_bn == 32 ? 32 : 64;
        return halo_plan(bn, 4, W, (unsigned)((int)(rows / 128) * (Cout / bn)));
    }
    if (p.splitk <= 1 && conv3x3 && W % HT_W == 0 && H % 4 == 0 && !o.conv_nohalo) {
        const int th = (H % 8 == 0 && o.conv_halo_th == 8) ? 8 : 4;
        // (fmt bit 2, ONE panorama: the launch is a fraction of a block per CU and costs the length of a block's life — 32-channel blocks are twice as many and
        //  half as long; option conv_halo_bn_lat, for the 4-row blocks)
        const bool bn32 = o.conv_halo_bn == 32 || (th == 4 && (fmt & 4) && o.conv_halo_bn_lat == 32);
        const int bn = (Cout % 64 == 0 && !bn32) ? 64 : 32;
        return halo_plan(bn, th, 0, (unsigned)(M * (H / th) * (W / HT_W) * (Cout / bn)));
    }
    // tile: results do not depend on it (every output element is the same k-ordered chain), so it is a pure tuning choice
    // -1 auto (= 8): the largest 8-wave tile the layer allows (256x128, 128x128, else 128x64: 3/8, 1/2, 3/4 of the L2 -> LDS bytes per MFMA
    // of a 64x64 tile) wherever the launch still has >= 128 blocks, 64x64 below that.  Measured interleaved in one process
    // (tools/pipe_ab.py, tools/plain_ab.py): +5.1 % panoramas/s with three forwards in flight (+1.2 % of it from 256x128), +1.7 % for plain
    // calls at 8 panoramas, -1 % at 4, 0 at 1.
    // 0: 64x64 everywhere; 1: 128x64 (4 waves); 2: 128x128 (4 waves); 3 / 4: the 8-wave forms everywhere; 5..7: auto without 256x128, with 64 / 128 / 256 blocks
    const int tile = o.conv_sh_tile < 0 ? 8 : o.conv_sh_tile;
    const bool c128 = Cout % 128 == 0;
    const bool fill128 = c128 && conv_sh_blocks(p, 128, 128) >= 128, fill64 = conv_sh_blocks(p, 128, 64) >= 128;   // 128 blocks of the 128-row tiles remain
    const bool big256 = tile == 8 && c128 && conv_sh_blocks(p, 256, 128) >= std::max(1, o.conv_big_blocks);
    // 3x3 on 8 x 8 and 4 x 4 images: the position-major form of the two ping-pong tile kernels (omni_conv_pm.hip) skips the K-steps of the taps that are
    // zero padding for every row of a tile — the same bits, so the choice may depend on anything.  Option conv_pm: 1 (default) where the launch would take
    // one of those two kernels | 0 never | 2 wherever the shape allows, whatever the row count (tests) | 3 / 4: as 1 for the 8 x 8 / the 4 x 4 images only
    const int pm = o.conv_pm;
    const bool pm_shape = pm > 0 && conv3x3 && H == W && (W == 8 || W == 4) && Cout % 64 == 0 && !has_post &&
                          o.conv_pingpong && !(pm == 3 && W != 8) && !(pm == 4 && W != 4);
    if (pm_shape && pm == 2) return pm_plan(p, c128 ? 128 : 64);
    if (pm_shape && tile == 8 && !big256 && (fill128 || fill64)) return pm_plan(p, fill128 ? 128 : 64);
    if (Cout % 64 != 0) return tile_plan(p, o, 128, 32, 4, 1);
    if (tile == 2 && c128) return tile_plan(p, o, 128, 128, 2, 2);
    if (tile == 1) return tile_plan(p, o, 128, 64, 2, 2);
    if (tile == 3) return tile_plan(p, o, 128, 64, 4, 2);            // 8 waves
    if (tile == 4 && c128) return tile_plan(p, o, 128, 128, 4, 2);
    if (big256) return tile_plan(p, o, 256, 128, 4, 2);              // each wave a 64x64 tile: 0.67 KB of LDS reads per MFMA instead of 1
    // (128x128 and 128x64 with four LOADER waves beside the eight matrix waves: layer3 51.3 -> 45.8 us, de_conv0_0 90 -> 79, layer4 43.3 -> 41.3, same bits;
    //  tile = 9: without them.  256x128 has no registers to spare for a third wave per SIMD.)
    if (tile == 8 && fill128) return tile_plan(p, o, 128, 128, 4, 2, 3, 4);
    if (tile == 8 && fill64) return tile_plan(p, o, 128, 64, 4, 2, 3, 4);
    if (tile == 9 && c128 && conv_sh_blocks(p, 256, 128) >= 128) return tile_plan(p, o, 256, 128, 4, 2);
    if (tile == 9 && fill128) return tile_plan(p, o, 128, 128, 4, 2);
    if (tile == 9 && fill64) return tile_plan(p, o, 128, 64, 4, 2);
    if (tile >= 5 && tile <= 7 && c128 && conv_sh_blocks(p, 128, 128) >= (32ll << (tile - 4))) return tile_plan(p, o, 128, 128, 4, 2);
    if (tile >= 5 && tile <= 7 && conv_sh_blocks(p, 128, 64) >= (32ll << (tile - 4))) return tile_plan(p, o, 128, 64, 4, 2);
    // one round of at most one block per CU (the transformer GEMMs; every deep layer at batch 1): the K loop is pure latency,
    // keep 5 stages in flight instead of 2 (96 KiB of LDS, which a single resident block can afford)
    // (conv_deep_loaders = 1: four loader waves beside the four matrix waves — at one block per CU a K-step is the four DMA pieces a matrix wave issues,
    //  ~400 cycles for its 192 of matrix work)
    if (conv_sh_blocks(p, 64, 64) <= 256 && conv_sh_ksteps(p) >= 8 && !o.conv_nodeep) return tile_plan(p, o, 64, 64, 2, 2, 6, o.conv_deep_loaders ? 4 : 0);
    return tile_plan(p, o, 64, 64, 2, 2);
}

// Launches what a plan says: the one place that instantiates conv_sh_kernel for omni_conv2d_sh_f16x3_ws (the Winograd entry point launches its own form),
// in both arithmetic modes (x1: fmt bit 3, f16x1); the other families through their units' launchers.
static int conv_sh_launch(const ConvShPlan& p, const ShConvArgs& a, bool x1, hipStream_t s)
{
    if (p.family == CONV_SH_HALO2) return omni_halo2_launch(&a, p.iw, x1, p.grid_x, s);
    if (p.family == CONV_SH_HALO) return omni_halo_launch(&a, p.bn, p.th, false, p.iw, x1, p.grid_x, s);
    if (p.family == CONV_SH_PM) return omni_conv_pm_launch(&a, p.bn, x1, p.grid_x, p.grid_y, s);
#define OMNI_TILE(BM, BN, WM, WN, NST, NL, PP) \
    if (p.bm == BM && p.bn == BN && p.wm == WM && p.wn == WN && p.nst == NST && p.nl == NL && p.pp == PP) { \
        if (x1) hipLaunchKernelGGL((conv_sh_kernel<BM, BN, WM, WN, NST, NL, PP, false, true>), dim3(p.grid_x, p.grid_y), dim3(p.threads), 0, s, a); \
        else    hipLaunchKernelGGL((conv_sh_kernel<BM, BN, WM, WN, NST, NL, PP, false, false>), dim3(p.grid_x, p.grid_y), dim3(p.threads), 0, s, a); \
        return OMNI_OK; }
    OMNI_TILE(128, 32, 4, 1, 3, 0, false) OMNI_TILE(128, 128, 2, 2, 3, 0, false) OMNI_TILE(128, 64, 2, 2, 3, 0, false)                                   // four waves
    OMNI_TILE(64, 64, 2, 2, 6, 4, false) OMNI_TILE(64, 64, 2, 2, 6, 0, false) OMNI_TILE(64, 64, 2, 2, 3, 0, false)                                       // ... 64 x 64, deep and plain
    OMNI_TILE(128, 64, 4, 2, 3, 0, false) OMNI_TILE(128, 128, 4, 2, 3, 0, false) OMNI_TILE(256, 128, 4, 2, 3, 0, false)                                  // eight
    OMNI_TILE(128, 128, 4, 2, 3, 4, true) OMNI_TILE(128, 128, 4, 2, 3, 4, false) OMNI_TILE(128, 64, 4, 2, 3, 4, true) OMNI_TILE(128, 64, 4, 2, 3, 4, false)   // eight + four loader waves
#undef OMNI_TILE
    OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_sh: no conv_sh_kernel<" + std::to_string(p.bm) + ", " + std::to_string(p.bn) + ", ..> of this plan");   // a programming error, not a user error
}

static int conv2d_sh_impl(const void* src1, const void* src2, const void* wt16, const float* bias,
                          const void* res, void* dst, int fmt, int M, int H, int W, int C1, int C2, int Cout,
                          int KH, int KW, int stride, int pad, int act, int splitk, float* ws, size_t ws_bytes,
                          const float* post, size_t post_elems, omni_stream_t stream, bool reduce)
{
    if (!src1 || !wt16 || !dst || (C2 > 0 && !src2)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh: null pointer");
    ShConvArgs a;
    if (const int rc = conv_sh_shape(a, M, H, W, C1, C2, Cout, KH, KW, stride, pad, splitk, post != nullptr); rc != OMNI_OK) return rc;
    const long long rows = a.rows;
    a.src1 = src1; a.src2 = src2; a.wt = wt16; a.bias = bias; a.res = res; a.dst = dst; a.dst_sh = fmt & 1; a.res_f32 = (fmt >> 1) & 1; a.act = act;
    a.dbg = 0; a.noxcd = omni_options().conv_noxcd; a.wt_major = 0; a.epi_lds = omni_options().conv_epi_lds && !(fmt & 4);   // (fmt bit 2, one panorama: the extra barrier and LDS round trip cost more than the wider stores save)
#ifdef OMNI_DEBUG_BUILD
    a.dbg = omni_debug_bits("OMNI_CONV_DBG");
#endif
    if (a.splitk > 1 && (!ws || ws_bytes < (size_t)a.splitk * rows * Cout * sizeof(float)))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh: split-K workspace too small");
    a.ws = ws;
    // block order of conv_sh_kernel: weight-stationary per XCD where the weight matrix is larger than the activation tensor(s) (option conv_wt_major:
    // 1 auto | 0 never | 2 always)
    a.wt_major = omni_options().conv_wt_major == 2 || (omni_options().conv_wt_major == 1 &&
                 (long long)Cout * conv_sh_ksteps(a) * 128 > (long long)M * H * W * (C1 + C2) * 4) ? 1 : 0;
    a.post = post; a.post_rows = 1; a.wino_th = a.wino_tw = a.wino_pix = 0;
    if (post) {
        if (post_elems == 0 || post_elems % (size_t)Cout || post_elems / (size_t)Cout > 0x7fffffffull)
            OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh: the post-activation addend must hold whole rows of Cout channels");
        a.post_rows = (unsigned)(post_elems / (size_t)Cout);
    }
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = conv_sh_launch(conv_sh_plan(a, fmt, post != nullptr, omni_options()), a, (fmt & 8) != 0, s); rc != OMNI_OK) return rc;   // fmt bit 3: f16x1
    OMNI_HIP(hipGetLastError());
    if (a.splitk > 1 && reduce) {
        const size_t n4 = (size_t)rows * Cout / 4;
        hipLaunchKernelGGL(sh_splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float*)ws, bias, res, dst,
                           n4, Cout, a.splitk, (size_t)rows * Cout, act, a.dst_sh, a.res_f32);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}

// The plan omni_conv2d_sh_f16x3_ws (has_post: ..._post_ws) would launch for these arguments under the current options (include/omnifusion.h); host only.
extern "C" int omni_conv2d_sh_plan(int fmt, int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, int splitk, int has_post,
                                   int* out, int n_out)
{
    if (!out || n_out < 14) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_sh_plan: needs room for 14 integers");
    ShConvArgs p{};
    if (const int rc = conv_sh_shape(p, M, H, W, C1, C2, Cout, KH, KW, stride, pad, splitk, has_post != 0); rc != OMNI_OK) return rc;
    const ConvShPlan q = conv_sh_plan(p, fmt, has_post != 0, omni_options());
    const int v[14] = {q.family, q.bm, q.bn, q.wm, q.wn, q.nst, q.nl, q.pp, q.th, q.iw, (int)q.grid_x, (int)q.grid_y, q.threads, p.splitk};
    std::copy(v, v + 14, out);
    return OMNI_OK;
}

// tok [rows,512] = sum_s parts[s] + bias + res, y = LayerNorm(tok) as SH (fmt bit 0) or fp32: the second pass of a split-K / K-sliced GEMM with 512
// columns on its own (sh_splitk_reduce_ln512_kernel; omni_gemm_sh_f16x3_ln512_ws runs it behind its GEMM).
extern "C" int omni_splitk_reduce_ln512(const float* parts, int nparts, const float* bias, const float* res, float* tok, const float* lg, const float* lb,
                                        float eps, void* y, int fmt, int rows, omni_stream_t stream)
{
    if (!parts || nparts < 1 || !tok || !lg || !lb || !y || rows <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_splitk_reduce_ln512: null pointer or empty input");
    hipStream_t s = (hipStream_t)stream;
    if (fmt & 1) hipLaunchKernelGGL(sh_splitk_reduce_ln512_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, s, parts, bias, res, tok, lg, lb, y, rows, nparts, (size_t)rows * 512, eps);
    else         hipLaunchKernelGGL(sh_splitk_reduce_ln512_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, s, parts, bias, res, tok, lg, lb, y, rows, nparts, (size_t)rows * 512, eps);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// layout conversions (n = number of elements, a multiple of 32 channels per pixel)
OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_conv)          // this translation unit's copy of the sticky range flag

extern "C" int omni_sh_overflow(int* flag, int reset)
{
    if (!flag) OMNI_FAIL(OMNI_ERR_INVALID, "omni_sh_overflow: null output");
    OMNI_HIP(hipDeviceSynchronize());                    // diagnostic entry point, never on the hot path
    unsigned v = 0;
    if (omni_sh_overflow_conv(&v, reset) != 0 || omni_sh_overflow_halo(&v, reset) != 0 || omni_sh_overflow_up2(&v, reset) != 0 ||
        omni_sh_overflow_rows(&v, reset) != 0 || omni_sh_overflow_net(&v, reset) != 0 || omni_sh_overflow_pm(&v, reset) != 0 ||
        omni_sh_overflow_halo2(&v, reset) != 0 || omni_sh_overflow_up2_taps(&v, reset) != 0 ||
        omni_sh_overflow_up2_heads_taps(&v, reset) != 0)
        OMNI_FAIL(OMNI_ERR_HIP, "omni_sh_overflow: could not read the device flag");
    *flag = v ? 1 : 0;
    return OMNI_OK;
}

extern "C" int omni_sh_from_f32(const float* src, void* dst, size_t n, omni_stream_t stream)
{
    if (!src || !dst || n % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_sh_from_f32: null pointer or n % 32 != 0");
    if (n == 0) return OMNI_OK;
    hipLaunchKernelGGL(sh_from_f32_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n / 4);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
extern "C" int omni_sh_to_f32(const void* src, float* dst, size_t n, omni_stream_t stream)
{
    if (!src || !dst || n % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_sh_to_f32: null pointer or n % 32 != 0");
    if (n == 0) return OMNI_OK;
    hipLaunchKernelGGL(sh_to_f32_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n / 4);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// ================================================================== Winograd F(2x2, 3x3), EXPERIMENTAL: everything but conv_sh_kernel's `if constexpr (WINO)` branches and wino_coef
namespace {

// Winograd F(2x2, 3x3) input transform: V[p = 4 xi + nu][tile][c] = (B^T d B)[xi][nu], d = the 4 x 4 window (rows 2 ty - 1 .. 2 ty + 2, columns 2 tx - 1 .. 2 tx + 2,
// zeros outside the image) of tile (m, ty, tx); B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]].  SH in, SH out; one thread per (tile, 4 channels).
__global__ __launch_bounds__(256) void wino_input_sh_kernel(const void* __restrict__ src, void* __restrict__ V, int M, int H, int W, int C, size_t nt)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int cq = C >> 2;
    if (i >= nt * cq) return;
    const size_t tl = i / cq;
    const int c = (int)(i - tl * cq) * 4;
    const int tw = W >> 1, th = H >> 1;
    const int m = (int)(tl / (size_t)(th * tw)), rem = (int)(tl - (size_t)m * th * tw), ty = rem / tw, tx = rem - ty * tw;
    f4v d[4][4];
#pragma unroll
    for (int a_ = 0; a_ < 4; ++a_)
#pragma unroll
        for (int b_ = 0; b_ < 4; ++b_) {
            const int y = 2 * ty - 1 + a_, x = 2 * tx - 1 + b_;
            d[a_][b_] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? act_load4<true>(src, (((size_t)m * H + y) * W + x) * C + c) : (f4v)(0.0f);
        }
    f4v u[4][4];                                                  // B^T d
#pragma unroll
    for (int b_ = 0; b_ < 4; ++b_) { u[0][b_] = d[0][b_] - d[2][b_]; u[1][b_] = d[1][b_] + d[2][b_]; u[2][b_] = d[2][b_] - d[1][b_]; u[3][b_] = d[1][b_] - d[3][b_]; }
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {                              // (B^T d) B
        const f4v v0 = u[xi][0] - u[xi][2], v1 = u[xi][1] + u[xi][2], v2 = u[xi][2] - u[xi][1], v3 = u[xi][1] - u[xi][3];
        act_store4<true>(V, ((size_t)(4 * xi + 0) * nt + tl) * C + c, v0);
        act_store4<true>(V, ((size_t)(4 * xi + 1) * nt + tl) * C + c, v1);
        act_store4<true>(V, ((size_t)(4 * xi + 2) * nt + tl) * C + c, v2);
        act_store4<true>(V, ((size_t)(4 * xi + 3) * nt + tl) * C + c, v3);
    }
}

}  // namespace

// ---- Winograd F(2x2, 3x3) for 3x3 stride-1 pad-1 convolutions of small images (EXPERIMENTAL, round 6; conv_sh_kernel<.., WINO>)
// omni_wino_input_sh: src SH [M,H,W,C] (H, W even) -> V SH [16][M * H/2 * W/2][C].
extern "C" int omni_wino_input_sh(const void* src, void* V, int M, int H, int W, int C, omni_stream_t stream)
{
    if (!src || !V) OMNI_FAIL(OMNI_ERR_INVALID, "omni_wino_input_sh: null pointer");
    if (M <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0 || C % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_wino_input_sh: even image sides, channels a multiple of 32");
    const size_t nt = (size_t)M * (H / 2) * (W / 2), n = nt * (C / 4);
    if (16 * nt * C * 4 >= (1ull << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_wino_input_sh: the transformed tensor must stay under 2 GiB (32-bit buffer offsets)");
    hipLaunchKernelGGL(wino_input_sh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, V, M, H, W, C, nt);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// dst [M,H,W,Cout] = act(conv3x3(x) + bias + res) from V = omni_wino_input_sh(x) and wt16 = the f16x3 split (omni_conv2d's weight format) of the matrix
// [Cout][16 * C], k = p * C + c, holding U_p = (G g G^T)[p] (G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]).  fmt as omni_conv2d_sh_f16x3_ws (bit 0: dst SH; bit 1: res fp32).
// splitk in {1, 2, 4}: the sixteen positions divided over that many blocks per tile, partial outputs to ws (splitk * M*H*W * Cout floats) and
// sh_splitk_reduce_kernel.  Cout % 64 == 0, C % 32 == 0.  Equal to the direct convolution up to rounding (measured 1e-6 against float64, tools/winograd_proto.py).
extern "C" int omni_conv3x3_wino_sh_f16x3(const void* V, const void* wt16, const float* bias, const void* res, void* dst, int fmt,
                                          int M, int H, int W, int C, int Cout, int act, int splitk, float* ws, size_t ws_bytes, omni_stream_t stream)
{
    if (!V || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_wino_sh: null pointer");
    if (M <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0 || C % 32 || Cout <= 0 || Cout % 64) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_wino_sh: even image sides, C % 32 == 0, Cout % 64 == 0");
    if (splitk != 1 && splitk != 2 && splitk != 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_wino_sh: splitk must be 1, 2 or 4 (it divides the sixteen positions)");
    if (fmt & 8) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_wino_sh: no f16x1 form (fmt bit 3)");
    const long long nt = (long long)M * (H / 2) * (W / 2), pix = (long long)M * H * W;
    if (16 * nt * C * 4 >= (1ll << 31) || (long long)Cout * 16 * C * 4 >= (1ll << 31) || pix >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_wino_sh: an operand of 2 GiB or more");
    if (splitk > 1 && (!ws || ws_bytes < (size_t)splitk * pix * Cout * sizeof(float))) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_wino_sh: split workspace too small");
    ShConvArgs a;
    a.src1 = V; a.src2 = nullptr; a.wt = wt16; a.bias = bias; a.res = res; a.dst = dst; a.dst_sh = fmt & 1; a.res_f32 = (fmt >> 1) & 1;
    a.dbg = 0; a.noxcd = omni_options().conv_noxcd; a.wt_major = 0; a.epi_lds = 0;
    a.M = 1; a.H = 16; a.W = (int)nt; a.C1 = C; a.C2 = 0; a.Cout = Cout; a.KH = 16; a.KW = 1; a.stride = 1; a.pad = 0; a.act = act;
    a.Ho = H; a.Wo = W; a.rows = (int)nt; a.splitk = splitk; a.ws = ws; a.post = nullptr; a.post_rows = 1;
    a.wino_th = H / 2; a.wino_tw = W / 2; a.wino_pix = (int)pix;
    hipStream_t s = (hipStream_t)stream;
    const int tiles = (int)((nt + 127) / 128) * (Cout / 64);
    hipLaunchKernelGGL((conv_sh_kernel<128, 64, 4, 2, 3, 4, true, true>), dim3(tiles, splitk), dim3(64 * 12), 0, s, a);
    OMNI_HIP(hipGetLastError());
    if (splitk > 1) {
        const size_t n4 = (size_t)pix * Cout / 4;
        hipLaunchKernelGGL(sh_splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float*)ws, bias, res, dst,
                           n4, Cout, splitk, (size_t)pix * Cout, act, a.dst_sh, a.res_f32);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}
