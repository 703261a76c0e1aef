// omni_conv_sh_common.h — what the split-half convolution units share (omni_conv_sh.hip, omni_conv_halo.hip with the stem, omni_conv_up2.hip, omni_gemm_rows.hip).
// Device side: forceinline helpers, types and macros only — the library is built without relocatable device code, every __global__ lives in exactly one
// .hip.  Host side: the few functions that cross units.  The convolution of the network on the fp16 matrix cores with SPLIT-HALF activations (gfx950):
//
// Same operator as omni_conv.hip (reference: Conv3d(k,k,1)+BatchNorm3d(+ReLU)(+residual), model/spherical_model.py:
// 122-167 encoder, :29-37,214-222 decoder) and the same "f16x3" arithmetic (x = hi + lo*2^-11, three
// v_mfma_f32_32x32x16_f16 per product block, fp32 accumulation), but the activations travel between layers ALREADY
// split: the "SH" layout stores, per pixel and per group of 32 channels, 32 hi halfs followed by 32 lo halfs (128 bytes:
// the footprint of 32 floats, and the very row format of the pre-split weights).  The split is done once, by the
// producer's epilogue, instead of once per (tap, output-channel tile) by every consumer — in the fp32-activation kernel
// that VALU work cost as much issue time as the matrix instructions (ablation: 41 us of an 82 us layer3 convolution).
//
// With both operands in their final bit pattern the tiles go HBM/L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds):
// no staging registers, no conversion, no ds_write.  A block keeps NST stages of (A: BM pixels x 128 B, B: BN output
// channels x 128 B) in flight; per K-step (one tap x 32 channels) there is ONE barrier:
//      s_waitcnt vmcnt((NST-2)*LPS)   my pieces of stage k have landed       (LPS = DMA instructions per wave and stage)
//      s_barrier                      ... everybody's have, and everybody is done reading stage k-1
//      issue DMA for stage k+NST-1    into the slot stage k-1 occupied
//      8 x ds_read_b128 + 6 x MFMA per 32x32 tile pair on stage k
// Out-of-image taps and rows past the end need no branch: their buffer offset is out of range and the DMA deposits zeros
// (checked on hardware: tools/dbg_dma.py).
//
// LDS image: a DMA instruction deposits its 64 lanes' 16-byte pieces back to back, so rows are 128 B with no padding;
// bank conflicts are avoided by permuting the 16 pieces of each 256-B row pair with the row-pair index (g' = g ^ (d & 15)):
// the lane that owns LDS slot g' of pair d FETCHES piece g' ^ (d & 15) and the fragment reads apply the same involution.
// Every ds_read_b128 lane group then touches 16 distinct 16-byte bank groups.
//
// The matrix instruction is fed weights as its row operand and pixels as its column operand, so a lane ends up with FOUR
// CONSECUTIVE channels of ONE pixel per register quad: bias / residual / output move as 8-byte (SH) or 16-byte (fp32)
// pieces instead of scalars.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include "omni_internal.h"
#include "omni_sh.h"

// Compile-time ablations for tools/convabl.sh (a library variant per value; the product is built with 0): 4 no epilogue | 16, 32, 64 drop the
// weight-lo / activation-lo / hi.hi product | 128 no operand DMA | 256 no block barrier in the K loop | 512 no fragment reads | conv3x3_up2_g1_kernel: 1024 no
// halo arithmetic, 2048 no stores, 4096 no pixel loads, 8192 four accumulators, 16384 no heads part, 32768 time stamps of block 0 (tools/g1_stamps.py; conv3x3_halo_sh_kernel: tools/halo_stamps.py; conv_sh_kernel: tools/tile_stamps.py).  (The debug
// build's RUN-time bits put branches around the matrix instructions and run 2-5x slower than the product: useless for timing.)
#ifndef OMNI_CONV_ABL
#define OMNI_CONV_ABL 0
#endif
#define OMNI_ABL(bit) ((OMNI_CONV_ABL & (bit)) != 0)
#ifndef OMNI_PP_PRIO
#define OMNI_PP_PRIO 0                                         // conv_sh_kernel<.., PP>: s_setprio 1 around a phase's matrix instructions
#endif
#ifndef OMNI_G1_PW
#define OMNI_G1_PW 4                                           // producer waves of conv3x3_up2_g1_kernel<HEADS> (8: measured equal)
#endif

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const void* p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0,
                                             (int)(unsigned)(bytes > 0xffffffffull ? 0xffffffffull : bytes), 0x00020000);
}

// one LDS-DMA instruction: lane l's 16 bytes at buffer offset voff (+ soff, wave-uniform) land at lds + 16 l; offsets
// outside the buffer deposit zeros.  (A plain function: the builtin is not accepted inside a kernel template's body by
// the host pass, which then silently drops the kernel's launch stub.)
__device__ __forceinline__ void dma16(rsrc_t rs, unsigned char* lds, int voff, int soff)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)lds, 16, voff, soff, 0, 0);
}

// s_waitcnt vmcnt(N) with a compile-time count (the LDS-DMA pieces still allowed in flight)
template <int N> __device__ __forceinline__ void wait_vm()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
#define OMNI_VM(K) else if constexpr (N == K) asm volatile("s_waitcnt vmcnt(" #K ")" ::: "memory");
    if constexpr (N < 0) {}
    OMNI_VM(0) OMNI_VM(1) OMNI_VM(2) OMNI_VM(3) OMNI_VM(4) OMNI_VM(5) OMNI_VM(6) OMNI_VM(7)
    OMNI_VM(8) OMNI_VM(9) OMNI_VM(10) OMNI_VM(11) OMNI_VM(12) OMNI_VM(13) OMNI_VM(14) OMNI_VM(15)
    OMNI_VM(16) OMNI_VM(17) OMNI_VM(18) OMNI_VM(19) OMNI_VM(20) OMNI_VM(21) OMNI_VM(22) OMNI_VM(23)
    OMNI_VM(24) OMNI_VM(25) OMNI_VM(26) OMNI_VM(27) OMNI_VM(28) OMNI_VM(29) OMNI_VM(30) OMNI_VM(31)
    OMNI_VM(32) OMNI_VM(33) OMNI_VM(34) OMNI_VM(35) OMNI_VM(36) OMNI_VM(37) OMNI_VM(38) OMNI_VM(39)
    OMNI_VM(40) OMNI_VM(41) OMNI_VM(42) OMNI_VM(43) OMNI_VM(44) OMNI_VM(45) OMNI_VM(46) OMNI_VM(47)
    OMNI_VM(48) OMNI_VM(49) OMNI_VM(50) OMNI_VM(51) OMNI_VM(52) OMNI_VM(53) OMNI_VM(54) OMNI_VM(55)
    OMNI_VM(56) OMNI_VM(57) OMNI_VM(58) OMNI_VM(59) OMNI_VM(60) OMNI_VM(61) OMNI_VM(62) OMNI_VM(63)
#undef OMNI_VM
}

// Every LDS read this wave has issued has returned.  REQUIRED in front of a barrier that licenses another wave to overwrite the
// buffer those reads came from: hipcc sinks the MFMAs that consume a stage's last fragments (and the s_waitcnt lgkmcnt that guards
// them) BELOW the following s_barrier, so without this wait a wave can pass the barrier with ds_reads still queued and a faster
// wave's LDS-DMA for the next stage then lands in the buffer first.  Measured: one wrong output row in 1 of 600 forwards at 8
// panoramas on two streams (1 of 30 at 16) with the 4-wave halo kernel, none in 3000 with the wait (tools/lanes_trace.py).
__device__ __forceinline__ void wait_lds_reads() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The arithmetic mode of a convolution kernel (template flag X1, fmt bit 3 of the C ABI): false = "f16x3", three matrix instructions per
// product block, x = acc + 2^-11 acc1 with acc = A_hi.W_hi and acc1 = A_hi.W_lo + A_lo.W_hi; true = "f16x1", ONE matrix instruction,
// A_hi.W_hi, with fp32 accumulation: the lo fragments are never read, acc1 is never written and its registers do not exist (the operand
// tiles still arrive as whole 128-byte hi|lo rows: the loaders and their counted waits are the same code).
template <bool X1> __device__ __forceinline__ float acc_join(float a1, float a0)
{
    if constexpr (X1) return a0;
    else return fmaf(a1, 4.8828125e-4f, a0);
}

struct ShConvArgs {
    const void* src1; const void* src2;      // SH activations [M,H,W,C1], [M,H,W,C2] (src2 may be null)
    const void* wt;                          // halfs [Cout][KH*KW*(C1+C2)/32][hi32|lo32], BN folded
    const float* bias;                       // [Cout] or null
    const void* res;                         // residual (SH), same shape as dst, or null
    void* dst;                               // [M,Ho,Wo,Cout]: SH (dst_sh) or fp32 NHWC
    int M, H, W, C1, C2, Ho, Wo, Cout;
    int KH, KW, stride, pad, act;
    int rows;                                // M*Ho*Wo
    int dst_sh;
    int res_f32;                             // residual is plain fp32 NHWC instead of SH
    int dbg;                                 // debug build only (OMNI_CONV_DBG): 4 = skip the epilogue
    int noxcd;                               // 1: identity block order (tuning, OMNI_CONV_NOXCD)
    int wt_major;                            // 1: an XCD's contiguous block range walks tile_m fastest — it owns a range of OUTPUT-CHANNEL tiles and touches only their weights (conv_sh_kernel)
    int epi_lds;                             // 1: SH epilogues through an LDS transposition (16-byte pieces), OMNI_CONV_EPI_LDS
    int splitk; float* ws;                   // >1: blockIdx.y owns a K range, raw fp32 partial sums to ws[y][rows][Cout]
    int wino_th, wino_tw, wino_pix;          // WINO kernels: tiles per image (H/2, W/2) and output pixels M*H*W (rows = tiles, Ho / Wo = the image)
    const float* post; unsigned post_rows;   // fp32 [post_rows][Cout] added AFTER the activation, row index modulo post_rows (layer1 + point_feat), or null
};

// Fused epilogue of NT accumulator tiles of ONE pixel row r (D = W x pixels: a lane holds, per register quad q, the four
// consecutive channels c0[j] + 8q + 4(lane>>5) .. +3 of its pixel).  Two phases: every bias / residual load is issued
// before the first store, so the loads overlap instead of serialising load -> wait -> store once per quad.
// QC: register quads of a tile whose loads are in flight together (4 = all; 2 where the register budget is tight)
template <int NT, int QC = 4, bool X1 = false>
__device__ __forceinline__ void epilogue_row(const f16v (&acc)[NT], const f16v (&acc1)[NT], const ShConvArgs& a, size_t r,
                                             const int (&c0)[NT], int lane, bool dst_sh)
{
    const float* post = a.post ? a.post + (size_t)((unsigned)r % a.post_rows) * a.Cout : nullptr;
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += QC) {
        f4v bq[NT * QC], rf[NT * QC]; h4v rh[NT * QC], rl[NT * QC];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int qq = 0; qq < QC; ++qq) {
                const int q = q0 + qq, c = c0[j] + 8 * q + 4 * (lane >> 5);
                bq[j * QC + qq] = a.bias ? *reinterpret_cast<const f4v*>(a.bias + c) : (f4v)(0.0f);
                if (a.res && a.res_f32) rf[j * QC + qq] = *reinterpret_cast<const f4v*>((const float*)a.res + r * a.Cout + c);
                else if (a.res) {
                    const unsigned char* rp = (const unsigned char*)a.res + sh_off(r * a.Cout + c);
                    rh[j * QC + qq] = *reinterpret_cast<const h4v*>(rp); rl[j * QC + qq] = *reinterpret_cast<const h4v*>(rp + 64);
                }
            }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int qq = 0; qq < QC; ++qq) {
                const int q = q0 + qq, c = c0[j] + 8 * q + 4 * (lane >> 5);
                f4v v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[j][4 * q + e], acc[j][4 * q + e]);
                v += bq[j * QC + qq];
                if (a.res && a.res_f32) v += rf[j * QC + qq];
                else if (a.res) v += sh_join4(rh[j * QC + qq], rl[j * QC + qq]);
                if (a.act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                else if (a.act == OMNI_ACT_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
                }
                if (post) v += *reinterpret_cast<const f4v*>(post + c);
                const size_t o = r * a.Cout + c;
                if (dst_sh) act_store4<true>(a.dst, o, v);
                else        act_store4<false>(a.dst, o, v);
            }
    }
}

// The same epilogue through LDS, for SH outputs (and SH or no residual): a wave's NT accumulator tiles of 32 CONSECUTIVE pixel rows
// r0 .. r0+31 go to a wave-private [32][32 NT + 4] float tile and come back as (pixel, 32-channel group, 8-channel piece) tasks, four
// consecutive lanes per pixel group: the residual arrives and the result leaves as 16-byte pieces, 64 contiguous bytes per pixel and
// half (hi | lo) per instruction.  epilogue_row moves 8 bytes per lane, 16 per pixel and instruction — 4.7 M sixteen-byte requests for
// layer1's 75 MB, which is what its 23-us skeleton is made of.  Same operations on every element in the same order: same bits.
// `tile` = 32 * (32 NT + 4) floats of LDS owned by this wave (the K loop's buffers, after a block barrier).
// (r1: the pixel row of accumulator column 16 when the 32 columns are two runs of 16 consecutive rows — the stem's 2 x 16 tiles; default r0 + 16)
// POST: the caller may carry a post-activation addend (a.post) — only the halo kernel does; the tile kernel compiles the addend's registers
// away.  The tasks are processed HALF at a time (loads of a half issued together, then its arithmetic and stores): the live set is what lets
// conv_sh_kernel<128,128,4,2,3,4> — twelve waves per block, a 168-register budget — run its epilogue without scratch (it carried 236 B).
template <int NT, bool POST = true, bool X1 = false>
__device__ __forceinline__ void epilogue_tile_lds(const f16v (&acc)[NT], const f16v (&acc1)[NT], const ShConvArgs& a, size_t r0, int nrows,
                                                  const int (&c0)[NT], int lane, float* tile, size_t r1 = ~(size_t)0)
{
    if (r1 == ~(size_t)0) r1 = r0 + 16;
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
    const bool post = POST && a.post != nullptr;
#pragma unroll
    for (int k0 = 0; k0 < TASKS; k0 += HALF) {
        f4v va[HALF], vb[HALF], pa[HALF], pb[HALF]; h8v rh[HALF], rl[HALF];
        size_t off[HALF]; bool ok[HALF];
#pragma unroll
        for (int kk = 0; kk < HALF; ++kk) {
            const int task = (k0 + kk) * 64 + lane, px = task / (4 * NT), rem = task - px * (4 * NT), j = rem >> 2, pc = rem & 3;
            ok[kk] = px < nrows;
            va[kk] = *reinterpret_cast<const f4v*>(tile + px * PITCH + 32 * j + 8 * pc);
            vb[kk] = *reinterpret_cast<const f4v*>(tile + px * PITCH + 32 * j + 8 * pc + 4);
            off[kk] = ((px < 16 ? r0 + px : r1 + (px - 16)) * a.Cout + c0[j]) * 4 + 16 * pc;     // byte offset of the hi piece (the lo piece: + 64)
            if (a.bias) { va[kk] += *reinterpret_cast<const f4v*>(a.bias + c0[j] + 8 * pc); vb[kk] += *reinterpret_cast<const f4v*>(a.bias + c0[j] + 8 * pc + 4); }
            if (a.res && ok[kk]) {
                rh[kk] = *reinterpret_cast<const h8v*>((const unsigned char*)a.res + off[kk]);
                rl[kk] = *reinterpret_cast<const h8v*>((const unsigned char*)a.res + off[kk] + 64);
            }
            if (post && ok[kk]) {                                 // added AFTER the activation, as in epilogue_row
                const float* pp = a.post + (size_t)((unsigned)(px < 16 ? r0 + px : r1 + (px - 16)) % a.post_rows) * a.Cout + c0[j] + 8 * pc;
                pa[kk] = *reinterpret_cast<const f4v*>(pp); pb[kk] = *reinterpret_cast<const f4v*>(pp + 4);
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
            if (post) { v0 += pa[kk]; v1 += pb[kk]; }
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

// dst[o .. o+3] = act(v + bias + res): the tail of a split-K sum (v = the partial sums added in slab order), 4 channels at flat index o
__device__ __forceinline__ void splitk_finish(f4v v, size_t o, const float* __restrict__ bias, const void* __restrict__ res, void* __restrict__ dst,
                                              int Cout, int act, int dst_sh, int res_f32)
{
    if (bias) v += *reinterpret_cast<const f4v*>(bias + (o % Cout));
    if (res && res_f32) v += *reinterpret_cast<const f4v*>((const float*)res + o);
    else if (res) {
        const unsigned char* rp = (const unsigned char*)res + sh_off(o);
        v += sh_join4(*reinterpret_cast<const h4v*>(rp), *reinterpret_cast<const h4v*>(rp + 64));
    }
    if (act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    else if (act == OMNI_ACT_GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    }
    if (dst_sh) {
        h4v hi, lo; sh_split4(v, hi, lo);
        unsigned char* dp = (unsigned char*)dst + sh_off(o);
        *reinterpret_cast<h4v*>(dp) = hi; *reinterpret_cast<h4v*>(dp + 64) = lo;
    } else {
        *reinterpret_cast<f4v*>((float*)dst + o) = v;
    }
}

constexpr int HT_W = 32, HPW = HT_W + 2;                     // the halo kernels' tile row (omni_conv_halo.hip, omni_conv_up2.hip): 32 pixels + one halo pixel each side

}  // namespace

// ---- host functions that cross units
// The launchers of the kernel families that live in other units.  Which form runs and on what grid is the caller's decision (conv_sh_plan in omni_conv_sh.hip;
// omni_conv3x3_up2_sh_f16x3 for the up-sampling halo): a launcher launches exactly that, or fails with OMNI_ERR_UNSUPPORTED on a form it does not instantiate.
// `args`: the caller's ShConvArgs (the type lives in every unit's anonymous namespace, like the kernels that take it, so it crosses as bytes)
// omni_conv_halo.hip: conv3x3_halo_sh_kernel<bn, th, up2, iw, x1> on `grid` blocks of 64 * th threads
int omni_halo_launch(const void* args, int bn, int th, bool up2, int iw, bool x1, unsigned grid, hipStream_t s);
// omni_conv_pm.hip: conv_pm_sh_kernel<bn, x1>, the position-major form of the 128 x bn ping-pong tile kernel (3x3, stride 1, pad 1, H = W in {4, 8}; bn 128 | 64) on
// grid_x tiles x grid_y K ranges of 768 threads
int omni_conv_pm_launch(const void* args, int bn, bool x1, unsigned grid_x, unsigned grid_y, hipStream_t s);
int omni_sh_overflow_pm(unsigned* out, int reset);
// omni_conv_halo2.hip: halo2_sh_kernel<iw, x1>, the 64-channel halo convolution on 256-pixel tiles with 64 x 64 wave tiles (3x3, stride 1, pad 1, no split-K, Cout % 64 == 0;
// iw 0: W % 32 == 0 and H % 8 == 0 | iw 16: H == W == 16 and rows % 256 == 0) on `grid` blocks of 256 threads
int omni_halo2_launch(const void* args, int iw, bool x1, unsigned grid, hipStream_t s);
int omni_sh_overflow_halo2(unsigned* out, int reset);
int omni_sh_overflow_up2_taps(unsigned* out, int reset);  // omni_conv_up2_taps.hip's (up2_taps_fused_kernel; its entry point lives in that unit)
// omni_conv_up2_heads_taps.hip: up2_heads_taps_kernel, de_conv4_0 + the heads' first half as tap products on the low-resolution map (f16x3, P == 128 only: src SH
// [M, 64, 64, 32], hr = the scratch of omni_conv3x3_up2_heads_sh_f16x3) on one persistent block of 512 threads per CU
int omni_up2_heads_taps_launch(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float* hr, int M, hipStream_t s);
int omni_sh_overflow_up2_heads_taps(unsigned* out, int reset);
// the sticky range flag of omni_sh.h, one copy per translation unit whose kernels write SH: omni_sh_overflow (omni_conv_sh.hip) reads them all
int omni_sh_overflow_halo(unsigned* out, int reset);
int omni_sh_overflow_up2(unsigned* out, int reset);
int omni_sh_overflow_rows(unsigned* out, int reset);
int omni_sh_overflow_net(unsigned* out, int reset);      // omni_net.hip's
