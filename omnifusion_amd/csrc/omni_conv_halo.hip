// omni_conv_halo.hip — conv3x3_halo_sh_kernel: 3x3 stride-1 split-half convolutions with halo-tile reuse, all twenty instantiations, behind their one
// launcher (no entry points of their own: omni_conv2d_sh_f16x3_ws in omni_conv_sh.hip and omni_conv3x3_up2_sh_f16x3 in omni_conv_up2.hip choose the form),
// and the stem (stem_f16x3_kernel, stem_f16x3_pc_kernel, omni_stem_sh_f16x3 / _f16x1).
// Why the stem is HERE: it and the 32-channel halo forms are the two users of epilogue_tile_lds<1, true, X1>, and only the halo kernel leaves that helper's
// last argument at its default.  Alone in a unit every call site passes the same constant, the compiler folds it into the helper BEFORE inlining and the ten
// 32-channel halo kernels come out one or two instructions shorter than the pinned code (tools/split_isa_diff.py).  Same arithmetic either way; kept bit-identical.
#include <string.h>
#include "omni_conv_sh_common.h"

namespace {

// ------------------------------------------------------------------ 3x3 stride-1 convolution with halo-tile reuse (SH)
// The tile kernel above fetches every input pixel group once per tap (9x the input through L2 -> LDS), which is what
// bounds the wide, shallow decoder layers (de_conv3_x, de_conv4_0: 64^2 / 128^2 images, 32-128 channels).  Here a block
// owns a 4x32 pixel tile of ONE image and BN output channels; per 32-channel group it DMAs the 6x34 halo patch into LDS
// ONCE (pixel-major 128-B rows, same pair swizzle, out-of-image pixels arrive as zeros) and serves the nine taps from it:
// wave w owns image row y0+w (32 pixels = one MFMA column tile), its pixel fragment for tap (ky,kx) is the same LDS image
// shifted by ky rows and kx pixels.  The weights arrive one kernel row (3 taps) at a time through a double buffer: the
// next row's DMA is in flight under the 18*BN/32 MFMAs of the current one.  Requires W % 32 == 0, H % 4 == 0.

// TH = image rows per block = waves per block (4: 6x34 halo, 26 KiB; 8: 10x34 halo, 43 KiB, half the weight traffic per pixel)
//
// UP2: the convolution of the 2x bilinear up-sampling of src1 ([M, H/2, W/2, C1]; F.interpolate(align_corners=False) followed by
// ConvBnReLU, model/spherical_model.py:279-301) without the up-sampled tensor ever existing: the halo patch is COMPUTED into LDS
// instead of copied.  The 6 x 34 halo pixels are 3 x 17 cells of 2 x 2 pixels that share their four source pixels; thread
// (cell, 8 channels) loads those once (8 x 16 B), joins hi/lo, evaluates up-sample_sh8_kernel's expression for its 4 pixels and
// writes the 8 split pieces where the DMA would have put them (out-of-image halo pixels: zeros, the convolution's padding).
// Same arithmetic, same bits as the two kernels it replaces; one pass over HBM less in each direction for the widest tensors.
//
// IW > 0: images narrower than a 32-pixel tile row (layer2-4 and the first decoder stages: 16 x 16, 8 x 8, 4 x 4).  The tile is TH*32
// CONSECUTIVE pixels of the flattened [M, H, W] index — NSUB bands of SUBROWS whole image rows (8 rows of a 16 x 16 image; two 8 x 8 or
// eight 4 x 4 images) — each band with its own (SUBROWS+2) x (IW+2) halo in LDS; wave w owns pixels 32w .. 32w+31 of the tile.  Against
// conv_sh_kernel's im2col tiles (every pixel group fetched once per tap) a K-step brings the weights only: 0.6x the LDS-DMA pieces per
// matrix instruction at 128 x 128, which is what bounds those layers (tools/convabl.sh: the operand traffic of a layer3 convolution costs
// as much time as its matrix instructions and overlaps them for a third).  Needs H == W == IW and rows % (TH*32) == 0.
template <int BN, int TH, bool UP2 = false, int IW = 0, bool X1 = false>      // X1: f16x1 (acc_join)
__global__ __launch_bounds__(64 * TH, (TH == 8 && BN == 32) ? 4 : 1) void conv3x3_halo_sh_kernel(ShConvArgs a)      // (8 rows x 32 channels: 128 registers, two 8-wave blocks per CU)
{
    static_assert(!UP2 || (TH == 4 && IW == 0), "the cell decomposition of the up-sampling halo is written for 4-row tiles of wide images");
    constexpr int TN = BN / 32, NW = TH, RPP = 8 * NW;
    constexpr int IWD = IW > 0 ? IW : 1;
    constexpr int SUBROWS = (TH * 32 / IWD) < IWD ? (TH * 32 / IWD) : IWD, SUBPX = SUBROWS * IWD, NSUB = TH * 32 / SUBPX;
    constexpr int HPS = (SUBROWS + 2) * (IWD + 2);               // halo pixels of one band
    static_assert(IW == 0 || (NSUB * SUBPX == TH * 32 && IW * IW % SUBPX == 0), "bands must tile the images");
    constexpr int HPX = IW > 0 ? NSUB * HPS : (TH + 2) * HPW, HA_INSTR = (HPX * 8 + 63) / 64, HA_BYTES = HA_INSTR * 1024;
    constexpr int APASS = (HA_INSTR + NW - 1) / NW, BROWS = 3 * BN, BPASS = (BROWS + RPP - 1) / RPP, B_BYTES = BROWS * 128;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[HA_BYTES + 2 * B_BYTES];
    // (ablation 32768, tools/halo_stamps.py: s_memtime of wave 0 of blocks 0 and 600 — start, prologue done, per K stage: before its waits / behind the barrier / weights
    //  issued / matrix instructions issued, epilogue done — dumped to a.ws)
    __shared__ long long hst[OMNI_ABL(32768) ? 64 : 1];
    const bool stamped = OMNI_ABL(32768) && (blockIdx.x == 0 || blockIdx.x == 600) && a.ws != nullptr;
    auto hstamp = [&](int k) { if (OMNI_ABL(32768) && stamped && threadIdx.x == 0 && k < 64) hst[k] = clock64(); };
    auto hdump = [&]() { if (OMNI_ABL(32768) && stamped && threadIdx.x == 0) for (int i = 0; i < 64; ++i) reinterpret_cast<long long*>(a.ws)[(blockIdx.x ? 64 : 0) + i] = hst[i]; };
    hstamp(0);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ntn = a.Cout / BN, tw = IW > 0 ? 1 : a.W / HT_W, th = IW > 0 ? 1 : a.H / TH;
    int bid = a.noxcd ? blockIdx.x : omni_xcd_remap(blockIdx.x, gridDim.x);   // neighbouring tiles (shared halos, same A for all tile_n) on one XCD
    const int tile_n = bid % ntn; bid /= ntn;
    const int tx = bid % tw; bid /= tw;
    const int ty = bid % th; const int m = bid / th;              // (IW > 0: m = tile index, first pixel m * TH * 32)
    const int y0 = ty * TH, x0 = tx * HT_W, col0 = tile_n * BN;
    const int G1 = a.C1 >> 5, G = (a.C1 + a.C2) >> 5, ksteps = 9 * G;
    const int pix0 = m * (TH * 32);                               // IW > 0: flattened index of the tile's first pixel

    // DMA geometry (as in conv_sh_kernel): lane -> row rl + 32*pass of the region, 16-byte piece pc16/16
    const int gs = (lane & 15) ^ ((4 * wave + (lane >> 4)) & 15);
    const int rl = 8 * wave + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
    int apix[APASS];                                              // image pixel index of halo pixel rl + 32*i, or -1
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
        const int p = rl + RPP * i;
        if constexpr (IW > 0) {
            const int sb = p / HPS, q = p - sb * HPS, hy = q / (IW + 2), hx = q - hy * (IW + 2);
            const int first = pix0 + sb * SUBPX;                  // first pixel of the band: image first / IW^2, image row (first % IW^2) / IW
            const int img = first / (IW * IW), gy0 = (first - img * (IW * IW)) / IW;
            const int iy = gy0 - 1 + hy, ix = hx - 1;
            apix[i] = (p < HPX && (unsigned)iy < (unsigned)IW && (unsigned)ix < (unsigned)IW) ? (img * IW + iy) * IW + ix : -1;
        } else {
            const int hy = p / HPW, hx = p - hy * HPW;
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            apix[i] = (p < HPX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? (m * a.H + iy) * a.W + ix : -1;
        }
    }
    int wbase[BPASS];                                             // weight row (kx, co) = row rl + 32*i of a kernel-row stage
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
        const int r = rl + RPP * i, kx = r / BN, co = r - kx * BN;
        wbase[i] = r < BROWS ? ((col0 + co) * ksteps + kx * G) * 128 + pc16 : (int)0x80000000;
    }
    const rsrc_t rs1 = make_rsrc(a.src1, (size_t)a.M * a.H * a.W * a.C1 * 4);
    const rsrc_t rs2 = make_rsrc(a.src2 ? a.src2 : a.src1, a.src2 ? (size_t)a.M * a.H * a.W * a.C2 * 4 : 0);
    const rsrc_t rsw = make_rsrc(a.wt, (size_t)a.Cout * ksteps * 128);

    auto issue_a = [&](int g) {
        const bool first = g < G1;
        const int cs4 = (first ? a.C1 : a.C2) * 4;
        const int soff = (first ? g : g - G1) * 128 + pc16;
        unsigned char* sb = lds + wave * 1024;
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            if (wave + NW * i < HA_INSTR) {
                const int off = apix[i] >= 0 ? apix[i] * cs4 + soff : (int)0x80000000;
                if (OMNI_ABL(128)) {}
                else if (first) dma16(rs1, sb + i * (1024 * NW), off, 0);
                else       dma16(rs2, sb + i * (1024 * NW), off, 0);
            }
        }
    };
    // ---- UP2: this thread's cell of the halo and the byte offsets of its four source pixels
    const int Hl = a.H >> 1, Wl = a.W >> 1;
    const int u_c8 = t & 3, u_cell = t >> 2, u_ci = u_cell / 17, u_cj = u_cell - u_ci * 17;
    const int u_k = (y0 >> 1) - 1 + u_ci, u_j = (x0 >> 1) - 1 + u_cj;
    size_t u_src[4];
    float u_ly[2], u_lx[2];
    bool u_in[2][2];
    if constexpr (UP2) {
        const int ra = min(max(u_k, 0), Hl - 1), rb = min(max(u_k + 1, 0), Hl - 1), ca = min(max(u_j, 0), Wl - 1), cb = min(max(u_j + 1, 0), Wl - 1);
        const size_t pp = (size_t)a.C1 * 4, img = (size_t)m * Hl * Wl;
        u_src[0] = (img + (size_t)ra * Wl + ca) * pp + u_c8 * 16; u_src[1] = (img + (size_t)ra * Wl + cb) * pp + u_c8 * 16;
        u_src[2] = (img + (size_t)rb * Wl + ca) * pp + u_c8 * 16; u_src[3] = (img + (size_t)rb * Wl + cb) * pp + u_c8 * 16;
#pragma unroll
        for (int d = 0; d < 2; ++d) {                             // the weights of up-sample_sh8_kernel for rows / columns 2k+1+d
            const int oy = 2 * u_k + 1 + d, ox = 2 * u_j + 1 + d;
            const float fy = fmaxf(0.5f * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(0.5f * ((float)ox + 0.5f) - 0.5f, 0.0f);
            u_ly[d] = fy - (float)(int)fy; u_lx[d] = fx - (float)(int)fx;
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
                u_in[dy][dx] = (unsigned)(2 * u_k + 1 + dy) < (unsigned)a.H && (unsigned)(2 * u_j + 1 + dx) < (unsigned)a.W;
    }
    auto fill_a = [&](int g) {
        if (t >= 51 * 4) return;
        const unsigned char* sp = (const unsigned char*)a.src1 + (size_t)g * 128;
        h8v ch[4], cl[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ch[q] = *reinterpret_cast<const h8v*>(sp + u_src[q]); cl[q] = *reinterpret_cast<const h8v*>(sp + u_src[q] + 64); }
        float v[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[q][e] = fmaf((float)cl[q][e], 4.8828125e-4f, (float)ch[q][e]);
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float ly = u_ly[dy], lx = u_lx[dx], hy = 1.0f - ly, hx = 1.0f - lx;
                h8v oh, ol;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float o = hy * (hx * v[0][e] + lx * v[1][e]) + ly * (hx * v[2][e] + lx * v[3][e]);
                    const _Float16 hh = (fabsf(o) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)o;
                    oh[e] = u_in[dy][dx] ? hh : (_Float16)0.0f;
                    ol[e] = u_in[dy][dx] ? (_Float16)((o - (float)hh) * 2048.0f) : (_Float16)0.0f;
                }
                const int p = (2 * u_ci + dy) * HPW + 2 * u_cj + dx, d = p >> 1, pc = (p & 1) * 8 + u_c8;
                *reinterpret_cast<h8v*>(lds + d * 256 + ((pc ^ (d & 15)) * 16)) = oh;
                *reinterpret_cast<h8v*>(lds + d * 256 + (((pc + 4) ^ (d & 15)) * 16)) = ol;
            }
    };
    auto issue_b = [&](int g, int ky, int buf) {
        unsigned char* sb = lds + HA_BYTES + buf * B_BYTES + wave * 1024;
        const int soff = (ky * 3 * G + g) * 128;
#pragma unroll
        for (int i = 0; i < BPASS; ++i)
            if (wave + NW * i < BROWS / 8 && !OMNI_ABL(128)) dma16(rsw, sb + i * (1024 * NW), wbase[i], soff);
    };

    // pixel fragment offsets of the nine taps: halo pixel p = (wave+ky)*34 + (lane&31) + kx, row pair d = p >> 1,
    // first piece (hi, k chunk 0) at d*256 + 16*((8*(p&1) + (lane>>5)) ^ (d&15)); the other three pieces are that offset
    // XOR 32 / 64 / 96 (k chunk 1, lo chunk 0, lo chunk 1)
    int ao[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int p = (wave + ky) * HPW + (lane & 31) + kx;
            if constexpr (IW > 0) {
                const int tp = 32 * wave + (lane & 31), sb = tp / SUBPX, w_ = tp - sb * SUBPX, y = w_ / IW, x = w_ - y * IW;
                p = sb * HPS + (y + ky) * (IW + 2) + x + kx;
            }
            const int d = p >> 1;
            ao[ky * 3 + kx] = d * 256 + ((((p & 1) * 8 + (lane >> 5)) ^ (d & 15)) * 16);
        }
    int fo[4];                                                    // weight fragment offsets (32 consecutive rows)
    {
        const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) fo[k] = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
    }

    f16v acc[TN], acc1[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) { acc[j] = (f16v)(0.0f); acc1[j] = (f16v)(0.0f); }

    hstamp(63);
    if constexpr (UP2) { issue_b(0, 0, 0); fill_a(0); }            // (the weights travel while the halo is computed)
    else               { issue_a(0); issue_b(0, 0, 0); }
    int buf = 0;
    hstamp(1);
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            hstamp(4 + 4 * (3 * g + ky));
            wait_vm<0>();                                         // halo (ky == 0) and this kernel row's weights have landed
            wait_lds_reads();                                     // ... and my reads of the other weight buffer have returned
            if (!OMNI_ABL(256)) __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            hstamp(5 + 4 * (3 * g + ky));
            if (ky < 2) issue_b(g, ky + 1, buf ^ 1);              // next weights under this row's matrix work
            else if (g + 1 < G) issue_b(g + 1, 0, buf ^ 1);
            hstamp(6 + 4 * (3 * g + ky));
            const unsigned char* sB = lds + HA_BYTES + buf * B_BYTES;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int a0 = ao[ky * 3 + kx];
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const h8v ah = OMNI_ABL(512) ? (h8v)((_Float16)1.0f) : *reinterpret_cast<const h8v*>(lds + (a0 ^ (kc * 32)));
                    h8v al;
                    if constexpr (!X1) al = OMNI_ABL(512) ? (h8v)((_Float16)1.0f) : *reinterpret_cast<const h8v*>(lds + (a0 ^ (64 + kc * 32)));
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const unsigned char* bp = sB + (kx * BN + j * 32) * 128;
                        const h8v bh = OMNI_ABL(512) ? (h8v)((_Float16)1.0f) : *reinterpret_cast<const h8v*>(bp + fo[kc]);
                        h8v bl;
                        if constexpr (!X1) bl = OMNI_ABL(512) ? (h8v)((_Float16)1.0f) : *reinterpret_cast<const h8v*>(bp + fo[2 + kc]);
                        if (!OMNI_ABL(64)) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, ah, acc[j], 0, 0, 0);
                        if constexpr (!X1) {
                            if (!OMNI_ABL(16) && !OMNI_DBG(a, 16)) acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, ah, acc1[j], 0, 0, 0);
                            if (!OMNI_ABL(32) && !OMNI_DBG(a, 32)) acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, al, acc1[j], 0, 0, 0);
                        }
                    }
                }
            }
            buf ^= 1;
            hstamp(7 + 4 * (3 * g + ky));
        }
        if (g + 1 < G) {                                          // everybody is done with this group's halo: fetch the next
            wait_lds_reads();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if constexpr (UP2) fill_a(g + 1); else issue_a(g + 1);
        }
    }

    // ---- epilogue (as conv_sh_kernel): column lane & 31 = pixel x0 + (lane & 31) of image row y0 + wave
    const int r = IW > 0 ? pix0 + 32 * wave + (lane & 31) : (m * a.H + y0 + wave) * a.W + x0 + (lane & 31);
    int c0[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) c0[j] = col0 + j * 32;
    if (a.dst_sh && !a.res_f32 && a.epi_lds) {
        static_assert(TH * 32 * (32 * TN + 4) * 4 <= (int)sizeof(lds), "the transposition tiles must fit the K loop's buffers");
        wait_lds_reads();
        __syncthreads();                                          // every wave is done with the halo and the weights
        hstamp(2);
        epilogue_tile_lds<TN, true, X1>(acc, acc1, a, (size_t)(r - (lane & 31)), 32, c0, lane, reinterpret_cast<float*>(lds) + wave * (32 * (32 * TN + 4)));
        hstamp(62);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        hstamp(3); hdump();
        return;
    }
    hstamp(2);
    epilogue_row<TN, 4, X1>(acc, acc1, a, (size_t)r, c0, lane, a.dst_sh != 0);
    hstamp(3); hdump();
}

// ------------------------------------------------------------------ stem: conv 7x7 s2 p3, 3 -> 64, + folded BN + ReLU (f16x3)
// model/spherical_model.py:254 (conv1, bn1, relu) as an implicit GEMM on the fp16 matrix cores.  K is laid out as
// (c, ky, kx padded 7 -> 8): one 8-wide MFMA fragment is then 8 CONSECUTIVE input pixels of one (channel, kernel row) — four
// 4-byte reads from the input patch parked in LDS as a hi and a lo half image (split once per pixel at load time); K = 3*7*8 = 168, padded to 192 = 6
// groups of 32 with zero weights.  A block owns an 8-row strip of one patch's output (Po columns in tiles of 16): the 64 x 192
// pre-split filter bank (48 KiB) is DMA'd into LDS once per block, wave w owns output rows 2w, 2w+1 of the strip.
// Output: SH [M, Po, Po, 64].
constexpr int SM_TH = 8, SM_TW = 16, SM_IH = 2 * SM_TH + 5, SM_IW = 2 * SM_TW + 5, SM_IP = 40, SM_G = 6;

template <bool X1 = false>                                         // X1: f16x1 (acc_join)
__global__ __launch_bounds__(256) void stem_f16x3_kernel(const float* __restrict__ src, const void* __restrict__ wt16,
                                                         const float* __restrict__ bias, void* __restrict__ dst, int M, int P, int Po, int epi_lds)
{
    __shared__ __attribute__((aligned(1024))) unsigned char wl[64 * SM_G * 128];
    __shared__ __attribute__((aligned(16))) _Float16 imh[3 * SM_IH * SM_IP], iml[3 * SM_IH * SM_IP];   // the input patch, split ONCE per pixel
    __shared__ __attribute__((aligned(16))) float etile[4][32 * 36];                                     // a transposition tile per wave (epilogue_tile_lds, one 32-channel group at a time: two blocks per CU stay)
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int strips = Po / SM_TH;
    const int m = blockIdx.x / strips, oy0 = (blockIdx.x % strips) * SM_TH;

    // filter bank -> LDS: SM_G regions of 64 rows x 128 B, same pair swizzle as the convolution tiles
    {
        const int gs = (lane & 15) ^ ((4 * wave + (lane >> 4)) & 15);
        const int rl = 8 * wave + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
        const rsrc_t rsw = make_rsrc(wt16, (size_t)64 * SM_G * 128);
#pragma unroll
        for (int g = 0; g < SM_G; ++g)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                dma16(rsw, wl + g * 8192 + wave * 1024 + i * 4096, ((rl + 32 * i) * SM_G + g) * 128 + pc16, 0);
    }
    int fo[4];
    {
        const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) fo[k] = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
    }
    // this lane's output pixel inside a tile and its 12 fragment rows: fragment (g, kc) is input row (c, ky) = divmod(4g+2kc+h, 7)
    const int py = 2 * wave + ((lane & 31) >> 4), px = lane & 15;
    int rowoff[2 * SM_G];
#pragma unroll
    for (int f = 0; f < 2 * SM_G; ++f) {
        int rr = 2 * f + (lane >> 5);
        rr = rr < 21 ? rr : 20;                                   // rows 21..23 carry zero weights: any finite data will do
        rowoff[f] = ((rr / 7) * SM_IH + rr % 7 + 2 * py) * SM_IP + 2 * px;
    }
    ShConvArgs e;
    e.bias = bias; e.res = nullptr; e.res_f32 = 0; e.act = OMNI_ACT_RELU; e.Cout = 64; e.dst = dst; e.post = nullptr; e.post_rows = 1; e.epi_lds = epi_lds;

    // gridDim.y column ranges per strip (a lone panorama's 18 patches are 144 strips: a quarter strip per block fills the chip)
    const int ox_first = blockIdx.y * (Po / gridDim.y), ox_last = ox_first + Po / gridDim.y;
    // the next tile's input pixels travel (global -> registers) under the current tile's matrix work
    constexpr int IMG = 3 * SM_IH * SM_IP, IPT = (IMG + 255) / 256;
    float pre[IPT];
    auto prefetch = [&](int ox0) {
        const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {                           // (the pad columns 37..39 are read by the zero-weight kx = 7 lane slots)
            const int i = t + 256 * k;
            const int c = i / (SM_IH * SM_IP), r = (i % (SM_IH * SM_IP)) / SM_IP, q = i % SM_IP;
            const int iy = iy0 + r, ix = ix0 + q;
            pre[k] = (i < IMG && q < SM_IW && (unsigned)iy < (unsigned)P && (unsigned)ix < (unsigned)P) ? src[((size_t)m * 3 + c) * P * P + (size_t)iy * P + ix] : 0.0f;
        }
    };
    prefetch(ox_first);
    for (int ox0 = ox_first; ox0 < ox_last; ox0 += SM_TW) {
        __syncthreads();                                          // the previous tile's fragment reads are done
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            const int i = t + 256 * k;
            const float x = pre[k];
            const _Float16 hh = (fabsf(x) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)x;
            if (i < IMG) { imh[i] = hh; iml[i] = (_Float16)((x - (float)hh) * 2048.0f); }
        }
        if (ox0 == ox_first) wait_vm<0>();                        // the filter bank has landed
        __syncthreads();
        if (ox0 + SM_TW < ox_last) prefetch(ox0 + SM_TW);
        f16v acc[2], acc1[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) { acc[j] = (f16v)(0.0f); acc1[j] = (f16v)(0.0f); }
#pragma unroll
        for (int g = 0; g < SM_G; ++g)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                // 8 consecutive pixels from an even column: four 4-byte reads per half image (every input pixel serves ~28 fragments and
                // is split once, at load time)
                const int ro = rowoff[2 * g + kc];
                h8v ah, al;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const h2v xh = *reinterpret_cast<const h2v*>(imh + ro + 2 * u);
                    ah[2 * u] = xh[0]; ah[2 * u + 1] = xh[1];
                    if constexpr (!X1) { const h2v xl = *reinterpret_cast<const h2v*>(iml + ro + 2 * u); al[2 * u] = xl[0]; al[2 * u + 1] = xl[1]; }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned char* bp = wl + g * 8192 + j * 4096;
                    const h8v bh = *reinterpret_cast<const h8v*>(bp + fo[kc]);
                    h8v bl;
                    if constexpr (!X1) bl = *reinterpret_cast<const h8v*>(bp + fo[2 + kc]);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, ah, acc[j], 0, 0, 0);
                    if constexpr (!X1) {
                        acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, ah, acc1[j], 0, 0, 0);
                        acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, al, acc1[j], 0, 0, 0);
                    }
                }
            }
        const size_t r = ((size_t)m * Po + oy0 + py) * Po + ox0 + px;
        const int c0[2] = {0, 32};
        if (e.epi_lds) {                                          // 151 MB of output at 8 panoramas: as 16-byte pieces (the wave's two rows of 16 pixels)
            const size_t ra = ((size_t)m * Po + oy0 + 2 * wave) * Po + ox0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f16v ea[1] = {acc[j]}, eb[1] = {acc1[j]};
                const int cj[1] = {32 * j};
                epilogue_tile_lds<1, true, X1>(ea, eb, e, ra, 32, cj, lane, etile[wave], ra + Po);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        } else epilogue_row<2, 4, X1>(acc, acc1, e, r, c0, lane, true);
    }
}

// ---- the stem with producer / consumer waves (option conv_stem_pc)
// Twelve waves: 0-7 consume (fragment reads, 36 matrix instructions per tile, stores), 8-11 produce (input pixels global -> registers -> hi / lo
// split -> the NEXT tile's image in LDS, two image buffers) — loads and stores retire through one in-order counter, so a wave that does both
// waits for its previous stores' acknowledges whenever it waits for pixels (as conv3x3_up2_g1_kernel found); one block barrier per tile.
// Consumer wave w owns the two tile rows 2 (w & 3) and the 32 output channels of half w >> 2 (round 5; rounds 3-4: four consumers with both halves).
// With ONE consumer per SIMD a tile cost its K loop (2.8 us: 144 LDS reads whose latency nothing hid) PLUS its epilogue (2.7 us) — 95 us for 144
// patches with the matrix instructions themselves worth 12 (profiles/r05g_stem_ablations.txt); two consumers per SIMD run one's epilogue under the
// other's K loop.  The A fragments are read twice (LDS traffic per tile 2.3 -> 3.1 k cycles); every output element is the same sum as before.
template <bool X1 = false>                                         // X1: f16x1 (acc_join)
__global__ __launch_bounds__(768) void stem_f16x3_pc_kernel(const float* __restrict__ src, const void* __restrict__ wt16,
                                                         const float* __restrict__ bias, void* __restrict__ dst, int M, int P, int Po, int epi_lds, int tpb)
{
    constexpr int IMG = 3 * SM_IH * SM_IP, IPT = (IMG + 255) / 256;
    // rows are STORED 48 halfs apart (SM_IP = 40 are written and read): a wave's fragment read takes pixel rows y and y + 1 of two image rows each —
    // 2 x 40 halfs = 40 dwords apart they share 8 of 32 banks (every read two passes), 48 dwords apart none
    constexpr int SM_IS = 48, IMGS = 3 * SM_IH * SM_IS;
    __shared__ __attribute__((aligned(1024))) unsigned char wl[64 * SM_G * 128];
    __shared__ __attribute__((aligned(16))) _Float16 imh[2][IMGS], iml[2][IMGS];                          // the input patch of a tile, split ONCE per pixel; two tiles
    __shared__ __attribute__((aligned(16))) float etile[8][32 * 36];                                     // a transposition tile per consumer wave (epilogue_tile_lds: its 32-channel group)
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // A block walks tpb consecutive tiles of the flat sequence (patch, strip of SM_TH rows, SM_TW columns): a quarter strip where the launch is small
    // (a lone panorama's 18 patches are 576 tiles), 18 tiles = 4.5 strips at 8 panoramas — ONE block per CU for the whole launch: the filter bank is
    // loaded once per CU instead of 4.5 times and the producers' pipeline is filled once (round 5; before: a strip per block, 4 tiles, 19 us per block
    // of which 4 x ~2.5 were its tiles).
    const int sps = Po / SM_TH, tps = Po / SM_TW, ntiles = M * sps * tps;
    const int T0 = blockIdx.x * tpb, T1 = min(T0 + tpb, ntiles);
    if (T0 >= T1) return;
    auto where = [&](int T, int& m, int& oy0, int& ox0) { const int strip = T / tps; ox0 = (T - strip * tps) * SM_TW; m = strip / sps; oy0 = (strip - m * sps) * SM_TH; };

    if (wave >= 8) {
        // ---- producers
        const int ft = t - 512;
        float pre[IPT], nxt[IPT];
        // what does not depend on the tile, once per thread: the pixel's offset inside the patch's 3 x P x P image, its (row, column) inside the tile's
        // input window, its LDS slot (the index arithmetic — divisions by 840 and 40, 64-bit address products — was ~30 quarter-rate integer
        // multiplies per tile and wave: profiles/r05g_stem_ablations.txt)
        int po[IPT], rq[IPT], ls[IPT];
#pragma unroll
        for (int k = 0; k < IPT; ++k) {                           // (the pad columns 37..39 are read by the zero-weight kx = 7 lane slots)
            const int i = ft + 256 * k;
            const int c = i / (SM_IH * SM_IP), r = (i % (SM_IH * SM_IP)) / SM_IP, q = i % SM_IP;
            po[k] = (c * P + r) * P + q;
            rq[k] = (i < IMG && q < SM_IW) ? (r | (q << 8)) : -1;
            ls[k] = i < IMG ? (i / SM_IP) * SM_IS + q : -1;
        }
        // the tile whose pixels are fetched next: (patch, strip, column tile), divided once and stepped
        int fm, fs, fc;
        { const int strip = T0 / tps; fc = T0 - strip * tps; fm = strip / sps; fs = strip - fm * sps; }
        auto fetch = [&](float (&v)[IPT]) {                       // ... and steps to the following tile
            const int m = fm, oy0 = fs * SM_TH, ox0 = fc * SM_TW;
            if (++fc == tps) { fc = 0; if (++fs == sps) { fs = 0; ++fm; } }
            const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
            const float* base = src + (size_t)m * 3 * P * P + ((long long)iy0 * P + ix0);       // (wave-uniform; dereferenced only where the pixel exists)
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const int iy = iy0 + (rq[k] & 0xff), ix = ix0 + (rq[k] >> 8);
                v[k] = (rq[k] >= 0 && (unsigned)iy < (unsigned)P && (unsigned)ix < (unsigned)P) ? base[po[k]] : 0.0f;
            }
        };
        auto park = [&](int b, const float (&v)[IPT]) {
#pragma unroll
            for (int k = 0; k < IPT; ++k) {
                const float x = v[k];
                const _Float16 hh = (fabsf(x) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)x;
                if (ls[k] >= 0) { imh[b][ls[k]] = hh; iml[b][ls[k]] = (_Float16)((x - (float)hh) * 2048.0f); }
            }
        };
        // Two register sets in turn: a set is re-fetched (tile T + 2) as soon as it is parked — the loads are issued at the END of a tile's work, when the consumers are
        // in their epilogues, not behind the barrier where their fragment reads start (conv3x3_up2_g1_kernel's producers stood a whole K loop in front of their loads there:
        // profiles/r05h_up2_producer.txt, 8.-9.)
        fetch(pre);
        if (T0 + 1 < T1) fetch(nxt);
        park(0, pre);
        if (T0 + 2 < T1) fetch(pre);
        __syncthreads();                                          // (the consumers' first barrier)
        int b = 0, T = T0 + 1;
        for (;;) {
            if (T >= T1) break;
            b ^= 1; park(b, nxt);
            if (T + 2 < T1) fetch(nxt);
            __syncthreads();
            if (++T >= T1) break;
            b ^= 1; park(b, pre);
            if (T + 2 < T1) fetch(pre);
            __syncthreads();
            ++T;
        }
        return;
    }

    // ---- consumers.  filter bank -> LDS: SM_G regions of 64 rows x 128 B, same pair swizzle as the convolution tiles
    const int pr = wave & 3, cj = wave >> 2;                      // tile rows 2 pr, 2 pr + 1; output channels 32 cj .. 32 cj + 31
    {
        const int gs = (lane & 15) ^ ((4 * pr + (lane >> 4)) & 15);
        const int rl = 8 * pr + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
        const rsrc_t rsw = make_rsrc(wt16, (size_t)64 * SM_G * 128);
#pragma unroll
        for (int g = 0; g < SM_G; ++g)
            dma16(rsw, wl + g * 8192 + pr * 1024 + cj * 4096, ((rl + 32 * cj) * SM_G + g) * 128 + pc16, 0);
    }
    int fo[4];
    {
        const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) fo[k] = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
    }
    // this lane's output pixel inside a tile and its 12 fragment rows: fragment (g, kc) is input row (c, ky) = divmod(4g+2kc+h, 7)
    const int py = 2 * pr + ((lane & 31) >> 4), px = lane & 15;
    int rowoff[2 * SM_G];
#pragma unroll
    for (int f = 0; f < 2 * SM_G; ++f) {
        int rr = 2 * f + (lane >> 5);
        rr = rr < 21 ? rr : 20;                                   // rows 21..23 carry zero weights: any finite data will do
        rowoff[f] = ((rr / 7) * SM_IH + rr % 7 + 2 * py) * SM_IS + 2 * px;
    }
    ShConvArgs e;
    e.bias = bias; e.res = nullptr; e.res_f32 = 0; e.act = OMNI_ACT_RELU; e.Cout = 64; e.dst = dst; e.post = nullptr; e.post_rows = 1; e.epi_lds = epi_lds;
    wait_vm<0>();                                                 // the filter bank has landed
    __syncthreads();                                              // ... everybody's; the first image is there
    // the K loop of one tile (image buffer b) and the epilogue of one tile, as two steps: the channel halves run them in OPPOSITE order between two
    // barriers — half 0: K loop(T), epilogue(T); half 1: epilogue(T - 1), K loop(T) — so that of the two consumers of a SIMD one is in its
    // fragment reads / matrix instructions while the other is in its conversions / stores (in the same order both sat in the same phase: the
    // tile cost the SUM of the two chains whatever the number of waves)
    auto kloop = [&](int b, f16v (&acc)[1], f16v (&acc1)[1]) {
        const _Float16* ih = imh[b];
        const _Float16* il = iml[b];
        acc[0] = (f16v)(0.0f); acc1[0] = (f16v)(0.0f);
#pragma unroll
        for (int g = 0; g < SM_G; ++g)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                // 8 consecutive pixels from an even column: four 4-byte reads per half image (every input pixel serves ~28 fragments and
                // is split once, at load time)
                const int ro = rowoff[2 * g + kc];
                h8v ah, al;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const h2v xh = *reinterpret_cast<const h2v*>(ih + ro + 2 * u);
                    ah[2 * u] = xh[0]; ah[2 * u + 1] = xh[1];
                    if constexpr (!X1) { const h2v xl = *reinterpret_cast<const h2v*>(il + ro + 2 * u); al[2 * u] = xl[0]; al[2 * u + 1] = xl[1]; }
                }
                const unsigned char* bp = wl + g * 8192 + cj * 4096;
                const h8v bh = *reinterpret_cast<const h8v*>(bp + fo[kc]);
                h8v bl;
                if constexpr (!X1) bl = *reinterpret_cast<const h8v*>(bp + fo[2 + kc]);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, ah, acc[0], 0, 0, 0);
                if constexpr (!X1) {
                    acc1[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, ah, acc1[0], 0, 0, 0);
                    acc1[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, al, acc1[0], 0, 0, 0);
                }
            }
    };
    auto epi = [&](int T, const f16v (&acc)[1], const f16v (&acc1)[1]) {
        int m, oy0, ox0;
        where(T, m, oy0, ox0);
        const int c0[1] = {32 * cj};
        if (e.epi_lds) {                                          // 151 MB of output at 8 panoramas: as 16-byte pieces (the wave's two rows of 16 pixels)
            const size_t ra = ((size_t)m * Po + oy0 + 2 * pr) * Po + ox0;
            epilogue_tile_lds<1, true, X1>(acc, acc1, e, ra, 32, c0, lane, etile[wave], ra + Po);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else epilogue_row<1, 4, X1>(acc, acc1, e, ((size_t)m * Po + oy0 + py) * Po + ox0 + px, c0, lane, true);
    };
    f16v acc[1], acc1[1];
    int b = 0;
    if (cj == 0) {
        for (int T = T0; T < T1; ++T) {
            kloop(b, acc, acc1);
            epi(T, acc, acc1);
            if (T + 1 >= T1) break;                               // (the producers leave at the same point: no barrier after the last tile)
            wait_lds_reads();
            __syncthreads();                                      // this image buffer is free, the other one is complete
            b ^= 1;
        }
    } else {
        for (int T = T0; T < T1; ++T) {
            if (T > T0) epi(T - 1, acc, acc1);
            kloop(b, acc, acc1);
            if (T + 1 >= T1) break;
            wait_lds_reads();
            __syncthreads();
            b ^= 1;
        }
        epi(T1 - 1, acc, acc1);
    }
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_halo)

int omni_halo_launch(const void* args, int bn, int th, bool up2, int iw, bool x1, unsigned grid, hipStream_t s)
{
    ShConvArgs a;
    memcpy(&a, args, sizeof(a));
#define OMNI_HALO(BN, TH, UP2, IW) \
    if (bn == BN && th == TH && up2 == UP2 && iw == IW) { \
        if (x1) hipLaunchKernelGGL((conv3x3_halo_sh_kernel<BN, TH, UP2, IW, true>), dim3(grid), dim3(64 * TH), 0, s, a); \
        else    hipLaunchKernelGGL((conv3x3_halo_sh_kernel<BN, TH, UP2, IW, false>), dim3(grid), dim3(64 * TH), 0, s, a); \
        return OMNI_OK; }
    OMNI_HALO(32, 4, false, 16) OMNI_HALO(32, 4, false, 8) OMNI_HALO(64, 4, false, 16) OMNI_HALO(64, 4, false, 8)     // small square images
    OMNI_HALO(64, 8, false, 0) OMNI_HALO(32, 8, false, 0) OMNI_HALO(64, 4, false, 0) OMNI_HALO(32, 4, false, 0)       // wide images
    OMNI_HALO(64, 4, true, 0) OMNI_HALO(32, 4, true, 0)                                                               // the up-sampling halo
#undef OMNI_HALO
    OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_halo_launch: no conv3x3_halo_sh_kernel<" + std::to_string(bn) + ", " + std::to_string(th) + ", " + std::to_string((int)up2) +
                                    ", " + std::to_string(iw) + ">");        // a programming error, not a user error
}

// conv1 7x7 s2 p3 (3 -> 64) + bn1 + ReLU on the fp16 matrix cores.  src planar [M,3,P,P]; wt16: the folded filter bank as
// [64][192] with k = (c*7 + ky)*8 + kx (kx = 7 and k >= 168: zeros), split like every other f16x3 weight matrix
// ([64][6][hi32|lo32]); dst SH [M,P/2,P/2,64].
template <bool X1>
static int stem_sh_impl(const float* src, const void* wt16, const float* bias, void* dst, int M, int P, omni_stream_t stream)
{
    if (!src || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem: null pointer");
    if (P % 32 || M <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_sh_f16x3: patch size must be a multiple of 32");
    const int Po = P / 2;
    const int strips = M * (Po / SM_TH);
    const int split = (strips < 256 && Po % (4 * SM_TW) == 0) ? 4 : (strips < 512 && Po % (2 * SM_TW) == 0) ? 2 : 1;    // same bits either way
    if (omni_options().conv_stem_pc) {
        // tiles per block: the column range of the split above where the launch is small; one block per CU walking ntiles / CUs tiles where it is not
        const int tps = Po / SM_TW, ntiles = strips * tps;
        int tpb = tps / split;
        const int ncu = omni_num_cus();
        if (split == 1 && ntiles > ncu * tps) tpb = (ntiles + ncu - 1) / ncu;
        hipLaunchKernelGGL(stem_f16x3_pc_kernel<X1>, dim3((unsigned)((ntiles + tpb - 1) / tpb)), dim3(768), 0, (hipStream_t)stream, src, wt16, bias, dst, M, P, Po, omni_options().conv_epi_lds, tpb);
    }
    else hipLaunchKernelGGL(stem_f16x3_kernel<X1>, dim3(strips, split), dim3(256), 0, (hipStream_t)stream, src, wt16, bias, dst, M, P, Po, omni_options().conv_epi_lds);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
extern "C" int omni_stem_sh_f16x3(const float* src, const void* wt16, const float* bias, void* dst, int M, int P, omni_stream_t stream)
{
    return stem_sh_impl<false>(src, wt16, bias, dst, M, P, stream);
}
// the same with one matrix instruction per product block (f16x1: input hi x weight hi)
extern "C" int omni_stem_sh_f16x1(const float* src, const void* wt16, const float* bias, void* dst, int M, int P, omni_stream_t stream)
{
    return stem_sh_impl<true>(src, wt16, bias, dst, M, P, stream);
}
