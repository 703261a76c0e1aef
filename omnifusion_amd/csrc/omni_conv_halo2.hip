// omni_conv_halo2.hip — halo2_sh_kernel: the 3x3 stride-1 split-half halo convolution with 64 output channels per block (conv3x3_halo_sh_kernel<64, 4, false,
// 0 | 16> of omni_conv_halo.hip, the parent) on 256-pixel tiles with 64 x 64 WAVE tiles.  The SH layout, the LDS image and the shared device helpers:
// omni_conv_sh_common.h; the kernel choice (option conv_halo2): omni_conv_sh.hip.
//
// The parent's wave owns 32 pixels x 64 channels: per (tap, 16-channel chunk) it reads one pixel fragment pair (hi, lo) and two weight fragment pairs for six
// matrix instructions — 1 KiB of LDS per instruction — and its 4 x 32-pixel block fetches a 6 x 34 halo and all nine taps of weights per channel group.  Here:
//   * a block owns 8 x 32 pixels of one image (IW = 0: 10 x 34 halo) or one whole 16 x 16 image (IW = 16: 18 x 18 halo): the same 72 KiB of weights per group
//     serve twice the pixels and the halo overhead shrinks — 114.5 KiB of operands into LDS per 256 pixels and group instead of 195;
//   * a wave owns TWO pixel fragments p = 0, 1 x 64 channels, chosen so that fragment 1 is fragment 0 one image row further down (IW = 0: tile rows 2w and
//     2w + 1; IW = 16: image rows {4w, 4w + 2} and {4w + 1, 4w + 3}).  The pixel operand of fragment 1 at kernel row ky is then fragment 0's at ky + 1: it is
//     read once and KEPT in registers for the next kernel row.  Per group a wave reads 4 halo rows x 12 pixel fragments + 9 taps x 8 weight fragments = 120
//     ds_read_b128 for 216 matrix instructions (0.56 KiB each; the parent: 108 for 108);
//   * the weights arrive one TAP (64 rows, 8 KiB) at a time through a ring of four slots, three taps ahead of the matrix work: 43 KiB of halo + 32 KiB of
//     ring = 75 KiB, two blocks per CU as the parent (its 2 x 24-KiB kernel-row double buffer does not fit beside the larger halo).
// Same bits as the parent: every accumulator takes its products in the parent's order (group, ky, kx, chunk; acc: Wh.Ah, acc1: Wl.Ah then Wh.Al) and the
// epilogues are the shared helpers'.  Both arithmetic modes (X1) and the post-activation addend are supported, so no launch of these shapes falls back.
#include <string.h>
#include "omni_conv_sh_common.h"

namespace {

template <int IW, bool X1>
__global__ __launch_bounds__(256, 2) void halo2_sh_kernel(ShConvArgs a)
{
    static_assert(IW == 0 || IW == 16, "8 x 32 tiles of wide images, or whole 16 x 16 images");
    constexpr int BN = 64, TN = 2, NW = 4, RPP = 8 * NW, RING = 4, TROWS = 8;
    constexpr int HROW = IW > 0 ? IW + 2 : HPW;                   // pixels of a halo row
    constexpr int HPX = IW > 0 ? (IW + 2) * (IW + 2) : (TROWS + 2) * HPW, HA_INSTR = (HPX * 8 + 63) / 64, HA_BYTES = HA_INSTR * 1024;
    constexpr int APASS = (HA_INSTR + NW - 1) / NW, BPASS = BN / RPP, B_BYTES = BN * 128;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[HA_BYTES + RING * B_BYTES];
    static_assert(sizeof(lds) <= 80 * 1024, "two blocks per CU");

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);     // wave-uniform: LDS-DMA bases stay in scalar registers
    const int ntn = a.Cout / BN, tw = IW > 0 ? 1 : a.W / HT_W, th = IW > 0 ? 1 : a.H / TROWS;
    int bid = a.noxcd ? blockIdx.x : omni_xcd_remap(blockIdx.x, gridDim.x);   // neighbouring tiles (shared halos, same A for all tile_n) on one XCD
    const int tile_n = bid % ntn; bid /= ntn;
    const int tx = bid % tw; bid /= tw;
    const int ty = bid % th; const int m = bid / th;              // (IW > 0: m = image)
    const int y0 = ty * TROWS, x0 = tx * HT_W, col0 = tile_n * BN;
    const int G1 = a.C1 >> 5, G = (a.C1 + a.C2) >> 5, ksteps = 9 * G;

    // DMA geometry (as in conv3x3_halo_sh_kernel): lane -> row rl + 32*pass of the region, 16-byte piece pc16/16
    const int gs = (lane & 15) ^ ((4 * wave + (lane >> 4)) & 15);
    const int rl = 8 * wave + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
    // image pixel index of halo pixel p = rl + 32*i, or -1.  Recomputed per channel group from a laundered rl (eleven registers the K loop has no room for:
    // the compiler would hoist the eleven values out of the loop and spill them)
    auto halo_pixel = [&](int p) {
        const int hy = p / HROW, hx = p - hy * HROW;
        if constexpr (IW > 0) {
            const int iy = hy - 1, ix = hx - 1;
            return (p < HPX && (unsigned)iy < (unsigned)IW && (unsigned)ix < (unsigned)IW) ? (m * IW + iy) * IW + ix : -1;
        } else {
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            return (p < HPX && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? (m * a.H + iy) * a.W + ix : -1;
        }
    };
    int wbase[BPASS];                                             // weight row co = rl + 32*i of a tap's stage
#pragma unroll
    for (int i = 0; i < BPASS; ++i) wbase[i] = (col0 + rl + RPP * i) * ksteps * 128 + pc16;
    const rsrc_t rs1 = make_rsrc(a.src1, (size_t)a.M * a.H * a.W * a.C1 * 4);
    const rsrc_t rs2 = make_rsrc(a.src2 ? a.src2 : a.src1, a.src2 ? (size_t)a.M * a.H * a.W * a.C2 * 4 : 0);
    const rsrc_t rsw = make_rsrc(a.wt, (size_t)a.Cout * ksteps * 128);

    auto issue_a = [&](int g) {
        const bool first = g < G1;
        const int cs4 = (first ? a.C1 : a.C2) * 4;
        const int soff = (first ? g : g - G1) * 128 + pc16;
        unsigned char* sb = lds + wave * 1024;
        int rlv = rl;
        asm volatile("" : "+v"(rlv));
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            if (wave + NW * i < HA_INSTR) {
                const int px = halo_pixel(rlv + RPP * i);
                const int off = px >= 0 ? px * cs4 + soff : (int)0x80000000;
                if (first) dma16(rs1, sb + i * (1024 * NW), off, 0);
                else       dma16(rs2, sb + i * (1024 * NW), off, 0);
            }
        }
    };
    auto issue_b = [&](int g, int tap, int slot) {                // BPASS pieces per wave
        unsigned char* sb = lds + HA_BYTES + slot * B_BYTES + wave * 1024;
        const int soff = (tap * G + g) * 128;
#pragma unroll
        for (int i = 0; i < BPASS; ++i) dma16(rsw, sb + i * (1024 * NW), wbase[i], soff);
    };

    // pixel fragment offsets: halo row offset r = 0 .. 3 below the first halo row of the wave's fragment 0 (fragment p at kernel row ky: r = ky + p), kx;
    // halo pixel q, row pair d = q >> 1, first piece (hi, k chunk 0) at d*256 + 16*((8*(q&1) + (lane>>5)) ^ (d&15)); the other three pieces are that offset
    // XOR 32 / 64 / 96 (k chunk 1, lo chunk 0, lo chunk 1)
    int ao[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int q;
            if constexpr (IW > 0) q = (4 * wave + 2 * ((lane & 31) >> 4) + r) * HROW + (lane & 15) + kx;
            else                  q = (2 * wave + r) * HROW + (lane & 31) + kx;
            const int d = q >> 1;
            ao[r][kx] = d * 256 + ((((q & 1) * 8 + (lane >> 5)) ^ (d & 15)) * 16);
        }
    int fo[4];                                                    // weight fragment offsets (32 consecutive rows)
    {
        const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
        for (int k = 0; k < 4; ++k) fo[k] = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
    }

    f16v acc[2][TN], acc1[2][TN];                                 // [pixel fragment][channel tile]
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < TN; ++j) { acc[p][j] = (f16v)(0.0f); acc1[p][j] = (f16v)(0.0f); }
    h8v kh[3][2], kl[3][2];                                       // the kept pixel fragments (kx, chunk) of halo row offset ky: fragment 0's operand at ky

    issue_a(0);
    issue_b(0, 0, 0); issue_b(0, 1, 1); issue_b(0, 2, 2);
    int T = 0;                                                    // taps done, all groups: tap T lives in ring slot T & 3
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            // my pieces of tap T have landed (taps T + 1, T + 2 may be in flight; the halo was issued behind them: everything at tap 0)
            if (tap == 0 || T + 1 >= ksteps) wait_vm<0>();
            else if (T + 2 >= ksteps) wait_vm<BPASS>();
            else wait_vm<2 * BPASS>();
            wait_lds_reads();                                     // ... and my reads of slot (T - 1) & 3 have returned
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (T + 3 < ksteps) {                                 // tap T + 3 into the slot tap T - 1 occupied
                if (tap + 3 < 9) issue_b(g, tap + 3, (T + 3) & 3);
                else             issue_b(g + 1, tap + 3 - 9, (T + 3) & 3);
            }
            const unsigned char* sB = lds + HA_BYTES + (T & 3) * B_BYTES;
            // (laundered: the compiler would otherwise hoist all 48 XORed fragment addresses out of the group loop and spill)
            int a_old = ao[0][kx], a_new = ao[ky + 1][kx];
            asm volatile("" : "+v"(a_old), "+v"(a_new));
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                if (ky == 0) {
                    kh[kx][kc] = *reinterpret_cast<const h8v*>(lds + (a_old ^ (kc * 32)));
                    if constexpr (!X1) kl[kx][kc] = *reinterpret_cast<const h8v*>(lds + (a_old ^ (64 + kc * 32)));
                }
                const h8v nh = *reinterpret_cast<const h8v*>(lds + (a_new ^ (kc * 32)));
                h8v nl;
                if constexpr (!X1) nl = *reinterpret_cast<const h8v*>(lds + (a_new ^ (64 + kc * 32)));
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const unsigned char* bp = sB + j * 32 * 128;
                    const h8v bh = *reinterpret_cast<const h8v*>(bp + fo[kc]);
                    h8v bl;
                    if constexpr (!X1) bl = *reinterpret_cast<const h8v*>(bp + fo[2 + kc]);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, kh[kx][kc], acc[0][j], 0, 0, 0);
                    if constexpr (!X1) {
                        acc1[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, kh[kx][kc], acc1[0][j], 0, 0, 0);
                        acc1[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, kl[kx][kc], acc1[0][j], 0, 0, 0);
                    }
                    acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, nh, acc[1][j], 0, 0, 0);
                    if constexpr (!X1) {
                        acc1[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, nh, acc1[1][j], 0, 0, 0);
                        acc1[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, nl, acc1[1][j], 0, 0, 0);
                    }
                }
                kh[kx][kc] = nh;                                  // fragment 1's operand at ky is fragment 0's at ky + 1
                if constexpr (!X1) kl[kx][kc] = nl;
            }
            ++T;
        }
        if (g + 1 < G) {                                          // everybody is done with this group's halo: fetch the next
            wait_lds_reads();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            issue_a(g + 1);
        }
    }

    // ---- epilogue (the shared helpers): fragment p, column lane & 31 -> pixel row r0 + (lane & 15) of the first run of 16, r1 + (lane & 15) of the second
    int c0[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) c0[j] = col0 + j * 32;
    size_t r0[2], r1[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if constexpr (IW > 0) { r0[p] = ((size_t)m * IW + 4 * wave + p) * IW; r1[p] = r0[p] + 2 * IW; }
        else                  { r0[p] = ((size_t)m * a.H + y0 + 2 * wave + p) * a.W + x0; r1[p] = r0[p] + 16; }
    }
    if (a.dst_sh && !a.res_f32 && a.epi_lds) {
        static_assert(NW * 32 * (32 * TN + 4) * 4 <= (int)sizeof(lds), "the transposition tiles must fit the K loop's buffers");
        wait_lds_reads();
        __syncthreads();                                          // every wave is done with the halo and the weights
        float* tile = reinterpret_cast<float*>(lds) + wave * (32 * (32 * TN + 4));
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            epilogue_tile_lds<TN, true, X1>(acc[p], acc1[p], a, r0[p], 32, c0, lane, tile, r1[p]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // (the wave's reads of its tile have returned before fragment 1 overwrites it)
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const size_t r = ((lane & 31) < 16 ? r0[p] : r1[p]) + (lane & 15);
#pragma unroll
        for (int j = 0; j < TN; ++j) {                            // 128 accumulator registers are live: one channel tile, two register quads at a time
            const f16v ea[1] = {acc[p][j]}, eb[1] = {acc1[p][j]};
            const int cj[1] = {c0[j]};
            epilogue_row<1, 2, X1>(ea, eb, a, r, cj, lane, a.dst_sh != 0);
        }
    }
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_halo2)         // this translation unit's copy of the sticky range flag

int omni_halo2_launch(const void* args, int iw, bool x1, unsigned grid, hipStream_t s)
{
    ShConvArgs a;
    memcpy(&a, args, sizeof(a));
    const dim3 block(256);
    if (iw == 16 && !x1)     hipLaunchKernelGGL((halo2_sh_kernel<16, false>), dim3(grid), block, 0, s, a);
    else if (iw == 16)       hipLaunchKernelGGL((halo2_sh_kernel<16, true>), dim3(grid), block, 0, s, a);
    else if (iw == 0 && !x1) hipLaunchKernelGGL((halo2_sh_kernel<0, false>), dim3(grid), block, 0, s, a);
    else if (iw == 0)        hipLaunchKernelGGL((halo2_sh_kernel<0, true>), dim3(grid), block, 0, s, a);
    else OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_halo2_launch: no halo2_sh_kernel<" + std::to_string(iw) + ">");      // a programming error, not a user error
    return OMNI_OK;
}
