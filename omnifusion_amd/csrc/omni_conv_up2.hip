// omni_conv_up2.hip — the decoder's up-sampling convolutions: conv3x3_up2_g1_kernel (de_conv4_0, persistent, optionally with the two heads fused),
// heads_finish_kernel, and the entry points omni_conv3x3_up2_sh_f16x3, omni_conv3x3_up2_heads_sh_f16x3 / _f16x1, omni_heads_pack_f16x3.
// The other up-sampling shapes run conv3x3_halo_sh_kernel<.., UP2> (omni_conv_halo.hip) through omni_halo_launch.
#include "omni_conv_sh_common.h"
#include "omni_heads_hr.h"

namespace {

// ------------------------------------------------------------------ de_conv4_0: conv3x3(up2(x)), 32 -> 32 channels, PERSISTENT
// conv3x3_halo_sh_kernel<32, 4, UP2> spends 12.8 us per block at this shape (144 patches, 128 x 128 outputs: 18 432 blocks) around 0.72 us
// of matrix work: a chain of dependent round trips — the source pixels of the halo, three kernel-row weight stages each issued one 0.24-us
// matrix phase ahead of its use, the bias, the stores — that twelve waves per CU do not hide (19 % MFMA-busy).  With ONE input group all
// nine taps of the weights are 36 KiB: here a block keeps them in LDS for its whole life and walks over tiles, and its eight waves split
// the work by what they WAIT for (loads and stores retire through one in-order counter: a wave that does both waits for its previous
// tile's store acknowledges whenever it waits for pixels — measured: 277 us, as slow as the kernel this replaces):
//   waves 4-7, producers: source pixels global -> registers -> up-sampling arithmetic -> the halo of tile k+1 in LDS (two halo buffers);
//   waves 0-3, consumers: 54 matrix instructions per wave on the halo of tile k, bias from registers, stores — never a wait on memory.
// One block barrier per tile hands the buffers over.  Same cells, same K order (ky, kx, k chunk): same bits as the kernel it replaces.
//
// HEADS (round 5): the `pred` / `weight_pred` heads (3x3, 32 -> 1 each, model/spherical_model.py:223-224,304-306) start HERE instead of in a kernel
// that re-reads this one's output: de_conv4_0's result is the widest tensor of the network (302 MB at 8 panoramas, written once and read once by
// heads_kernel: 290 us for the pair) and never exists in this form.  out[q] = sum_{dy,dx} w[dy][dx] . x[q + (dy,dx)] is turned around: pixel p, where
// x[p] lives in registers, contributes w[dy][dx] . x[p] to q = p - (dy,dx) — eighteen 32-channel dot products per pixel (9 taps x 2 heads), which are
// ONE more matrix product: rows = (dy, head, dx), k = the 32 channels in the order the accumulator quads already hold them (a lane's 16 channels
// are its two k chunks: no data movement), three f16x3 terms like every other product = 6 matrix instructions per wave and tile beside the 54 of
// the convolution.  The product, the sum of its three dx terms across neighbouring lanes and the record `hr` they leave — 3.4 KB per tile instead of
// 16 KB — are omni_heads_hr.h's.  heads_finish_kernel adds the three rows (dy) and the neighbour tiles' outer sums in a fixed order, then bias, ReLU /
// sigmoid and the product.  Deterministic; equal to heads_kernel up to fp32 summation order.
struct HeadsArgs { const void* w16; float* hr; };           // w16: the heads' weights in fragment order (Engine: heads.w16f), [hi kc0, hi kc1, lo kc0, lo kc1][64 lanes] x 16 B

template <bool HEADS, bool X1 = false>                       // X1: f16x1 for the convolution (acc_join); the heads' own products stay f16x3
__global__ __launch_bounds__(HEADS ? 64 * (4 + OMNI_G1_PW) : 512) void conv3x3_up2_g1_kernel(ShConvArgs a, int ntiles, HeadsArgs hd)
{
    constexpr int BN = 32, TH = 4, NW = 4, RPP = 8 * NW;
    constexpr int PW = HEADS ? OMNI_G1_PW : 4, CPT = 32 / PW;    // producer waves, channels per producer thread
    constexpr int HPX = (TH + 2) * HPW, HA_INSTR = (HPX * 8 + 63) / 64, HA_BYTES = HA_INSTR * 1024;
    constexpr int BROWS = 3 * BN, BPASS = (BROWS + RPP - 1) / RPP, B_BYTES = BROWS * 128, W_OFF = 2 * HA_BYTES;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * HA_BYTES + 3 * B_BYTES];
    // (ablation 32768, tools/g1_stamps.py: s_memtime of consumer wave 0 / producer wave 4 of block 0 at three points of each of its first 40 tiles, written over hd.hr at the end)
    constexpr int ST_N = 40, ST_K = 5;
    __shared__ long long stamps[OMNI_ABL(32768) ? 2 * ST_N * ST_K : 1];
    auto stamp = [&](int who, int it, int k) { if (OMNI_ABL(32768) && blockIdx.x == 0 && it < ST_N && (threadIdx.x & 63) == 0) stamps[(who * ST_N + it) * ST_K + k] = clock64(); };

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool consumer = wave < NW;
    const int tw = a.W / HT_W, th = a.H / TH, per_img = tw * th;
    // tiles of this block: XCD x (blocks x mod 8) owns one contiguous range of tiles, its blocks walk it with stride gridDim.x / 8
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3, nlb = gridDim.x >> 3;
    const int per = (ntiles + 7) >> 3, t_end = min(ntiles, (xcd + 1) * per);
    int tile = xcd * per + lb;
    if (tile >= t_end) return;
    // tile -> (patch, tile row, tile column): divided ONCE per wave, then stepped — a producer spent 2400 of its 6400 cycles per tile in front of its loads, most of them
    // in the three integer divisions per tile index (two indices per tile: profiles/r05h_up2_producer.txt, 8.)
    struct TileXY { int m, ty, tx; };
    auto coords = [&](int tl) { TileXY c; c.m = tl / per_img; const int r = tl - c.m * per_img; c.ty = r / tw; c.tx = r - c.ty * tw; return c; };
    const TileXY tstep = coords(nlb);
    auto advance = [&](TileXY& c) { c.tx += tstep.tx; c.ty += tstep.ty; c.m += tstep.m; if (c.tx >= tw) { c.tx -= tw; ++c.ty; } if (c.ty >= th) { c.ty -= th; ++c.m; } };

    if (consumer) {
        // ---- the nine taps' weights, once (three kernel-row stages of the halo kernel's layout, side by side)
        const int gs = (lane & 15) ^ ((4 * wave + (lane >> 4)) & 15);
        const int rl = 8 * wave + 2 * (lane >> 4) + (gs >> 3), pc16 = (gs & 7) * 16;
        const rsrc_t rsw = make_rsrc(a.wt, (size_t)a.Cout * 9 * 128);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int i = 0; i < BPASS; ++i) {
                const int r = rl + RPP * i, kx = r / BN, co = r - kx * BN;
                if (wave + NW * i < BROWS / 8) dma16(rsw, lds + W_OFF + ky * B_BYTES + wave * 1024 + i * (1024 * NW), (co * 9 + kx) * 128 + pc16, ky * 3 * 128);
            }
        f4v bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = a.bias ? *reinterpret_cast<const f4v*>(a.bias + 8 * q + 4 * (lane >> 5)) : (f4v)(0.0f);
        h8v hwf[4];                                              // HEADS: this lane's weight fragments (row lane & 31, k chunk lane >> 5)
        if constexpr (HEADS) {
#pragma unroll
            for (int k = 0; k < 4; ++k) hwf[k] = *reinterpret_cast<const h8v*>((const unsigned char*)hd.w16 + k * 1024 + lane * 16);
        }
        int ao[9], fo[4];                                        // fragment offsets, as in conv3x3_halo_sh_kernel
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int p = (wave + ky) * HPW + (lane & 31) + kx, d = p >> 1;
                ao[ky * 3 + kx] = d * 256 + ((((p & 1) * 8 + (lane >> 5)) ^ (d & 15)) * 16);
            }
        {
            const int r = lane & 31, v = r >> 1, h = lane >> 5;
#pragma unroll
            for (int k = 0; k < 4; ++k) fo[k] = v * 256 + ((((r & 1) * 8 + 2 * k + h) ^ v) * 16);
        }
        wait_vm<0>();                                             // weights (and bias) have landed
        __syncthreads();                                          // ... everybody's; the first halo is there
        TileXY ct = coords(tile);                                  // (the epilogue's tile)
        for (int it = 0;; ++it, advance(ct)) {
            const unsigned char* ha = lds + (it & 1) * HA_BYTES;
            if (wave == 0) stamp(0, it, 0);
            // the eight fragments of tap k+1 are read while the six matrix instructions of tap k run
            f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f), accx = (f16v)(0.0f), accy = (f16v)(0.0f);
            h8v fa[2][4], fb[2][4];                               // [buffer][hi k0, hi k1, lo k0, lo k1] of the pixels / of the weights
            auto read_tap = [&](int tap, int bf) {
                const int a0 = ao[tap];
                const unsigned char* bp = lds + W_OFF + (tap / 3) * B_BYTES + ((tap % 3) * BN) * 128;
#pragma unroll
                for (int k = 0; k < (X1 ? 2 : 4); ++k) {                   // (f16x1: the hi pieces only)
                    if (OMNI_ABL(512)) { fa[bf][k] = (h8v)((_Float16)(float)(a0 & 3)); fb[bf][k] = (h8v)((_Float16)(float)(fo[k] & 3)); continue; }   // (ablation: no fragment reads)
                    fa[bf][k] = *reinterpret_cast<const h8v*>(ha + (a0 ^ (k * 32)));
                    fb[bf][k] = *reinterpret_cast<const h8v*>(bp + fo[k]);
                }
            };
            read_tap(0, 0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int bf = tap & 1;
                __builtin_amdgcn_sched_barrier(0);
                if (tap + 1 < 9) read_tap(tap + 1, bf ^ 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    if (!X1 && OMNI_ABL(8192)) {                  // (ablation: four accumulators instead of two — another summation order)
                        if (kc == 0) { acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][kc], acc, 0, 0, 0);
                                       acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][2 + kc], fa[bf][kc], acc1, 0, 0, 0);
                                       accx = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][2 + kc], accx, 0, 0, 0); }
                        else         { accy = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][kc], accy, 0, 0, 0);
                                       accx = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][2 + kc], fa[bf][kc], accx, 0, 0, 0);
                                       acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][2 + kc], acc1, 0, 0, 0); }
                        continue;
                    }
                    if (!OMNI_ABL(64)) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][kc], acc, 0, 0, 0);
                    else acc[0] += (float)fb[bf][kc][0] * (float)fa[bf][kc][0] + (float)fb[bf][2 + kc][0] * (float)fa[bf][2 + kc][0];
                    if constexpr (!X1) {
                        if (!OMNI_ABL(16)) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][2 + kc], fa[bf][kc], acc1, 0, 0, 0);
                        if (!OMNI_ABL(32)) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[bf][kc], fa[bf][2 + kc], acc1, 0, 0, 0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (OMNI_ABL(8192)) { acc += accy; acc1 += accx; }
            if (wave == 0) stamp(0, it, 1);
            if constexpr (HEADS) if (OMNI_ABL(16384)) { if (acc[0] == 12345.678f && acc1[3] == 3.0f) hd.hr[lane] = acc[1]; } else {
                // the tile's result stays in registers: v[q] = channels 8q + 4h .. + 3 of pixel lane & 31 — the lane's k chunk kc is its quads 2kc, 2kc + 1
                h8v ph[2], pl[2];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f4v v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[4 * q + e], acc[4 * q + e]);
                    v += bq[q];
                    if (a.act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    h4v hi, lo; sh_split4(v, hi, lo);            // (the split every SH epilogue does: range guard included)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ph[q >> 1][4 * (q & 1) + e] = hi[e]; pl[q >> 1][4 * (q & 1) + e] = lo[e]; }
                }
                if (OMNI_ABL(32768)) { if (ph[0][0] == (_Float16)77.0f && pl[1][3] == (_Float16)3.0f) hd.hr[1] = 1.0f; if (wave == 0) stamp(0, it, 2); }
                f16v d0, d1;
                heads_product(hwf, ph, pl, d0, d1);
                if (OMNI_ABL(32768)) { if (d0[0] == 12345.678f && d1[5] == 3.0f) hd.hr[2] = 1.0f; if (wave == 0) stamp(0, it, 3); }
                const int px = lane & 31, h = lane >> 5;
                float* hp = hd.hr + ((size_t)tile * TH + wave) * (6 * HR_PITCH);
                OMNI_HEADS_HR_WRITE(d0, d1, hp, px, h)
            } else
            {   // epilogue of this tile: column lane & 31 = pixel x0 + (lane & 31) of image row y0 + wave (through an LDS transposition, split-half or
                // fp32: 247 | 248 us — the stores are not this kernel's limit, and 18 KB of LDS more per block are felt beside other kernels)
                const int m = ct.m, y0 = ct.ty * TH, x0 = ct.tx * HT_W;
                const size_t r = (size_t)(m * a.H + y0 + wave) * a.W + x0 + (lane & 31);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f4v v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc_join<X1>(acc1[4 * q + e], acc[4 * q + e]);
                    v += bq[q];
                    if (a.act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                    else if (a.act == OMNI_ACT_GELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
                    }
                    const size_t o = r * BN + 8 * q + 4 * (lane >> 5);
                    if (OMNI_ABL(2048)) { if (v.x == 12345.678f) act_store4<false>(a.dst, o, v); }
                    else if (a.dst_sh) act_store4<true>(a.dst, o, v);
                    else               act_store4<false>(a.dst, o, v);
                }
            }
            if (wave == 0) stamp(0, it, 4);
            tile += nlb;
            if (tile >= t_end) break;
            wait_lds_reads();
            __syncthreads();                                      // this halo buffer is free, the other one is complete
        }
        if (OMNI_ABL(32768) && blockIdx.x == 0 && wave == 0 && lane == 0) for (int i = 0; i < ST_N * ST_K; ++i) reinterpret_cast<long long*>(hd.hr)[i] = stamps[i];
        return;
    }

    // ---- producers: thread (cell, CPT channels) of the 3 x 17 cells of 2 x 2 pixels of a tile's halo (see conv3x3_halo_sh_kernel, UP2); PW = 4 producer waves: 8 channels
    // per thread (the product); PW = 8: 4 channels per thread, two producer waves per SIMD (-DOMNI_G1_PW=8: measured equal, profiles/r05h_up2_producer.txt)
    using hcv = std::conditional_t<CPT == 8, h8v, h4v>;
    const int ft = t - 64 * NW;
    const int Hl = a.H >> 1, Wl = a.W >> 1;
    constexpr int TPC = 32 / CPT;                                 // threads per cell
    const int u_cg = ft % TPC, u_cell = ft / TPC, u_ci = u_cell / 17, u_cj = u_cell - u_ci * 17;
    const int u_c8 = u_cg * CPT / 8, u_sub = (u_cg * CPT % 8) * 2; // 16-byte piece (8 channels) and byte offset inside it
    const bool filler = ft < 51 * TPC;
    auto load_src = [&](const TileXY& c, hcv (&ch)[4], hcv (&cl)[4]) {
        if (!filler) return;
        const int m = c.m, y0 = c.ty * TH, x0 = c.tx * HT_W;
        const int u_k = (y0 >> 1) - 1 + u_ci, u_j = (x0 >> 1) - 1 + u_cj;
        const int ra = min(max(u_k, 0), Hl - 1), rb = min(max(u_k + 1, 0), Hl - 1), ca = min(max(u_j, 0), Wl - 1), cb = min(max(u_j + 1, 0), Wl - 1);
        const size_t img = (size_t)m * Hl * Wl;
        const unsigned char* sp = (const unsigned char*)a.src1 + u_cg * (CPT * 2);
        const size_t so[4] = {(img + (size_t)ra * Wl + ca) * 128, (img + (size_t)ra * Wl + cb) * 128, (img + (size_t)rb * Wl + ca) * 128, (img + (size_t)rb * Wl + cb) * 128};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (OMNI_ABL(4096)) { ch[q] = (hcv)((_Float16)1.0f); cl[q] = ch[q]; }
            else { ch[q] = *reinterpret_cast<const hcv*>(sp + so[q]); cl[q] = *reinterpret_cast<const hcv*>(sp + so[q] + 64); }
        }
    };
    auto write_halo = [&](const TileXY& c, unsigned char* hb, const hcv (&ch)[4], const hcv (&cl)[4], int it) {
        if (!filler || OMNI_ABL(1024)) return;
        const int y0 = c.ty * TH, x0 = c.tx * HT_W;
        const int u_k = (y0 >> 1) - 1 + u_ci, u_j = (x0 >> 1) - 1 + u_cj;
        float v[4][CPT];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < CPT; ++e) v[q][e] = fmaf((float)cl[q][e], 4.8828125e-4f, (float)ch[q][e]);
        if (OMNI_ABL(32768)) { float z = 0.0f; for (int q = 0; q < 4; ++q) for (int e = 0; e < CPT; ++e) z += v[q][e]; if (z == 12345.678f) hd.hr[0] = z; if (wave == NW) stamp(1, it, 1); }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int oy = 2 * u_k + 1 + dy, ox = 2 * u_j + 1 + dx;
                const float fy = fmaxf(0.5f * ((float)oy + 0.5f) - 0.5f, 0.0f), fx = fmaxf(0.5f * ((float)ox + 0.5f) - 0.5f, 0.0f);
                const float ly = fy - (float)(int)fy, lx = fx - (float)(int)fx, hy = 1.0f - ly, hx = 1.0f - lx;
                const bool in = (unsigned)oy < (unsigned)a.H && (unsigned)ox < (unsigned)a.W;
                hcv oh, ol;
#pragma unroll
                for (int e = 0; e < CPT; ++e) {
                    const float o = hy * (hx * v[0][e] + lx * v[1][e]) + ly * (hx * v[2][e] + lx * v[3][e]);
                    const _Float16 hh = (fabsf(o) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)o;
                    oh[e] = in ? hh : (_Float16)0.0f;
                    ol[e] = in ? (_Float16)((o - (float)hh) * 2048.0f) : (_Float16)0.0f;
                }
                const int p = (2 * u_ci + dy) * HPW + 2 * u_cj + dx, d = p >> 1, pc = (p & 1) * 8 + u_c8;
                *reinterpret_cast<hcv*>(hb + d * 256 + ((pc ^ (d & 15)) * 16) + u_sub) = oh;
                *reinterpret_cast<hcv*>(hb + d * 256 + (((pc + 4) ^ (d & 15)) * 16) + u_sub) = ol;
            }
            if (dy == 0 && wave == NW) stamp(1, it, 2);
        }
    };
    // the pixels of tile k+2 are on their way while the halo of tile k+1 is computed (a producer issues no stores: its waits are for loads only)
    // Two register sets in turn, no copies: a set is re-loaded (tile k+2) as soon as its halo (tile k) is written — the loads are issued at the END of a tile's work,
    // the arithmetic starts right behind the barrier.
    hcv rh[2][4], rl_[2][4];
    TileXY cw = coords(tile), cn = cw;                            // the tile whose halo is written next / the tile loaded last
    load_src(cw, rh[0], rl_[0]);
    advance(cn);
    if (tile + nlb < t_end) load_src(cn, rh[1], rl_[1]);
    write_halo(cw, lds, rh[0], rl_[0], ST_N);
    cw = cn; advance(cn);
    if (tile + 2 * nlb < t_end) load_src(cn, rh[0], rl_[0]);
    __syncthreads();                                              // (the consumers' first barrier)
    int it = 0;
#define OMNI_G1_STEP(SET) { \
        const int next = tile + nlb; \
        if (wave == NW) stamp(1, it, 0); \
        if (next >= t_end) break;                                 /* (the consumers leave at the same point: no barrier after the last tile) */ \
        write_halo(cw, lds + ((it + 1) & 1) * HA_BYTES, rh[SET], rl_[SET], it); \
        if (wave == NW) stamp(1, it, 3); \
        cw = cn; advance(cn); \
        if (next + 2 * nlb < t_end) load_src(cn, rh[SET], rl_[SET]); \
        if (wave == NW) stamp(1, it, 4); \
        __syncthreads(); \
        tile = next; ++it; }
    for (;;) {
        OMNI_G1_STEP(1)
        OMNI_G1_STEP(0)
    }
#undef OMNI_G1_STEP
    if (OMNI_ABL(32768) && blockIdx.x == 0 && wave == NW && lane == 0) for (int i = 0; i < ST_N * ST_K; ++i) reinterpret_cast<long long*>(hd.hr)[ST_N * ST_K + i] = stamps[ST_N * ST_K + i];
}

// Second half of the fused heads (see conv3x3_up2_g1_kernel<HEADS>): one thread per output pixel adds, for each head, the partial sums of the three
// source rows (dy = -1, 0, +1: row y + dy of its tile, (dy, head) plane, position 1 + x % 32) and, at a tile's first / last column, the outer sums
// of the horizontally neighbouring tile (its pixel 32 / pixel -1 slots) — in that fixed order — then heads_kernel's own tail (bias, ReLU, sigmoid, product).
__global__ __launch_bounds__(256) void heads_finish_kernel(const float* __restrict__ hr, float bp, float bw, float* __restrict__ outa, float* __restrict__ outc,
                                                           int M, int P, int conf)
{
    const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;  // four consecutive pixels of a row per thread (16-byte loads and stores)
    if (i4 >= (size_t)M * P * P / 4) return;
    const size_t i = i4 * 4;
    const int x = (int)(i % P), y = (int)((i / P) % P), m = (int)(i / ((size_t)P * P));
    const int tw = P / HT_W, th = P / 4, c = x & 31;
    f4v s[2] = {(f4v)(0.0f), (f4v)(0.0f)};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int py = y + dy;
        if ((unsigned)py >= (unsigned)P) continue;
        const size_t tile = ((size_t)m * th + (py >> 2)) * tw + (x >> 5);
        const float* rowp = hr + (tile * 4 + (py & 3)) * (6 * HR_PITCH) + (dy + 1) * 2 * HR_PITCH;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            s[hd] += *reinterpret_cast<const f4v*>(rowp + hd * HR_PITCH + c);
            if (c == 0 && x > 0) s[hd].x += rowp[hd * HR_PITCH + 33 - 4 * 6 * HR_PITCH];        // the left neighbour tile's pixel 32
            if (c == 28 && x + 4 < P) s[hd].w += rowp[hd * HR_PITCH + 32 + 4 * 6 * HR_PITCH];   // the right neighbour tile's pixel -1
        }
    }
    f4v oa, oc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ap = s[0][e] + bp, aw = s[1][e] + bw;
        const float pr = fmaxf(ap, 0.0f), cf = 1.0f / (1.0f + expf(-aw));
        oa[e] = conf ? pr * cf : pr; oc[e] = cf;
    }
    *reinterpret_cast<f4v*>(outa + i) = oa;
    if (outc) *reinterpret_cast<f4v*>(outc + i) = oc;
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_up2)

// dst = act(conv3x3(pad 1)(bilinear 2x up-sampling of src) + bias): F.interpolate(scale 2, align_corners=False) + ConvBnReLU of the
// decoder (model/spherical_model.py:279-301) in one kernel (conv3x3_halo_sh_kernel<.., UP2>).  src SH [M, Hl, Wl, C], dst [M, 2Hl, 2Wl, Cout]
// SH (fmt bit 0) or fp32; needs 2Wl % 32 == 0, 2Hl % 4 == 0 (OMNI_ERR_UNSUPPORTED otherwise: run omni_upsample_bilinear_sh +
// omni_conv2d_sh_f16x3_ws, which give the same bits).
extern "C" int omni_conv3x3_up2_sh_f16x3(const void* src, const void* wt16, const float* bias, void* dst, int fmt,
                                         int M, int Hl, int Wl, int C, int Cout, int act, omni_stream_t stream)
{
    if (!src || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_sh: null pointer");
    if (M <= 0 || Hl <= 0 || Wl <= 0 || C <= 0 || C % 32 || Cout <= 0 || Cout % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_sh: bad shape (channels must be multiples of 32)");
    const int H = 2 * Hl, W = 2 * Wl;
    if (W % HT_W || H % 4) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_up2_sh: the output must be a multiple of 4 rows x 32 columns");
    if ((long long)M * H * W >= (1ll << 31) || (long long)Cout * 9 * C * 4 >= (1ll << 31))
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_up2_sh: tensor too large for 32-bit indices");
    ShConvArgs a;
    a.src1 = src; a.src2 = nullptr; a.wt = wt16; a.bias = bias; a.res = nullptr; a.dst = dst; a.dst_sh = fmt & 1; a.res_f32 = 0;
    a.dbg = 0; a.noxcd = omni_options().conv_noxcd; a.wt_major = 0; a.epi_lds = omni_options().conv_epi_lds && !(fmt & 4);   // (fmt bit 2, one panorama: the extra barrier and LDS round trip cost more than the wider stores save)
#ifdef OMNI_DEBUG_BUILD
    a.dbg = omni_debug_bits("OMNI_CONV_DBG");
#endif
    a.M = M; a.H = H; a.W = W; a.C1 = C; a.C2 = 0; a.Cout = Cout; a.KH = 3; a.KW = 3; a.stride = 1; a.pad = 1; a.act = act;
    a.Ho = H; a.Wo = W; a.rows = M * H * W; a.splitk = 1; a.ws = nullptr; a.post = nullptr; a.post_rows = 1; a.wino_th = a.wino_tw = a.wino_pix = 0;
    const int grid = M * (H / 4) * (W / HT_W);
    const bool x1 = (fmt & 8) != 0;                                   // f16x1
    if (C == 32 && Cout == 32 && omni_options().conv_up2_persist) {    // de_conv4_0: resident weights, one persistent block of 8 waves per CU
        const dim3 g1(grid < 256 ? (grid + 7) / 8 * 8 : 256);
        if (x1) hipLaunchKernelGGL((conv3x3_up2_g1_kernel<false, true>), g1, dim3(512), 0, (hipStream_t)stream, a, grid, HeadsArgs{nullptr, nullptr});
        else    hipLaunchKernelGGL(conv3x3_up2_g1_kernel<false>, g1, dim3(512), 0, (hipStream_t)stream, a, grid, HeadsArgs{nullptr, nullptr});
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    // (the up-sampling halo is COMPUTED per block — ~700 vector instructions per 2 x 2 cell: blocks of 32 output channels would do it twice — 64 per block here whatever conv_halo_bn says:
    //  de_conv2_0 51 -> 64 us, de_conv3_0 180 -> 240 us with 32, profiles/r06e_halo_bn.txt)
    const bool bn64 = Cout % 64 == 0 && !((fmt & 4) && omni_options().conv_halo_up2_bn_lat == 32);
    const int bn = bn64 ? 64 : 32;
    if (const int rc = omni_halo_launch(&a, bn, 4, true, 0, x1, grid * (Cout / bn), (hipStream_t)stream); rc != OMNI_OK) return rc;
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// de_conv4_0 + the two heads (model/spherical_model.py:300-307): a = relu(pred(y)) (* sigmoid(weight_pred(y)) when confidence), c = sigmoid(weight_pred(y)),
// y = relu(conv3x3(up2(src)) + bias) with 32 -> 32 channels — y never exists (conv3x3_up2_g1_kernel<HEADS> + heads_finish_kernel, see there).
// src SH [M, P/2, P/2, 32]; wt16 / bias: de_conv4_0's; heads_w16f: 4 KB, the heads' [2][9][32] weights in the fragment order of omni_heads_pack_f16x3;
// scratch: omni_up2_heads_scratch_bytes(M, P) bytes; out_a / out_c planar [M, P, P] (out_c may be NULL).  P % 32 == 0.
// Equal to omni_conv3x3_up2_sh_f16x3 (fp32 output) + omni_heads_f32 up to fp32 summation order (the heads' products run f16x3: ~1e-6 relative).
extern "C" size_t omni_up2_heads_scratch_bytes(int M, int P)
{
    if (M <= 0 || P <= 0 || P % 32) return 0;
    return (size_t)M * (P / 4) * (P / 32) * 4 * 6 * HR_PITCH * sizeof(float);
}
template <bool X1>
static int up2_heads_impl(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float bias_pred, float bias_weight,
                          float* scratch, size_t scratch_bytes, float* out_a, float* out_c, int M, int P, int confidence, omni_stream_t stream)
{
    if (!src || !wt16 || !heads_w16f || !scratch || !out_a) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_heads_sh: null pointer");
    if (M <= 0 || P <= 0 || P % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_heads_sh: the patch size must be a multiple of 32");
    if (scratch_bytes < omni_up2_heads_scratch_bytes(M, P)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv3x3_up2_heads_sh: scratch too small (omni_up2_heads_scratch_bytes)");
    if ((long long)M * P * P >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv3x3_up2_heads_sh: tensor too large for 32-bit indices");
    ShConvArgs a;
    a.src1 = src; a.src2 = nullptr; a.wt = wt16; a.bias = bias; a.res = nullptr; a.dst = nullptr; a.dst_sh = 0; a.res_f32 = 0;
    a.dbg = 0; a.noxcd = omni_options().conv_noxcd; a.wt_major = 0; a.epi_lds = 0;
    a.M = M; a.H = P; a.W = P; a.C1 = 32; a.C2 = 0; a.Cout = 32; a.KH = 3; a.KW = 3; a.stride = 1; a.pad = 1; a.act = OMNI_ACT_RELU;
    a.Ho = P; a.Wo = P; a.rows = M * P * P; a.splitk = 1; a.ws = nullptr; a.post = nullptr; a.post_rows = 1; a.wino_th = a.wino_tw = a.wino_pix = 0;
    const int grid = M * (P / 4) * (P / HT_W);
    // f16x3 at P == 128 with conv_up2_heads_taps: the tap products on the 64 x 64 map (omni_conv_up2_heads_taps.hip; a band needs the full low-resolution width of 64)
    const bool taps = !X1 && P == 128 && omni_options().conv_up2_heads_taps == 1 &&
                      !((uintptr_t)src % 16 || (uintptr_t)wt16 % 16 || (uintptr_t)bias % 16 || (uintptr_t)heads_w16f % 16 || (uintptr_t)scratch % 16);
    if (taps) {
        if (const int rc = omni_up2_heads_taps_launch(src, wt16, bias, heads_w16f, scratch, M, (hipStream_t)stream); rc != OMNI_OK) return rc;
    } else {
        hipLaunchKernelGGL((conv3x3_up2_g1_kernel<true, X1>), dim3(grid < 256 ? (grid + 7) / 8 * 8 : 256), dim3(64 * (4 + OMNI_G1_PW)), 0, (hipStream_t)stream, a, grid, HeadsArgs{heads_w16f, scratch});
        OMNI_HIP(hipGetLastError());
    }
    const size_t n = (size_t)M * P * P / 4;
    hipLaunchKernelGGL(heads_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, bias_pred, bias_weight,
                       out_a, out_c, M, P, confidence);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
extern "C" int omni_conv3x3_up2_heads_sh_f16x3(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float bias_pred, float bias_weight,
                                               float* scratch, size_t scratch_bytes, float* out_a, float* out_c, int M, int P, int confidence, omni_stream_t stream)
{
    return up2_heads_impl<false>(src, wt16, bias, heads_w16f, bias_pred, bias_weight, scratch, scratch_bytes, out_a, out_c, M, P, confidence, stream);
}
// the same with de_conv4_0 in f16x1 (one matrix instruction per product block); the heads' own products stay f16x3
extern "C" int omni_conv3x3_up2_heads_sh_f16x1(const void* src, const void* wt16, const float* bias, const void* heads_w16f, float bias_pred, float bias_weight,
                                               float* scratch, size_t scratch_bytes, float* out_a, float* out_c, int M, int P, int confidence, omni_stream_t stream)
{
    return up2_heads_impl<true>(src, wt16, bias, heads_w16f, bias_pred, bias_weight, scratch, scratch_bytes, out_a, out_c, M, P, confidence, stream);
}

// The heads' weights w [2 heads][9 taps][32 channels] (fp32, host or device memory readable by the host — 2.3 KB, packed once per checkpoint) in the
// fragment order of conv3x3_up2_g1_kernel<HEADS>: dst 4 x 64 x 8 halfs = [hi kc0 | hi kc1 | lo kc0 | lo kc1][lane = row + 32 kgroup][8], row r of the
// matrix product = (register group g = r >> 3, lane half hh = (r >> 2) & 1, dx = (r & 3) - 1): (dy, head) pair g + 3 hh; element e of k chunk kc, k group h
// = channel 16 kc + 8 (e >> 2) + 4 h + (e & 3) (the order in which a lane's accumulator quads hold the convolution's output channels).
extern "C" int omni_heads_pack_f16x3(const float* w_host, void* dst_host)
{
    if (!w_host || !dst_host) OMNI_FAIL(OMNI_ERR_INVALID, "omni_heads_pack: null pointer");
    _Float16* o = (_Float16*)dst_host;
    for (int kc = 0; kc < 2; ++kc)
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
                const int r = lane & 31, h = lane >> 5, g = r >> 3, hh = (r >> 2) & 1, dxi = r & 3;
                float w = 0.0f;
                if (g < 3 && dxi < 3) {
                    const int pair = g + 3 * hh, dy = pair / 2, head = pair % 2, ch = 16 * kc + 8 * (e >> 2) + 4 * h + (e & 3);
                    w = w_host[(head * 9 + dy * 3 + dxi) * 32 + ch];
                }
                const _Float16 hi = (w < 6.103515625e-05f && w > -6.103515625e-05f) ? (_Float16)0.0f : (_Float16)w;
                o[(kc * 64 + lane) * 8 + e] = hi;
                o[((2 + kc) * 64 + lane) * 8 + e] = (_Float16)((w - (float)hi) * 2048.0f);
            }
    return OMNI_OK;
}
