// omni_conv_bwd.hip — the backward of the implicit-GEMM convolution of omni_conv.hip on the fp16 matrix cores (gfx950), DESIGN.md §19.
//
// Forward (omni_conv2d_nhwc_f16x3_ws):  out = act(Z),  Z = conv(src1 ++ src2, wt) + bias + res,  act = none | ReLU.
// Backward, three calls on one stream:
//   1. gradient epilogue   dZ = grad_out . [out > 0];  grad_bias[j] = sum_r dZ[r][j];  the residual's gradient is dZ itself;
//                          scale = the power of two that brings max|dZ| into [2^8, 2^9)  (written to DEVICE memory, nothing is read back)
//   2. data gradient       dX[m,y,x,ci] = sum_{ky,kx,co} dZ[m,(y+p-ky)/s,(x+p-kx)/s,co] . wt[co][(ky,kx,ci)]      (conv_dgrad_kernel)
//   3. weight gradient     dW[co][(ky,kx,ci)] = sum_r dZ[r][co] . A[r][(ky,kx,ci)],  A = the forward's implicit im2col  (conv_wgrad_kernel)
//
// Products are the forward's f16x3: every operand x = hi + lo 2^-11 (hi = fp16(x), 0 below 2^-14; lo = fp16((x - hi) 2^11)) and a product
// block is three v_mfma_f32_32x32x16_f16 with fp32 accumulation, hi.hi + 2^-11 (hi.lo + lo.hi).  That format holds values of order 1; a
// gradient of a loss averaged over 5e5 pixels is of order 1e-6, where hi is 0 and lo keeps 11 bits or fewer.  So dZ is multiplied by `scale`
// BEFORE it is split (in the loaders of both kernels) and the accumulator by 1 / scale in the epilogue: both are powers of two, so the scaling
// itself is exact and grad_out . 2^n gives every gradient . 2^n bit for bit.
//
// Determinism: no floating-point atomics.  The bias sums are two fixed-order stages (8 x 8 rows per block, then the column finish of
// omni_partials.h over the blocks); wgrad cuts the rows into chunks of `conv_wgrad_rows` rows (option; 0 = the library's plan), every chunk writes raw partial sums
// and a second pass adds them in chunk order: a result is a function of the inputs and the chunk length only.
//
// f16x1 (X1 = true): an operand is hi alone, a product block ONE matrix instruction; no lo images in LDS, no acc1, no
// fmaf(acc1, 2^-11, acc) in the epilogue.  Same loaders, same gathers, same chunks, same epilogue pass and scale; the weight operand of
// dgrad is the hi-only transposed image.  An element of dZ below 2^-22 max|dZ| (2^-14 after the scale) is 0 there.
//
// A tap that does not apply (outside the image; at stride 2 the wrong parity) is never read: its lanes get an out-of-range buffer offset,
// for which the buffer unit returns zeros — a NaN in dZ reaches exactly the elements whose sum contains it.
#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));

// raw buffer descriptor (V#) over [p, p+bytes): stride 0, num_records = bytes; gfx9-family flags dword
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0,
                                             (int)(unsigned)(bytes > 0xffffffffull ? 0xffffffffull : bytes), 0x00020000);
}
constexpr int OOR = (int)0x80000000;         // a byte offset past every descriptor: the load returns zeros

constexpr int BK = 32;
constexpr int HP = BK + 8;                   // LDS row pitch in halfs: 80 B, conflict-free ds_read_b128

// the forward's operand split (conv_igemm_f32_kernel<.., F16X3 = true>::stash)
__device__ __forceinline__ void split1(const float x, _Float16& hi, _Float16& lo)
{
    const _Float16 h = (fabsf(x) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)x;
    hi = h; lo = (_Float16)((x - (float)h) * 2048.0f);
}
__device__ __forceinline__ void split4(const f4v x, h4v& hi, h4v& lo)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) { _Float16 h, l; split1(x[e], h, l); hi[e] = h; lo[e] = l; }
}
// f16x1: the hi of the split alone
__device__ __forceinline__ h4v hi4(const f4v x)
{
    h4v hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) hi[e] = (fabsf(x[e]) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)x[e];
    return hi;
}

// ------------------------------------------------------------------ gradient epilogue
// Stage 1: a block owns EPI_ROWS rows and all channels; thread (row lane t >> 5, channel t & 31) adds its 8 rows in order, the 8 row lanes are
// added as ((0+1)+(2+3)) + ((4+5)+(6+7)).  part[block][Cout]: the block's channel sums; pmax[block]: max |dZ| as the bit pattern of the
// magnitude (an integer maximum: a NaN is larger than inf is larger than every finite value, so a non-finite element is SEEN).
constexpr int EPI_ROWS = 64;

__global__ __launch_bounds__(256) void conv_bwd_epilogue_kernel(const float* __restrict__ grad_out, const float* __restrict__ out,
                                                                float* __restrict__ dz, float* __restrict__ part, int* __restrict__ pmax,
                                                                int rows, int Cout, int relu)
{
    __shared__ float red[8][32];
    __shared__ int mred[4];
    const int t = threadIdx.x, cl = t & 31, rl = t >> 5;
    const int r0 = blockIdx.x * EPI_ROWS;
    int mx = 0;
    for (int g = 0; g < Cout; g += 32) {
        float s = 0.0f;
        for (int i = 0; i < EPI_ROWS / 8; ++i) {
            const int r = r0 + rl + 8 * i;
            if (r < rows) {
                const size_t o = (size_t)r * Cout + g + cl;
                float v = grad_out[o];
                if (relu) v = out[o] > 0.0f ? v : 0.0f;          // a select, not a product: a NaN behind an inactive ReLU stops here
                if (dz) dz[o] = v;
                s += v;
                mx = max(mx, (int)(__float_as_uint(v) & 0x7fffffffu));
            }
        }
        red[rl][cl] = s;
        __syncthreads();
        if (rl == 0)
            part[(size_t)blockIdx.x * Cout + g + cl] = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) +
                                                       ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
        __syncthreads();
    }
    mx = wave_max(mx);
    if ((t & 63) == 0) mred[t >> 6] = mx;
    __syncthreads();
    if (t == 0) pmax[blockIdx.x] = max(max(mred[0], mred[1]), max(mred[2], mred[3]));
}

// Stage 2: block j < Cout adds channel j's partial sums over the blocks (the column finish, N = 1 over float partials), in double, rounded
// once; block Cout takes the maximum and writes scale[0] = 2^s, scale[1] = 2^-s with s = 8 - floor(log2 max|dZ|) clamped to
// [-126, 126] (both stay normal numbers).  max = 0 or not finite: s = 0.
__global__ __launch_bounds__(256) void conv_bwd_epilogue_finish_kernel(const float* __restrict__ part, const int* __restrict__ pmax, int nblk,
                                                                       int Cout, float* __restrict__ grad_bias, float* __restrict__ scale)
{
    __shared__ double red[1][4];
    __shared__ int mred[4];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < Cout) {
        double v[1];
        column_sums<1>(part + blockIdx.x, nblk, Cout, 0, v, red);
        if (t == 0) grad_bias[blockIdx.x] = (float)v[0];
    } else {
        int mx = 0;
        for (int b = t; b < nblk; b += 256) mx = max(mx, pmax[b]);
        mx = block_reduce(mx, true, mred);
        if (t == 0) {
            const int e = mx >> 23;                              // biased exponent of the largest magnitude
            int s = 0;
            if (mx != 0 && e != 255) { s = 135 - e; s = s > 126 ? 126 : (s < -126 ? -126 : s); }
            scale[0] = __uint_as_float((unsigned)(127 + s) << 23);
            scale[1] = __uint_as_float((unsigned)(127 - s) << 23);
        }
    }
}

// ------------------------------------------------------------------ weights: split into halfs, optionally transposed
// transpose = 0: w [R = Cout][K = taps * Cin]  ->  halfs [Cout][K/32][hi32|lo32]           (the forward's operand)
// transpose = 1: w [Cout][(tap, ci)]           ->  halfs [Cin][taps * Cout/32][hi32|lo32], k = (tap, co)   (dgrad's operand: taps NOT flipped,
//                the dgrad loader walks the source pixel instead)
// X1: the hi-only image, halfs [row][kd] with the same row and k order (f16x1)
template <bool X1>
__global__ __launch_bounds__(256) void conv_wsplit_kernel(const float* __restrict__ w, _Float16* __restrict__ out, int Cout, int taps, int Cin,
                                                          int transpose)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)Cout * taps * Cin;
    if (i >= total) return;
    size_t src = i, row, kk, kd;
    if (!transpose) { kd = (size_t)taps * Cin; row = i / kd; kk = i - row * kd; }
    else {
        kd = (size_t)taps * Cout; row = i / kd; kk = i - row * kd;               // row = ci, kk = tap * Cout + co
        const size_t tap = kk / Cout, co = kk - tap * Cout;
        src = (co * taps + tap) * Cin + row;
    }
    _Float16 h, l;
    split1(w[src], h, l);
    if (X1) { out[row * kd + kk] = h; return; }
    const size_t d = (row * (kd >> 5) + (kk >> 5)) * 64 + (kk & 31);
    out[d] = h; out[d + 32] = l;
}

// ------------------------------------------------------------------ data gradient
// GEMM view: D[r][ci] = sum_k Z[r][k] Wt[ci][k], r = INPUT pixel (m, y, x), k = (tap, output channel).  Z is gathered: tap (ky, kx) of pixel
// (y, x) is dZ at ((y+p-ky)/s, (x+p-kx)/s) where both divisions are exact and the result lies inside the Ho x Wo map.  The tile loop, the LDS
// images and the fragment reads are those of the forward's f16x3 kernel; column tiles below C1 go to dx1, the others to dx2.  Every element of
// both is stored: a pixel no tap reaches (three in four at stride 2 with a 1x1 kernel) is a sum of zeros.
struct DgradArgs {
    const float* dz; const void* wt16; const float* scale; float* dx1; float* dx2;
    int M, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, pad;
    int rows;                                // M*H*W
};

template <int BM, int BN, int WM, int WN, bool X1>
__global__ __launch_bounds__(256, (X1 ? 4 : 2)) void conv_dgrad_kernel(DgradArgs a)
{
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int APASS = BM / 32, BPASS = BN / 32;
    __shared__ __attribute__((aligned(16))) _Float16 lds[(X1 ? 1 : 2) * (BM + BN) * HP];
    _Float16* Ah = lds;
    _Float16* Al = Ah + (X1 ? 0 : BM * HP);                      // (X1: no lo images; Al and Bl are never touched)
    _Float16* Bh = Al + BM * HP;
    _Float16* Bl = Bh + (X1 ? 0 : BN * HP);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int Cin = a.C1 + a.C2;
    const int ntn = Cin / BN;
    const int tile_m = blockIdx.x / ntn, tile_n = blockIdx.x % ntn;
    const int row0 = tile_m * BM, col0 = tile_n * BN;
    const bool to1 = col0 < a.C1;
    float* const dx = to1 ? a.dx1 : a.dx2;
    if (!dx) return;                                             // (block-uniform) this input needs no gradient
    const int cchunks = a.Cout / BK;
    const int ksteps = a.KH * a.KW * cchunks;
    const int sh = a.stride - 1;                                 // stride 1 | 2
    const float sc = a.scale[0], isc = a.scale[1];

    const int lr = t >> 3, kq = (t & 7) * 4;
    int zbase[APASS], yy[APASS], xx[APASS];                      // m*Ho*Wo (or -1: row past the end), y + pad, x + pad
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
        const int r = row0 + lr + 32 * i;
        zbase[i] = -1; yy[i] = 0; xx[i] = 0;
        if (r < a.rows) {
            const int hw = a.H * a.W;
            const int m = r / hw, rem = r - m * hw;
            const int y = rem / a.W;
            zbase[i] = m * a.Ho * a.Wo; yy[i] = y + a.pad; xx[i] = rem - y * a.W + a.pad;
        }
    }
    const rsrc_t rsz = make_rsrc(a.dz, (size_t)a.M * a.Ho * a.Wo * a.Cout * 4);
    const rsrc_t rsw = make_rsrc(a.wt16, (size_t)Cin * ksteps * (X1 ? 64 : 128));
    // f16x3: a 32-k piece of a row is 128 B (hi32 | lo32), eight 16-byte loads; X1: 64 B, the loads of lanes t&7 >= 4 are out of range
    int wbase[BPASS];
#pragma unroll
    for (int i = 0; i < BPASS; ++i)
        wbase[i] = X1 ? ((t & 7) < 4 ? ((col0 + lr + 32 * i) * ksteps * 32 + (t & 3) * 8) * 2 : OOR)
                      : ((col0 + lr + 32 * i) * ksteps * 64 + (t & 7) * 8) * 2;

    f4v ra[APASS], rb[BPASS];
    int f_c = 0, f_ky = 0, f_kx = 0;                             // (tap, channel chunk) of the NEXT fetch
    auto fetch = [&](int ks) {
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            const int ty = yy[i] - f_ky, tx = xx[i] - f_kx;
            const int sy = ty >> sh, sx = tx >> sh;
            const bool ok = zbase[i] >= 0 && ty >= 0 && tx >= 0 && ((ty | tx) & sh) == 0 && sy < a.Ho && sx < a.Wo;
            const int off = ok ? ((zbase[i] + sy * a.Wo + sx) * a.Cout + f_c + kq) * 4 : OOR;
            ra[i] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsz, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < BPASS; ++i)
            rb[i] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsw, wbase[i], ks * (X1 ? BK * 2 : BK * 4), 0));
        f_c += BK;
        if (f_c == a.Cout) { f_c = 0; if (++f_kx == a.KW) { f_kx = 0; ++f_ky; } }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < APASS; ++i) {
            if (X1) { *reinterpret_cast<h4v*>(Ah + (lr + 32 * i) * HP + kq) = hi4(ra[i] * sc); continue; }
            h4v hi, lo;
            split4(ra[i] * sc, hi, lo);                          // the scaled split
            *reinterpret_cast<h4v*>(Ah + (lr + 32 * i) * HP + kq) = hi;
            *reinterpret_cast<h4v*>(Al + (lr + 32 * i) * HP + kq) = lo;
        }
        if (X1 && (t & 7) >= 4) return;
        _Float16* bd = ((t & 7) >= 4 ? Bl : Bh) + lr * HP + (t & 3) * 8;
#pragma unroll
        for (int i = 0; i < BPASS; ++i) *reinterpret_cast<f4v*>(bd + 32 * i * HP) = rb[i];
    };

    f16v acc[TM][TN], acc1[X1 ? 1 : TM][X1 ? 1 : TN];            // acc = hi.hi, acc1 = hi.lo + lo.hi (scaled by 2^11)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) { acc[i][j] = (f16v)(0.0f); if (!X1) acc1[i][j] = (f16v)(0.0f); }

    fetch(0);
    for (int ks = 0; ks < ksteps; ++ks) {
        __syncthreads();                     // previous step's fragment reads are done
        stash();
        __syncthreads();
        if (ks + 1 < ksteps) fetch(ks + 1);
        const int foff = (lane & 31) * HP + (lane >> 5) * 8;     // fragment: row lane&31, k = 8*(lane>>5) .. +7 of a 16-wide chunk
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            h8v ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = *reinterpret_cast<const h8v*>(Ah + ((wm * TM + i) * 32) * HP + foff + kc * 16);
                if (!X1) al[i] = *reinterpret_cast<const h8v*>(Al + ((wm * TM + i) * 32) * HP + foff + kc * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[j] = *reinterpret_cast<const h8v*>(Bh + ((wn * TN + j) * 32) * HP + foff + kc * 16);
                if (!X1) bl[j] = *reinterpret_cast<const h8v*>(Bl + ((wn * TN + j) * 32) * HP + foff + kc * 16);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    if (X1) continue;
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc1[i][j], 0, 0, 0);
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc1[i][j], 0, 0, 0);
                }
        }
    }

    // ---- epilogue: D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); undo the scale (exact)
    const int cs = to1 ? a.C1 : a.C2, cb = to1 ? col0 : col0 - a.C1;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = cb + (wn * TN + j) * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = row0 + (wm * TM + i) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (r < a.rows) dx[(size_t)r * cs + col] = (X1 ? acc[i][j][reg] : fmaf(acc1[i][j][reg], 4.8828125e-4f, acc[i][j][reg])) * isc;
            }
        }
    }
}

// ------------------------------------------------------------------ weight gradient
// GEMM view: D[co][k] = sum_r Z[r][co] A[r][k], k = (tap, input channel): the sum runs over ROWS, so an MFMA fragment is eight consecutive
// rows of one channel.  Both operands lie row-major with the channels contiguous; the loader therefore writes its split halfs into LDS
// TRANSPOSED — images [channel][32 rows] of pitch HP — and the fragment reads are the forward's plain 16-byte reads (see DESIGN.md §19 for why
// not ds_read_b64_tr_b16).  A block owns 64 output channels x 64 k (two 32-channel pieces of the im2col row, fixed for the block) and the rows
// [blockIdx.y * chunk, + chunk); wave (w >> 1, w & 1) owns one 32 x 32 tile.  Pieces past Cout or past K load zeros (out-of-range offsets)
// and are not stored: no lane is ever masked around a matrix instruction.  ws[chunk][Cout][K]: raw partial sums, still scaled.
struct WgradArgs {
    const float* dz; const float* src1; const float* src2; const float* scale; float* ws;
    int M, H, W, C1, C2, Ho, Wo, Cout, KH, KW, stride, pad;
    int rows;                                // M*Ho*Wo
    int chunk;                               // rows per blockIdx.y, a multiple of 32
};

template <bool X1>
__global__ __launch_bounds__(256, (X1 ? 4 : 2)) void conv_wgrad_kernel(WgradArgs a)
{
    __shared__ __attribute__((aligned(16))) _Float16 lds[(X1 ? 2 : 4) * 64 * HP];
    _Float16* Zh = lds;
    _Float16* Zl = Zh + (X1 ? 0 : 64 * HP);                      // (X1: no lo images; Zl and Al are never touched)
    _Float16* Ah = Zl + 64 * HP;
    _Float16* Al = Ah + (X1 ? 0 : 64 * HP);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Cin = a.C1 + a.C2;
    const int cchunks = Cin / BK, nk32 = a.KH * a.KW * cchunks;
    const int nkt = (nk32 + 1) >> 1;
    const int tile_co = blockIdx.x / nkt, tile_k = blockIdx.x % nkt;
    const int co0 = tile_co * 64, kc0 = tile_k * 2;
    const int Kfull = nk32 * BK;
    const float sc = a.scale[0];

    const int lr = t >> 3, kq = (t & 7) * 4;
    // the block's two im2col pieces: tap (ky, kx), source, channel offset
    int p_ky[2], p_kx[2], p_c[2], p_cs[2]; bool p_ok[2], p_first[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int kc = kc0 + i;
        p_ok[i] = kc < nk32;
        const int tap = kc / cchunks, c = (kc - tap * cchunks) * BK;
        p_ky[i] = tap / a.KW; p_kx[i] = tap - p_ky[i] * a.KW;
        p_first[i] = c < a.C1; p_cs[i] = p_first[i] ? a.C1 : a.C2; p_c[i] = (p_first[i] ? c : c - a.C1) + kq;
    }
    const rsrc_t rsz = make_rsrc(a.dz, (size_t)a.rows * a.Cout * 4);
    const rsrc_t rs1 = make_rsrc(a.src1, (size_t)a.M * a.H * a.W * a.C1 * 4);
    const rsrc_t rs2 = make_rsrc(a.src2 ? a.src2 : a.src1, a.src2 ? (size_t)a.M * a.H * a.W * a.C2 * 4 : 0);

    const int rbegin = blockIdx.y * a.chunk, rend = min(a.rows, rbegin + a.chunk);
    const int steps = (rend - rbegin + 31) >> 5;
    const int hw = a.Ho * a.Wo;

    f4v rz[2], ra[2];
    auto fetch = [&](int st) {
        const int r = rbegin + st * 32 + lr;
        const bool rok = r < rend;
        const int m = r / hw, rem = r - m * hw;
        const int q = rem / a.Wo;
        const int oy = q * a.stride - a.pad, ox = (rem - q * a.Wo) * a.stride - a.pad;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int co = co0 + 32 * i + kq;
            const int off = (rok && co < a.Cout) ? (r * a.Cout + co) * 4 : OOR;
            rz[i] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsz, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = oy + p_ky[i], ix = ox + p_kx[i];
            const bool ok = rok && p_ok[i] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const int off = ok ? (((m * a.H + iy) * a.W + ix) * p_cs[i] + p_c[i]) * 4 : OOR;
            ra[i] = p_first[i] ? __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rs1, off, 0, 0))
                               : __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rs2, off, 0, 0));
        }
    };
    auto stash = [&]() {                                         // transposed: channel 32 i + kq + e is an LDS row, the tile's row lr a column
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            h4v zh, zl, ah, al;
            if (X1) { zh = hi4(rz[i] * sc); ah = hi4(ra[i]); }
            else {
                split4(rz[i] * sc, zh, zl);                      // the scaled split
                split4(ra[i], ah, al);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = (32 * i + kq + e) * HP + lr;
                Zh[o] = zh[e];
                if (!X1) Zl[o] = zl[e];
                Ah[o] = ah[e];
                if (!X1) Al[o] = al[e];
            }
        }
    };

    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
    if (steps > 0) fetch(0);
    for (int st = 0; st < steps; ++st) {
        __syncthreads();                     // previous step's fragment reads are done
        stash();
        __syncthreads();
        if (st + 1 < steps) fetch(st + 1);
        const int zo = (wm * 32 + (lane & 31)) * HP + (lane >> 5) * 8;      // fragment: channel lane&31, rows 8*(lane>>5) .. +7 of a 16-row chunk
        const int ao = (wn * 32 + (lane & 31)) * HP + (lane >> 5) * 8;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            h8v zl, al;
            const h8v zh = *reinterpret_cast<const h8v*>(Zh + zo + kc * 16);
            if (!X1) zl = *reinterpret_cast<const h8v*>(Zl + zo + kc * 16);
            const h8v ah = *reinterpret_cast<const h8v*>(Ah + ao + kc * 16);
            if (!X1) al = *reinterpret_cast<const h8v*>(Al + ao + kc * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(zh, ah, acc, 0, 0, 0);
            if (X1) continue;
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(zh, al, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(zl, ah, acc1, 0, 0, 0);
        }
    }

    // D layout: col (k) = lane&31, row (co) = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    if (kc0 + wn < nk32) {
        const int k = (kc0 + wn) * BK + (lane & 31);
        float* const w = a.ws + (size_t)blockIdx.y * a.Cout * Kfull;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int co = co0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (co < a.Cout) w[(size_t)co * Kfull + k] = X1 ? acc[reg] : fmaf(acc1[reg], 4.8828125e-4f, acc[reg]);
        }
    }
}

// dW = (sum_c ws[c]) / scale, chunks added in index order (4 elements per thread)
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ scale,
                                                                float* __restrict__ dw, size_t n4, int nchunks, size_t slab)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const size_t o = i * 4;
    f4v v = *reinterpret_cast<const f4v*>(ws + o);
    for (int c = 1; c < nchunks; ++c) v += *reinterpret_cast<const f4v*>(ws + (size_t)c * slab + o);
    *reinterpret_cast<f4v*>(dw + o) = v * scale[1];
}

// ------------------------------------------------------------------ host side
struct BwdShape { int Ho, Wo; long long rows_out, rows_in, K; };

// the shapes the backward covers: the forward's, narrowed to square 1x1 / 3x3 kernels and strides 1 / 2
int bwd_shape(int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, BwdShape& s, const char*& why)
{
    if (C1 <= 0 || C1 % BK || C2 < 0 || C2 % BK || Cout <= 0 || Cout % 32) { why = "channels must be multiples of 32"; return OMNI_ERR_INVALID; }
    if (M <= 0 || H <= 0 || W <= 0 || pad < 0) { why = "bad shape"; return OMNI_ERR_INVALID; }
    if (KH != KW || (KH != 1 && KH != 3)) { why = "kernels are 1x1 or 3x3"; return OMNI_ERR_UNSUPPORTED; }
    if (stride != 1 && stride != 2) { why = "stride is 1 or 2"; return OMNI_ERR_UNSUPPORTED; }
    if (H + 2 * pad < KH || W + 2 * pad < KW) { why = "kernel larger than the padded image"; return OMNI_ERR_INVALID; }
    s.Ho = (H + 2 * pad - KH) / stride + 1; s.Wo = (W + 2 * pad - KW) / stride + 1;
    s.rows_out = (long long)M * s.Ho * s.Wo; s.rows_in = (long long)M * H * W; s.K = (long long)KH * KW * (C1 + C2);
    const long long lim = 1ll << 31;
    if (s.rows_out >= lim || s.rows_in >= lim) { why = "too many pixels for 32-bit row indices"; return OMNI_ERR_UNSUPPORTED; }
    if (s.rows_in * (C1 > C2 ? C1 : C2) * 4 >= lim || s.rows_out * Cout * 4 >= lim || (long long)Cout * s.K * 4 >= lim) {
        why = "an operand of 2 GiB or more (32-bit buffer offsets)"; return OMNI_ERR_UNSUPPORTED;
    }
    return OMNI_OK;
}

// rows per wgrad chunk: the option, or about 1024 blocks over the launch with at least 256 rows per chunk and at most 256 chunks
int plan_wgrad_rows(long long rows, int Cout, long long K)
{
    const int opt = omni_options().conv_wgrad_rows;
    if (opt > 0) return (opt + 31) / 32 * 32;
    const long long tiles = ((Cout + 63) / 64) * ((K / 32 + 1) / 2);
    long long n = 1024 / tiles;
    n = n < 1 ? 1 : (n > 256 ? 256 : n);
    long long chunk = (rows + n - 1) / n;
    if (chunk < 256) chunk = 256;
    return (int)((chunk + 31) / 32 * 32);
}

size_t epilogue_ws_bytes(long long rows, int Cout) { return (size_t)((rows + EPI_ROWS - 1) / EPI_ROWS) * (Cout + 1) * 4; }
size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
}  // namespace

extern "C" size_t omni_conv2d_bwd_workspace_bytes(int M, int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad)
{
    BwdShape s; const char* why = "";
    if (bwd_shape(M, H, W, C1, C2, Cout, KH, KW, stride, pad, s, why) != OMNI_OK) return 0;
    const int chunk = plan_wgrad_rows(s.rows_out, Cout, s.K);
    const size_t nchunks = (size_t)((s.rows_out + chunk - 1) / chunk);
    size_t n = epilogue_ws_bytes(s.rows_out, Cout);
    const size_t nd = (size_t)Cout * s.K * 4, nw = nchunks * Cout * s.K * 4;
    if (nd > n) n = nd;
    if (nw > n) n = nw;
    return align16(n);
}

extern "C" int omni_conv2d_bwd_epilogue_f32(const float* grad_out, const float* out, float* dz, float* grad_bias, float* scale,
                                            long long rows, int Cout, int act, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    if (act == OMNI_ACT_GELU) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_bwd_epilogue: no GELU backward (the forward does not keep the pre-activation)");
    if (act != OMNI_ACT_NONE && act != OMNI_ACT_RELU) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_epilogue: unknown activation");
    if (!grad_out || !grad_bias || !scale || !workspace) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_epilogue: null pointer");
    if (act == OMNI_ACT_RELU && (!out || !dz)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_epilogue: ReLU needs the forward's output and a dZ buffer");
    if (rows <= 0 || Cout <= 0 || Cout % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_epilogue: rows >= 1, channels a multiple of 32");
    if (rows >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_bwd_epilogue: too many pixels for 32-bit row indices");
    if (ws_bytes < epilogue_ws_bytes(rows, Cout)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_epilogue: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (int)((rows + EPI_ROWS - 1) / EPI_ROWS);
    float* part = (float*)workspace;
    int* pmax = (int*)(part + (size_t)nblk * Cout);
    hipLaunchKernelGGL(conv_bwd_epilogue_kernel, dim3(nblk), dim3(256), 0, s, grad_out, out, dz, part, pmax, (int)rows, Cout,
                       act == OMNI_ACT_RELU ? 1 : 0);
    OMNI_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv_bwd_epilogue_finish_kernel, dim3(Cout + 1), dim3(256), 0, s, (const float*)part, (const int*)pmax, nblk, Cout,
                       grad_bias, scale);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

namespace {
template <bool X1>
int split_weights_impl(const float* wt, void* wt16, int Cout, int K, omni_stream_t stream)
{
    if (!wt || !wt16) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_split_weights: null pointer");
    if (Cout <= 0 || K <= 0 || K % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_split_weights: K must be a multiple of 32");
    const size_t total = (size_t)Cout * K;
    if (total * 4 >= (1ull << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_split_weights: an operand of 2 GiB or more");
    hipLaunchKernelGGL(conv_wsplit_kernel<X1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wt, (_Float16*)wt16, Cout, 1,
                       K, 0);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

template <bool X1>
int bwd_data_impl(const float* dz, const float* wt, const float* scale, float* dx1, float* dx2, int M, int H, int W, int C1, int C2, int Cout,
                  int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    BwdShape sh; const char* why = "";
    if (const int rc = bwd_shape(M, H, W, C1, C2, Cout, KH, KW, stride, pad, sh, why); rc != OMNI_OK)
        OMNI_FAIL(rc, std::string("omni_conv2d_bwd_data: ") + why);
    if (!dz || !wt || !scale || !workspace) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_data: null pointer");
    if (!dx1 && !(C2 > 0 && dx2)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_data: no gradient requested");
    if (ws_bytes < (size_t)Cout * sh.K * 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_data: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int Cin = C1 + C2;
    const size_t total = (size_t)Cout * sh.K;
    hipLaunchKernelGGL(conv_wsplit_kernel<X1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wt, (_Float16*)workspace, Cout, KH * KW, Cin, 1);
    OMNI_HIP(hipGetLastError());
    DgradArgs a;
    a.dz = dz; a.wt16 = workspace; a.scale = scale; a.dx1 = dx1; a.dx2 = C2 > 0 ? dx2 : nullptr;
    a.M = M; a.H = H; a.W = W; a.C1 = C1; a.C2 = C2; a.Ho = sh.Ho; a.Wo = sh.Wo; a.Cout = Cout;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.rows = (int)sh.rows_in;
    if (C1 % 64 == 0 && C2 % 64 == 0) {
        const long long grid = ((sh.rows_in + 63) / 64) * (Cin / 64);
        if (grid >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_bwd_data: too many blocks");
        hipLaunchKernelGGL((conv_dgrad_kernel<64, 64, 2, 2, X1>), dim3((unsigned)grid), dim3(256), 0, s, a);
    } else {
        const long long grid = ((sh.rows_in + 127) / 128) * (Cin / 32);
        if (grid >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_bwd_data: too many blocks");
        hipLaunchKernelGGL((conv_dgrad_kernel<128, 32, 4, 1, X1>), dim3((unsigned)grid), dim3(256), 0, s, a);
    }
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

template <bool X1>
int bwd_weight_impl(const float* dz, const float* src1, const float* src2, const float* scale, float* dw, int M, int H, int W, int C1, int C2,
                    int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    BwdShape sh; const char* why = "";
    if (const int rc = bwd_shape(M, H, W, C1, C2, Cout, KH, KW, stride, pad, sh, why); rc != OMNI_OK)
        OMNI_FAIL(rc, std::string("omni_conv2d_bwd_weight: ") + why);
    if (!dz || !src1 || !scale || !dw || !workspace || (C2 > 0 && !src2)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_weight: null pointer");
    const int chunk = plan_wgrad_rows(sh.rows_out, Cout, sh.K);
    const long long nchunks = (sh.rows_out + chunk - 1) / chunk;
    if (nchunks > 65535) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_conv2d_bwd_weight: more than 65535 chunks (raise conv_wgrad_rows)");
    const size_t slab = (size_t)Cout * sh.K;
    if (ws_bytes < (size_t)nchunks * slab * 4) OMNI_FAIL(OMNI_ERR_INVALID, "omni_conv2d_bwd_weight: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    WgradArgs a;
    a.dz = dz; a.src1 = src1; a.src2 = C2 > 0 ? src2 : nullptr; a.scale = scale; a.ws = (float*)workspace;
    a.M = M; a.H = H; a.W = W; a.C1 = C1; a.C2 = C2; a.Ho = sh.Ho; a.Wo = sh.Wo; a.Cout = Cout;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.rows = (int)sh.rows_out; a.chunk = chunk;
    const int tiles = ((Cout + 63) / 64) * (int)((sh.K / 32 + 1) / 2);
    hipLaunchKernelGGL(conv_wgrad_kernel<X1>, dim3(tiles, (unsigned)nchunks), dim3(256), 0, s, a);
    OMNI_HIP(hipGetLastError());
    const size_t n4 = slab / 4;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float*)workspace, scale, dw, n4,
                       (int)nchunks, slab);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
}  // namespace

extern "C" int omni_conv2d_split_weights_f16x3(const float* wt, void* wt16, int Cout, int K, omni_stream_t stream)
{
    return split_weights_impl<false>(wt, wt16, Cout, K, stream);
}

extern "C" int omni_conv2d_split_weights_f16x1(const float* wt, void* wt16, int Cout, int K, omni_stream_t stream)
{
    return split_weights_impl<true>(wt, wt16, Cout, K, stream);
}

extern "C" int omni_conv2d_bwd_data_f16x3(const float* dz, const float* wt, const float* scale, float* dx1, float* dx2, int M, int H, int W,
                                          int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                                          omni_stream_t stream)
{
    return bwd_data_impl<false>(dz, wt, scale, dx1, dx2, M, H, W, C1, C2, Cout, KH, KW, stride, pad, workspace, ws_bytes, stream);
}

extern "C" int omni_conv2d_bwd_data_f16x1(const float* dz, const float* wt, const float* scale, float* dx1, float* dx2, int M, int H, int W,
                                          int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t ws_bytes,
                                          omni_stream_t stream)
{
    return bwd_data_impl<true>(dz, wt, scale, dx1, dx2, M, H, W, C1, C2, Cout, KH, KW, stride, pad, workspace, ws_bytes, stream);
}

extern "C" int omni_conv2d_bwd_weight_f16x3(const float* dz, const float* src1, const float* src2, const float* scale, float* dw, int M,
                                            int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                                            size_t ws_bytes, omni_stream_t stream)
{
    return bwd_weight_impl<false>(dz, src1, src2, scale, dw, M, H, W, C1, C2, Cout, KH, KW, stride, pad, workspace, ws_bytes, stream);
}

extern "C" int omni_conv2d_bwd_weight_f16x1(const float* dz, const float* src1, const float* src2, const float* scale, float* dw, int M,
                                            int H, int W, int C1, int C2, int Cout, int KH, int KW, int stride, int pad, void* workspace,
                                            size_t ws_bytes, omni_stream_t stream)
{
    return bwd_weight_impl<true>(dz, src1, src2, scale, dw, M, H, W, C1, C2, Cout, KH, KW, stride, pad, workspace, ws_bytes, stream);
}
