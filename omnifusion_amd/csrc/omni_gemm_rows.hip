// omni_gemm_rows.hip — the transformer GEMMs of a lone panorama (<= 32 rows): gemm_rows_pack_kernel, gemm_rows_sh_kernel, gemm_rows_ln_sh_kernel and the
// entry points omni_gemm_rows_pack, omni_gemm_rows_sh_f16x3, omni_gemm_rows_ln_sh_f16x3, omni_gemm_rows_slices_sh_f16x3, omni_gemm_rows_ln_parts_sh_f16x3.
#include "omni_conv_sh_common.h"

namespace {

// ------------------------------------------------------------------ GEMM over a handful of rows (a lone panorama's tokens)
// out[rows <= 32, N] = act(x[rows, K] . W[N, K]^T + bias + res): the 24 transformer GEMMs of ONE panorama have 18 rows — one column
// tile of the matrix instruction — and are nothing but a stream of weights (1-4 MB each) behind a launch.  Through the tile kernel
// above they cost 8-19 us each (16-64 barrier-synchronised K-steps through LDS, fc2 a split-K launch plus its reduction); here a block
// owns 32 output channels, its 8 waves split K between them and fetch both operands STRAIGHT INTO REGISTERS in fragment order (no LDS,
// no barrier in the K loop, up to four K-steps = 32 sixteen-byte loads per lane in flight), and the 8 partial tiles meet once in LDS
// in a fixed order.  Within a 32-channel group lane half h takes halfs 16h .. 16h+15 (32 contiguous bytes) for BOTH operands: which k
// meets which inside one matrix instruction is free as long as the two sides agree.
struct RowsGemmArgs {
    const void* x; const void* wt; const float* bias; const float* res; void* dst;
    int rows, K, N, act, dst_sh;
    // K slices (round 6): gemm_rows_sh_kernel with blockIdx.y = slice s writes its RAW partial sums to parts[s][rows][N] (no bias / residual / activation);
    // gemm_rows_ln_sh_kernel with nparts > 0 takes its input as x = sum_s parts[s] + pbias + pres (and block 0 writes it to xout: the next residual)
    float* parts; int nparts; const float* pbias; const float* pres; float* xout;
};

// dst (fragment order, see gemm_rows_sh_kernel) <- src [N][K/32][hi32|lo32]; one 16-byte piece per thread
__global__ __launch_bounds__(256) void gemm_rows_pack_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int ksteps, size_t pieces)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= pieces) return;
    const int lane = i & 63, f = (i >> 6) & 3;
    const size_t bk = i >> 8;
    const int ks = bk % ksteps; const size_t b = bk / ksteps;
    const int r = lane & 31, h = lane >> 5, part = f >> 1, kc = f & 1;
    *reinterpret_cast<f4v*>(dst + i * 16) = *reinterpret_cast<const f4v*>(src + ((b * 32 + r) * ksteps + ks) * 128 + part * 64 + (h * 16 + kc * 8) * 2);
}

template <int KPW>                                               // K-steps per wave (K = 256 * KPW)
__global__ __launch_bounds__(512) void gemm_rows_sh_kernel(RowsGemmArgs a)
{
    constexpr int NWV = 8, DEPTH = KPW < 4 ? KPW : 4, PITCH = 36;
    __shared__ float red[NWV][32][PITCH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int col0 = blockIdx.x * 32, ksteps = a.K >> 5, ks0 = (blockIdx.y * NWV + wave) * KPW;       // (blockIdx.y: the K slice of a sliced launch)
    // weights in FRAGMENT ORDER (omni_gemm_rows_pack): [column tile][K-step][hi kc0, hi kc1, lo kc0, lo kc1][lane] x 16 B — a wave's load is
    // one contiguous KiB (8 cache lines) instead of 32 B out of each of 32 lines 8 KiB apart, which made the address unit the bound
    const unsigned char* wp = (const unsigned char*)a.wt + ((size_t)blockIdx.x * ksteps + ks0) * 4096 + lane * 16;
    const unsigned char* xp = (const unsigned char*)a.x + ((size_t)r * ksteps + ks0) * 128 + h * 32;
    const bool live = r < a.rows;                                // token columns past the end stay zero and are never stored
    h8v wh[DEPTH][2], wl[DEPTH][2], xh[DEPTH][2], xl[DEPTH][2];
    auto fetch = [&](int slot, int i) {
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            wh[slot][kc] = *reinterpret_cast<const h8v*>(wp + i * 4096 + kc * 1024);
            wl[slot][kc] = *reinterpret_cast<const h8v*>(wp + i * 4096 + 2048 + kc * 1024);
            xh[slot][kc] = live ? *reinterpret_cast<const h8v*>(xp + i * 128 + kc * 16) : (h8v)(_Float16)0.0f;
            xl[slot][kc] = live ? *reinterpret_cast<const h8v*>(xp + i * 128 + 64 + kc * 16) : (h8v)(_Float16)0.0f;
        }
    };
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) fetch(i, i);
    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[i % DEPTH][kc], xh[i % DEPTH][kc], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[i % DEPTH][kc], xh[i % DEPTH][kc], acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[i % DEPTH][kc], xl[i % DEPTH][kc], acc1, 0, 0, 0);
        }
        if (i + DEPTH < KPW) fetch(i % DEPTH, i + DEPTH);
    }
    // D = W x tokens: column (lane & 31) = token, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = channel
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f4v v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(acc1[4 * q + e], 4.8828125e-4f, acc[4 * q + e]);
        *reinterpret_cast<f4v*>(&red[wave][r][8 * q + 4 * h]) = v;
    }
    __syncthreads();
    const int tok = t >> 3, c4 = (t & 7) * 4;
    if (t >= 256 || tok >= a.rows) return;
    f4v v = *reinterpret_cast<const f4v*>(&red[0][tok][c4]);
#pragma unroll
    for (int w = 1; w < NWV; ++w) v += *reinterpret_cast<const f4v*>(&red[w][tok][c4]);
    const size_t o = (size_t)tok * a.N + col0 + c4;
    if (a.parts) { *reinterpret_cast<f4v*>(a.parts + (size_t)blockIdx.y * a.rows * a.N + o) = v; return; }     // a K slice: raw partial sums
    if (a.bias) v += *reinterpret_cast<const f4v*>(a.bias + col0 + c4);
    if (a.res) v += *reinterpret_cast<const f4v*>(a.res + o);
    if (a.act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    else if (a.act == OMNI_ACT_GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    }
    if (a.dst_sh) act_store4<true>(a.dst, o, v);
    else          act_store4<false>(a.dst, o, v);
}

// LayerNorm(512) + the rows GEMM in one launch (K = 512): every block normalises all <= 32 rows itself — one wave per row, layernorm512_kernel's
// own loads, butterflies and expression, so the split-half values are the ones that kernel would have written — into LDS, where the
// fragment loads then find them; the block's weights are already travelling (they do not depend on x).  Saves a 3.4-us launch per
// LayerNorm of a lone panorama's transformer (12 of its 42); same bits as omni_layernorm512_sh + omni_gemm_rows_sh_f16x3.
__global__ __launch_bounds__(512) void gemm_rows_ln_sh_kernel(RowsGemmArgs a, const float* __restrict__ lg, const float* __restrict__ lb, float eps)
{
    constexpr int NWV = 8, KPW = 2, DEPTH = 2, PITCH = 36;
    __shared__ float red[NWV][32][PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char xs[32 * 2048];           // LayerNorm(x) as split-half rows [32][16 groups][hi32|lo32]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int col0 = blockIdx.x * 32, ksteps = 16, ks0 = wave * KPW;
    const unsigned char* wp = (const unsigned char*)a.wt + ((size_t)blockIdx.x * ksteps + ks0) * 4096 + lane * 16;
    h8v wh[DEPTH][2], wl[DEPTH][2];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            wh[i][kc] = *reinterpret_cast<const h8v*>(wp + i * 4096 + kc * 1024);
            wl[i][kc] = *reinterpret_cast<const h8v*>(wp + i * 4096 + 2048 + kc * 1024);
        }
    // ---- LayerNorm, one wave per row (rows wave, wave + 8, ...): layernorm512_kernel<true>, writing to LDS
    for (int row = wave; row < a.rows; row += NWV) {
        f4v v0, v1;
        if (a.nparts > 0) {
            // the input is the previous GEMM's K slices: x = (slice 0 + slice 1 + ...) + bias + residual, in that order (sh_splitk_reduce_ln512_kernel's);
            // every block forms it for itself, block 0 also stores it (the next residual)
            const size_t o = (size_t)row * 512, slab = (size_t)a.rows * 512;
            v0 = *reinterpret_cast<const f4v*>(a.parts + o + lane * 4); v1 = *reinterpret_cast<const f4v*>(a.parts + o + 256 + lane * 4);
            for (int sl = 1; sl < a.nparts; ++sl) {
                v0 += *reinterpret_cast<const f4v*>(a.parts + sl * slab + o + lane * 4);
                v1 += *reinterpret_cast<const f4v*>(a.parts + sl * slab + o + 256 + lane * 4);
            }
            if (a.pbias) { v0 += *reinterpret_cast<const f4v*>(a.pbias + lane * 4); v1 += *reinterpret_cast<const f4v*>(a.pbias + 256 + lane * 4); }
            if (a.pres) { v0 += *reinterpret_cast<const f4v*>(a.pres + o + lane * 4); v1 += *reinterpret_cast<const f4v*>(a.pres + o + 256 + lane * 4); }
            if (blockIdx.x == 0 && a.xout) { *reinterpret_cast<f4v*>(a.xout + o + lane * 4) = v0; *reinterpret_cast<f4v*>(a.xout + o + 256 + lane * 4) = v1; }
        } else {
            const float* p = (const float*)a.x + (size_t)row * 512;
            v0 = *reinterpret_cast<const f4v*>(p + lane * 4); v1 = *reinterpret_cast<const f4v*>(p + 256 + lane * 4);
        }
        float s = (v0.x + v0.y) + (v0.z + v0.w) + (v1.x + v1.y) + (v1.z + v1.w);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s * (1.0f / 512.0f);
        v0 -= mean; v1 -= mean;
        float q = (v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w) + (v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q * (1.0f / 512.0f) + eps);
        const f4v g0 = *reinterpret_cast<const f4v*>(lg + lane * 4), g1 = *reinterpret_cast<const f4v*>(lg + 256 + lane * 4);
        const f4v b0 = *reinterpret_cast<const f4v*>(lb + lane * 4), b1 = *reinterpret_cast<const f4v*>(lb + 256 + lane * 4);
        act_store4<true>(xs, (size_t)row * 512 + lane * 4, v0 * rstd * g0 + b0);
        act_store4<true>(xs, (size_t)row * 512 + 256 + lane * 4, v1 * rstd * g1 + b1);
    }
    __syncthreads();
    const unsigned char* xp = xs + ((size_t)r * ksteps + ks0) * 128 + h * 32;
    const bool live = r < a.rows;
    f16v acc = (f16v)(0.0f), acc1 = (f16v)(0.0f);
#pragma unroll
    for (int i = 0; i < KPW; ++i)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            const h8v xh = live ? *reinterpret_cast<const h8v*>(xp + i * 128 + kc * 16) : (h8v)(_Float16)0.0f;
            const h8v xl = live ? *reinterpret_cast<const h8v*>(xp + i * 128 + 64 + kc * 16) : (h8v)(_Float16)0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[i][kc], xh, acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[i][kc], xh, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[i][kc], xl, acc1, 0, 0, 0);
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f4v v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(acc1[4 * q + e], 4.8828125e-4f, acc[4 * q + e]);
        *reinterpret_cast<f4v*>(&red[wave][r][8 * q + 4 * h]) = v;
    }
    __syncthreads();
    const int tok = t >> 3, c4 = (t & 7) * 4;
    if (t >= 256 || tok >= a.rows) return;
    f4v v = *reinterpret_cast<const f4v*>(&red[0][tok][c4]);
#pragma unroll
    for (int w = 1; w < NWV; ++w) v += *reinterpret_cast<const f4v*>(&red[w][tok][c4]);
    const size_t o = (size_t)tok * a.N + col0 + c4;
    if (a.bias) v += *reinterpret_cast<const f4v*>(a.bias + col0 + c4);
    if (a.res) v += *reinterpret_cast<const f4v*>(a.res + o);
    if (a.act == OMNI_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    else if (a.act == OMNI_ACT_GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    }
    if (a.dst_sh) act_store4<true>(a.dst, o, v);
    else          act_store4<false>(a.dst, o, v);
}

}  // namespace

OMNI_SH_OVERFLOW_ACCESSOR(omni_sh_overflow_rows)

// Weights of omni_gemm_rows_sh_f16x3: wt16 [N][K/32][hi32|lo32] (as for omni_conv2d_sh_f16x3_ws) -> fragment order, same size.
extern "C" int omni_gemm_rows_pack(const void* wt16, void* wt16r, int N, int K, omni_stream_t stream)
{
    if (!wt16 || !wt16r || N <= 0 || N % 32 || K <= 0 || K % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_pack: null pointer or N, K not multiples of 32");
    const size_t pieces = (size_t)N * (K / 32) * 8;
    hipLaunchKernelGGL(gemm_rows_pack_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)wt16, (unsigned char*)wt16r, K / 32, pieces);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// out[rows, N] = act(x . W^T + bias + res) for rows <= 32 (see gemm_rows_sh_kernel): x SH [rows, K], wt16r from omni_gemm_rows_pack,
// res fp32 [rows, N] or null, fmt bit 0: dst is SH (else fp32).  K in {512, 2048}, N % 32 == 0.  The K summation order differs from the
// tile kernel's: equal to it up to fp32 rounding, not bit for bit.
extern "C" int omni_gemm_rows_sh_f16x3(const void* x, const void* wt16, const float* bias, const float* res, void* dst, int fmt,
                                       int rows, int K, int N, int act, omni_stream_t stream)
{
    if (!x || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_sh: null pointer");
    if (rows <= 0 || rows > 32 || N <= 0 || N % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_sh: 1..32 rows, N a multiple of 32");
    if (K != 512 && K != 2048) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_gemm_rows_sh: K must be 512 or 2048");
    if (fmt & 8) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_gemm_rows_sh: no f16x1 form (fmt bit 3)");
    RowsGemmArgs a;
    a.x = x; a.wt = wt16; a.bias = bias; a.res = res; a.dst = dst; a.rows = rows; a.K = K; a.N = N; a.act = act; a.dst_sh = fmt & 1;
    a.parts = nullptr; a.nparts = 0; a.pbias = nullptr; a.pres = nullptr; a.xout = nullptr;
    if (K == 512) hipLaunchKernelGGL(gemm_rows_sh_kernel<2>, dim3(N / 32), dim3(512), 0, (hipStream_t)stream, a);
    else          hipLaunchKernelGGL(gemm_rows_sh_kernel<8>, dim3(N / 32), dim3(512), 0, (hipStream_t)stream, a);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// LayerNorm over 512 channels (weight lg, bias lb, eps) of x fp32 [rows, 512], then omni_gemm_rows_sh_f16x3 on the result, in one launch
// (gemm_rows_ln_sh_kernel): the same bits as omni_layernorm512_sh followed by omni_gemm_rows_sh_f16x3.  rows <= 32, K = 512.
extern "C" int omni_gemm_rows_ln_sh_f16x3(const float* x, const float* lg, const float* lb, float eps, const void* wt16, const float* bias,
                                          const float* res, void* dst, int fmt, int rows, int N, int act, omni_stream_t stream)
{
    if (!x || !lg || !lb || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_ln_sh: null pointer");
    if (rows <= 0 || rows > 32 || N <= 0 || N % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_ln_sh: 1..32 rows, N a multiple of 32");
    if (fmt & 8) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_gemm_rows_ln_sh: no f16x1 form (fmt bit 3)");
    RowsGemmArgs a;
    a.x = x; a.wt = wt16; a.bias = bias; a.res = res; a.dst = dst; a.rows = rows; a.K = 512; a.N = N; a.act = act; a.dst_sh = fmt & 1;
    a.parts = nullptr; a.nparts = 0; a.pbias = nullptr; a.pres = nullptr; a.xout = nullptr;
    hipLaunchKernelGGL(gemm_rows_ln_sh_kernel, dim3(N / 32), dim3(512), 0, (hipStream_t)stream, a, lg, lb, eps);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// The K = 2048 rows GEMM (a lone panorama's fc2) as `slices` K slices over blockIdx.y: N / 32 x slices blocks instead of N / 32 — 16 blocks stream
// the 4 MB of fc2's weights in ~12 us, 64 in a third of that — each writing its RAW partial sums to parts[slice][rows][N] (fp32, no bias / residual).
// The consumer sums them: omni_gemm_rows_ln_parts_sh_f16x3 (the next block's norm1 + qkv) or omni_splitk_reduce_ln512 (encoder_norm).
// slices in {1, 2, 4} (K / 32 / slices / 8 K-steps per wave).
extern "C" int omni_gemm_rows_slices_sh_f16x3(const void* x, const void* wt16, float* parts, int rows, int K, int N, int slices, omni_stream_t stream)
{
    if (!x || !wt16 || !parts) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_slices_sh: null pointer");
    if (rows <= 0 || rows > 32 || N <= 0 || N % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_slices_sh: 1..32 rows, N a multiple of 32");
    if (K != 2048 || (slices != 1 && slices != 2 && slices != 4)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_gemm_rows_slices_sh: K = 2048 in 1, 2 or 4 slices");
    RowsGemmArgs a;
    a.x = x; a.wt = wt16; a.bias = nullptr; a.res = nullptr; a.dst = nullptr; a.rows = rows; a.K = K; a.N = N; a.act = OMNI_ACT_NONE; a.dst_sh = 0;
    a.parts = parts; a.nparts = slices; a.pbias = nullptr; a.pres = nullptr; a.xout = nullptr;
    const dim3 grid(N / 32, slices);
    if (slices == 4)      hipLaunchKernelGGL(gemm_rows_sh_kernel<2>, grid, dim3(512), 0, (hipStream_t)stream, a);
    else if (slices == 2) hipLaunchKernelGGL(gemm_rows_sh_kernel<4>, grid, dim3(512), 0, (hipStream_t)stream, a);
    else                  hipLaunchKernelGGL(gemm_rows_sh_kernel<8>, grid, dim3(512), 0, (hipStream_t)stream, a);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// omni_gemm_rows_ln_sh_f16x3 whose input is the previous GEMM's K slices: x = sum_s parts[s] + pbias + pres (fp32 [rows,512]; pbias / pres may be null),
// written to xout (the next residual) by one block; then LayerNorm + the rows GEMM as before.
extern "C" int omni_gemm_rows_ln_parts_sh_f16x3(const float* parts, int nparts, const float* pbias, const float* pres, float* xout,
                                                const float* lg, const float* lb, float eps, const void* wt16, const float* bias,
                                                void* dst, int fmt, int rows, int N, int act, omni_stream_t stream)
{
    if (!parts || nparts < 1 || nparts > 8 || !xout || !lg || !lb || !wt16 || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_ln_parts_sh: null pointer or 1..8 slices");
    if (rows <= 0 || rows > 32 || N <= 0 || N % 32) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gemm_rows_ln_parts_sh: 1..32 rows, N a multiple of 32");
    RowsGemmArgs a;
    a.x = nullptr; a.wt = wt16; a.bias = bias; a.res = nullptr; a.dst = dst; a.rows = rows; a.K = 512; a.N = N; a.act = act; a.dst_sh = fmt & 1;
    a.parts = const_cast<float*>(parts); a.nparts = nparts; a.pbias = pbias; a.pres = pres; a.xout = xout;
    hipLaunchKernelGGL(gemm_rows_ln_sh_kernel, dim3(N / 32), dim3(512), 0, (hipStream_t)stream, a, lg, lb, eps);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
