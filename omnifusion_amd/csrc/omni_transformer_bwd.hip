// omni_transformer_bwd.hip — what a training step of the transformer between layer4 and the decoder needs beyond its five linear layers
// (DESIGN.md §21): layer normalisation over the last axis with its backward, the backward of the attention core (omni_attention_f32, the
// forward, lives in omni_net.hip and is not restated here) and the exact GELU with its backward.  fp32 only.
//
// Nothing is kept from a forward: the layer norm's backward recomputes mean and rstd from x with the forward's own code (ln_row_stats), the
// attention's backward recomputes the probabilities from q and k with the forward's arithmetic, GELU's backward reads x.
//
// Sums.  Within a row of a layer norm: every lane adds its quads in ascending order, pairs first ((x + y) + (z + w)), then the butterfly of
// omni_reduce.h — layernorm512_kernel's order, so that C = 512 gives its bits.  dgamma / dbeta: a thread owns a channel quad and adds the
// rows of its slab in ascending order in double (no lane ever adds another lane's value), the finish kernel adds a channel's slab partials
// by the column finish of omni_partials.h; one rounding to fp32.  Attention: the softmax sums are the forward's wave
// sums; delta_i, dq_i (over the keys j) and dk_j, dv_j (over the queries i) are added serially in ascending index order.  Nothing is
// allocated, nothing synchronises, nothing is read back, no read-modify-write of global memory: the same bits on every run.
#include <cmath>

#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- layer normalisation
constexpr int LN_MAX_C = 1024;             // four quads per lane of the row's wave
constexpr int LN_SLAB_ROWS = 8;            // rows per slab of the dgamma / dbeta partials at the least ...
constexpr int LN_MAX_SLABS = 1024;         // ... and slabs at the most

struct LnPlan { int slab, nslab; };

bool ln_plan(long long rows, int C, LnPlan& p)
{
    if (rows <= 0 || rows > 0x7fffffffll - 1024 || C < 4 || C > LN_MAX_C || C % 4) return false;
    return partials_plan(rows, 1, LN_SLAB_ROWS, LN_MAX_SLABS, p.slab, p.nslab);
}

size_t ln_part_bytes(const LnPlan& p, int C) { return (size_t)p.nslab * 2 * C * sizeof(double); }
size_t ln_ws_bytes(const LnPlan& p, long long rows, int C) { return (ln_part_bytes(p, C) + (size_t)rows * 2 * sizeof(float) + 15) & ~(size_t)15; }

// The wave's row: lane holds the quads lane, lane + 64, lane + 128, lane + 192 that lie inside C, centred on return.  The two-pass mean and
// centred variance of layernorm512_kernel, with C a run-time value (x / 512 and x * (1 / 512) are the same number).
__device__ __forceinline__ void ln_row_stats(const float* __restrict__ p, int C, int lane, f4v (&v)[4], bool (&on)[4], float& mean, float& rstd,
                                             float eps)
{
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        on[k] = (lane + 64 * k) * 4 < C;
        v[k] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
        if (on[k]) {
            v[k] = *reinterpret_cast<const f4v*>(p + (lane + 64 * k) * 4);
            if (k == 0) s = (v[k].x + v[k].y) + (v[k].z + v[k].w);
            else { s = s + (v[k].x + v[k].y); s = s + (v[k].z + v[k].w); }
        }
    }
    s = wave_sum(s);
    mean = s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (on[k]) {
            v[k] -= mean;
            if (k == 0) q = (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
            else { q = q + (v[k].x * v[k].x + v[k].y * v[k].y); q = q + (v[k].z * v[k].z + v[k].w * v[k].w); }
        }
    }
    q = wave_sum(q);
    rstd = 1.0f / sqrtf(q / (float)C + eps);
}

// one wave per row: y = v . rstd . g + b
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                     float* __restrict__ y, int rows, int C, float eps)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    f4v v[4]; bool on[4]; float mean, rstd;
    ln_row_stats(x + (size_t)row * C, C, lane, v, on, mean, rstd, eps);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!on[k]) continue;
        const int c = (lane + 64 * k) * 4;
        f4v o = v[k] * rstd;
        if (g) o = o * *reinterpret_cast<const f4v*>(g + c);
        if (b) o = o + *reinterpret_cast<const f4v*>(b + c);
        *reinterpret_cast<f4v*>(y + (size_t)row * C + c) = o;
    }
}

// one wave per row: stats[row] = (mean, rstd) where the reduction pass follows; dx = rstd . (a - mean_c(a) - xhat . mean_c(a . xhat)),
// a = grad_y . gamma, where dx is wanted
__global__ __launch_bounds__(256) void ln_bwd_row_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ g,
                                                         float* __restrict__ dx, float* __restrict__ stats, int rows, int C, float eps)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    f4v v[4]; bool on[4]; float mean, rstd;
    ln_row_stats(x + (size_t)row * C, C, lane, v, on, mean, rstd, eps);
    if (stats && lane == 0) { stats[2 * (size_t)row] = mean; stats[2 * (size_t)row + 1] = rstd; }
    if (!dx) return;
    f4v a[4];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!on[k]) continue;
        const int c = (lane + 64 * k) * 4;
        a[k] = *reinterpret_cast<const f4v*>(gy + (size_t)row * C + c);
        if (g) a[k] = a[k] * *reinterpret_cast<const f4v*>(g + c);
        v[k] = v[k] * rstd;                                                      // xhat
        const f4v ax = a[k] * v[k];
        if (k == 0) { s1 = (a[k].x + a[k].y) + (a[k].z + a[k].w); s2 = (ax.x + ax.y) + (ax.z + ax.w); }
        else {
            s1 = s1 + (a[k].x + a[k].y); s1 = s1 + (a[k].z + a[k].w);
            s2 = s2 + (ax.x + ax.y); s2 = s2 + (ax.z + ax.w);
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    const float m1 = s1 / (float)C, m2 = s2 / (float)C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!on[k]) continue;
        const int c = (lane + 64 * k) * 4;
        *reinterpret_cast<f4v*>(dx + (size_t)row * C + c) = ((a[k] - m1) - v[k] * m2) * rstd;
    }
}

// Block = one slab of rows, thread t = channel quad t: part[slab][0][c] = sum_r gy[r][c], part[slab][1][c] = sum_r gy[r][c] . xhat[r][c], the
// rows of the slab in ascending order, in double.  xhat = (x - mean) . rstd with the row pass's pair: the forward's value.
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ stats,
                                                            double* __restrict__ part, int rows, int C, int slab)
{
    const int q = threadIdx.x;
    if (4 * q >= C) return;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, sx[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0; r < rend; ++r) {
        const size_t o = (size_t)r * C + 4 * q;
        const f4v d = *reinterpret_cast<const f4v*>(gy + o), v = *reinterpret_cast<const f4v*>(x + o);
        const float mean = stats[2 * (size_t)r], rstd = stats[2 * (size_t)r + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (v[e] - mean) * rstd;
            s[e] += (double)d[e];
            sx[e] = fma((double)d[e], (double)xh, sx[e]);
        }
    }
    double* p0 = part + (size_t)blockIdx.x * 2 * C + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) { p0[e] = s[e]; p0[C + e] = sx[e]; }
}

// Block c: channel c; the column finish over the slab partials, rounded once.
__global__ __launch_bounds__(256) void ln_bwd_finish_kernel(const double* __restrict__ part, int nslab, int C, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta)
{
    __shared__ double red[2][4];
    const int t = threadIdx.x, c = blockIdx.x;
    double v[2];
    column_sums<2>(part + c, nslab, (size_t)2 * C, C, v, red);
    if (t == 0) {
        if (dbeta) dbeta[c] = (float)v[0];
        if (dgamma) dgamma[c] = (float)v[1];
    }
}

int ln_check(const char* who, long long rows, int C, float eps, std::string& why, LnPlan& p)
{
    if (C < 4 || C % 4) { why = std::string(who) + ": the row length must be a positive multiple of 4"; return OMNI_ERR_INVALID; }
    if (C > LN_MAX_C) { why = std::string(who) + ": at most 1024 values per row (one wave per row)"; return OMNI_ERR_UNSUPPORTED; }
    if (rows <= 0) { why = std::string(who) + ": rows >= 1"; return OMNI_ERR_INVALID; }
    if (!(eps > 0.0f) || !std::isfinite(eps)) { why = std::string(who) + ": eps must be positive and finite"; return OMNI_ERR_INVALID; }
    if (!ln_plan(rows, C, p)) { why = std::string(who) + ": too many rows for 32-bit row indices"; return OMNI_ERR_UNSUPPORTED; }
    return OMNI_OK;
}

// ---------------------------------------------------------------------------------------------------------------- attention, backward
constexpr float ATT_SCALE = 0.08838834764831845f;          // 128^-1/2, omni_attention_f32's

// Kernel 1, the forward's grid: block = (item, head) x a group of four queries, one wave per query i.  Recomputes row i of P with
// attention_kernel's arithmetic, then dP_ij = dO_i . v_j, delta_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - delta_i),
// dq_i = scale . sum_j dS_ij k_j; rows i of P and dS go to the workspace for kernel 2 (pw / dsw null: dkv is not wanted).
__global__ __launch_bounds__(256) void attention_bwd_rows_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                 const float* __restrict__ go, float* __restrict__ dq, float* __restrict__ pw,
                                                                 float* __restrict__ dsw, int N, float scale)
{
    __shared__ float ks[64][129];
    __shared__ float vs[64][129];
    __shared__ float ps[4][64];
    const int b = blockIdx.x >> 2, h = blockIdx.x & 3;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = t; i < N * 32; i += 256) {
        const int j = i >> 5, d = (i & 31) * 4;
        const float* row = kv + (size_t)(b * N + j) * 1024 + h * 128 + d;
        const f4v kk = *reinterpret_cast<const f4v*>(row), vv = *reinterpret_cast<const f4v*>(row + 512);
        ks[j][d] = kk.x; ks[j][d + 1] = kk.y; ks[j][d + 2] = kk.z; ks[j][d + 3] = kk.w;
        vs[j][d] = vv.x; vs[j][d + 1] = vv.y; vs[j][d + 2] = vv.z; vs[j][d + 3] = vv.w;
    }
    __syncthreads();
    const int i = blockIdx.y * 4 + wave;
    if (i >= N) return;                                            // (no barrier below: the waves only meet above)
    const float* qi = q + (size_t)(b * N + i) * 512 + h * 128;
    const float* gi = go + (size_t)(b * N + i) * 512 + h * 128;
    float s = -INFINITY, dp = 0.0f;
    if (lane < N) {
        float acc = 0.0f, acc2 = 0.0f;
        for (int d = 0; d < 128; ++d) acc = fmaf(qi[d], ks[lane][d], acc);
        for (int d = 0; d < 128; ++d) acc2 = fmaf(gi[d], vs[lane][d], acc2);
        s = acc * scale;
        dp = acc2;
    }
    const float mx = wave_max(s);
    const float e = (lane < N) ? expf(s - mx) : 0.0f;
    const float sum = wave_sum(e);
    const float p = e / sum;
    ps[wave][lane] = (lane < N) ? p * dp : 0.0f;
    __builtin_amdgcn_wave_barrier();
    float delta = 0.0f;
    for (int j = 0; j < N; ++j) delta += ps[wave][j];
    const float ds = p * (dp - delta);
    if (pw && lane < N) {
        const size_t o = ((size_t)blockIdx.x * N + i) * N + lane;
        pw[o] = p; dsw[o] = ds;
    }
    if (!dq) return;
    __builtin_amdgcn_wave_barrier();
    ps[wave][lane] = ds;
    __builtin_amdgcn_wave_barrier();
    float d0 = 0.0f, d1 = 0.0f;
    for (int j = 0; j < N; ++j) { const float dj = ps[wave][j]; d0 = fmaf(dj, ks[j][lane], d0); d1 = fmaf(dj, ks[j][lane + 64], d1); }
    float* oi = dq + (size_t)(b * N + i) * 512 + h * 128;
    oi[lane] = d0 * scale; oi[lane + 64] = d1 * scale;
}

// Kernel 2: block = (item, head) x a group of four keys, one wave per key j; lane i holds P_ij and dS_ij, lanes d and d + 64 the result:
// dv_j = sum_i P_ij dO_i, dk_j = scale . sum_i dS_ij q_i, i ascending.
__global__ __launch_bounds__(256) void attention_bwd_keys_kernel(const float* __restrict__ q, const float* __restrict__ go,
                                                                 const float* __restrict__ pw, const float* __restrict__ dsw,
                                                                 float* __restrict__ dkv, int N, float scale)
{
    __shared__ __attribute__((aligned(16))) float qs[64][128];
    __shared__ __attribute__((aligned(16))) float gs[64][128];
    const int b = blockIdx.x >> 2, h = blockIdx.x & 3;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = t; i < N * 32; i += 256) {
        const int r = i >> 5, d = (i & 31) * 4;
        const size_t o = (size_t)(b * N + r) * 512 + h * 128 + d;
        *reinterpret_cast<f4v*>(&qs[r][d]) = *reinterpret_cast<const f4v*>(q + o);
        *reinterpret_cast<f4v*>(&gs[r][d]) = *reinterpret_cast<const f4v*>(go + o);
    }
    __syncthreads();
    const int j = blockIdx.y * 4 + wave;
    if (j >= N) return;
    float pj = 0.0f, dsj = 0.0f;
    if (lane < N) {
        const size_t o = ((size_t)blockIdx.x * N + lane) * N + j;
        pj = pw[o]; dsj = dsw[o];
    }
    float v0 = 0.0f, v1 = 0.0f, k0 = 0.0f, k1 = 0.0f;
    for (int i = 0; i < N; ++i) {
        const float pi = __shfl(pj, i), di = __shfl(dsj, i);
        v0 = fmaf(pi, gs[i][lane], v0); v1 = fmaf(pi, gs[i][lane + 64], v1);
        k0 = fmaf(di, qs[i][lane], k0); k1 = fmaf(di, qs[i][lane + 64], k1);
    }
    float* o = dkv + (size_t)(b * N + j) * 1024 + h * 128;
    o[lane] = k0 * scale; o[lane + 64] = k1 * scale;
    o[512 + lane] = v0; o[512 + lane + 64] = v1;
}

size_t att_ws_bytes(int B, int N) { return (size_t)2 * B * 4 * N * N * sizeof(float); }
bool att_in_scope(int B, int N) { return B >= 1 && B <= (1 << 20) && N >= 1 && N <= 64; }

// ---------------------------------------------------------------------------------------------------------------- GELU (exact)
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f4v v = *reinterpret_cast<const f4v*>(x + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    *reinterpret_cast<f4v*>(y + 4 * i) = v;
}

// dx = g . (Phi(x) + x . phi(x)),  Phi(x) = 0.5 (1 + erf(x / sqrt 2)),  phi(x) = exp(-x^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ dx, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f4v v = *reinterpret_cast<const f4v*>(x + 4 * i), gv = *reinterpret_cast<const f4v*>(g + 4 * i);
    f4v o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float cdf = 0.5f * (1.0f + erff(v[e] * 0.70710678118654752440f));
        const float pdf = expf(-0.5f * v[e] * v[e]) * 0.39894228040143267794f;
        o[e] = gv[e] * (cdf + v[e] * pdf);
    }
    *reinterpret_cast<f4v*>(dx + 4 * i) = o;
}

}  // namespace

// ================================================================================================================ entry points
extern "C" size_t omni_layernorm_bwd_workspace_bytes(long long rows, int C)
{
    LnPlan p;
    if (!ln_plan(rows, C, p)) return 0;
    return ln_ws_bytes(p, rows, C);
}

extern "C" int omni_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, long long rows, int C, float eps,
                                      omni_stream_t stream)
{
    LnPlan p; std::string why;
    const int rc = ln_check("omni_layernorm_fwd", rows, C, eps, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!x || !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_layernorm_fwd: null pointer");
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, (int)rows, C, eps);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_layernorm_bwd_f32(const float* grad_y, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta,
                                      long long rows, int C, float eps, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    LnPlan p; std::string why;
    const int rc = ln_check("omni_layernorm_bwd", rows, C, eps, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!grad_y || !x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_layernorm_bwd: null pointer");
    if (!dx && !dgamma && !dbeta) OMNI_FAIL(OMNI_ERR_INVALID, "omni_layernorm_bwd: no gradient requested");
    const bool reduce = dgamma || dbeta;
    if (reduce && (!workspace || ws_bytes < ln_ws_bytes(p, rows, C))) OMNI_FAIL(OMNI_ERR_INVALID, "omni_layernorm_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    float* stats = reduce ? (float*)((char*)workspace + ln_part_bytes(p, C)) : nullptr;
    hipLaunchKernelGGL(ln_bwd_row_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, grad_y, x, gamma, dx, stats, (int)rows, C, eps);
    OMNI_HIP(hipGetLastError());
    if (reduce) {
        hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3(p.nslab), dim3(256), 0, s, grad_y, x, (const float*)stats, part, (int)rows, C, p.slab);
        OMNI_HIP(hipGetLastError());
        hipLaunchKernelGGL(ln_bwd_finish_kernel, dim3(C), dim3(256), 0, s, (const double*)part, p.nslab, C, dgamma, dbeta);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}

extern "C" size_t omni_attention_bwd_workspace_bytes(int B, int N)
{
    return att_in_scope(B, N) ? att_ws_bytes(B, N) : 0;
}

extern "C" int omni_attention_bwd_f32(const float* q, const float* kv, const float* grad_out, float* dq, float* dkv, int B, int N,
                                      void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    if (B < 1 || N < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_attention_bwd: B >= 1 and N >= 1");
    if (N > 64) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_attention_bwd: at most 64 tokens");
    if (!att_in_scope(B, N)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_attention_bwd: too many batch items");
    if (!q || !kv || !grad_out) OMNI_FAIL(OMNI_ERR_INVALID, "omni_attention_bwd: null pointer");
    if (!dq && !dkv) OMNI_FAIL(OMNI_ERR_INVALID, "omni_attention_bwd: no gradient requested");
    if (dkv && (!workspace || ws_bytes < att_ws_bytes(B, N))) OMNI_FAIL(OMNI_ERR_INVALID, "omni_attention_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B * 4, (N + 3) / 4);
    float* pw = dkv ? (float*)workspace : nullptr;
    float* dsw = dkv ? pw + (size_t)B * 4 * N * N : nullptr;
    hipLaunchKernelGGL(attention_bwd_rows_kernel, grid, dim3(256), 0, s, q, kv, grad_out, dq, pw, dsw, N, ATT_SCALE);
    OMNI_HIP(hipGetLastError());
    if (dkv) {
        hipLaunchKernelGGL(attention_bwd_keys_kernel, grid, dim3(256), 0, s, q, grad_out, (const float*)pw, (const float*)dsw, dkv, N, ATT_SCALE);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}

static int gelu_check(const char* who, long long n, std::string& why)
{
    if (n <= 0 || n % 4) { why = std::string(who) + ": the element count must be a positive multiple of 4"; return OMNI_ERR_INVALID; }
    if (n / 4 > 0x7fffffffll * 256) { why = std::string(who) + ": too many elements for one launch"; return OMNI_ERR_UNSUPPORTED; }
    return OMNI_OK;
}

extern "C" int omni_gelu_fwd_f32(const float* x, float* y, long long n, omni_stream_t stream)
{
    std::string why;
    const int rc = gelu_check("omni_gelu_fwd", n, why);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!x || !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gelu_fwd: null pointer");
    const size_t n4 = (size_t)n / 4;
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n4);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_gelu_bwd_f32(const float* grad_y, const float* x, float* dx, long long n, omni_stream_t stream)
{
    std::string why;
    const int rc = gelu_check("omni_gelu_bwd", n, why);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!grad_y || !x || !dx) OMNI_FAIL(OMNI_ERR_INVALID, "omni_gelu_bwd: null pointer");
    const size_t n4 = (size_t)n / 4;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_y, x, dx, n4);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
