// omni_batchnorm.hip — batch normalisation in the library's NHWC layout with its backward:
//
//     y = act(batch_norm(x) + res),     x, res, y: fp32 [rows = M.H.W][C], C a multiple of 4, act none | relu
//
// Forward, training:  stats pass (per-slab partial sums of x and x^2 in DOUBLE)  ->  finish (mean, invstd, running buffers)  ->  apply.
// Forward, eval:      a one-block kernel turns the running buffers into the saved (mean, invstd) pair  ->  apply.
// Backward:           reduce pass (per-slab partials of sum dZ and sum dZ.xhat, in double)  ->  finish (dbeta, dgamma)  ->  apply (dx).
//
// One thread layout serves every element-wise and every reduction pass: a block of 256 threads owns a slab of rows and a column group of
// QW channel quads (QW = the power of two >= min(C/4, 64)); thread t holds quad t % QW in registers — its mean, scale and shift are loaded
// once — and walks the rows t / QW, t / QW + RL, ... of the slab (RL = 256 / QW).  A wave reads 64 / QW row segments of QW . 16 bytes.
//
// Sums: every thread adds its rows in order, in double (x is fp32, so x . x is exact there: a channel whose mean is large against its
// spread keeps its variance, which fp32 sums of x and x^2 do not).  The row lanes of a wave are added with the butterfly of omni_reduce.h
// stopped at offset QW (lanes that differ in a bit >= QW hold the same quad), the four waves as (w0 + w1) + (w2 + w3): block_sum's order,
// spelled out here because block_sum reduces all 64 lanes.  The finish kernels add a channel's slab partials by the column finish of
// omni_partials.h.  No atomics, nothing allocated, nothing synchronised, nothing read back: the same bits on every run.
//
// Statistics across ranks (omni_syncbn_*): the same passes, cut at the two finishes.  A rank leaves its two sums per channel
// in double with its row count (the exchange record, 2 C + 1 doubles); the caller gathers the records of all ranks; the forward's finish and
// the backward apply's prologue add them in rank order.  With one record the four calls give the bits of the two calls above.
#include <cmath>
#include <cstdint>

#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// Rows per thread at the least (the partials stay <= 1/8 of the slab's bytes) and slabs at the most.  Measured at the network's shapes
// (DESIGN §20): 16 rows and 2048 slabs cost the shapes of 4.5 to 18 MiB 10 to 30 % (too few blocks), 4 rows gain nothing over 8; the shapes
// of 72 MiB and more do not care.
constexpr int BN_MIN_ITERS = 8;
constexpr int BN_MAX_SLABS = 1024;

struct BnPlan { int qw, qshift, rl, slab, nslab, ncol; };

bool bn_plan(long long rows, int C, BnPlan& p)
{
    if (rows <= 0 || rows > 0x7fffffffll - 1024 || C <= 0 || C % 4) return false;          // (int row indices, stepped by up to 256)
    const int c4 = C / 4;
    p.qw = 1; p.qshift = 0;
    while (p.qw < c4 && p.qw < 64) { p.qw <<= 1; ++p.qshift; }
    p.rl = 256 / p.qw;
    p.ncol = (c4 + p.qw - 1) / p.qw;
    return partials_plan(rows, p.rl, BN_MIN_ITERS, BN_MAX_SLABS, p.slab, p.nslab);
}

size_t bn_part_bytes(const BnPlan& p, int C) { return (size_t)p.nslab * 2 * C * sizeof(double); }
size_t bn_ws_bytes(const BnPlan& p, int C) { return (bn_part_bytes(p, C) + (size_t)2 * C * sizeof(float) + 15) & ~(size_t)15; }

// The block's sums of a[0..4) and b[0..4) over its row lanes -> part[slab][0][4q..4q+4), part[slab][1][4q..4q+4).
__device__ __forceinline__ void bn_block_partials(double (&a)[4], double (&b)[4], double* __restrict__ part, int C, int q, bool active, int qw)
{
    __shared__ double red[4][8][64];
    const int t = threadIdx.x, lane = t & 63;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        for (int o = 32; o >= qw; o >>= 1) { a[e] += __shfl_xor(a[e], o); b[e] += __shfl_xor(b[e], o); }
    }
    if (lane < qw) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[t >> 6][e][lane] = a[e]; red[t >> 6][4 + e][lane] = b[e]; }
    }
    __syncthreads();
    if (t < qw && active) {                  // t < qw: lane == t == the quad's index in the column group, q is this thread's quad
        double* p0 = part + (size_t)blockIdx.x * 2 * C + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p0[e] = (red[0][e][t] + red[1][e][t]) + (red[2][e][t] + red[3][e][t]);
            p0[C + e] = (red[0][4 + e][t] + red[1][4 + e][t]) + (red[2][4 + e][t] + red[3][4 + e][t]);
        }
    }
}

// With qw < 64 a wave holds 64 / qw row lanes, with qw = 64 one; the waves' row lanes differ either way, so the four wave values are the
// block's.  (For qw < 64 the rows of wave w are rl = w . 64 / qw + lane / qw.)

__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int rows, int C, int qw,
                                                       int qshift, int slab)
{
    const int t = threadIdx.x, q = blockIdx.y * qw + (t & (qw - 1)), rl = 256 >> qshift;
    const bool active = 4 * q < C;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
#pragma unroll 4
        for (int r = r0 + (t >> qshift); r < rend; r += rl) {
            const f4v v = *(const f4v*)(x + (size_t)r * C + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double d = (double)v[e]; s[e] += d; ss[e] = fma(d, d, ss[e]); }
        }
    }
    bn_block_partials(s, ss, part, C, q, active, qw);
}

// Channel c from its two sums over n values: saved[0][c] = mean, saved[1][c] = 1 / sqrt(var_biased + eps), both computed in double and rounded
// once; the running buffers (both or neither) move by the momentum, the variance unbiased.
__device__ __forceinline__ void bn_finish_channel(double sum, double sumsq, double n, double eps, double momentum, int c, int C,
                                                  float* __restrict__ saved, float* __restrict__ running_mean, float* __restrict__ running_var)
{
    const double mean = sum / n;
    double var = sumsq / n - mean * mean;
    var = var < 0.0 ? 0.0 : var;                                 // (a NaN stays a NaN)
    saved[c] = (float)mean;
    saved[C + c] = (float)(1.0 / sqrt(var + eps));
    if (running_mean) {
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * (n / (n - 1.0))));
    }
}

// Block c: channel c, n = rows.
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ part, int nslab, int C, double n, double eps,
                                                              double momentum, float* __restrict__ saved, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var)
{
    __shared__ double red[2][4];
    const int t = threadIdx.x, c = blockIdx.x;
    double v[2];
    column_sums<2>(part + c, nslab, (size_t)2 * C, C, v, red);
    if (t == 0) bn_finish_channel(v[0], v[1], n, eps, momentum, c, C, saved, running_mean, running_var);
}

// Statistics across ranks.  A rank's exchange record is 2 C + 1 doubles: the two sums of every channel over its own rows —
// the column finish of its slab partials, left in double — and its row count.  Block c: channel c; dbeta / dgamma (backward; may be null)
// get the rank's own sums rounded once.
__global__ __launch_bounds__(256) void bn_record_finish_kernel(const double* __restrict__ part, int nslab, int C, double n,
                                                               double* __restrict__ rec, float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    __shared__ double red[2][4];
    const int t = threadIdx.x, c = blockIdx.x;
    double v[2];
    column_sums<2>(part + c, nslab, (size_t)2 * C, C, v, red);
    if (t == 0) {
        rec[c] = v[0];
        rec[C + c] = v[1];
        if (c == 0) rec[2 * C] = n;
        if (dbeta) dbeta[c] = (float)v[0];
        if (dgamma) dgamma[c] = (float)v[1];
    }
}

// Slot i of the gathered records all[world][2 C + 1], added in ascending rank order in double: every rank adds the same numbers in the same
// order, so all of them hold the same bits.  world == 1: the record's own value.
__device__ __forceinline__ double bn_rank_total(const double* __restrict__ all, int world, int C, int i)
{
    double v = all[i];
    for (int r = 1; r < world; ++r) v += all[(size_t)r * (2 * C + 1) + i];
    return v;
}

// Thread c: channel c from the totals over the ranks, n = the total of their row counts.
__global__ __launch_bounds__(256) void bn_sync_stats_finish_kernel(const double* __restrict__ all, int world, int C, double eps, double momentum,
                                                                   float* __restrict__ saved, float* __restrict__ running_mean,
                                                                   float* __restrict__ running_var)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double n = bn_rank_total(all, world, C, 2 * C);
    bn_finish_channel(bn_rank_total(all, world, C, c), bn_rank_total(all, world, C, C + c), n, eps, momentum, c, C, saved, running_mean,
                      running_var);
}

// eval mode: the saved pair from the running buffers
__global__ __launch_bounds__(256) void bn_eval_saved_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var, int C,
                                                            double eps, float* __restrict__ saved)
{
    for (int c = threadIdx.x; c < C; c += 256) {
        saved[c] = running_mean[c];
        saved[C + c] = (float)(1.0 / sqrt((double)running_var[c] + eps));
    }
}

__device__ __forceinline__ f4v ld4(const float* p, int q, float dflt)
{
    if (!p) return f4v{dflt, dflt, dflt, dflt};
    return *(const f4v*)(p + 4 * q);
}

// y = act(fmaf(x - mean, invstd . gamma, beta) + res)
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ saved, float* __restrict__ y,
                                                       int rows, int C, int qw, int qshift, int slab, int relu)
{
    const int t = threadIdx.x, q = blockIdx.y * qw + (t & (qw - 1)), rl = 256 >> qshift;
    if (4 * q >= C) return;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
    const f4v mean = ld4(saved, q, 0.0f), a = ld4(saved + C, q, 0.0f) * ld4(gamma, q, 1.0f), b = ld4(beta, q, 0.0f);
#pragma unroll 4
    for (int r = r0 + (t >> qshift); r < rend; r += rl) {
        const size_t o = (size_t)r * C + 4 * q;
        const f4v v = *(const f4v*)(x + o);
        f4v out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = fmaf(v[e] - mean[e], a[e], b[e]);
        if (res) { const f4v rv = *(const f4v*)(res + o); out += rv; }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = out[e] < 0.0f ? 0.0f : out[e];          // (a NaN passes, as in torch)
        }
        *(f4v*)(y + o) = out;
    }
}

// dZ = y > 0 ? g : 0 where the operator had a ReLU (y != null): a select, so a NaN behind an inactive ReLU stops here
__device__ __forceinline__ f4v bn_dz(const float* __restrict__ g, const float* __restrict__ y, size_t o)
{
    f4v v = *(const f4v*)(g + o);
    if (y) {
        const f4v yv = *(const f4v*)(y + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = yv[e] > 0.0f ? v[e] : 0.0f;
    }
    return v;
}

// partials of sum dZ and sum dZ . xhat, xhat = (x - mean) . invstd; dz != null: dZ is written for the apply pass and the residual
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ x,
                                                            const float* __restrict__ saved, float* __restrict__ dz, double* __restrict__ part,
                                                            int rows, int C, int qw, int qshift, int slab)
{
    const int t = threadIdx.x, q = blockIdx.y * qw + (t & (qw - 1)), rl = 256 >> qshift;
    const bool active = 4 * q < C;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, sx[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const f4v mean = ld4(saved, q, 0.0f), inv = ld4(saved + C, q, 0.0f);
#pragma unroll 4
        for (int r = r0 + (t >> qshift); r < rend; r += rl) {
            const size_t o = (size_t)r * C + 4 * q;
            const f4v d = bn_dz(g, y, o);
            const f4v v = *(const f4v*)(x + o);
            if (dz) *(f4v*)(dz + o) = d;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (v[e] - mean[e]) * inv[e];
                s[e] += (double)d[e];
                sx[e] = fma((double)d[e], (double)xh, sx[e]);
            }
        }
    }
    bn_block_partials(s, sx, part, C, q, active, qw);
}

// Block c: sums[0][c] = dbeta[c] = sum dZ, sums[1][c] = dgamma[c] = sum dZ . xhat, added in double and rounded once; the apply pass reads
// the rounded pair from `sums` (in the workspace), the caller's dbeta / dgamma are written where they are asked for.
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ part, int nslab, int C, float* __restrict__ sums,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    __shared__ double red[2][4];
    const int t = threadIdx.x, c = blockIdx.x;
    double v[2];
    column_sums<2>(part + c, nslab, (size_t)2 * C, C, v, red);
    if (t == 0) {
        sums[c] = (float)v[0];
        sums[C + c] = (float)v[1];
        if (dbeta) dbeta[c] = (float)v[0];
        if (dgamma) dgamma[c] = (float)v[1];
    }
}

// training (sums != null):  dx = gamma . invstd . ((dZ - dbeta / n) - xhat . dgamma / n);   eval:  dx = gamma . invstd . dZ.
// dres != null: dZ is written too (the residual's gradient, where no reduce pass ran).  dx may be null then.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ saved,
                                                           const float* __restrict__ sums, float* __restrict__ dx, float* __restrict__ dres,
                                                           int rows, int C, int qw, int qshift, int slab, double n)
{
    const int t = threadIdx.x, q = blockIdx.y * qw + (t & (qw - 1)), rl = 256 >> qshift;
    if (4 * q >= C) return;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
    f4v mean = {0.0f, 0.0f, 0.0f, 0.0f}, inv = mean, a = mean, k1 = mean, k2 = mean;
    if (dx) {
        mean = ld4(saved, q, 0.0f);
        inv = ld4(saved + C, q, 0.0f);
        a = inv * ld4(gamma, q, 1.0f);
        if (sums) {
            const f4v sb = ld4(sums, q, 0.0f), sg = ld4(sums + C, q, 0.0f);
#pragma unroll
            for (int e = 0; e < 4; ++e) { k1[e] = (float)((double)sb[e] / n); k2[e] = (float)((double)sg[e] / n); }
        }
    }
#pragma unroll 4
    for (int r = r0 + (t >> qshift); r < rend; r += rl) {
        const size_t o = (size_t)r * C + 4 * q;
        const f4v d = bn_dz(g, y, o);
        if (dres) *(f4v*)(dres + o) = d;
        if (dx) {
            f4v out;
            if (sums) {
                const f4v v = *(const f4v*)(x + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (v[e] - mean[e]) * inv[e];
                    out[e] = a[e] * fmaf(-xh, k2[e], d[e] - k1[e]);
                }
            } else {
                out = a * d;
            }
            *(f4v*)(dx + o) = out;
        }
    }
}

// The apply loop of bn_bwd_apply_kernel in training mode for a caller that holds k1 and k2 (statistics across ranks; that kernel keeps its
// own copy: its machine code is pinned).  dx = gamma . invstd . ((dZ - k1) - xhat . k2), a = gamma . invstd; dres != null: dZ is written too;
// dx may be null then.
__device__ __forceinline__ void bn_bwd_apply_rows(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ x,
                                                  float* __restrict__ dx, float* __restrict__ dres, int rows, int C, int q, int qshift, int slab,
                                                  f4v mean, f4v inv, f4v a, f4v k1, f4v k2)
{
    const int t = threadIdx.x, rl = 256 >> qshift;
    const int r0 = blockIdx.x * slab, rend = min(rows - r0, slab) + r0;
#pragma unroll 4
    for (int r = r0 + (t >> qshift); r < rend; r += rl) {
        const size_t o = (size_t)r * C + 4 * q;
        const f4v d = bn_dz(g, y, o);
        if (dres) *(f4v*)(dres + o) = d;
        if (dx) {
            const f4v v = *(const f4v*)(x + o);
            f4v out;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (v[e] - mean[e]) * inv[e];
                out[e] = a[e] * fmaf(-xh, k2[e], d[e] - k1[e]);
            }
            *(f4v*)(dx + o) = out;
        }
    }
}

// Statistics across ranks: the prologue adds the ranks' records of the thread's four channels (bn_rank_total), rounds each total once to
// fp32 — the pair the one-device backward keeps in its workspace — and divides by n = the total of the row counts.
__global__ __launch_bounds__(256) void bn_sync_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ x,
                                                                const float* __restrict__ gamma, const float* __restrict__ saved,
                                                                const double* __restrict__ all, int world, float* __restrict__ dx,
                                                                float* __restrict__ dres, int rows, int C, int qw, int qshift, int slab)
{
    const int q = blockIdx.y * qw + (threadIdx.x & (qw - 1));
    if (4 * q >= C) return;
    f4v mean = {0.0f, 0.0f, 0.0f, 0.0f}, inv = mean, a = mean, k1 = mean, k2 = mean;
    if (dx) {
        mean = ld4(saved, q, 0.0f);
        inv = ld4(saved + C, q, 0.0f);
        a = inv * ld4(gamma, q, 1.0f);
        const double n = bn_rank_total(all, world, C, 2 * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sb = (float)bn_rank_total(all, world, C, 4 * q + e), sg = (float)bn_rank_total(all, world, C, C + 4 * q + e);
            k1[e] = (float)((double)sb / n);
            k2[e] = (float)((double)sg / n);
        }
    }
    bn_bwd_apply_rows(g, y, x, dx, dres, rows, C, q, qshift, slab, mean, inv, a, k1, k2);
}

int bn_check_common(const char* who, long long rows, int C, int act, std::string& why, BnPlan& p)
{
    if (act == OMNI_ACT_GELU) { why = std::string(who) + ": no GELU (the operator keeps no pre-activation for its backward)"; return OMNI_ERR_UNSUPPORTED; }
    if (act != OMNI_ACT_NONE && act != OMNI_ACT_RELU) { why = std::string(who) + ": unknown activation"; return OMNI_ERR_INVALID; }
    if (C <= 0 || C % 4) { why = std::string(who) + ": channels must be a positive multiple of 4"; return OMNI_ERR_INVALID; }
    if (rows <= 0) { why = std::string(who) + ": rows >= 1"; return OMNI_ERR_INVALID; }
    if (!bn_plan(rows, C, p)) { why = std::string(who) + ": too many rows for 32-bit row indices"; return OMNI_ERR_UNSUPPORTED; }
    return OMNI_OK;
}

}  // namespace

extern "C" size_t omni_batchnorm_workspace_bytes(long long rows, int C)
{
    BnPlan p;
    if (!bn_plan(rows, C, p)) return 0;
    return bn_ws_bytes(p, C);
}

extern "C" int omni_batchnorm_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                      float* running_var, float* y, float* saved, long long rows, int C, int training, double momentum,
                                      double eps, int act, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_batchnorm_fwd", rows, C, act, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!x || !y || !saved) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: null pointer");
    if (!(eps > 0.0) || !std::isfinite(eps)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: eps must be positive and finite");
    if (!(momentum >= 0.0 && momentum <= 1.0)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: momentum must lie in [0, 1]");
    if ((running_mean == nullptr) != (running_var == nullptr))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: running_mean and running_var come together");
    if (!training && !running_mean) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: eval mode needs the running buffers");
    if (training && rows == 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: training mode expects more than 1 value per channel");
    if (training && (!workspace || ws_bytes < bn_ws_bytes(p, C))) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_fwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(p.nslab, p.ncol);
    if (training) {
        double* part = (double*)workspace;
        hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(256), 0, s, x, part, (int)rows, C, p.qw, p.qshift, p.slab);
        OMNI_HIP(hipGetLastError());
        hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(C), dim3(256), 0, s, (const double*)part, p.nslab, C, (double)rows, eps, momentum, saved,
                           running_mean, running_var);
        OMNI_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(bn_eval_saved_kernel, dim3(1), dim3(256), 0, s, (const float*)running_mean, (const float*)running_var, C, eps, saved);
        OMNI_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(256), 0, s, x, res, gamma, beta, (const float*)saved, y, (int)rows, C, p.qw, p.qshift, p.slab,
                       act == OMNI_ACT_RELU ? 1 : 0);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_batchnorm_bwd_f32(const float* g, const float* x, const float* y, const float* gamma, const float* saved, float* dx,
                                      float* dres, float* dgamma, float* dbeta, long long rows, int C, int training, int act, void* workspace,
                                      size_t ws_bytes, omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_batchnorm_bwd", rows, C, act, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    const bool relu = act == OMNI_ACT_RELU;
    if (!g) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: null pointer");
    if (!dx && !dres && !dgamma && !dbeta) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: no gradient requested");
    if (relu && !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: ReLU needs the forward's output");
    if (!relu && dres) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: without an activation the residual's gradient is g itself (pass dres = NULL)");
    if (training && rows == 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: training mode expects more than 1 value per channel");
    const bool params = dgamma || dbeta;
    const bool reduce = training ? (dx || params) : params;      // training: dx needs the two sums whatever is frozen
    if ((reduce || dx) && !saved) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: null pointer (the forward's saved mean and invstd)");
    if ((reduce || (dx && training)) && !x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: null pointer (x)");
    if (reduce && (!workspace || ws_bytes < bn_ws_bytes(p, C))) OMNI_FAIL(OMNI_ERR_INVALID, "omni_batchnorm_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(p.nslab, p.ncol);
    const float* ym = relu ? y : nullptr;
    float* sums = nullptr;
    bool dz_written = false;
    if (reduce) {
        double* part = (double*)workspace;
        sums = (float*)((char*)workspace + bn_part_bytes(p, C));
        dz_written = relu && dres;                               // the reduce pass writes dZ only where the residual wants it
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, grid, dim3(256), 0, s, g, ym, x, saved, dz_written ? dres : (float*)nullptr, part, (int)rows, C,
                           p.qw, p.qshift, p.slab);
        OMNI_HIP(hipGetLastError());
        hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(C), dim3(256), 0, s, (const double*)part, p.nslab, C, sums, dgamma, dbeta);
        OMNI_HIP(hipGetLastError());
    }
    const bool dres_in_apply = relu && dres && !dz_written;
    if (dx || dres_in_apply) {
        hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(256), 0, s, dz_written ? (const float*)dres : g, dz_written ? (const float*)nullptr : ym,
                           x, gamma, saved, training ? (const float*)sums : (const float*)nullptr, dx, dres_in_apply ? dres : (float*)nullptr,
                           (int)rows, C, p.qw, p.qshift, p.slab, (double)rows);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}

// ---------------------------------------------------------------------------------------------------------------- statistics across ranks
namespace {

bool bn_misaligned8(const void* p) { return ((uintptr_t)p & 7) != 0; }

}  // namespace

extern "C" int omni_syncbn_stats_f32(const float* x, double* sums, long long rows, int C, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_syncbn_stats", rows, C, OMNI_ACT_NONE, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!x || !sums) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_stats: null pointer");
    if (bn_misaligned8(sums)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_stats: the record must be 8-byte aligned");
    if (!workspace || ws_bytes < bn_ws_bytes(p, C)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_stats: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(bn_stats_kernel, dim3(p.nslab, p.ncol), dim3(256), 0, s, x, part, (int)rows, C, p.qw, p.qshift, p.slab);
    OMNI_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_record_finish_kernel, dim3(C), dim3(256), 0, s, (const double*)part, p.nslab, C, (double)rows, sums, (float*)nullptr,
                       (float*)nullptr);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_syncbn_fwd_apply_f32(const float* x, const float* res, const float* gamma, const float* beta, const double* all_sums,
                                         int world, float* running_mean, float* running_var, float* y, float* saved, long long rows, int C,
                                         double momentum, double eps, int act, omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_syncbn_fwd_apply", rows, C, act, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    if (!x || !y || !saved || !all_sums) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: null pointer");
    if (world < 1 || world > 64) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: world must lie in [1, 64]");
    if (bn_misaligned8(all_sums)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: the records must be 8-byte aligned");
    if (!(eps > 0.0) || !std::isfinite(eps)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: eps must be positive and finite");
    if (!(momentum >= 0.0 && momentum <= 1.0)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: momentum must lie in [0, 1]");
    if ((running_mean == nullptr) != (running_var == nullptr))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: running_mean and running_var come together");
    if (world == 1 && rows == 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_fwd_apply: training mode expects more than 1 value per channel");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_sync_stats_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, all_sums, world, C, eps, momentum, saved, running_mean,
                       running_var);
    OMNI_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_apply_kernel, dim3(p.nslab, p.ncol), dim3(256), 0, s, x, res, gamma, beta, (const float*)saved, y, (int)rows, C, p.qw,
                       p.qshift, p.slab, act == OMNI_ACT_RELU ? 1 : 0);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_syncbn_bwd_reduce_f32(const float* g, const float* x, const float* y, const float* saved, float* dz, double* sums,
                                          float* dgamma, float* dbeta, long long rows, int C, int act, void* workspace, size_t ws_bytes,
                                          omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_syncbn_bwd_reduce", rows, C, act, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    const bool relu = act == OMNI_ACT_RELU;
    if (!g || !x || !saved || !sums) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_reduce: null pointer");
    if (bn_misaligned8(sums)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_reduce: the record must be 8-byte aligned");
    if (relu && !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_reduce: ReLU needs the forward's output");
    if (!relu && dz) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_reduce: without an activation dZ is g itself (pass dz = NULL)");
    if (!workspace || ws_bytes < bn_ws_bytes(p, C)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_reduce: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(p.nslab, p.ncol), dim3(256), 0, s, g, relu ? y : (const float*)nullptr, x, saved, dz, part,
                       (int)rows, C, p.qw, p.qshift, p.slab);
    OMNI_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_record_finish_kernel, dim3(C), dim3(256), 0, s, (const double*)part, p.nslab, C, (double)rows, sums, dgamma, dbeta);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_syncbn_bwd_apply_f32(const float* g_or_dz, const float* y, const float* x, const float* gamma, const float* saved,
                                         const double* all_sums, int world, float* dx, float* dres, long long rows, int C, int act,
                                         omni_stream_t stream)
{
    BnPlan p; std::string why;
    const int rc = bn_check_common("omni_syncbn_bwd_apply", rows, C, act, why, p);
    if (rc != OMNI_OK) OMNI_FAIL(rc, why);
    const bool relu = act == OMNI_ACT_RELU;
    if (!g_or_dz) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: null pointer");
    if (!dx && !dres) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: no gradient requested");
    if (dres && !(relu && y))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: dres is dZ = g . [y > 0]: it needs act RELU and the forward's output (else the "
                                    "residual's gradient is the first argument itself)");
    if (dx && (!x || !saved || !all_sums)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: null pointer (x, saved and the records, for dx)");
    if (dx && (world < 1 || world > 64)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: world must lie in [1, 64]");
    if (dx && bn_misaligned8(all_sums)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: the records must be 8-byte aligned");
    if (dx && world == 1 && rows == 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_syncbn_bwd_apply: training mode expects more than 1 value per channel");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_sync_bwd_apply_kernel, dim3(p.nslab, p.ncol), dim3(256), 0, s, g_or_dz, relu ? y : (const float*)nullptr, x, gamma, saved,
                       all_sums, world, dx, dres, (int)rows, C, p.qw, p.qshift, p.slab);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
