// omni_optim.hip — AdamW on the device over one flat arena: the optimiser of the training scripts, with the gradient norm
// and the clip of clip_grad_norm_, as three launches that read everything that changes from step to step out of device memory.
//
// Layout.  Parameters live in one fp32 arena, a segment per tensor, every segment at a multiple of 64 floats; exp_avg and exp_avg_sq are
// two more arenas of the same layout.  The padding between segments is zero and no kernel reads or writes it.  A chunk is OPT_CHUNK
// elements of ONE segment (chunks start at segment starts, the last chunk of a segment is short), so a block never needs to know where a
// tensor ends inside its chunk other than by the segment's count.  Two device tables describe the work, both built by the caller:
//     segments  long long [nseg][4]   arena offset (floats), element count, address of the gradient (0: none), parameter group
//     chunks    int [nchunk][2]       segment, offset of the chunk within the segment (a multiple of OPT_CHUNK)
// Thread t of a block owns the quads 4 t + 1024 k, k < 4, of a chunk — in the norm pass and in the update alike, and whether the gradient
// is read with 16-byte loads (its address is 16-byte aligned: decided per segment) or with four scalar loads: the same elements meet in
// the same order, so a gradient's alignment never changes a bit.
//
//   1. grad_sqnorm_kernel   one double per chunk: sum of g . g in double (exact products), per thread over its elements ascending, then
//                           block_sum.  A segment without a gradient contributes 0.  At most OPT_MAX_BLOCKS blocks; block b walks the chunks
//                           b, b + grid, ...
//   2. prepare_kernel       ONE block: the partials added by the column finish of omni_partials.h, rounded once to fp32, then the square
//                           root; writes the step record (below) and moves the counters.  The only place the step counter changes.
//   3. apply_kernel         torch's AdamW in fp32 over the chunk table; reads the record, never writes a gradient.
//
// Step record, float [4 + 8 . ngroups]:  [0] the norm before clipping, [1] clip = min(1, max_norm / (norm + 1e-6)) (1 without clipping),
// [2] 1 where the norm is not finite, [3] 1 where the step is skipped; then per group  1 - lr . wd,  lr / (1 - beta1^t),  sqrt(1 - beta2^t),
// eps,  beta2,  1 - beta1,  1 - beta2,  0 — each computed in double from the group table (lr, beta1, beta2, eps, weight_decay as doubles)
// and rounded once.  Counters, long long [2]: the step count t, the skipped steps.
//
// No atomics, nothing allocated, nothing synchronised, nothing read back: the same bits on every run, and the three calls can be captured.
#include <cmath>
#include <cstdint>

#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int OPT_CHUNK = 4096;            // elements per chunk: 256 threads x 4 quads (omnifusion_amd/optim.py: CHUNK)
constexpr int OPT_MAX_BLOCKS = 2048;
constexpr int OPT_MAX_GROUPS = 256;        // one thread of the prepare block per group
constexpr int OPT_REC_HEAD = 4, OPT_REC_GROUP = 8;

struct OptChunk { const float* g; long long base; int count; int group; };

// The chunk's segment: false where the tables disagree with nseg (never dereferenced then).
__device__ __forceinline__ bool opt_chunk(const long long* __restrict__ seg, int nseg, const int2* __restrict__ chunks, int c, OptChunk& out)
{
    const int2 ch = chunks[c];
    if (ch.x < 0 || ch.x >= nseg || ch.y < 0) return false;
    const long long* s = seg + 4 * (size_t)ch.x;
    const long long left = s[1] - ch.y;
    if (left <= 0) return false;
    out.g = (const float*)(uintptr_t)s[2];
    if (out.g) out.g += ch.y;
    out.base = s[0] + ch.y;
    out.count = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    out.group = (int)s[3];
    return true;
}

// Quad e0 .. e0 + 3 of a chunk of `count` elements; elements past the count read as `dflt` and are never touched.
__device__ __forceinline__ f4v opt_load(const float* __restrict__ p, int e0, int count, bool wide, float dflt)
{
    if (wide && e0 + 4 <= count) return *(const f4v*)(p + e0);
    f4v v = {dflt, dflt, dflt, dflt};
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e0 + e < count) v[e] = p[e0 + e];
    return v;
}

__device__ __forceinline__ void opt_store(float* __restrict__ p, int e0, int count, f4v v)
{
    if (e0 + 4 <= count) { *(f4v*)(p + e0) = v; return; }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e0 + e < count) p[e0 + e] = v[e];
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const long long* __restrict__ seg, int nseg, const int2* __restrict__ chunks, int nchunk,
                                                          double* __restrict__ part)
{
    __shared__ double red[1][4];
    const int t = threadIdx.x;
    for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
        OptChunk ch;
        double v[1] = {0.0};
        if (opt_chunk(seg, nseg, chunks, c, ch) && ch.g) {                      // (uniform over the block)
            const bool wide = ((uintptr_t)ch.g & 15) == 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e0 = 4 * t + 1024 * k;
                if (e0 < ch.count) {
                    const f4v g = opt_load(ch.g, e0, ch.count, wide, 0.0f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[0] += (double)g[e] * (double)g[e];
                }
            }
        }
        block_sum<1>(v, red);
        if (t == 0) part[c] = v[0];
        __syncthreads();                                                        // red is reused by the next chunk
    }
}

__global__ __launch_bounds__(256) void prepare_kernel(const double* __restrict__ part, int nchunk, const double* __restrict__ groups, int ngroups,
                                                      double max_norm, int skip_nonfinite, float* __restrict__ rec, long long* __restrict__ counters)
{
    __shared__ double red[1][4];
    const int t = threadIdx.x;
    double v[1];
    column_sums<1>(part, nchunk, 1, 0, v, red);
    const float norm = sqrtf((float)v[0]);
    const bool bad = !(fabsf(norm) <= 3.402823466e38f);                        // inf or NaN
    const bool skip = skip_nonfinite && bad;
    const long long step = counters[0] + (skip ? 0 : 1);
    __syncthreads();                                                            // every thread has read the counter
    if (t == 0) {
        float clip = 1.0f;
        if (max_norm >= 0.0) {
            const float c = (float)max_norm / (norm + 1e-6f);                   // torch's clip_grad_norm_, in fp32
            clip = c < 1.0f || c != c ? c : 1.0f;                               // (a NaN stays a NaN, as torch.clamp leaves it)
        }
        rec[0] = norm;
        rec[1] = clip;
        rec[2] = bad ? 1.0f : 0.0f;
        rec[3] = skip ? 1.0f : 0.0f;
        if (skip) counters[1] += 1; else counters[0] = step;
    }
    if (t < ngroups) {
        const double lr = groups[5 * t], beta1 = groups[5 * t + 1], beta2 = groups[5 * t + 2], eps = groups[5 * t + 3], wd = groups[5 * t + 4];
        float* r = rec + OPT_REC_HEAD + OPT_REC_GROUP * t;
        r[0] = (float)(1.0 - lr * wd);
        r[1] = (float)(lr / (1.0 - pow(beta1, (double)step)));
        r[2] = (float)sqrt(1.0 - pow(beta2, (double)step));
        r[3] = (float)eps;
        r[4] = (float)beta2;
        r[5] = (float)(1.0 - beta1);
        r[6] = (float)(1.0 - beta2);
        r[7] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void apply_kernel(float* __restrict__ params, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                    const long long* __restrict__ seg, int nseg, const int2* __restrict__ chunks, int nchunk,
                                                    const float* __restrict__ rec, int ngroups)
{
    if (rec[3] != 0.0f) return;                                                 // a skipped step touches nothing
    const float clip = rec[1];
    const int t = threadIdx.x;
    for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
        OptChunk ch;
        if (!opt_chunk(seg, nseg, chunks, c, ch) || !ch.g || ch.group < 0 || ch.group >= ngroups) continue;
        const float* r = rec + OPT_REC_HEAD + OPT_REC_GROUP * ch.group;
        const float decay = r[0], step_size = r[1], bc2_sqrt = r[2], eps = r[3], beta2 = r[4], omb1 = r[5], omb2 = r[6];
        const bool wide = ((uintptr_t)ch.g & 15) == 0;
        float* p = params + ch.base;
        float* m = exp_avg + ch.base;
        float* s = exp_avg_sq + ch.base;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e0 = 4 * t + 1024 * k;
            if (e0 >= ch.count) continue;
            const f4v gv = opt_load(ch.g, e0, ch.count, wide, 0.0f);
            f4v pv = opt_load(p, e0, ch.count, true, 0.0f), mv = opt_load(m, e0, ch.count, true, 0.0f), sv = opt_load(s, e0, ch.count, true, 0.0f);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = gv[e] * clip;
                const float pd = pv[e] * decay;
                mv[e] = fmaf(g - mv[e], omb1, mv[e]);
                sv[e] = fmaf(omb2 * g, g, sv[e] * beta2);
                const float denom = sqrtf(sv[e]) / bc2_sqrt + eps;
                pv[e] = fmaf(-step_size, mv[e] / denom, pd);
            }
            opt_store(p, e0, ch.count, pv);
            opt_store(m, e0, ch.count, mv);
            opt_store(s, e0, ch.count, sv);
        }
    }
}

int opt_check_tables(const char* who, const void* segments, int nseg, const int* chunks, int nchunk)
{
    if (!segments || !chunks) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": null table");
    if (nseg <= 0 || nchunk <= 0) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": nseg and nchunk must be positive");
    if (((uintptr_t)segments & 7) || ((uintptr_t)chunks & 7)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": tables must be 8-byte aligned");
    return OMNI_OK;
}

}  // namespace

extern "C" int omni_adamw_grad_sqnorm_f32(const void* segments, int nseg, const int* chunks, int nchunk, double* partials, omni_stream_t stream)
{
    const int rc = opt_check_tables("omni_adamw_grad_sqnorm", segments, nseg, chunks, nchunk);
    if (rc != OMNI_OK) return rc;
    if (!partials || ((uintptr_t)partials & 7)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_grad_sqnorm: partials must be a non-null, 8-byte aligned pointer");
    const int grid = nchunk < OPT_MAX_BLOCKS ? nchunk : OPT_MAX_BLOCKS;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const long long*)segments, nseg, (const int2*)chunks,
                       nchunk, partials);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_adamw_prepare_f32(const double* partials, int nchunk, const double* groups, int ngroups, double max_norm, int skip_nonfinite,
                                      float* record, long long* counters, omni_stream_t stream)
{
    if (!partials || !groups || !record || !counters) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_prepare: null pointer");
    if (nchunk <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_prepare: nchunk must be positive");
    if (ngroups <= 0 || ngroups > OPT_MAX_GROUPS) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_prepare: 1 to 256 parameter groups");
    if (max_norm != max_norm) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_prepare: max_norm is NaN (negative: no clipping)");
    if (((uintptr_t)partials & 7) || ((uintptr_t)groups & 7) || ((uintptr_t)counters & 7) || ((uintptr_t)record & 3))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_prepare: misaligned pointer");
    hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nchunk, groups, ngroups, max_norm,
                       skip_nonfinite ? 1 : 0, record, counters);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_adamw_apply_f32(float* params, float* exp_avg, float* exp_avg_sq, const void* segments, int nseg, const int* chunks, int nchunk,
                                    const float* record, int ngroups, omni_stream_t stream)
{
    const int rc = opt_check_tables("omni_adamw_apply", segments, nseg, chunks, nchunk);
    if (rc != OMNI_OK) return rc;
    if (!params || !exp_avg || !exp_avg_sq || !record) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_apply: null pointer");
    if (((uintptr_t)params & 15) || ((uintptr_t)exp_avg & 15) || ((uintptr_t)exp_avg_sq & 15))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_apply: the arenas must be 16-byte aligned");
    if (ngroups <= 0 || ngroups > OPT_MAX_GROUPS) OMNI_FAIL(OMNI_ERR_INVALID, "omni_adamw_apply: 1 to 256 parameter groups");
    const int grid = nchunk < OPT_MAX_BLOCKS ? nchunk : OPT_MAX_BLOCKS;
    hipLaunchKernelGGL(apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, params, exp_avg, exp_avg_sq, (const long long*)segments, nseg,
                       (const int2*)chunks, nchunk, record, ngroups);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
