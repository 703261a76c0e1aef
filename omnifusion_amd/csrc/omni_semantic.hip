// omni_semantic.hip — the supervision and scoring of the reference's segmentation script (train_erp_sem.py:203-210, 261-278; iou.py:21-24) in one
// streaming pass over the logits [B, C, H, W]:
//
//   omni_semantic_step_f32      F.cross_entropy(logits, target, ignore_index) (mean), argmax over the classes and confusion[pred, gt], one read
//                               of each logit.  A lane owns a pixel (four where H*W is a multiple of 4: 16-byte loads) and walks the C planes,
//                               so every plane read is coalesced across the wave.
//   omni_semantic_grad_f32      grad_logits = (softmax - onehot) * (*grad_out) / count from the per-pixel log-sum-exp the forward saved
//   omni_confusion_matrix_i64   the same histogram from two label maps
//
// The loss sum is reproducible: per-block partials in double, summed by one block in a fixed order.  The confusion counts go into a per-block LDS
// histogram (lanes of a wave that hit the same bin are counted by ONE add: label maps are piecewise constant) and leave with 64-bit integer
// atomics, whose sum does not depend on the order.  Pixel rules: a target equal to ignore_index is outside the loss, a negative
// label is outside the matrix (iou.py:23), and a label or prediction that is neither is dropped from both and counted in n_bad — nothing is
// ever read or counted out of range.
#include "omni_internal.h"
#include "omni_reduce.h"

namespace {

constexpr int SEM_THREADS = 256;
constexpr int SEM_MAX_BLOCKS = 2048;
constexpr int SEM_MAX_K = 64;
constexpr int SEM_LEADERS = 4;            // distinct bins a wave counts by ballot before its remaining lanes add one by one
constexpr size_t SEM_HEADER = 64;         // workspace: int64 count, int64 n_bad | SEM_MAX_BLOCKS x SemPart | float lse[npix]

struct SemPart { double sum; long long count; long long bad; };

__host__ __device__ inline size_t sem_lse_offset() { return SEM_HEADER + sizeof(SemPart) * (size_t)SEM_MAX_BLOCKS; }

// One add per distinct bin of the wave for the first SEM_LEADERS bins, then one per lane.  bin < 0: nothing to count.  Every lane of the wave calls it.
__device__ __forceinline__ void hist_add(unsigned* __restrict__ h, int bin)
{
    unsigned long long todo = __ballot(bin >= 0);
    for (int it = 0; it < SEM_LEADERS && todo; ++it) {
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const int lb = __shfl(bin, lead);
        const unsigned long long same = __ballot(bin == lb);
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[lb], (unsigned)__popcll(same));
        todo &= ~same;
        if (bin == lb) bin = -1;
    }
    if (bin >= 0) atomicAdd(&h[bin], 1u);
}

__device__ __forceinline__ void hist_flush(const unsigned* __restrict__ h, int KK, long long* __restrict__ confusion)
{
    for (int i = threadIdx.x; i < KK; i += SEM_THREADS)
        if (h[i]) atomicAdd(reinterpret_cast<unsigned long long*>(confusion) + i, (unsigned long long)h[i]);
}

// bin of one pixel of the matrix, -1 if the pixel is outside it; bad: the pixel is dropped under the out-of-range rule
__device__ __forceinline__ int conf_bin(long long pred, long long gt, int K, bool& bad)
{
    if (gt < 0) return -1;                                                   // iou.py:23 (also UNKNOWN_ID = -100)
    if (gt >= K || pred < 0 || pred >= K) { bad = true; return -1; }
    return (int)pred * K + (int)gt;
}

template <int PX> struct Vec;
template <> struct Vec<1> { using F = float; };
template <> struct Vec<4> { using F = float4; };
__device__ __forceinline__ float elem(const float& v, int) { return v; }
__device__ __forceinline__ float elem(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
// PX consecutive elements as 16-byte accesses (PX = 4: the address is 16-byte aligned)
template <int PX> __device__ __forceinline__ void load_px(const long long* __restrict__ p, long long (&v)[PX])
{
    if constexpr (PX == 4) {
        const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else v[0] = *p;
}
template <int PX> __device__ __forceinline__ void store_px(long long* __restrict__ p, const int (&v)[PX])
{
    if constexpr (PX == 4) {
        reinterpret_cast<longlong2*>(p)[0] = make_longlong2(v[0], v[1]);
        reinterpret_cast<longlong2*>(p)[1] = make_longlong2(v[2], v[3]);
    } else *p = v[0];
}
template <int PX> __device__ __forceinline__ void load_px(const float* __restrict__ p, float (&v)[PX])
{
    if constexpr (PX == 4) { const float4 a = *reinterpret_cast<const float4*>(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
    else v[0] = *p;
}
template <int PX> __device__ __forceinline__ void store_px(float* __restrict__ p, const float (&v)[PX])
{
    if constexpr (PX == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// PX pixels per lane (PX = 4 needs HW % 4 == 0 and 16-byte aligned bases: the four pixels then lie in one image, 16 bytes apart per plane)
template <int PX>
__global__ __launch_bounds__(SEM_THREADS) void semantic_step_kernel(const float* __restrict__ logits, const long long* __restrict__ target, int C,
                                                                    size_t HW, size_t npix, long long ignore_index, int K,
                                                                    SemPart* __restrict__ part, float* __restrict__ lse_out,
                                                                    long long* __restrict__ pred_out, long long* __restrict__ confusion)
{
    using F = typename Vec<PX>::F;
    __shared__ unsigned hist[SEM_MAX_K * SEM_MAX_K];
    __shared__ double red_sum[1][SEM_THREADS / 64];
    __shared__ long long red_cnt[2][SEM_THREADS / 64];                        // count, bad
    const int KK = K * K;
    if (confusion) {
        for (int i = threadIdx.x; i < KK; i += SEM_THREADS) hist[i] = 0;
        __syncthreads();
    }
    double sum = 0.0;
    long long count = 0, nbad = 0;
    const size_t step = (size_t)gridDim.x * SEM_THREADS * PX;
    for (size_t base = (size_t)blockIdx.x * SEM_THREADS * PX; base < npix; base += step) {          // block-uniform: every lane runs every round
        const size_t p = base + (size_t)threadIdx.x * PX;
        const bool in = p < npix;                                            // (PX = 4: npix % 4 == 0, all four or none)
        const size_t b = in ? p / HW : 0, i = in ? p - b * HW : 0;
        const float* x0 = logits + b * (size_t)C * HW + i;
        long long t[PX];
        float m[PX], s[PX], xt[PX];
        int best[PX];
        if (in) {
            load_px<PX>(target + p, t);
            const F v = *reinterpret_cast<const F*>(x0);
#pragma unroll
            for (int k = 0; k < PX; ++k) { m[k] = elem(v, k); s[k] = 1.0f; best[k] = 0; xt[k] = m[k]; }
#pragma unroll 4
            for (int c = 1; c < C; ++c) {
                const F w = *reinterpret_cast<const F*>(x0 + (size_t)c * HW);
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const float x = elem(w, k);
                    // running maximum with torch.argmax's rules: the first index wins a tie, a NaN wins over everything and is then kept
                    const bool up = (x > m[k]) || (x != x && m[k] == m[k]);
                    const float e = (x == m[k] && x < 0.0f) ? 1.0f : expf(-fabsf(x - m[k]));    // one exponential per logit, argument <= 0 (-inf beside -inf counts once each, as in torch)
                    s[k] = up ? fmaf(s[k], e, 1.0f) : s[k] + e;
                    m[k] = up ? x : m[k];
                    best[k] = up ? c : best[k];
                    xt[k] = (t[k] == (long long)c) ? x : xt[k];
                }
            }
        }
        float lse[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            int bin = -1;
            if (in) {
                const bool ignored = t[k] == ignore_index;
                const bool valid = !ignored && t[k] >= 0 && t[k] < (long long)C;
                bool bad = !ignored && !valid;
                const float ls = logf(s[k]);
                if (valid) { sum += ((double)m[k] - (double)xt[k]) + (double)ls; ++count; }      // lse - x[target]; m - x[target] is exact in double
                lse[k] = m[k] + ls;
                if (confusion && !ignored) bin = conf_bin(best[k], t[k], K, bad);
                nbad += bad ? 1 : 0;
            }
            if (confusion) hist_add(hist, bin);
        }
        if (in) {
            store_px<PX>(lse_out + p, lse);
            if (pred_out) store_px<PX>(pred_out + p, best);
        }
    }
    double s[1] = {sum};
    long long n[2] = {count, nbad};
    block_sum<1>(s, red_sum);
    block_sum<2>(n, red_cnt);
    if (threadIdx.x == 0) part[blockIdx.x] = SemPart{s[0], n[0], n[1]};
    if (confusion) hist_flush(hist, KK, confusion);                          // (block_sum's barrier orders the LDS adds before the reads)
}

// one block: thread t sums partials t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(SEM_THREADS) void semantic_final_kernel(const SemPart* __restrict__ part, int nblocks, long long* __restrict__ header,
                                                                     float* __restrict__ loss)
{
    __shared__ double ssum[SEM_THREADS];
    __shared__ long long scnt[SEM_THREADS], sbad[SEM_THREADS];
    double sum = 0.0;
    long long cnt = 0, bad = 0;
    for (int b = threadIdx.x; b < nblocks; b += SEM_THREADS) { sum += part[b].sum; cnt += part[b].count; bad += part[b].bad; }
    ssum[threadIdx.x] = sum; scnt[threadIdx.x] = cnt; sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int o = SEM_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { ssum[threadIdx.x] += ssum[threadIdx.x + o]; scnt[threadIdx.x] += scnt[threadIdx.x + o]; sbad[threadIdx.x] += sbad[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        header[0] = scnt[0];
        header[1] = sbad[0];
        *loss = (float)(ssum[0] / (double)scnt[0]);                          // nothing valid: 0 / 0 = NaN, as torch
    }
}

template <int PX>
__global__ __launch_bounds__(SEM_THREADS) void semantic_grad_kernel(const float* __restrict__ logits, const long long* __restrict__ target, int C,
                                                                    size_t HW, size_t npix, long long ignore_index,
                                                                    const long long* __restrict__ header, const float* __restrict__ lse,
                                                                    const float* __restrict__ grad_out, float* __restrict__ grad)
{
    using F = typename Vec<PX>::F;
    const float scale = *grad_out / (float)header[0];
    const size_t step = (size_t)gridDim.x * SEM_THREADS * PX;
    for (size_t p = ((size_t)blockIdx.x * SEM_THREADS + threadIdx.x) * PX; p < npix; p += step) {
        const size_t b = p / HW, i = p - b * HW;
        const size_t off = b * (size_t)C * HW + i;
        long long t[PX];
        float l[PX];
        bool valid[PX];
        load_px<PX>(target + p, t);
        load_px<PX>(lse + p, l);
#pragma unroll
        for (int k = 0; k < PX; ++k) valid[k] = t[k] != ignore_index && t[k] >= 0 && t[k] < (long long)C;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const F w = *reinterpret_cast<const F*>(logits + off + (size_t)c * HW);
            float g[PX];
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const float pr = expf(elem(w, k) - l[k]);
                g[k] = valid[k] ? (pr - (t[k] == (long long)c ? 1.0f : 0.0f)) * scale : 0.0f;
            }
            store_px<PX>(grad + off + (size_t)c * HW, g);
        }
    }
}

__global__ __launch_bounds__(SEM_THREADS) void confusion_kernel(const long long* __restrict__ pred, const long long* __restrict__ gt, size_t n, int K,
                                                                long long* __restrict__ confusion, long long* __restrict__ n_bad)
{
    __shared__ unsigned hist[SEM_MAX_K * SEM_MAX_K];
    __shared__ long long red_bad[1][SEM_THREADS / 64];
    const int KK = K * K;
    for (int i = threadIdx.x; i < KK; i += SEM_THREADS) hist[i] = 0;
    __syncthreads();
    long long nbad[1] = {0};
    const size_t step = (size_t)gridDim.x * SEM_THREADS;
    for (size_t base = (size_t)blockIdx.x * SEM_THREADS; base < n; base += step) {                   // block-uniform
        const size_t p = base + threadIdx.x;
        int bin = -1;
        if (p < n) {
            bool bad = false;
            bin = conf_bin(pred[p], gt[p], K, bad);
            nbad[0] += bad ? 1 : 0;
        }
        hist_add(hist, bin);
    }
    block_sum<1>(nbad, red_bad);                                             // (its barrier also orders the LDS adds before the flush)
    hist_flush(hist, KK, confusion);
    if (threadIdx.x == 0 && n_bad && nbad[0]) atomicAdd(reinterpret_cast<unsigned long long*>(n_bad), (unsigned long long)nbad[0]);
}

// a block's 32-bit bins cannot overflow below 2^32 pixels per block; far above anything a device holds
constexpr size_t SEM_MAX_PIXELS = (size_t)1 << 40;

int sem_check(const char* who, const void* logits, const void* target, int B, int C, size_t HW)
{
    if (!logits || !target) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": null device pointer");
    if (B < 1 || HW < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": empty batch");
    if (C < 2 || C > SEM_MAX_K) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": 2 <= C <= 64 classes are supported, got " + std::to_string(C));
    if (HW >= SEM_MAX_PIXELS || (size_t)B * HW >= SEM_MAX_PIXELS) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 2^40 pixels");
    return OMNI_OK;
}

int sem_blocks(size_t per_block_pixels, size_t npix)
{
    const size_t want = (npix + per_block_pixels - 1) / per_block_pixels;
    size_t cap = (size_t)omni_num_cus() * 4;                                 // four blocks per CU: 16 waves, and few flushes into one matrix
    if (cap < 1) cap = 1;
    if (cap > (size_t)SEM_MAX_BLOCKS) cap = SEM_MAX_BLOCKS;
    return (int)(want < cap ? want : cap);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" size_t omni_semantic_workspace_bytes(size_t npix) { return sem_lse_offset() + sizeof(float) * npix; }

extern "C" int omni_semantic_step_f32(const float* logits, const int64_t* target, int B, int C, size_t HW, int64_t ignore_index, int K,
                                      void* workspace, float* loss, int64_t* pred, int64_t* confusion, omni_stream_t stream)
{
    if (const int rc = sem_check("omni_semantic_step_f32", logits, target, B, C, HW)) return rc;
    if (!workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_semantic_step_f32: null workspace or loss pointer");
    if (K == 0) K = C;
    if (K < C || K > SEM_MAX_K) OMNI_FAIL(OMNI_ERR_INVALID, "omni_semantic_step_f32: C <= K <= 64 required (argmax yields every class index below C)");
    const size_t npix = (size_t)B * HW;
    char* ws = (char*)workspace;
    long long* header = (long long*)ws;
    SemPart* part = (SemPart*)(ws + SEM_HEADER);
    float* lse = (float*)(ws + sem_lse_offset());
    hipStream_t s = (hipStream_t)stream;
    const bool wide = HW % 4 == 0 && aligned16(logits) && aligned16(target) && aligned16(workspace) && (!pred || aligned16(pred));
    const int blocks = sem_blocks((size_t)SEM_THREADS * (wide ? 4 : 1), npix);
    if (wide)
        hipLaunchKernelGGL(semantic_step_kernel<4>, dim3(blocks), dim3(SEM_THREADS), 0, s, logits, (const long long*)target, C, HW, npix,
                           (long long)ignore_index, K, part, lse, (long long*)pred, (long long*)confusion);
    else
        hipLaunchKernelGGL(semantic_step_kernel<1>, dim3(blocks), dim3(SEM_THREADS), 0, s, logits, (const long long*)target, C, HW, npix,
                           (long long)ignore_index, K, part, lse, (long long*)pred, (long long*)confusion);
    hipLaunchKernelGGL(semantic_final_kernel, dim3(1), dim3(SEM_THREADS), 0, s, (const SemPart*)part, blocks, header, loss);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_semantic_grad_f32(const float* logits, const int64_t* target, int B, int C, size_t HW, int64_t ignore_index,
                                      const void* workspace, const float* grad_out, float* grad_logits, omni_stream_t stream)
{
    if (const int rc = sem_check("omni_semantic_grad_f32", logits, target, B, C, HW)) return rc;
    if (!workspace || !grad_out || !grad_logits) OMNI_FAIL(OMNI_ERR_INVALID, "omni_semantic_grad_f32: null device pointer");
    const size_t npix = (size_t)B * HW;
    const char* ws = (const char*)workspace;
    const long long* header = (const long long*)ws;
    const float* lse = (const float*)(ws + sem_lse_offset());
    const bool wide = HW % 4 == 0 && aligned16(logits) && aligned16(target) && aligned16(workspace) && aligned16(grad_logits);
    const int blocks = sem_blocks((size_t)SEM_THREADS * (wide ? 4 : 1), npix);
    hipStream_t s = (hipStream_t)stream;
    if (wide)
        hipLaunchKernelGGL(semantic_grad_kernel<4>, dim3(blocks), dim3(SEM_THREADS), 0, s, logits, (const long long*)target, C, HW, npix,
                           (long long)ignore_index, header, lse, grad_out, grad_logits);
    else
        hipLaunchKernelGGL(semantic_grad_kernel<1>, dim3(blocks), dim3(SEM_THREADS), 0, s, logits, (const long long*)target, C, HW, npix,
                           (long long)ignore_index, header, lse, grad_out, grad_logits);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_confusion_matrix_i64(const int64_t* pred, const int64_t* gt, size_t n, int K, int64_t* confusion, int64_t* n_bad,
                                         omni_stream_t stream)
{
    if (!pred || !gt || !confusion) OMNI_FAIL(OMNI_ERR_INVALID, "omni_confusion_matrix_i64: null device pointer");
    if (K < 1 || K > SEM_MAX_K) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_confusion_matrix_i64: 1 <= K <= 64 classes are supported, got " + std::to_string(K));
    if (n >= SEM_MAX_PIXELS) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_confusion_matrix_i64: more than 2^40 pixels");
    if (n == 0) return OMNI_OK;
    const int blocks = sem_blocks(SEM_THREADS, n);
    hipLaunchKernelGGL(confusion_kernel, dim3(blocks), dim3(SEM_THREADS), 0, (hipStream_t)stream, (const long long*)pred, (const long long*)gt, n, K,
                       (long long*)confusion, (long long*)n_bad);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
