// omni_losses.hip — the device side of supervision/direct.py: the two masked-mean losses of the depth objective (train_erp_depth.py:267-275)
// and their gradients w.r.t. the prediction.  gfx950 only.
//
//   omni_berhu_loss_f32 / _grad_f32   supervision/direct.py:3-18 calculate_berhu_loss, c = max|gt - pred| / 5 kept on the device
//   omni_l1_loss_f32 / _grad_f32      supervision/direct.py:20-26 calculate_l1_loss
//
// Both are loss = mean_b(sum_b / count_b): per item, up to 256 blocks each store one double partial pair (fixed block -> slot mapping, the
// block's own sum by omni_reduce.h), and ONE final kernel adds the slots serially.  No atomics in the sums: the bits do not change from run to
// run.  This is "the BerHu scheme" the photometric, semantic and geometry units refer to.
#include "omni_normals.h"   // geo::sign0
#include "omni_reduce.h"

namespace {

constexpr int MM_MAX_BLOCKS = 256;                                           // partial slots per item
constexpr int MM_MAX_B = 65535;                                              // gridDim.y
constexpr size_t BERHU_HEADER = 64;                                          // the bits of max|gt - pred| in front of the partials

// workspace of a masked mean: `header` bytes | double part[B][MM_MAX_BLOCKS][2] (sum, count) | float counts[B] (kept for the gradient)
struct MaskedMeanWs {
    double* part; float* counts;
    MaskedMeanWs(const void* ws, int B, size_t header)
        : part((double*)((char*)ws + header)), counts((float*)(part + 2 * MM_MAX_BLOCKS * (size_t)B)) {}
    static size_t bytes(int B, size_t header) { const size_t b = B > 0 ? B : 1; return header + sizeof(double) * 2 * MM_MAX_BLOCKS * b + sizeof(float) * b; }
};

inline unsigned mm_blocks(size_t per_item) { const size_t want = (per_item + 255) / 256; return (unsigned)(want < (size_t)MM_MAX_BLOCKS ? want : (size_t)MM_MAX_BLOCKS); }

__device__ __forceinline__ void store_partial(double* __restrict__ part, int b, const double (&s)[2])
{
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        p[0] = s[0]; p[1] = s[1];
    }
}

// loss = mean_b(sum_b / count_b) (:18, :26); counts[b] kept for the gradient.  One thread, slots in index order.
__global__ void masked_mean_final_kernel(const double* __restrict__ part, int B, int nblk, float* __restrict__ loss, float* __restrict__ counts)
{
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0, c = 0.0;
        for (int k = 0; k < nblk; ++k) { s += part[((size_t)b * nblk + k) * 2]; c += part[((size_t)b * nblk + k) * 2 + 1]; }
        counts[b] = (float)c;
        tot += (double)((float)s / (float)c);          // fp32 division like torch (0/0 -> NaN for an empty mask, like the reference)
    }
    *loss = (float)(tot / B);
}

// ------------------------------------------------------------------ BerHu (reverse Huber), supervision/direct.py:3-18
// pass 1: max |gt - pred| over EVERYTHING (:7 — not only the masked elements), non-negative floats order like their bits
__global__ __launch_bounds__(256) void berhu_max_kernel(const float* __restrict__ pred, const float* __restrict__ gt, size_t n, unsigned* __restrict__ maxbits)
{
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(gt[i] - pred[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, __float_as_uint(m));
}

// pass 2: per batch item, partial sums of loss*mask*weight and of mask
__global__ __launch_bounds__(256) void berhu_sum_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                        const float* __restrict__ wt, size_t per, const unsigned* __restrict__ maxbits,
                                                        double* __restrict__ part /* [B][gridDim.x][2] */)
{
    __shared__ double red[2][4];
    const int b = blockIdx.y;
    const float c = __uint_as_float(*maxbits) / 5.0f;                  // :7
    double s[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        const size_t j = (size_t)b * per + i;
        const float d = gt[j] - pred[j], ad = fabsf(d);
        const float l = (ad <= c) ? ad : (d * d + c * c) / (2.0f * c);             // :8-10
        s[0] += (double)(l * mask[j] * wt[j]);                                     // :16-17
        s[1] += (double)mask[j];                                                   // :15
    }
    block_sum<2>(s, red);
    store_partial(part, b, s);
}

// gradient w.r.t. pred (c is a Python float in the reference — `.item()` — hence a constant):
// dL/dpred = -(g / B) * mask * weight / count_b * (|d| <= c ? sign(d) : d / c)
__global__ __launch_bounds__(256) void berhu_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                         const float* __restrict__ wt, size_t per, size_t n, const unsigned* __restrict__ maxbits,
                                                         const float* __restrict__ counts, const float* __restrict__ gout, int B, float* __restrict__ grad)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float c = __uint_as_float(*maxbits) / 5.0f;
    const int b = (int)(j / per);
    const float d = gt[j] - pred[j], ad = fabsf(d);
    const float dl = (ad <= c) ? (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) : d / c;      // d loss / d diff
    grad[j] = -(*gout / (float)B) * (mask[j] * wt[j] / counts[b]) * dl;
}

// ------------------------------------------------------------------ L1, supervision/direct.py:20-26
// part: [B][gridDim.x][2] = sum(|gt - pred| * mask), sum(mask) — the mask summed as it is stored ([B,1,...] once, [B,C,...] C planes)
__global__ __launch_bounds__(256) void l1_sum_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                     int C, size_t hw, int mask_c, double* __restrict__ part)
{
    __shared__ double red[2][4];
    const int b = blockIdx.y;
    const size_t per = (size_t)C * hw;
    double s[2] = {0.0, 0.0};
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const size_t c = e / hw, o = e - c * hw;
        const float m = mask[(size_t)b * mask_c * hw + (mask_c == 1 ? o : e)];
        s[0] += (double)(fabsf(gt[b * per + e] - pred[b * per + e]) * m);
        if (mask_c != 1 || c == 0) s[1] += (double)m;
    }
    block_sum<2>(s, red);
    store_partial(part, b, s);
}

__global__ __launch_bounds__(256) void l1_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                      int B, int C, size_t hw, int mask_c, size_t n, const float* __restrict__ counts,
                                                      const float* __restrict__ gout, float* __restrict__ grad)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const size_t per = (size_t)C * hw, b = p / per, e = p - b * per;
    const float m = mask[b * mask_c * hw + (mask_c == 1 ? e % hw : e)];
    grad[p] = -(*gout / (float)B) * (m / counts[b]) * geo::sign0(gt[p] - pred[p]);
}

int l1_check(const char* who, int B, int C, size_t hw, int mask_c)
{
    if (B < 1 || C < 1 || hw < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": empty batch");
    if (mask_c != 1 && mask_c != C) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": the mask has 1 or C channels");
    if (B > MM_MAX_B) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 items");
    return OMNI_OK;
}

}  // namespace

extern "C" size_t omni_berhu_workspace_bytes(int B) { return MaskedMeanWs::bytes(B, BERHU_HEADER); }

extern "C" int omni_berhu_loss_f32(const float* pred, const float* gt, const float* mask, const float* weights, int B, size_t per_item,
                                   void* workspace, float* loss, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !weights || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_berhu_loss_f32: null device pointer");
    if (B < 1 || per_item < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_berhu_loss_f32: empty batch");
    hipStream_t s = (hipStream_t)stream;
    unsigned* maxbits = (unsigned*)workspace;
    const MaskedMeanWs ws(workspace, B, BERHU_HEADER);
    const size_t n = (size_t)B * per_item;
    OMNI_HIP(hipMemsetAsync(maxbits, 0, sizeof(unsigned), s));
    const unsigned g1 = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(berhu_max_kernel, dim3(g1), dim3(256), 0, s, pred, gt, n, maxbits);
    const unsigned nblk = mm_blocks(per_item);
    hipLaunchKernelGGL(berhu_sum_kernel, dim3(nblk, B), dim3(256), 0, s, pred, gt, mask, weights, per_item, (const unsigned*)maxbits, ws.part);
    hipLaunchKernelGGL(masked_mean_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws.part, B, (int)nblk, loss, ws.counts);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_berhu_grad_f32(const float* pred, const float* gt, const float* mask, const float* weights, int B, size_t per_item,
                                   const void* workspace, const float* grad_out, float* grad_pred, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !weights || !workspace || !grad_out || !grad_pred) OMNI_FAIL(OMNI_ERR_INVALID, "omni_berhu_grad_f32: null device pointer");
    if (B < 1 || per_item < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_berhu_grad_f32: empty batch");
    const unsigned* maxbits = (const unsigned*)workspace;
    const MaskedMeanWs ws(workspace, B, BERHU_HEADER);
    const size_t n = (size_t)B * per_item;
    hipLaunchKernelGGL(berhu_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, gt, mask, weights, per_item, n,
                       maxbits, (const float*)ws.counts, grad_out, B, grad_pred);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_l1_workspace_bytes(int B) { return MaskedMeanWs::bytes(B, 0); }

extern "C" int omni_l1_loss_f32(const float* pred, const float* gt, const float* mask, int B, int C, size_t hw, int mask_c, void* workspace,
                                float* loss, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_l1_loss_f32: null device pointer");
    if (const int rc = l1_check("omni_l1_loss_f32", B, C, hw, mask_c)) return rc;
    const MaskedMeanWs ws(workspace, B, 0);
    const unsigned nblk = mm_blocks((size_t)C * hw);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(l1_sum_kernel, dim3(nblk, B), dim3(256), 0, s, pred, gt, mask, C, hw, mask_c, ws.part);
    hipLaunchKernelGGL(masked_mean_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws.part, B, (int)nblk, loss, ws.counts);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_l1_grad_f32(const float* pred, const float* gt, const float* mask, int B, int C, size_t hw, int mask_c, const void* workspace,
                                const float* grad_out, float* grad_pred, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !workspace || !grad_out || !grad_pred) OMNI_FAIL(OMNI_ERR_INVALID, "omni_l1_grad_f32: null device pointer");
    if (const int rc = l1_check("omni_l1_grad_f32", B, C, hw, mask_c)) return rc;
    const MaskedMeanWs ws(workspace, B, 0);
    const size_t n = (size_t)B * C * hw;
    hipLaunchKernelGGL(l1_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, gt, mask, B, C, hw,
                       mask_c, n, (const float*)ws.counts, grad_out, grad_pred);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
