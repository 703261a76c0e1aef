// omni_smoothness.hip — the guided (edge-aware) smoothness term of the self-supervised objective (supervision/smoothness.py:3-8) and the
// functions it is made of (spherical/derivatives.py:7-24,190-214, spherical/cartesian.py:14-50):
//
//   omni_image_diff_f32               dI_du / dI_dv: t[i,j] - t[i,j+1] / t[i,j] - t[i+1,j] with replicate padding, [B,C,H,W] -> [B,C,H,W]
//   omni_image_diff_norm_f32          dI_duv: the 2-norm over the 2 C difference channels, [B,C,H,W] -> [B,1,H,W]
//   omni_vertex_diff_norm_f32         dV_dxyz: du = |du_x| + |du_y| + |du_z|, dv likewise, sqrt(du^2 + dv^2), [B,3,H,W] -> [B,1,H,W]
//   omni_guided_smoothness_f32        sum(mask ? input_duv exp(-guide_duv) weights : 0) / sum(mask != 0) over precomputed maps, and its gradient
//   omni_depth_smoothness_f32         the same loss of dV_dxyz(coords_3d(sgrid, depth)) and dI_duv(image) from ONE pass over depth, image, mask
//                                     and weights; no vertex, difference or magnitude map is written
//   omni_depth_smoothness_grad_f32    d loss / d depth, one gather kernel
//
// Fused forward: a block owns a 16 x 64 tile.  The vertices of the tile and of one more row and column (replicate padding = clamped
// coordinates, so the last column's du and the last row's dv are x - x = 0) go to LDS; a thread owns four pixels and reads the image, the
// mask and the weights of its pixels directly (the neighbours' image values are L1 hits).  The mask is a SELECT: a masked pixel's term is
// not evaluated at all, so nothing non-finite at such a pixel reaches the sum through that pixel's own term.  Sums go wave -> block -> one
// double pair per (item, tile); a final block adds the pairs in a fixed order and divides.  No atomics: the bits do not change from run to run.
// Backward: the same tile with one more row and column on the other side too.  Phase A recomputes, for every term of the tile and of the row
// above and the column left of it, dL/ddu and dL/ddv into LDS; phase B: a thread per depth pixel adds what its own term, its left
// neighbour's du and its upper neighbour's dv send to it, in that order.  Nothing is scattered.
// Kinks, as torch autograd: d|x|/dx = 0 at 0 (every last-column du, every last-row dv), the gradient of the 2-norm is 0 where the norm is 0
// (the bottom-right pixel).
// Directions come from four host-built maps [4][H][W] = cos phi | sin phi | cos theta | sin theta (no trigonometry here); the products keep
// the reference's order: x = depth cos(phi) (-1) cos(theta), y = depth sin(theta), z = depth sin(phi) cos(theta).
#include "omni_internal.h"
#include "omni_reduce.h"

namespace {

constexpr int ST_W = 64, ST_H = 16, S_THREADS = 256, S_ROWS = S_THREADS / ST_W, S_PX = ST_H / S_ROWS;
constexpr int EW_MAX_BLOCKS = 1024;                                          // of the element-wise loss: its partials depend on n alone

__device__ __forceinline__ float sign0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }      // d|x|/dx, 0 at 0

// Vertices of rows y0 - LO .. y0 + ST_H and columns x0 - LO .. x0 + ST_W (coordinates clamped to the image) into three planes of
// (ST_H + 1 + LO) x (ST_W + 1 + LO) floats
template <int LO>
__device__ __forceinline__ void stage_vertices(const float* __restrict__ depth, const float* __restrict__ fac, int H, int W, int y0, int x0,
                                               float* __restrict__ sx, float* __restrict__ sy, float* __restrict__ sz)
{
    constexpr int SW = ST_W + 1 + LO, SH = ST_H + 1 + LO;
    const size_t hw = (size_t)H * W;
    for (int k = threadIdx.x; k < SH * SW; k += S_THREADS) {
        const int r = k / SW, c = k - r * SW;
        const int y = min(max(y0 - LO + r, 0), H - 1), x = min(max(x0 - LO + c, 0), W - 1);
        const size_t o = (size_t)y * W + x;
        const float d = depth[o], cp = fac[o], sp = fac[hw + o], ct = fac[2 * hw + o], st = fac[3 * hw + o];
        sx[k] = -((d * cp) * ct);
        sy[k] = d * st;
        sz[k] = (d * sp) * ct;
    }
}

// du, dv and their 2-norm at staged position o of planes with row stride sw
__device__ __forceinline__ float vertex_diffs(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int o, int sw,
                                              float& du, float& dv)
{
    du = (fabsf(sx[o] - sx[o + 1]) + fabsf(sy[o] - sy[o + 1])) + fabsf(sz[o] - sz[o + 1]);
    dv = (fabsf(sx[o] - sx[o + sw]) + fabsf(sy[o] - sy[o + sw])) + fabsf(sz[o] - sz[o + sw]);
    return sqrtf(du * du + dv * dv);
}

// dI_duv at pixel (i, j) of one item's image [C][H][W]: the du channels are summed first, then the dv channels
__device__ __forceinline__ float guide_at(const float* __restrict__ img, int C, size_t hw, int i, int j, int H, int W)
{
    const size_t o = (size_t)i * W + j, o_r = (size_t)i * W + min(j + 1, W - 1), o_d = (size_t)min(i + 1, H - 1) * W + j;
    float su = 0.0f, sv = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float* p = img + c * hw;
        const float a = p[o], u = a - p[o_r], v = a - p[o_d];
        su += u * u;
        sv += v * v;
    }
    return sqrtf(su + sv);
}

// ------------------------------------------------------------------ fused forward
// part: [B][ntiles][2] = sum of the terms, number of valid pixels of the tile
template <bool WEIGHTS>
__global__ __launch_bounds__(S_THREADS) void depth_smoothness_kernel(const float* __restrict__ depth, const float* __restrict__ image, const float* __restrict__ mask,
                                                                     const float* __restrict__ weights, const float* __restrict__ fac, int C, int H, int W,
                                                                     int tiles_x, double* __restrict__ part)
{
    constexpr int SW = ST_W + 1, SH = ST_H + 1;
    __shared__ float sx[SH * SW], sy[SH * SW], sz[SH * SW];
    __shared__ double red[2][S_THREADS / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * ST_H, x0 = (tile % tiles_x) * ST_W;
    const size_t hw = (size_t)H * W, plane = (size_t)b * hw;
    stage_vertices<0>(depth + plane, fac, H, W, y0, x0, sx, sy, sz);
    __syncthreads();
    double s[2] = {0.0, 0.0};
    const int tx = threadIdx.x & (ST_W - 1), ty = threadIdx.x / ST_W;
#pragma unroll
    for (int k = 0; k < S_PX; ++k) {
        const int r = ty + k * S_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const size_t p = plane + (size_t)i * W + j;
        if (mask[p] != 0.0f) {
            float du, dv;
            float t = vertex_diffs(sx, sy, sz, r * SW + tx, SW, du, dv) * expf(-guide_at(image + plane * C, C, hw, i, j, H, W));
            if constexpr (WEIGHTS) t *= weights[p];
            s[0] += (double)t;
            s[1] += 1.0;
        }
    }
    block_sum<2>(s, red);
    if (threadIdx.x == 0) {
        double* q = part + ((size_t)b * gridDim.x + tile) * 2;
        q[0] = s[0]; q[1] = s[1];
    }
}

// One block: thread t adds pairs t, t + 256, ... in that order, then the fixed tree.  head[0] = sum(mask != 0) as float32 (what torch.sum(mask)
// becomes in the reference's division), head[1] = the sum of the terms; *loss = head[1] / head[0]: 0 / 0 = NaN for an empty mask.
__global__ __launch_bounds__(S_THREADS) void smoothness_final_kernel(const double* __restrict__ part, size_t nparts, float* __restrict__ head,
                                                                     float* __restrict__ loss)
{
    __shared__ double red[2][S_THREADS / 64];
    double s[2] = {0.0, 0.0};
    for (size_t k = threadIdx.x; k < nparts; k += S_THREADS) {
        s[0] += part[2 * k];
        s[1] += part[2 * k + 1];
    }
    block_sum<2>(s, red);
    if (threadIdx.x == 0) {
        head[0] = (float)s[1];
        head[1] = (float)s[0];
        *loss = (float)s[0] / (float)s[1];
    }
}

// ------------------------------------------------------------------ fused backward
template <bool WEIGHTS>
__global__ __launch_bounds__(S_THREADS) void depth_smoothness_grad_kernel(const float* __restrict__ depth, const float* __restrict__ image, const float* __restrict__ mask,
                                                                          const float* __restrict__ weights, const float* __restrict__ fac, int C, int H, int W,
                                                                          int tiles_x, const float* __restrict__ head, const float* __restrict__ up,
                                                                          float* __restrict__ grad)
{
    constexpr int SW = ST_W + 2, SH = ST_H + 2, AW = ST_W + 1, AH = ST_H + 1;
    __shared__ float sx[SH * SW], sy[SH * SW], sz[SH * SW];                  // origin (y0 - 1, x0 - 1)
    __shared__ float gu[AH * AW], gv[AH * AW];                               // dL/ddu, dL/ddv of the terms, origin (y0 - 1, x0 - 1)
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * ST_H, x0 = (tile % tiles_x) * ST_W;
    const size_t hw = (size_t)H * W, plane = (size_t)b * hw;
    stage_vertices<1>(depth + plane, fac, H, W, y0, x0, sx, sy, sz);
    __syncthreads();
    const float c0 = *up / head[0];
    for (int k = threadIdx.x; k < AH * AW; k += S_THREADS) {
        const int r = k / AW, c = k - r * AW;
        const int i = y0 - 1 + r, j = x0 - 1 + c;
        float a = 0.0f, d = 0.0f;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            const size_t p = plane + (size_t)i * W + j;
            if (mask[p] != 0.0f) {                                           // a masked term sends nothing, whatever its values are
                float du, dv;
                const float mag = vertex_diffs(sx, sy, sz, r * SW + c, SW, du, dv);
                if (mag != 0.0f) {                                           // the 2-norm's gradient is 0 at 0
                    float cq = c0 * expf(-guide_at(image + plane * C, C, hw, i, j, H, W));
                    if constexpr (WEIGHTS) cq *= weights[p];
                    a = cq * (du / mag);
                    d = cq * (dv / mag);
                }
            }
        }
        gu[k] = a; gv[k] = d;
    }
    __syncthreads();
    const int tx = threadIdx.x & (ST_W - 1), ty = threadIdx.x / ST_W;
#pragma unroll
    for (int k = 0; k < S_PX; ++k) {
        const int r = ty + k * S_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const int o = (r + 1) * SW + tx + 1, t = (r + 1) * AW + tx + 1;
        const size_t q = (size_t)i * W + j;
        const float cp = fac[q], sp = fac[hw + q], ct = fac[2 * hw + q], st = fac[3 * hw + q];
        const float fx = -(cp * ct), fy = st, fz = sp * ct;                  // d vertex / d depth of this pixel
        const float x = sx[o], y = sy[o], z = sz[o];
        const float own_u = (sign0(x - sx[o + 1]) * fx + sign0(y - sy[o + 1]) * fy) + sign0(z - sz[o + 1]) * fz;
        const float own_v = (sign0(x - sx[o + SW]) * fx + sign0(y - sy[o + SW]) * fy) + sign0(z - sz[o + SW]) * fz;
        const float left_u = (sign0(sx[o - 1] - x) * fx + sign0(sy[o - 1] - y) * fy) + sign0(sz[o - 1] - z) * fz;
        const float up_v = (sign0(sx[o - SW] - x) * fx + sign0(sy[o - SW] - y) * fy) + sign0(sz[o - SW] - z) * fz;
        grad[plane + q] = ((gu[t] * own_u + gv[t] * own_v) - gu[t - 1] * left_u) - gv[t - AW] * up_v;
    }
}

// ------------------------------------------------------------------ the stand-alone maps
__global__ __launch_bounds__(S_THREADS) void image_diff_kernel(const float* __restrict__ img, size_t n, int H, int W, int axis, float* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (p >= n) return;
    const size_t row = p / W;
    const int j = (int)(p - row * W), i = (int)(row % H);
    const size_t nb = axis == 0 ? (j + 1 < W ? p + 1 : p) : (i + 1 < H ? p + W : p);
    out[p] = img[p] - img[nb];
}

__global__ __launch_bounds__(S_THREADS) void image_diff_norm_kernel(const float* __restrict__ img, size_t n, int C, int H, int W, float* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (p >= n) return;
    const size_t hw = (size_t)H * W, b = p / hw, o = p - b * hw;
    const int i = (int)(o / W), j = (int)(o - (size_t)i * W);
    out[p] = guide_at(img + b * C * hw, C, hw, i, j, H, W);
}

__global__ __launch_bounds__(S_THREADS) void vertex_diff_norm_kernel(const float* __restrict__ pcloud, size_t n, int H, int W, float* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (p >= n) return;
    const size_t hw = (size_t)H * W, b = p / hw, o = p - b * hw;
    const int i = (int)(o / W), j = (int)(o - (size_t)i * W);
    const size_t o_r = j + 1 < W ? o + 1 : o, o_d = i + 1 < H ? o + W : o;
    const float *x = pcloud + b * 3 * hw, *y = x + hw, *z = y + hw;
    const float du = (fabsf(x[o] - x[o_r]) + fabsf(y[o] - y[o_r])) + fabsf(z[o] - z[o_r]);
    const float dv = (fabsf(x[o] - x[o_d]) + fabsf(y[o] - y[o_d])) + fabsf(z[o] - z[o_d]);
    out[p] = sqrtf(du * du + dv * dv);
}

// ------------------------------------------------------------------ the element-wise loss over precomputed maps
__global__ __launch_bounds__(S_THREADS) void guided_smoothness_kernel(const float* __restrict__ input, const float* __restrict__ guide, const float* __restrict__ mask,
                                                                      const float* __restrict__ weights, size_t n, double* __restrict__ part)
{
    __shared__ double red[2][S_THREADS / 64];
    double s[2] = {0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * S_THREADS + threadIdx.x; p < n; p += (size_t)gridDim.x * S_THREADS)
        if (mask[p] != 0.0f) {
            s[0] += (double)((input[p] * expf(-guide[p])) * weights[p]);
            s[1] += 1.0;
        }
    block_sum<2>(s, red);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s[0];
        part[2 * (size_t)blockIdx.x + 1] = s[1];
    }
}

__global__ __launch_bounds__(S_THREADS) void guided_smoothness_grad_kernel(const float* __restrict__ guide, const float* __restrict__ mask, const float* __restrict__ weights,
                                                                           size_t n, const float* __restrict__ head, const float* __restrict__ up,
                                                                           float* __restrict__ grad)
{
    const size_t p = (size_t)blockIdx.x * S_THREADS + threadIdx.x;
    if (p >= n) return;
    grad[p] = mask[p] != 0.0f ? ((*up / head[0]) * expf(-guide[p])) * weights[p] : 0.0f;
}

// ------------------------------------------------------------------ host side
constexpr int SMOOTH_MAX_B = 65535;                                          // gridDim.y
constexpr size_t HEAD_BYTES = 64;                                            // workspace: float head[2], padded | double part[nparts][2]

int smooth_check(const char* who, int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": B, C, H, W >= 1 required");
    if (B > SMOOTH_MAX_B || (size_t)H * W >= ((size_t)1 << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 items or 2^31 pixels per item");
    return OMNI_OK;
}

inline int tiles_x_of(int W) { return (W + ST_W - 1) / ST_W; }
inline int tiles_of(int H, int W) { return tiles_x_of(W) * ((H + ST_H - 1) / ST_H); }
inline bool too_many(size_t n) { return n / S_THREADS >= ((size_t)1 << 31) - 1; }      // one thread per element: gridDim.x
inline unsigned blocks_of(size_t n) { return (unsigned)((n + S_THREADS - 1) / S_THREADS); }
inline unsigned ew_blocks_of(size_t n) { const size_t b = (n + S_THREADS - 1) / S_THREADS; return (unsigned)(b < EW_MAX_BLOCKS ? b : EW_MAX_BLOCKS); }

}  // namespace

extern "C" int omni_image_diff_f32(const float* img, int B, int C, int H, int W, int axis, float* out, omni_stream_t stream)
{
    if (!img || !out) OMNI_FAIL(OMNI_ERR_INVALID, "omni_image_diff_f32: null device pointer");
    if (axis != 0 && axis != 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_image_diff_f32: axis is 0 (du, along a row) or 1 (dv, along a column)");
    if (const int rc = smooth_check("omni_image_diff_f32", B, C, H, W)) return rc;
    const size_t n = (size_t)B * C * H * W;
    if (too_many(n)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_image_diff_f32: more than 2^39 elements");
    hipLaunchKernelGGL(image_diff_kernel, dim3(blocks_of(n)), dim3(S_THREADS), 0, (hipStream_t)stream, img, n, H, W, axis, out);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_image_diff_norm_f32(const float* img, int B, int C, int H, int W, float* out, omni_stream_t stream)
{
    if (!img || !out) OMNI_FAIL(OMNI_ERR_INVALID, "omni_image_diff_norm_f32: null device pointer");
    if (const int rc = smooth_check("omni_image_diff_norm_f32", B, C, H, W)) return rc;
    const size_t n = (size_t)B * H * W;
    if (too_many(n)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_image_diff_norm_f32: more than 2^39 elements");
    hipLaunchKernelGGL(image_diff_norm_kernel, dim3(blocks_of(n)), dim3(S_THREADS), 0, (hipStream_t)stream, img, n, C, H, W, out);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_vertex_diff_norm_f32(const float* pcloud, int B, int H, int W, float* out, omni_stream_t stream)
{
    if (!pcloud || !out) OMNI_FAIL(OMNI_ERR_INVALID, "omni_vertex_diff_norm_f32: null device pointer");
    if (const int rc = smooth_check("omni_vertex_diff_norm_f32", B, 3, H, W)) return rc;
    const size_t n = (size_t)B * H * W;
    if (too_many(n)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_vertex_diff_norm_f32: more than 2^39 elements");
    hipLaunchKernelGGL(vertex_diff_norm_kernel, dim3(blocks_of(n)), dim3(S_THREADS), 0, (hipStream_t)stream, pcloud, n, H, W, out);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_guided_smoothness_workspace_bytes(size_t n)
{
    if (n < 1) return 0;
    return HEAD_BYTES + sizeof(double) * 2 * (size_t)ew_blocks_of(n);
}

extern "C" int omni_guided_smoothness_f32(const float* input_duv, const float* guide_duv, const float* mask, const float* weights, size_t n,
                                          void* workspace, float* loss, omni_stream_t stream)
{
    if (!input_duv || !guide_duv || !mask || !weights || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_guided_smoothness_f32: null device pointer");
    if (n < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_guided_smoothness_f32: no elements");
    float* head = (float*)workspace;
    double* part = (double*)((char*)workspace + HEAD_BYTES);
    const unsigned nb = ew_blocks_of(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(guided_smoothness_kernel, dim3(nb), dim3(S_THREADS), 0, s, input_duv, guide_duv, mask, weights, n, part);
    hipLaunchKernelGGL(smoothness_final_kernel, dim3(1), dim3(S_THREADS), 0, s, (const double*)part, (size_t)nb, head, loss);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_guided_smoothness_grad_f32(const float* guide_duv, const float* mask, const float* weights, size_t n, const void* workspace,
                                               const float* grad_out, float* grad_input, omni_stream_t stream)
{
    if (!guide_duv || !mask || !weights || !workspace || !grad_out || !grad_input) OMNI_FAIL(OMNI_ERR_INVALID, "omni_guided_smoothness_grad_f32: null device pointer");
    if (n < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_guided_smoothness_grad_f32: no elements");
    if (too_many(n)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_guided_smoothness_grad_f32: more than 2^39 elements");
    hipLaunchKernelGGL(guided_smoothness_grad_kernel, dim3(blocks_of(n)), dim3(S_THREADS), 0, (hipStream_t)stream, guide_duv, mask, weights, n,
                       (const float*)workspace, grad_out, grad_input);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_depth_smoothness_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return 0;
    return HEAD_BYTES + sizeof(double) * 2 * (size_t)B * tiles_of(H, W);
}

extern "C" int omni_depth_smoothness_f32(const float* depth, const float* image, const float* mask, const float* weights, const float* factors, int B,
                                         int C, int H, int W, void* workspace, float* loss, omni_stream_t stream)
{
    if (!depth || !image || !mask || !factors || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_smoothness_f32: null device pointer");
    if (const int rc = smooth_check("omni_depth_smoothness_f32", B, C, H, W)) return rc;
    float* head = (float*)workspace;
    double* part = (double*)((char*)workspace + HEAD_BYTES);
    const int ntiles = tiles_of(H, W), tx = tiles_x_of(W);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ntiles, B), block(S_THREADS);
    if (weights) hipLaunchKernelGGL((depth_smoothness_kernel<true>), grid, block, 0, s, depth, image, mask, weights, factors, C, H, W, tx, part);
    else hipLaunchKernelGGL((depth_smoothness_kernel<false>), grid, block, 0, s, depth, image, mask, weights, factors, C, H, W, tx, part);
    hipLaunchKernelGGL(smoothness_final_kernel, dim3(1), block, 0, s, (const double*)part, (size_t)B * ntiles, head, loss);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_depth_smoothness_grad_f32(const float* depth, const float* image, const float* mask, const float* weights, const float* factors,
                                              int B, int C, int H, int W, const void* workspace, const float* grad_out, float* grad_depth,
                                              omni_stream_t stream)
{
    if (!depth || !image || !mask || !factors || !workspace || !grad_out || !grad_depth) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_smoothness_grad_f32: null device pointer");
    if (const int rc = smooth_check("omni_depth_smoothness_grad_f32", B, C, H, W)) return rc;
    const float* head = (const float*)workspace;
    const int ntiles = tiles_of(H, W), tx = tiles_x_of(W);
    const dim3 grid(ntiles, B), block(S_THREADS);
    if (weights) hipLaunchKernelGGL((depth_smoothness_grad_kernel<true>), grid, block, 0, (hipStream_t)stream, depth, image, mask, weights, factors, C, H, W, tx, head, grad_out, grad_depth);
    else hipLaunchKernelGGL((depth_smoothness_grad_kernel<false>), grid, block, 0, (hipStream_t)stream, depth, image, mask, weights, factors, C, H, W, tx, head, grad_out, grad_depth);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
