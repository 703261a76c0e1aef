// omni_normals.hip — the two geometry terms of the depth objective (train_erp_depth.py:267-275: loss = berhu + 0.2 normal_loss + 0.05 grad_loss)
// and the functions they are made of:
//
//   omni_depth_normals_f32            util.py:332-382 depth2normal_gpu: depth [B,1,H,W] -> unit normals [B,3,H,W]
//   omni_sobel_f32                    util.py:426-446 imgrad: channel mean, then the two 3x3 Sobel maps [B,1,H,W]
//   omni_geometry_terms_f32           normal_loss = 1 - mean_b(sum_b(pn gn mask) / sum(mask)) and grad_loss = calculate_l1_loss(imgrad_yx(pred),
//                                     imgrad_yx(gt), mask) from ONE pass over pred, gt and mask; no normal or Sobel map is written
//   omni_geometry_terms_grad_f32      d(g_n normal_loss + g_g grad_loss) / d pred, one gather kernel
//
// Forward: a block owns a 16 x 64 tile; pred, gt and mask are staged in LDS with a one-pixel halo (16-byte loads of the interior where the
// rows are aligned, scalar loads of the halo columns), a thread owns four pixels.  Sums go wave -> block -> one double partial per (item,
// tile); a final block adds them in a fixed order (the BerHu scheme of omni_losses.hip).  No atomics: the bits do not change from run to run.
// Backward: the same tile with a two-pixel halo.  Phase A recomputes, for the tile and a one-pixel ring around it, what each pixel q sends
// to the five depths its normal read and the two Sobel adjoints, into LDS; phase B: a thread per output pixel gathers from its own entry
// and its neighbours'.  Nothing is scattered, nothing is stored by the forward but the mask sums.
// Per-pixel arithmetic: omni_normals.h, shared with the two mirrors.  Rays come from four host-built tables (no trigonometry here).
#include "omni_normals.h"
#include "omni_reduce.h"

namespace {

using geo::V3;

constexpr int GT_W = 64, GT_H = 16, G_THREADS = 256, G_ROWS = G_THREADS / GT_W, G_PX = GT_H / G_ROWS;
constexpr int TERM_NORMAL = 1, TERM_GRAD = 2;

// Rows y0 - HALO .. y0 + GT_H + HALO, columns x0 - HALO .. x0 + GT_W + HALO of one H x W plane into lds[(GT_H + 2 HALO)][(GT_W + 2 HALO)];
// `fill` outside the image.  vec: W % 4 == 0 and the plane is 16-byte aligned, so every aligned group of four columns is inside or outside.
template <int HALO>
__device__ __forceinline__ void stage(const float* __restrict__ plane, int H, int W, int y0, int x0, bool vec, float fill, float* __restrict__ lds)
{
    constexpr int SW = GT_W + 2 * HALO, SH = GT_H + 2 * HALO;
    if (vec) {
        for (int k = threadIdx.x; k < SH * (GT_W / 4); k += G_THREADS) {
            const int r = k / (GT_W / 4), c = 4 * (k % (GT_W / 4));
            const int y = y0 - HALO + r, x = x0 + c;
            float4 v = make_float4(fill, fill, fill, fill);
            if (y >= 0 && y < H && x < W) v = *reinterpret_cast<const float4*>(plane + (size_t)y * W + x);
            float* d = lds + r * SW + HALO + c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        for (int k = threadIdx.x; k < SH * GT_W; k += G_THREADS) {
            const int r = k / GT_W, c = k % GT_W;
            const int y = y0 - HALO + r, x = x0 + c;
            lds[r * SW + HALO + c] = (y >= 0 && y < H && x < W) ? plane[(size_t)y * W + x] : fill;
        }
    }
    for (int k = threadIdx.x; k < SH * 2 * HALO; k += G_THREADS) {
        const int r = k / (2 * HALO), h = k % (2 * HALO);
        const int c = h < HALO ? h : GT_W + h;                               // staged column: the left halo, then the right one
        const int y = y0 - HALO + r, x = x0 - HALO + c;
        lds[r * SW + c] = (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : fill;
    }
}

struct TileAt {                                                              // accessor of omni_normals.h over a staged tile
    const float* p; int sw;
    __device__ __forceinline__ float operator()(int di, int dj) const { return p[di * sw + dj]; }
};

// ------------------------------------------------------------------ fused forward
// part: [B][ntiles][3] = sum(pn . gn * m), sum(m), sum((|dgy| + |dgx|) * m) of the tile
template <bool NORMAL, bool GRAD>
__global__ __launch_bounds__(G_THREADS) void geometry_terms_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                                   const float* __restrict__ tab, int H, int W, int tiles_x, int erode, int vec,
                                                                   double* __restrict__ part)
{
    constexpr int SW = GT_W + 2, SH = GT_H + 2;
    __shared__ float sp[SH * SW], sg[SH * SW], sm[SH * SW];
    __shared__ double red[3][G_THREADS / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * GT_H, x0 = (tile % tiles_x) * GT_W;
    const size_t plane = (size_t)b * H * W;
    stage<1>(pred + plane, H, W, y0, x0, vec != 0, 0.0f, sp);
    stage<1>(gt + plane, H, W, y0, x0, vec != 0, 0.0f, sg);
    stage<1>(mask + plane, H, W, y0, x0, vec != 0, 1.0f, sm);
    __syncthreads();
    const geo::Rays rays = geo::rays_of(tab, H, W);
    double s[3] = {0.0, 0.0, 0.0};
    const int tx = threadIdx.x & (GT_W - 1), ty = threadIdx.x / GT_W;
#pragma unroll
    for (int k = 0; k < G_PX; ++k) {
        const int r = ty + k * G_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const int o = (r + 1) * SW + tx + 1;
        const float m = geo::mask_at(TileAt{sm + o, SW}, erode != 0);
        s[1] += (double)m;
        if constexpr (NORMAL) {
            geo::Normal np, ng;
            geo::normal_at(TileAt{sp + o, SW}, rays, i, j, H, W, np);
            geo::normal_at(TileAt{sg + o, SW}, rays, i, j, H, W, ng);
            s[0] += ((double)(np.out.x * ng.out.x * m) + (double)(np.out.y * ng.out.y * m)) + (double)(np.out.z * ng.out.z * m);
        }
        if constexpr (GRAD) {
            float py, px, gy, gx;
            geo::sobel_at(TileAt{sp + o, SW}, py, px);
            geo::sobel_at(TileAt{sg + o, SW}, gy, gx);
            s[2] += (double)(fabsf(gy - py) * m) + (double)(fabsf(gx - px) * m);
        }
    }
    block_sum<3>(s, red);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)b * gridDim.x + tile) * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    }
}

// One block.  Per item: thread t adds partials t, t + 256, ... in that order, then the fixed tree.  head[0] = sum(mask) of the batch,
// head[1 + b] = sum(mask) of item b (float32, as `count` in the reference); losses[0] = normal_loss, losses[1] = grad_loss.
// An empty mask divides 0 by 0: NaN, as masked_mean_final_kernel.
__global__ __launch_bounds__(G_THREADS) void geometry_final_kernel(const double* __restrict__ part, int B, int ntiles, float* __restrict__ head,
                                                                   float* __restrict__ losses)
{
    __shared__ double red[3][G_THREADS / 64];
    double total = 0.0, grad_tot = 0.0, normal_sum = 0.0;
    for (int b = 0; b < B; ++b) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int k = threadIdx.x; k < ntiles; k += G_THREADS) {
            const double* p = part + ((size_t)b * ntiles + k) * 3;
            s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
        }
        __syncthreads();                                                     // (red is reused per item)
        block_sum<3>(s, red);
        if (threadIdx.x == 0) {
            head[1 + b] = (float)s[1];
            total += s[1];
            grad_tot += (double)((float)s[2] / (float)s[1]);
            head[1 + B + b] = (float)s[0];                                   // divided by the batch's mask sum below, once it is known
        }
    }
    if (threadIdx.x == 0) {
        const float M = (float)total;
        for (int b = 0; b < B; ++b) normal_sum += (double)(head[1 + B + b] / M);
        head[0] = M;
        losses[0] = 1.0f - (float)(normal_sum / B);
        losses[1] = (float)(grad_tot / B);
    }
}

// ------------------------------------------------------------------ fused backward
// adj: per pixel q of the tile and its one-pixel ring, [0..4] what q's normal sends to itself and its right / lower / left / upper neighbour,
// [5], [6] dL/dgrad_y(q), dL/dgrad_x(q)
template <bool NORMAL, bool GRAD>
__global__ __launch_bounds__(G_THREADS) void geometry_terms_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                                        const float* __restrict__ tab, int B, int H, int W, int tiles_x, int erode, int vec,
                                                                        const float* __restrict__ head, const float* __restrict__ up_normal,
                                                                        const float* __restrict__ up_grad, float* __restrict__ grad)
{
    constexpr int SW = GT_W + 4, SH = GT_H + 4, AW = GT_W + 2, AH = GT_H + 2, NA = (NORMAL ? 5 : 0) + (GRAD ? 2 : 0), GO = NORMAL ? 5 : 0;
    __shared__ float sp[SH * SW], sg[SH * SW], sm[SH * SW];
    __shared__ float adj[NA][AH * AW];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * GT_H, x0 = (tile % tiles_x) * GT_W;
    const size_t plane = (size_t)b * H * W;
    stage<2>(pred + plane, H, W, y0, x0, vec != 0, 0.0f, sp);
    stage<2>(gt + plane, H, W, y0, x0, vec != 0, 0.0f, sg);
    stage<2>(mask + plane, H, W, y0, x0, vec != 0, 1.0f, sm);
    __syncthreads();
    const geo::Rays rays = geo::rays_of(tab, H, W);
    // normal_loss = 1 - (1 / B) sum(pn . gn m) / M;  grad_loss = (1 / B) sum_b sum(|gt' - pred'| m) / count_b
    float cn = 0.0f, cg = 0.0f;
    if constexpr (NORMAL) cn = -(*up_normal / (float)B);
    if constexpr (GRAD) cg = -(*up_grad / (float)B);
    const float M = head[0], count = head[1 + b];
    for (int k = threadIdx.x; k < AH * AW; k += G_THREADS) {
        const int r = k / AW, c = k % AW;
        const int i = y0 - 1 + r, j = x0 - 1 + c;
        const bool in = i >= 0 && i < H && j >= 0 && j < W;
        const int o = (r + 1) * SW + c + 1;
        float m = 0.0f;
        if (in) m = geo::mask_at(TileAt{sm + o, SW}, erode != 0);
        if constexpr (NORMAL) {
            float d[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (in) {
                geo::Normal np, ng;
                geo::normal_at(TileAt{sg + o, SW}, rays, i, j, H, W, ng);
                geo::normal_at(TileAt{sp + o, SW}, rays, i, j, H, W, np);
                geo::normal_bwd(np, rays, i, j, ng.out * (cn * (m / M)), d);
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) adj[q][k] = d[q];
        }
        if constexpr (GRAD) {
            float wy = 0.0f, wx = 0.0f;
            if (in) {
                float py, px, gy, gx;
                geo::sobel_at(TileAt{sp + o, SW}, py, px);
                geo::sobel_at(TileAt{sg + o, SW}, gy, gx);
                const float w = cg * (m / count);
                wy = w * geo::sign0(gy - py);
                wx = w * geo::sign0(gx - px);
            }
            adj[GO][k] = wy; adj[GO + 1][k] = wx;
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & (GT_W - 1), ty = threadIdx.x / GT_W;
#pragma unroll
    for (int k = 0; k < G_PX; ++k) {
        const int r = ty + k * G_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const int o = (r + 1) * AW + tx + 1;
        float g = 0.0f;
        if constexpr (NORMAL)       // own term, then what the left / upper / right / lower neighbour sends to its right / lower / left / upper one
            g = (((adj[0][o] + adj[1][o - 1]) + adj[2][o - AW]) + adj[3][o + 1]) + adj[4][o + AW];
        if constexpr (GRAD) {
            const float t = geo::sobel_bwd_at(TileAt{adj[GO] + o, AW}, TileAt{adj[GO + 1] + o, AW});
            g = NORMAL ? g + t : t;
        }
        grad[plane + (size_t)i * W + j] = g;
    }
}

// ------------------------------------------------------------------ the mirrors
struct PlaneAt {                                                             // accessor over one plane in global memory, `fill` outside
    const float* p; int i, j, H, W;
    __device__ __forceinline__ float operator()(int di, int dj) const
    {
        const int y = i + di, x = j + dj;
        return (y >= 0 && y < H && x >= 0 && x < W) ? p[(size_t)y * W + x] : 0.0f;
    }
};
struct MeanAt {                                                              // torch.mean(img, 1): the channel sum in index order, divided by C
    const float* p; int C, i, j, H, W;
    __device__ __forceinline__ float operator()(int di, int dj) const
    {
        const int y = i + di, x = j + dj;
        if (y < 0 || y >= H || x < 0 || x >= W) return 0.0f;
        const size_t hw = (size_t)H * W, o = (size_t)y * W + x;
        float s = p[o];
        for (int c = 1; c < C; ++c) s += p[c * hw + o];
        return C == 1 ? s : s / (float)C;
    }
};

__global__ __launch_bounds__(G_THREADS) void depth_normals_kernel(const float* __restrict__ depth, const float* __restrict__ tab, size_t n, int H, int W,
                                                                  float* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * G_THREADS + threadIdx.x;
    if (p >= n) return;
    const size_t hw = (size_t)H * W, b = p / hw, o = p - b * hw;
    const int i = (int)(o / W), j = (int)(o - (size_t)i * W);
    geo::Normal f;
    geo::normal_at(PlaneAt{depth + b * hw, i, j, H, W}, geo::rays_of(tab, H, W), i, j, H, W, f);
    float* q = out + b * 3 * hw + o;
    q[0] = f.out.x; q[hw] = f.out.y; q[2 * hw] = f.out.z;
}

__global__ __launch_bounds__(G_THREADS) void sobel_kernel(const float* __restrict__ img, size_t n, int C, int H, int W, float* __restrict__ grad_y,
                                                          float* __restrict__ grad_x)
{
    const size_t p = (size_t)blockIdx.x * G_THREADS + threadIdx.x;
    if (p >= n) return;
    const size_t hw = (size_t)H * W, b = p / hw, o = p - b * hw;
    const int i = (int)(o / W), j = (int)(o - (size_t)i * W);
    float gy, gx;
    geo::sobel_at(MeanAt{img + b * C * hw, C, i, j, H, W}, gy, gx);
    grad_y[p] = gy; grad_x[p] = gx;
}

// ------------------------------------------------------------------ host side
constexpr int GEO_MAX_B = 65535;                                             // gridDim.y

int geo_check(const char* who, int B, int H, int W)
{
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": empty batch");
    if (H < 2 || W < 2) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": H, W >= 2 required, got " + std::to_string(H) + " x " + std::to_string(W));
    if (B > GEO_MAX_B || (size_t)H * W >= ((size_t)1 << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 items or 2^31 pixels per item");
    return OMNI_OK;
}

inline int tiles_x_of(int W) { return (W + GT_W - 1) / GT_W; }
inline int tiles_of(int H, int W) { return tiles_x_of(W) * ((H + GT_H - 1) / GT_H); }
// workspace: float head[1 + 2 B] (batch mask sum, per-item mask sums, per-item normal sums), padded to 64 bytes | double part[B][ntiles][3]
inline size_t head_bytes(int B) { return ((sizeof(float) * (1 + 2 * (size_t)B) + 63) / 64) * 64; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool can_vec(int W, const void* a, const void* b, const void* c) { return W % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(c); }

}  // namespace

extern "C" int omni_depth_normals_f32(const float* depth, const float* ray_tables, int B, int H, int W, float* normals, omni_stream_t stream)
{
    if (!depth || !ray_tables || !normals) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_normals_f32: null device pointer");
    if (const int rc = geo_check("omni_depth_normals_f32", B, H, W)) return rc;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)((n + G_THREADS - 1) / G_THREADS)), dim3(G_THREADS), 0, (hipStream_t)stream, depth, ray_tables, n, H, W, normals);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_sobel_f32(const float* img, int B, int C, int H, int W, float* grad_y, float* grad_x, omni_stream_t stream)
{
    if (!img || !grad_y || !grad_x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_sobel_f32: null device pointer");
    if (C < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_sobel_f32: C >= 1 required");
    if (const int rc = geo_check("omni_sobel_f32", B, H, W)) return rc;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(sobel_kernel, dim3((unsigned)((n + G_THREADS - 1) / G_THREADS)), dim3(G_THREADS), 0, (hipStream_t)stream, img, n, C, H, W, grad_y, grad_x);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_geometry_terms_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 2 || W < 2) return 0;
    return head_bytes(B) + sizeof(double) * 3 * (size_t)B * tiles_of(H, W);
}

extern "C" int omni_geometry_terms_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W, int terms,
                                       int erode_mask, void* workspace, float* losses, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !ray_tables || !workspace || !losses) OMNI_FAIL(OMNI_ERR_INVALID, "omni_geometry_terms_f32: null device pointer");
    if (const int rc = geo_check("omni_geometry_terms_f32", B, H, W)) return rc;
    if (terms < 1 || terms > (TERM_NORMAL | TERM_GRAD)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_geometry_terms_f32: terms is 1 (normal), 2 (gradient) or 3 (both)");
    float* head = (float*)workspace;
    double* part = (double*)((char*)workspace + head_bytes(B));
    const int ntiles = tiles_of(H, W), tx = tiles_x_of(W), vec = can_vec(W, pred, gt, mask) ? 1 : 0, er = erode_mask ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ntiles, B), block(G_THREADS);
    if (terms == (TERM_NORMAL | TERM_GRAD)) hipLaunchKernelGGL((geometry_terms_kernel<true, true>), grid, block, 0, s, pred, gt, mask, ray_tables, H, W, tx, er, vec, part);
    else if (terms == TERM_NORMAL) hipLaunchKernelGGL((geometry_terms_kernel<true, false>), grid, block, 0, s, pred, gt, mask, ray_tables, H, W, tx, er, vec, part);
    else hipLaunchKernelGGL((geometry_terms_kernel<false, true>), grid, block, 0, s, pred, gt, mask, ray_tables, H, W, tx, er, vec, part);
    hipLaunchKernelGGL(geometry_final_kernel, dim3(1), block, 0, s, (const double*)part, B, ntiles, head, losses);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_geometry_terms_grad_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W,
                                            int erode_mask, const void* workspace, const float* grad_normal, const float* grad_grad, float* grad_pred,
                                            omni_stream_t stream)
{
    if (!pred || !gt || !mask || !ray_tables || !workspace || !grad_pred) OMNI_FAIL(OMNI_ERR_INVALID, "omni_geometry_terms_grad_f32: null device pointer");
    if (!grad_normal && !grad_grad) OMNI_FAIL(OMNI_ERR_INVALID, "omni_geometry_terms_grad_f32: no upstream gradient");
    if (const int rc = geo_check("omni_geometry_terms_grad_f32", B, H, W)) return rc;
    const float* head = (const float*)workspace;
    const int ntiles = tiles_of(H, W), tx = tiles_x_of(W), vec = can_vec(W, pred, gt, mask) ? 1 : 0, er = erode_mask ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ntiles, B), block(G_THREADS);
    if (grad_normal && grad_grad)
        hipLaunchKernelGGL((geometry_terms_grad_kernel<true, true>), grid, block, 0, s, pred, gt, mask, ray_tables, B, H, W, tx, er, vec, head, grad_normal, grad_grad, grad_pred);
    else if (grad_normal)
        hipLaunchKernelGGL((geometry_terms_grad_kernel<true, false>), grid, block, 0, s, pred, gt, mask, ray_tables, B, H, W, tx, er, vec, head, grad_normal, grad_grad, grad_pred);
    else
        hipLaunchKernelGGL((geometry_terms_grad_kernel<false, true>), grid, block, 0, s, pred, gt, mask, ray_tables, B, H, W, tx, er, vec, head, grad_normal, grad_grad, grad_pred);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
