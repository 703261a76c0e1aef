// omni_freeview.hip — free-view sampling: perspective views of a panorama at any yaw / pitch / field of view, and back.
//
// Mirrors the reference's equi_pers/equi2pers_torch.py:37 `equi2pers` and equi_pers/pers2equi_torch.py:37 `pers2equi`, which build a
// sampling grid with per-pixel asin / atan2 / rotations on every call and hand it to F.grid_sample (bilinear, zeros, align_corners=True).
// Here the coordinates of a (view, pixel) are computed once by the thread that owns four consecutive output pixels and reused for all the
// image planes it loops over; no grid and no per-view intermediate is ever written.  freeview_merge_kernel (no reference counterpart)
// averages N views onto one ERP with the same per-(view, pixel) device function as freeview_p2e_kernel.
//
// The two 3x3 rotations of a view depend on (theta, phi) only: omni_freeview_rotations evaluates the reference's quaternion form
// (`rotation_matrix`, equi2pers_torch.py:12-34) on the host in double and rounds once; the kernels read them from a device table.  The launch
// functions allocate nothing, copy nothing and never synchronise: they can be captured on a single stream.  fp32 only.
#include <math.h>

#include "omni_internal.h"
#include "omni_freeview_taps.h"   // the tap-set device functions, shared with omni_freeview_bwd.hip

namespace {

constexpr int FV_MERGE_PLANES = 4;       // image planes a merge thread accumulates at once (16 accumulators)

// the summation order of every sample in this file
__device__ __forceinline__ float fv_sample(const float* __restrict__ plane, const FvTap& t)
{
    return ((plane[t.o00] * t.w00 + plane[t.o01] * t.w01) + plane[t.o10] * t.w10) + plane[t.o11] * t.w11;
}

// ---------------------------------------------------------------------------------------------------------------- ERP -> views
// erp [planes = B * C][H][W] -> pers: planar [B][N][C][h][w] (concat == 0) or the reference's [B][C][h][N * w] (concat == 1).
// One thread: FV_PX consecutive pixels of one row of one view; planes blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ __launch_bounds__(FV_BLOCK) void freeview_e2p_kernel(const float* __restrict__ erp, float* __restrict__ pers, const float* __restrict__ rot,
                                                                  int C, int planes, int H, int W, int N, int h, int w, int groups, int total,
                                                                  float h_len, float w_len, int concat)
{
    const int t = blockIdx.x * FV_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int g = t % groups, i = (t / groups) % h, v = t / (groups * h);
    const int j0 = g * FV_PX, n = min(FV_PX, w - j0);
    const float* r = rot + (size_t)v * 9;
    FvTap tap[FV_PX];
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) tap[k] = fv_e2p_tap(r, h_len, w_len, h, w, i, min(j0 + k, w - 1), H, W);
    const size_t HW = (size_t)H * W;
    const bool vec = (w & 3) == 0;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        const float* src = erp + (size_t)p * HW;
        const int b = p / C, c = p - b * C;
        float* dst = concat ? pers + ((size_t)p * h + i) * ((size_t)N * w) + (size_t)v * w + j0
                            : pers + ((((size_t)b * N + v) * C + c) * h + i) * (size_t)w + j0;
        float o[FV_PX];
#pragma unroll
        for (int k = 0; k < FV_PX; ++k) o[k] = fv_sample(src, tap[k]);
        if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < FV_PX; ++k)
                if (k < n) dst[k] = o[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- views -> ERP
// pers [N][C][h][w] -> erp [N][C][H][W] (zero outside the view) and mask [N][1][H][W] (uint8).  One thread: FV_PX consecutive ERP pixels of one view.
__global__ __launch_bounds__(FV_BLOCK) void freeview_p2e_kernel(const float* __restrict__ pers, float* __restrict__ erp, unsigned char* __restrict__ mask,
                                                                  const float* __restrict__ rot_inv, int C, int h, int w, int H, int W, int groups, int total,
                                                                  float h_len, float w_len)
{
    const int t = blockIdx.x * FV_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int g = t % groups, row = (t / groups) % H, v = t / (groups * H);
    const int c0 = g * FV_PX, n = min(FV_PX, W - c0);
    const float* ri = rot_inv + (size_t)v * 18;
    FvTap tap[FV_PX];
    bool in[FV_PX];
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) {
        tap[k] = FvTap{0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
        in[k] = fv_p2e_tap(ri, fv_erp_ray(H, W, row, min(c0 + k, W - 1)), h_len, w_len, h, w, tap[k]);
    }
    const bool vec = (W & 3) == 0;
    const size_t hw = (size_t)h * w, HW = (size_t)H * W, at = (size_t)row * W + c0;
    unsigned char* m = mask + (size_t)v * HW + at;
    if (vec) {
        *reinterpret_cast<uchar4*>(m) = make_uchar4(in[0], in[1], in[2], in[3]);
    } else {
#pragma unroll
        for (int k = 0; k < FV_PX; ++k)
            if (k < n) m[k] = in[k];
    }
    for (int c = 0; c < C; ++c) {
        const float* src = pers + ((size_t)v * C + c) * hw;
        float* dst = erp + ((size_t)v * C + c) * HW + at;
        float o[FV_PX];
#pragma unroll
        for (int k = 0; k < FV_PX; ++k) o[k] = in[k] ? fv_sample(src, tap[k]) : 0.0f;
        if (vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < FV_PX; ++k)
                if (k < n) dst[k] = o[k];
        }
    }
}

// pers [B][N][C][h][w] -> erp [B * C][H][W] = sum_v sample_v * mask_v / max(sum_v mask_v, 1), views in index order; count [H][W] = sum_v mask_v.
// One thread: FV_PX consecutive ERP pixels x FV_MERGE_PLANES planes (blockIdx.y: the plane chunk); the N intermediates are never written.
__global__ __launch_bounds__(FV_BLOCK) void freeview_merge_kernel(const float* __restrict__ pers, float* __restrict__ erp, unsigned char* __restrict__ count,
                                                                    const float* __restrict__ rot_inv, int N, int C, int planes, int h, int w, int H, int W,
                                                                    int groups, int total, float h_len, float w_len)
{
    const int t = blockIdx.x * FV_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int g = t % groups, row = t / groups;
    const int c0 = g * FV_PX, n = min(FV_PX, W - c0);
    const int p0 = blockIdx.y * FV_MERGE_PLANES, np = min(FV_MERGE_PLANES, planes - p0);
    FvRay q[FV_PX];
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) q[k] = fv_erp_ray(H, W, row, min(c0 + k, W - 1));
    const size_t hw = (size_t)h * w, HW = (size_t)H * W, at = (size_t)row * W + c0;
    const float* src[FV_MERGE_PLANES];
#pragma unroll
    for (int j = 0; j < FV_MERGE_PLANES; ++j) {
        const int p = min(p0 + j, planes - 1), b = p / C, c = p - b * C;
        src[j] = pers + ((size_t)b * N * C + c) * hw;               // view 0 of plane (b, c); view v is v * C * hw further
    }
    float acc[FV_MERGE_PLANES][FV_PX];
    int cnt[FV_PX];
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) {
        cnt[k] = 0;
#pragma unroll
        for (int j = 0; j < FV_MERGE_PLANES; ++j) acc[j][k] = 0.0f;
    }
    for (int v = 0; v < N; ++v) {
        const float* ri = rot_inv + (size_t)v * 18;
        const size_t vo = (size_t)v * C * hw;
#pragma unroll
        for (int k = 0; k < FV_PX; ++k) {
            FvTap tap;
            if (fv_p2e_tap(ri, q[k], h_len, w_len, h, w, tap)) {
                ++cnt[k];
#pragma unroll
                for (int j = 0; j < FV_MERGE_PLANES; ++j)
                    if (j < np) acc[j][k] += fv_sample(src[j] + vo, tap);
            }
        }
    }
    const bool vec = (W & 3) == 0;
    if (blockIdx.y == 0) {
        unsigned char* m = count + at;
        if (vec) {
            *reinterpret_cast<uchar4*>(m) = make_uchar4(cnt[0], cnt[1], cnt[2], cnt[3]);
        } else {
#pragma unroll
            for (int k = 0; k < FV_PX; ++k)
                if (k < n) m[k] = (unsigned char)cnt[k];
        }
    }
#pragma unroll
    for (int j = 0; j < FV_MERGE_PLANES; ++j) {
        if (j < np) {
            float* dst = erp + (size_t)(p0 + j) * HW + at;
            float o[FV_PX];
#pragma unroll
            for (int k = 0; k < FV_PX; ++k) o[k] = acc[j][k] / (float)max(cnt[k], 1);
            if (vec) {
                *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int k = 0; k < FV_PX; ++k)
                    if (k < n) dst[k] = o[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// `rotation_matrix` of the reference (equi2pers_torch.py:12-34) in double: the quaternion (a, b, c, d) = (cos(t / 2), -axis sin(t / 2)).
void fv_rotation(double theta, const double axis_in[3], double m[9])
{
    const double nrm = sqrt(axis_in[0] * axis_in[0] + axis_in[1] * axis_in[1] + axis_in[2] * axis_in[2]);
    const double s = nrm > 1e-12 ? 1.0 / nrm : 1.0 / 1e-12;        // F.normalize's eps
    const double a = cos(theta / 2.0), sn = sin(theta / 2.0);
    const double b = -axis_in[0] * s * sn, c = -axis_in[1] * s * sn, d = -axis_in[2] * s * sn;
    const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const double bc = b * c, ad = a * d, ac = a * c, ab = a * b, bd = b * d, cd = c * d;
    m[0] = aa + bb - cc - dd; m[1] = 2 * (bc + ad);     m[2] = 2 * (bd - ac);
    m[3] = 2 * (bc - ad);     m[4] = aa + cc - bb - dd; m[5] = 2 * (cd + ab);
    m[6] = 2 * (bd + ac);     m[7] = 2 * (cd - ab);     m[8] = aa + dd - bb - cc;
}

}  // namespace

extern "C" int omni_freeview_rotations(const float* theta_deg, const float* phi_deg, int N, float* rot_fwd_host, float* rot_inv_host)
{
    if (!theta_deg || !phi_deg) OMNI_FAIL(OMNI_ERR_INVALID, "omni_freeview_rotations: null angle pointer");
    if (!rot_fwd_host && !rot_inv_host) OMNI_FAIL(OMNI_ERR_INVALID, "omni_freeview_rotations: no output requested");
    if (N < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_freeview_rotations: N must be >= 1");
    const double rad = 3.14159265358979323846 / 180.0;
    for (int v = 0; v < N; ++v) {
        if (!(fabsf(theta_deg[v]) <= 3.402823466e38f) || !(fabsf(phi_deg[v]) <= 3.402823466e38f))
            OMNI_FAIL(OMNI_ERR_INVALID, "omni_freeview_rotations: theta and phi must be finite");
        const double zaxis[3] = {0.0, 0.0, 1.0};
        double r1[9], r2[9];
        fv_rotation((double)theta_deg[v] * rad, zaxis, r1);
        const double axis2[3] = {r1[1], r1[4], r1[7]};             // R1 . (0, 1, 0)
        fv_rotation(-(double)phi_deg[v] * rad, axis2, r2);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                if (rot_fwd_host) {
                    double acc = 0.0;
                    for (int k = 0; k < 3; ++k) acc += r2[i * 3 + k] * r1[k * 3 + j];
                    rot_fwd_host[(size_t)v * 9 + i * 3 + j] = (float)acc;
                }
                if (rot_inv_host) {                                 // rotations: the inverse is the transpose
                    rot_inv_host[(size_t)v * 18 + i * 3 + j] = (float)r2[j * 3 + i];
                    rot_inv_host[(size_t)v * 18 + 9 + i * 3 + j] = (float)r1[j * 3 + i];
                }
            }
    }
    return OMNI_OK;
}

extern "C" int omni_freeview_equi2pers_f32(const float* erp, float* pers, const float* rot_fwd_dev, int B, int C, int H, int W, int N, int h, int w,
                                           float hfov_deg, float wfov_deg, int layout, omni_stream_t stream)
{
    const char* what = "omni_freeview_equi2pers_f32";
    if (!erp || !pers || !rot_fwd_dev) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": B must be >= 1");
    if (layout != OMNI_LAYOUT_BNCHW && layout != OMNI_LAYOUT_BCHNW) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": layout must be OMNI_LAYOUT_BNCHW or OMNI_LAYOUT_BCHNW");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, h, w, N, s)) return e;
    if ((long long)B * C > (1ll << 24)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": too many image planes");
    if ((uintptr_t)pers & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": pers must be 16-byte aligned");
    const int planes = B * C, blocks = (s.total + FV_BLOCK - 1) / FV_BLOCK;
    // small views: spread the planes over blockIdx.y until the launch has ~1024 blocks (each thread then recomputes its coordinates per plane range)
    int gy = blocks >= 1024 ? 1 : (1024 + blocks - 1) / blocks;
    if (gy > planes) gy = planes;
    hipLaunchKernelGGL(freeview_e2p_kernel, dim3(blocks, gy), dim3(FV_BLOCK), 0, (hipStream_t)stream, erp, pers, rot_fwd_dev, C, planes, H, W, N, h, w,
                       s.groups, s.total, s.h_len, s.w_len, layout == OMNI_LAYOUT_BCHNW ? 1 : 0);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_freeview_pers2equi_f32(const float* pers, float* erp, unsigned char* mask, const float* rot_inv_dev, int N, int C, int h, int w,
                                           int H, int W, float hfov_deg, float wfov_deg, omni_stream_t stream)
{
    const char* what = "omni_freeview_pers2equi_f32";
    if (!pers || !erp || !mask || !rot_inv_dev) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, H, W, N, s)) return e;
    if (((uintptr_t)erp & 15) || ((uintptr_t)mask & 3)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": erp must be 16-byte and mask 4-byte aligned");
    hipLaunchKernelGGL(freeview_p2e_kernel, dim3((s.total + FV_BLOCK - 1) / FV_BLOCK), dim3(FV_BLOCK), 0, (hipStream_t)stream, pers, erp, mask, rot_inv_dev,
                       C, h, w, H, W, s.groups, s.total, s.h_len, s.w_len);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_freeview_merge_f32(const float* pers, float* erp, unsigned char* count, const float* rot_inv_dev, int B, int N, int C, int h, int w,
                                       int H, int W, float hfov_deg, float wfov_deg, omni_stream_t stream)
{
    const char* what = "omni_freeview_merge_f32";
    if (!pers || !erp || !count || !rot_inv_dev) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": B must be >= 1");
    if (N > 255) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": at most 255 views (count is uint8)");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, H, W, 1, s)) return e;
    if ((long long)B * C > 65535ll * FV_MERGE_PLANES) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": too many image planes");
    if (((uintptr_t)erp & 15) || ((uintptr_t)count & 3)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": erp must be 16-byte and count 4-byte aligned");
    const int planes = B * C;
    hipLaunchKernelGGL(freeview_merge_kernel, dim3((s.total + FV_BLOCK - 1) / FV_BLOCK, (planes + FV_MERGE_PLANES - 1) / FV_MERGE_PLANES), dim3(FV_BLOCK), 0,
                       (hipStream_t)stream, pers, erp, count, rot_inv_dev, N, C, planes, h, w, H, W, s.groups, s.total, s.h_len, s.w_len);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
