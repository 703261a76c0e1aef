// omni_freeview_taps.h — the tap set of a free-view sample: which four pixels a (view, pixel) reads and with which weights.
//
// One copy for omni_freeview.hip (the gathers) and omni_freeview_bwd.hip (their transposes): forward and backward agree on every corner,
// weight and mask bit by construction, as dibr_source<> does for §11.  fp32, in the reference's operation order.
#pragma once
#include <math.h>
#include <string>

#include "omni_internal.h"

namespace {

constexpr int FV_BLOCK = 256;
constexpr int FV_PX = 4;                 // consecutive output pixels per thread: one 16-byte store per plane
constexpr float FV_PI = 3.14159265358979323846f;

// torch.linspace(start, end, steps)[i] in float32: symmetric about the middle (the second half counts down from `end`)
__device__ __forceinline__ float fv_linspace(float start, float end, int steps, int i)
{
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? start + step * (float)i : end - step * (float)(steps - 1 - i);
}

// One bilinear tap set of F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True): four clamped offsets into a plane and
// four weights, zero where the corner is off the image (or the coordinate is not finite: every comparison fails).
struct FvTap {
    int o00, o01, o10, o11;
    float w00, w01, w10, w11;
    int valid;                           // bit k: corner k (00, 01, 10, 11) is on the image (its weight may still be 0); the backward's poison rule
};

__device__ __forceinline__ FvTap fv_tap(float ix, float iy, int H, int W)
{
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float fx = ix - x0, fy = iy - y0;
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
    const float xm = (float)(W - 1), ym = (float)(H - 1);
    const bool vx0 = x0 >= 0.0f && x0 <= xm, vx1 = x1 >= 0.0f && x1 <= xm;
    const bool vy0 = y0 >= 0.0f && y0 <= ym, vy1 = y1 >= 0.0f && y1 <= ym;
    const int cx0 = vx0 ? (int)x0 : 0, cx1 = vx1 ? (int)x1 : 0;
    const int cy0 = vy0 ? (int)y0 : 0, cy1 = vy1 ? (int)y1 : 0;
    FvTap t;
    t.o00 = cy0 * W + cx0; t.o01 = cy0 * W + cx1; t.o10 = cy1 * W + cx0; t.o11 = cy1 * W + cx1;
    t.w00 = (vx0 && vy0) ? (1.0f - fx) * (1.0f - fy) : 0.0f;
    t.w01 = (vx1 && vy0) ? fx * (1.0f - fy) : 0.0f;
    t.w10 = (vx0 && vy1) ? (1.0f - fx) * fy : 0.0f;
    t.w11 = (vx1 && vy1) ? fx * fy : 0.0f;
    t.valid = (vx0 && vy0 ? 1 : 0) | (vx1 && vy0 ? 2 : 0) | (vx0 && vy1 ? 4 : 0) | (vx1 && vy1 ? 8 : 0);
    return t;
}

// grid_sample's un-normalisation of the reference's normalised coordinate (p / size - 0.5) * 2, align_corners=True
__device__ __forceinline__ float fv_unnormalise(float p, int size)
{
    const float g = (p / (float)size - 0.5f) * 2.0f;
    return (g + 1.0f) * 0.5f * (float)(size - 1);
}

// ---------------------------------------------------------------------------------------------------------------- ERP -> views
// equi2pers_torch.py:51-93 for pixel (i, j) of a view whose forward rotation R2.R1 is r[9] -> the tap set into an H x W ERP plane.
__device__ __forceinline__ FvTap fv_e2p_tap(const float* __restrict__ r, float h_len, float w_len, int h, int w, int i, int j, int H, int W)
{
    const float y = fv_linspace(-w_len, w_len, w, j);
    const float z = -fv_linspace(-h_len, h_len, h, i);
    const float d = sqrtf((1.0f + y * y) + z * z);
    const float px = 1.0f / d, py = y / d, pz = z / d;
    const float rx = (r[0] * px + r[1] * py) + r[2] * pz;
    const float ry = (r[3] * px + r[4] * py) + r[5] * pz;
    const float rz = (r[6] * px + r[7] * py) + r[8] * pz;
    const float lat = asinf(fminf(fmaxf(rz, -1.0f), 1.0f));       // |rz| can exceed 1 by an ulp (the reference's asin would return NaN there)
    const float lon = atan2f(ry, rx);
    const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
    const float u = lon / FV_PI * cx + cx;                         // (lon / pi * 180) / 180 * cx + cx
    const float v = -lat / (FV_PI * 0.5f) * cy + cy;               // (-lat / pi * 180) / 90 * cy + cy
    return fv_tap(fv_unnormalise(u, W), fv_unnormalise(v, H), H, W);
}

// ---------------------------------------------------------------------------------------------------------------- views -> ERP
// The unit ray of ERP pixel (row, col): pers2equi_torch.py:42-45 (linspace in degrees, deg2rad, sin / cos).
struct FvRay { float x, y, z; };

__device__ __forceinline__ FvRay fv_erp_ray(int H, int W, int row, int col)
{
    const float k = FV_PI / 180.0f;
    const float lat = fv_linspace(90.0f, -90.0f, H, row) * k, lon = fv_linspace(-180.0f, 180.0f, W, col) * k;
    const float cl = cosf(lat);
    FvRay q;
    q.x = cosf(lon) * cl; q.y = sinf(lon) * cl; q.z = sinf(lat);
    return q;
}

// THE per-(view, pixel) sample of pers2equi_torch.py:57-73, shared by freeview_p2e_kernel and freeview_merge_kernel: rotate the ERP ray by
// R2^-1 (ri[0..8]) then R1^-1 (ri[9..17]), divide by x, test the frustum (all strict; a non-finite y / x or z / x fails it) and x > 0.
// fv_p2e_frustum: the mask bit alone, and the frustum coordinates (y / x, z / x) it was decided on.
__device__ __forceinline__ bool fv_p2e_frustum(const float* __restrict__ ri, const FvRay& q, float h_len, float w_len, float& y, float& z)
{
    const float ax = (ri[0] * q.x + ri[1] * q.y) + ri[2] * q.z;
    const float ay = (ri[3] * q.x + ri[4] * q.y) + ri[5] * q.z;
    const float az = (ri[6] * q.x + ri[7] * q.y) + ri[8] * q.z;
    const float bx = (ri[9] * ax + ri[10] * ay) + ri[11] * az;
    const float by = (ri[12] * ax + ri[13] * ay) + ri[14] * az;
    const float bz = (ri[15] * ax + ri[16] * ay) + ri[17] * az;
    y = by / bx; z = bz / bx;
    return (-w_len < y) && (y < w_len) && (-h_len < z) && (z < h_len) && (bx > 0.0f);
}

// Returns whether the view covers the pixel; if so `tap` addresses an h x w view plane.
__device__ __forceinline__ bool fv_p2e_tap(const float* __restrict__ ri, const FvRay& q, float h_len, float w_len, int h, int w, FvTap& tap)
{
    float y, z;
    if (!fv_p2e_frustum(ri, q, h_len, w_len, y, z)) return false;
    const float u = (y + w_len) / 2.0f / w_len * (float)w;
    const float v = (-z + h_len) / 2.0f / h_len * (float)h;
    tap = fv_tap(fv_unnormalise(u, w), fv_unnormalise(v, h), h, w);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- host
// The argument checks and the launch shape that the forward launches and their backwards share (kept beside the tap set so that the two
// translation units cannot drift apart on what they accept).
struct FvShape { int groups, total; float h_len, w_len; };

// the checks common to the three launches; (oh, ow): the output image whose rows the threads tile
inline int fv_check(const char* what, int N, int C, int h, int w, int H, int W, float hfov, float wfov, int oh, int ow, long long images, FvShape& s)
{
    if (N < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": N must be >= 1");
    if (C < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": C must be >= 1");
    if (h < 2 || w < 2) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": a view needs h >= 2 and w >= 2");
    if (H < 2 || W < 2) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": the ERP needs H >= 2 and W >= 2");
    if (!(hfov > 0.0f && hfov < 180.0f) || !(wfov > 0.0f && wfov < 180.0f))
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": hFOV and wFOV must lie in (0, 180) degrees");
    if ((long long)H * W > (1ll << 30) || (long long)h * w > (1ll << 30)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": image too large");
    s.groups = (ow + FV_PX - 1) / FV_PX;
    const long long total = images * oh * s.groups;
    if (total > (1ll << 31) - FV_BLOCK) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": too many output pixels for one launch");
    s.total = (int)total;
    const double rad = 3.14159265358979323846 / 180.0;
    s.h_len = (float)tan(hfov * 0.5 * rad);
    s.w_len = (float)tan(wfov * 0.5 * rad);
    return OMNI_OK;
}

}  // namespace
