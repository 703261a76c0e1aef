// omni_photometric.hip — the photometric loss of view synthesis (SSIM + L1), forward and backward, gfx950 only.
//
//   omni_ssim_f32                supervision/ssim.py:86-90 `ssim_loss`: the SSIM map, 'gaussian' (:23-63, zero-padded depthwise window) or
//                                'box' (:65-84, valid average, the map zero-padded)
//   omni_photometric_loss_f32    supervision/photometric.py:34-51 `calculate_loss`: mean_b( sum_chw( (alpha d_ssim + (1 - alpha) l1) mask
//                                weights ) / sum(mask) ), d_ssim = clamp((1 - ssim) / 2, 0, 1), on pred * mask and gt * mask
//   omni_photometric_grad_f32    its gradient w.r.t. pred
//
// Forward: a block takes a 16 x 32 tile of one (item, channel) plane, stages masked pred and gt with a halo of window / 2 in LDS once
// (zeros beyond the image: the reference's zero padding), runs the window separably — rows, then columns — over the five moments
// x, y, x^2, y^2, xy, and forms SSIM, d_ssim, L1 and the weighted loss in registers.  No map is written (omni_ssim_f32 apart).
// The window sums and SSIM run in fp64: sigma^2 = E[x^2] - mu^2 cancels against C2 = 9e-4, where fp32 sums leave ~1e-4 relative.
// The per-item sum is two-stage with a fixed block -> slot mapping (the BerHu scheme of omni_losses.hip): deterministic, no atomics, the
// scalar stays on the device.
//
// Backward w.r.t. pred: the window is symmetric and the padding zero, so the adjoint of a window sum is the same window sum.
//   pass 1 recomputes the moments (same code as the forward) and writes, per pixel, P1 = g ds/dmu_x, P2 = g ds/dE[x^2], P3 = g ds/dE[xy]
//          (g carries the loss weights and the clamp's gate; ds/dmu_x is total: through sigma_x^2 and sigma_xy as well)
//   pass 2 windows the three planes and combines  mask * (win P1 + 2 x win P2 + y win P3) + the L1 term.
// 'box': P is zero on the border ring (the map there is the constant 0), which is all the valid-only adjoint needs.
#include "omni_internal.h"
#include "omni_reduce.h"

namespace {

constexpr int PT_H = 16, PT_W = 32, PR_MAX = 5, PS_H = PT_H + 2 * PR_MAX, PS_W = PT_W + 2 * PR_MAX;
constexpr double SSIM_C1 = 0.0001, SSIM_C2 = 0.0009;               // 0.01^2, 0.03^2 (ssim.py:39-40)

struct PhotoArgs {
    const float *pred, *gt, *mask, *wts;                            // mask / wts: nullable (ssim map), [B,mask_c,H,W] / [B,wts_c,H,W]
    int mask_c, wts_c, B, C, H, W, r, box;
    float win[2 * PR_MAX + 1];                                      // the 1-D window (fp32 values, as the reference builds it)
    double alpha;
};

__device__ __forceinline__ float mask_at(const PhotoArgs& a, int b, int c, size_t HW, size_t p)
{
    return a.mask ? a.mask[((size_t)b * a.mask_c + (a.mask_c == 1 ? 0 : c)) * HW + p] : 1.0f;
}

// Stage the masked tile + halo of pred and gt; zero beyond the image.
__device__ __forceinline__ void stage_xy(const PhotoArgs& a, int b, int c, int y0, int x0, float* xs, float* ys)
{
    const int SW = PT_W + 2 * a.r, SH = PT_H + 2 * a.r;
    const size_t HW = (size_t)a.H * a.W, base = ((size_t)b * a.C + c) * HW;
    for (int e = threadIdx.x; e < SH * SW; e += 256) {
        const int sy = e / SW, sx = e - sy * SW, gy = y0 - a.r + sy, gx = x0 - a.r + sx;
        float x = 0.0f, y = 0.0f;
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            const size_t p = (size_t)gy * a.W + gx;
            const float m = mask_at(a, b, c, HW, p);
            x = a.pred[base + p] * m;
            y = a.gt[base + p] * m;
        }
        xs[e] = x; ys[e] = y;
    }
}

// Row pass: hm[m][row][col] = sum_k win[k] * moment_m(row, col + k) for the PT_H + 2 r staged rows
__device__ __forceinline__ void rows_xy(const PhotoArgs& a, const double* wd, const float* xs, const float* ys, double* hm)
{
    const int SW = PT_W + 2 * a.r, SH = PT_H + 2 * a.r, K = 2 * a.r + 1;
    for (int e = threadIdx.x; e < SH * PT_W; e += 256) {
        const int row = e / PT_W, col = e - row * PT_W;
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) {
            const double w = wd[k], x = (double)xs[row * SW + col + k], y = (double)ys[row * SW + col + k];
            s[0] += w * x; s[1] += w * y; s[2] += w * (x * x); s[3] += w * (y * y); s[4] += w * (x * y);
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) hm[(size_t)m * PS_H * PT_W + e] = s[m];
    }
}

template <int N>
__device__ __forceinline__ void cols(const double* wd, const double* hm, int r, int row, int col, double* out)
{
#pragma unroll
    for (int m = 0; m < N; ++m) out[m] = 0.0;
    for (int k = 0; k <= 2 * r; ++k) {
        const double w = wd[k];
#pragma unroll
        for (int m = 0; m < N; ++m) out[m] += w * hm[(size_t)m * PS_H * PT_W + (row + k) * PT_W + col];
    }
}

struct Ssim { double s, dmx, dexx, dexy; };                         // the map and ds/dmu_x (total), ds/dE[x^2], ds/dE[xy]

__device__ __forceinline__ Ssim ssim_of(const double* mo, bool grad)
{
    const double mx = mo[0], my = mo[1];
    const double sxx = mo[2] - mx * mx, syy = mo[3] - my * my, sxy = mo[4] - mx * my;
    const double a1 = 2.0 * (mx * my) + SSIM_C1, a2 = 2.0 * sxy + SSIM_C2, b1 = mx * mx + my * my + SSIM_C1, b2 = sxx + syy + SSIM_C2;
    Ssim o;
    o.s = (a1 * a2) / (b1 * b2);
    o.dmx = o.dexx = o.dexy = 0.0;
    if (grad) {
        o.dexx = -o.s / b2;
        o.dexy = 2.0 * a1 / (b1 * b2);
        o.dmx = 2.0 * my * a2 / (b1 * b2) - 2.0 * mx * o.s / b1 - 2.0 * mx * o.dexx - my * o.dexy;
    }
    return o;
}

__device__ __forceinline__ bool box_interior(const PhotoArgs& a, int y, int x)
{
    return y >= a.r && y < a.H - a.r && x >= a.r && x < a.W - a.r;
}

// MODE 0: loss partials (and / or the SSIM map); MODE 1: backward pass 1 (the three P planes)
template <int MODE>
__global__ __launch_bounds__(256) void photo_kernel(PhotoArgs a, int tiles_x, double* __restrict__ part /* [B][nblk][2] */,
                                                    float* __restrict__ ssim_map, const float* __restrict__ counts, const float* __restrict__ gout,
                                                    float* __restrict__ P /* [3][B][C][H][W] */)
{
    __shared__ float xs[PS_H * PS_W], ys[PS_H * PS_W];
    __shared__ double hm[5 * PS_H * PT_W];
    __shared__ double wd[2 * PR_MAX + 1];
    __shared__ double red[2][4];
    const int b = blockIdx.z, c = blockIdx.y;
    const int x0 = (int)(blockIdx.x % tiles_x) * PT_W, y0 = (int)(blockIdx.x / tiles_x) * PT_H;
    const size_t HW = (size_t)a.H * a.W, plane = ((size_t)b * a.C + c) * HW, n = (size_t)a.B * a.C * HW;
    if (threadIdx.x <= 2 * a.r) wd[threadIdx.x] = a.box ? 1.0 / (double)(2 * a.r + 1) : (double)a.win[threadIdx.x];   // box: the exact 1/k (a float32 1/3 leaves 1.5e-8 in sigma^2)
    stage_xy(a, b, c, y0, x0, xs, ys);
    __syncthreads();
    rows_xy(a, wd, xs, ys, hm);
    __syncthreads();
    const int SW = PT_W + 2 * a.r;
    double sum[2] = {0.0, 0.0};                                     // loss, mask
    for (int e = threadIdx.x; e < PT_H * PT_W; e += 256) {
        const int row = e / PT_W, col = e - row * PT_W, y = y0 + row, x = x0 + col;
        if (y >= a.H || x >= a.W) continue;
        const size_t p = (size_t)y * a.W + x;
        double mo[5];
        cols<5>(wd, hm, a.r, row, col, mo);
        Ssim s = ssim_of(mo, MODE == 1);
        const bool live = !a.box || box_interior(a, y, x);
        if (!live) s.s = 0.0;
        const double h = (1.0 - s.s) * 0.5;
        const float m = mask_at(a, b, c, HW, p);
        const float wt = a.wts ? a.wts[((size_t)b * a.wts_c + (a.wts_c == 1 ? 0 : c)) * HW + p] : 1.0f;
        if (MODE == 0) {
            if (ssim_map) ssim_map[plane + p] = (float)s.s;
            if (part) {
                const double dss = h < 0.0 ? 0.0 : (h > 1.0 ? 1.0 : h);             // NaN stays NaN, like torch.clamp
                const double l1 = (double)fabsf(ys[(row + a.r) * SW + col + a.r] - xs[(row + a.r) * SW + col + a.r]);
                sum[0] += ((a.alpha * dss + (1.0 - a.alpha) * l1) * (double)m) * (double)wt;
                if (a.mask_c != 1 || c == 0) sum[1] += (double)m;
            }
        } else {
            // d loss / d ssim at this pixel: (gout / B) / count_b * weights * mask * alpha * (-1/2) inside the clamp, 0 outside
            const double g = (double)(*gout / (float)a.B) / (double)counts[b] * (double)wt * (double)m;
            const double gs = (live && h >= 0.0 && h <= 1.0) ? g * a.alpha * -0.5 : 0.0;
            P[plane + p] = (float)(gs * s.dmx);
            P[n + plane + p] = (float)(gs * s.dexx);
            P[2 * n + plane + p] = (float)(gs * s.dexy);
        }
    }
    if (MODE == 0 && part) {
        block_sum<2>(sum, red);
        if (threadIdx.x == 0) {
            double* o = part + ((size_t)b * (gridDim.x * gridDim.y) + (size_t)c * gridDim.x + blockIdx.x) * 2;
            o[0] = sum[0]; o[1] = sum[1];
        }
    }
}

// Stage 2 of the sum: one block; per item, 256 strided partial sums in a fixed order, then a fixed tree.  loss = mean_b(sum_b / count_b).
__global__ __launch_bounds__(256) void photo_final_kernel(const double* __restrict__ part, int B, int nblk, float* __restrict__ loss,
                                                          float* __restrict__ counts)
{
    __shared__ double red[2][256];
    double tot = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0, c = 0.0;
        for (int k = threadIdx.x; k < nblk; k += 256) { s += part[((size_t)b * nblk + k) * 2]; c += part[((size_t)b * nblk + k) * 2 + 1]; }
        red[0][threadIdx.x] = s; red[1][threadIdx.x] = c;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            counts[b] = (float)red[1][0];
            tot += (double)((float)red[0][0] / (float)red[1][0]);    // fp32 division like torch (an empty mask gives NaN, like the reference)
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(tot / B);
}

// Backward pass 2: window the three P planes (zero beyond the image) and combine.
__global__ __launch_bounds__(256) void photo_grad_kernel(PhotoArgs a, int tiles_x, const float* __restrict__ P, const float* __restrict__ counts,
                                                         const float* __restrict__ gout, float* __restrict__ grad)
{
    __shared__ float ps[3 * PS_H * PS_W];
    __shared__ double hm[3 * PS_H * PT_W];
    __shared__ double wd[2 * PR_MAX + 1];
    const int b = blockIdx.z, c = blockIdx.y;
    const int x0 = (int)(blockIdx.x % tiles_x) * PT_W, y0 = (int)(blockIdx.x / tiles_x) * PT_H;
    const size_t HW = (size_t)a.H * a.W, plane = ((size_t)b * a.C + c) * HW, n = (size_t)a.B * a.C * HW;
    const int SW = PT_W + 2 * a.r, SH = PT_H + 2 * a.r, K = 2 * a.r + 1;
    if (threadIdx.x <= 2 * a.r) wd[threadIdx.x] = a.box ? 1.0 / (double)(2 * a.r + 1) : (double)a.win[threadIdx.x];   // box: the exact 1/k (a float32 1/3 leaves 1.5e-8 in sigma^2)
    for (int e = threadIdx.x; e < SH * SW; e += 256) {
        const int sy = e / SW, sx = e - sy * SW, gy = y0 - a.r + sy, gx = x0 - a.r + sx;
        const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        const size_t p = in ? plane + (size_t)gy * a.W + gx : 0;
#pragma unroll
        for (int m = 0; m < 3; ++m) ps[m * PS_H * PS_W + e] = in ? P[(size_t)m * n + p] : 0.0f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SH * PT_W; e += 256) {
        const int row = e / PT_W, col = e - row * PT_W;
        double s[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < K; ++k) {
            const double w = wd[k];
#pragma unroll
            for (int m = 0; m < 3; ++m) s[m] += w * (double)ps[m * PS_H * PS_W + row * SW + col + k];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) hm[(size_t)m * PS_H * PT_W + e] = s[m];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PT_H * PT_W; e += 256) {
        const int row = e / PT_W, col = e - row * PT_W, y = y0 + row, x = x0 + col;
        if (y >= a.H || x >= a.W) continue;
        const size_t p = (size_t)y * a.W + x;
        double q[3];
        cols<3>(wd, hm, a.r, row, col, q);
        const float m = mask_at(a, b, c, HW, p);
        const float wt = a.wts[((size_t)b * a.wts_c + (a.wts_c == 1 ? 0 : c)) * HW + p];
        const float xv = a.pred[plane + p] * m, yv = a.gt[plane + p] * m;
        const double g = (double)(*gout / (float)a.B) / (double)counts[b] * (double)wt * (double)m;
        const float d = yv - xv;                                     // l1 = |gt m - pred m|: d l1 / d(pred m) = -sign(d)
        const double l1g = g * (1.0 - a.alpha) * (d > 0.0f ? -1.0 : (d < 0.0f ? 1.0 : 0.0));
        grad[plane + p] = (float)((double)m * (((q[0] + 2.0 * (double)xv * q[1]) + (double)yv * q[2]) + l1g));
    }
}

int fill_args(PhotoArgs& a, const float* pred, const float* gt, const float* mask, int mask_c, const float* wts, int wts_c, int B, int C, int H, int W,
              int window, const float* win, int box, double alpha, const char* what)
{
    if (!pred || !gt || !win) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null pointer");
    if (B < 1 || C < 1 || H < 1 || W < 1 || B > 65535 || C > 65535 || (long long)B * C * H * W > (1ll << 31) - 1)
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": bad shape");
    if (window < 3 || window > 2 * PR_MAX + 1 || !(window & 1)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": window must be odd, 3 .. 11");
    if (box != 0 && box != 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": mode must be 0 (gaussian) or 1 (box)");
    if (box && (H < window || W < window)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": the box window does not fit the image");
    if ((mask && mask_c != 1 && mask_c != C) || (wts && wts_c != 1 && wts_c != C))
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": mask / weights must have 1 or C channels");
    a.pred = pred; a.gt = gt; a.mask = mask; a.wts = wts; a.mask_c = mask_c; a.wts_c = wts_c;
    a.B = B; a.C = C; a.H = H; a.W = W; a.r = window / 2; a.box = box; a.alpha = alpha;
    for (int k = 0; k < 2 * PR_MAX + 1; ++k) a.win[k] = k < window ? win[k] : 0.0f;
    return OMNI_OK;
}

struct PhotoWs { size_t part, counts, total; unsigned nblk; };

PhotoWs photo_ws(int B, int C, int H, int W)
{
    PhotoWs l;
    l.nblk = (unsigned)(((W + PT_W - 1) / PT_W) * ((H + PT_H - 1) / PT_H)) * (unsigned)C;
    l.part = 0;
    l.counts = sizeof(double) * 2 * (size_t)l.nblk * B;
    l.total = (l.counts + sizeof(float) * (size_t)B + 255) / 256 * 256;
    return l;
}

}  // namespace

extern "C" int omni_ssim_f32(const float* pred, const float* gt, int B, int C, int H, int W, int window, const float* win, int mode, float* ssim,
                             omni_stream_t stream)
{
    PhotoArgs a;
    if (!ssim) OMNI_FAIL(OMNI_ERR_INVALID, "omni_ssim_f32: null device pointer");
    const int st = fill_args(a, pred, gt, nullptr, 1, nullptr, 1, B, C, H, W, window, win, mode, 0.0, "omni_ssim_f32");
    if (st != OMNI_OK) return st;
    const int tiles_x = (W + PT_W - 1) / PT_W, tiles = tiles_x * ((H + PT_H - 1) / PT_H);
    hipLaunchKernelGGL(photo_kernel<0>, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, a, tiles_x, (double*)nullptr, ssim,
                       (const float*)nullptr, (const float*)nullptr, (float*)nullptr);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_photometric_workspace_bytes(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return photo_ws(B, C, H, W).total;
}

extern "C" size_t omni_photometric_grad_scratch_bytes(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * 3 * (size_t)B * C * H * W;
}

extern "C" int omni_photometric_loss_f32(const float* pred, const float* gt, const float* mask, int mask_c, const float* weights, int weights_c,
                                         int B, int C, int H, int W, int window, const float* win, int mode, float alpha, void* workspace,
                                         float* loss, omni_stream_t stream)
{
    PhotoArgs a;
    if (!mask || !weights || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_photometric_loss_f32: null device pointer");
    if ((uintptr_t)workspace & 7) OMNI_FAIL(OMNI_ERR_INVALID, "omni_photometric_loss_f32: workspace must be 8-byte aligned");
    const int st = fill_args(a, pred, gt, mask, mask_c, weights, weights_c, B, C, H, W, window, win, mode, (double)alpha, "omni_photometric_loss_f32");
    if (st != OMNI_OK) return st;
    const PhotoWs l = photo_ws(B, C, H, W);
    double* part = (double*)((char*)workspace + l.part);
    float* counts = (float*)((char*)workspace + l.counts);
    const int tiles_x = (W + PT_W - 1) / PT_W, tiles = tiles_x * ((H + PT_H - 1) / PT_H);
    hipLaunchKernelGGL(photo_kernel<0>, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, a, tiles_x, part, (float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(photo_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, B, (int)l.nblk, loss, counts);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_photometric_grad_f32(const float* pred, const float* gt, const float* mask, int mask_c, const float* weights, int weights_c,
                                         int B, int C, int H, int W, int window, const float* win, int mode, float alpha, const void* workspace,
                                         void* scratch, const float* grad_out, float* grad_pred, omni_stream_t stream)
{
    PhotoArgs a;
    if (!mask || !weights || !workspace || !scratch || !grad_out || !grad_pred) OMNI_FAIL(OMNI_ERR_INVALID, "omni_photometric_grad_f32: null device pointer");
    const int st = fill_args(a, pred, gt, mask, mask_c, weights, weights_c, B, C, H, W, window, win, mode, (double)alpha, "omni_photometric_grad_f32");
    if (st != OMNI_OK) return st;
    const PhotoWs l = photo_ws(B, C, H, W);
    const float* counts = (const float*)((const char*)workspace + l.counts);
    float* P = (float*)scratch;
    const int tiles_x = (W + PT_W - 1) / PT_W, tiles = tiles_x * ((H + PT_H - 1) / PT_H);
    hipLaunchKernelGGL(photo_kernel<1>, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, a, tiles_x, (double*)nullptr, (float*)nullptr, counts,
                       grad_out, P);
    hipLaunchKernelGGL(photo_grad_kernel, dim3(tiles, C, B), dim3(256), 0, (hipStream_t)stream, a, tiles_x, (const float*)P, counts, grad_out, grad_pred);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
