// omni_io.hip — the host-facing ends of the hot path: what sits between the loader / the export
// code of the reference and the equi_pers operators, moved onto the device so that the GPU is never fed or drained by
// per-pixel host work.  gfx950 only.  All kernels are HBM-bound streaming passes (coalesced 16-byte accesses where the layout allows).
//
//   omni_preprocess_rgb_u8     decoded BGR uint8 HWC frame(s) -> cv2.INTER_AREA resize -> /255 -> float32 CHW
//                              (dataset_loader_stanford.py:54,92-97 `readRGBPano` + `rgb.astype(np.float32)/255` + transpose(2,0,1) :85)
//   omni_preprocess_depth_u16  16-bit depth frame -> float32 -> INTER_AREA resize -> /65535*128 -> mask (0.1, 8] -> depth *= mask
//                              (dataset_loader_stanford.py:99-109 `readDepthPano`, :76-80)
//   omni_pointcloud_ply_f32    depth map + panorama -> binary PLY vertex records x,y,z,blue,green,red (test.py:210-240, util.py:159-174)
#include "omni_internal.h"
#include "omni_area.h"          // AreaSpan, area_span, area_sample, area_round_u8 (shared with omni_augment.hip)

namespace {

__global__ __launch_bounds__(256) void prep_rgb_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int B, int Hs, int Ws,
                                                       int H, int W, float sy_, float sx_)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // one thread per destination pixel (all 3 channels)
    if (i >= (size_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((size_t)H * W));
    const unsigned char* s = src + (size_t)b * Hs * Ws * 3;
    float v[3];
    if (Hs == H && Ws == W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)s[((size_t)y * Ws + x) * 3 + c];
    } else {
        const AreaSpan ay = area_span(y, sy_, Hs), ax = area_span(x, sx_, Ws);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float avg = area_sample<unsigned char>(s, Hs, Ws, 3, c, ay, ax);
            v[c] = area_round_u8(avg, Hs == 2 * H && Ws == 2 * W);      // back to uint8 before the /255
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(((size_t)b * 3 + c) * H + y) * W + x] = v[c] / 255.0f;     // :54  (BGR order kept: quirk q10)
}

// frames that already have the network's size (no INTER_AREA pass): four pixels per thread — three aligned 4-byte loads, one 16-byte store
// per channel (the byte-per-lane form above: 44 us for 8 x 512 x 1024, 1.4 TB/s; same arithmetic, same bits)
__global__ __launch_bounds__(256) void prep_rgb_same_kernel(const unsigned* __restrict__ src, float* __restrict__ dst, size_t quads, size_t plane /* H*W */)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const unsigned w0 = src[3 * q], w1 = src[3 * q + 1], w2 = src[3 * q + 2];      // 12 bytes: b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
    const size_t px = 4 * q, b = px / plane, o = px - b * plane;
    float* d = dst + b * 3 * plane + o;
    const float c0[4] = {(float)(w0 & 255u), (float)(w0 >> 24), (float)((w1 >> 16) & 255u), (float)((w2 >> 8) & 255u)};
    const float c1[4] = {(float)((w0 >> 8) & 255u), (float)(w1 & 255u), (float)(w1 >> 24), (float)((w2 >> 16) & 255u)};
    const float c2[4] = {(float)((w0 >> 16) & 255u), (float)((w1 >> 8) & 255u), (float)(w2 & 255u), (float)(w2 >> 24)};
    *reinterpret_cast<float4*>(d) = make_float4(c0[0] / 255.0f, c0[1] / 255.0f, c0[2] / 255.0f, c0[3] / 255.0f);
    *reinterpret_cast<float4*>(d + plane) = make_float4(c1[0] / 255.0f, c1[1] / 255.0f, c1[2] / 255.0f, c1[3] / 255.0f);
    *reinterpret_cast<float4*>(d + 2 * plane) = make_float4(c2[0] / 255.0f, c2[1] / 255.0f, c2[2] / 255.0f, c2[3] / 255.0f);
}

__global__ __launch_bounds__(256) void prep_depth_kernel(const unsigned short* __restrict__ src, float* __restrict__ depth, unsigned char* __restrict__ mask,
                                                         int B, int Hs, int Ws, int H, int W, float sy_, float sx_, float min_d, float max_d)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((size_t)H * W));
    const unsigned short* s = src + (size_t)b * Hs * Ws;
    float v;
    if (Hs == H && Ws == W) v = (float)s[(size_t)y * Ws + x];
    else { const AreaSpan ay = area_span(y, sy_, Hs), ax = area_span(x, sx_, Ws); v = area_sample<unsigned short>(s, Hs, Ws, 1, 0, ay, ax); }
    v = v / 65535.0f * 128.0f;                                         // :108
    const bool m = (v <= max_d) && (v > min_d);                        // :76
    depth[i] = m ? v : 0.0f;                                           // :79  depth *= mask
    mask[i] = m ? 1 : 0;
}

// ------------------------------------------------------------------ point cloud, test.py:210-240
// vertex i of image b (row-major, x fastest — np.meshgrid(range(w), range(h)) reshaped, :211-213):
//   coords = (x+1, y+1);  u = (cx - (w/2 + 0.5)) / w * 2 pi,  v = -(cy - (h/2 + 0.5)) / h * pi          util.py:159-165
//   xyz = (cos v sin u, cos v cos u, sin v) * depth                                                      util.py:168-173, test.py:218-219
//   colour = uint8(rgb * 255) of the three image channels in loader order, written as blue, green, red   test.py:229,236
// record: 3 x float32 + 3 x uint8 = 15 bytes, packed (the numpy structured array ply.py:303-314 writes)
__global__ __launch_bounds__(256) void pointcloud_kernel(const float* __restrict__ depth, const float* __restrict__ rgb, unsigned char* __restrict__ out,
                                                         int B, int H, int W)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((size_t)H * W));
    const float PI_F = 3.14159265358979323846f;
    // numpy float32 arithmetic of coords2uv: (int - python float) -> float64, / w * 2 * pi in float64, stored to float32
    const double u64 = ((double)(x + 1) - ((double)W / 2.0 + 0.5)) / (double)W * 2.0 * 3.141592653589793;
    const double v64 = -((double)(y + 1) - ((double)H / 2.0 + 0.5)) / (double)H * 3.141592653589793;
    const float u = (float)u64, v = (float)v64;
    (void)PI_F;
    const float cv = cosf(v), sv = sinf(v), su = sinf(u), cu = cosf(u);
    const float d = depth[i];
    float p[3] = {cv * su * d, cv * cu * d, sv * d};
    unsigned char* o = out + i * 15;
    __builtin_memcpy(o, p, 12);
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float col = rgb[((size_t)b * 3 + c) * plane + pix] * 255.0f;
        o[12 + c] = (unsigned char)(int)fminf(255.0f, fmaxf(0.0f, col));            // astype(np.uint8): truncation
    }
}

}  // namespace

extern "C" int omni_preprocess_rgb_u8(const unsigned char* src_hwc, float* dst_chw, int B, int Hs, int Ws, int H, int W, omni_stream_t stream)
{
    if (!src_hwc || !dst_chw) OMNI_FAIL(OMNI_ERR_INVALID, "omni_preprocess_rgb_u8: null device pointer");
    if (B < 0 || Hs < 1 || Ws < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_preprocess_rgb_u8: bad shape");
    if (H > Hs || W > Ws) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_preprocess_rgb_u8: INTER_AREA is a down-scale here (the loader shrinks 4096x2048 scans)");
    if (B == 0) return OMNI_OK;
    const size_t n = (size_t)B * H * W;
    if (Hs == H && Ws == W && ((size_t)H * W) % 4 == 0 && (uintptr_t)src_hwc % 4 == 0 && (uintptr_t)dst_chw % 16 == 0) {
        hipLaunchKernelGGL(prep_rgb_same_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)src_hwc, dst_chw, n / 4, (size_t)H * W);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    hipLaunchKernelGGL(prep_rgb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src_hwc, dst_chw, B, Hs, Ws, H, W,
                       (float)((double)Hs / H), (float)((double)Ws / W));
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_preprocess_depth_u16(const unsigned short* src, float* depth, unsigned char* mask, int B, int Hs, int Ws, int H, int W,
                                         float min_depth, float max_depth, omni_stream_t stream)
{
    if (!src || !depth || !mask) OMNI_FAIL(OMNI_ERR_INVALID, "omni_preprocess_depth_u16: null device pointer");
    if (B < 0 || Hs < 1 || Ws < 1 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_preprocess_depth_u16: bad shape");
    if (H > Hs || W > Ws) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_preprocess_depth_u16: INTER_AREA is a down-scale here");
    if (B == 0) return OMNI_OK;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(prep_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, depth, mask, B, Hs, Ws, H, W,
                       (float)((double)Hs / H), (float)((double)Ws / W), min_depth, max_depth);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_pointcloud_ply_f32(const float* depth, const float* rgb, unsigned char* records, int B, int H, int W, omni_stream_t stream)
{
    if (!depth || !rgb || !records) OMNI_FAIL(OMNI_ERR_INVALID, "omni_pointcloud_ply_f32: null device pointer");
    if (B < 0 || H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_pointcloud_ply_f32: bad shape");
    if (B == 0) return OMNI_OK;
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(pointcloud_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, rgb, records, B, H, W);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
