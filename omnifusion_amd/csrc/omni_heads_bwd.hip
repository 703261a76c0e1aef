// omni_heads_bwd.hip — the two depth heads in training mode: pred and weight_pred, 3x3 convolutions from 32 channels to 1
// with bias, followed by ReLU, sigmoid and the product (model/spherical_model.py:304-307), and their backward.  fp32 FMAs throughout.
//
//     x  NHWC [M,H,W,32], any H, W >= 1      w [2][9][32] (pred, weight_pred; the layout of omni_heads_f32)      bias [2], DEVICE memory
//     p, q  the two pre-activations, planar [M,H,W]      a = relu(p) . (confidence ? sigmoid(q) : 1),  c = sigmoid(q), planar [M,H,W]
//
// Forward: the tiling of omni_net.hip's heads_kernel — persistent blocks, a 16x16 pixel tile with its 18x18x32 halo in LDS at pixel
// pitch 36, the next tile's halo in flight in registers, the two filters through the scalar cache — with tiles cut per axis,
// ceil(H/16) x ceil(W/16), the biases read from the device, and p and q written next to a and c when a gradient is pending.  p and q
// (8 B per pixel) are KEPT for the backward: recomputing them would read the 128 B per pixel of x a second time.
//
// Backward, three passes:
//   pre    gp = ga . s . [p > 0], gq = (ga . relu(p) + gc) . s (1 - s), s = sigmoid(q) (confidence = 0: gp = ga . [p > 0], gq = gc . s (1 - s)),
//          one thread per pixel, written interleaved [pixel][2] into the workspace.  An absent ga or gc counts as zero.
//   dgrad  dx[m,y,x,c] = sum_tap gp[y-ky+1, x-kx+1] . w[0][tap][c] + gq[...] . w[1][tap][c].  Block = a 16x16 tile; the (gp, gq) tile with a
//          one-pixel halo sits in LDS (zero outside the map: a tap outside the map is never read from memory); thread (quad = t & 7,
//          pixels t >> 3 + 32 k) holds the 2 x 9 x 4 weights of its channel quad and writes 16 bytes per pixel: a wave stores 1 KiB of
//          contiguous NHWC.
//   wgrad  dw[h][tap][c] = sum over the pixels of g_h[pixel] . x[pixel + tap - 1][c], db[h] = sum g_h.  A block walks a chunk of tiles;
//          thread (quad, pixel group) reads 16 bytes of x per pixel and feeds 72 FMAs against the 9 (gp, gq) neighbours in LDS, 72
//          accumulators in registers.  At the end the 8 pixel groups of a wave are added by xor-shuffles (8, 16, 32), the four waves in
//          order through LDS, and the block writes ONE partial [578] (dw [2][9][32], then db [2]).  The finish kernel adds the chunks'
//          partials in double by the chunk finish of omni_partials.h, as the stem's does.  No atomics, nothing
//          synchronised, the same bits on every run; dx of an item depends on that item alone.
#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr int DH_T = 16, DH_HALO = DH_T + 2, DH_PITCH = 36;
constexpr int DH_NW = 2 * 9 * 32;                     // floats of the two filters
constexpr int DH_PART = DH_NW + 2;                    // floats of one partial: dw [2][9][32], then db [2]
constexpr int DH_MIN_TILES = 4;                       // tiles per chunk at the least ...
constexpr int DH_MAX_CHUNKS = 1024;                   // ... and chunks at the most
constexpr int DH_FWD_BLOCKS = 768;

struct HeadsPlan { int tx, ty, ntiles, tpc, nchunk; long long n; };

bool heads_plan(int M, int H, int W, HeadsPlan& p)
{
    if (M <= 0 || H <= 0 || W <= 0) return false;
    p.n = (long long)M * H * W;
    if (p.n >= (1ll << 31)) return false;                              // (int pixel and tile indices)
    p.ty = (H + DH_T - 1) / DH_T; p.tx = (W + DH_T - 1) / DH_T;
    p.ntiles = (int)((long long)M * p.ty * p.tx);                      // <= n
    return partials_plan(p.ntiles, 1, DH_MIN_TILES, DH_MAX_CHUNKS, p.tpc, p.nchunk);
}

size_t heads_gpq_bytes(const HeadsPlan& p) { return ((size_t)p.n * 2 * sizeof(float) + 15) / 16 * 16; }
size_t heads_ws_bytes(const HeadsPlan& p) { return heads_gpq_bytes(p) + (size_t)p.nchunk * DH_PART * sizeof(float); }

__device__ __forceinline__ float dh_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(256) void dheads_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w /*[2][9][32]*/,
                                                         const float* __restrict__ bias /*[2]*/, float* __restrict__ outa,
                                                         float* __restrict__ outc, float* __restrict__ outp, float* __restrict__ outq,
                                                         int H, int W, int tx, int ty, int conf, int ntiles)
{
    __shared__ __attribute__((aligned(16))) float tile[DH_HALO * DH_HALO * DH_PITCH];
    constexpr int NQ = DH_HALO * DH_HALO * 8;                          // 16-byte pieces of a halo tile
    constexpr int NLD = (NQ + 255) / 256;
    const int per = tx * ty;
    const float bp = bias[0], bw = bias[1];
    f4v pre[NLD];
    auto fetch = [&](int tid) {
        const int m = tid / per, tt = tid % per;
        const int y0 = (tt / tx) * DH_T - 1, x0 = (tt % tx) * DH_T - 1;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = threadIdx.x + 256 * k;
            const int px = i >> 3, q = i & 7;
            const int iy = y0 + px / DH_HALO, ix = x0 + px % DH_HALO;
            pre[k] = (f4v)(0.0f);
            if (i < NQ && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                pre[k] = *reinterpret_cast<const f4v*>(x + (((size_t)m * H + iy) * W + ix) * 32 + q * 4);
        }
    };
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    int tid = blockIdx.x;
    if (tid < ntiles) fetch(tid);
    for (; tid < ntiles; tid += gridDim.x) {
        __syncthreads();                                               // the previous tile's taps are done
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (i < NQ) *reinterpret_cast<f4v*>(tile + (i >> 3) * DH_PITCH + (i & 7) * 4) = pre[k];
        }
        __syncthreads();
        if (tid + (int)gridDim.x < ntiles) fetch(tid + gridDim.x);
        float ap = bp, aw = bw;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float* px = tile + ((ly + ky) * DH_HALO + lx + kx) * DH_PITCH;
                const float* w0 = w + (ky * 3 + kx) * 32; const float* w1 = w0 + 288;
#pragma unroll
                for (int c = 0; c < 32; c += 4) {
                    const f4v v = *reinterpret_cast<const f4v*>(px + c);
                    ap = fmaf(v.x, w0[c], ap); ap = fmaf(v.y, w0[c + 1], ap); ap = fmaf(v.z, w0[c + 2], ap); ap = fmaf(v.w, w0[c + 3], ap);
                    aw = fmaf(v.x, w1[c], aw); aw = fmaf(v.y, w1[c + 1], aw); aw = fmaf(v.z, w1[c + 2], aw); aw = fmaf(v.w, w1[c + 3], aw);
                }
            }
        const int m = tid / per, tt = tid % per;
        const int oy = (tt / tx) * DH_T + ly, ox = (tt % tx) * DH_T + lx;
        if (oy < H && ox < W) {
            const size_t i = ((size_t)m * H + oy) * W + ox;
            const float pr = fmaxf(ap, 0.0f), cf = dh_sigmoid(aw);
            outa[i] = conf ? pr * cf : pr;
            if (outc) outc[i] = cf;
            if (outp) outp[i] = ap;
            if (outq) outq[i] = aw;
        }
    }
}

// one thread per pixel; ga, gc, q may each be null (an absent gradient is zero; without q there is no gq)
__global__ __launch_bounds__(256) void dheads_pre_kernel(const float* __restrict__ ga, const float* __restrict__ gc, const float* __restrict__ p,
                                                         const float* __restrict__ q, f2v* __restrict__ gpq, int n, int conf)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float pv = p[i];
    const float a = ga ? ga[i] : 0.0f, c = gc ? gc[i] : 0.0f;
    float gp, gq = 0.0f;
    if (conf) {
        const float s = dh_sigmoid(q[i]);
        gp = pv > 0.0f ? a * s : 0.0f;
        gq = (a * fmaxf(pv, 0.0f) + c) * (s * (1.0f - s));
    } else {
        gp = pv > 0.0f ? a : 0.0f;
        if (gc) { const float s = dh_sigmoid(q[i]); gq = c * (s * (1.0f - s)); }
    }
    gpq[i] = f2v{gp, gq};
}

// the (gp, gq) tile under the 16x16 pixels at (y0, x0) of item m with a one-pixel halo; zero outside the map
__device__ __forceinline__ void dh_load_g(f2v (&g)[DH_HALO][DH_HALO + 1], const f2v* __restrict__ gpq, size_t m, int y0, int x0, int H, int W)
{
    for (int i = threadIdx.x; i < DH_HALO * DH_HALO; i += 256) {
        const int r = i / DH_HALO, c = i % DH_HALO;
        const int iy = y0 - 1 + r, ix = x0 - 1 + c;
        f2v v = {0.0f, 0.0f};
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = gpq[(m * H + iy) * (size_t)W + ix];
        g[r][c] = v;
    }
}

__global__ __launch_bounds__(256) void dheads_dgrad_kernel(const f2v* __restrict__ gpq, const float* __restrict__ w, float* __restrict__ dx,
                                                           int H, int W, int tx, int ty)
{
    __shared__ f2v g[DH_HALO][DH_HALO + 1];
    const int t = threadIdx.x, quad = t & 7, pg = t >> 3;
    const unsigned per = (unsigned)(tx * ty), tt = blockIdx.x % per;
    const size_t m = blockIdx.x / per;
    const int y0 = (int)(tt / (unsigned)tx) * DH_T, x0 = (int)(tt % (unsigned)tx) * DH_T;
    dh_load_g(g, gpq, m, y0, x0, H, W);
    f4v wp[9], wq[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        wp[tap] = *reinterpret_cast<const f4v*>(w + tap * 32 + quad * 4);
        wq[tap] = *reinterpret_cast<const f4v*>(w + 288 + tap * 32 + quad * 4);
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < 8; ++k) {
        const int pix = pg + 32 * k, py = pix >> 4, px = pix & 15;
        const int oy = y0 + py, ox = x0 + px;
        if (oy >= H || ox >= W) continue;                              // the partial tiles at the right and bottom edges
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f2v gv = g[py + 2 - ky][px + 2 - kx];            // the output pixel (oy - ky + 1, ox - kx + 1) that read this one by tap (ky, kx)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[e] = fmaf(gv.x, wp[ky * 3 + kx][e], acc[e]);
                    acc[e] = fmaf(gv.y, wq[ky * 3 + kx][e], acc[e]);
                }
            }
        *reinterpret_cast<f4v*>(dx + ((m * H + oy) * (size_t)W + ox) * 32 + quad * 4) = f4v{acc[0], acc[1], acc[2], acc[3]};
    }
}

__global__ __launch_bounds__(256) void dheads_wgrad_kernel(const f2v* __restrict__ gpq, const float* __restrict__ x, float* __restrict__ part,
                                                           int H, int W, int tx, int ty, int ntiles, int tpc)
{
    __shared__ f2v g[DH_HALO][DH_HALO + 1];
    __shared__ float red[4][DH_PART + 2];
    const int t = threadIdx.x, quad = t & 7, pg = t >> 3;
    float acc[2][9][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[h][tap][e] = 0.0f;
    float accb[2] = {0.0f, 0.0f};
    const unsigned per = (unsigned)(tx * ty);
    const int tile0 = blockIdx.x * tpc, tile1 = min(ntiles - tile0, tpc) + tile0;
    for (int tile = tile0; tile < tile1; ++tile) {
        const unsigned tt = (unsigned)tile % per;
        const size_t m = (unsigned)tile / per;
        const int y0 = (int)(tt / (unsigned)tx) * DH_T, x0 = (int)(tt % (unsigned)tx) * DH_T;
        f4v xv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pix = pg + 32 * k, iy = y0 + (pix >> 4), ix = x0 + (pix & 15);
            xv[k] = (f4v)(0.0f);
            if (iy < H && ix < W) xv[k] = *reinterpret_cast<const f4v*>(x + ((m * H + iy) * (size_t)W + ix) * 32 + quad * 4);
        }
        __syncthreads();                                               // the previous tile's neighbours are read
        dh_load_g(g, gpq, m, y0, x0, H, W);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int pix = pg + 32 * k, py = pix >> 4, px = pix & 15;
            if (y0 + py >= H || x0 + px >= W) continue;                // a pixel past the edge adds nothing
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const f2v gv = g[py + 2 - ky][px + 2 - kx];        // the output pixel that reads this input pixel by tap (ky, kx)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[0][ky * 3 + kx][e] = fmaf(gv.x, xv[k][e], acc[0][ky * 3 + kx][e]);
                        acc[1][ky * 3 + kx][e] = fmaf(gv.y, xv[k][e], acc[1][ky * 3 + kx][e]);
                    }
                    if (ky == 1 && kx == 1) { accb[0] += gv.x; accb[1] += gv.y; }      // every pixel of the map once: the bias gradient
                }
        }
    }
    // the 8 pixel groups of a wave (lanes quad, quad + 8, ...), then the four waves in order
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[h][tap][e];
                v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
                if (lane < 8) red[wave][(h * 9 + tap) * 32 + quad * 4 + e] = v;
            }
        float v = accb[h];
        v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        if (lane == 0) red[wave][DH_NW + h] = v;
    }
    __syncthreads();
    float* po = part + (size_t)blockIdx.x * DH_PART;
    for (int i = t; i < DH_PART; i += 256) po[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// Block b: outputs 16 b .. 16 b + 15 of the 578.  dw and db may each be null (not asked for).
__global__ __launch_bounds__(256) void dheads_wgrad_finish_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ dw,
                                                                  float* __restrict__ db)
{
    chunk_sums<DH_PART, DH_NW>(part, nchunk, dw, db);
}

}  // namespace

extern "C" int omni_depth_heads_fwd_f32(const float* x, const float* w, const float* bias, float* out_a, float* out_c, float* out_p,
                                        float* out_q, int M, int H, int W, int confidence, omni_stream_t stream)
{
    if (!x || !w || !bias || !out_a) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_fwd: null pointer");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_fwd: M, H, W >= 1");
    HeadsPlan p;
    if (!heads_plan(M, H, W, p)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_depth_heads_fwd: tensor too large for 32-bit pixel indices");
    hipLaunchKernelGGL(dheads_fwd_kernel, dim3(p.ntiles < DH_FWD_BLOCKS ? p.ntiles : DH_FWD_BLOCKS), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                       out_a, out_c, out_p, out_q, H, W, p.tx, p.ty, confidence, p.ntiles);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_depth_heads_bwd_workspace_bytes(int M, int H, int W)
{
    HeadsPlan p;
    if (!heads_plan(M, H, W, p)) return 0;
    return heads_ws_bytes(p);
}

extern "C" int omni_depth_heads_bwd_f32(const float* grad_a, const float* grad_c, const float* p, const float* q, const float* x, const float* w,
                                        float* dx, float* dw, float* dbias, int M, int H, int W, int confidence, void* workspace,
                                        size_t ws_bytes, omni_stream_t stream)
{
    if (!p || !w) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: null pointer");
    if (!grad_a && !grad_c) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: neither grad_a nor grad_c");
    if (!dx && !dw && !dbias) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: no gradient requested");
    if ((confidence || grad_c) && !q) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: q is needed with confidence or grad_c");
    if ((dw || dbias) && !x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: the weight gradient reads x");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: M, H, W >= 1");
    HeadsPlan pl;
    if (!heads_plan(M, H, W, pl)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_depth_heads_bwd: tensor too large for 32-bit pixel indices");
    if (!workspace || ws_bytes < heads_ws_bytes(pl)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_depth_heads_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    f2v* gpq = (f2v*)workspace;
    float* part = (float*)((char*)workspace + heads_gpq_bytes(pl));
    const int n = (int)pl.n;
    hipLaunchKernelGGL(dheads_pre_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grad_a, grad_c, p, q, gpq, n, confidence);
    OMNI_HIP(hipGetLastError());
    if (dx) {
        hipLaunchKernelGGL(dheads_dgrad_kernel, dim3((unsigned)pl.ntiles), dim3(256), 0, s, (const f2v*)gpq, w, dx, H, W, pl.tx, pl.ty);
        OMNI_HIP(hipGetLastError());
    }
    if (dw || dbias) {
        hipLaunchKernelGGL(dheads_wgrad_kernel, dim3((unsigned)pl.nchunk), dim3(256), 0, s, (const f2v*)gpq, x, part, H, W, pl.tx, pl.ty, pl.ntiles,
                           pl.tpc);
        OMNI_HIP(hipGetLastError());
        hipLaunchKernelGGL(dheads_wgrad_finish_kernel, dim3((DH_PART + 15) / 16), dim3(256), 0, s, (const float*)part, pl.nchunk, dw, dbias);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}
