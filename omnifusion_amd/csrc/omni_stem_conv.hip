// omni_stem_conv.hip — the stem convolution for training: conv1 of the encoder, 7x7 at stride 2 with padding 3, 3 -> 64
// channels, WITHOUT the folded batch normalisation and the ReLU of omni_stem_f32 (a training-mode batch normalisation follows it), and
// its gradient w.r.t. the filter bank and the bias.  fp32 FMAs throughout: K = 147 fits the matrix cores badly and the layer is ~2 % of
// the forward's flops.
//
//     x  planar [M,3,H,W], any H, W >= 1      wt [147][64], k = (ky*7+kx)*3+c (the layout of omni_stem_f32)      y, g  NHWC [M,Ho,Wo,64]
//
// Forward: the block of omni_net.hip's stem_kernel — the zero-padded input patch and the whole filter bank in LDS, thread = (pixel, 16
// channels), the four 16-byte weight reads per tap wave-uniform — with FOUR pixels per thread (rows py, py + 8 and columns px, px + 8 of
// a 16 x 16 output tile over a 37 x 37 x 3 patch): each weight read feeds 16 FMAs instead of 4, which is what that kernel is bound by
// (LDS reads, not FMAs), and the 37-KiB bank is fetched once per 256 pixels.  Every tile edge is guarded: tiles are cut per axis,
// ceil(Ho/16) x ceil(Wo/16).
//
// Weight gradient: dw[k][o] = sum over the M.Ho.Wo output pixels of g[pixel][o] . patch[pixel][k].  A block of 256 threads owns ALL
// 148 x 64 outputs (row 147 is the bias gradient) and walks a chunk of tiles; per tile it stages g (64 pixels x 64 channels, 16 KiB) and
// the input patch (5.4 KiB) in LDS.  Thread (q = t & 15, kg = t >> 4) holds the 10 x 4 outputs of taps 10 kg .. 10 kg + 9 and channel quad
// q in registers: per pixel one 16-byte read of g and ten 4-byte reads of the patch feed 40 FMAs.  In a wave the sixteen quads read 256
// contiguous bytes of g (each address shared by four lanes) and the four tap groups four patch addresses (broadcast): no bank conflicts.
// Taps 147 .. 159 do not exist: their threads read patch offset 0 and drop the result, except that the thread group kg = 15 (no real tap
// at all) multiplies by 1 in its first row and so sums g itself: the bias gradient, out of the same pass.
// The block's partial sums go to the workspace; the finish kernel adds the chunks' partials in double by the chunk finish of
// omni_partials.h.  No atomics, nothing synchronised, the same bits on every run.
#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int ST_K = 147, ST_CO = 64, ST_TILE = 8;
constexpr int ST_PATCH = 2 * ST_TILE + 5;             // 21 input rows / columns under an 8 x 8 output tile
constexpr int ST_FTILE = 2 * ST_TILE;                 // output rows / columns of a forward tile
constexpr int ST_FPATCH = 2 * ST_FTILE + 5;           // 37 input rows / columns under it
constexpr int ST_PITCH = ST_PATCH + 1;
constexpr int ST_KPT = 10;                            // taps per thread of the weight gradient: 16 groups x 10 >= 147
constexpr int ST_PART = (ST_K + 1) * ST_CO;           // floats of one partial: dw [147][64], then dbias [64]
constexpr int ST_MIN_TILES = 4;                       // tiles per chunk at the least (256 pixels in one fp32 chain) ...
constexpr int ST_MAX_CHUNKS = 1024;                   // ... and chunks at the most

struct StemPlan { int Ho, Wo, tx, ty, ntiles, tpc, nchunk; };

bool stem_plan(int M, int H, int W, StemPlan& p)
{
    if (M <= 0 || H <= 0 || W <= 0) return false;
    p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
    p.ty = (p.Ho + ST_TILE - 1) / ST_TILE; p.tx = (p.Wo + ST_TILE - 1) / ST_TILE;
    const long long nt = (long long)M * p.ty * p.tx;
    if (nt > 0x7fffffffll - (1 << 22)) return false;                   // (int tile indices, stepped by a chunk of up to 2^21 tiles)
    p.ntiles = (int)nt;
    return partials_plan(p.ntiles, 1, ST_MIN_TILES, ST_MAX_CHUNKS, p.tpc, p.nchunk);
}

size_t stem_ws_bytes(const StemPlan& p) { return (size_t)p.nchunk * ST_PART * sizeof(float); }

// the zero-padded input patch under the tile at (oy0, ox0) of image m
template <int N>
__device__ __forceinline__ void stem_load_patch(float (&in)[3][N][N + 1], const float* __restrict__ x, size_t m, int oy0, int ox0, int H, int W)
{
    const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
    for (int i = threadIdx.x; i < 3 * N * N; i += 256) {
        const int c = i / (N * N), r = (i % (N * N)) / N, q = i % N;
        const int iy = iy0 + r, ix = ix0 + q;
        float v = 0.0f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = x[((m * 3 + c) * (size_t)H + iy) * (size_t)W + ix];
        in[c][r][q] = v;
    }
}

__global__ __launch_bounds__(256) void stem_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, float* __restrict__ y, int H, int W, int Ho,
                                                            int Wo, int tx, int ty)
{
    __shared__ __attribute__((aligned(16))) float wl[ST_K * ST_CO];
    __shared__ float in[3][ST_FPATCH][ST_FPATCH + 1];
    const int t = threadIdx.x;
    const unsigned per = (unsigned)(tx * ty), tt = blockIdx.x % per;
    const size_t m = blockIdx.x / per;
    const int oy0 = (int)(tt / (unsigned)tx) * ST_FTILE, ox0 = (int)(tt % (unsigned)tx) * ST_FTILE;
    for (int i = t; i < ST_K * ST_CO / 4; i += 256) reinterpret_cast<f4v*>(wl)[i] = reinterpret_cast<const f4v*>(wt)[i];
    stem_load_patch<ST_FPATCH>(in, x, m, oy0, ox0, H, W);
    __syncthreads();
    const int p = t & 63, cg = (t >> 6) * 16;
    const int py = p >> 3, px = p & 7;
    float acc[4][16];                                                  // pixel h: row py + 8 (h >> 1), column px + 8 (h & 1)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[0][j] = acc[1][j] = acc[2][j] = acc[3][j] = bias ? bias[cg + j] : 0.0f;
    for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) v[h] = in[c][(py + ST_TILE * (h >> 1)) * 2 + ky][(px + ST_TILE * (h & 1)) * 2 + kx];
                const float* w = wl + ((ky * 7 + kx) * 3 + c) * ST_CO + cg;
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) {
                    const f4v wv = *reinterpret_cast<const f4v*>(w + 4 * j4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int h = 0; h < 4; ++h) acc[h][4 * j4 + e] = fmaf(v[h], wv[e], acc[h][4 * j4 + e]);
                }
            }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int oy = oy0 + py + ST_TILE * (h >> 1), ox = ox0 + px + ST_TILE * (h & 1);
        if (oy >= Ho || ox >= Wo) continue;                            // the partial tiles at the right and bottom edges
        float* o = y + ((m * Ho + oy) * (size_t)Wo + ox) * ST_CO + cg;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
            *reinterpret_cast<f4v*>(o + 4 * j4) = f4v{acc[h][4 * j4], acc[h][4 * j4 + 1], acc[h][4 * j4 + 2], acc[h][4 * j4 + 3]};
    }
}

__global__ __launch_bounds__(256) void stem_conv_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part,
                                                              int H, int W, int Ho, int Wo, int tx, int ty, int ntiles, int tpc)
{
    __shared__ __attribute__((aligned(16))) float gl[64 * ST_CO];
    __shared__ float in[3][ST_PATCH][ST_PITCH];
    const int t = threadIdx.x, q = t & 15, kg = t >> 4;
    int off[ST_KPT];
#pragma unroll
    for (int j = 0; j < ST_KPT; ++j) {
        const int k = kg * ST_KPT + j;
        const int tap = k / 3, c = k % 3;
        off[j] = k < ST_K ? (c * ST_PATCH + tap / 7) * ST_PITCH + tap % 7 : 0;
    }
    const bool ones = kg == 15;                                        // taps 150 .. 159: none is real; row 0 of this group sums g
    float acc[ST_KPT][4];
#pragma unroll
    for (int j = 0; j < ST_KPT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = 0.0f;
    const unsigned per = (unsigned)(tx * ty);
    const int tile0 = blockIdx.x * tpc, tile1 = min(ntiles - tile0, tpc) + tile0;
    const float* inf = &in[0][0][0];
    for (int tile = tile0; tile < tile1; ++tile) {
        const unsigned tt = (unsigned)tile % per;
        const size_t m = (unsigned)tile / per;
        const int oy0 = (int)(tt / (unsigned)tx) * ST_TILE, ox0 = (int)(tt % (unsigned)tx) * ST_TILE;
        for (int i = t; i < 64 * ST_CO / 4; i += 256) {
            const int p = i >> 4, oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
            f4v v = {0.0f, 0.0f, 0.0f, 0.0f};                         // a pixel past the edge adds nothing
            if (oy < Ho && ox < Wo) v = *reinterpret_cast<const f4v*>(g + ((m * Ho + oy) * (size_t)Wo + ox) * ST_CO + 4 * (i & 15));
            reinterpret_cast<f4v*>(gl)[i] = v;
        }
        stem_load_patch<ST_PATCH>(in, x, m, oy0, ox0, H, W);
        __syncthreads();
        for (int py = 0; py < ST_TILE; ++py) {
#pragma unroll
            for (int px = 0; px < ST_TILE; ++px) {
                const f4v gv = *reinterpret_cast<const f4v*>(gl + (py * ST_TILE + px) * ST_CO + 4 * q);
                const float* ip = inf + py * 2 * ST_PITCH + px * 2;
#pragma unroll
                for (int j = 0; j < ST_KPT; ++j) {
                    float v = ip[off[j]];
                    if (j == 0) v = ones ? 1.0f : v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(v, gv[e], acc[j][e]);
                }
            }
        }
        __syncthreads();
    }
    float* p0 = part + (size_t)blockIdx.x * ST_PART + 4 * q;
#pragma unroll
    for (int j = 0; j < ST_KPT; ++j) {
        const int k = kg * ST_KPT + j;
        if (k < ST_K) *reinterpret_cast<f4v*>(p0 + k * ST_CO) = f4v{acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
    }
    if (ones) *reinterpret_cast<f4v*>(p0 + ST_K * ST_CO) = f4v{acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
}

// Block b: outputs 16 b .. 16 b + 15 of the 148 x 64 (9472 = 592 x 16).  dw and dbias may each be null (not asked for).
__global__ __launch_bounds__(256) void stem_conv_wgrad_finish_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ dw,
                                                                     float* __restrict__ dbias)
{
    chunk_sums<ST_PART, ST_K * ST_CO>(part, nchunk, dw, dbias);
}

}  // namespace

extern "C" int omni_stem_conv_fwd_f32(const float* x, const float* wt, const float* bias, float* y, int M, int H, int W, omni_stream_t stream)
{
    if (!x || !wt || !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_fwd: null pointer");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_fwd: M, H, W >= 1");
    StemPlan p;
    if (!stem_plan(M, H, W, p)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_stem_conv_fwd: too many tiles for one launch");
    const int fty = (p.Ho + ST_FTILE - 1) / ST_FTILE, ftx = (p.Wo + ST_FTILE - 1) / ST_FTILE;      // 16 x 16 tiles: no more of them than p.ntiles
    hipLaunchKernelGGL(stem_conv_fwd_kernel, dim3((unsigned)M * fty * ftx), dim3(256), 0, (hipStream_t)stream, x, wt, bias, y, H, W, p.Ho, p.Wo, ftx,
                       fty);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" size_t omni_stem_conv_bwd_workspace_bytes(int M, int H, int W)
{
    StemPlan p;
    if (!stem_plan(M, H, W, p)) return 0;
    return stem_ws_bytes(p);
}

extern "C" int omni_stem_conv_bwd_weight_f32(const float* g, const float* x, float* dw, float* dbias, int M, int H, int W, void* workspace,
                                             size_t ws_bytes, omni_stream_t stream)
{
    if (!g || !x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_bwd_weight: null pointer");
    if (!dw && !dbias) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_bwd_weight: no gradient requested");
    if (M <= 0 || H <= 0 || W <= 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_bwd_weight: M, H, W >= 1");
    StemPlan p;
    if (!stem_plan(M, H, W, p)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_stem_conv_bwd_weight: too many tiles for one launch");
    if (!workspace || ws_bytes < stem_ws_bytes(p)) OMNI_FAIL(OMNI_ERR_INVALID, "omni_stem_conv_bwd_weight: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    hipLaunchKernelGGL(stem_conv_wgrad_kernel, dim3(p.nchunk), dim3(256), 0, s, g, x, part, H, W, p.Ho, p.Wo, p.tx, p.ty, p.ntiles, p.tpc);
    OMNI_HIP(hipGetLastError());
    hipLaunchKernelGGL(stem_conv_wgrad_finish_kernel, dim3(ST_PART / 16), dim3(256), 0, s, (const float*)part, p.nchunk, dw, dbias);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
