// omni_point_conv.hip — the 1x1 convolutions of the point-feature MLPs in training mode: mlp_points1 / mlp_points2 of
// model/spherical_model_iterative.py:290-305, 387-393 (and mlp_points of the single pass), small channel counts, no bias, fp32 FMAs.
//
//     y[m, hw, o] = sum_c W[o][c] . (x[m mod Mx, c, hw] . (scale ? scale[m, hw] : 1))          rows = M . HW < 2^31
//
// Three instantiations, nothing else:   3 -> 16   x planar [Mx,3,HW], broadcast over M / Mx repeats, optional scale [M,HW]
//                                       5 -> 16   x planar [M,5,HW]
//                                      16 -> 64   x NHWC [M,HW,16]
// W is the parameter's own storage [Cout][Cin]; y, gy NHWC [M,HW,Cout]; the product x . scale is rounded before the FMAs, as the
// reference's `xyz * depth` is before its convolution; the sum runs over c in ascending order from 0.
//
// Forward: thread (row, quad of outputs) holds its 4 x Cin weights in registers and walks rows with a grid stride; Cout / 4 neighbouring
//          lanes share a row (the loads of x are broadcasts) and write 16 bytes each: a wave stores 1 KiB of contiguous NHWC.
// dscale:  dscale[m,hw] = sum_c x[m mod Mx,c,hw] . t_c, t_c = sum_o W[o][c] . gy[m,hw,o] (o ascending, then c ascending): one thread per
//          pixel, a gather.
// dx:      dx[m,hw,c] = sum_o W[o][c] . gy[m,hw,o], o ascending (16 -> 64 only): thread (row, quad of c), W in LDS, 16-byte stores.
// dW:      dW[o][c] = sum over the rows of gy[row][o] . (x . scale)[row][c].  A block walks a chunk of rows (partials_plan of
//          omni_partials.h) in tiles of 64 rows staged in LDS; a thread OWNS its accumulators — 16 -> 64: 4 of the 1024 per thread, all
//          rows; 5 -> 16: one of the 80 per thread of a 128-thread group, two groups on alternate rows; 3 -> 16: one of the 48 per lane of
//          a wave, four waves on every fourth row — so nothing is exchanged but the groups' sums, added in group order through LDS.  The
//          block writes ONE partial [Cout . Cin]; the chunk finish of omni_partials.h adds the partials.
// No atomics, nothing synchronised, nothing allocated: capturable, the same bits on every run; dscale and dx of an item depend on that
// item alone.
#include "omni_internal.h"
#include "omni_partials.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int PC_TILE = 64;                           // rows staged per step of the weight-gradient pass
constexpr int PC_MIN_TILES = 5;                       // tiles per chunk at the least ...
constexpr int PC_MAX_CHUNKS = 1024;                   // ... and chunks at the most
constexpr int PC_FWD_BLOCKS = 2048;

struct PointPlan { int rows, per, nchunk; };

bool point_form(int Cin, int Cout) { return (Cin == 3 && Cout == 16) || (Cin == 5 && Cout == 16) || (Cin == 16 && Cout == 64); }

bool point_plan(int M, int HW, PointPlan& p)
{
    if (M <= 0 || HW <= 0) return false;
    const long long rows = (long long)M * HW;
    if (rows >= (1ll << 31)) return false;                             // (int row indices)
    p.rows = (int)rows;
    return partials_plan(rows, PC_TILE, PC_MIN_TILES, PC_MAX_CHUNKS, p.per, p.nchunk);
}

// the CIN inputs of a row, scaled: planar x is read at (m mod Mx, c, hw), NHWC x as four 16-byte pieces
template <int CIN, bool NHWC>
__device__ __forceinline__ void pc_load_row(float (&xv)[CIN], const float* __restrict__ x, const float* __restrict__ scale, int row, int Mx, int HW)
{
    if constexpr (NHWC) {
#pragma unroll
        for (int c = 0; c < CIN; c += 4) {
            const f4v v = *reinterpret_cast<const f4v*>(x + (size_t)row * CIN + c);
            xv[c] = v.x; xv[c + 1] = v.y; xv[c + 2] = v.z; xv[c + 3] = v.w;
        }
    } else {
        const int m = row / HW, hw = row - m * HW;
        const float* px = x + (size_t)(m % Mx) * CIN * HW + hw;
#pragma unroll
        for (int c = 0; c < CIN; ++c) xv[c] = px[(size_t)c * HW];
        if (scale) {
            const float s = scale[row];
#pragma unroll
            for (int c = 0; c < CIN; ++c) xv[c] *= s;
        }
    }
}

template <int CIN, int COUT, bool NHWC>
__global__ __launch_bounds__(256) void point_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                        float* __restrict__ y, int Mx, int HW, int rows)
{
    constexpr int QPR = COUT / 4, RPB = 256 / QPR;                     // quads per row, rows per block
    const int q = threadIdx.x % QPR;
    float wr[4][CIN];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < CIN; ++c) wr[e][c] = w[(q * 4 + e) * CIN + c];
    const long long step = (long long)gridDim.x * RPB;
    for (long long r = (long long)blockIdx.x * RPB + threadIdx.x / QPR; r < rows; r += step) {
        const int row = (int)r;
        float xv[CIN];
        pc_load_row<CIN, NHWC>(xv, x, scale, row, Mx, HW);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CIN; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wr[e][c], xv[c], acc[e]);
        *reinterpret_cast<f4v*>(y + (size_t)row * COUT + q * 4) = f4v{acc[0], acc[1], acc[2], acc[3]};
    }
}

// one thread per pixel; x planar (the only form that takes a scale)
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void point_dscale_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ w,
                                                           float* __restrict__ dscale, int Mx, int HW, int rows)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int row = (int)r;
    float t[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) t[c] = 0.0f;
#pragma unroll
    for (int o = 0; o < COUT; o += 4) {
        const f4v g = *reinterpret_cast<const f4v*>(gy + (size_t)row * COUT + o);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < CIN; ++c) t[c] = fmaf(w[(o + e) * CIN + c], g[e], t[c]);
    }
    float xv[CIN];
    pc_load_row<CIN, false>(xv, x, nullptr, row, Mx, HW);
    float d = 0.0f;
#pragma unroll
    for (int c = 0; c < CIN; ++c) d = fmaf(xv[c], t[c], d);
    dscale[row] = d;
}

// thread (row, quad of input channels): 256 / (CIN / 4) rows per block
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void point_dx_kernel(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ dx, int rows)
{
    constexpr int QPR = CIN / 4, RPB = 256 / QPR;
    __shared__ __attribute__((aligned(16))) float wl[COUT * CIN];
    for (int i = threadIdx.x; i < COUT * CIN; i += 256) wl[i] = w[i];
    __syncthreads();
    const int q = threadIdx.x % QPR;
    const long long r = (long long)blockIdx.x * RPB + threadIdx.x / QPR;
    if (r >= rows) return;
    const float* pg = gy + (size_t)r * COUT;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int o = 0; o < COUT; o += 4) {
        const f4v g = *reinterpret_cast<const f4v*>(pg + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f4v wv = *reinterpret_cast<const f4v*>(wl + (o + e) * CIN + q * 4);
            acc[0] = fmaf(wv.x, g[e], acc[0]); acc[1] = fmaf(wv.y, g[e], acc[1]);
            acc[2] = fmaf(wv.z, g[e], acc[2]); acc[3] = fmaf(wv.w, g[e], acc[3]);
        }
    }
    *reinterpret_cast<f4v*>(dx + (size_t)r * CIN + q * 4) = f4v{acc[0], acc[1], acc[2], acc[3]};
}

// Block b: the rows [b . per, min(rows, (b + 1) . per)), one partial [COUT . CIN].  CPT input channels per thread in CS slots per output
// channel; a group of COUT . CS threads covers every accumulator once, and the 256 / (COUT . CS) groups take alternate rows of a tile.
template <int CIN, int COUT, bool NHWC>
__global__ __launch_bounds__(256) void point_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ scale,
                                                          float* __restrict__ part, int Mx, int HW, int rows, int per)
{
    constexpr int CPT = CIN == 16 ? 4 : 1;
    constexpr int CS = CIN == 16 ? 4 : (CIN == 3 ? 4 : 8);             // slots per output channel (CIN / CPT rounded up to a power of two)
    constexpr int XP = CS * CPT;                                       // floats of a staged input row
    constexpr int TPG = COUT * CS, G = 256 / TPG;
    constexpr int NACC = COUT * CIN;
    static_assert(TPG * G == 256 && CS * CPT >= CIN, "point_wgrad_kernel: thread map");
    __shared__ __attribute__((aligned(16))) float gt[PC_TILE * COUT];
    __shared__ __attribute__((aligned(16))) float xt[PC_TILE * XP];
    __shared__ float red[G > 1 ? G * NACC : 1];
    const int t = threadIdx.x, grp = t / TPG, l = t % TPG, o = l / CS, cs = l % CS;
    const bool active = CPT == 4 || cs < CIN;
    float acc[CPT];
#pragma unroll
    for (int e = 0; e < CPT; ++e) acc[e] = 0.0f;
    const long long first = (long long)blockIdx.x * per;
    const int row0 = (int)first, row1 = (int)(first + per < rows ? first + per : rows);
    for (int base = row0; base < row1; base += PC_TILE) {
        const int cnt = row1 - base < PC_TILE ? row1 - base : PC_TILE;
        __syncthreads();                                               // the previous tile is consumed
        for (int i = t; i < cnt * (COUT / 4); i += 256)                // gy rows are contiguous: a flat copy
            *reinterpret_cast<f4v*>(gt + i * 4) = *reinterpret_cast<const f4v*>(gy + (size_t)base * COUT + (size_t)i * 4);
        if constexpr (NHWC) {
            for (int i = t; i < cnt * (CIN / 4); i += 256)
                *reinterpret_cast<f4v*>(xt + i * 4) = *reinterpret_cast<const f4v*>(x + (size_t)base * CIN + (size_t)i * 4);
        } else {
            for (int i = t; i < CIN * PC_TILE; i += 256) {             // (c, r): neighbouring threads read neighbouring pixels
                const int c = i / PC_TILE, r = i % PC_TILE;
                if (r < cnt) {
                    const int row = base + r, m = row / HW, hw = row - m * HW;
                    float v = x[((size_t)(m % Mx) * CIN + c) * HW + hw];
                    if (scale) v *= scale[row];
                    xt[r * XP + c] = v;
                }
            }
        }
        __syncthreads();
        if (active) {
            for (int r = grp; r < cnt; r += G) {
                const float g = gt[r * COUT + o];
                if constexpr (CPT == 4) {
                    const f4v v = *reinterpret_cast<const f4v*>(xt + r * XP + cs * 4);
                    acc[0] = fmaf(g, v.x, acc[0]); acc[1] = fmaf(g, v.y, acc[1]); acc[2] = fmaf(g, v.z, acc[2]); acc[3] = fmaf(g, v.w, acc[3]);
                } else {
                    acc[0] = fmaf(g, xt[r * XP + cs], acc[0]);
                }
            }
        }
    }
    float* po = part + (size_t)blockIdx.x * NACC;
    if constexpr (G == 1) {
#pragma unroll
        for (int e = 0; e < CPT; ++e) po[o * CIN + cs * CPT + e] = acc[e];
    } else {
        if (active) red[grp * NACC + o * CIN + cs] = acc[0];
        __syncthreads();
        for (int i = t; i < NACC; i += 256) {
            float v = red[i];
#pragma unroll
            for (int g = 1; g < G; ++g) v += red[g * NACC + i];        // the groups in order
            po[i] = v;
        }
    }
}

template <int NACC>
__global__ __launch_bounds__(256) void point_wgrad_finish_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ dw)
{
    chunk_sums<NACC, NACC>(part, nchunk, dw, nullptr);
}

template <int CIN, int COUT, bool NHWC>
int point_fwd(const float* x, const float* w, const float* scale, float* y, int Mx, int HW, const PointPlan& p, hipStream_t s)
{
    constexpr int RPB = 256 / (COUT / 4);
    const long long nb = ((long long)p.rows + RPB - 1) / RPB;
    hipLaunchKernelGGL((point_fwd_kernel<CIN, COUT, NHWC>), dim3((unsigned)(nb < PC_FWD_BLOCKS ? nb : PC_FWD_BLOCKS)), dim3(256), 0, s, x, w, scale, y,
                       Mx, HW, p.rows);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

template <int CIN, int COUT, bool NHWC>
int point_bwd(const float* gy, const float* x, const float* w, const float* scale, float* dx, float* dw, float* dscale, int Mx, int HW,
              const PointPlan& p, float* part, hipStream_t s)
{
    if constexpr (CIN == 3) {                                          // the only form with a scale
        if (dscale) {
            hipLaunchKernelGGL((point_dscale_kernel<CIN, COUT>), dim3((unsigned)(((long long)p.rows + 255) / 256)), dim3(256), 0, s, gy, x, w, dscale,
                               Mx, HW, p.rows);
            OMNI_HIP(hipGetLastError());
        }
    } else if constexpr (NHWC) {                                       // the only form with a dx
        if (dx) {
            constexpr int RPB = 256 / (CIN / 4);
            hipLaunchKernelGGL((point_dx_kernel<CIN, COUT>), dim3((unsigned)(((long long)p.rows + RPB - 1) / RPB)), dim3(256), 0, s, gy, w, dx, p.rows);
            OMNI_HIP(hipGetLastError());
        }
    }
    if (dw) {
        hipLaunchKernelGGL((point_wgrad_kernel<CIN, COUT, NHWC>), dim3((unsigned)p.nchunk), dim3(256), 0, s, gy, x, scale, part, Mx, HW, p.rows, p.per);
        OMNI_HIP(hipGetLastError());
        hipLaunchKernelGGL((point_wgrad_finish_kernel<CIN * COUT>), dim3((CIN * COUT + 15) / 16), dim3(256), 0, s, (const float*)part, p.nchunk, dw);
        OMNI_HIP(hipGetLastError());
    }
    return OMNI_OK;
}

// the checks the forward and the backward share; `who` opens the message
int point_check(const char* who, int Mx, int M, int HW, int Cin, int Cout, const float* scale, PointPlan& p)
{
    const std::string head = std::string(who) + ": ";
    if (!point_form(Cin, Cout)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, head + "only 3 -> 16, 5 -> 16 and 16 -> 64 channels are built");
    if (Mx <= 0 || M <= 0 || HW <= 0 || M % Mx) OMNI_FAIL(OMNI_ERR_INVALID, head + "Mx, M, HW >= 1 and M a multiple of Mx");
    if (Cin != 3 && (scale || M != Mx)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, head + "only the 3 -> 16 form takes a scale or a broadcast x");
    if (!point_plan(M, HW, p)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, head + "tensor too large for 32-bit row indices");
    return OMNI_OK;
}

}  // namespace

extern "C" int omni_point_conv_fwd_f32(const float* x, const float* w, const float* scale, float* y, int Mx, int M, int HW, int Cin, int Cout,
                                       omni_stream_t stream)
{
    if (!x || !w || !y) OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_fwd: null pointer");
    PointPlan p;
    if (const int rc = point_check("omni_point_conv_fwd", Mx, M, HW, Cin, Cout, scale, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (Cin == 3) return point_fwd<3, 16, false>(x, w, scale, y, Mx, HW, p, s);
    if (Cin == 5) return point_fwd<5, 16, false>(x, w, nullptr, y, Mx, HW, p, s);
    return point_fwd<16, 64, true>(x, w, nullptr, y, Mx, HW, p, s);
}

extern "C" size_t omni_point_conv_bwd_workspace_bytes(int M, int HW, int Cin, int Cout)
{
    PointPlan p;
    if (!point_form(Cin, Cout) || !point_plan(M, HW, p)) return 0;
    return (size_t)p.nchunk * Cin * Cout * sizeof(float);
}

extern "C" int omni_point_conv_bwd_f32(const float* gy, const float* x, const float* w, const float* scale, float* dx, float* dw, float* dscale,
                                       int Mx, int M, int HW, int Cin, int Cout, void* workspace, size_t ws_bytes, omni_stream_t stream)
{
    if (!gy || !w) OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_bwd: null pointer");
    if (!dx && !dw && !dscale) OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_bwd: no gradient requested");
    PointPlan p;
    if (const int rc = point_check("omni_point_conv_bwd", Mx, M, HW, Cin, Cout, scale, p)) return rc;
    if (dx && Cin != 16) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_point_conv_bwd: dx is built for the 16 -> 64 form only (the rays are constants)");
    if (dscale && !scale) OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_bwd: dscale without a scale");
    if ((dw || dscale) && !x) OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_bwd: the weight and scale gradients read x");
    if (dw && (!workspace || ws_bytes < (size_t)p.nchunk * Cin * Cout * sizeof(float)))
        OMNI_FAIL(OMNI_ERR_INVALID, "omni_point_conv_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    if (Cin == 3) return point_bwd<3, 16, false>(gy, x, w, scale, nullptr, dw, dscale, Mx, HW, p, part, s);
    if (Cin == 5) return point_bwd<5, 16, false>(gy, x, w, nullptr, nullptr, dw, nullptr, Mx, HW, p, part, s);
    return point_bwd<16, 64, true>(gy, x, w, nullptr, dx, dw, nullptr, Mx, HW, p, part, s);
}
