// omni_dibr.hip — depth-image-based rendering (DIBR) of a panorama from a displaced viewpoint, gfx950 only.
//
//   omni_splat_render_f32   supervision/splatting.py:73-80 `render(img, depth, coords, max_depth)`: forward bilinear splat of
//                           img * w and of w (w = 1 / exp(2 depth / max_depth)), then recon = acc / wacc, mask = wacc > 1e-3
//   omni_dibr_f32           util.py:384-413 `dibr_vertical` / `dibr_horizontal`: the same splat, the target coordinates evaluated
//                           in registers from depth, sgrid and uvgrid (spherical/derivatives.py:53-71,93-105,168-177)
//   omni_*_wt_f32           the same forwards, also writing the splatted weight sum Wt [B,1,H,W] (what the backward needs)
//   omni_splat_render_bwd_f32 / omni_dibr_bwd_f32   the backwards: a gather, no atomics (DESIGN.md §11 "Backward")
//
// Determinism: the reference accumulates with fp32 scatter_add, whose sum depends on the order of arrival.  Here every
// contribution x is rounded ONCE to a fixed-point integer q = rint(x * 2^s) and added with a 64-bit integer atomic
// (global_atomic_add_x2, no return): integer addition is associative, so the sums are the same bits in any order — run to run, under
// graph replay, and for a batch against its items one at a time (s is chosen per batch item, from that item's data only).
//
// Scale: a pre-pass stores, per batch item, max |img * w| and max w over the finite values (as uint bits: non-negative floats order
// like their bits).  With e = ceil(log2 max) and L = ceil(log2 (H*W)), s = 62 - L - e.  Every |q| <= 2^(62-L), a target receives at
// most one contribution per source pixel (a source's four corners are distinct pixels), so no sum can exceed 2^62.  At 512 x 1024 and
// max w = 1 the weight resolution is 2^-43.
//
// Non-finite values: a source whose weight is not finite poisons the targets it reaches (recon NaN, mask 0); a source whose img * w is
// not finite poisons them for recon only.  The reference propagates inf / NaN through its float sums instead.
// Sources whose coordinates are not finite are dropped (render only: the DIBR modes clean their coordinates as the reference does).
#include "omni_internal.h"
#include "omni_fixedpoint.h"   // finite, dibr_exponent, pow2f, fixq, dibr_zero_kernel
#include "omni_reduce.h"       // block_reduce

namespace {

constexpr int DIBR_RENDER = -1, DIBR_VERTICAL = 0, DIBR_HORIZONTAL = 1;

__device__ __forceinline__ float dibr_weight(float depth, float max_depth)
{
    return 1.0f / expf(2.0f * depth / max_depth);                   // splatting.py:68-70, IEEE division
}

// ---------------------------------------------------------------- pass 1: per-item scale
__global__ __launch_bounds__(256) void dibr_max_kernel(const float* __restrict__ img, const float* __restrict__ depth, float max_depth,
                                                       int C, size_t HW, unsigned* __restrict__ maxbits /* [2][B] */)
{
    const int b = blockIdx.y, B = gridDim.y;
    float mi = 0.0f, mw = 0.0f;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
        const float w = dibr_weight(depth[(size_t)b * HW + p], max_depth);
        if (!finite(w)) continue;
        mw = fmaxf(mw, w);
        for (int c = 0; c < C; ++c) {
            const float v = img[((size_t)b * C + c) * HW + p] * w;
            if (finite(v)) mi = fmaxf(mi, fabsf(v));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mi = fmaxf(mi, __shfl_xor(mi, o)); mw = fmaxf(mw, __shfl_xor(mw, o)); }
    __shared__ float part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = mi; part[1][threadIdx.x >> 6] = mw; }
    __syncthreads();
    if (threadIdx.x == 0) {                                          // one atomic pair per block (same-address atomics serialise)
        atomicMax(maxbits + b, __float_as_uint(fmaxf(fmaxf(part[0][0], part[0][1]), fmaxf(part[0][2], part[0][3]))));
        atomicMax(maxbits + B + b, __float_as_uint(fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]))));
    }
}

// ---------------------------------------------------------------- pass 2: the splat
// A block takes a tile of TILE_R x 64 source pixels of one batch item (a row across the lanes of a wave, TILE_R / 4 rows per wave).
// The targets of a tile usually fall in a small box (DIBR displacements are smooth): when the box of all surviving corners fits
// DIBR_WIN int64 words per channel set, the block sums into LDS (ds_add_u64) and then adds each touched target to global memory once
// (one 64-bit atomic per target and channel instead of one per corner and channel).  Otherwise (a tile across the seam wrap, noisy
// depth) every contribution goes straight to a global atomic.  Either way the integer sums are the same bits.
constexpr int TILE_R = 16, TILE_C = 64, DIBR_WIN = 6144;            // 48 KiB of LDS per block

struct Src { float cw[4], w; int u0, v0, live; };

// What the backward needs on top of Src: the four 1-D weights (0 where the corner is off the image), d weight / d coordinate of each
// (-1, +1 or 0) and d u / d depth, d v / d depth of the DIBR modes with the reference's gates (a cleaned-up or clamped displacement
// passes no gradient); `dead`: depth == 0 or a non-finite raw displacement — the depth gradient is 0 there.
struct SrcGrad { float uw[2], vw[2], duw[2], dvw[2], du_dd, dv_dd; int dead; };

template <int MODE, bool GRAD = false>
__device__ __forceinline__ Src dibr_source(const float* __restrict__ depth, const float* __restrict__ coords, const float* __restrict__ uvgrid,
                                           const float* __restrict__ sgrid, int grid_batched, float baseline, float max_depth,
                                           int b, int H, int W, size_t HW, size_t p, SrcGrad* sg = nullptr)
{
    Src r;
    r.live = 0;
    if (GRAD) {
        sg->du_dd = sg->dv_dd = 0.0f; sg->dead = 0;
        sg->uw[0] = sg->uw[1] = sg->vw[0] = sg->vw[1] = sg->duw[0] = sg->duw[1] = sg->dvw[0] = sg->dvw[1] = 0.0f;
    }
    const float d = depth[(size_t)b * HW + p];
    float u, v;
    if (MODE == DIBR_RENDER) {
        u = coords[((size_t)b * 2) * HW + p];
        v = coords[((size_t)b * 2 + 1) * HW + p];
        if (!finite(u) || !finite(v)) return r;                     // undefined in the reference (an out-of-range scatter index): dropped
    } else {
        const size_t g = (grid_batched ? (size_t)b * 2 * HW : 0) + p;
        const float hs = (float)((double)H / 3.14159265358979323846);     // fp32(h / numpy.pi), derivatives.py:65,103,175
        const float th = sgrid[g + HW];
        if (MODE == DIBR_VERTICAL) {
            float dth = cosf(th) * baseline / d * hs;                // :168-177, torch's op order
            if (GRAD) { sg->dead = !finite(dth) || d == 0.0f; sg->dv_dd = sg->dead ? 0.0f : -dth / d; }
            if (!finite(dth)) dth = 0.0f;                            // NaN and +-inf -> 0
            u = uvgrid[g];
            v = uvgrid[g + HW] + dth;
        } else {
            const float ph = sgrid[g], fH = (float)H;
            float dph = sinf(ph) / (d * cosf(th)) * baseline * hs;   // :53-71 (clip variant): clamp(-h, h), then NaN -> 0
            float dth = cosf(ph) * sinf(th) * baseline / d * hs;     // :93-105: clamp(0, h); a NaN stays (torch.clamp propagates it)
            if (GRAD) {                                              // clamp passes the gradient inside [min, max] (bounds included)
                sg->dead = !finite(dph) || !finite(dth) || d == 0.0f;
                sg->du_dd = (!sg->dead && dph >= -fH && dph <= fH) ? -dph / d : 0.0f;
                sg->dv_dd = (!sg->dead && dth >= 0.0f && dth <= fH) ? -dth / d : 0.0f;
            }
            dph = dph != dph ? 0.0f : fminf(fmaxf(dph, -fH), fH);
            if (dth == dth) dth = fminf(fmaxf(dth, 0.0f), fH);
            u = uvgrid[g] + dph;
            v = uvgrid[g + HW] + dth;
            u = fmodf(u + 512.0f, 512.0f);                            // util.py:409: the literal 512, not W
        }
        if (GRAD) { if (!finite(u)) sg->du_dd = 0.0f; if (!finite(v)) sg->dv_dd = 0.0f; }
        if (!finite(u)) u = 0.0f;                                    // util.py:395-396,410-411: absolute 0, not zero displacement
        if (!finite(v)) v = 0.0f;
    }
    // splatting.py:9-44
    const float u0 = floorf(u), v0 = floorf(v), u1 = u0 + 1.0f, v1 = v0 + 1.0f;
    const bool iu0 = u0 >= 0.0f && u0 <= (float)(W - 1), iu1 = u1 >= 0.0f && u1 <= (float)(W - 1);
    const bool iv0 = v0 >= 0.0f && v0 <= (float)(H - 1), iv1 = v1 >= 0.0f && v1 <= (float)(H - 1);
    const float u0w = iu0 ? u1 - u : 0.0f, u1w = iu1 ? u - u0 : 0.0f;
    const float v0w = iv0 ? v1 - v : 0.0f, v1w = iv1 ? v - v0 : 0.0f;
    r.cw[0] = u0w * v0w; r.cw[1] = u1w * v0w; r.cw[2] = u0w * v1w; r.cw[3] = u1w * v1w;
    if (GRAD) {
        sg->uw[0] = u0w; sg->uw[1] = u1w; sg->vw[0] = v0w; sg->vw[1] = v1w;
        sg->duw[0] = iu0 ? -1.0f : 0.0f; sg->duw[1] = iu1 ? 1.0f : 0.0f;
        sg->dvw[0] = iv0 ? -1.0f : 0.0f; sg->dvw[1] = iv1 ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!(r.cw[k] >= 1e-3f)) r.cw[k] = 0.0f;                     // weight_threshold, :40-44
        r.live |= r.cw[k] != 0.0f;
    }
    if (r.live) {                                                    // a surviving corner lies inside the image: these ints are in range
        r.u0 = (int)fmaxf(u0, -1.0f);
        r.v0 = (int)fmaxf(v0, -1.0f);
    }
    r.w = dibr_weight(d, max_depth);
    return r;
}

template <int MODE>
__global__ __launch_bounds__(256) void dibr_splat_kernel(const float* __restrict__ img, const float* __restrict__ depth,
                                                         const float* __restrict__ coords, const float* __restrict__ uvgrid,
                                                         const float* __restrict__ sgrid, int grid_batched, float baseline, float max_depth,
                                                         int B, int C, int H, int W, int log2hw, int tiles_c, const unsigned* __restrict__ maxbits,
                                                         unsigned long long* __restrict__ acc /* [B][C+1][H][W] */,
                                                         unsigned* __restrict__ poison /* [B][H][W] */)
{
    __shared__ unsigned long long win[DIBR_WIN];
    __shared__ int red[4];
    constexpr int SPT = TILE_R / 4;                                  // source rows per thread
    const size_t HW = (size_t)H * W;
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = (int)(blockIdx.x % tiles_c) * TILE_C + lane;
    const int y0 = (int)(blockIdx.x / tiles_c) * TILE_R + wv * SPT;
    Src src[SPT];
    int rmin = 1 << 30, rmax = -1, cmin = 1 << 30, cmax = -1;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        src[j].live = 0;
        if (x < W && y0 + j < H)
            src[j] = dibr_source<MODE>(depth, coords, uvgrid, sgrid, grid_batched, baseline, max_depth, b, H, W, HW, (size_t)(y0 + j) * W + x);
        if (src[j].live) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (src[j].cw[k] != 0.0f) {
                    const int r = src[j].v0 + (k >> 1), c = src[j].u0 + (k & 1);
                    rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
                }
        }
    }
    rmin = block_reduce(rmin, false, red); rmax = block_reduce(rmax, true, red);
    cmin = block_reduce(cmin, false, red); cmax = block_reduce(cmax, true, red);
    if (rmax < 0) return;                                            // no surviving corner in the whole tile (block-uniform)
    const int R = rmax - rmin + 1, Cc = cmax - cmin + 1, box = R * Cc;
#ifdef OMNI_DIBR_NO_LDS
    const bool use_lds = false;                                      // (A/B build for tools/dibr_bench.py: global atomics only)
#else
    const bool use_lds = (long long)box * (C + 1) <= DIBR_WIN;        // block-uniform
#endif

    const int L = log2hw;
    const float sc_w = pow2f(62 - L - dibr_exponent(maxbits[B + b]));
    const float sc_i = pow2f(62 - L - dibr_exponent(maxbits[b]));
    if (use_lds) {
        for (int e = threadIdx.x; e < box * (C + 1); e += 256) win[e] = 0ull;
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        if (!src[j].live) continue;
        const Src& sj = src[j];
        const size_t p = (size_t)(y0 + j) * W + x;
        int tgt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = sj.v0 + (k >> 1), c = sj.u0 + (k & 1);
            tgt[k] = use_lds ? (r - rmin) * Cc + (c - cmin) : r * W + c;
        }
        auto add = [&](int ch, int k, long long q) {
            if (q == 0) return;
            if (use_lds) atomicAdd(win + (size_t)ch * box + tgt[k], (unsigned long long)q);
            else atomicAdd(acc + ((size_t)b * (C + 1) + ch) * HW + tgt[k], (unsigned long long)q);   // two's complement: signed sums wrap
        };
        unsigned pbits = 0;
        if (!finite(sj.w)) {
            pbits = 3u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (sj.cw[k] != 0.0f) add(C, k, fixq(sj.w * sj.cw[k], sc_w));
            for (int c = 0; c < C; ++c) {
                const float xv = img[((size_t)b * C + c) * HW + p] * sj.w;   // splatting.py:76 img * weights, then * corner weight (:49-52)
                if (!finite(xv)) { pbits |= 1u; continue; }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (sj.cw[k] != 0.0f) add(c, k, fixq(xv * sj.cw[k], sc_i));
            }
        }
        if (pbits) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (sj.cw[k] != 0.0f) atomicOr(poison + (size_t)b * HW + (size_t)(sj.v0 + (k >> 1)) * W + (sj.u0 + (k & 1)), pbits);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int e = threadIdx.x; e < box; e += 256) {
            const int r = e / Cc, c = e - r * Cc;
            const size_t t = (size_t)(rmin + r) * W + (cmin + c);
            for (int ch = 0; ch <= C; ++ch) {
                const unsigned long long q = win[(size_t)ch * box + e];
                if (q) atomicAdd(acc + ((size_t)b * (C + 1) + ch) * HW + t, q);
            }
        }
    }
}

// ---------------------------------------------------------------- pass 3: int64 sums -> recon, mask (splatting.py:63-66,78-79)
__global__ __launch_bounds__(256) void dibr_normalise_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ poison,
                                                             const unsigned* __restrict__ maxbits, int B, int C, size_t HW, int log2hw,
                                                             float* __restrict__ recon, unsigned char* __restrict__ mask,
                                                             float* __restrict__ wt /* nullable: the weight sum, for the backward */)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const int b = (int)(i / HW);
    const size_t p = i - (size_t)b * HW;
    const unsigned pb = poison[i];
    const float inv_w = pow2f(-(62 - log2hw - dibr_exponent(maxbits[B + b])));
    const float inv_i = pow2f(-(62 - log2hw - dibr_exponent(maxbits[b])));
    const float wsum = (float)acc[((size_t)b * (C + 1) + C) * HW + p] * inv_w;
    const float den = wsum + (wsum <= 1e-8f ? 1e-8f : 0.0f);         // weights + epsilon * (weights <= epsilon)
    for (int c = 0; c < C; ++c) {
        const float a = (float)acc[((size_t)b * (C + 1) + c) * HW + p] * inv_i;
        recon[((size_t)b * C + c) * HW + p] = pb ? __int_as_float(0x7fc00000) : a / den;
    }
    if (mask) mask[i] = (wsum > 1e-3f && !(pb & 2u)) ? 1 : 0;
    if (wt) wt[i] = (pb & 2u) ? __int_as_float(0x7fc00000) : wsum;
}

// ---------------------------------------------------------------- backward (DESIGN.md §11 "Backward")
// recon_c[t] = S_c[t] / den[t], S_c[t] = sum c_ik w_i img_ic, Wt[t] = sum c_ik w_i.  With G = dL/drecon:
//   A_c[t] = G_c[t] / den[t]  (= dL/dS_c)         Bt[t] = -sum_c G_c[t] recon_c[t] / den[t]  (= dL/dWt)
// Pass 1 writes them as ONE record of RS = roundup4(C + 1) floats per target (A_0 .. A_{C-1}, Bt, padding): the gather of pass 2 then
// costs one 16-byte read per corner at C = 3 instead of 2 C + 1 four-byte ones.
__global__ __launch_bounds__(256) void dibr_bwd_prep_kernel(const float* __restrict__ G, const float* __restrict__ recon, const float* __restrict__ wt,
                                                            int B, int C, size_t HW, int RS, float* __restrict__ rec /* [B][HW][RS] */)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const int b = (int)(i / HW);
    const size_t p = i - (size_t)b * HW;
    const float wsum = wt[i];
    const float den = wsum + (wsum <= 1e-8f ? 1e-8f : 0.0f);
    float* r = rec + i * RS;
    float bt = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float g = G[((size_t)b * C + c) * HW + p];
        r[c] = g / den;
        bt -= g * recon[((size_t)b * C + c) * HW + p] / den;
    }
    r[C] = bt;
    for (int c = C + 1; c < RS; ++c) r[c] = 0.0f;
}

// Pass 2: one thread per SOURCE pixel (a block = 4 rows x 64 columns of one item).  It re-derives its corners with dibr_source — the
// function the forward splat uses, so both agree on which corners survived — reads the records of at most four targets and writes its
// own gradients: nothing is accumulated across threads, so there are no atomics and the summation order is a constant.
template <int MODE>
__global__ __launch_bounds__(256) void dibr_bwd_gather_kernel(const float* __restrict__ img, const float* __restrict__ depth,
                                                              const float* __restrict__ coords, const float* __restrict__ uvgrid,
                                                              const float* __restrict__ sgrid, int grid_batched, float baseline, float max_depth,
                                                              int C, int H, int W, int tiles_c, int RS, const float* __restrict__ rec,
                                                              float* __restrict__ gimg, float* __restrict__ gdepth, float* __restrict__ gcoords)
{
    const size_t HW = (size_t)H * W;
    const int b = blockIdx.y;
    const int x = (int)(blockIdx.x % tiles_c) * TILE_C + (threadIdx.x & 63);
    const int y = (int)(blockIdx.x / tiles_c) * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    SrcGrad sg;
    const Src s = dibr_source<MODE, true>(depth, coords, uvgrid, sgrid, grid_batched, baseline, max_depth, b, H, W, HW, p, &sg);
    if (!s.live) {                                                   // no surviving corner: this source reached nothing
        if (gimg) for (int c = 0; c < C; ++c) gimg[((size_t)b * C + c) * HW + p] = 0.0f;
        if (gdepth) gdepth[(size_t)b * HW + p] = 0.0f;
        if (gcoords) { gcoords[((size_t)b * 2) * HW + p] = 0.0f; gcoords[((size_t)b * 2 + 1) * HW + p] = 0.0f; }
        return;
    }
    const float* rk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        rk[k] = (s.cw[k] != 0.0f) ? rec + ((size_t)b * HW + (size_t)(s.v0 + (k >> 1)) * W + (s.u0 + (k & 1))) * RS : nullptr;
    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};                          // q_ik = sum_c img_ic A_c[t_ik] + Bt[t_ik]
    const bool need_q = gdepth || gcoords;
    if (RS == 4) {                                                   // C <= 3: the whole record is one 16-byte read
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = rk[k] ? *(const float4*)rk[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int c = 0; c < C; ++c) {
            float a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = c == 0 ? v[k].x : (c == 1 ? v[k].y : v[k].z);
            if (gimg) gimg[((size_t)b * C + c) * HW + p] = s.w * (((s.cw[0] * a[0] + s.cw[1] * a[1]) + s.cw[2] * a[2]) + s.cw[3] * a[3]);
            if (need_q) {
                const float iv = img[((size_t)b * C + c) * HW + p];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] += iv * a[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] += C == 1 ? v[k].y : (C == 2 ? v[k].z : v[k].w);
    } else {
        for (int c = 0; c < C; ++c) {
            float a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = rk[k] ? rk[k][c] : 0.0f;
            if (gimg) gimg[((size_t)b * C + c) * HW + p] = s.w * (((s.cw[0] * a[0] + s.cw[1] * a[1]) + s.cw[2] * a[2]) + s.cw[3] * a[3]);
            if (need_q) {
                const float iv = img[((size_t)b * C + c) * HW + p];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] += iv * a[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] += rk[k] ? rk[k][C] : 0.0f;
    }
    if (!need_q) return;
    float gw = 0.0f, gu = 0.0f, gv = 0.0f;                           // dL/dw_i, dL/du_i, dL/dv_i
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!rk[k]) continue;                                        // a dropped corner is a constant 0 (its gate is detached)
        gw += s.cw[k] * q[k];
        const float gc = s.w * q[k];                                 // dL/dc_ik
        gu += gc * (sg.duw[k & 1] * sg.vw[k >> 1]);
        gv += gc * (sg.uw[k & 1] * sg.dvw[k >> 1]);
    }
    if (gcoords) {
        gcoords[((size_t)b * 2) * HW + p] = gu;
        gcoords[((size_t)b * 2 + 1) * HW + p] = gv;
    }
    if (gdepth) {
        float gd = -(2.0f / max_depth) * s.w * gw;                   // through w = 1 / exp(2 d / max_depth)
        if (MODE != DIBR_RENDER) gd = sg.dead ? 0.0f : (gd + gu * sg.du_dd) + gv * sg.dv_dd;
        gdepth[(size_t)b * HW + p] = gd;
    }
}

struct WsLayout { size_t hdr, acc, poison, total; };

WsLayout ws_layout(int B, int C, int H, int W)
{
    WsLayout l;
    const size_t n = (size_t)B * H * W;
    l.hdr = 0;
    l.acc = ((size_t)2 * B * sizeof(unsigned) + 255) / 256 * 256;
    l.poison = l.acc + sizeof(long long) * (size_t)(C + 1) * n;
    l.total = (l.poison + sizeof(unsigned) * n + 255) / 256 * 256;
    return l;
}

int dibr_run(int mode, const float* img, const float* depth, const float* coords, const float* uvgrid, const float* sgrid, int grid_batched,
             float baseline, float max_depth, float* recon, unsigned char* mask, float* wt, int B, int C, int H, int W, void* workspace,
             hipStream_t s, const char* what)
{
    if (!img || !depth || !recon || !workspace || (mode == DIBR_RENDER ? !coords : (!uvgrid || !sgrid)))
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (B < 1 || C < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30) || (long long)B * H * W > (1ll << 31) - 1)
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": bad shape");
    if (!(max_depth > 0.0f) || !(max_depth <= 3.402823466e38f)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": max_depth must be finite and > 0");
    if (mode != DIBR_RENDER && !(fabsf(baseline) <= 3.402823466e38f)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": baseline must be finite");
    if ((uintptr_t)workspace & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": workspace must be 16-byte aligned");
    const WsLayout l = ws_layout(B, C, H, W);
    char* ws = (char*)workspace;
    unsigned* maxbits = (unsigned*)(ws + l.hdr);
    unsigned long long* acc = (unsigned long long*)(ws + l.acc);
    unsigned* poison = (unsigned*)(ws + l.poison);
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    int log2hw = 0;
    while ((1ull << log2hw) < HW) ++log2hw;
    // zeroed by a kernel (not hipMemsetAsync): the call is captured into graphs with the same meaning
    hipLaunchKernelGGL(dibr_zero_kernel, dim3(2048), dim3(256), 0, s, (uint4*)workspace, l.total / 16);
    const unsigned gx = (unsigned)((HW + 255) / 256 < 128 ? (HW + 255) / 256 : 128);   // enough waves in flight; 2 x 128 same-address atomics per item
    hipLaunchKernelGGL(dibr_max_kernel, dim3(gx, B), dim3(256), 0, s, img, depth, max_depth, C, HW, maxbits);
    const int tiles_c = (W + TILE_C - 1) / TILE_C, tiles = tiles_c * ((H + TILE_R - 1) / TILE_R);
    const dim3 sg(tiles, B);
    if (mode == DIBR_RENDER)
        hipLaunchKernelGGL(dibr_splat_kernel<DIBR_RENDER>, sg, dim3(256), 0, s, img, depth, coords, nullptr, nullptr, 0, 0.0f, max_depth,
                           B, C, H, W, log2hw, tiles_c, (const unsigned*)maxbits, acc, poison);
    else if (mode == DIBR_VERTICAL)
        hipLaunchKernelGGL(dibr_splat_kernel<DIBR_VERTICAL>, sg, dim3(256), 0, s, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline,
                           max_depth, B, C, H, W, log2hw, tiles_c, (const unsigned*)maxbits, acc, poison);
    else
        hipLaunchKernelGGL(dibr_splat_kernel<DIBR_HORIZONTAL>, sg, dim3(256), 0, s, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline,
                           max_depth, B, C, H, W, log2hw, tiles_c, (const unsigned*)maxbits, acc, poison);
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dibr_normalise_kernel, dim3(g), dim3(256), 0, s, (const long long*)acc, (const unsigned*)poison, (const unsigned*)maxbits,
                       B, C, HW, log2hw, recon, mask, wt);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

int dibr_bwd_run(int mode, const float* grad_recon, const float* recon, const float* wt, const float* img, const float* depth, const float* coords,
                 const float* uvgrid, const float* sgrid, int grid_batched, float baseline, float max_depth, float* gimg, float* gdepth,
                 float* gcoords, int B, int C, int H, int W, void* workspace, hipStream_t s, const char* what)
{
    if (!grad_recon || !recon || !wt || !img || !depth || !workspace || (mode == DIBR_RENDER ? !coords : (!uvgrid || !sgrid)))
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (!gimg && !gdepth && !gcoords) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": no gradient requested");
    if (B < 1 || C < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30) || (long long)B * H * W > (1ll << 31) - 1)
        OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": bad shape");
    if (!(max_depth > 0.0f) || !(max_depth <= 3.402823466e38f)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": max_depth must be finite and > 0");
    if (mode != DIBR_RENDER && !(fabsf(baseline) <= 3.402823466e38f)) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": baseline must be finite");
    if ((uintptr_t)workspace & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": workspace must be 16-byte aligned");
    const size_t HW = (size_t)H * W, n = (size_t)B * HW;
    const int RS = (C + 1 + 3) & ~3;
    float* rec = (float*)workspace;
    hipLaunchKernelGGL(dibr_bwd_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grad_recon, recon, wt, B, C, HW, RS, rec);
    const int tiles_c = (W + TILE_C - 1) / TILE_C, tiles = tiles_c * ((H + 3) / 4);
    const dim3 sgd(tiles, B);
    if (mode == DIBR_RENDER)
        hipLaunchKernelGGL(dibr_bwd_gather_kernel<DIBR_RENDER>, sgd, dim3(256), 0, s, img, depth, coords, nullptr, nullptr, 0, 0.0f, max_depth,
                           C, H, W, tiles_c, RS, (const float*)rec, gimg, gdepth, gcoords);
    else if (mode == DIBR_VERTICAL)
        hipLaunchKernelGGL(dibr_bwd_gather_kernel<DIBR_VERTICAL>, sgd, dim3(256), 0, s, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline,
                           max_depth, C, H, W, tiles_c, RS, (const float*)rec, gimg, gdepth, nullptr);
    else
        hipLaunchKernelGGL(dibr_bwd_gather_kernel<DIBR_HORIZONTAL>, sgd, dim3(256), 0, s, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline,
                           max_depth, C, H, W, tiles_c, RS, (const float*)rec, gimg, gdepth, nullptr);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

}  // namespace

extern "C" size_t omni_dibr_workspace_bytes(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return ws_layout(B, C, H, W).total;
}

extern "C" int omni_splat_render_f32(const float* img, const float* depth, const float* coords, float max_depth, float* recon, unsigned char* mask,
                                     int B, int C, int H, int W, void* workspace, omni_stream_t stream)
{
    return dibr_run(DIBR_RENDER, img, depth, coords, nullptr, nullptr, 0, 0.0f, max_depth, recon, mask, nullptr, B, C, H, W, workspace,
                    (hipStream_t)stream, "omni_splat_render_f32");
}

extern "C" int omni_splat_render_wt_f32(const float* img, const float* depth, const float* coords, float max_depth, float* recon, unsigned char* mask,
                                        float* wt, int B, int C, int H, int W, void* workspace, omni_stream_t stream)
{
    if (!wt) OMNI_FAIL(OMNI_ERR_INVALID, "omni_splat_render_wt_f32: null device pointer");
    return dibr_run(DIBR_RENDER, img, depth, coords, nullptr, nullptr, 0, 0.0f, max_depth, recon, mask, wt, B, C, H, W, workspace,
                    (hipStream_t)stream, "omni_splat_render_wt_f32");
}

extern "C" size_t omni_dibr_bwd_workspace_bytes(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return sizeof(float) * (size_t)((C + 1 + 3) & ~3) * B * H * W;
}

extern "C" int omni_splat_render_bwd_f32(const float* grad_recon, const float* recon, const float* wt, const float* img, const float* depth,
                                         const float* coords, float max_depth, float* grad_img, float* grad_depth, float* grad_coords,
                                         int B, int C, int H, int W, void* workspace, omni_stream_t stream)
{
    return dibr_bwd_run(DIBR_RENDER, grad_recon, recon, wt, img, depth, coords, nullptr, nullptr, 0, 0.0f, max_depth, grad_img, grad_depth,
                        grad_coords, B, C, H, W, workspace, (hipStream_t)stream, "omni_splat_render_bwd_f32");
}

extern "C" int omni_dibr_f32(const float* img, const float* depth, const float* uvgrid, const float* sgrid, int grid_batched, float baseline,
                             int mode, float* recon, unsigned char* mask, int B, int C, int H, int W, void* workspace, omni_stream_t stream)
{
    if (mode != DIBR_VERTICAL && mode != DIBR_HORIZONTAL) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_f32: mode must be 0 (vertical) or 1 (horizontal)");
    if (grid_batched != 0 && grid_batched != 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_f32: grid_batched must be 0 or 1");
    return dibr_run(mode, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline, 8.0f, recon, mask, nullptr, B, C, H, W, workspace,
                    (hipStream_t)stream, "omni_dibr_f32");
}

extern "C" int omni_dibr_wt_f32(const float* img, const float* depth, const float* uvgrid, const float* sgrid, int grid_batched, float baseline,
                                int mode, float* recon, unsigned char* mask, float* wt, int B, int C, int H, int W, void* workspace,
                                omni_stream_t stream)
{
    if (mode != DIBR_VERTICAL && mode != DIBR_HORIZONTAL) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_wt_f32: mode must be 0 (vertical) or 1 (horizontal)");
    if (grid_batched != 0 && grid_batched != 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_wt_f32: grid_batched must be 0 or 1");
    if (!wt) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_wt_f32: null device pointer");
    return dibr_run(mode, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline, 8.0f, recon, mask, wt, B, C, H, W, workspace,
                    (hipStream_t)stream, "omni_dibr_wt_f32");
}

extern "C" int omni_dibr_bwd_f32(const float* grad_recon, const float* recon, const float* wt, const float* img, const float* depth,
                                 const float* uvgrid, const float* sgrid, int grid_batched, float baseline, int mode, float* grad_img,
                                 float* grad_depth, int B, int C, int H, int W, void* workspace, omni_stream_t stream)
{
    if (mode != DIBR_VERTICAL && mode != DIBR_HORIZONTAL) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_bwd_f32: mode must be 0 (vertical) or 1 (horizontal)");
    if (grid_batched != 0 && grid_batched != 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_dibr_bwd_f32: grid_batched must be 0 or 1");
    return dibr_bwd_run(mode, grad_recon, recon, wt, img, depth, nullptr, uvgrid, sgrid, grid_batched, baseline, 8.0f, grad_img, grad_depth,
                        nullptr, B, C, H, W, workspace, (hipStream_t)stream, "omni_dibr_bwd_f32");
}
