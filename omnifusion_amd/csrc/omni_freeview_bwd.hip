// omni_freeview_bwd.hip — the backwards of free-view sampling (DESIGN.md §12 "Backward"): the transposes of the three gathers of
// omni_freeview.hip, as deterministic scatters.
//
//   omni_freeview_equi2pers_bwd_f32   grad_pers (either layout) -> grad_erp [B,C,H,W], summed over the N views
//   omni_freeview_pers2equi_bwd_f32   grad_erp [N,C,H,W] -> grad_pers [N,C,h,w], only where the view covers the ERP pixel
//   omni_freeview_merge_bwd_f32       grad_erp [B,C,H,W] -> grad_pers [B,N,C,h,w], once per covering view, scaled by 1 / max(count, 1)
//
// The operators are linear in the image and their coordinates depend on the geometry only, so a backward sends w_k * g through the tap
// set of the forward — the SAME device functions (omni_freeview_taps.h), so both agree on every corner, weight and mask bit.
//
// Summation: §11's scheme (omni_fixedpoint.h).  Four launches on the caller's stream into a caller-provided workspace — a kernel zeroes
// it; a max pass stores max |g| per item over its finite values; the scatter rounds each contribution once, q = rint(w_k g 2^s) with
// s = 62 - ceil(log2 S) - e (S sources per item; a target takes at most one contribution per source: a source's four corners are distinct
// pixels), and adds it with a 64-bit integer atomic; a last kernel converts the sums to fp32.  No allocation, no host synchronisation.
//
// A block owns a tile of source pixels of one view (four consecutive pixels of a row per thread, the coordinates computed once and applied
// to every plane) and reduces the bounding box of its corners on the target image: where planes x box fits FVB_WIN words it sums in LDS
// (ds_add_u64) and adds each touched target to global memory once, otherwise every contribution is a global atomic (option fv_bwd_lds = 0:
// always).  Both give the same integer sums.
//
// Non-finite g: one poison bit per target element.  A source whose g is not finite makes NaN every target it reaches through a corner
// that is on the image — zero-weight corners included, where the reference's autograd yields 0 * inf = NaN too — and nothing else.  A
// source outside pers2equi's mask reaches nothing, whatever its g.
#include <algorithm>

#include "omni_internal.h"
#include "omni_fixedpoint.h"
#include "omni_reduce.h"
#include "omni_freeview_taps.h"

namespace {

constexpr int FVB_E2P = 0, FVB_P2E = 1, FVB_MERGE = 2;
constexpr int FVB_WIN = 6144;                                        // int64 words of LDS per block (48 KiB)

struct FvbWs { size_t hdr, acc, poison, total; };

// images: target images of C planes of Ht x Wt pixels (B | N | B * N)
FvbWs fvb_layout(long long images, int C, int Ht, int Wt)
{
    const size_t n = (size_t)images * C * Ht * Wt;
    FvbWs l;
    l.hdr = ((size_t)images * sizeof(unsigned) + 255) / 256 * 256;      // max |g| bits, one word per item (items <= images)
    l.acc = l.hdr;
    l.poison = l.acc + sizeof(long long) * n;
    l.total = (l.poison + ((n + 31) / 32) * sizeof(unsigned) + 255) / 256 * 256;
    return l;
}

// pass 1: maxbits[item] = max |g| over the finite values of the item's `per` contiguous floats
__global__ __launch_bounds__(256) void fvb_max_kernel(const float* __restrict__ g, size_t per, unsigned* __restrict__ maxbits)
{
    const float* p = g + (size_t)blockIdx.y * per;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        const float v = p[i];
        if (finite(v)) m = fmaxf(m, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(maxbits + blockIdx.y, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}

struct FvbArgs {
    const float* g;                  // upstream gradient
    const float* rot;                // rot_fwd [N][9] (e2p) or rot_inv [N][18]
    unsigned long long* acc;         // [images][C][Ht][Wt]
    unsigned* poison;                // one bit per element of acc
    const unsigned* maxbits;         // [items]
    int C, N;
    int Hs, Ws, Ht, Wt;              // source image (the forward's output), target image (the forward's input)
    int groups, tgl, tiles_x, tiles; // groups of FV_PX pixels per source row; a tile is (1 << tgl) groups x (256 >> tgl) rows
    int L;                           // ceil(log2 sources per item)
    int concat, use_lds;
    float h_len, w_len;
};

// pass 2.  grid.x = N * tiles (a block never spans two views), grid.y = B (e2p, merge) or 1
template <int OP>
__global__ __launch_bounds__(256) void fvb_scatter_kernel(const FvbArgs a)
{
    __shared__ unsigned long long win[FVB_WIN];
    __shared__ int red[4];
    const int v = blockIdx.x / a.tiles, tile = blockIdx.x - v * a.tiles;
    const int b = blockIdx.y;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int g = (tx << a.tgl) + (threadIdx.x & ((1 << a.tgl) - 1));
    const int row = ty * (256 >> a.tgl) + (threadIdx.x >> a.tgl);
    const int j0 = g * FV_PX;
    const bool live = g < a.groups && row < a.Hs;
    const int Ht = a.Ht, Wt = a.Wt, C = a.C;

    int off[FV_PX][4], valid[FV_PX];
    float wt[FV_PX][4], scale[FV_PX];
    int rmin = 1 << 30, rmax = -1, cmin = 1 << 30, cmax = -1;
#pragma unroll
    for (int k = 0; k < FV_PX; ++k) {
        valid[k] = 0;
        scale[k] = 1.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) { off[k][q] = 0; wt[k][q] = 0.0f; }
        if (!live || j0 + k >= a.Ws) continue;
        FvTap t;
        if (OP == FVB_E2P) {
            t = fv_e2p_tap(a.rot + (size_t)v * 9, a.h_len, a.w_len, a.Hs, a.Ws, row, j0 + k, Ht, Wt);
        } else {
            const FvRay ray = fv_erp_ray(a.Hs, a.Ws, row, j0 + k);
            if (!fv_p2e_tap(a.rot + (size_t)v * 18, ray, a.h_len, a.w_len, Ht, Wt, t)) continue;      // outside the mask: reaches nothing
            if (OP == FVB_MERGE) {
                // the forward's count, from the same mask bits; evaluated only for a pixel THIS view covers, so an ERP pixel costs
                // N + count * N frustum tests over all its view blocks (count is 1 - 3 for tangent or cube layouts), not N * N
                int cnt = 0;
                float fy, fz;
                for (int u = 0; u < a.N; ++u) cnt += fv_p2e_frustum(a.rot + (size_t)u * 18, ray, a.h_len, a.w_len, fy, fz) ? 1 : 0;
                scale[k] = (float)max(cnt, 1);
            }
        }
        valid[k] = t.valid;
        off[k][0] = t.o00; off[k][1] = t.o01; off[k][2] = t.o10; off[k][3] = t.o11;
        wt[k][0] = t.w00; wt[k][1] = t.w01; wt[k][2] = t.w10; wt[k][3] = t.w11;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (valid[k] >> q & 1) {
                const int r = off[k][q] / Wt, c = off[k][q] - r * Wt;
                rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
            }
    }
    rmin = block_reduce(rmin, false, red); rmax = block_reduce(rmax, true, red);
    cmin = block_reduce(cmin, false, red); cmax = block_reduce(cmax, true, red);
    if (rmax < 0) return;                                            // no corner on the image in the whole tile (block-uniform)
    const int Cc = cmax - cmin + 1;
    const long long box = (long long)(rmax - rmin + 1) * Cc;
    const bool use_lds = a.use_lds && box <= FVB_WIN;                // block-uniform
    const int ppr = use_lds ? min(C, (int)(FVB_WIN / box)) : C;      // planes per LDS round
    if (use_lds) {
#pragma unroll
        for (int k = 0; k < FV_PX; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (valid[k] >> q & 1) {
                    const int r = off[k][q] / Wt, c = off[k][q] - r * Wt;
                    off[k][q] = (r - rmin) * Cc + (c - cmin);        // from here on: an offset into the box
                }
    }

    const size_t HWt = (size_t)Ht * Wt, HWs = (size_t)a.Hs * a.Ws;
    const int item = OP == FVB_P2E ? v : b;                          // whose max |g| scales the sums
    const size_t img = OP == FVB_E2P ? (size_t)b : OP == FVB_P2E ? (size_t)v : (size_t)b * a.N + v;      // target image
    const float sc = pow2f(62 - a.L - dibr_exponent(a.maxbits[item]));
    unsigned long long* accb = a.acc + img * C * HWt;
    // upstream gradient of plane 0 at (row, j0); plane stride gs
    size_t gs;
    const float* gp;
    if (OP == FVB_E2P) {
        if (a.concat) { gs = (size_t)a.Hs * a.N * a.Ws; gp = a.g + ((size_t)b * C * a.Hs + row) * ((size_t)a.N * a.Ws) + (size_t)v * a.Ws + j0; }
        else { gs = HWs; gp = a.g + ((size_t)b * a.N + v) * C * HWs + (size_t)row * a.Ws + j0; }
    } else {
        gs = HWs;
        gp = a.g + (size_t)(OP == FVB_P2E ? v : b) * C * HWs + (size_t)row * a.Ws + j0;
    }

    // off[][] as an offset into the target image again (the poison bits live in global memory on either path)
    auto image_offset = [&](int o) { return use_lds ? (rmin + o / Cc) * Wt + cmin + o % Cc : o; };

    for (int c0 = 0; c0 < C; c0 += ppr) {
        const int np = min(ppr, C - c0);
        if (use_lds) {
            for (int e = threadIdx.x; e < np * (int)box; e += 256) win[e] = 0ull;
            __syncthreads();
        }
        if (live) {
            for (int c = c0; c < c0 + np; ++c) {
#pragma unroll
                for (int k = 0; k < FV_PX; ++k) {
                    if (!valid[k]) continue;
                    float x = gp[(size_t)c * gs + k];
                    if (OP == FVB_MERGE) x = x / scale[k];
                    if (!finite(x)) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (valid[k] >> q & 1) {
                                const size_t e = (img * C + c) * HWt + image_offset(off[k][q]);
                                atomicOr(a.poison + (e >> 5), 1u << (e & 31));
                            }
                        continue;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (valid[k] >> q & 1) {
                            const long long qv = fixq(wt[k][q] * x, sc);
                            if (qv == 0) continue;
                            if (use_lds) atomicAdd(win + (size_t)(c - c0) * box + off[k][q], (unsigned long long)qv);
                            else atomicAdd(accb + (size_t)c * HWt + off[k][q], (unsigned long long)qv);      // two's complement: signed sums wrap
                        }
                }
            }
        }
        if (use_lds) {
            __syncthreads();
            for (int e = threadIdx.x; e < np * (int)box; e += 256) {
                const unsigned long long qv = win[e];
                if (!qv) continue;
                const int p = e / (int)box, o = e - p * (int)box, r = o / Cc, c = o - r * Cc;
                atomicAdd(accb + (size_t)(c0 + p) * HWt + (size_t)(rmin + r) * Wt + (cmin + c), qv);
            }
            __syncthreads();
        }
    }
}

// pass 3: int64 sums -> fp32; a poisoned element is NaN.  per_item: elements of acc per scale item
__global__ __launch_bounds__(256) void fvb_convert_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ poison,
                                                          const unsigned* __restrict__ maxbits, size_t n, size_t per_item, int L,
                                                          float* __restrict__ grad)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float inv = pow2f(-(62 - L - dibr_exponent(maxbits[i / per_item])));
        const bool bad = poison[i >> 5] >> (i & 31) & 1u;
        grad[i] = bad ? __int_as_float(0x7fc00000) : (float)acc[i] * inv;
    }
}

int ceil_log2(long long n)
{
    int l = 0;
    while ((1ll << l) < n) ++l;
    return l;
}

// the four launches.  (Hs, Ws) / (Ht, Wt): source / target image; items: scale items (B | N | B), each `g_per` contiguous upstream floats and
// `images / items` target images; by: grid.y of the scatter
template <int OP>
int fvb_run(const char* what, const float* g, float* grad, const float* rot, int N, int C, int Hs, int Ws, int Ht, int Wt, int items, long long images,
            int by, long long sources, float h_len, float w_len, int concat, void* ws, hipStream_t s)
{
    if ((uintptr_t)ws & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": the workspace must be 16-byte aligned");
    if (images * C > (1ll << 24) || by > 65535) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": too many image planes");
    const FvbWs l = fvb_layout(images, C, Ht, Wt);
    char* base = (char*)ws;
    FvbArgs a;
    a.g = g; a.rot = rot;
    a.acc = (unsigned long long*)(base + l.acc); a.poison = (unsigned*)(base + l.poison); a.maxbits = (const unsigned*)base;
    a.C = C; a.N = N; a.Hs = Hs; a.Ws = Ws; a.Ht = Ht; a.Wt = Wt;
    a.groups = (Ws + FV_PX - 1) / FV_PX;
    a.tgl = 0;
    while (a.tgl < 4 && (1 << a.tgl) < a.groups) ++a.tgl;
    const int tg = 1 << a.tgl, tr = 256 >> a.tgl;
    a.tiles_x = (a.groups + tg - 1) / tg;
    a.tiles = a.tiles_x * ((Hs + tr - 1) / tr);
    if ((long long)a.tiles * N > (1ll << 31) - 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": too many source pixels for one launch");
    a.L = ceil_log2(sources);
    a.concat = concat; a.use_lds = omni_options().fv_bwd_lds ? 1 : 0;
    a.h_len = h_len; a.w_len = w_len;
    const size_t n = (size_t)images * C * Ht * Wt, g_per = (size_t)(OP == FVB_E2P ? N : 1) * C * Hs * Ws;

    hipLaunchKernelGGL(dibr_zero_kernel, dim3(2048), dim3(256), 0, s, (uint4*)ws, l.total / 16);
    const int mx = (int)std::min<size_t>((g_per + 1023) / 1024, 256);
    hipLaunchKernelGGL(fvb_max_kernel, dim3(mx, items), dim3(256), 0, s, g, g_per, (unsigned*)base);
    hipLaunchKernelGGL(fvb_scatter_kernel<OP>, dim3(a.tiles * N, by), dim3(256), 0, s, a);
    const int cb = (int)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(fvb_convert_kernel, dim3(cb), dim3(256), 0, s, (const long long*)a.acc, (const unsigned*)a.poison, a.maxbits, n,
                       n / (size_t)items, a.L, grad);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

}  // namespace

extern "C" size_t omni_freeview_bwd_workspace_bytes(int op, int items, int C, int Ht, int Wt)
{
    if (op < 0 || op > 2 || items < 1 || C < 1 || Ht < 1 || Wt < 1) return 0;
    return fvb_layout(items, C, Ht, Wt).total;
}

extern "C" int omni_freeview_equi2pers_bwd_f32(const float* grad_pers, float* grad_erp, const float* rot_fwd_dev, int B, int C, int H, int W,
                                               int N, int h, int w, float hfov_deg, float wfov_deg, int layout, void* ws, omni_stream_t stream)
{
    const char* what = "omni_freeview_equi2pers_bwd_f32";
    if (!grad_pers || !grad_erp || !rot_fwd_dev || !ws) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": B must be >= 1");
    if (layout != OMNI_LAYOUT_BNCHW && layout != OMNI_LAYOUT_BCHNW) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": layout must be OMNI_LAYOUT_BNCHW or OMNI_LAYOUT_BCHNW");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, h, w, N, s)) return e;
    return fvb_run<FVB_E2P>(what, grad_pers, grad_erp, rot_fwd_dev, N, C, h, w, H, W, B, B, B, (long long)N * h * w, s.h_len, s.w_len,
                            layout == OMNI_LAYOUT_BCHNW ? 1 : 0, ws, (hipStream_t)stream);
}

extern "C" int omni_freeview_pers2equi_bwd_f32(const float* grad_erp, float* grad_pers, const float* rot_inv_dev, int N, int C, int h, int w,
                                               int H, int W, float hfov_deg, float wfov_deg, void* ws, omni_stream_t stream)
{
    const char* what = "omni_freeview_pers2equi_bwd_f32";
    if (!grad_erp || !grad_pers || !rot_inv_dev || !ws) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, H, W, N, s)) return e;
    return fvb_run<FVB_P2E>(what, grad_erp, grad_pers, rot_inv_dev, N, C, H, W, h, w, N, N, 1, (long long)H * W, s.h_len, s.w_len, 0, ws,
                            (hipStream_t)stream);
}

extern "C" int omni_freeview_merge_bwd_f32(const float* grad_erp, float* grad_pers, const float* rot_inv_dev, int B, int N, int C, int h, int w,
                                           int H, int W, float hfov_deg, float wfov_deg, void* ws, omni_stream_t stream)
{
    const char* what = "omni_freeview_merge_bwd_f32";
    if (!grad_erp || !grad_pers || !rot_inv_dev || !ws) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": null device pointer");
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": B must be >= 1");
    if (N > 255) OMNI_FAIL(OMNI_ERR_INVALID, std::string(what) + ": at most 255 views (count is uint8)");
    FvShape s;
    if (int e = fv_check(what, N, C, h, w, H, W, hfov_deg, wfov_deg, H, W, N, s)) return e;
    return fvb_run<FVB_MERGE>(what, grad_erp, grad_pers, rot_inv_dev, N, C, H, W, h, w, B, (long long)B * N, B, (long long)H * W, s.h_len, s.w_len, 0,
                              ws, (hipStream_t)stream);
}
