// omni_pers2equi_bwd.hip — backward of pers2equi (omni_pers2equi.hip): the scatter kernel p2e_bwd_kernel, the backward by gathers, the walk kernel that
// emits the entries of the sparse-matrix form (applied by omni_spgather.hip), their tables and omni_pers2equi_bwd.
#include "omni_p2e_common.h"
#include "omni_spgather.h"

namespace {

// ------------------------------------------------------------------ backward
// g_pers[b,c,y,x,n] = sum over the ERP pixels (i,j) whose tap of patch n is (y,x) of w~ * g_erp[b,c,i,j], w~ the thresholded,
// L1-normalised weights of the forward (the operator is linear in the patches; the weights do not depend on them).
// One thread per ERP pixel, two passes over the candidate patches (normaliser, then scatter); fp32 hardware atomics into a
// zeroed g_pers.
__global__ __launch_bounds__(256) void p2e_bwd_kernel(P2EArgs a /* erp = g_erp (in), pers = g_pers (out) */, int nblocks)
{
    const unsigned lb = omni_xcd_remap(blockIdx.x, nblocks);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = lb % a.ntx;
    const int i = __builtin_amdgcn_readfirstlane((int)(lb / a.ntx) * 4 + wave);
    const int j = tx * 64 + lane;
    if (i >= a.H) return;
    const bool inside = j < a.W;
    const float2 rt = a.row_trig[i];
    const float2 ct = a.col_trig[inside ? j : a.W - 1];
    const unsigned long long cm_ = a.cand[(size_t)i * a.ntx + tx];
    const unsigned cm_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ >> 32));
    const unsigned cm_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ & 0xffffffffull));
    const unsigned long long cmask = ((unsigned long long)cm_hi << 32) | (unsigned long long)cm_lo;
    float l1 = 0.0f;
    for (unsigned long long m = cmask; m;) {
        const int n = __builtin_ctzll(m); m &= m - 1;
        Taps t; p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
        l1 += (t.wa + t.wb) + (t.wc + t.wd);
    }
    if (!inside) return;
    const float rden = 1.0f / fmaxf(l1, 1e-12f);
    const float* gerp = (const float*)a.erp;
    float* gp = (float*)const_cast<void*>(a.pers);
    const size_t erp_plane = (size_t)a.H * a.W, pix = (size_t)i * a.W + j;
    for (unsigned long long m = cmask; m;) {
        const int n = __builtin_ctzll(m); m &= m - 1;
        Taps t; p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
        if (!((t.wa + t.wb) + (t.wc + t.wd) > 0.0f)) continue;
        const size_t oa = (size_t)n * a.sN + (size_t)t.y0 * a.sY + (size_t)t.x0 * a.sX, ob = (size_t)n * a.sN + (size_t)t.y1 * a.sY + (size_t)t.x0 * a.sX;
        const size_t oc = (size_t)n * a.sN + (size_t)t.y0 * a.sY + (size_t)t.x1 * a.sX, od = (size_t)n * a.sN + (size_t)t.y1 * a.sY + (size_t)t.x1 * a.sX;
        for (int b = 0; b < a.B; ++b)
            for (int c = 0; c < a.C; ++c) {
                const float g = gerp[((size_t)b * a.C + c) * erp_plane + pix] * rden;
                float* q = gp + (size_t)b * a.sB + (size_t)c * a.sC;
                if (t.wa != 0.0f) atomicAdd(q + oa, g * t.wa);
                if (t.wb != 0.0f) atomicAdd(q + ob, g * t.wb);
                if (t.wc != 0.0f) atomicAdd(q + oc, g * t.wc);
                if (t.wd != 0.0f) atomicAdd(q + od, g * t.wd);
            }
    }
}
}  // namespace

// Vector-Jacobian product of pers2equi w.r.t. the patches: grad_erp [B,C,H,W] -> grad_pers in the layout of the forward's
// input (overwritten).  fp32 only.  Replaces what autograd derives from the advanced-indexing gathers of
// pers2equi_v3.py:174-196 in the reference's training scripts.
namespace {
// ---- backward by gathers (no global atomics, nothing to zero).  The scatter kernel above issues 4 global atomics per (ERP pixel, covering
// patch, plane): 35 M of them at B = 8, 18 x 256^2 — 1.28 ms, bound by the L2 atomic rate.  Transposed, every PATCH pixel is the sum over the ERP
// pixels whose bilinear taps touch it, and patch tiles are disjoint: one wave owns a 4 x 32 tile of one patch, walks the ERP box of the
// pixels that can touch it (a constant of the geometry, built once with the SAME tap function — exact superset), evaluates their taps
// for this patch, and accumulates the ones that fall into its tile in LDS (ds_add_f32: order within the wave's own instruction stream);
// then it writes the tile once, coalesced.  An ERP pixel is visited by every tile its taps touch (1-4 per covering patch), so the tap
// geometry is evaluated ~2.5x as often as in the forward; the L1 normaliser of a pixel (all covering patches) is a table.
constexpr int P2B_TH = 4, P2B_TW = 32;

__device__ __forceinline__ int p2b_centre_col(const P2EArgs& a, int n)
{
    return (int)((a.tab.lam0[n] + 3.14159265358979f) * (0.5f / 3.14159265358979f) * (float)(a.W - 1) + 0.5f);
}
__device__ __forceinline__ int p2b_wrap(int dx, int W)              // column difference into [-W/2, W - W/2)
{
    const int h = W >> 1;
    dx = dx >= W - h ? dx - W : dx;
    return dx < -h ? dx + W : dx;
}

// one wave per 64 ERP pixels of one row: the L1 normaliser of every pixel and, per (patch, tile), the box of the pixels touching it
__global__ __launch_bounds__(256) void p2e_bwd_box_kernel(P2EArgs a, int* __restrict__ boxes, float* __restrict__ rden, int btx, int bty)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x % a.ntx;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / a.ntx) * 4 + wave);
    const int j = tx * 64 + lane;
    if (i >= a.H) return;
    const bool inside = j < a.W;
    const float2 rt = a.row_trig[i];
    const float2 ct = a.col_trig[inside ? j : a.W - 1];
    const unsigned long long cm_ = a.cand[(size_t)i * a.ntx + tx];
    const unsigned cm_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ >> 32));
    const unsigned cm_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ & 0xffffffffull));
    const unsigned long long cmask = ((unsigned long long)cm_hi << 32) | (unsigned long long)cm_lo;
    float l1 = 0.0f;
    for (unsigned long long m = cmask; m;) {
        const int n = __builtin_ctzll(m); m &= m - 1;
        Taps t; p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
        const float wsum = (t.wa + t.wb) + (t.wc + t.wd);
        l1 += wsum;
        if (!(inside && wsum > 0.0f)) continue;
        const int dx = p2b_wrap(j - p2b_centre_col(a, n), a.W);
        const int xs[2] = {t.x0, t.x1}, ys[2] = {t.y0, t.y1};
        const float w[4] = {t.wa, t.wb, t.wc, t.wd};               // (y0,x0) (y1,x0) (y0,x1) (y1,x1)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (w[k] == 0.0f) continue;
            const int id = (n * bty + ys[k & 1] / P2B_TH) * btx + xs[k >> 1] / P2B_TW;
            atomicMin(boxes + 4 * id + 0, dx); atomicMax(boxes + 4 * id + 1, dx);
            atomicMin(boxes + 4 * id + 2, i);  atomicMax(boxes + 4 * id + 3, i);
        }
    }
    if (inside) rden[(size_t)i * a.W + j] = 1.0f / fmaxf(l1, 1e-12f);
}

// planar [planes][N][pp] -> the reference's [planes][pp][N] (N innermost), 64 samples of all N patches per block through LDS: coalesced
// reads (N runs of 256 bytes) and one contiguous run of 64 N floats out.  (Writing N-innermost straight from the gather kernel puts 4 bytes
// into every 4 N: 260 MB of write traffic for 38 MB at 18 x 256^2.)
__global__ __launch_bounds__(256) void p2e_nlast_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int pp, int C)
{
    extern __shared__ float nl_tile[];                            // [64][N | 1]
    const int NP = N | 1, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int p = blockIdx.y, b = p / C, c = p - b * C, s0 = blockIdx.x * 64, ns = min(64, pp - s0);
    const float* sp = src + ((size_t)b * N * C + c) * pp + s0;    // + n * C * pp
    for (int n = wave; n < N; n += 4)
        if (lane < ns) nl_tile[lane * NP + n] = sp[(size_t)n * C * pp + lane];
    __syncthreads();
    float* dp = dst + ((size_t)p * pp + s0) * N;
    for (int i = t; i < ns * N; i += 256) { const int px = i / N, n = i - px * N; dp[i] = nl_tile[px * NP + n]; }
}

// The transpose as a sparse matrix (omni_spgather.h): every (ERP pixel, covering patch, tap with a non-zero weight) is one entry
// (source = the pixel, weight = w_tap / l1) of the row of the patch pixel the tap reads.  Same traversal and tap function as above.
__global__ __launch_bounds__(256) void p2e_sp_walk_kernel(P2EArgs a, const float* __restrict__ rden, SpEmit b)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x % a.ntx;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / a.ntx) * 4 + wave);
    const int j = tx * 64 + lane;
    if (i >= a.H || j >= a.W) return;
    const float2 rt = a.row_trig[i], ct = a.col_trig[j];
    const size_t pix = (size_t)i * a.W + j;
    const float r = rden[pix];
    const unsigned long long cm_ = a.cand[(size_t)i * a.ntx + tx];
    const unsigned cm_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ >> 32));
    const unsigned cm_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ & 0xffffffffull));
    for (unsigned long long m = ((unsigned long long)cm_hi << 32) | (unsigned long long)cm_lo; m;) {
        const int n = __builtin_ctzll(m); m &= m - 1;
        Taps t; p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
        const int xs[2] = {t.x0, t.x1}, ys[2] = {t.y0, t.y1};
        const float w[4] = {t.wa, t.wb, t.wc, t.wd};               // (y0,x0) (y1,x0) (y0,x1) (y1,x1)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w[k] != 0.0f) sp_emit(b, (n * a.ph + ys[k & 1]) * a.pw + xs[k >> 1], (unsigned)pix, w[k] * r);
    }
}

// NT threads per tile: 64 for the ordinary tiles, 1024 for the few polar ones whose box is whole ERP rows (tens of thousands of pixels)
template <int PL, int NT>
__global__ __launch_bounds__(NT) void p2e_bwd_gather_kernel(P2EArgs a /* erp = g_erp (in), pers = g_pers (out) */, const int4* __restrict__ boxes,
                                                            const float* __restrict__ rden, const int* __restrict__ ids, int btx, int bty, int planes)
{
    __shared__ float acc[PL][P2B_TH * P2B_TW];
    const int lane = threadIdx.x;
    const int id = ids[blockIdx.x], p0 = blockIdx.y * PL;
    const int n = id / (btx * bty), tt = id - n * (btx * bty);
    const int ty0 = (tt / btx) * P2B_TH, tx0 = (tt % btx) * P2B_TW;
#pragma unroll
    for (int p = 0; p < PL; ++p)
        for (int e = lane; e < P2B_TH * P2B_TW; e += NT) acc[p][e] = 0.0f;
    if (NT > 64) __syncthreads();
    const int4 box = boxes[id];                                    // dx min, dx max, row min, row max
    const float* gerp = (const float*)a.erp;
    const size_t erp_plane = (size_t)a.H * a.W;
    if (box.x <= box.y) {
        const int bw = box.y - box.x + 1, npx = bw * (box.w - box.z + 1);
        const int xc = p2b_centre_col(a, n);
        const float rbw = 1.0f / (float)bw;
        for (int base = 0; base < npx; base += NT) {
            const int idx = base + lane;
            const bool in = idx < npx;
            int dy = (int)(((float)idx + 0.5f) * rbw);               // idx / bw (exact for the sizes here, fixed up below)
            int dxi = idx - dy * bw;
            if (dxi < 0) { --dy; dxi += bw; } else if (dxi >= bw) { ++dy; dxi -= bw; }
            const int i = in ? box.z + dy : box.z;
            int j = xc + box.x + (in ? dxi : 0);
            j = j < 0 ? j + a.W : (j >= a.W ? j - a.W : j);
            const float2 rt = a.row_trig[i], ct = a.col_trig[j];
            Taps t; p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
            const size_t pix = (size_t)i * a.W + j;
            const float r = in ? rden[pix] : 0.0f;
            // tile-relative tap positions; a tap outside my tile belongs to a neighbouring wave
            const int ya = t.y0 - ty0, yb = t.y1 - ty0, xa = t.x0 - tx0, xb = t.x1 - tx0;
            const bool ya_in = (unsigned)ya < (unsigned)P2B_TH, yb_in = (unsigned)yb < (unsigned)P2B_TH;
            const bool xa_in = (unsigned)xa < (unsigned)P2B_TW, xb_in = (unsigned)xb < (unsigned)P2B_TW;
            const float wa = (ya_in && xa_in) ? t.wa * r : 0.0f, wb = (yb_in && xa_in) ? t.wb * r : 0.0f;
            const float wc = (ya_in && xb_in) ? t.wc * r : 0.0f, wd = (yb_in && xb_in) ? t.wd * r : 0.0f;
            if (wa == 0.0f && wb == 0.0f && wc == 0.0f && wd == 0.0f) continue;
#pragma unroll
            for (int p = 0; p < PL; ++p) {
                if (p0 + p >= planes) break;
                const float g = gerp[(size_t)(p0 + p) * erp_plane + pix];
                if (wa != 0.0f) atomicAdd(&acc[p][ya * P2B_TW + xa], g * wa);
                if (wb != 0.0f) atomicAdd(&acc[p][yb * P2B_TW + xa], g * wb);
                if (wc != 0.0f) atomicAdd(&acc[p][ya * P2B_TW + xb], g * wc);
                if (wd != 0.0f) atomicAdd(&acc[p][yb * P2B_TW + xb], g * wd);
            }
        }
    }
    __syncthreads();                                               // the LDS adds of every wave are done
    float* gp = (float*)const_cast<void*>(a.pers);
#pragma unroll
    for (int p = 0; p < PL; ++p) {
        if (p0 + p >= planes) break;
        const size_t pb = (size_t)((p0 + p) / a.C) * a.sB + (size_t)((p0 + p) % a.C) * a.sC + (size_t)n * a.sN;
        for (int e = lane; e < P2B_TH * P2B_TW; e += NT) {
            const int y = ty0 + e / P2B_TW, x = tx0 + e % P2B_TW;
            if (y < a.ph && x < a.pw) gp[pb + (size_t)y * a.sY + (size_t)x * a.sX] = acc[p][e];
        }
    }
}
}  // namespace

int omni_p2e_build_bwd(omni_geometry* g, hipStream_t stream)
{
    P2EArgs a;
    int rc = fill_args(a, g, nullptr, nullptr, nullptr, 1, 1, OMNI_LAYOUT_BNCHW);
    if (rc != OMNI_OK) return rc;
    g->p2e_btx = (g->pw + P2B_TW - 1) / P2B_TW; g->p2e_bty = (g->ph + P2B_TH - 1) / P2B_TH;
    const size_t ntiles = (size_t)g->N * g->p2e_btx * g->p2e_bty;
    if (ntiles == 0 || ntiles >= (1u << 30)) return OMNI_OK;       // no table: the scatter kernel serves this geometry
    const int rows4 = (g->H + 3) / 4;
    BwdBoxes bx;
    rc = omni_bwd_boxes(&g->p2e_bwd_box, &g->p2e_bwd_ids, ntiles, 1, 2048, stream, &bx, [&](int4* boxes) {
        OMNI_HIP(hipMalloc((void**)&g->p2e_rden, sizeof(float) * (size_t)g->H * g->W));     // (the kernel's other output: 1 / L1 norm per ERP pixel)
        hipLaunchKernelGGL(p2e_bwd_box_kernel, dim3(rows4 * g->ntx), dim3(256), 0, stream, a, (int*)boxes, g->p2e_rden, g->p2e_btx, g->p2e_bty);
        return OMNI_OK;
    });
    if (rc != OMNI_OK) return rc;
    g->p2e_bwd_nsmall = bx.nsmall; g->p2e_bwd_nbig = bx.nbig; g->p2e_bwd_ok = 1;
    if (omni_options().e2p_verbose)
        fprintf(stderr, "[omni] pers2equi backward boxes (%dx%d ERP, %dx%d patches): %zu tiles, %d big; box pixels small %lld big %lld, largest %lld\n",
                g->H, g->W, g->ph, g->pw, ntiles, g->p2e_bwd_nbig, bx.ps, bx.pb, bx.mx);
    // the sparse-matrix form (the default): rows = patch pixels.  (ERP pixel indices must fit the 24-bit source field.)
    const long long nrows = (long long)g->N * g->ph * g->pw;
    if (nrows < (1ll << 31) && (long long)g->H * g->W <= (1ll << 24))
        return omni_sp_build(&g->p2e_sp, (int)nrows, (size_t)omni_options().bwd_table_mb << 20, stream, "pers2equi", [&](SpEmit e) {
            hipLaunchKernelGGL(p2e_sp_walk_kernel, dim3(rows4 * g->ntx), dim3(256), 0, stream, a, (const float*)g->p2e_rden, e);
        });
    return OMNI_OK;
}

extern "C" int omni_pers2equi_bwd(const void* grad_erp, void* grad_pers, int dtype, int B, int C, int ph, int pw,
                                  int H, int W, int nrows, float fov_h, float fov_w, int layout, omni_stream_t stream)
{
    if (dtype != OMNI_F32) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_pers2equi_bwd: fp32 only");
    const omni_geometry* g = nullptr;
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, H, W, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    rc = check_common(g, B, C, "omni_pers2equi_bwd");
    if (rc != OMNI_OK) return rc;
    if (B == 0 || C == 0) return OMNI_OK;
    if (!grad_erp || !grad_pers) OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi_bwd: null device pointer");
    P2EArgs a;
    rc = fill_args(a, g, grad_pers, nullptr, const_cast<void*>(grad_erp), B, C, layout);
    if (rc != OMNI_OK) return rc;
    rc = omni_bwd_build_once(g, &omni_geometry::p2e_bwd_tried, omni_p2e_build_bwd, (hipStream_t)stream);   // first backward of this geometry: its tables
    if (rc != OMNI_OK) return rc;
    if (g->p2e_sp.ok && omni_options().p2e_bwd_simple == 0 && a.sY == (long long)pw * a.sX) {
        SpApply s;
        s.src = (const float*)grad_erp; s.dst = (float*)grad_pers; s.C = C; s.planes = B * C;
        s.s_sB = (long long)C * H * W; s.s_sC = (long long)H * W; s.s_hi = 0; s.s_lo = 1;
        s.d_sB = a.sB; s.d_sC = a.sC; s.rdiv = ph * pw; s.d_hi = a.sN; s.d_lo = (int)a.sX;
        s.PT = (B * C + 3) / 4 * 4; s.nhi = 1; s.nlo = H * W; s.hi_fastest = 0; s.chunk = 16;
        float* ws = nullptr;
        if (omni_options().bwd_wide) {
            // reference layout: the gathers write the planar form into the scratch, p2e_nlast_kernel turns it N-innermost
            const size_t n1 = (size_t)H * W * s.PT, n2 = layout == OMNI_LAYOUT_BCHWN ? (size_t)B * C * g->N * ph * pw : 0;
            rc = omni_bwd_workspace(const_cast<omni_geometry*>(g), (hipStream_t)stream, (n1 + n2) * sizeof(float), &ws);
            if (rc != OMNI_OK) return rc;
            if (n2) {
                const long long pp = (long long)ph * pw;
                s.dst = ws + n1; s.d_sB = (long long)g->N * C * pp; s.d_sC = pp; s.d_hi = C * pp; s.d_lo = 1;
                rc = omni_sp_apply(g->p2e_sp, s, (hipStream_t)stream, ws);
                if (rc != OMNI_OK) return rc;
                hipLaunchKernelGGL(p2e_nlast_kernel, dim3((unsigned)((pp + 63) / 64), (unsigned)(B * C)), dim3(256), sizeof(float) * 64 * (g->N | 1), (hipStream_t)stream,
                                   (const float*)(ws + n1), (float*)grad_pers, g->N, (int)pp, C);
                OMNI_HIP(hipGetLastError());
                return OMNI_OK;
            }
        }
        return omni_sp_apply(g->p2e_sp, s, (hipStream_t)stream, ws);
    }
    if (g->p2e_bwd_ok && omni_options().p2e_bwd_simple != 1) {
        constexpr int PL = 4;
        const int groups = (B * C + PL - 1) / PL;
        if (g->p2e_bwd_nbig)                                      // first: they are the long ones
            hipLaunchKernelGGL((p2e_bwd_gather_kernel<PL, 1024>), dim3(g->p2e_bwd_nbig, groups), dim3(1024), 0, (hipStream_t)stream, a,
                               (const int4*)g->p2e_bwd_box, (const float*)g->p2e_rden, (const int*)g->p2e_bwd_ids + g->p2e_bwd_nsmall,
                               g->p2e_btx, g->p2e_bty, B * C);
        if (g->p2e_bwd_nsmall)
            hipLaunchKernelGGL((p2e_bwd_gather_kernel<PL, 64>), dim3(g->p2e_bwd_nsmall, groups), dim3(64), 0, (hipStream_t)stream, a,
                               (const int4*)g->p2e_bwd_box, (const float*)g->p2e_rden, (const int*)g->p2e_bwd_ids, g->p2e_btx, g->p2e_bty, B * C);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    OMNI_HIP(hipMemsetAsync(grad_pers, 0, (size_t)B * C * g->N * ph * pw * sizeof(float), (hipStream_t)stream));
    const int rows4 = (g->H + 3) / 4, nblocks = rows4 * g->ntx;
    hipLaunchKernelGGL(p2e_bwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a, nblocks);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
