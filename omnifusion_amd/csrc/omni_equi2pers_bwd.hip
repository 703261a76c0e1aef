// omni_equi2pers_bwd.hip — backward of equi2pers (omni_equi2pers.hip): the scatter kernel e2p_bwd_kernel, the transposed LDS-box kernel (e2p_lds_kernel<TS, true>,
// omni_e2p_common.h), the backward by gathers, the walk kernel that emits the entries of the sparse-matrix form (applied by omni_spgather.hip), their tables and omni_equi2pers_bwd.
#include "omni_e2p_common.h"
#include "omni_spgather.h"

namespace {

// ------------------------------------------------------------------ backward
// g_erp[b,c,y,x] = sum over patch samples and their four taps of w_tap * g_pers[b,c,h,w,n]: the transpose of the bilinear
// gather (ATen grid_sampler_2d_backward with bilinear / border / align_corners=True; taps outside the image are dropped).
// One thread per patch sample, all B*C planes; fp32 hardware atomics into a zeroed g_erp (the summation order is not
// deterministic, exactly like the reference's CUDA/HIP grid_sample backward).
__global__ __launch_bounds__(256) void e2p_bwd_kernel(E2PArgs a /* erp = g_erp (out), pers = g_pers (in) */, int n_fastest, int total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int n, h, w;
    if (n_fastest) { n = i % a.tab.N; w = (i / a.tab.N) % a.pw; h = i / (a.tab.N * a.pw); }     // [B,C,h,w,N]: coalesced reads
    else           { w = i % a.pw; h = (i / a.pw) % a.ph; n = i / (a.pw * a.ph); }              // [B,N,C,h,w]
    float ix, iy;
    if (a.ixy) { const float2 c = a.ixy[((size_t)n * a.ph + h) * a.pw + w]; ix = c.x; iy = c.y; }
    else e2p_sample_xy(a, n, h, w, ix, iy);
    if (!(ix == ix) || !(iy == iy)) return;                       // (never taken: the clip of e2p_sample_xy has already sent the NaN row coordinate of the q4 centre
                                                                  //  sample to 0, so its gradient goes to row 0, where the forward reads it: the exact transpose)
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy, ex = 1.0f - tx, ey = 1.0f - ty;
    const bool okx = x0 + 1 < a.W, oky = y0 + 1 < a.H;
    const size_t plane = (size_t)a.H * a.W, pp = (size_t)a.ph * a.pw;
    float* gerp = (float*)a.erp;
    const float* gp = (const float*)a.pers;
    const size_t o00 = (size_t)y0 * a.W + x0;
    for (int b = 0; b < a.B; ++b)
        for (int c = 0; c < a.C; ++c) {
            const size_t src = n_fastest ? ((((size_t)b * a.C + c) * a.ph + h) * a.pw + w) * a.tab.N + n
                                         : (((size_t)b * a.tab.N + n) * a.C + c) * pp + (size_t)h * a.pw + w;
            const float g = gp[src];
            float* e = gerp + ((size_t)b * a.C + c) * plane + o00;
            atomicAdd(e, g * (ey * ex));
            if (okx) atomicAdd(e + 1, g * (ey * tx));
            if (oky) atomicAdd(e + a.W, g * (ty * ex));
            if (okx && oky) atomicAdd(e + a.W + 1, g * (ty * tx));
        }
}
}  // namespace

// Vector-Jacobian product of equi2pers w.r.t. the ERP image (the operator is linear in it): grad_pers in the layout of the
// forward's output, grad_erp [B,C,H,W] is overwritten.  fp32 only.  Replaces what autograd derives from F.grid_sample
// (equi2pers_v3.py:111) in the reference's training scripts (train_erp_depth.py:255-300).
// ---- backward by gathers (no global atomics, nothing to zero): the mirror image of p2e_bwd_gather_kernel (omni_pers2equi_bwd.hip).  ERP tiles
// are disjoint: one wave owns a 4 x 32 ERP tile, walks — per patch — the box of the samples whose bilinear taps can touch it (a constant
// of the geometry, from the same coordinate table and tap arithmetic: exact superset), adds the taps that land inside its tile into an
// LDS accumulator and writes the tile once.  Taps as in e2p_bwd_kernel (= what autograd derives from F.grid_sample, border padding).
namespace {
constexpr int E2G_TH = 4, E2G_TW = 32;

__global__ __launch_bounds__(256) void e2p_bwd_box_kernel(E2PArgs a, int* __restrict__ boxes, int gtx, int total)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= total) return;
    const int w = s % a.pw, h = (s / a.pw) % a.ph, n = s / (a.pw * a.ph);
    const float2 c = a.ixy[s];
    if (!(c.x == c.x) || !(c.y == c.y)) return;
    const int x0 = (int)floorf(c.x), y0 = (int)floorf(c.y);
    const int x1 = x0 + 1 < a.W ? x0 + 1 : x0, y1 = y0 + 1 < a.H ? y0 + 1 : y0;
    const int xs[2] = {x0, x1}, ys[2] = {y0, y1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == 1 && x1 == x0) continue;
        if (k == 2 && y1 == y0) continue;
        if (k == 3 && (x1 == x0 || y1 == y0)) continue;
        int* b = boxes + 4 * ((size_t)((ys[k >> 1] / E2G_TH) * gtx + xs[k & 1] / E2G_TW) * a.tab.N + n);
        atomicMin(b + 0, h); atomicMax(b + 1, h); atomicMin(b + 2, w); atomicMax(b + 3, w);
    }
}

// The transpose as a sparse matrix (omni_spgather.h): every tap of every patch sample is one entry (source = the sample, packed
// patch << 24 | h * pw + w; weight = the bilinear weight) of the row of the ERP pixel it reads.  Taps as in e2p_bwd_kernel.
__global__ __launch_bounds__(256) void e2p_sp_walk_kernel(E2PArgs a, int total, SpEmit b)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= total) return;
    const int pp = a.ph * a.pw, n = s / pp;
    const unsigned src = ((unsigned)n << 24) | (unsigned)(s - n * pp);
    const float2 c = a.ixy[s];
    if (!(c.x == c.x) || !(c.y == c.y)) return;                   // (never taken, see e2p_bwd_kernel: the table holds the clipped coordinate, the q4 sample scatters into row 0)
    const float fx = floorf(c.x), fy = floorf(c.y);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = c.x - fx, ty = c.y - fy, ex = 1.0f - tx, ey = 1.0f - ty;
    const bool okx = x0 + 1 < a.W, oky = y0 + 1 < a.H;
    const int row = y0 * a.W + x0;
    sp_emit(b, row, src, ey * ex);
    if (okx) sp_emit(b, row + 1, src, ey * tx);
    if (oky) sp_emit(b, row + a.W, src, ty * ex);
    if (okx && oky) sp_emit(b, row + a.W + 1, src, ty * tx);
}

template <int PL, int NT>
__global__ __launch_bounds__(NT) void e2p_bwd_gather_kernel(E2PArgs a /* erp = g_erp (out), pers = g_pers (in) */, const int4* __restrict__ boxes,
                                                            const int* __restrict__ ids, int gtx, int planes, int n_fastest)
{
    __shared__ float acc[PL][E2G_TH * E2G_TW];
    const int lane = threadIdx.x;
    const int id = ids[blockIdx.x], p0 = blockIdx.y * PL;
    const int ty0 = (id / gtx) * E2G_TH, tx0 = (id % gtx) * E2G_TW;
#pragma unroll
    for (int p = 0; p < PL; ++p)
        for (int e = lane; e < E2G_TH * E2G_TW; e += NT) acc[p][e] = 0.0f;
    if (NT > 64) __syncthreads();
    const float* gp = (const float*)a.pers;
    const size_t pp = (size_t)a.ph * a.pw;
    for (int n = 0; n < a.tab.N; ++n) {
        const int4 box = boxes[(size_t)id * a.tab.N + n];          // sample rows min, max, columns min, max
        if (box.x > box.y) continue;                               // (wave-uniform)
        const int bw = box.w - box.z + 1, npx = bw * (box.y - box.x + 1);
        const float rbw = 1.0f / (float)bw;
        for (int base = 0; base < npx; base += NT) {
            const int idx = base + lane;
            if (idx >= npx) continue;
            int dy = (int)(((float)idx + 0.5f) * rbw);
            int dxi = idx - dy * bw;
            if (dxi < 0) { --dy; dxi += bw; } else if (dxi >= bw) { ++dy; dxi -= bw; }
            const int h = box.x + dy, w = box.z + dxi;
            const float2 c = a.ixy[((size_t)n * a.ph + h) * a.pw + w];
            if (!(c.x == c.x) || !(c.y == c.y)) continue;
            const float fx = floorf(c.x), fy = floorf(c.y);
            const int x0 = (int)fx, y0 = (int)fy;
            const float tx = c.x - fx, ty = c.y - fy, ex = 1.0f - tx, ey = 1.0f - ty;
            const bool okx = x0 + 1 < a.W, oky = y0 + 1 < a.H;
            const int xa = x0 - tx0, xb = xa + 1, ya = y0 - ty0, yb = ya + 1;
            const bool xa_in = (unsigned)xa < (unsigned)E2G_TW, xb_in = okx && (unsigned)xb < (unsigned)E2G_TW;
            const bool ya_in = (unsigned)ya < (unsigned)E2G_TH, yb_in = oky && (unsigned)yb < (unsigned)E2G_TH;
            const float w00 = (ya_in && xa_in) ? ey * ex : 0.0f, w01 = (ya_in && xb_in) ? ey * tx : 0.0f;
            const float w10 = (yb_in && xa_in) ? ty * ex : 0.0f, w11 = (yb_in && xb_in) ? ty * tx : 0.0f;
            if (!((ya_in || yb_in) && (xa_in || xb_in))) continue;
#pragma unroll
            for (int p = 0; p < PL; ++p) {
                if (p0 + p >= planes) break;
                const int b = (p0 + p) / a.C, ch = (p0 + p) % a.C;
                const size_t src = n_fastest ? ((((size_t)b * a.C + ch) * a.ph + h) * a.pw + w) * a.tab.N + n
                                             : (((size_t)b * a.tab.N + n) * a.C + ch) * pp + (size_t)h * a.pw + w;
                const float g = gp[src];
                // (a zero weight of a tap INSIDE the tile must still be added as 0 x g only if g is finite: skip instead, like a tap outside)
                if (ya_in && xa_in) atomicAdd(&acc[p][ya * E2G_TW + xa], g * w00);
                if (ya_in && xb_in) atomicAdd(&acc[p][ya * E2G_TW + xb], g * w01);
                if (yb_in && xa_in) atomicAdd(&acc[p][yb * E2G_TW + xa], g * w10);
                if (yb_in && xb_in) atomicAdd(&acc[p][yb * E2G_TW + xb], g * w11);
            }
        }
    }
    __syncthreads();
    float* gerp = (float*)const_cast<void*>(a.erp);
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int p = 0; p < PL; ++p) {
        if (p0 + p >= planes) break;
        for (int e = lane; e < E2G_TH * E2G_TW; e += NT) {
            const int y = ty0 + e / E2G_TW, x = tx0 + e % E2G_TW;
            if (y < a.H && x < a.W) gerp[(size_t)(p0 + p) * plane + (size_t)y * a.W + x] = acc[p][e];
        }
    }
}
}  // namespace

int omni_e2p_build_bwd(omni_geometry* g, hipStream_t stream)
{
    if (!g->e2p_ixy) return OMNI_OK;                               // no coordinate table: the scatter kernels serve this geometry
    E2PArgs a; fill_args(a, g, nullptr, nullptr, 1, 1);
    g->e2p_gtx = (g->W + E2G_TW - 1) / E2G_TW; g->e2p_gty = (g->H + E2G_TH - 1) / E2G_TH;
    const size_t ntiles = (size_t)g->e2p_gtx * g->e2p_gty, nbox = ntiles * g->N;
    const long long total = (long long)g->N * g->ph * g->pw;
    if (ntiles == 0 || nbox >= (1u << 28) || total >= (1ll << 31)) return OMNI_OK;
    BwdBoxes bx;
    int rc = omni_bwd_boxes(&g->e2p_bwd_box, &g->e2p_bwd_ids, ntiles, g->N, 4096, stream, &bx, [&](int4* boxes) {
        hipLaunchKernelGGL(e2p_bwd_box_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, (int*)boxes, g->e2p_gtx, (int)total);
        return OMNI_OK;
    });
    if (rc != OMNI_OK) return rc;
    if (omni_options().e2p_verbose)
        fprintf(stderr, "[omni] equi2pers backward boxes (%dx%d ERP, %d patches %dx%d): %zu tiles, %zu big; box samples small %lld big %lld, largest %lld\n",
                g->H, g->W, g->N, g->ph, g->pw, ntiles, (size_t)bx.nbig, bx.ps, bx.pb, bx.mx);
    g->e2p_bwd_nsmall = bx.nsmall; g->e2p_bwd_nbig = bx.nbig; g->e2p_bwd_ok = 1;
    // the sparse-matrix form (the default): rows = ERP pixels, sources = patch samples (patch in the high 8 bits, sample in the low 24)
    if ((long long)g->H * g->W < (1ll << 31) && (long long)g->ph * g->pw <= (1ll << 24) && g->N < 256)
        return omni_sp_build(&g->e2p_sp, g->H * g->W, (size_t)omni_options().bwd_table_mb << 20, stream, "equi2pers", [&](SpEmit e) {
            hipLaunchKernelGGL(e2p_sp_walk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, (int)total, e);
        });
    return OMNI_OK;
}

extern "C" int omni_equi2pers_bwd(const void* grad_pers, void* grad_erp, int dtype, int B, int C, int H, int W,
                                  int ph, int pw, int nrows, float fov_h, float fov_w, int layout, omni_stream_t stream)
{
    if (dtype != OMNI_F32) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers_bwd: fp32 only");
    if (layout != OMNI_LAYOUT_BCHWN && layout != OMNI_LAYOUT_BNCHW) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers_bwd: layout must be BCHWN or BNCHW");
    const omni_geometry* g = nullptr;
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, H, W, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    if (B < 0 || C < 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers_bwd: negative batch/channels");
    if (B == 0 || C == 0) return OMNI_OK;
    if (!grad_pers || !grad_erp) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers_bwd: null device pointer");
    E2PArgs a; fill_args(a, g, grad_erp, const_cast<void*>(grad_pers), B, C);
    rc = omni_bwd_build_once(g, &omni_geometry::e2p_bwd_tried, omni_e2p_build_bwd, (hipStream_t)stream);   // first backward of this geometry: its tables
    if (rc != OMNI_OK) return rc;
    const int mode = omni_options().e2p_bwd_simple;
    if (g->e2p_sp.ok && (mode == 0 || mode == 4)) {               // the sparse-matrix gather: no atomics, nothing to zero
        SpApply s;
        const long long pp = (long long)ph * pw;
        s.src = (const float*)grad_pers; s.dst = (float*)grad_erp; s.C = C; s.planes = B * C;
        if (layout == OMNI_LAYOUT_BNCHW) { s.s_sB = (long long)g->N * C * pp; s.s_sC = pp; s.s_hi = (int)(C * pp); s.s_lo = 1; }
        else                             { s.s_sB = (long long)C * pp * g->N; s.s_sC = pp * g->N; s.s_hi = 1; s.s_lo = g->N; }
        s.d_sB = (long long)C * H * W; s.d_sC = (long long)H * W; s.rdiv = 0x7fffffff; s.d_hi = 0; s.d_lo = 1;
        s.PT = (B * C + 3) / 4 * 4; s.nhi = g->N; s.nlo = (int)pp; s.hi_fastest = layout == OMNI_LAYOUT_BCHWN; s.chunk = 16;
        if ((long long)g->N * C * pp < (1ll << 31)) {
            float* ws = nullptr;
            if (omni_options().bwd_wide) {
                rc = omni_bwd_workspace(const_cast<omni_geometry*>(g), (hipStream_t)stream, (size_t)g->N * pp * s.PT * sizeof(float), &ws);
                if (rc != OMNI_OK) return rc;
            }
            return omni_sp_apply(g->e2p_sp, s, (hipStream_t)stream, ws);
        }
    }
    // without the table, mode 0: whichever is faster for the layout — measured at B = 8, cfg 1: planar 0.74 ms (LDS boxes + coalesced global atomics) vs
    // 0.88 ms (gathers); reference layout 0.88 ms (gathers) vs 3.17 ms (plain scatter).  3 forces the gathers, 1 the plain scatter, 2 the LDS boxes.
    const bool planar_boxes = layout == OMNI_LAYOUT_BNCHW && g->W >= 2;
    if (g->e2p_bwd_ok && (mode == 3 || (mode == 0 && !planar_boxes))) {
        constexpr int PL = 4;
        const int groups = (B * C + PL - 1) / PL, nf = layout == OMNI_LAYOUT_BCHWN ? 1 : 0;
        if (g->e2p_bwd_nbig)
            hipLaunchKernelGGL((e2p_bwd_gather_kernel<PL, 1024>), dim3(g->e2p_bwd_nbig, groups), dim3(1024), 0, (hipStream_t)stream, a,
                               (const int4*)g->e2p_bwd_box, (const int*)g->e2p_bwd_ids + g->e2p_bwd_nsmall, g->e2p_gtx, B * C, nf);
        if (g->e2p_bwd_nsmall)
            hipLaunchKernelGGL((e2p_bwd_gather_kernel<PL, 64>), dim3(g->e2p_bwd_nsmall, groups), dim3(64), 0, (hipStream_t)stream, a,
                               (const int4*)g->e2p_bwd_box, (const int*)g->e2p_bwd_ids, g->e2p_gtx, B * C, nf);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    OMNI_HIP(hipMemsetAsync(grad_erp, 0, (size_t)B * C * H * W * sizeof(float), (hipStream_t)stream));
    const long long total = (long long)g->N * ph * pw;
    if (total >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers_bwd: too many patch samples");
    if (planar_boxes && mode != 1) {
        // planar layout: the transposed LDS-box kernel (same tiling and fallback list as the forward)
        const int ts = g->e2p_ts, tx = (g->pw + ts - 1) / ts, ty = (g->ph + ts - 1) / ts, nt = g->N * tx * ty;
        if (ts == 32) hipLaunchKernelGGL((e2p_lds_kernel<32, true>), dim3(nt + g->e2p_nfb * B), dim3(256), 0, (hipStream_t)stream, a, tx, tx * ty, nt,
                                         (const int*)g->e2p_fb_tiles, (unsigned char*)nullptr);
        else          hipLaunchKernelGGL((e2p_lds_kernel<16, true>), dim3(nt + g->e2p_nfb * B), dim3(256), 0, (hipStream_t)stream, a, tx, tx * ty, nt,
                                         (const int*)g->e2p_fb_tiles, (unsigned char*)nullptr);
        OMNI_HIP(hipGetLastError());
        return OMNI_OK;
    }
    hipLaunchKernelGGL(e2p_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                       layout == OMNI_LAYOUT_BCHWN ? 1 : 0, (int)total);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
