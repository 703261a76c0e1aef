// omni_e2p_tables.hip — the one-time geometry tables of equi2pers, built once per handle (omni_geometry.hip calls the builders): the sampling-coordinate
// table (e2p_ixy_kernel), the tile flags of e2p_lds_kernel (omni_e2p_build_tileflags) and the per-tile tap boxes of e2p_box_kernel / e2p_ref_kernel
// (e2b_tiles_kernel, omni_e2p_build_boxes).  The fp32 forward by e2p_lds_kernel is launched from here too: the tile-flag builder runs the same
// instantiations, and a kernel lives in one unit.
#include "omni_e2p_common.h"

namespace {

__global__ __launch_bounds__(256) void e2p_ixy_kernel(E2PArgs a, float2* __restrict__ tab, int total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int w = i % a.pw, h = (i / a.pw) % a.ph, n = i / (a.pw * a.ph);
    float ix, iy;
    e2p_sample_xy(a, n, h, w, ix, iy);
    tab[i] = make_float2(ix, iy);
}

template <int NPX>
__global__ __launch_bounds__(256) void e2b_tiles_kernel(E2PArgs a, uint2* __restrict__ ent, int tiles_x, int tiles_pp, int ntiles, int epc,
                                                        int cap_chunks, int odd_pitch, int* __restrict__ stats)
{
    const int wid = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (wid >= ntiles) return;
    const int n = wid / tiles_pp, t = wid - n * tiles_pp;
    const int th0 = (t / tiles_x) * (2 * NPX), tw0 = (t % tiles_x) * E2B_TW;
    const int w = min(tw0 + (lane & 31), a.pw - 1);
    const int W = a.W, H = a.H, half = W >> 1;
    int x0[NPX], ymin = 0x7fffffff, ymax = -1;
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        const int h = min(th0 + (lane >> 5) + 2 * k, a.ph - 1);
        float ix, iy;
        e2b_xy(a, n, h, w, ix, iy);
        const int y0 = (int)floorf(iy);                            // (NaN -> 0: ATen clips the NaN row coordinate of quirk q4 to 0)
        x0[k] = (int)floorf(ix);
        ymin = min(ymin, y0); ymax = max(ymax, min(y0 + 1, H - 1));
    }
    const int xc = __shfl(x0[0], 0);
    int dmin = 0x7fffffff, dmax = -0x7fffffff;
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        int d = x0[k] - xc;
        if (d >= half) d -= W;
        if (d < -half) d += W;
        dmin = min(dmin, d); dmax = max(dmax, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ymin = min(ymin, __shfl_xor(ymin, o)); ymax = max(ymax, __shfl_xor(ymax, o));
        dmin = min(dmin, __shfl_xor(dmin, o)); dmax = max(dmax, __shfl_xor(dmax, o));
    }
    int xs = xc + dmin;
    if (xs < 0) xs += W;
    if (xs >= W) xs -= W;
    const int xs4 = xs / epc * epc, shift = xs - xs4;
    int bw4 = (dmax - dmin + 2 + shift + epc - 1) / epc;           // columns x0 .. x0+1 of every sample, whole 16-byte chunks
    if (odd_pitch && (bw4 & 1) == 0 && (bw4 + 1) * epc <= W) ++bw4;   // odd number of chunks per box row: consecutive rows start 4, 12, 20, 28 banks apart
    const int bh = ymax - ymin + 1;
    const bool fits = (W % epc == 0) && bw4 * epc <= W && bw4 < 4096 && bh < 4096 && bw4 * bh <= cap_chunks;
    if (lane == 0) {
        ent[wid] = make_uint2((unsigned)(bw4 & 4095) | ((unsigned)(bh & 4095) << 12) | (fits ? 0x80000000u : 0u), (unsigned)xs4 | ((unsigned)ymin << 16));
        if (fits) atomicMax(&stats[0], bw4 * bh);
        else stats[2 + atomicAdd(&stats[1], 1)] = wid;             // fallback list (order irrelevant)
    }
}
}  // namespace

int omni_e2p_build_tileflags(omni_geometry* g, hipStream_t stream)
{
    E2PArgs a; fill_args(a, g, nullptr, nullptr, 1, 1);
    // sampling-coordinate table (8 bytes per patch sample: 9.4 MB at 18 x 256^2), read once per launch instead of two
    // transcendentals per sample and tile
    const long long total = (long long)g->N * g->ph * g->pw;
    if (!g->e2p_ixy && total < (1ll << 28) && !omni_options().e2p_notab) {
        OMNI_HIP(hipMalloc((void**)&g->e2p_ixy, sizeof(float2) * (size_t)total));
        hipLaunchKernelGGL(e2p_ixy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, g->e2p_ixy, (int)total);
        OMNI_HIP(hipGetLastError());
        a.ixy = g->e2p_ixy;
    }
    // tiles whose ERP footprint does not fit the LDS box are listed once per geometry and take the gather fallback
    std::vector<int> list;
    int ts = 32;
    for (;;) {
        const int tx = (g->pw + ts - 1) / ts, ty = (g->ph + ts - 1) / ts;
        const int nt = g->N * tx * ty;
        unsigned char* dflags = nullptr;
        OMNI_HIP(hipMalloc((void**)&dflags, nt));
        if (ts == 32) hipLaunchKernelGGL(e2p_lds_kernel<32>, dim3(nt), dim3(256), 0, stream, a, tx, tx * ty, nt, (const int*)nullptr, dflags);
        else          hipLaunchKernelGGL(e2p_lds_kernel<16>, dim3(nt), dim3(256), 0, stream, a, tx, tx * ty, nt, (const int*)nullptr, dflags);
        OMNI_HIP(hipGetLastError());
        std::vector<unsigned char> hf(nt);
        OMNI_HIP(hipMemcpyAsync(hf.data(), dflags, nt, hipMemcpyDeviceToHost, stream));
        OMNI_HIP(hipStreamSynchronize(stream));
        (void)hipFree(dflags);
        list.clear();
        for (int i = 0; i < nt; ++i) if (hf[i]) list.push_back(i);
        if (omni_options().e2p_verbose) fprintf(stderr, "[omni] equi2pers %dx%d patches on %dx%d, %dx%d tiles: %d of %d take the gather fallback\n",
                                                g->ph, g->pw, g->H, g->W, ts, ts, (int)list.size(), nt);
        // (16x16 tiles — OMNI_E2P_TS=16 — cut the fallback count 3-5x where footprints are large (P = 128 at 512x1024, nrows = 6)
        //  but amortise the per-tile prologue over a quarter of the samples: measured equal or slower, so not selected automatically)
        break;
    }
    g->e2p_ts = ts;
    g->e2p_nfb = (int)list.size();
    if (!list.empty()) {
        OMNI_HIP(hipMalloc((void**)&g->e2p_fb_tiles, sizeof(int) * list.size()));
        OMNI_HIP(hipMemcpy(g->e2p_fb_tiles, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    }
    return OMNI_OK;
}

// fp32, layout BNCHW, where the box tables do not serve the shape: e2p_lds_kernel with the tile flags built above
int omni_e2p_launch_lds(const omni_geometry* g, const void* erp, void* pers, int B, int C, hipStream_t stream)
{
    E2PArgs a; fill_args(a, g, erp, pers, B, C);
    const int N = g->N;
    const int ts = g->e2p_ts;
    const int tx = (g->pw + ts - 1) / ts, ty = (g->ph + ts - 1) / ts;
    const int nt = N * tx * ty;
    int psplit = 1;                                      // plane ranges (tuning hook; splitting repeats the per-tile prologue)
    if (ts == 32) hipLaunchKernelGGL(e2p_lds_kernel<32>, dim3(nt + g->e2p_nfb * B, psplit), dim3(256), 0, stream, a, tx, tx * ty, nt,
                                     (const int*)g->e2p_fb_tiles, (unsigned char*)nullptr);
    else          hipLaunchKernelGGL(e2p_lds_kernel<16>, dim3(nt + g->e2p_nfb * B, psplit), dim3(256), 0, stream, a, tx, tx * ty, nt,
                                     (const int*)g->e2p_fb_tiles, (unsigned char*)nullptr);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// Per-tile tap boxes of e2p_box_kernel, one table per element size (tile shape and 16-byte chunk alignment differ).  One-time setup.
int omni_e2p_build_boxes(omni_geometry* g, hipStream_t stream)
{
    E2PArgs a; fill_args(a, g, nullptr, nullptr, 1, 1);
    int cap_kb = omni_options().e2p_slot_kb;
    if (cap_kb < 1) cap_kb = 1;
    if (cap_kb > E2B_NJMAX) cap_kb = E2B_NJMAX;
    // tile height: 8 x 32 samples (option e2p_tile_h: 4 = 4 x 32 tiles, 2 = 4 x 32 where more than 1 tile in 8 of the 8-row tiling would take the gather
    // path — a sample spans several ERP pixels: 128^2 patches on 512 x 1024, 256^2 on 1024 x 2048, 512^2 on 2048 x 4096)
    auto build_one = [&](int e, int th) -> int {
        auto& tt = g->e2p_boxes[e];
        if (tt.ent) (void)hipFree(tt.ent);
        if (tt.fb) (void)hipFree(tt.fb);
        if (tt.order) (void)hipFree(tt.order);
        tt.ent = nullptr; tt.fb = nullptr; tt.order = nullptr; tt.norder = 0; tt.nfb = 0; tt.h_fb.clear();
        tt.tw = E2B_TW; tt.th = th;
        tt.ok = 0;
        if (g->pw % tt.tw != 0 || g->ph % tt.th != 0 || g->W < 2) return OMNI_OK;      // whole tiles only (16-byte stores, static store count per stage)
        tt.tx = g->pw / tt.tw; tt.ty = g->ph / tt.th;
        const long long ntiles = (long long)g->N * tt.tx * tt.ty;
        if (ntiles >= (1ll << 24)) return OMNI_OK;
        const int epc = e ? 8 : 4;
        int* dstats = nullptr;
        OMNI_HIP(hipMalloc((void**)&dstats, sizeof(int) * (size_t)(2 + ntiles)));
        if (hipMalloc((void**)&tt.ent, sizeof(uint2) * (size_t)ntiles) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_e2p_build_boxes: out of memory"); }
        (void)hipMemsetAsync(dstats, 0, 2 * sizeof(int), stream);
        const unsigned nb = (unsigned)((ntiles + 3) / 4);
        if (tt.th == 8) hipLaunchKernelGGL(e2b_tiles_kernel<4>, dim3(nb), dim3(256), 0, stream, a, tt.ent, tt.tx, tt.tx * tt.ty, (int)ntiles, epc, cap_kb * 64, e /* odd pitch: fp16 */, dstats);
        else            hipLaunchKernelGGL(e2b_tiles_kernel<2>, dim3(nb), dim3(256), 0, stream, a, tt.ent, tt.tx, tt.tx * tt.ty, (int)ntiles, epc, cap_kb * 64, e, dstats);
        std::vector<int> hs((size_t)(2 + ntiles));
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hs.data(), dstats, sizeof(int) * hs.size(), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_e2p_build_boxes: kernel failed"); }
        (void)hipFree(dstats);
        tt.max_chunks = hs[0]; tt.nfb = hs[1];
        {
            // LDS-path tiles grouped by the ERP REGION of their box centre, one region per XCD: 4 longitude sectors x 2 hemispheres
            // (a box is ~40-100 x 10 pixels: few boxes straddle the borders of a 256 x H/2 region, whereas with 8 longitude strips
            // of W/8 columns every second box did and was fetched by two XCDs).  Inside a region by latitude band, then longitude:
            // tiles that run at the same time read neighbouring boxes.
            std::vector<uint2> he((size_t)ntiles);
            OMNI_HIP(hipMemcpy(he.data(), tt.ent, sizeof(uint2) * (size_t)ntiles, hipMemcpyDeviceToHost));
            // (round 3, option e2p_region = 1: 8 LATITUDE BANDS of equal estimated cost instead.  A pole tile reads a few ERP rows over hundreds
            //  of columns; with the tiles of a cap spread over four sector XCDs — and the gather tiles over all eight — every XCD fetched the
            //  polar rows of every plane: FETCH_SIZE 100 MB for the 50-MB input, 91 MB with half as many gather tiles.  A band keeps a cap on one XCD.)
            std::vector<std::vector<std::pair<unsigned, int>>> sec(8);
            std::vector<int> region((size_t)ntiles, 0);
            struct TI { int wid, xc, yc, ymin; bool fit; };
            std::vector<TI> all((size_t)ntiles);
            for (int i = 0; i < (int)ntiles; ++i) {
                const int xs4 = (int)(he[i].y & 0xffff), ymin = (int)(he[i].y >> 16), bw = (int)(he[i].x & 4095) * epc, bh = (int)((he[i].x >> 12) & 4095);
                int xc = xs4 + bw / 2; if (xc >= g->W) xc -= g->W;
                all[i] = {i, xc, ymin + bh / 2, ymin, (he[i].x >> 31) != 0};
                region[i] = ((int)((long long)xc * 4 / g->W) & 3) + 4 * (all[i].yc * 2 >= g->H ? 1 : 0);
            }
            if (omni_options().e2p_region == 1) {
                std::vector<TI> srt = all;
                std::sort(srt.begin(), srt.end(), [](const TI& p, const TI& q) { return p.yc != q.yc ? p.yc < q.yc : p.xc < q.xc; });
                auto cost = [](const TI& t) { return t.fit ? 166ll : 430ll; };       // a streaming tile vs a gather tile (8 blocks of 3 planes), 0.1 us
                long long total = 0, run = 0;
                for (auto& t : srt) total += cost(t);
                for (auto& t : srt) { region[t.wid] = (int)std::min<long long>(7, run * 8 / std::max<long long>(1, total)); run += cost(t); }
            }
            for (int i = 0; i < (int)ntiles; ++i)
                if (all[i].fit) sec[region[i]].push_back({((unsigned)(all[i].ymin / 8) << 16) | (unsigned)all[i].xc, i});
            tt.h_region = region;
            size_t mx = 0;
            for (auto& v : sec) { std::sort(v.begin(), v.end()); mx = v.size() > mx ? v.size() : mx; }
            std::vector<int> ord(mx * 8, -1);
            for (int x = 0; x < 8; ++x) for (size_t i = 0; i < sec[x].size(); ++i) ord[i * 8 + x] = sec[x][i].second;
            tt.norder = (int)ord.size();
            tt.h_ent = he; tt.h_order = ord;
            if (tt.norder > 0) {
                OMNI_HIP(hipMalloc((void**)&tt.order, sizeof(int) * ord.size()));
                OMNI_HIP(hipMemcpy(tt.order, ord.data(), sizeof(int) * ord.size(), hipMemcpyHostToDevice));
            }
        }
        tt.h_fb.assign(hs.begin() + 2, hs.begin() + 2 + tt.nfb);
        if (tt.nfb > 0) {
            OMNI_HIP(hipMalloc((void**)&tt.fb, sizeof(int) * (size_t)tt.nfb));
            OMNI_HIP(hipMemcpy(tt.fb, hs.data() + 2, sizeof(int) * (size_t)tt.nfb, hipMemcpyHostToDevice));
        }
        tt.ok = (tt.max_chunks > 0 || tt.nfb > 0) ? 1 : 0;
        if (omni_options().e2p_verbose)
            fprintf(stderr, "[omni] equi2pers %dx%d patches on %dx%d, %d-byte elements, %dx%d sample tiles: largest staged tap box %d chunks, "
                            "%d of %lld tiles take the gather path (box > %d KiB)\n", g->ph, g->pw, g->H, g->W, 16 / epc, tt.th, tt.tw, tt.max_chunks,
                    tt.nfb, ntiles, cap_kb);
        return OMNI_OK;
    };
    for (int e = 0; e < 2; ++e) {
        const int opt = omni_options().e2p_tile_h;
        int rc = build_one(e, opt == 4 ? 4 : 8);
        if (rc != OMNI_OK) return rc;
        auto& tt = g->e2p_boxes[e];
        // (round 4: 4 x 32 tiles where more than 1 tile in 8 would gather — option e2p_tile_h = 2 — measured: 18 x 128^2 patches at 8 panoramas
        //  24.4 -> 20.9 us, but every single-panorama shape LOSES (cfg 3 26.5 -> 28.8 us, cfg 5 fp16 72.9 -> 95.9: twice the blocks, each with its
        //  set-up, and only 1-3 planes to amortise it over; the gather share only falls from 37 % to 21 %: the boxes are WIDE, not tall) — not the default)
        if (opt == 2 && tt.ok && (long long)tt.nfb * 8 > (long long)g->N * tt.tx * tt.ty && g->ph % 4 == 0) {
            rc = build_one(e, 4);
            if (rc != OMNI_OK) return rc;
        }
    }
    return OMNI_OK;
}
