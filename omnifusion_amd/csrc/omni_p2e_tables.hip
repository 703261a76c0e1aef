// omni_p2e_tables.hip — the one-time geometry tables of pers2equi, built once per handle (omni_geometry.hip calls the builders): the candidate masks
// of the gather blend (p2e_candidates_kernel, omni_p2e_build_candidates) and the per-tile box tables, slot order and walk records of the LDS kernels
// (p2e_tiles_kernel, omni_p2e_build_tiles).  Both go through the tap functions of omni_p2e_common.h, the ones the blends use: exact supersets.
#include "omni_p2e_common.h"

namespace {

// One wave per 64-pixel tile: bit n of cand[row][tile] = any lane valid for patch n.
__global__ __launch_bounds__(256) void p2e_candidates_kernel(P2EArgs a, unsigned long long* cand)
{
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= a.H * a.ntx) return;
    const int i = wave / a.ntx, j = (wave % a.ntx) * 64 + lane;
    const float2 rt = a.row_trig[i];
    const float2 ct = a.col_trig[min(j, a.W - 1)];
    unsigned long long m = 0;
    for (int n = 0; n < a.tab.N; ++n) {
        Taps t;
        const bool v = p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t) && (j < a.W);
        if (__ballot(v) != 0ull) m |= (1ull << n);
    }
    if (lane == 0) cand[wave] = m;
}

// entry: x = n | bw4 << 6 | bh << 16 | (entry 0 only) count << 26 (bw4 = 16-byte chunks per box row, bh = box rows, both <= 512;
// count = covering patches of the tile), y = xa | ymin << 16
template <int TH>                                                  // tile height: P2E_TH (every LDS kernel) or 8 (the one-plane walk kernel, round 5)
__global__ __launch_bounds__(256) void p2e_tiles_kernel(P2EArgs a, uint2* __restrict__ ent, int tiles_x, int ntiles, int epc,
                                                        int* __restrict__ stats)
{
    const int wid = (int)((blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (wid >= ntiles) return;
    const int ti = wid / tiles_x, tj = wid - ti * tiles_x;
    const int col = lane & 31, rsub = lane >> 5;
    const int j = tj * P2E_TW + col;
    const bool jin = j < a.W;
    const float2 ct = a.col_trig[jin ? j : a.W - 1];
    int cnt = 0, maxch = 0, sumch = 0;
    for (int n = 0; n < a.tab.N; ++n) {
        int xmin = 0x7fffffff, xmax = -1, ymin = 0x7fffffff, ymax = -1;
#pragma unroll
        for (int k = 0; k < TH / 2; ++k) {
            const int i = ti * TH + rsub + 2 * k;
            const bool iin = i < a.H;
            const float2 rt = a.row_trig[iin ? i : a.H - 1];
            Taps t;
            p2e_taps(a, n, rt.x, rt.y, ct.x, ct.y, t);
            const float wsum = (t.wa + t.wb) + (t.wc + t.wd);
            if (jin && iin && wsum > 0.0f) {
                xmin = min(xmin, t.x0); xmax = max(xmax, t.x1); ymin = min(ymin, t.y0); ymax = max(ymax, t.y1);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            xmin = min(xmin, __shfl_xor(xmin, o)); xmax = max(xmax, __shfl_xor(xmax, o));
            ymin = min(ymin, __shfl_xor(ymin, o)); ymax = max(ymax, __shfl_xor(ymax, o));
        }
        if (xmax < 0) continue;                                   // wave-uniform: patch n covers no pixel of this tile
        int xa = xmin / epc * epc;
        int bw4 = (xmax / epc * epc + epc - xa) / epc;
        const int bh = ymax - ymin + 1;
        const bool fits = bw4 < 1024 && bh < 1024 && xa < 65536 && ymin < 65536 && bw4 * bh <= P2E_MAX_CHUNKS;
        maxch = max(maxch, fits ? bw4 * bh : P2E_MAX_CHUNKS + 1);
        sumch += fits ? bw4 * bh : (1 << 20);
        if (lane == 0 && cnt < P2E_MAXC && fits)
            ent[(size_t)wid * P2E_MAXC + cnt] = make_uint2((unsigned)n | ((unsigned)bw4 << 6) | ((unsigned)bh << 16),
                                                           (unsigned)xa | ((unsigned)ymin << 16));
        ++cnt;
    }
    if (lane == 0) {
        for (int c = cnt; c < P2E_MAXC; ++c) ent[(size_t)wid * P2E_MAXC + c] = make_uint2(0u, 0u);
        if (cnt <= P2E_MAXC) ent[(size_t)wid * P2E_MAXC].x |= (unsigned)cnt << 26;
        atomicMax(&stats[0], maxch); atomicMax(&stats[1], cnt); atomicMax(&stats[2], sumch);
    }
}
}  // namespace

int omni_p2e_build_candidates(omni_geometry* g, hipStream_t stream)
{
    P2EArgs a;
    int rc = fill_args(a, g, nullptr, nullptr, nullptr, 0, 1, OMNI_LAYOUT_BNCHW);
    if (rc != OMNI_OK) return rc;
    const int waves = g->H * g->ntx;
    hipLaunchKernelGGL(p2e_candidates_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, a, g->cand);
    OMNI_HIP(hipGetLastError());
    // one-time setup: make the table visible to every stream that may use this handle later
    OMNI_HIP(hipStreamSynchronize(stream));
    return OMNI_OK;
}

// Per-tile box tables of the LDS path (one per element size: the 16-byte chunk alignment differs).  One-time setup.
int omni_p2e_build_tiles(omni_geometry* g, hipStream_t stream)
{
    P2EArgs a;
    int rc = fill_args(a, g, nullptr, nullptr, nullptr, 0, 1, OMNI_LAYOUT_BNCHW);
    if (rc != OMNI_OK) return rc;
    g->p2e_tx = (g->W + P2E_TW - 1) / P2E_TW; g->p2e_ty = (g->H + P2E_TH - 1) / P2E_TH;
    if ((long long)g->p2e_tx * g->p2e_ty >= (1ll << 28)) return OMNI_OK;                     // absurd sizes: gather path only
    int* dstats = nullptr;
    OMNI_HIP(hipMalloc((void**)&dstats, 3 * sizeof(int)));
    // sets 0 / 1: P2E_TH-row tiles (4- / 2-byte elements), what every LDS kernel reads; sets 2 / 3: 8-row tiles for the one-plane walk kernel (its slot
    // table only; built when the 4-row set of the element size exists)
    for (int e = 0; e < 4; ++e) {
        auto& tt = g->p2e_tiles[e];
        const int epc = (e & 1) ? 8 : 4, TH = e < 2 ? P2E_TH : 8;
        if (e >= 2 && (!g->p2e_tiles[e - 2].ok || !omni_options().p2e_tile8)) continue;
        const int ty_set = (g->H + TH - 1) / TH;
        const long long ntiles = (long long)g->p2e_tx * ty_set;
        if (hipMalloc((void**)&tt.ent, sizeof(uint2) * (size_t)ntiles * P2E_MAXC) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: out of memory"); }
        if (hipMemsetAsync(dstats, 0, 3 * sizeof(int), stream) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: memset"); }
        if (TH == 8) hipLaunchKernelGGL(p2e_tiles_kernel<8>, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, stream, a, tt.ent, g->p2e_tx, (int)ntiles, epc, dstats);
        else         hipLaunchKernelGGL(p2e_tiles_kernel<P2E_TH>, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, stream, a, tt.ent, g->p2e_tx, (int)ntiles, epc, dstats);
        int hs[3] = {0, 0, 0};
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hs, dstats, sizeof(hs), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: kernel failed"); }
        tt.max_chunks = hs[0]; tt.max_cand = hs[1];
        tt.ok = (hs[0] <= P2E_MAX_CHUNKS && hs[1] <= P2E_MAXC && g->pw % epc == 0) ? 1 : 0;
        tt.sum_chunks = hs[2];
        if (tt.ok) {
            // ---- block order.  A block's duration grows with the number of covering patches of its tile (3.3 us + 2.9 us per patch at
            // cfg 1, tools/trace_resample.py), all blocks of a BASELINE-size launch are resident at once, and the dispatcher deals an XCD's
            // blocks to its 32 CUs round-robin (block b -> XCD b % 8, CU (b / 8) % 32 of it: tools/trace_cu.py) — with 32 tiles per ERP
            // row every CU got ONE column strip of the image and the CU on a patch seam 56 patch-tiles where the median CU has 34; the
            // launch ended when that CU did (17.4 us for blocks of 9.8 us on average).  So: whole bands of tile rows per XCD as before
            // (vertical neighbours share their boxes in one L2), bands dealt to the XCDs by cost (heaviest with lightest), and inside an
            // XCD the tiles sorted by cost and dealt to the 32 round-robin positions in snake order.  Pure speed: any order is correct.
            std::vector<uint2> he((size_t)ntiles * P2E_MAXC);
            if (hipMemcpy(he.data(), tt.ent, sizeof(uint2) * he.size(), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: copy"); }
            const int tx = g->p2e_tx, ty = ty_set, band = omni_options().p2e_band > 0 ? omni_options().p2e_band : std::max(1, ty / 8), nbands = (ty + band - 1) / band;   // (one contiguous range of tile rows per XCD: 15.8 us, FETCH 52 MB; 8-row bands 16.0, 4-row 17.2 / 61 MB, 2-row 19.6 / 85 MB)
            auto cost = [&](int wid) { return 2 + (int)(he[(size_t)wid * P2E_MAXC].x >> 26); };
            std::vector<std::pair<long long, int>> bc(nbands);
            for (int b = 0; b < nbands; ++b) {
                long long c = 0;
                for (int r = b * band; r < std::min(ty, (b + 1) * band); ++r) for (int x = 0; x < tx; ++x) c += cost(r * tx + x);
                bc[b] = {-c, b};
            }
            std::sort(bc.begin(), bc.end());
            std::vector<std::vector<int>> per(8);
            for (int k = 0; k < nbands; ++k) {
                const int r = k / 8, i = k % 8, xcd = (r & 1) ? 7 - i : i, b = bc[k].second;
                for (int row = b * band; row < std::min(ty, (b + 1) * band); ++row) for (int x = 0; x < tx; ++x) per[xcd].push_back(row * tx + x);
            }
            size_t mx = 0;
            for (auto& v : per) {
                std::stable_sort(v.begin(), v.end(), [&](int p, int q) { return cost(p) > cost(q); });
                mx = std::max(mx, v.size());
            }
            const size_t rounds = (mx + 31) / 32;
            tt.nslots = (int)(rounds * 32 * 8);
            std::vector<uint2> ord((size_t)tt.nslots * 4 * P2E_REC, make_uint2(0u, 0u));       // (a 32-byte record = 4 uint2)
            for (int s2 = 0; s2 < tt.nslots; ++s2) ord[(size_t)s2 * 4 * P2E_REC].x = 0xffffffffu;
            auto fbits = [](float f) { unsigned u; memcpy(&u, &f, 4); return u; };
            for (int xcd = 0; xcd < 8; ++xcd)
                for (size_t k = 0; k < per[xcd].size(); ++k) {
                    const size_t r = k / 32, i = k % 32, pos = r * 32 + ((r & 1) ? 31 - i : i);
                    const size_t slot = pos * 8 + (size_t)xcd;
                    const int wid = per[xcd][k];
                    uint2* rec = ord.data() + slot * 4 * P2E_REC;
                    const int cnt = (int)(he[(size_t)wid * P2E_MAXC].x >> 26);
                    rec[0] = make_uint2((unsigned)wid, (unsigned)cnt);
                    for (int c = 0; c < P2E_MAXC; ++c) {
                        const uint2 e2 = he[(size_t)wid * P2E_MAXC + c];
                        const int n = (int)(e2.x & 63u);
                        rec[4 * (c + 1) + 0] = e2;
                        rec[4 * (c + 1) + 1] = make_uint2(fbits(g->p2e.slam[n]), fbits(g->p2e.clam[n]));
                        rec[4 * (c + 1) + 2] = make_uint2(fbits(g->p2e.sphi[n]), fbits(g->p2e.cphi[n]));
                    }
                }
            if (e < 2 && (hipMalloc((void**)&tt.ord, sizeof(uint2) * ord.size()) != hipSuccess ||
                hipMemcpy(tt.ord, ord.data(), sizeof(uint2) * ord.size(), hipMemcpyHostToDevice) != hipSuccess)) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: order table"); }
            // ---- the same slots for p2e_walk_kernel: header {tile | -1, covering patches, pieces per stage (tile-uniform)}, the patch records, the tile's trig
            {
                std::vector<float2> hrow((size_t)g->H), hcol((size_t)g->W);
                if (hipMemcpy(hrow.data(), g->row_trig, sizeof(float2) * hrow.size(), hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(hcol.data(), g->col_trig, sizeof(float2) * hcol.size(), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: trig copy"); }
                // block b of the walk kernel = P2W_WPB waves = the slots WPB b .. WPB b + WPB - 1, all on CU (b / 8) % 32 of XCD b % 8: the tile that
                // the one-wave-per-block order gives to (XCD x, CU c, round r) keeps its CU — slot WPB (((r / WPB) 32 + c) 8 + x) + r % WPB
                const size_t rounds_w = (rounds + P2W_WPB - 1) / P2W_WPB * P2W_WPB;
                tt.nslots_walk = (int)(rounds_w * 32 * 8);
                std::vector<unsigned char> wt((size_t)tt.nslots_walk * P2W_SLOT, 0);
                for (int s2 = 0; s2 < tt.nslots_walk; ++s2) { const unsigned m1 = 0xffffffffu; memcpy(wt.data() + (size_t)s2 * P2W_SLOT, &m1, 4); }
                int hist[P2E_NJMAX + 1] = {0};
                for (int s2 = 0; s2 < tt.nslots; ++s2) {
                    const uint2* rec = ord.data() + (size_t)s2 * 4 * P2E_REC;
                    const size_t x8 = (size_t)s2 % 8, pos = (size_t)s2 / 8, rr = pos / 32, cu = pos % 32;
                    unsigned char* dst = wt.data() + ((((rr / P2W_WPB) * 32 + cu) * 8 + x8) * P2W_WPB + rr % P2W_WPB) * P2W_SLOT;
                    const int wid = (int)rec[0].x, cnt = (int)rec[0].y;
                    int njt = 1;
                    if (wid >= 0)
                        for (int c = 0; c < cnt && c < P2E_MAXC; ++c) {
                            const unsigned e0 = rec[4 * (c + 1)].x;
                            const int nchunk = (int)((e0 >> 6) & 1023) * (int)((e0 >> 16) & 1023);
                            njt = std::max(njt, (nchunk + 63) / 64);
                        }
                    if (wid >= 0) ++hist[std::min(njt, P2E_NJMAX)];
                    const unsigned hdr[8] = {(unsigned)wid, (unsigned)cnt, (unsigned)njt, 0u, 0u, 0u, 0u, 0u};
                    memcpy(dst, hdr, 32);
                    memcpy(dst + P2W_OFF_PATCH, rec + 4, 32 * P2E_MAXC);
                    if (wid >= 0) {
                        const int ti = wid / tx, tj = wid - ti * tx;
                        float2* tg = reinterpret_cast<float2*>(dst + P2W_OFF_TRIG);
                        for (int cc = 0; cc < P2E_TW; ++cc) tg[cc] = hcol[(size_t)std::min(tj * P2E_TW + cc, g->W - 1)];
                        for (int r = 0; r < TH; ++r) tg[P2E_TW + r] = hrow[(size_t)std::min(ti * TH + r, g->H - 1)];
                    }
                }
                if (omni_options().e2p_verbose)
                    fprintf(stderr, "[omni] pers2equi %dx%d <- %dx%d, %d-byte elements: tiles by KiB pieces per stage (largest box of the tile): 1:%d 2:%d 3:%d 4:%d 5:%d 6:%d 7:%d 8:%d\n",
                            g->H, g->W, g->ph, g->pw, 16 / epc, hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], hist[8]);
                if (hipMalloc((void**)&tt.walk, wt.size()) != hipSuccess ||
                    hipMemcpy(tt.walk, wt.data(), wt.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dstats); OMNI_FAIL(OMNI_ERR_HIP, "omni_p2e_build_tiles: walk table"); }
            }
        }
        (void)hipFree(tt.ent); tt.ent = nullptr;                     // the kernels read only the ordered table (tt.ord)
        if (omni_options().e2p_verbose)
            fprintf(stderr, "[omni] pers2equi %dx%d <- %d patches %dx%d, %d-byte elements: largest tap box %d chunks, <= %d patches and <= %d chunks per %dx%d tile -> %s\n",
                    g->H, g->W, g->N, g->ph, g->pw, 16 / epc, hs[0], hs[1], hs[2], TH, P2E_TW, tt.ok ? "LDS path" : "gather path");
    }
    (void)hipFree(dstats);
    return OMNI_OK;
}
