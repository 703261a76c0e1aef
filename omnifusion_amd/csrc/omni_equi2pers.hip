// omni_equi2pers.hip — ERP -> N tangent-plane patches (gfx950).
//
// Replaces /root/reference/equi_pers/equi2pers_v3.py:20-122:
//   K1  CPU grid build + repeat(bs) + H2D (:24-109)        -> evaluated in-kernel, closed form
//   K2  F.grid_sample(bilinear, border, align_corners=True) (:111) -> gather below
//   K3  F.unfold + reshape to [B,C,ph,pw,N] (:112-113)      -> fused into the store (LDS transpose)
//   K4  uv2xyz rays (:13-18,115-118), uv (:120-121)         -> omni_equi2pers_aux
//   K5  dead erp_mask work (:49-74)                         -> dropped
//
// Geometry.  The reference evaluates (fp32)  rho=sqrt(x^2+y^2), c=atan(rho),
//   lat = asin(cos c sin p1 + y sin c cos p1 / rho),
//   lon = l0 + atan2(x sin c, rho cos p1 cos c - y sin p1 sin c)             (:95-100)
// With sin c = rho/sqrt(1+rho^2), cos c = 1/sqrt(1+rho^2) this is identically
//   lat = asin((sin p1 + y cos p1) / sqrt(1+x^2+y^2)),   lon = l0 + atan2(x, cos p1 - y sin p1)
// which needs two transcendental calls instead of six (the reference's 0/0 at an exact patch
// centre, quirk q4, is reproduced explicitly in e2p_lonlat) and differs from the reference's fp32 chain by coordinate round-off only (a few 1e-4 px
// away from the poles; tests/ carry the tolerance).
//
// Memory behaviour: one thread owns one (or four consecutive) sample position(s) and loops
// over all B*C image planes, so geometry is evaluated once and amortised; ERP reads are
// 4-byte gathers with wave-level locality (a wave walks a short curve on the ERP), patch
// writes are fully coalesced.  HBM-bound: algorithmic bytes B*C*(H*W + ph*pw*N)*sizeof(T).
//
// This unit: the C entry points, the choice of kernel (launch_e2p) and the default planar path — e2p_box_kernel with its work-table scheduler.
// omni_e2p_common.h: argument block, tap helpers, e2p_lds_kernel | omni_e2p_ref.hip: reference layout and direct gathers | omni_e2p_tables.hip: the
// per-geometry tables | omni_equi2pers_bwd.hip: the backward.
#include "omni_e2p_common.h"

namespace {

// ------------------------------------------------------------------ planar output, one wave per small sample tile (default)
// e2p_lds_kernel (omni_e2p_common.h) synchronises a 256-thread block once per image plane and keeps two boxes in flight; measured 46 us for the
// 164 MB of BASELINE cfg 4 (3.6 TB/s), its waves parked at the barrier / the DMA wait most of the time.  Here ONE WAVE owns a
// tile of 8 x 32 samples (4 horizontally adjacent ones per lane: one 16-byte store per lane and plane) and streams the B*C image planes through a ring of NB LDS slots: per plane the bounding box of the tile's taps on
// the ERP arrives by LDS-DMA (buffer_load ... lds, 1 KiB pieces), the wave waits with a COUNTED s_waitcnt for exactly the
// pieces of the stage it is about to read (the NB-1 younger stages and the stores stay in flight), takes the taps from LDS and
// stores 4 samples per lane.  No barrier, no block-level reduction: the box of every tile is a constant of the geometry (table
// built once per handle from the same sampling coordinates).  The stage loop is instantiated per NJ = pieces per box, so every
// wait count and piece loop is a compile-time constant.  Tiles whose box exceeds the slot (the pole inside or next to the
// tile) are listed per geometry and handled by extra blocks of the same launch with direct gathers, one per (tile, batch item).

// NPX results of one lane -> NPX adjacent elements, one store
template <typename T> struct E2BStore4;
template <> struct E2BStore4<float> {
    static __device__ __forceinline__ void st(float* p, const float (&r)[2]) { *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]); }
    static __device__ __forceinline__ void st_nt(float* p, const float (&r)[2])
    {
        typedef float v2f __attribute__((ext_vector_type(2)));
        const v2f v = {r[0], r[1]};
        __builtin_nontemporal_store(v, reinterpret_cast<v2f*>(p));
    }
    static __device__ __forceinline__ void st(float* p, const float (&r)[4]) { *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]); }
    // non-temporal form: the output is never re-read by this kernel (the ERP boxes are), and at 16 panoramas — 327 MB per launch, more than
    // the 256-MB memory-side cache — it is what keeps the launch at the 8-panorama rate (106 -> 64-74 us; 8 panoramas 38.5 -> 36.8).  sc1
    // (write-through, line dropped from the XCD's L2) measured no better than plain stores.
    static __device__ __forceinline__ void st_nt(float* p, const float (&r)[4])
    {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f v = {r[0], r[1], r[2], r[3]};
        __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p));
    }
};
template <> struct E2BStore4<__half> {
    static __device__ __forceinline__ void st(__half* p, const float (&r)[2])
    { __half2 v = __floats2half2_rn(r[0], r[1]); *reinterpret_cast<unsigned*>(p) = *reinterpret_cast<unsigned*>(&v); }
    static __device__ __forceinline__ void st_nt(__half* p, const float (&r)[2])
    { __half2 v = __floats2half2_rn(r[0], r[1]); __builtin_nontemporal_store(*reinterpret_cast<unsigned*>(&v), reinterpret_cast<unsigned*>(p)); }
    static __device__ __forceinline__ void st(__half* p, const float (&r)[4])
    { __half2 lo = __floats2half2_rn(r[0], r[1]), hi = __floats2half2_rn(r[2], r[3]); uint2 v; v.x = *reinterpret_cast<unsigned*>(&lo); v.y = *reinterpret_cast<unsigned*>(&hi); *reinterpret_cast<uint2*>(p) = v; }
    static __device__ __forceinline__ void st_nt(__half* p, const float (&r)[4])
    {
        __half2 lo = __floats2half2_rn(r[0], r[1]), hi = __floats2half2_rn(r[2], r[3]);
        typedef unsigned v2u __attribute__((ext_vector_type(2)));
        const v2u v = {*reinterpret_cast<unsigned*>(&lo), *reinterpret_cast<unsigned*>(&hi)};
        __builtin_nontemporal_store(v, reinterpret_cast<v2u*>(p));
    }
};

template <typename T, int NBMAX, bool ROWMAP, int NPX = E2B_NPX>
__global__ __launch_bounds__(64, 4) void e2p_box_kernel(E2PArgs a, const uint4* __restrict__ work, int tiles_x, int tiles_pp, unsigned tensor_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char e2b_smem[];        // the ONLY LDS object of this kernel
    constexpr int EPC = 16 / (int)sizeof(T), TILE_H = 2 * NPX, LPR = E2B_TW / NPX;   // tile rows; lanes per tile row of the direct lane map
    const int lane = threadIdx.x;
    long long tr0 = 0, tr1 = 0;
    if (OMNI_DBG(a, 16)) tr0 = wall_clock64();
    // block -> (tile, plane range): the work table of this (geometry, plane count), e2p_work_table().  x = tile | gather flag << 31,
    // y = first plane | planes << 16, (z, w) = the tile's box entry.  Block b runs on XCD b % 8 and the table keeps the tiles of one
    // ERP region on one XCD (an ERP pixel is sampled by 2.1 patches on average; only tiles on ONE XCD share an L2).
    const uint4 wk = work[blockIdx.x];                             // wave-uniform address: scalar load
    const int np = (int)(wk.y >> 16), p_start = (int)(wk.y & 0xffffu);
    if (np == 0) return;                                           // padding
    const bool fb_block = (wk.x >> 31) != 0;
    const int wid = (int)(wk.x & 0x7fffffffu);
    const uint2 e = make_uint2(wk.z, wk.w);
    const int n = wid / tiles_pp, t = wid - n * tiles_pp;
    const int th0 = (t / tiles_x) * TILE_H, tw0 = (t % tiles_x) * E2B_TW;
    const int W = a.W, H = a.H;
    // lane -> samples.  ROWMAP (2-byte elements): lane computes (row lane/32 + 2k, column lane%32) — a half-wave, the conflict group of
    // ds_read2_b32, reads the taps of 32 consecutive samples of one row — and the results are transposed inside each quad before the
    // store.  Otherwise (4-byte elements) lane computes the 4 adjacent samples (row lane/8, columns 4 (lane%8) + k) it stores; measured
    // per shape: fp32 22 vs 27 us at P = 128 and equal at P = 256 in favour of the direct form, fp16 cfg5 72 vs 126 us in favour of ROWMAP.
    const int w = ROWMAP ? tw0 + (lane & 31) : tw0 + NPX * (lane % LPR), hb = ROWMAP ? th0 + (lane >> 5) : th0 + lane / LPR;
    const int xs4 = (int)(e.y & 0xffff), ymin = (int)(e.y >> 16), bw4 = (int)(e.x & 4095), bh = (int)((e.x >> 12) & 4095);
    const int pitch = bw4 * EPC;

    // ---- the sampling coordinates of my NPX samples go out FIRST (plain loads, hand-counted: the compiler does not see them), the first
    // NB boxes right behind them, and the taps are computed while both travel: a block's set-up was two dependent round trips in front
    // of its first DMA (work entry -> coordinates; 2.3 us of a third-of-a-tile block's 5.6 us), now the boxes ride on the second
    typedef float e2b_v2f __attribute__((ext_vector_type(2)));
    e2b_v2f cxy[NPX];
    const bool tab = a.ixy != nullptr;
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        const int hh = ROWMAP ? hb + 2 * k : hb, ww = ROWMAP ? w : w + k;
        if (tab) {
            const float2* q = a.ixy + ((size_t)n * a.ph + hh) * a.pw + ww;
            asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(cxy[k]) : "v"(q) : "memory");
        } else {
            float ix, iy;
            e2p_sample_xy(a, n, hh, ww, ix, iy);
            cxy[k].x = ix; cxy[k].y = iy;
        }
    }
    const int plane = a.ph * a.pw;
    const size_t img_plane = (size_t)H * W;
    const e2b_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.erp), (short)0, (int)tensor_bytes, 0x00020000);
    const unsigned rowb = (unsigned)W * (unsigned)sizeof(T), planeb = (unsigned)img_plane * (unsigned)sizeof(T);
    const int nchunk = bw4 * bh, njj = (nchunk + 63) >> 6;
    unsigned g[E2B_NJMAX];                                          // byte offset of my chunk of piece q inside an image plane
    auto prologue = [&]<int NJ>(std::integral_constant<int, NJ>) {
        constexpr int NBR = E2B_RING_KB / NJ >= 4 ? 4 : E2B_RING_KB / NJ >= 2 ? 2 : 1;
        constexpr int NB = NBR < NBMAX ? NBR : NBMAX;
        constexpr unsigned slot_bytes = NJ * 1024u;
        const float rbw = __builtin_amdgcn_rcpf((float)bw4);
#pragma unroll
        for (int q = 0; q < NJ; ++q) {
            const int qc = q * 64 + lane;
            const int rr = (int)(((float)qc + 0.5f) * rbw);                    // qc / bw4, exact for qc, bw4 <= 4096
            int gx = xs4 + (qc - rr * bw4) * EPC;
            if (gx >= W) gx -= W;                                                 // the box wraps at the seam
            g[q] = qc < nchunk ? (unsigned)(ymin + rr) * rowb + (unsigned)gx * (unsigned)sizeof(T) : 0x80000000u;   // past the end: zeros
            if (OMNI_DBG(a, 64) && (qc & 63) >= 40) g[q] = 0x80000000u;   // (debug bit 64: 3/8 of every piece's lanes read nothing — the volume packed row spans would move)
        }
        if (!OMNI_DBG(a, 2)) {
#pragma unroll
            for (int d = 0; d < NB; ++d) {
                const unsigned so = OMNI_DBG(a, 32) ? 0u : (unsigned)(p_start + d) * planeb;       // (debug bit 32: every plane reads plane 0 — no input traffic)
#pragma unroll
                for (int q = 0; q < NJ; ++q) e2b_dma16(rs, e2b_smem + (unsigned)d * slot_bytes + q * 1024, g[q], so);
            }
            e2b_wait_vm<NB * NJ>();                                 // the coordinates are older than the NB * NJ pieces: they have landed
        } else e2b_wait_vm<0>();
    };
    if (fb_block) e2b_wait_vm<0>();
    else switch (njj) {
    case 1: prologue(std::integral_constant<int, 1>()); break;
    case 2: prologue(std::integral_constant<int, 2>()); break;
    case 3: prologue(std::integral_constant<int, 3>()); break;
    case 4: prologue(std::integral_constant<int, 4>()); break;
    case 5: prologue(std::integral_constant<int, 5>()); break;
    case 6: prologue(std::integral_constant<int, 6>()); break;
    case 7: prologue(std::integral_constant<int, 7>()); break;
    default: prologue(std::integral_constant<int, 8>()); break;
    }
    // ---- taps of my NPX samples: LDS element offsets inside the box + ATen's four weights
    int r0[NPX], r1[NPX];
    float w00[NPX], w01[NPX], w10[NPX], w11[NPX];
    int gx0[NPX], gy0[NPX], gy1[NPX];                              // (fallback path: absolute taps)
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        asm volatile("" : "+v"(cxy[k]));                           // (use only behind the wait above)
        const float ix = cxy[k].x, iy = cxy[k].y;
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float tx = ix - fx, ty = iy - fy, ex = 1.0f - tx, ey = 1.0f - ty;
        w00[k] = ey * ex; w01[k] = ey * tx; w10[k] = ty * ex; w11[k] = ty * tx;
        const int y1 = min(y0 + 1, H - 1);
        gx0[k] = x0; gy0[k] = y0; gy1[k] = y1;
        int c0 = x0 - xs4;                                         // column inside the (seam-wrapping) box
        if (c0 < 0) c0 += W;
        if (x0 + 1 >= W) {
            // ix is clamped to W-1: tx == 0, the +1 column is outside the image and its weights (w01, w11) are exactly 0.  Read the
            // pair (x0-1, x0) instead and move the x0 weights to the pair's SECOND element: e2p_blend then returns
            // 0 + (v00 w00 + v10 w10) with the same roundings, and nothing outside the image row is read.
            c0 -= 1;
            w01[k] = w00[k]; w00[k] = 0.0f; w11[k] = w10[k]; w10[k] = 0.0f;
        }
        r0[k] = (y0 - ymin) * pitch + c0;
        r1[k] = (y1 - ymin) * pitch + c0;
    }
    const size_t out_bstride = (size_t)a.tab.N * a.C * plane;
    // ROWMAP: after the transpose inside each group of NPX lanes, lane l holds row hb + 2 (l % NPX), columns NPX ((l % 32) / NPX) .. + NPX - 1 of the tile
    const int b0 = p_start / a.C, c0p = p_start - b0 * a.C;        // batch item / channel of my first plane
    T* out = (T*)a.pers + (size_t)b0 * out_bstride + ((size_t)n * a.C + c0p) * plane +
             (ROWMAP ? (size_t)(hb + 2 * (lane % NPX)) * a.pw + tw0 + NPX * ((lane & 31) / NPX) : (size_t)hb * a.pw + w);
    const size_t bskip = out_bstride - (size_t)a.C * plane;

    if (fb_block) {
        // ---- direct gathers (same taps, same fma chain) for a tile whose box does not fit a slot: planes [p_start, p_start + np), FBU at a
        // time — their pair loads are all in flight before the first is used (a block of these is a chain of memory round trips and
        // nothing else)
        const T* img = (const T*)a.erp + (size_t)p_start * img_plane;
        T* dstb = out;
        int cc = c0p;
        int g0[NPX], g1[NPX];
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const int sh = (gx0[k] + 1 >= W) ? 1 : 0;              // pair moved one column left (see above)
            g0[k] = gy0[k] * W + gx0[k] - sh; g1[k] = gy1[k] * W + gx0[k] - sh;
        }
        constexpr int FBU = sizeof(T) == 4 ? 2 : 3;              // (three fp32 planes: 48 result registers, and the kernel spills at 128)
        for (int p = 0; p < np; p += FBU) {
            float v[FBU][NPX][4];
#pragma unroll
            for (int u = 0; u < FBU; ++u) {
                const T* im = img + (size_t)min(u, np - 1 - p) * img_plane;      // (past the range: the last plane again, result unused)
#pragma unroll
                for (int k = 0; k < NPX; ++k) {
                    Pair<T>::ld(im + g0[k], v[u][k][0], v[u][k][1]);
                    Pair<T>::ld(im + g1[k], v[u][k][2], v[u][k][3]);
                }
            }
#pragma unroll
            for (int u = 0; u < FBU; ++u) {
                if (p + u < np) {
                    float r[NPX];
#pragma unroll
                    for (int k = 0; k < NPX; ++k) r[k] = e2p_blend(v[u][k][0], v[u][k][1], v[u][k][2], v[u][k][3], w00[k], w01[k], w10[k], w11[k]);
                    if (ROWMAP) e2b_transpose(r, lane);
                    E2BStore4<T>::st(dstb, r);
                    dstb += plane;
                    if (++cc == a.C) { cc = 0; dstb += bskip; }
                }
            }
            img += (size_t)FBU * img_plane;
        }
        return;
    }
    // nothing but LDS-DMA pieces and stores below
    if (OMNI_DBG(a, 16)) tr1 = wall_clock64();

    auto run = [&]<int NJ>(std::integral_constant<int, NJ>) {
        // ring of E2B_RING_KB 1-KiB pieces per wave: a box of NJ pieces gets NB = min(NBMAX, largest power of two <= RING / NJ) slots of
        // exactly NJ KiB — small boxes (the common case) keep 4 stages in flight, the rare large ones 2 or 1, in the same LDS footprint
        constexpr int NBR = E2B_RING_KB / NJ >= 4 ? 4 : E2B_RING_KB / NJ >= 2 ? 2 : 1;
        constexpr int NB = NBR < NBMAX ? NBR : NBMAX;
        constexpr unsigned slot_bytes = NJ * 1024u;
        auto issue = [&](int p, int slot) {
            if (OMNI_DBG(a, 2)) return;
            unsigned char* dst = e2b_smem + (unsigned)slot * slot_bytes;
            const unsigned so = OMNI_DBG(a, 32) ? 0u : (unsigned)(p_start + p) * planeb;
#pragma unroll
            for (int q = 0; q < NJ; ++q) e2b_dma16(rs, dst + q * 1024, g[q], so);
        };
        T* dst = out;
        int cc = c0p;
        auto consume = [&](int slot, float (&r)[NPX]) {
            const unsigned char* box = e2b_smem + (unsigned)slot * slot_bytes;
#pragma unroll
            for (int k = 0; k < NPX; ++k) {
                float a0, a1, b0, b1;
                E2BPair<T>::ld(box, r0[k], a0, a1);
                E2BPair<T>::ld(box, r1[k], b0, b1);
                r[k] = e2p_blend(a0, a1, b0, b1, w00[k], w01[k], w10[k], w11[k]);
            }
            if (ROWMAP) e2b_transpose(r, lane);
        };
        auto store = [&](const float (&r)[NPX]) {
            if (OMNI_DBG(a, 128)) { if (lane == 0) E2BStore4<T>::st_nt(dst, r); }      // (debug bit 128: the store instruction with ONE active lane — its acknowledge without its bytes)
            else if (!OMNI_DBG(a, 1)) { if (a.store_mode) E2BStore4<T>::st_nt(dst, r); else E2BStore4<T>::st(dst, r); }
            dst += plane;
            if (++cc == a.C) { cc = 0; dst += bskip; }
        };
        // groups of NB stages, then np % NB single stages (NB <= np: the work table never cuts a range shorter).  vmcnt counts, per stage s of a
        // group (in-order completion; the ONE store of a stage counts like a DMA piece):  first group  (NB-1) NJ + s   |  middle  (NB-1)(1 + NJ)
        //                                             last group   (NB-1) + (NB-1-s) NJ   |  only group  (NB-1-s) NJ + s
        // (round 3: issuing a stage's refill BEFORE its store, so that a write acknowledge has two stage-times instead of one before a
        //  counted wait can stall on it, measured no different: 39.3 vs 38.5 us — the stores are not what the waits wait for)
        const int groups = np / NB;                                 // (the first NB stages went out in the prologue)
        auto group = [&]<int KIND>(std::integral_constant<int, KIND>, int p0) {
            [&]<int... S>(std::integer_sequence<int, S...>) {
                (([&] {
                    constexpr int CNT = KIND == 0 ? (NB - 1) * NJ + S : KIND == 1 ? (NB - 1) * (1 + NJ)
                                      : KIND == 2 ? (NB - 1) + (NB - 1 - S) * NJ : (NB - 1 - S) * NJ + S;
                    e2b_wait_vm<CNT>();
                    float r[NPX];
                    consume(S, r);
                    store(r);
                    if (KIND <= 1) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); issue(p0 + S + NB, S); }
                }()), ...);
            }(std::make_integer_sequence<int, NB>());
        };
        if (groups == 1) group(std::integral_constant<int, 3>(), 0);
        else {
            group(std::integral_constant<int, 0>(), 0);
            for (int gi = 1; gi + 1 < groups; ++gi) group(std::integral_constant<int, 1>(), gi * NB);
            group(std::integral_constant<int, 2>(), (groups - 1) * NB);
        }
        for (int p = groups * NB; p < np; ++p) {                 // an odd plane count (3 planes of ONE panorama): the rest, one stage at a time
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(p, 0);
            e2b_wait_vm<0>();
            float r[NPX];
            consume(0, r);
            store(r);
        }
    };
    switch (njj) {
    case 1: run(std::integral_constant<int, 1>()); break;
    case 2: run(std::integral_constant<int, 2>()); break;
    case 3: run(std::integral_constant<int, 3>()); break;
    case 4: run(std::integral_constant<int, 4>()); break;
    case 5: run(std::integral_constant<int, 5>()); break;
    case 6: run(std::integral_constant<int, 6>()); break;
    case 7: run(std::integral_constant<int, 7>()); break;
    default: run(std::integral_constant<int, 8>()); break;
    }
    if (OMNI_DBG(a, 16)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 && a.trace) {
            long long* t = a.trace + 4 * (size_t)blockIdx.x;
            t[0] = tr0; t[1] = tr1; t[2] = wall_clock64();
            t[3] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | ((long long)njj << 40);
        }
    }
}

// ------------------------------------------------------------------ aux outputs
// xyz[n,:,h,w] = (cos lat sin lon, cos lat cos lon, sin lat) from the UNWRAPPED lon (:13-18,115-118),
// here without further trig:  cos lat * (sin|cos)(l0 + atan2(x,q)) = inv * (..) algebraically.
// uv[b,:,h,a] = strip[h, a*N + b]  (:106-108,120 — the reference reinterprets the [ph, N*pw] strip
// as [ph, pw, N]).
__global__ __launch_bounds__(256) void e2p_aux_kernel(E2PArgs a, float* xyz, float* uv)
{
    const int N = a.tab.N, plane = a.ph * a.pw;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * plane) return;
    const int n = idx / plane, e = idx % plane, h = e / a.pw, w = e % a.pw;
    if (xyz) {
        float lon, lat, x, q, t, inv;
        e2p_lonlat(a, n, h, w, lon, lat, x, q, t, inv);
        const float sl = a.tab.slam[n], cl = a.tab.clam[n];
        const bool q4 = lat != lat;                  // quirk q4: NaN latitude poisons the whole ray
        xyz[((size_t)n * 3 + 0) * plane + e] = q4 ? lat : inv * (sl * q + cl * x);
        xyz[((size_t)n * 3 + 1) * plane + e] = q4 ? lat : inv * (cl * q - sl * x);
        xyz[((size_t)n * 3 + 2) * plane + e] = q4 ? lat : fminf(1.0f, fmaxf(-1.0f, t * inv));
    }
    if (uv) {
        const int s = w * N + n;                     // here (n, w) play the roles (b, a)
        const int n2 = s / a.pw, w2 = s % a.pw;
        float lon, lat, x, q, t, inv, u, v;
        e2p_lonlat(a, n2, h, w2, lon, lat, x, q, t, inv);
        e2p_uv(lon, lat, u, v);
        uv[((size_t)n * 2 + 0) * plane + e] = u;
        uv[((size_t)n * 2 + 1) * plane + e] = v;
    }
}

// ---- work table of e2p_box_kernel for one plane count: which (tile, plane range) each block processes.
// A block's life is set-up (~2.6 us: table entry -> sampling coordinates -> taps) + np stages; with ONE block per tile, 4372 streaming blocks of
// ~16 us each on the 3072 wave slots of the chip (12 per CU: the LDS ring) are 1.42 rounds — per-block time stamps (tools/trace_resample.py,
// profiles/r03a_trace.txt) show the chip full only from 8 to 24 us of a 36-us launch: the gather blocks of the pole tiles took 60 % of the slots
// for the first 5 us, and the second round ran at 40 % occupancy.  List scheduling, longest first: every XCD gets as many whole tiles as it has
// slots, the remaining tiles are cut into `split` plane ranges (short blocks that fill the slots the long ones free, and end together), and the
// gather blocks — the shortest — come last.  Block b runs on XCD b % 8: column x of the table holds tiles of ERP region x only.
struct E2PWork { uint4* dev = nullptr; int nblocks = 0; };

// LDS one wave of e2p_box_kernel really uses for a geometry whose largest staged box is `max_chunks` 16-byte chunks: NB(NJ) slots of NJ KiB for the
// largest NJ (the ring is addressed slot by slot, so smaller boxes use less).  cfg 1 (boxes to 6 KiB): 12 KiB; cfg 3 / cfg 5 (1-2 KiB): 4 KiB — LDS
// then admits far more waves than the registers (16 per CU)
static size_t e2b_lds_bytes(int max_chunks, int nbmax)
{
    const int njmax = std::max(1, (max_chunks + 63) / 64);
    int kb = 1;
    for (int nj = 1; nj <= std::min(njmax, E2B_NJMAX); ++nj) {
        const int nbr = E2B_RING_KB / nj >= 4 ? 4 : E2B_RING_KB / nj >= 2 ? 2 : 1;
        kb = std::max(kb, std::min(nbr, nbmax) * nj);
    }
    return (size_t)std::max(kb, njmax) * 1024;
}

template <int E>
int e2p_work_table(const omni_geometry* gc, int planes, int nbmax, hipStream_t stream, E2PWork& out)
{
    omni_geometry* g = const_cast<omni_geometry*>(gc);             // (the cache is a mutable part of the handle)
    auto& tt = g->e2p_boxes[E];
    const OmniOptions& o = omni_options();
    // wave slots per CU the schedule plans for: what the kernel's LDS footprint admits (e2b_lds_bytes: 12 KiB at cfg 1 -> 12 or 13), at most the 16
    // that 108 registers per wave admit
    const int slots_lds = (int)std::min<size_t>(16, (160 * 1024) / std::max<size_t>(1024, e2b_lds_bytes(tt.max_chunks, nbmax)));
    const int slots_cu = o.e2p_slots > 0 ? o.e2p_slots : std::min(slots_lds, 12) == 12 ? 12 : slots_lds, split = o.e2p_split > 0 ? o.e2p_split : 3,
              fbp = o.e2p_fb_planes > 0 && o.e2p_fb_planes < 90 ? o.e2p_fb_planes : std::min(tt.norder < slots_cu * omni_num_cus() ? 6 : 12, planes);   // (shorter where the launch is under one round: P = 128)
    // key = everything the table depends on: the plane count and the option set (NOT the channel count: the table holds plane ranges, the
    // kernel splits a plane index into (batch item, channel) itself — B * 3 and 3 B * 1 planes share one table).  Every field whole (ADVICE r3:
    // `e2p_fb_pos & 3` made 4 an alias of 0).
    const long long key = ((long long)planes << 40) | ((long long)(slots_cu & 0xff) << 32) | ((long long)(split & 0xff) << 24) | ((long long)(fbp & 0xff) << 16) |
                          ((long long)(nbmax & 0xf) << 12) | ((long long)(o.e2p_fb_planes >= 98 ? o.e2p_fb_planes - 97 : 0) << 10) | ((long long)(o.e2p_fb_pos & 7) << 7) |
                          ((long long)((o.e2p_full + 1) & 0x7f));
    std::lock_guard<std::mutex> lk(g->work_mu);
    for (auto& w : tt.work) if (w.key == key) { out.dev = w.dev; out.nblocks = w.nblocks; return OMNI_OK; }
    {   // a new plane count under capture cannot be served (an allocation and a synchronous copy would invalidate the capture): like a new
        // geometry, it must have been run once before the capture starts
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive)
            OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers: first use of a plane count (B * C) on this geometry while its stream is being captured (run the shape once before capturing)");
    }
    const int slots_xcd = slots_cu * (omni_num_cus() / 8);
    std::vector<std::vector<uint4>> col(8);
    auto seg = [&](int wid, bool fb, int p0, int np) { return make_uint4((unsigned)wid | (fb ? 0x80000000u : 0u), (unsigned)p0 | ((unsigned)np << 16), tt.h_ent[wid].x, tt.h_ent[wid].y); };
    // streaming tiles, in the region order of the geometry (order[k]: XCD k % 8)
    std::vector<std::vector<int>> tiles(8);
    for (int k = 0; k < tt.norder; ++k) if (tt.h_order[k] >= 0) tiles[k % 8].push_back(tt.h_order[k]);
    const int parts = std::max(1, std::min(split, planes / std::max(1, nbmax)));
    for (int x = 0; x < 8; ++x) {
        const int nt = (int)tiles[x].size();
        // whole tiles while they fill the slots exactly once; the rest in `parts` ranges (all of one range first: blocks that start together run the same planes)
        int nfb_x = 0;
        for (int f = 0; f < tt.nfb; ++f) if ((tt.h_region[tt.h_fb[f]] & 7) == x) nfb_x += (planes + fbp - 1) / fbp;
        const int first = o.e2p_fb_pos == 0 ? std::max(0, slots_xcd - nfb_x) : slots_xcd;   // slots left for whole tiles in round one
        const int nfull = nt <= first ? nt : (o.e2p_full >= 0 ? std::min(nt, first * o.e2p_full / 100) : first);
        auto gathers = [&]() {
            if (o.e2p_fb_planes == 99) return;                         // (tuning: no gather blocks at all — results wrong, timing of the streaming part)
            for (int f = 0; f < tt.nfb; ++f)
                if ((tt.h_region[tt.h_fb[f]] & 7) == x)
                    for (int p0 = 0; p0 < planes; p0 += fbp) col[x].push_back(seg(tt.h_fb[f], true, p0, std::min(fbp, planes - p0)));
        };
        // (the gather blocks go FIRST, 12 planes each: latency-bound blocks about as long as a whole streaming tile, on 1 slot in 13 — as a tail
        //  of 3-plane blocks they cost 5 us: 36.4 -> 33.4 us, 16 panoramas 69 -> 64 us)
        const int fb_pos = o.e2p_fb_pos == 0 ? 3 : o.e2p_fb_pos;   // 3 = first (default): the longest blocks of the launch, beside the whole tiles
        if (fb_pos == 3) gathers();
        if (o.e2p_fb_planes == 98) { gathers(); continue; }            // (tuning: ONLY the gather blocks)
        for (int i = 0; i < nfull; ++i) col[x].push_back(seg(tiles[x][i], false, 0, planes));
        if (fb_pos == 1) gathers();
        for (int q = 0; q < parts; ++q) {
            const int p0 = (int)((long long)planes * q / parts), p1 = (int)((long long)planes * (q + 1) / parts);
            for (int i = nfull; i < nt; ++i) col[x].push_back(seg(tiles[x][i], false, p0, p1 - p0));
            if (fb_pos == 2 && q == 0) gathers();
        }
        if (fb_pos == 4) gathers();
    }
    // (gather tiles: ranges of fbp planes, spread over the XCDs — behind the whole tiles or last, see above)
    size_t mx = 0;
    for (auto& c : col) mx = std::max(mx, c.size());
    std::vector<uint4> tab(mx * 8, make_uint4(0u, 0u, 0u, 0u));
    for (int x = 0; x < 8; ++x) for (size_t i = 0; i < col[x].size(); ++i) tab[i * 8 + x] = col[x][i];
    if (tab.empty()) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: empty work table");
    if (tt.work.size() >= 256) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers: more than 256 distinct plane counts / option sets on one geometry handle (omni_geometry_cache_clear() drops them)");
    uint4* dev = nullptr;
    OMNI_HIP(hipMalloc((void**)&dev, sizeof(uint4) * tab.size()));
    if (hipMemcpy(dev, tab.data(), sizeof(uint4) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); OMNI_FAIL(OMNI_ERR_HIP, "omni_equi2pers: work table upload"); }
    // a table lives as long as its geometry handle (omni_geometry.hip frees them with it; a handle a hipGraph holds is pinned and never
    // destroyed): a launch in flight on another stream, or a captured graph, may hold the pointer — never freed here (the FIFO
    // that was here freed tables under running kernels).  A table is 16 B per block, ~100 KB; one per plane count seen.
    tt.work.push_back({key, dev, (int)tab.size()});
    out.dev = dev; out.nblocks = (int)tab.size();
    return OMNI_OK;
}

template <typename T, int NBMAX>
int launch_e2b_nb(const E2PArgs& a, const omni_geometry* g, int B, int C, size_t tensor_bytes, hipStream_t stream)
{
    constexpr int E = sizeof(T) == 2 ? 1 : 0;
    const auto& tt = g->e2p_boxes[E];
    E2PWork wk;
    int rc = e2p_work_table<E>(g, B * C, NBMAX, stream, wk);
    if (rc != OMNI_OK) return rc;
    const int njmax = (tt.max_chunks + 63) / 64;
    const size_t lds = e2b_lds_bytes(tt.max_chunks, NBMAX);
    (void)njmax;
    if (tt.th == 8) hipLaunchKernelGGL((e2p_box_kernel<T, NBMAX, sizeof(T) == 2, 4>), dim3(wk.nblocks), dim3(64), lds, stream, a, (const uint4*)wk.dev, tt.tx, tt.tx * tt.ty,
                                       (unsigned)tensor_bytes);
    else            hipLaunchKernelGGL((e2p_box_kernel<T, NBMAX, sizeof(T) == 2, 2>), dim3(wk.nblocks), dim3(64), lds, stream, a, (const uint4*)wk.dev, tt.tx, tt.tx * tt.ty,
                                       (unsigned)tensor_bytes);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

template <typename T>
int launch_e2b(const E2PArgs& a, const omni_geometry* g, int B, int C, size_t tensor_bytes, hipStream_t stream)
{
    // stages in flight: 1, 2 or 4 (option e2p_nbuf), at most the plane count (the stage loop runs in groups of NB, the remainder singly)
    const int planes = B * C;
    if (planes >= 65536) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers: B * C must be < 65536");
    int nb = omni_options().e2p_nbuf;
    if (nb <= 0) nb = 2;                               // (4 stages in flight measured slower: 41.5 vs 38.3 us at B = 8, 18 x 256^2)
    if (nb >= 4 && planes >= 4) return launch_e2b_nb<T, 4>(a, g, B, C, tensor_bytes, stream);
    if (nb >= 2 && planes >= 2) return launch_e2b_nb<T, 2>(a, g, B, C, tensor_bytes, stream);
    return launch_e2b_nb<T, 1>(a, g, B, C, tensor_bytes, stream);
}

template <typename T>
int launch_e2p(const omni_geometry* g, const void* erp, void* pers, int B, int C, int layout, hipStream_t stream)
{
    constexpr int dtype = sizeof(T) == 2 ? OMNI_F16 : OMNI_F32;
    if (layout == OMNI_LAYOUT_BNCHW) {
        E2PArgs a; fill_args(a, g, erp, pers, B, C);
        const auto& bt = g->e2p_boxes[sizeof(T) == 2 ? 1 : 0];
        const long long tensor_bytes = (long long)B * C * g->H * g->W * (long long)sizeof(T);
        if (bt.ok && !omni_options().e2p_gather && tensor_bytes < (1ll << 31) && (uintptr_t)erp % 16 == 0 && (uintptr_t)pers % 16 == 0)
            return launch_e2b<T>(a, g, B, C, (size_t)tensor_bytes, stream);
        if (sizeof(T) == 4 && !omni_options().e2p_gather && g->W >= 2) return omni_e2p_launch_lds(g, erp, pers, B, C, stream);
        return omni_e2p_launch_planar(g, erp, pers, dtype, B, C, stream);
    } else if (layout == OMNI_LAYOUT_BCHWN) {
        return omni_e2p_launch_ref(g, erp, pers, dtype, B, C, stream);
    } else {
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers: layout must be OMNI_LAYOUT_BCHWN or OMNI_LAYOUT_BNCHW");
    }
}
}  // namespace

extern "C" int omni_equi2pers_g(const omni_geometry_t* g, const void* erp, void* pers, int dtype,
                                int B, int C, int layout, omni_stream_t stream)
{
    if (!g) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: null geometry");
    if (B < 0 || C < 0) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: negative batch/channels");
    if (B == 0 || C == 0) return OMNI_OK;                         // empty input: nothing to do
    if (g->H < 1 || g->W < 1) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: empty ERP image");
    if (!erp || !pers) OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: null device pointer");
    if ((size_t)g->H * g->W >= (1u << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_equi2pers: ERP plane too large");
    if (dtype == OMNI_F32) return launch_e2p<float>(g, erp, pers, B, C, layout, (hipStream_t)stream);
    if (dtype == OMNI_F16) return launch_e2p<__half>(g, erp, pers, B, C, layout, (hipStream_t)stream);
    OMNI_FAIL(OMNI_ERR_INVALID, "omni_equi2pers: dtype must be OMNI_F32 or OMNI_F16");
}

extern "C" int omni_equi2pers(const void* erp, void* pers, int dtype, int B, int C, int H, int W,
                              int ph, int pw, int nrows, float fov_h, float fov_w, int layout,
                              omni_stream_t stream)
{
    const omni_geometry* g = nullptr;
    // the sampler does not need the ERP-side tables; key them by (H,W) anyway so one handle serves both operators
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, H, W, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    return omni_equi2pers_g(g, erp, pers, dtype, B, C, layout, stream);
}

extern "C" int omni_equi2pers_aux(float* xyz, float* uv, int ph, int pw, int nrows, float fov_h, float fov_w,
                                  omni_stream_t stream)
{
    const omni_geometry* g = nullptr;
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, 0, 0, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    if (!xyz && !uv) return OMNI_OK;
    E2PArgs a; fill_args(a, g, nullptr, nullptr, 0, 0);
    const int total = g->N * ph * pw;
    hipLaunchKernelGGL(e2p_aux_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, xyz, uv);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
