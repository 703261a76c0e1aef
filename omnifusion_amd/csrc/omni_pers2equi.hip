// omni_pers2equi.hip — N tangent-plane patches -> one ERP map (gfx950).
//
// Replaces /root/reference/equi_pers/pers2equi_v3.py:16-198:
//   K6  [N,H,W] int64 tap tables + [N,H,W,4] weights, torch.save / torch.load of a 0.5 GB file
//       per call (:29-167)                          -> evaluated in-kernel per (pixel, patch)
//   K7  4 dense advanced-index gathers [B,C,N,H,W] (:174-177) -> gathers over COVERING patches only
//   K8  mask multiply, permutes (:179-187)          -> fused
//   K9  threshold 1e-5, L1-normalise over N*4 (:189-193) -> running sum of weights
//   K10 weighted sum (:194-196)                     -> fused
//   K11 confidence fusion, spherical_model.py:307-311 -> p2e kernel with CONF = true
//
// One thread owns one ERP pixel and all B*C planes of it; a wave owns 64 consecutive pixels
// of one ERP row.  Which patches can cover a 64-pixel tile is a constant of the geometry: a
// 64-bit mask per tile (H * ceil(W/64) words, built once by p2e_candidates_kernel with the SAME
// device function the blend uses, so the mask is an exact superset by construction).  The blend
// loops over the set bits only (wave-uniform scalar loop; mean 2.1 of 18 patches for nrows=4,
// 4.8 of 46 for nrows=6) instead of the reference's dense N.
//
// Per (pixel, patch) arithmetic follows pers2equi_v3.py:112-152 exactly in structure —
// including the quirks that define parity (X scaled by height and compared with
// width, clamped x1/y1 in the weights, strict 0<X<P mask, threshold 1e-5, L1 over all taps) —
// but takes sin/cos of lat_i, lon_j and the centre angles from tables evaluated in double on the
// host:  cos(lon-l0) = cos lon cos l0 + sin lon sin l0  etc.  No transcendental in the kernel.
//
// HBM-bound: algorithmic bytes B*C*(ph*pw*N + H*W)*sizeof(T); tables read: 8 B per tile.
//
// This unit: the C entry points, the launchers and the blend kernels (direct gathers, p2e_lds_kernel, p2e_walk_kernel).  omni_p2e_common.h: argument
// block, tap geometry, table layout | omni_p2e_tables.hip: candidate masks and tile tables | omni_pers2equi_bwd.hip: the backward.
#include "omni_p2e_common.h"

namespace {

// four taps of one plane.  XS1: the patch rows are unit-stride in x (planar layout), so the two
// x-taps of a row come from ONE 8-byte load of (xb, xb+1), xb = min(x0, pw-2); when x0 == pw-1 the
// reference's clamped x1 equals x0 and both taps read element xb+1 (sel = 1).
template <typename T, bool XS1>
__device__ __forceinline__ float p2e_fetch(const T* __restrict__ q, unsigned o0, unsigned o1, unsigned dx, int sel,
                                           const Taps& t)
{
    float va, vb, vc, vd;
    if (XS1) {
        float ax, ay, bx, by;
        Pair<T>::ld(q + o0, ax, ay);
        Pair<T>::ld(q + o1, bx, by);
        va = sel ? ay : ax; vc = ay; vb = sel ? by : bx; vd = by;
    } else {
        va = Store<T>::ld(q + o0); vc = Store<T>::ld(q + o0 + dx);
        vb = Store<T>::ld(q + o1); vd = Store<T>::ld(q + o1 + dx);
    }
    return fmaf(vd, t.wd, fmaf(vc, t.wc, fmaf(vb, t.wb, va * t.wa)));
}

// Blend.  PL = planes accumulated per pass (B*C are walked in chunks of PL).
template <typename T, int PL, bool CONF, bool XS1>
__global__ __launch_bounds__(256) void p2e_kernel(P2EArgs a, int tiles_per_row4, int nblocks)
{
    // block = 4 waves = 4 consecutive rows x 64 columns (vertical neighbours share gather lines in L1)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int r4, tx;
    if (!omni_xcd_rows(blockIdx.x, tiles_per_row4, a.ntx, r4, tx)) return;        // tiles_per_row4 = groups of 4 rows
    const int i = __builtin_amdgcn_readfirstlane(r4 * 4 + wave);                   // wave-uniform row
    const int j = tx * 64 + lane;
    if (i >= a.H) return;
    const bool inside = j < a.W;
    const float2 rt = a.row_trig[i];
    const float2 ct = a.col_trig[inside ? j : a.W - 1];
    const unsigned long long cm_ = a.cand[(size_t)i * a.ntx + tx];
    // keep the candidate mask in SGPRs: the patch loop below is then a scalar loop and the
    // per-patch constants come in through scalar loads from the kernarg segment
    // (readfirstlane returns a signed int: go through unsigned or bit 31 sign-extends into bits 32..63)
    const unsigned cm_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ >> 32));
    const unsigned cm_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(cm_ & 0xffffffffull));
    const unsigned long long cmask = ((unsigned long long)cm_hi << 32) | (unsigned long long)cm_lo;
    const T* pers = (const T*)a.pers;
    const T* pers2 = (const T*)a.pers2;
    const int planes = CONF ? a.B : a.B * a.C;
    const size_t erp_plane = (size_t)a.H * a.W;
    const size_t pix = (size_t)i * a.W + j;
    const unsigned sX = (unsigned)a.sX, sY = (unsigned)a.sY, sN = (unsigned)a.sN;   // < 2^31 (host-checked)

    for (int p0 = 0; p0 < planes; p0 += PL) {
        float acc[PL], acc2[CONF ? PL : 1];
#pragma unroll
        for (int k = 0; k < PL; ++k) acc[k] = 0.0f;
        if (CONF) {
#pragma unroll
            for (int k = 0; k < PL; ++k) acc2[k] = 0.0f;
        }
        float l1 = 0.0f;
        unsigned long long m = cmask;
        // wave-uniform loop over candidate patches, TWO per trip: both patches' tap loads are in flight before the first
        // is consumed (the blend is a chain of dependent memory round trips: candidate mask -> patch constants -> taps)
        while (m) {
            const int n0 = __builtin_ctzll(m);
            m &= m - 1;
            const bool two = m != 0ull;
            const int n1 = two ? __builtin_ctzll(m) : n0;
            if (two) m &= m - 1;
            Taps t[2];
            p2e_taps(a, n0, rt.x, rt.y, ct.x, ct.y, t[0]);
            p2e_taps(a, n1, rt.x, rt.y, ct.x, ct.y, t[1]);
            if (!two) { t[1].wa = 0.0f; t[1].wb = 0.0f; t[1].wc = 0.0f; t[1].wd = 0.0f; }
            unsigned o0[2], o1[2], dx[2]; int sel[2]; bool any[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = u ? n1 : n0;
                const float wsum = (t[u].wa + t[u].wb) + (t[u].wc + t[u].wd);   // all >= 0 after the threshold
                l1 += wsum;
                any[u] = inside && wsum > 0.0f;
                dx[u] = 0; sel[u] = 0;
                if (XS1) {
                    const int xb = min(t[u].x0, a.pw - 2);
                    sel[u] = t[u].x0 - xb;
                    o0[u] = (unsigned)n * sN + (unsigned)t[u].y0 * sY + (unsigned)xb;
                    o1[u] = (unsigned)n * sN + (unsigned)t[u].y1 * sY + (unsigned)xb;
                } else {
                    o0[u] = (unsigned)n * sN + (unsigned)t[u].y0 * sY + (unsigned)t[u].x0 * sX;
                    o1[u] = (unsigned)n * sN + (unsigned)t[u].y1 * sY + (unsigned)t[u].x0 * sX;
                    dx[u] = (unsigned)(t[u].x1 - t[u].x0) * sX;
                }
            }
#pragma unroll
            for (int k = 0; k < PL; ++k) {
                const int p = p0 + k;
                if (p < planes) {
                    const size_t base = CONF ? (size_t)p * (size_t)a.sB
                                             : (size_t)(p / a.C) * (size_t)a.sB + (size_t)(p % a.C) * (size_t)a.sC;
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (any[u]) {
                            acc[k] += p2e_fetch<T, XS1>(pers + base, o0[u], o1[u], dx[u], sel[u], t[u]);
                            if (CONF) acc2[k] += p2e_fetch<T, XS1>(pers2 + base, o0[u], o1[u], dx[u], sel[u], t[u]);
                        }
                }
            }
        }
        if (inside) {
            const float rden = 1.0f / fmaxf(l1, 1e-12f);           // F.normalize(p=1, eps=1e-12), :192
#pragma unroll
            for (int k = 0; k < PL; ++k) {
                const int p = p0 + k;
                if (p < planes) {
                    if (CONF) {
                        const float pr = acc[k] * rden, cf = acc2[k] * rden;
                        const float z = (cf <= 1e-8f) ? 1.0f : 0.0f;                // spherical_model.py:310
                        reinterpret_cast<float*>(a.erp)[(size_t)p * erp_plane + pix] = pr / (cf + 1e-8f * z);   // :311
                    } else {
                        Store<T>::st(reinterpret_cast<T*>(a.erp) + (size_t)p * erp_plane + pix, acc[k] * rden);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ LDS-staged blend (planar layout)
// The gather kernel above is bound by the vector L1 (a 64-lane gather of 8-byte pairs costs ~20 tag look-ups for 0.5 KB of
// useful data, profiles/r01f_resample_pmc.txt), not by HBM.  Here ONE WAVE owns an ERP tile of P2E_TH x P2E_TW pixels (4 per
// lane) and, per covering patch and image plane, streams the bounding box of the tile's bilinear taps inside the patch into
// LDS with 16-byte LDS-DMA pieces (global_load_lds: 64 useful bytes per L1 access, no VGPR staging, no ds_write) and takes the
// taps from LDS.  Boxes are constants of the geometry: a per-tile table (patch, origin, size) is built once per handle by the
// SAME tap function the blend uses (exact superset by construction), so the blend itself has no reduction, no barrier and no
// block-level synchronisation at all — a wave orders its own DMA -> ds_read hand-off with counted `s_waitcnt vmcnt(N)`, and
// keeps `nbuf` boxes in flight (ring of equal slots, sized for the largest box of the geometry).  Arithmetic, summation order
// and therefore every output bit are those of the gather kernel (tests compare the two with torch.equal).
// ONE WAVE (= one 64-thread block) per (ERP tile, group of PL planes); nothing in here synchronises with another wave.  The
// covering patches of the tile are walked one after the other; per patch: (1) the first NB boxes are put in flight, (2) the tap
// geometry of my NPX pixels is evaluated while they travel, (3) the PL stages run.  A stage = (patch, plane p): the box of the
// patch in plane p, NJ = ceil(chunks / 64) DMA pieces of 1 KiB, NB ring slots (stages in flight; PL % NB == 0 so that a stage's
// slot is a compile-time constant).  The stage loop is instantiated per NJ (1..8), which makes every s_waitcnt count and every
// DMA piece loop a compile-time constant: waiting for stage p leaves min(NB-1, PL-1-p) later stages = that many x NJ pieces in
// flight.  The tile is small (4 x 32 pixels, 2 per lane) so that a launch of BASELINE size still has >= 16 waves per CU to
// hide each other's latencies: with one big tile per wave the launch is a handful of long dependent instruction chains per SIMD
// (measured: 8 x 32 tiles, 24 us at B = 8 whatever the ring depth).
// ring of P2E_RING_KB 1-KiB pieces per wave: a stage of `pieces` pieces (NJ, x2 for the fused confidence blend) gets the largest power
// of two <= RING / pieces slots (at most nbmax, at most PL — PL % NB == 0 keeps a stage's slot a compile-time constant), each of
// exactly `pieces` KiB: small boxes (the common case) keep 4 stages in flight, the rare large ones 2 or 1, in one LDS footprint
constexpr int P2E_RING_KB = 10;
constexpr int p2e_slots(int pieces, int nbmax, int pl)
{
    int nb = P2E_RING_KB / pieces >= 4 ? 4 : P2E_RING_KB / pieces >= 2 ? 2 : 1;
    if (nb > nbmax) nb = nbmax;
    while (nb > pl) nb >>= 1;
    return nb;
}

template <typename T, int PL, bool CONF, int NBMAX>
__global__ __launch_bounds__(64, 4) void p2e_lds_kernel(P2EArgs a, const uint2* __restrict__ tiles, int tiles_x, int tiles_y,
                                                        unsigned tensor_bytes, int p_first)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char p2e_smem[];        // the ONLY LDS object of this kernel
    constexpr int EPC = 16 / (int)sizeof(T), M = CONF ? 2 : 1, NPX = P2E_NPX;
    const int lane = threadIdx.x;
    long long tr0 = 0, tr1 = 0;
    if (OMNI_DBG(a, 16)) tr0 = wall_clock64();
    // block -> tile: the ordered table of the geometry (omni_p2e_build_tiles: whole bands of tile rows per XCD, and inside an XCD the
    // tiles dealt so that every CU gets the same amount of work; slot blockIdx.x holds the tile's entries and its id)
    const uint4* __restrict__ sl = reinterpret_cast<const uint4*>(tiles) + (size_t)blockIdx.x * (2 * P2E_REC);
    const uint4 hd = sl[0];
    const int wid = (int)hd.x;
    if (wid < 0) return;                                                            // padding slot (block-uniform)
    const int ti = wid / tiles_x, tj = wid - ti * tiles_x;
    const int col = lane & 31, rsub = lane >> 5;
    const int j = tj * P2E_TW + col;
    const bool jin = j < a.W;
    const int p_begin = p_first + (int)blockIdx.y * PL;
    unsigned char* const ring = p2e_smem;
    const p2e_rsrc_t rs1 = p2e_make_rsrc(a.pers, tensor_bytes);
    const p2e_rsrc_t rs2 = p2e_make_rsrc(CONF ? a.pers2 : a.pers, tensor_bytes);
    const unsigned sYb = (unsigned)a.sY * (unsigned)sizeof(T), sNb = (unsigned)a.sN * (unsigned)sizeof(T);

    // ---- the trig of my pixels (vector loads) and the tile's patch list (wave-uniform address: scalar loads)
    const float2 ct = a.col_trig[jin ? j : a.W - 1];
    float2 rt[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) rt[k] = a.row_trig[min(ti * P2E_TH + rsub + 2 * k, a.H - 1)];
    const int ncand = (int)hd.y;
    uint4 ea = sl[2], eb = sl[3];                                  // record of the first patch
    unsigned poff_l;                                               // lane p: byte offset of plane p_begin + p (< 2^31, host-checked)
    {
        const int p = p_begin + min(lane, PL - 1);
        const unsigned e = CONF ? (unsigned)p * (unsigned)a.sB : (unsigned)(p / a.C) * (unsigned)a.sB + (unsigned)(p % a.C) * (unsigned)a.sC;
        poff_l = e * (unsigned)sizeof(T);
    }
    // all ordinary vector loads are consumed HERE, before the first LDS-DMA is issued (a later first use would make the compiler
    // drain the DMA queue with vmcnt(0))
    asm volatile("" ::"v"(ct.x), "v"(ct.y));
#pragma unroll
    for (int k = 0; k < NPX; ++k) asm volatile("" ::"v"(rt[k].x), "v"(rt[k].y));

    if (OMNI_DBG(a, 16)) tr1 = wall_clock64();
    float acc[PL][NPX], acc2[CONF ? PL : 1][NPX], l1[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        l1[k] = 0.0f;
#pragma unroll
        for (int p = 0; p < PL; ++p) { acc[p][k] = 0.0f; if constexpr (CONF) acc2[p][k] = 0.0f; }
    }

    for (int c = 0; c < ncand; ++c) {
        const uint4 na = sl[2 * (c + 2)], nb4 = sl[2 * (c + 2) + 1];   // the NEXT patch's record travels under this patch's stages
        const unsigned e0 = ea.x, e1 = ea.y;
        const float sl0 = __uint_as_float(ea.z), cl0 = __uint_as_float(ea.w), sp = __uint_as_float(eb.x), cp = __uint_as_float(eb.y);
        const int n = e0 & 63, bw4 = (e0 >> 6) & 1023, xa = e1 & 0xffff, ymin = e1 >> 16;
        const int nchunk = bw4 * (int)((e0 >> 16) & 1023), njj = (nchunk + 63) >> 6;
        const unsigned base = (unsigned)n * sNb + (unsigned)ymin * sYb + (unsigned)xa * (unsigned)sizeof(T);
        unsigned g[P2E_NJMAX];                                      // byte offset of my chunk of piece q, from the box origin
        // ---- (1) fill the ring: stages 0..NB-1
        auto prologue = [&]<int NJ>(std::integral_constant<int, NJ>) {
            constexpr int NB = p2e_slots(NJ * M, NBMAX, PL);
            constexpr unsigned slot_bytes = NJ * M * 1024u;
            const float rbw = __builtin_amdgcn_rcpf((float)bw4);
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                const int qc = q * 64 + lane;
                const int rr = (int)(((float)qc + 0.5f) * rbw);                        // qc / bw4, exact for qc, bw4 <= 1024
                g[q] = qc < nchunk ? (unsigned)rr * sYb + (unsigned)(qc - rr * bw4) * 16u : 0x80000000u;   // past the end: zeros
            }
            if (OMNI_DBG(a, 4)) return;
#pragma unroll
            for (int d = 0; d < NB; ++d) {
                const unsigned so = (unsigned)__builtin_amdgcn_readlane((int)poff_l, d) + base;
                unsigned char* dst = ring + (unsigned)d * slot_bytes;
#pragma unroll
                for (int q = 0; q < NJ; ++q) {
                    p2e_dma16(rs1, dst + q * 1024, g[q], so);
                    if (CONF) p2e_dma16(rs2, dst + NJ * 1024u + q * 1024, g[q], so);
                }
            }
        };
        switch (njj) {
        case 1: prologue(std::integral_constant<int, 1>()); break;
        case 2: prologue(std::integral_constant<int, 2>()); break;
        case 3: prologue(std::integral_constant<int, 3>()); break;
        case 4: prologue(std::integral_constant<int, 4>()); break;
        case 5: prologue(std::integral_constant<int, 5>()); break;
        case 6: prologue(std::integral_constant<int, 6>()); break;
        case 7: prologue(std::integral_constant<int, 7>()); break;
        default: prologue(std::integral_constant<int, 8>()); break;
        }
        // ---- (2) taps of patch n for my pixels, as LDS element offsets inside the box (the DMA latency overlaps this)
        const int pitch = bw4 * EPC;
        int r0[NPX], r1[NPX];
        float wa[NPX], wb[NPX], wc[NPX], wd[NPX];
        const float cd = ct.y * cl0 + ct.x * sl0;                   // p2e_lon with the record's constants (ct = (sin lon, cos lon)): cos(lon - l0)
        const float sd = ct.x * cl0 - ct.y * sl0;                   //                                                          sin(lon - l0)
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            // the pair (x0, x0+1) of both tap rows; at the right patch edge (x1 == x0: wa == wb == 0, see p2e_taps_f) the pair is
            // moved one column left so that its SECOND element is the x1 tap.  Pixels the patch does not cover have all weights 0
            // and read the box origin (p2e_taps_box).
            if (OMNI_DBG(a, 1)) { r0[k] = r1[k] = 1; wa[k] = wb[k] = wc[k] = wd[k] = 0.25f * rt[k].x; l1[k] += rt[k].x; continue; }
            l1[k] += p2e_taps_box(a, sp, cp, rt[k].x, rt[k].y, cd, sd, xa + 1, ymin, pitch, r0[k], r1[k], wa[k], wb[k], wc[k], wd[k]);
        }
        // ---- (3) the PL stages, instantiated on the number of DMA pieces per box
        auto stages = [&]<int NJ>(std::integral_constant<int, NJ>) {
            constexpr int NB = p2e_slots(NJ * M, NBMAX, PL);
            constexpr unsigned slot_bytes = NJ * M * 1024u;
            auto stage = [&]<int P>(std::integral_constant<int, P>) {
                constexpr int SLOT = P % NB;
                constexpr int K1 = (NB - 1 < PL - 1 - P) ? NB - 1 : PL - 1 - P;
                p2e_wait_vm<K1 * NJ * M>();
                const unsigned char* box = ring + (unsigned)SLOT * slot_bytes;
#pragma unroll
                for (int k = 0; k < NPX; ++k) {
                    if (OMNI_DBG(a, 2)) { acc[P][k] += wa[k] * (float)P; continue; }
                    float ax, ay, bx, by;
                    LdsPair<T>::ld(box, r0[k], ax, ay);
                    LdsPair<T>::ld(box, r1[k], bx, by);
                    // taps (y0,x0) (y1,x0) (y0,x1) (y1,x1) in the gather kernel's order of operations
                    acc[P][k] += fmaf(by, wd[k], fmaf(ay, wc[k], fmaf(bx, wb[k], ax * wa[k])));
                    if constexpr (CONF) {
                        const unsigned char* box2 = box + NJ * 1024u;
                        LdsPair<T>::ld(box2, r0[k], ax, ay);
                        LdsPair<T>::ld(box2, r1[k], bx, by);
                        acc2[P][k] += fmaf(by, wd[k], fmaf(ay, wc[k], fmaf(bx, wb[k], ax * wa[k])));
                    }
                }
                if constexpr (P + NB < PL) if (!OMNI_DBG(a, 4)) {   // refill the slot just read (its ds_reads must have returned first)
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    const unsigned so = (unsigned)__builtin_amdgcn_readlane((int)poff_l, P + NB) + base;
                    unsigned char* dst = ring + (unsigned)SLOT * slot_bytes;
#pragma unroll
                    for (int q = 0; q < NJ; ++q) {
                        p2e_dma16(rs1, dst + q * 1024, g[q], so);
                        if (CONF) p2e_dma16(rs2, dst + NJ * 1024u + q * 1024, g[q], so);
                    }
                }
            };
            [&]<int... P>(std::integer_sequence<int, P...>) { (stage(std::integral_constant<int, P>()), ...); }(std::make_integer_sequence<int, PL>());
        };
        switch (njj) {
        case 1: stages(std::integral_constant<int, 1>()); break;
        case 2: stages(std::integral_constant<int, 2>()); break;
        case 3: stages(std::integral_constant<int, 3>()); break;
        case 4: stages(std::integral_constant<int, 4>()); break;
        case 5: stages(std::integral_constant<int, 5>()); break;
        case 6: stages(std::integral_constant<int, 6>()); break;
        case 7: stages(std::integral_constant<int, 7>()); break;
        default: stages(std::integral_constant<int, 8>()); break;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // the ring is a DMA target again for the next patch
        ea = na; eb = nb4;
    }
    // ---- normalise and store (pers2equi_v3.py:192-196; K11: spherical_model.py:310-311)
    const size_t erp_plane = (size_t)a.H * a.W;
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        const int i = ti * P2E_TH + rsub + 2 * k;
        if (!(jin && i < a.H)) continue;
        if (OMNI_DBG(a, 8) && l1[k] != -1.0f) continue;
        const float rden = 1.0f / fmaxf(l1[k], 1e-12f);
        const size_t pix = (size_t)i * a.W + j;
#pragma unroll
        for (int p = 0; p < PL; ++p) {
            const size_t o = (size_t)(p_begin + p) * erp_plane + pix;
            if constexpr (CONF) {
                const float pr = acc[p][k] * rden, cf = acc2[p][k] * rden;
                const float z = (cf <= 1e-8f) ? 1.0f : 0.0f;
                const float r = pr / (cf + 1e-8f * z);
                if (a.store_nt) Store<float>::st_nt(reinterpret_cast<float*>(a.erp) + o, r); else reinterpret_cast<float*>(a.erp)[o] = r;
            } else {
                if (a.store_nt) Store<T>::st_nt(reinterpret_cast<T*>(a.erp) + o, acc[p][k] * rden);
                else Store<T>::st(reinterpret_cast<T*>(a.erp) + o, acc[p][k] * rden);
            }
        }
    }
    if (OMNI_DBG(a, 16)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 && a.trace) {
            long long* t = a.trace + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
            t[0] = tr0; t[1] = tr1; t[2] = wall_clock64();
            t[3] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | ((long long)ncand << 40);
        }
    }
}

// ------------------------------------------------------------------ flat-pipeline blend (round 4: default for the planar layout)
// What bounds p2e_lds_kernel is not bytes but its waves' dependent CHAINS: a launch of BASELINE size has one wave per tile, every wave resident
// at once, and ends with the longest chain — a 4-patch tile, 3.3 us + 2.9 us per patch (profiles/r03b_resample_sweeps.txt, r03_p2e_shed).  Its ISA
// shows why a patch costs 2.9 us: per stage [wait DMA -> 2 ds_read2 -> wait -> 4 fma -> 2 ds_read2 -> wait -> 4 fma -> wait -> refill], i.e. two
// exposed LDS round trips per plane; a drained ring at every patch boundary (the next patch's first boxes wait for its table record, then a full
// memory round trip); and in front of everything two DEPENDENT cold misses (slot record -> tile id -> trig tables).  This kernel keeps the tile,
// the taps, the boxes and every output bit of p2e_lds_kernel and changes the schedule:
//   * ONE stage stream per tile: stage s = (patch s / PL, plane s % PL), NB ring slots, refill distance NB — ACROSS patch boundaries: while the
//     last stages of patch c are consumed, the first stages of patch c+1 are already in flight (its DMA offsets are computed one patch ahead), so
//     the tap geometry of c+1 is evaluated under its own boxes' flight time;
//   * stages are consumed in PAIRS where 4 slots fit the ring (U = 2): one counted wait, all ds_read2 of both planes issued back to back, one LDS
//     wait, both refills, then the 16 fmas — one exposed LDS round trip per two planes instead of four;
//   * the number of 1-KiB pieces per stage is a constant of the TILE (the largest box of its patches; smaller boxes pad with out-of-range lanes,
//     which deposit zeros without touching memory): every s_waitcnt count of the flat stream is a compile-time constant of (NJ, last patch or not);
//   * the slot record carries the tile's trig (32 column + 4 row pairs, 288 B): header, first patch record and trig leave in parallel, ONE cold
//     round trip in front of the first DMA.
constexpr int p2w_nb(int pieces, int pl)
{
    int nb = P2E_RING_KB / pieces >= 4 ? 4 : P2E_RING_KB / pieces >= 2 ? 2 : 1;
    while (nb > pl) nb >>= 1;
    return nb;
}
constexpr int p2w_u(int nb, int pl) { return nb == 4 ? 2 : (nb == 2 && pl == 2) ? 2 : 1; }

// TH: rows of the ERP tile a wave owns (TH / 2 pixels per lane).  8 for ONE plane per wave (round 5): the per-(wave, patch) set-up — records, box
// parameters, the stage switch — is paid half as often (cfg 5 fp32 96 -> 88 us, cfg 3 27.3 -> 26.3, fp16 unchanged: profiles/r05f_p2e_tile8.txt).  Same taps, same candidate order, same blend
// expression per pixel (a patch that does not cover a pixel adds an exact 0): the bits do not depend on the tile.
template <typename T, int PL, bool CONF, int TH = P2E_TH>
__global__ __launch_bounds__(64 * P2W_WPB, TH > P2E_TH ? (CONF ? 4 : 5) : PL == 1 ? (CONF ? 6 : 8) : PL == 2 ? (CONF ? 5 : 6) : 4) void p2e_walk_kernel(P2EArgs a, const unsigned char* __restrict__ table, int tiles_x, unsigned tensor_bytes, int p_first, unsigned ring_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char p2w_smem_all[];    // the ONLY LDS object of this kernel: one ring per wave
    constexpr int EPC = 16 / (int)sizeof(T), M = CONF ? 2 : 1, NPX = TH / 2;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned char* const p2w_smem = p2w_smem_all + (unsigned)wv * ring_bytes;
    const unsigned char* __restrict__ slot = table + ((size_t)blockIdx.x * P2W_WPB + (size_t)wv) * P2W_SLOT;
    const uint4* __restrict__ sl = reinterpret_cast<const uint4*>(slot);            // wave-uniform addresses: scalar loads
    const uint4 hd = sl[0];
    // my pixels' trig: an address that does not depend on the header (issued beside it)
    const int col = lane & 31, rsub = lane >> 5;
    const float2* __restrict__ tg = reinterpret_cast<const float2*>(slot + P2W_OFF_TRIG);
    const float2 ct = tg[col];
    float2 rt[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) rt[k] = tg[P2E_TW + rsub + 2 * k];
    uint4 ea = sl[2], eb = sl[3];                                  // record of the first patch
    const int wid = (int)hd.x;
    if (wid < 0) return;                                           // padding slot (block-uniform)
    if (OMNI_DBG(a, 32)) return;                                   // (debug: the launch floor — blocks that read their header and end)
    const int ncand = (int)hd.y, njt = (int)hd.z;
    const int ti = wid / tiles_x, tj = wid - ti * tiles_x;
    const int j = tj * P2E_TW + col;
    const bool jin = j < a.W;
    const int p_begin = p_first + (int)blockIdx.y * PL;
    unsigned char* const ring = p2w_smem;
    const p2e_rsrc_t rs1 = p2e_make_rsrc(a.pers, tensor_bytes);
    const p2e_rsrc_t rs2 = p2e_make_rsrc(CONF ? a.pers2 : a.pers, tensor_bytes);
    const unsigned sYb = (unsigned)a.sY * (unsigned)sizeof(T), sNb = (unsigned)a.sN * (unsigned)sizeof(T);
    unsigned poff_l;                                               // lane p: byte offset of plane p_begin + p (< 2^31, host-checked)
    {
        const int p = p_begin + min(lane, PL - 1);
        const unsigned e = CONF ? (unsigned)p * (unsigned)a.sB : (unsigned)(p / a.C) * (unsigned)a.sB + (unsigned)(p % a.C) * (unsigned)a.sC;
        poff_l = e * (unsigned)sizeof(T);
    }
    // all ordinary vector loads are consumed HERE, before the first LDS-DMA is issued (a later first use would make the compiler drain the DMA
    // queue with vmcnt(0))
    asm volatile("" ::"v"(ct.x), "v"(ct.y));
#pragma unroll
    for (int k = 0; k < NPX; ++k) asm volatile("" ::"v"(rt[k].x), "v"(rt[k].y));

    float acc[PL][NPX], acc2[CONF ? PL : 1][NPX], l1[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        l1[k] = 0.0f;
#pragma unroll
        for (int p = 0; p < PL; ++p) { acc[p][k] = 0.0f; if constexpr (CONF) acc2[p][k] = 0.0f; }
    }
    // taps of the current patch for my pixels: LDS element offsets inside the box + the four weights (p2e_taps_core: the bits of every kernel)
    int r0[NPX], r1[NPX];
    float wa[NPX], wb[NPX], wc[NPX], wd[NPX];
    auto taps = [&](const uint4& ra, const uint4& rb) {
        const unsigned e0 = ra.x, e1 = ra.y;
        const float sl0 = __uint_as_float(ra.z), cl0 = __uint_as_float(ra.w), sp = __uint_as_float(rb.x), cp = __uint_as_float(rb.y);
        const int bw4 = (e0 >> 6) & 1023, xa = e1 & 0xffff, ymin = e1 >> 16, pitch = bw4 * EPC;
        const float cd = ct.y * cl0 + ct.x * sl0;                   // p2e_lon with the record's constants: cos(lon - l0)
        const float sd = ct.x * cl0 - ct.y * sl0;                   //                                      sin(lon - l0)
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            if (OMNI_DBG(a, 1)) { r0[k] = r1[k] = 1; wa[k] = wb[k] = wc[k] = wd[k] = 0.25f * rt[k].x; l1[k] += rt[k].x; (void)cd; (void)sd; continue; }
            l1[k] += p2e_taps_box(a, sp, cp, rt[k].x, rt[k].y, cd, sd, xa + 1, ymin, pitch, r0[k], r1[k], wa[k], wb[k], wc[k], wd[k]);   // (see p2e_lds_kernel)
        }
    };

    // byte offset of my chunk of piece q from the box origin + the box origin (wave-uniform) of the patch the NEXT refill reads: the current
    // patch for the iterations whose refill stages lie inside it, the following patch from iteration JS on (ONE set of registers: U | NB | PL,
    // so an iteration refills entirely from one patch).  Only the part of the program that depends on NJ — the DMA pieces, the stage loop and its
    // counted waits — is instantiated per NJ (the tap geometry, ~350 instructions, exists twice in the kernel, not twice per NJ: 45 -> ~25 KB of
    // code; the two CUs that share an instruction cache run tiles of every NJ at once).
    unsigned gc[P2W_NJMAX], base_c = 0;
    auto run = [&]<int NJ, int PHASE>(std::integral_constant<int, NJ>, std::integral_constant<int, PHASE>, const uint4& nrec) {
        constexpr int NB = p2w_nb(NJ * M, PL), U = p2w_u(NB, PL), ITERS = PL / U;
        constexpr unsigned slot_bytes = NJ * M * 1024u;
        static_assert(PL % NB == 0 && NB % U == 0, "a stage's ring slot must be a compile-time constant");
        constexpr int JS = (PL - NB) / U;                          // first iteration whose refills belong to the next patch
        auto dma_params = [&](const uint4& ra, unsigned (&g)[P2W_NJMAX], unsigned& base) {
            const unsigned e0 = ra.x, e1 = ra.y;
            const int n = e0 & 63, bw4 = (e0 >> 6) & 1023, xa = e1 & 0xffff, ymin = e1 >> 16;
            const int nchunk = bw4 * (int)((e0 >> 16) & 1023);
            base = (unsigned)n * sNb + (unsigned)ymin * sYb + (unsigned)xa * (unsigned)sizeof(T);
            const float rbw = __builtin_amdgcn_rcpf((float)bw4);
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                const int qc = q * 64 + lane;
                const int rr = (int)(((float)qc + 0.5f) * rbw);                        // qc / bw4, exact for qc, bw4 <= 1024
                g[q] = qc < nchunk ? (unsigned)__umul24((unsigned)rr, sYb) + (unsigned)(qc - __mul24(rr, bw4)) * 16u : 0x80000000u;   // past the end (of THIS patch's box): zeros  (row pitch < 2^24 bytes: host-checked)
            }
        };
        auto issue = [&](const unsigned (&g)[P2W_NJMAX], unsigned base, int plane, int slot_i) {
            if (OMNI_DBG(a, 4)) return;
            const unsigned so = (unsigned)__builtin_amdgcn_readlane((int)poff_l, plane) + base;
            unsigned char* dst = ring + (unsigned)slot_i * slot_bytes;
#pragma unroll
            for (int q = 0; q < NJ; ++q) {
                p2e_dma16(rs1, dst + q * 1024, g[q], so);
                if (CONF) p2e_dma16(rs2, dst + NJ * 1024u + q * 1024, g[q], so);
            }
        };
        // one patch of the stream: ITERS iterations of U stages.  LAST: no patch follows (nothing to refill from beyond plane PL - 1).
        auto body = [&]<bool LAST>(std::bool_constant<LAST>, const uint4& nrec) {
            [&]<int... J>(std::integer_sequence<int, J...>) {
                (([&] {
                    constexpr int first = J * U;
                    if constexpr (!LAST && J == JS) dma_params(nrec, gc, base_c);     // from here on the refills read the next patch
                    // stages younger than the ones consumed here and already in flight: first + U .. first + NB - 1 of the flat stream
                    constexpr int ahead = NB - U;
                    constexpr int left = PL - first - U;            // ... of which this many belong to THIS patch
                    constexpr int younger = LAST ? (left < ahead ? (left > 0 ? left : 0) : ahead) : ahead;
                    p2e_wait_vm<younger * NJ * M>();
                    float v[U][M][NPX][4];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const unsigned char* box = ring + (unsigned)((first + u) % NB) * slot_bytes;
#pragma unroll
                        for (int m = 0; m < M; ++m)
#pragma unroll
                            for (int k = 0; k < NPX; ++k) {
                                if (OMNI_DBG(a, 2)) { v[u][m][k][0] = v[u][m][k][1] = v[u][m][k][2] = v[u][m][k][3] = wa[k]; continue; }
                                LdsPair<T>::ld(box + m * NJ * 1024u, r0[k], v[u][m][k][0], v[u][m][k][1]);
                                LdsPair<T>::ld(box + m * NJ * 1024u, r1[k], v[u][m][k][2], v[u][m][k][3]);
                            }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every read of these slots has returned: they are DMA targets again
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int t = first + u + NB;
                        if (t < PL) issue(gc, base_c, t, (first + u) % NB);
                        else if (!LAST) issue(gc, base_c, t - PL, (first + u) % NB);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int k = 0; k < NPX; ++k) {
                            // taps (y0,x0) (y1,x0) (y0,x1) (y1,x1) in the gather kernel's order of operations
                            acc[first + u][k] += fmaf(v[u][0][k][3], wd[k], fmaf(v[u][0][k][1], wc[k], fmaf(v[u][0][k][2], wb[k], v[u][0][k][0] * wa[k])));
                            if constexpr (CONF)
                                acc2[first + u][k] += fmaf(v[u][1][k][3], wd[k], fmaf(v[u][1][k][1], wc[k], fmaf(v[u][1][k][2], wb[k], v[u][1][k][0] * wa[k])));
                            // the blend happens HERE (volatile statements keep their order): left to itself the scheduler defers the fmas of every
                            // iteration to the end of the patch and keeps all their operands alive — 64 registers, scratch spills
                            asm volatile("" : "+v"(acc[first + u][k]));
                            if constexpr (CONF) asm volatile("" : "+v"(acc2[first + u][k]));
                        }
                }()), ...);
            }(std::make_integer_sequence<int, ITERS>());
        };
        if constexpr (PHASE == 0) {                               // head of the stream: the first NB stages of patch 0 go out
            dma_params(nrec, gc, base_c);
#pragma unroll
            for (int d = 0; d < NB; ++d) issue(gc, base_c, d, d);
        } else if constexpr (PHASE == 1) body(std::bool_constant<false>(), nrec);
        else body(std::bool_constant<true>(), nrec);
    };
    // (boxes of up to P2W_NJMAX KiB: every BASELINE shape is 1-3; a geometry with larger boxes — patches much finer than the ERP — stays on p2e_lds_kernel)
    auto with_nj = [&]<int PHASE>(std::integral_constant<int, PHASE> ph, const uint4& nrec) {
        switch (njt) {
        case 1: run(std::integral_constant<int, 1>(), ph, nrec); break;
        case 2: run(std::integral_constant<int, 2>(), ph, nrec); break;
        case 3: run(std::integral_constant<int, 3>(), ph, nrec); break;
        case 4: run(std::integral_constant<int, 4>(), ph, nrec); break;
        case 5: run(std::integral_constant<int, 5>(), ph, nrec); break;
        default: run(std::integral_constant<int, P2W_NJMAX>(), ph, nrec); break;
        }
    };
    with_nj(std::integral_constant<int, 0>(), ea);
    taps(ea, eb);                                                  // ... evaluated while the first boxes travel
    for (int c = 0; c < ncand; ++c) {
        const uint4 na = sl[2 * (c + 2)], nb4 = sl[2 * (c + 2) + 1];        // record of patch c + 1 (a zero record past the list)
        if (c + 1 < ncand) {
            with_nj(std::integral_constant<int, 1>(), na);
            taps(na, nb4);                                          // ... under the flight time of its own first boxes
        } else {
            with_nj(std::integral_constant<int, 2>(), na);
        }
    }
    // ---- normalise and store (pers2equi_v3.py:192-196; K11: spherical_model.py:310-311)
    const size_t erp_plane = (size_t)a.H * a.W;
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
        const int i = ti * TH + rsub + 2 * k;
        if (!(jin && i < a.H)) continue;
        if (OMNI_DBG(a, 8) && l1[k] != -1.0f) continue;
        const float rden = 1.0f / fmaxf(l1[k], 1e-12f);
        const size_t pix = (size_t)i * a.W + j;
#pragma unroll
        for (int p = 0; p < PL; ++p) {
            const size_t o = (size_t)(p_begin + p) * erp_plane + pix;
            if constexpr (CONF) {
                const float pr = acc[p][k] * rden, cf = acc2[p][k] * rden;
                const float z = (cf <= 1e-8f) ? 1.0f : 0.0f;
                const float r = pr / (cf + 1e-8f * z);
                if (a.store_nt) Store<float>::st_nt(reinterpret_cast<float*>(a.erp) + o, r); else reinterpret_cast<float*>(a.erp)[o] = r;
            } else {
                if (a.store_nt) Store<T>::st_nt(reinterpret_cast<T*>(a.erp) + o, acc[p][k] * rden);
                else Store<T>::st(reinterpret_cast<T*>(a.erp) + o, acc[p][k] * rden);
            }
        }
    }
}

// ------------------------------------------------------------------ (round 5: ONE plane per wave with D = 2 / 3 patches in flight, measured and dropped)
// p2e_walk1_kernel kept the boxes of D consecutive patches of a single-plane tile in flight (the flat pipeline above holds ONE stage when a stage is a
// whole patch).  Same bits; BASELINE cfg 5 fp16 108.8 / 115.3 / 106.2 us and cfg 3 27.1 / 27.5 / 29.9 us for D = 1 / 2 / 3, same box
// (profiles/r05c_p2e_single_plane.txt): the one-plane blend is not waiting for its boxes.  Neither is it short of issue slots: 24 % fewer VALU
// instructions in the tap section (p2e_taps_box: validity on two factors, 24-bit index arithmetic — kept) changed nothing either.  With parts switched
// off (debug build): no tap geometry -47 us, no LDS reads -14, no DMA -1.5, no stores -6, everything off 54 us of 113: half of the kernel is the per-(wave,
// patch) skeleton — records, box parameters, the stage switch.  MORE PIXELS PER WAVE (8-row tiles, TH = 8 above: half as many (wave, patch) pairs) bought
// 8 % at fp32 (96 -> 88 us), 3 % at BASELINE cfg 3 and nothing at fp16: with 4.8 covering patches per ERP pixel at nrows 6 (2.1 at nrows 4; the oracle's cover count) the kernel is bound by the
// instructions it spends per (pixel, patch), which no tile shape changes.
// ------------------------------------------------------------------ (round 3: a plane-major form of this kernel, measured and dropped)
// p2e_tile_kernel swapped the loops: set-up once per tile (all table entries and patch constants in one batch of scalar loads, the taps of
// EVERY covering patch in registers, 6 per pixel and patch), then ONE pipeline of PL stages per tile, a stage = the boxes of all covering
// patches of one plane packed back to back into one ring slot (13.3 instead of 16.5 MB of LDS-DMA per plane at cfg 1), the blend of a pixel
// a loop over patches inside the stage.  Same bits.  B = 8, 18 x 256^2: 19.3 us against 18.4 us for the patch-by-patch kernel above (17.2 vs
// 15.9 with the balanced block order), 46.9 vs 33.3 us at nrows = 6: its per-block phases (tools/trace_resample.py) were loads 1.3 us, DMA
// addresses + ring fill 1.4, taps 1.4, the 8 stages 4.8, stores 0.8 for a 2-patch tile and still grew by 2.5 us per patch — a block's time is
// the WORK per patch (bytes, taps, geometry) divided by a throughput 16 waves per CU share, not the number of dependent pipelines.
// What the same traces did show: the CU on a patch seam had 56 patch-tiles to the median CU's 34 — see the block order in omni_p2e_build_tiles (omni_p2e_tables.hip).

template <typename T, bool CONF, bool XS1>
void launch_p2e_pl(const P2EArgs& a, int planes, int rows4, int nblocks, hipStream_t stream)
{
    if (planes <= 1)      hipLaunchKernelGGL((p2e_kernel<T, 1, CONF, XS1>), dim3(nblocks), dim3(256), 0, stream, a, rows4, nblocks);
    else if (planes <= 2) hipLaunchKernelGGL((p2e_kernel<T, 2, CONF, XS1>), dim3(nblocks), dim3(256), 0, stream, a, rows4, nblocks);
    else if (planes <= 4) hipLaunchKernelGGL((p2e_kernel<T, 4, CONF, XS1>), dim3(nblocks), dim3(256), 0, stream, a, rows4, nblocks);
    else                  hipLaunchKernelGGL((p2e_kernel<T, 8, CONF, XS1>), dim3(nblocks), dim3(256), 0, stream, a, rows4, nblocks);
}

// ---- LDS path: launch geometry.  One wave per (tile, group of PL planes); LDS per wave = the ring (or the largest stage of the
// geometry if that is larger); option "p2e_nbuf" caps the stages in flight (tuning).
template <typename T, int PL, bool CONF, int NBMAX>
int launch_p2e_lds_nb(const P2EArgs& a, const omni_geometry* g, int p_first, int planes, size_t tensor_bytes, hipStream_t stream)
{
    const auto& tt = g->p2e_tiles[sizeof(T) == 2 ? 1 : 0];
    const int stage_kb = (tt.max_chunks + 63) / 64 * (CONF ? 2 : 1);
    const size_t lds = std::max((size_t)(stage_kb > P2E_RING_KB ? stage_kb : P2E_RING_KB), (size_t)std::max(0, omni_options().p2e_lds_kb)) * 1024;
    hipLaunchKernelGGL((p2e_lds_kernel<T, PL, CONF, NBMAX>), dim3(tt.nslots, planes / PL), dim3(64), lds, stream, a,
                       (const uint2*)tt.ord, g->p2e_tx, g->p2e_ty, (unsigned)tensor_bytes, p_first);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

template <typename T, int PL, bool CONF>
int launch_p2e_walk_pl(const P2EArgs& a, const omni_geometry* g, int p_first, int planes, size_t tensor_bytes, hipStream_t stream)
{
    if constexpr (PL == 1) {
        // ONE plane per wave: the 8-row tile set where the geometry has one whose boxes fit (option p2e_tile8: 1 (default) | 0: 4-row tiles)
        const auto& t8 = g->p2e_tiles[2 + (sizeof(T) == 2 ? 1 : 0)];
        if (omni_options().p2e_tile8 && t8.walk && t8.max_chunks <= 64 * P2W_NJMAX && P2W_WPB == 1) {
            const size_t lds8 = (size_t)((t8.max_chunks + 63) / 64 * (CONF ? 2 : 1)) * 1024;
            hipLaunchKernelGGL((p2e_walk_kernel<T, 1, CONF, 8>), dim3(t8.nslots_walk, planes), dim3(64), lds8, stream, a,
                               (const unsigned char*)t8.walk, g->p2e_tx, (unsigned)tensor_bytes, p_first, (unsigned)lds8);
            OMNI_HIP(hipGetLastError());
            return OMNI_OK;
        }
    }
    const auto& tt = g->p2e_tiles[sizeof(T) == 2 ? 1 : 0];
    const int stage_kb = (tt.max_chunks + 63) / 64 * (CONF ? 2 : 1);
    // (ONE plane per wave keeps one stage in flight whatever the ring: its LDS is the largest stage of the geometry, 1-2 KiB — up to 32 waves per CU)
    const size_t lds = (size_t)(PL == 1 ? stage_kb : (stage_kb > P2E_RING_KB ? stage_kb : P2E_RING_KB)) * 1024;
    static_assert(256 % P2W_WPB == 0, "nslots is a multiple of 256");
    hipLaunchKernelGGL((p2e_walk_kernel<T, PL, CONF>), dim3(tt.nslots_walk / P2W_WPB, planes / PL), dim3(64 * P2W_WPB), lds * P2W_WPB, stream, a,
                       (const unsigned char*)tt.walk, g->p2e_tx, (unsigned)tensor_bytes, p_first, (unsigned)lds);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

// the forms of the walk kernel that fit 128 registers WITHOUT scratch (a scratch access inside the counted DMA pipeline would shift every
// s_waitcnt; omnifusion_amd/isa.py fails the build otherwise): 2-byte elements need extra registers for the byte-aligns of their tap pairs
template <typename T, int PL, bool CONF> constexpr bool p2w_fits() { return true; }

template <typename T, int PL, bool CONF>
int launch_p2e_lds_pl(const P2EArgs& a, const omni_geometry* g, int p_first, int planes, size_t tensor_bytes, hipStream_t stream)
{
    // option p2e_walk: 1 (default) the flat-pipeline kernel for waves of ONE or TWO planes — a lone panorama's depth map, BASELINE cfg 3 / cfg 5: 30.9 ->
    // 25.7 us, 110 -> 100 us (fp16), 105 -> 88 us — where its small LDS footprint (one stage) admits 24-32 waves per CU; with 4 / 8 planes per wave the
    // two kernels measure equal at 8 panoramas and p2e_lds_kernel 3 % ahead at 16 (profiles/r04_p2e_walk.txt) | 2: always | 0: never
    if constexpr (p2w_fits<T, PL, CONF>())
    if ((omni_options().p2e_walk == 2 || (omni_options().p2e_walk == 1 && PL <= 2)) && g->p2e_tiles[sizeof(T) == 2 ? 1 : 0].walk && g->p2e_tiles[sizeof(T) == 2 ? 1 : 0].max_chunks <= 64 * P2W_NJMAX &&
        (unsigned long long)a.sY * sizeof(T) < (1ull << 24))          // (its DMA offsets use the full-rate 24-bit multiply on the row pitch)
        return launch_p2e_walk_pl<T, PL, CONF>(a, g, p_first, planes, tensor_bytes, stream);
    int nb = omni_options().p2e_nbuf;
    if (nb <= 0) nb = 2;   // measured: 2 stages x 16 waves/CU beat 4 stages (18.4 vs 19.3 us at B=8 18x256^2)
    if (nb >= 4) return launch_p2e_lds_nb<T, PL, CONF, 4>(a, g, p_first, planes, tensor_bytes, stream);
    if (nb >= 2) return launch_p2e_lds_nb<T, PL, CONF, 2>(a, g, p_first, planes, tensor_bytes, stream);
    return launch_p2e_lds_nb<T, PL, CONF, 1>(a, g, p_first, planes, tensor_bytes, stream);
}

template <typename T, bool CONF>
int launch_p2e_lds(const P2EArgs& a, const omni_geometry* g, int planes, size_t tensor_bytes, hipStream_t stream)
{
    // planes per wave: 8, 4, 2 or 1 (the tap geometry is evaluated once per wave and patch and amortised over them); the groups go to
    // blockIdx.y.  A plane count that is not a multiple of 8 runs as up to four launches over consecutive plane ranges (7 = 4 + 2 + 1)
    // instead of falling to one plane per wave, where the geometry is as much work as the blend.
    // (CONF, 8 planes: 2 x 16 accumulators spill at 128 VGPRs, and a scratch access inside the DMA pipeline would shift every hand-counted
    //  s_waitcnt vmcnt(N) — that form is not instantiated at all; omnifusion_amd/isa.py checks that no counted-wait kernel has scratch)
    constexpr int CAPMAX = CONF ? 4 : 8;
    const int cap = std::min(CAPMAX, omni_options().p2e_planes > 0 ? omni_options().p2e_planes : CAPMAX);
    int p = 0;
    while (p < planes) {
        const int left = planes - p;
        int rc = OMNI_OK;
        if (left >= 8 && cap >= 8)      { const int n = left / 8 * 8; if constexpr (!CONF) rc = launch_p2e_lds_pl<T, 8, CONF>(a, g, p, n, tensor_bytes, stream); p += n; }
        else if (left >= 4 && cap >= 4) { const int n = left / 4 * 4; rc = launch_p2e_lds_pl<T, 4, CONF>(a, g, p, n, tensor_bytes, stream); p += n; }
        else if (left >= 2 && cap >= 2) { const int n = left / 2 * 2; rc = launch_p2e_lds_pl<T, 2, CONF>(a, g, p, n, tensor_bytes, stream); p += n; }
        else                            { rc = launch_p2e_lds_pl<T, 1, CONF>(a, g, p, left, tensor_bytes, stream); p += left; }
        if (rc != OMNI_OK) return rc;
    }
    return OMNI_OK;
}

template <typename T, bool CONF>
int launch_p2e(const omni_geometry* g, const void* pers, const void* pers2, void* erp, int B, int C,
               int layout, hipStream_t stream)
{
    P2EArgs a;
    int rc = fill_args(a, g, pers, pers2, erp, B, C, layout);
    if (rc != OMNI_OK) return rc;
    if ((long long)g->N * C * g->ph * g->pw >= (1ll << 31))
        OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_pers2equi: one batch item of the patch tensor must hold < 2^31 elements");
    const int planes = CONF ? B : B * C;
    // LDS-staged path: planar patches whose rows are whole 16-byte chunks, boxes that fit a slot, 32-bit element offsets
    const auto& tt = g->p2e_tiles[sizeof(T) == 2 ? 1 : 0];
    constexpr int EPC = 16 / (int)sizeof(T);
    const bool aligned = ((uintptr_t)pers % 16 == 0) && (!pers2 || (uintptr_t)pers2 % 16 == 0) &&
                         g->pw % EPC == 0 && (g->ph * g->pw) % EPC == 0;
    const long long tensor_bytes = (long long)B * g->N * C * g->ph * g->pw * (long long)sizeof(T);
    // (ONE plane — a lone panorama's depth map, BASELINE cfg 3 / cfg 5 — has nothing to amortise the boxes over: the launch is bound by the tap
    //  geometry of its (pixel, patch) pairs, ~100 vector instructions each, and the direct gathers are the shorter program: cfg 3 31.2 vs 33.6 us,
    //  cfg 5 fp16 108 vs 123 us; at 512x1024 the two are equal)
    // (round 4: with the flat-pipeline kernel the LDS path wins for one plane too; the gathers remain for option p2e_walk = 0)
    const bool single = planes == 1 && (long long)g->H * g->W >= (1ll << 20) && omni_options().p2e_gather != 2 &&
                        !(omni_options().p2e_walk && tt.walk && tt.max_chunks <= 64 * P2W_NJMAX);
    if (a.sX == 1 && tt.ok && aligned && omni_options().p2e_gather != 1 && !single && tensor_bytes < (1ll << 31))   // 32-bit buffer offsets
        return launch_p2e_lds<T, CONF>(a, g, planes, (size_t)tensor_bytes, stream);
    const int rows4 = (g->H + 3) / 4;
    const int nblocks = omni_xcd_rows_grid(rows4, g->ntx);
    if (a.sX == 1 && g->pw >= 2) launch_p2e_pl<T, CONF, true>(a, planes, rows4, nblocks, stream);
    else                         launch_p2e_pl<T, CONF, false>(a, planes, rows4, nblocks, stream);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
}  // namespace

// ------------------------------------------------------------------ reference layout -> planar
// [B,C,ph,pw,N] (N innermost: the reference's stack(dim=-1) / unfold layout) -> [B,N,C,ph,pw].  A blend over the N-innermost tensor
// touches every cache line of a patch region once per covering patch (18 patches share each line): 94.6 us for 8 x 18 x 256^2 where the
// LDS-staged kernel on planar patches takes 18.5.  Converting first costs one coalesced pass (256 pixels x N elements per block in,
// N runs of 256 elements out, transposed in LDS with an odd pitch): the drop-in pers2equi() runs both.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void patches_to_planar_kernel(const T* __restrict__ src, T* __restrict__ dst, int C, int N, int pp, int tiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char p2p_raw[];
    T* tile = reinterpret_cast<T*>(p2p_raw);                     // [256][N + 1]
    const int bc = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * 256;
    const int b = bc / C, c = bc % C;
    const int npx = min(256, pp - p0), run = npx * N, pitch = N + 1;
    const T* s = src + ((size_t)bc * pp + p0) * N;
    for (int i = threadIdx.x; i < run; i += 256) tile[(i / N) * pitch + i % N] = s[i];
    __syncthreads();
    if ((int)threadIdx.x < npx)
        for (int n = 0; n < N; ++n)
            dst[(((size_t)b * N + n) * C + c) * pp + p0 + threadIdx.x] = tile[threadIdx.x * pitch + n];
}
}  // namespace

extern "C" int omni_patches_to_planar(const void* src, void* dst, int dtype, int B, int C, int ph, int pw, int N, omni_stream_t stream)
{
    if (B < 0 || C < 0 || ph <= 0 || pw <= 0 || N <= 0 || N > 64) OMNI_FAIL(OMNI_ERR_INVALID, "omni_patches_to_planar: bad shape (1..64 patches)");
    if (B == 0 || C == 0) return OMNI_OK;
    if (!src || !dst) OMNI_FAIL(OMNI_ERR_INVALID, "omni_patches_to_planar: null device pointer");
    const int pp = ph * pw, tiles = (pp + 255) / 256;
    if ((long long)B * C * tiles >= (1ll << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, "omni_patches_to_planar: too many tiles");
    const dim3 grid((unsigned)(B * C * tiles));
    if (dtype == OMNI_F32)      hipLaunchKernelGGL(patches_to_planar_kernel<float>, grid, dim3(256), 256 * (N + 1) * 4, (hipStream_t)stream, (const float*)src, (float*)dst, C, N, pp, tiles);
    else if (dtype == OMNI_F16) hipLaunchKernelGGL(patches_to_planar_kernel<__half>, grid, dim3(256), 256 * (N + 1) * 2, (hipStream_t)stream, (const __half*)src, (__half*)dst, C, N, pp, tiles);
    else OMNI_FAIL(OMNI_ERR_INVALID, "omni_patches_to_planar: dtype must be OMNI_F32 or OMNI_F16");
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_pers2equi_g(const omni_geometry_t* g, const void* pers, void* erp, int dtype, int B, int C,
                                int layout, omni_stream_t stream)
{
    int rc = check_common(g, B, C, "omni_pers2equi");
    if (rc != OMNI_OK) return rc;
    if (B == 0 || C == 0) return OMNI_OK;
    if (!pers || !erp) OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi: null device pointer");
    if (dtype == OMNI_F32) return launch_p2e<float, false>(g, pers, nullptr, erp, B, C, layout, (hipStream_t)stream);
    if (dtype == OMNI_F16) return launch_p2e<__half, false>(g, pers, nullptr, erp, B, C, layout, (hipStream_t)stream);
    OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi: dtype must be OMNI_F32 or OMNI_F16");
}

extern "C" int omni_pers2equi(const void* pers, void* erp, int dtype, int B, int C, int ph, int pw,
                              int H, int W, int nrows, float fov_h, float fov_w, int layout,
                              omni_stream_t stream)
{
    const omni_geometry* g = nullptr;
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, H, W, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    return omni_pers2equi_g(g, pers, erp, dtype, B, C, layout, stream);
}

extern "C" int omni_pers2equi_conf(const void* pred_w, const void* conf, float* out, int dtype, int B,
                                   int ph, int pw, int H, int W, int nrows, float fov_h, float fov_w,
                                   int layout, omni_stream_t stream)
{
    const omni_geometry* g = nullptr;
    int rc = omni_geometry_lookup(&g, nrows, fov_h, fov_w, ph, pw, H, W, (hipStream_t)stream);
    if (rc != OMNI_OK) return rc;
    rc = check_common(g, B, 1, "omni_pers2equi_conf");
    if (rc != OMNI_OK) return rc;
    if (B == 0) return OMNI_OK;
    if (!pred_w || !conf || !out) OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi_conf: null device pointer");
    if (dtype == OMNI_F32) return launch_p2e<float, true>(g, pred_w, conf, out, B, 1, layout, (hipStream_t)stream);
    if (dtype == OMNI_F16) return launch_p2e<__half, true>(g, pred_w, conf, out, B, 1, layout, (hipStream_t)stream);
    OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi_conf: dtype must be OMNI_F32 or OMNI_F16");
}
