// omni_p2e_common.h — what the pers2equi units share (omni_pers2equi.hip: entry points, launchers and the blend kernels; omni_p2e_tables.hip: the
// per-geometry candidate masks and tile tables; omni_pers2equi_bwd.hip: the backward).  Device side: the argument block, the tap geometry (forceinline:
// candidate masks, tile boxes, blends and the backward all evaluate the SAME functions, same bits), the pair loaders, the LDS-DMA primitives and the layout
// constants of the tile / slot tables, which their builder and the kernels that read them must agree on.  Host side: fill_args and check_common.
// No kernel in here: every __global__ lives in exactly one .hip.
#pragma once
#include <stdio.h>
#include <string.h>
#include <utility>
#include <vector>
#include <algorithm>
#include "omni_internal.h"

namespace {

struct P2EArgs {
    const void* pers; const void* pers2;      // pers2: confidence tensor for the fused K11 blend
    void* erp;
    const float2* row_trig; const float2* col_trig;
    const unsigned long long* cand;
    int B, C, H, W, ph, pw, ntx;
    long long sB, sC, sN, sY, sX;              // element strides of the patch tensor
    float kx, ky;                              // 1/(FOVx*PI), 1/(FOVy*PI_2)   (:115-116)
    float half_h, half_w;                      // 0.5*height, 0.5*width        (:122-123)
    int store_nt;                              // 1: non-temporal ERP stores (option p2e_store)
    int dbg;                                   // debug build only (OMNI_P2E_DBG ablation bits): 1 no tap geometry, 2 no LDS tap reads, 4 no DMA, 8 no stores
    long long* trace;                          // debug build, bit 16: per-block time stamps (omni_debug_set_trace)
    PatchTab tab;
};

struct Taps { int x0, x1, y0, y1; float wa, wb, wc, wd; };

// pers2equi_v3.py:112-152 + :191 for one (pixel, patch).  Returns the validity mask.
// Split in two so that the pixels of one ERP column (same lon) share cos/sin(lon - l0); every kernel (candidate masks, tile
// boxes, gather blend, LDS blend) goes through these SAME two functions, so all of them see the same bits.
__device__ __forceinline__ void p2e_lon(const P2EArgs& a, int n, float slon, float clon, float& cd, float& sd)
{
    const float sl0 = a.tab.slam[n], cl0 = a.tab.clam[n];
    cd = clon * cl0 + slon * sl0;                                   // cos(lon - l0)
    sd = slon * cl0 - clon * sl0;                                   // sin(lon - l0)
}
// the float part of the taps (everything but the integer conversions): the four weights and the tap coordinates as floats
struct TapsF { float x0f, x1f, y0f, y1f; float wa, wb, wc, wd; };
__device__ __forceinline__ bool p2e_taps_f(const P2EArgs& a, float sp, float cp, float slat, float clat, float cd, float sd, TapsF& t)
{
    const float cos_c = sp * slat + cp * clat * cd;                 // :112
    // :113-114 divide twice by cos_c; one reciprocal and two products differ from that by <= 2 ulp of X, Y (a
    // validity / floor predicate can flip only where the reference's own coordinate is within round-off of the step)
    float rc = __builtin_amdgcn_rcpf(cos_c);                       // 1 ulp ...
    rc = fmaf(fmaf(-cos_c, rc, 1.0f), rc, rc);                      // ... + one Newton step: ~0.5 ulp (an IEEE division costs 11 instructions)
    float nx = (clat * sd) * rc;                                    // :113
    float ny = (cp * slat - sp * clat * cd) * rc;                   // :114
    nx = nx * a.kx;                                                 // :115
    ny = ny * a.ky;                                                 // :116
    const float X = (nx + 1.0f) * a.half_h;                         // :122 (sic)
    const float Y = (ny + 1.0f) * a.half_w;                         // :123 (sic)
    const float fw = (float)a.pw, fh = (float)a.ph;
    const bool valid = (X < fw) && (X > 0.0f) && (Y < fh) && (Y > 0.0f) && (cos_c > 0.0f);   // :118,126-127
    const float fx = floorf(X), fy = floorf(Y);                     // :129-132
    // :134-137 clamp x0, x1, y0, y1 to [0, P-1].  A VALID pixel has 0 < X < P, so floor(X) is already in range and only the +1
    // taps can leave it (at the far edge); for an invalid pixel every weight is zeroed below and no kernel uses its indices.
    const float x0f = fx, x1f = fminf(fx + 1.0f, fw - 1.0f);
    const float y0f = fy, y1f = fminf(fy + 1.0f, fh - 1.0f);
    // :144-147 multiply by mask: the mask goes onto the two x factors (two selects instead of four; for a valid pixel the products are the
    // reference's, for an invalid one they are 0, -0 or — where Y is not finite — NaN, and the threshold below turns all three into 0)
    const float hx1 = valid ? x1f - X : 0.0f, hx0 = valid ? X - x0f : 0.0f;
    const float wa = hx1 * (y1f - Y);                               // :139  tap (y0,x0)
    const float wb = hx1 * (Y - y0f);                               // :140  tap (y1,x0)
    const float wc = hx0 * (y1f - Y);                               // :141  tap (y0,x1)
    const float wd = hx0 * (Y - y0f);                               // :142  tap (y1,x1)
    // :191 zero everything <= 1e-5 (a NaN compares false)
    t.wa = wa > 1e-5f ? wa : 0.0f;
    t.wb = wb > 1e-5f ? wb : 0.0f;
    t.wc = wc > 1e-5f ? wc : 0.0f;
    t.wd = wd > 1e-5f ? wd : 0.0f;
    // Right patch edge (x1 == x0 == pw-1, X in [pw-1, pw)): the x0 taps carry the factor (x1 - X) <= 0, so wa and wb are already
    // exactly 0 — except in the corner cell, where y is clamped too and wa = (x1-X)(y1-Y) > 0.  There all four taps are the same
    // pixel; its weight is moved to the (y1, x1) tap (v*wa + v*wd -> v*(wa + wd): one rounding), so that EVERY kernel may assume
    // "x1 == x0  =>  wa == wb == 0" and read the tap pair one column to the left without a select.
    const bool xedge = x1f == x0f;
    t.wd = xedge ? t.wd + t.wa : t.wd;
    t.wa = xedge ? 0.0f : t.wa;
    t.x0f = x0f; t.x1f = x1f; t.y0f = y0f; t.y1f = y1f;
    return valid;
}
__device__ __forceinline__ bool p2e_taps_core(const P2EArgs& a, float sp, float cp, float slat, float clat, float cd, float sd, Taps& t)
{
    TapsF f;
    const bool valid = p2e_taps_f(a, sp, cp, slat, clat, cd, sd, f);
    t.wa = f.wa; t.wb = f.wb; t.wc = f.wc; t.wd = f.wd;
    t.x0 = (int)f.x0f; t.x1 = (int)f.x1f; t.y0 = (int)f.y0f; t.y1 = (int)f.y1f;
    return valid;
}
// The taps as the LDS kernels use them: element offsets of the two tap ROW pairs inside a box whose origin is (xa, ymin) and whose rows are `pitch`
// elements apart — the pair (x1 - 1, x1) of rows y0 and y1 (at the right patch edge, x1 == x0, wa == wb == 0 and the pair's second element is the x1
// tap: no select) — and the weights; a pixel the patch does not cover (all weights 0) reads the box origin.  Returns the weight sum.
// (xo = x0 - (xa + 1 - (x1 - x0)) = x1 - xa - 1; y1 - y0 is 0 or 1: one 24-bit multiply-add and one select instead of two 32-bit multiplies.)
__device__ __forceinline__ float p2e_taps_box(const P2EArgs& a, float sp, float cp, float slat, float clat, float cd, float sd, int xa1, int ymin, int pitch,
                                              int& r0, int& r1, float& wa, float& wb, float& wc, float& wd)
{
    TapsF f;
    p2e_taps_f(a, sp, cp, slat, clat, cd, sd, f);
    const float wsum = (f.wa + f.wb) + (f.wc + f.wd);               // all >= 0 after the threshold
    const bool used = wsum > 0.0f;
    const int o0 = __mul24((int)f.y0f - ymin, pitch) + ((int)f.x1f - xa1);
    r0 = used ? o0 : 0;
    r1 = used ? o0 + (f.y1f != f.y0f ? pitch : 0) : 0;
    wa = f.wa; wb = f.wb; wc = f.wc; wd = f.wd;
    return wsum;
}
__device__ __forceinline__ bool p2e_taps_cs(const P2EArgs& a, int n, float slat, float clat, float cd, float sd, Taps& t)
{
    return p2e_taps_core(a, a.tab.sphi[n], a.tab.cphi[n], slat, clat, cd, sd, t);
}
__device__ __forceinline__ bool p2e_taps(const P2EArgs& a, int n, float slat, float clat, float slon, float clon, Taps& t)
{
    float cd, sd;
    p2e_lon(a, n, slon, clon, cd, sd);
    return p2e_taps_cs(a, n, slat, clat, cd, sd, t);
}

template <typename T> struct Pair;
template <> struct Pair<float> {
    struct __attribute__((packed, aligned(4))) U { float x, y; };     // 4-byte aligned 8-byte load
    static __device__ __forceinline__ void ld(const float* p, float& x, float& y)
    { const U v = *reinterpret_cast<const U*>(p); x = v.x; y = v.y; }
};
template <> struct Pair<__half> {
    static __device__ __forceinline__ void ld(const __half* p, float& x, float& y)
    { unsigned u; __builtin_memcpy(&u, p, 4); const __half2 h = *reinterpret_cast<const __half2*>(&u);
      x = __low2float(h); y = __high2float(h); }
};

// ---- tile of the LDS kernels (p2e_lds_kernel, p2e_walk_kernel: omni_pers2equi.hip) and layout of their tables (omni_p2e_build_tiles, omni_p2e_tables.hip)
constexpr int P2E_TH = 4, P2E_TW = 32;          // ERP tile of one wave: NPX = TH/2 pixels per lane (lane -> column lane%32, rows lane/32 + 2k)
constexpr int P2E_NPX = P2E_TH / 2;
constexpr int P2E_MAXC = 12;                    // table entries (covering patches) per tile
// The ORDERED table the kernel reads: per block slot P2E_REC records of 32 bytes — {tile id | -1, covering patches, 0...}, then per covering
// patch {entry x, entry y, sin l0, cos l0 | sin p1, cos p1, 0, 0} (the patch constants ride with the entry: one scalar load per patch, issued
// one patch AHEAD, instead of a table entry and then four dependent loads from the argument segment in front of every patch), one spare.
constexpr int P2E_REC = P2E_MAXC + 2;
constexpr int P2E_NJMAX = 8;                    // 1-KiB DMA pieces per box at most: boxes up to 8 KiB
constexpr int P2E_MAX_CHUNKS = 64 * P2E_NJMAX;
constexpr int P2W_NJMAX = 6;                                   // largest box (KiB) the walk kernel is instantiated for
constexpr int P2W_SLOT = 768;                                  // bytes per block slot: header 32 | 12 patch records x 32 | trig 288 | pad
constexpr int P2W_OFF_PATCH = 32, P2W_OFF_TRIG = 32 + 32 * P2E_MAXC;
static_assert(P2W_OFF_TRIG + 8 * (P2E_TW + 8) <= P2W_SLOT, "slot layout (8-row tiles included)");
constexpr int P2W_WPB = 1;                                     // waves per block: independent waves (no barrier, each its own tile and ring) — 4x fewer workgroups to dispatch

// column origin of a tap pair: the box origin, shifted so that an x1 == x0 tap (right patch edge) becomes the pair's second element
__device__ __forceinline__ int xa_adj(int x0, int x1, int xa) { return xa + 1 - (x1 - x0); }

template <typename T> struct LdsPair;
template <> struct LdsPair<float> {
    static __device__ __forceinline__ void ld(const unsigned char* b, int o, float& x, float& y)
    { const float* p = reinterpret_cast<const float*>(b) + o; x = p[0]; y = p[1]; }              // one ds_read2_b32
};
template <> struct LdsPair<__half> {
    // halfs o, o+1: one ds_read2_b32 of the two 32-bit words around them + a byte-align (no 16-bit LDS reads, which cost a full
    // LDS instruction each)
    static __device__ __forceinline__ void ld(const unsigned char* b, int o, float& x, float& y)
    {
        const unsigned* p = reinterpret_cast<const unsigned*>(b) + (o >> 1);
        const unsigned w0 = p[0], w1 = p[1];
        const unsigned v = (o & 1) ? __builtin_amdgcn_alignbyte(w1, w0, 2u) : w0;
        const __half2 h = *reinterpret_cast<const __half2*>(&v);
        x = __low2float(h); y = __high2float(h);
    }
};

typedef __amdgpu_buffer_rsrc_t p2e_rsrc_t;
typedef __attribute__((address_space(3))) void* p2e_lptr_t;
__device__ __forceinline__ p2e_rsrc_t p2e_make_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// one LDS-DMA instruction: lane l's 16 bytes at buffer offset voff + soff (soff wave-uniform) land at lds + 16 l; an offset
// outside the buffer deposits zeros without touching memory (used for the padding lanes of a box's last piece).
// (A plain function: the host pass does not accept this builtin inside a kernel template's body.)
__device__ __forceinline__ void p2e_dma16(p2e_rsrc_t rs, unsigned char* lds, unsigned voff, unsigned soff)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (p2e_lptr_t)lds, 16, (int)voff, (int)soff, 0, 0);
}
template <int N> __device__ __forceinline__ void p2e_wait_vm()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

int fill_args(P2EArgs& a, const omni_geometry* g, const void* pers, const void* pers2, void* erp,
              int B, int C, int layout)
{
    a.pers = pers; a.pers2 = pers2; a.erp = erp;
    a.row_trig = g->row_trig; a.col_trig = g->col_trig; a.cand = g->cand;
    a.B = B; a.C = C; a.H = g->H; a.W = g->W; a.ph = g->ph; a.pw = g->pw; a.ntx = g->ntx;
    const long long N = g->N, ph = g->ph, pw = g->pw;
    if (layout == OMNI_LAYOUT_BCHWN)      { a.sX = N; a.sY = pw * N; a.sN = 1; a.sC = ph * pw * N; a.sB = C * a.sC; }
    else if (layout == OMNI_LAYOUT_BNCHW) { a.sX = 1; a.sY = pw; a.sC = ph * pw; a.sN = C * a.sC; a.sB = N * a.sN; }
    else if (layout == OMNI_LAYOUT_BNHWC) { a.sC = 1; a.sX = C; a.sY = pw * C; a.sN = ph * a.sY; a.sB = N * a.sN; }
    else OMNI_FAIL(OMNI_ERR_INVALID, "omni_pers2equi: unknown layout");
    const float PIf = (float)M_PI, PI2f = (float)(M_PI * 0.5);
    // the reference divides twice in fp32 (new_x / FOV[0] / PI); a reciprocal product differs by <= 1.5 ulp
    a.kx = (float)(1.0 / ((double)(g->fov_w / 360.0f) * (double)PIf));
    a.ky = (float)(1.0 / ((double)(g->fov_h / 180.0f) * (double)PI2f));
    a.half_h = 0.5f * (float)g->ph; a.half_w = 0.5f * (float)g->pw;
    a.tab = g->p2e;
    a.store_nt = omni_options().p2e_store ? 1 : 0;
    a.dbg = 0; a.trace = nullptr;
#ifdef OMNI_DEBUG_BUILD
    a.dbg = omni_debug_bits("OMNI_P2E_DBG");
    a.trace = omni_debug_trace_buf();
#endif
    return OMNI_OK;
}

int check_common(const omni_geometry* g, int B, int C, const char* who)
{
    if (!g) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": null geometry");
    if (B < 0 || C < 0) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": negative batch/channels");
    if (g->H < 1 || g->W < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": empty ERP size");
    return OMNI_OK;
}
}  // namespace
