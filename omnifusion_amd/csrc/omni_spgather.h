// omni_spgather.h — interface of omni_spgather.hip (the backward of equi2pers / pers2equi as a constant sparse matrix applied by gathers) and the
// host plumbing that omni_equi2pers_bwd.hip and omni_pers2equi_bwd.hip share: the box tables of their tile kernels, the build-once block.
#pragma once
#include "omni_internal.h"

// how one application addresses its operands: source element of entry e (hi 8 bits | lo 24 bits of e.x) and plane p, destination of row r
struct SpApply {                          // (the argument block of the gather kernels)
    const uint2* ent; const int* slice_off; const int* cnt; int nrows, nslices;
    const uint2* long_ent; const int* long_off; const int* long_row; int nlong;
    const float* src; float* dst;
    int C, planes;                        // plane p = (batch p / C, channel p % C)
    long long s_sB, s_sC, d_sB, d_sC;     // element strides of batch / channel in source and destination
    int s_hi, s_lo;                       // source offset inside a plane: (e.x >> 24) * s_hi + (e.x & 0xffffff) * s_lo
    int rdiv; long long d_hi; int d_lo;   // destination offset of row r inside a plane: (r / rdiv) * d_hi + (r % rdiv) * d_lo
    // the plane-interleaved copy of the source (sp_interleave_kernel): record (hi, lo) = PT consecutive floats, one per plane (padded to a multiple of 4)
    int chunk;                            // blocks (of 4 slices) per XCD chunk
    const float* ws; int PT; int nhi, nlo, hi_fastest;   // record index = hi_fastest ? lo * nhi + hi : hi * nlo + lo  (the order the source itself is contiguous in)
};
// fills the table's part of `s` and launches.  ws != null: through the plane-interleaved copy (ws holds nhi * nlo records of s.PT floats);
// else 4-byte gathers from the source itself
int omni_sp_apply(const OmniSpTable& t, SpApply s, hipStream_t stream, float* ws);

// host state of one table build and its three steps (omni_sp_build below runs them)
struct SpBuild {
    OmniSpTable* t = nullptr; int* d_cnt = nullptr; int* d_rowpos = nullptr; bool fits = false; std::vector<int> h_loff;
    ~SpBuild();
};
int omni_sp_begin(SpBuild& sb, OmniSpTable* t, int nrows, hipStream_t stream);
int omni_sp_layout(SpBuild& sb, size_t budget, hipStream_t stream);        // after pass 0
int omni_sp_finish(SpBuild& sb, const char* label, hipStream_t stream);     // after pass 1 (or over budget: frees the table)

// the first backward call of a geometry builds the operator's tables, under g->bwd_mu (synchronises the stream once)
int omni_bwd_build_once(const omni_geometry* g, int omni_geometry::*tried, int (*build)(omni_geometry*, hipStream_t), hipStream_t stream);

namespace {

struct SpEmit {
    int pass;                 // 0: count, 1: fill
    int* cnt;                 // pass 0: entries per row; pass 1: the cursor (zeroed again)
    const int* rowpos;        // pass 1: >= 0: index of the row's entry 0 in `ent` (stride 64); < 0: -(1 + index in long_ent) (stride 1)
    uint2* ent; uint2* long_ent;
};
__device__ __forceinline__ void sp_emit(const SpEmit& b, int row, unsigned src, float w)
{
    if (b.pass == 0) { atomicAdd(b.cnt + row, 1); return; }
    const int slot = atomicAdd(b.cnt + row, 1), rp = b.rowpos[row];
    const uint2 e = make_uint2(src, __float_as_uint(w));
    if (rp >= 0) b.ent[(size_t)rp + (size_t)slot * 64] = e;
    else         b.long_ent[(size_t)(-1 - rp) + slot] = e;
}

// Builds table `t` of `nrows` rows: walk(SpEmit) launches the operator's walk kernel on `stream`, once to count the entries of every row and, if
// the table stays within `budget` bytes, once more to deposit them; over budget the table is freed again (t->ok stays 0: the older kernels serve).
template <class Walk>
int omni_sp_build(OmniSpTable* t, int nrows, size_t budget, hipStream_t stream, const char* label, Walk&& walk)
{
    SpBuild sb;
    int rc = omni_sp_begin(sb, t, nrows, stream);
    if (rc != OMNI_OK) return rc;
    walk(SpEmit{0, sb.d_cnt, sb.d_rowpos, t->ent, t->long_ent});
    rc = omni_sp_layout(sb, budget, stream);
    if (rc != OMNI_OK) return rc;
    if (sb.fits) walk(SpEmit{1, sb.d_cnt, sb.d_rowpos, t->ent, t->long_ent});
    return omni_sp_finish(sb, label, stream);
}

// The box tables of the tile-gather kernels (the fallback of rounds 2-3): `per_tile` boxes (min, max, min, max: empty where x > y) per tile, filled
// by the operator's box kernel with atomicMin / atomicMax (launch(boxes), on `stream`: allocates what else that kernel writes, launches it, returns a
// status); then the tile ids, the tiles whose boxes together hold at most `limit` elements first (nsmall of them: one wave each), the big ones behind
// (1024 threads each).  ps / pb / mx: elements in small / big / the largest.  (Device allocations in the order they always had: boxes, the launch's, ids.)
struct BwdBoxes { int nsmall, nbig; long long ps, pb, mx; };
template <class Launch>
int omni_bwd_boxes(int4** boxes, int** ids, size_t ntiles, int per_tile, long long limit, hipStream_t stream, BwdBoxes* out, Launch&& launch)
{
    const size_t nbox = ntiles * per_tile;
    OMNI_HIP(hipMalloc((void**)boxes, sizeof(int4) * nbox));
    std::vector<int4> hb(nbox, make_int4(0x7fffffff, -0x7fffffff, 0x7fffffff, -0x7fffffff));
    OMNI_HIP(hipMemcpy(*boxes, hb.data(), sizeof(int4) * nbox, hipMemcpyHostToDevice));
    const int rc = launch(*boxes);
    if (rc != OMNI_OK) return rc;
    OMNI_HIP(hipGetLastError());
    OMNI_HIP(hipStreamSynchronize(stream));
    OMNI_HIP(hipMemcpy(hb.data(), *boxes, sizeof(int4) * nbox, hipMemcpyDeviceToHost));
    std::vector<int> small, big;
    BwdBoxes& r = *out = {0, 0, 0, 0, 0};
    for (size_t t = 0; t < ntiles; ++t) {
        long long npx = 0;
        for (int k = 0; k < per_tile; ++k) {
            const int4 b = hb[t * per_tile + k];
            if (b.x <= b.y) npx += (long long)(b.y - b.x + 1) * (b.w - b.z + 1);
        }
        (npx <= limit ? small : big).push_back((int)t);
        (npx <= limit ? r.ps : r.pb) += npx; r.mx = npx > r.mx ? npx : r.mx;
    }
    r.nsmall = (int)small.size(); r.nbig = (int)big.size();
    small.insert(small.end(), big.begin(), big.end());
    OMNI_HIP(hipMalloc((void**)ids, sizeof(int) * ntiles));
    OMNI_HIP(hipMemcpy(*ids, small.data(), sizeof(int) * ntiles, hipMemcpyHostToDevice));
    return OMNI_OK;
}
}  // namespace
