// omni_partials.h — sums that cross blocks, stated once: a pass writes one partial per slab of rows or chunk of tiles, a small
// finish kernel adds the partials in double in a FIXED order and rounds once.  That order decides the bits of every parameter gradient, so
// no unit restates it.  The passes that PRODUCE partials stay open-coded in their units (the note in omni_reduce.h).
#pragma once
#include "omni_reduce.h"

namespace {

// Host plan: per = max(ceil(ceil(units / max_parts) / step), min_steps) . step units in a partial — a floor on its work, at most max_parts
// partials — and n = ceil(units / per) partials.  False where per does not fit an int.
inline bool partials_plan(long long units, int step, int min_steps, int max_parts, int& per, int& n)
{
    long long steps = ((units + max_parts - 1) / max_parts + step - 1) / step;
    if (steps < min_steps) steps = min_steps;
    if (steps * step >= (1ll << 31)) return false;
    per = (int)(steps * step);
    n = (int)((units + per - 1) / per);
    return true;
}

// Column finish, a block of 256 threads: v[j] = sum over b < nparts of part[b . stride + j . plane], j < N.  Thread t adds b = t, t + 256, ...
// in ascending order in double (P: float or double), then block_sum<N>: every thread returns with the sums.  red: [N][4], LDS.
template <int N, typename P>
__device__ __forceinline__ void column_sums(const P* __restrict__ part, int nparts, size_t stride, size_t plane, double (&v)[N], double (*red)[4])
{
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 256) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += (double)part[(size_t)b * stride + j * plane];
    }
    block_sum<N>(v, red);
}

// Chunk finish over float part[nchunk][PART], a whole kernel: block b owns the outputs 16 b .. 16 b + 15 (ceil(PART / 16) blocks).  Lane
// l = t >> 4 adds the chunks l, l + 16, ... of output e = t & 15 in ascending order in double; thread e < 16 then adds the lanes 0 .. 15 in
// order and rounds once.  Outputs below SPLIT go to `lo`, the rest to `hi`; either may be null (not asked for).
template <int PART, int SPLIT>
__device__ __forceinline__ void chunk_sums(const float* __restrict__ part, int nchunk, float* __restrict__ lo, float* __restrict__ hi)
{
    __shared__ double red[16][16];
    const int t = threadIdx.x, e = t & 15, lane = t >> 4;
    const int idx = blockIdx.x * 16 + e;
    double s = 0.0;
    if (idx < PART) {
#pragma unroll 4
        for (int b = lane; b < nchunk; b += 16) s += (double)part[(size_t)b * PART + idx];
    }
    red[lane][e] = s;
    __syncthreads();
    if (t < 16 && idx < PART) {
        double v = red[0][t];
#pragma unroll
        for (int l = 1; l < 16; ++l) v += red[l][t];
        if (idx < SPLIT) { if (lo) lo[idx] = (float)v; }
        else if (hi) hi[idx - SPLIT] = (float)v;
    }
}

}  // namespace
