// omni_reduce.h — the wave and block reductions every unit uses, stated once: "fixed order, no atomics" is a property of this header.
//
// Wave level: the xor butterfly over the 64 lanes, offsets 32, 16, ..., 1, operand order v = op(v, shuffled); every lane ends with the result.
// Block level (256 threads = 4 waves): lane 0 of each wave stores its wave's value, one barrier, then (r0 + r1) + (r2 + r3) in every thread.
// The bits of a floating-point sum depend on exactly this order (the library is built with -ffp-contract=off), so a kernel that reduces by
// other means says why.  The order ACROSS blocks (partials per slab or chunk, added by a finish kernel) is stated in omni_partials.h.
//
// The kernels of the network and the resamplers (omni_net, omni_conv_sh, omni_gemm_rows, omni_spgather, omni_e2p_tables, omni_p2e_tables, the
// max passes of omni_dibr and omni_freeview_bwd) and block_reduce below still spell the same butterfly out.  Their machine code is pinned
// against the parent's (tools/split_isa_diff.py), and hipcc does not compile a call of these helpers to the instructions of the open-coded loop:
// the by-value parameter is `noundef`, which drops the freeze HIP's __shfl_xor puts on its operand, and the helper is simplified before it is
// inlined, which leaves operands commuted and address arithmetic scheduled elsewhere.  Same values, other instruction sequence; moving those
// sites here is a change of its own, with a benchmark beside it.
#pragma once
#include <hip/hip_runtime.h>

namespace {

template <typename T>
__device__ __forceinline__ T wave_sum(T v)                                   // float, double, long long
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Sums v[0..N) over the 256 threads of the block; every thread returns with the sums.  red: [N][4], LDS; a caller that reuses it puts a
// barrier between two calls.  T: double (the loss partials), long long (counts, whose sum has no order to keep).
template <int N, typename T>
__device__ __forceinline__ void block_sum(T (&v)[N], T (*red)[4])
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}

// min or max of an int over the 256 threads of the block, in every thread; red: [4], LDS, reused from call to call (hence the first barrier)
__device__ __forceinline__ int block_reduce(int v, bool is_max, int* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = is_max ? max(v, t) : min(v, t); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) v = is_max ? max(v, red[k]) : min(v, red[k]);
    return v;
}

}  // namespace
