// omni_fixedpoint.h — the order-independent scatter sum of DESIGN.md §11, shared by omni_dibr.hip and omni_freeview_bwd.hip.
//
// Every contribution x is rounded ONCE to q = rint(x * 2^s) and added with a 64-bit integer atomic; integer addition is associative, so a
// sum has the same bits in any order.  s = 62 - ceil(log2 sources) - e with e = ceil(log2 max|x|) over the finite values of one item.
#pragma once
#include "omni_internal.h"

namespace {

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e38f; }

// e = ceil(log2 m) of the per-item maximum (bits of a non-negative float), clamped so that both 2^s and 2^-s are normal floats
__device__ __forceinline__ int dibr_exponent(unsigned bits)
{
    const float m = __uint_as_float(bits);
    if (!(m > 0.0f)) return 0;
    int k;
    const float f = frexpf(m, &k);                                  // m = f * 2^k, f in [0.5, 1)
    const int e = (f == 0.5f) ? k - 1 : k;
    return e < -60 ? -60 : e;
}

__device__ __forceinline__ float pow2f(int s) { return __int_as_float((127 + s) << 23); }     // s in [-126, 127]

__device__ __forceinline__ long long fixq(float x, float scale) { return (long long)rintf(x * scale); }   // x * 2^s is exact; one rounding

__global__ __launch_bounds__(256) void dibr_zero_kernel(uint4* __restrict__ p, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace
