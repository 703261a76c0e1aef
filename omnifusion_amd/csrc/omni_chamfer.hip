// omni_chamfer.hip — the one-directional Chamfer term between two point clouds (util.py:201-257 of the reference,
// chamfer_distance_with_batch) and its gradient w.r.t. both clouds:
//
//   omni_chamfer_nn_f32      p1 [B,N,D], p2 [B,M,D], optional uint8 masks -> dist [B,N] = min_j |p1_i - p2_j|, idx [B,N] = argmin, *loss = sum(dist)
//   omni_chamfer_grad_f32    grad_p1 [B,N,D] = g_i (p1_i - p2_idx) / dist_i, grad_p2 [B,M,D] = -(the same vectors summed per target)
//
// The reference repeats both clouds to [B,N,M,D]; here nothing of size N x M exists.  Nearest neighbours: a block of 256 threads owns CH_QB =
// 512 queries of one item, two per thread in registers, and walks the targets of its chunk in tiles of CH_TILE = 256 padded float4 in LDS (a
// thread stages one target per tile, the next tile's target is already in flight while the current tile is scanned); every lane reads the
// same LDS address, so one broadcast read serves both queries.  The squared distance is dx dx + dy dy + dz dz from direct differences (the
// expansion |a|^2 + |b|^2 - 2ab loses two digits), compared with a strict < in ascending j: the lowest index wins a tie; sqrt once, of the
// winner.  A masked target is staged as +inf coordinates: its squared distance is +inf, which is never < anything.
// Few queries and many targets: gridDim.y chunks of whole tiles; each leaves (d^2, index) per query in the workspace and chamfer_merge_kernel
// takes them in chunk order with the same strict <, so the result has the bits of the unsplit walk.  Both paths end in chamfer_finish: the
// same thread adds the same two distances in double, the block sum of omni_reduce.h, one double per (item, query block); one final block
// adds those in a fixed order and rounds to float32 once.  No atomics: the same bits on every run.
// NaN: a valid point with a NaN coordinate is FOUND while staging (targets) or loading (queries), not left to the comparisons: a target's flag
// makes every distance of the item NaN, a query's flag its own — what torch.min gives the reference.  An item without a valid target:
// dist = +inf, idx = -1 (every squared distance is +inf, nothing is special-cased).
// Gradient: a thread per query recomputes the winner's difference and distance (the forward's arithmetic, so dist == 0 is the same
// predicate), writes grad_p1 and sends the negated vector to target idx_i through §11's 64-bit fixed-point sums (omni_fixedpoint.h): unit
// 2^(e + ceil(log2 N) - 62) with e = ceil(log2) of the item's largest |g_i| — the components of a unit vector are <= 1 and a target takes at
// most N contributions.  Integer atomics commute: the same bits in any order.  A non-finite contribution sets a poison bit of its target.
#include <algorithm>

#include "omni_internal.h"
#include "omni_fixedpoint.h"
#include "omni_reduce.h"

namespace {

constexpr int CH_THREADS = 256, CH_Q = 2, CH_QB = CH_THREADS * CH_Q, CH_TILE = CH_THREADS;
constexpr int CH_BATCH = 8;                               // targets read from LDS ahead of their arithmetic; divides CH_TILE
constexpr int CH_TARGET_BLOCKS = 2048;                    // the split plan aims at eight blocks per CU of a 256-CU device (more resident waves hide the LDS waits: DESIGN.md §16, Measured)
constexpr int CH_MAX_B = 65535;                           // gridDim.z
constexpr int CH_MAX_POINTS = 0x7fffffff - 2 * CH_QB;  // of one item's cloud: int indices, one tile or query block past the end included
constexpr float CH_INF = __builtin_inff();

struct ChPlan { int qblocks, chunks, chunk_len; };

// A function of the shape alone (not of the device): workspace sizes and the launch agree by construction.
ChPlan ch_plan(int B, int N, int M, bool split)
{
    ChPlan p;
    p.qblocks = (N + CH_QB - 1) / CH_QB;
    const long long tiles = ((long long)M + CH_TILE - 1) / CH_TILE, blocks = (long long)B * p.qblocks;
    long long want = split ? (CH_TARGET_BLOCKS + blocks - 1) / blocks : 1;
    if (want > tiles) want = tiles;
    if (want > 65535) want = 65535;
    const long long tiles_per = (tiles + want - 1) / want;
    p.chunks = (int)((tiles + tiles_per - 1) / tiles_per);
    p.chunk_len = p.chunks == 1 ? M : (int)(tiles_per * CH_TILE);      // chunks > 1: tiles_per * 256 < M
    return p;
}

struct ChWs { size_t part, flags, pairs, hdr, acc, poison, total; };

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

ChWs ch_layout(int B, int N, int M, int D)
{
    const ChPlan p = ch_plan(B, N, M, true);
    ChWs l;
    l.part = 0;                                                            // double [B][qblocks]
    l.flags = up256(sizeof(double) * (size_t)B * p.qblocks);               // int [B][chunks][qblocks]
    l.pairs = l.flags + up256(sizeof(int) * (size_t)B * p.chunks * p.qblocks);          // float2 (d^2, index bits) [B][chunks][N]
    l.hdr = l.pairs + (p.chunks > 1 ? up256(sizeof(float2) * (size_t)B * p.chunks * N) : 0);   // unsigned max |g| bits [B]
    l.acc = l.hdr + up256(sizeof(unsigned) * (size_t)B);                   // long long [B][M][D]
    l.poison = l.acc + sizeof(long long) * (size_t)B * M * D;              // one bit per target point
    l.total = up256(l.poison + (((size_t)B * M + 31) / 32) * sizeof(unsigned));
    return l;
}

// dist, idx and the block's double partial for the block's CH_QB queries; d2 / best / state per query of this thread (state: 0 masked or out
// of range, 1 valid, 2 valid with a NaN coordinate); nan_item: a valid target of the item has a NaN coordinate (block-uniform)
__device__ __forceinline__ void chamfer_finish(const float (&d2)[CH_Q], const int (&best)[CH_Q], const int (&state)[CH_Q], bool nan_item, int N, int q0,
                                               float* __restrict__ dist, int* __restrict__ idx, double* __restrict__ part)
{
    __shared__ double red[1][CH_THREADS / 64];
    double s[1] = {0.0};
#pragma unroll
    for (int k = 0; k < CH_Q; ++k) {
        const int i = q0 + k * CH_THREADS + threadIdx.x;
        if (i >= N) continue;
        float d = 0.0f;
        int j = -1;
        if (state[k]) {
            if (nan_item || state[k] == 2) d = __int_as_float(0x7fc00000);
            else { d = sqrtf(d2[k]); j = best[k]; }
            s[0] += (double)d;
        }
        dist[i] = d;
        idx[i] = j;
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) *part = s[0];
}

// The squared distance of direct differences.  The library is built with -ffp-contract=off, so the two fused multiply-adds are written out:
// one product and two fmaf, each rounded once — 9 vector instructions per pair with the three subtractions, the comparison and the two
// selects, where products and additions apart take 11.  The forward and the gradient call this one function: the same bits.
template <int D>
__device__ __forceinline__ float chamfer_d2(float dx, float dy, float dz)
{
    const float s = fmaf(dy, dy, dx * dx);
    if constexpr (D == 3) return fmaf(dz, dz, s);
    return s;
}

struct ChArgs {
    const float* p1; const float* p2;
    const unsigned char* mask1; const unsigned char* mask2;
    int N, M, chunk_len;
    float* dist; int* idx;
    double* part; int* flags; float2* pairs;
};

// grid (qblocks, chunks, B)
template <int D>
__global__ __launch_bounds__(CH_THREADS) void chamfer_nn_kernel(const ChArgs a)
{
    __shared__ float4 tile[CH_TILE];
    const int b = blockIdx.z, chunk = blockIdx.y, q0 = blockIdx.x * CH_QB;
    const int N = a.N, M = a.M;
    const size_t qbase = (size_t)b * N, tbase = (size_t)b * M;
    const int j_begin = chunk * a.chunk_len, j_end = j_begin + min(a.chunk_len, M - j_begin);      // chunk * chunk_len < M <= CH_MAX_POINTS

    float qx[CH_Q], qy[CH_Q], qz[CH_Q], d2[CH_Q];
    int best[CH_Q], state[CH_Q];
#pragma unroll
    for (int k = 0; k < CH_Q; ++k) {
        const int i = q0 + k * CH_THREADS + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0f;
        d2[k] = CH_INF; best[k] = -1; state[k] = 0;
        if (i < N && (!a.mask1 || a.mask1[qbase + i])) {
            const float* p = a.p1 + (qbase + i) * D;
            qx[k] = p[0]; qy[k] = p[1];
            if constexpr (D == 3) qz[k] = p[2];
            state[k] = (qx[k] != qx[k] || qy[k] != qy[k] || qz[k] != qz[k]) ? 2 : 1;
        }
    }

    // one target per thread and tile; a masked or out-of-range target is +inf and never the minimum
    bool nan_seen = false;
    auto fetch = [&](int j0) {
        const int j = j0 + threadIdx.x;
        float4 t = make_float4(CH_INF, CH_INF, D == 3 ? CH_INF : 0.0f, 0.0f);
        if (j < j_end && (!a.mask2 || a.mask2[tbase + j])) {
            const float* p = a.p2 + (tbase + j) * D;
            t.x = p[0]; t.y = p[1];
            if constexpr (D == 3) t.z = p[2];
            nan_seen |= (t.x != t.x || t.y != t.y || t.z != t.z);
        }
        return t;
    };

    float4 next = fetch(j_begin);
    for (int j0 = j_begin; j0 < j_end; j0 += CH_TILE) {
        __syncthreads();                                             // the previous tile has been scanned
        tile[threadIdx.x] = next;
        __syncthreads();
        if (j0 + CH_TILE < j_end) next = fetch(j0 + CH_TILE);
        const int cnt = min(CH_TILE, j_end - j0);                  // the slots past cnt hold +inf too: the scan runs in whole batches
        for (int t0 = 0; t0 < cnt; t0 += CH_BATCH) {
            float4 p[CH_BATCH];
#pragma unroll
            for (int u = 0; u < CH_BATCH; ++u) p[u] = tile[t0 + u];
#pragma unroll
            for (int u = 0; u < CH_BATCH; ++u) {
#pragma unroll
                for (int k = 0; k < CH_Q; ++k) {
                    float dz = 0.0f;
                    if constexpr (D == 3) dz = qz[k] - p[u].z;
                    const float s = chamfer_d2<D>(qx[k] - p[u].x, qy[k] - p[u].y, dz);
                    const bool lt = s < d2[k];                       // strict, ascending j: the lowest index keeps a tie
                    d2[k] = lt ? s : d2[k];
                    best[k] = lt ? j0 + t0 + u : best[k];
                }
            }
        }
    }
    const int nan_item = __syncthreads_or(nan_seen ? 1 : 0);

    if (gridDim.y == 1) {
        chamfer_finish(d2, best, state, nan_item != 0, N, q0, a.dist + qbase, a.idx + qbase, a.part + (size_t)b * gridDim.x + blockIdx.x);
        return;
    }
    const size_t slot = (size_t)b * gridDim.y + chunk;
    if (threadIdx.x == 0) a.flags[slot * gridDim.x + blockIdx.x] = nan_item;
#pragma unroll
    for (int k = 0; k < CH_Q; ++k) {
        const int i = q0 + k * CH_THREADS + threadIdx.x;
        if (i < N) a.pairs[slot * N + i] = make_float2(state[k] == 2 ? __int_as_float(0x7fc00000) : d2[k], __int_as_float(best[k]));      // a NaN query never left d2 = +inf: NaN carries its flag
    }
}

// grid (qblocks, 1, B): the chunks' candidates in chunk order = ascending j
__global__ __launch_bounds__(CH_THREADS) void chamfer_merge_kernel(const ChArgs a, int chunks)
{
    const int b = blockIdx.z, q0 = blockIdx.x * CH_QB, N = a.N;
    const size_t qbase = (size_t)b * N;
    float d2[CH_Q];
    int best[CH_Q], state[CH_Q];
#pragma unroll
    for (int k = 0; k < CH_Q; ++k) {
        const int i = q0 + k * CH_THREADS + threadIdx.x;
        d2[k] = CH_INF; best[k] = -1; state[k] = 0;
        if (i < N && (!a.mask1 || a.mask1[qbase + i])) state[k] = 1;
    }
    int nan_item = 0;
    for (int c = 0; c < chunks; ++c) {
        const size_t slot = (size_t)b * chunks + c;
        nan_item |= a.flags[slot * gridDim.x + blockIdx.x];
#pragma unroll
        for (int k = 0; k < CH_Q; ++k) {
            const int i = q0 + k * CH_THREADS + threadIdx.x;
            if (i >= N) continue;
            const float2 v = a.pairs[slot * N + i];
            if (v.x != v.x && state[k]) state[k] = 2;               // the query's own NaN flag (see chamfer_nn_kernel)
            const bool lt = v.x < d2[k];
            d2[k] = lt ? v.x : d2[k];
            best[k] = lt ? __float_as_int(v.y) : best[k];
        }
    }
    chamfer_finish(d2, best, state, nan_item != 0, N, q0, a.dist + qbase, a.idx + qbase, a.part + (size_t)b * gridDim.x + blockIdx.x);
}

// One block: thread t adds partials t, t + 256, ... in that order, then the fixed tree; one rounding to float32.
__global__ __launch_bounds__(CH_THREADS) void chamfer_final_kernel(const double* __restrict__ part, size_t nparts, float* __restrict__ loss)
{
    __shared__ double red[1][CH_THREADS / 64];
    double s[1] = {0.0};
    for (size_t k = threadIdx.x; k < nparts; k += CH_THREADS) s[0] += part[k];
    block_sum<1>(s, red);
    if (threadIdx.x == 0) *loss = (float)s[0];
}

// ------------------------------------------------------------------ gradient
__device__ __forceinline__ float chamfer_upstream(const float* __restrict__ grad_loss, const float* __restrict__ grad_dist, size_t q)
{
    const float gl = grad_loss ? *grad_loss : 0.0f;
    return grad_dist ? gl + grad_dist[q] : gl;
}

// maxbits[b] = max |g_i| over the item's queries that have a neighbour, finite values only; grid (blocks, B)
__global__ __launch_bounds__(CH_THREADS) void chamfer_gmax_kernel(const float* __restrict__ grad_loss, const float* __restrict__ grad_dist,
                                                                  const int* __restrict__ idx, int N, unsigned* __restrict__ maxbits)
{
    __shared__ float part[CH_THREADS / 64];
    const size_t qbase = (size_t)blockIdx.y * N;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * CH_THREADS + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * CH_THREADS) {
        if (idx[qbase + i] < 0) continue;
        const float g = chamfer_upstream(grad_loss, grad_dist, qbase + i);
        if (finite(g)) m = fmaxf(m, fabsf(g));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(maxbits + blockIdx.y, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}

// a thread per query; grid (ceil(N / 256), B).  acc == nullptr: grad_p1 only; grad_p1 == nullptr: the scatter only
template <int D>
__global__ __launch_bounds__(CH_THREADS) void chamfer_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2, const unsigned char* __restrict__ mask1,
                                                                  const int* __restrict__ idx, const float* __restrict__ grad_loss,
                                                                  const float* __restrict__ grad_dist, int N, int M, int L, float* __restrict__ grad_p1,
                                                                  unsigned long long* __restrict__ acc, unsigned* __restrict__ poison,
                                                                  const unsigned* __restrict__ maxbits)
{
    const int b = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * CH_THREADS + threadIdx.x;
    if (i >= (size_t)N) return;
    const size_t q = (size_t)b * N + i;
    const int j = idx[q];
    float v[3] = {0.0f, 0.0f, 0.0f};
    bool sends = false;
    if (j >= 0 && j < M && (!mask1 || mask1[q])) {
        const float* a = p1 + q * D;
        const float* t = p2 + ((size_t)b * M + j) * D;
        const float dx = a[0] - t[0], dy = a[1] - t[1];
        float dz = 0.0f;
        if constexpr (D == 3) dz = a[2] - t[2];
        const float d = sqrtf(chamfer_d2<D>(dx, dy, dz));            // the forward's arithmetic: the same bits, the same d == 0
        if (d != 0.0f) {                                             // the 2-norm's subgradient at 0 is 0
            const float g = chamfer_upstream(grad_loss, grad_dist, q);
            v[0] = g * (dx / d); v[1] = g * (dy / d); v[2] = g * (dz / d);
            sends = true;
        }
    }
    if (grad_p1) {
#pragma unroll
        for (int c = 0; c < D; ++c) grad_p1[q * D + c] = v[c];
    }
    if (acc && sends) {
        const size_t t = (size_t)b * M + j;
        const float sc = pow2f(62 - L - dibr_exponent(maxbits[b]));
        bool bad = false;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            if (!finite(v[c])) { bad = true; continue; }
            const long long qv = fixq(v[c], sc);
            if (qv != 0) atomicAdd(acc + t * D + c, (unsigned long long)(-qv));      // two's complement: signed sums wrap
        }
        if (bad) atomicOr(poison + (t >> 5), 1u << (t & 31));
    }
}

// int64 sums -> float32; every component of a poisoned target is NaN.  n = B M D elements, per_item = M D
__global__ __launch_bounds__(CH_THREADS) void chamfer_convert_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ poison,
                                                                     const unsigned* __restrict__ maxbits, size_t n, size_t per_item, int D, int L,
                                                                     float* __restrict__ grad)
{
    for (size_t e = (size_t)blockIdx.x * CH_THREADS + threadIdx.x; e < n; e += (size_t)gridDim.x * CH_THREADS) {
        const float inv = pow2f(-(62 - L - dibr_exponent(maxbits[e / per_item])));
        const size_t t = e / D;
        const bool bad = poison[t >> 5] >> (t & 31) & 1u;
        grad[e] = bad ? __int_as_float(0x7fc00000) : (float)acc[e] * inv;
    }
}

int ch_check(const char* who, int B, int N, int M, int D)
{
    if (B < 1 || N < 1 || M < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": B, N, M >= 1 required");
    if (D != 2 && D != 3) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": D must be 2 or 3");
    if (B > CH_MAX_B || N > CH_MAX_POINTS || M > CH_MAX_POINTS) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 items or 2^31 - 1025 points per item");
    return OMNI_OK;
}

int ch_ceil_log2(long long n)
{
    int l = 0;
    while ((1ll << l) < n) ++l;
    return l;
}

}  // namespace

extern "C" size_t omni_chamfer_workspace_bytes(int B, int N, int M, int D)
{
    if (B < 1 || N < 1 || M < 1 || (D != 2 && D != 3) || B > CH_MAX_B || N > CH_MAX_POINTS || M > CH_MAX_POINTS) return 0;
    return ch_layout(B, N, M, D).total;
}

extern "C" int omni_chamfer_nn_f32(const float* p1, const float* p2, const unsigned char* mask1, const unsigned char* mask2, int B, int N, int M,
                                   int D, float* dist, int* idx, float* loss, void* workspace, omni_stream_t stream)
{
    const char* who = "omni_chamfer_nn_f32";
    if (!p1 || !p2 || !dist || !idx || !loss || !workspace) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": null device pointer");
    if (const int rc = ch_check(who, B, N, M, D)) return rc;
    if ((uintptr_t)workspace & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": the workspace must be 16-byte aligned");
    const ChWs l = ch_layout(B, N, M, D);
    const ChPlan p = ch_plan(B, N, M, omni_options().chamfer_split != 0);      // never more chunks than the layout was sized for
    char* base = (char*)workspace;
    ChArgs a;
    a.p1 = p1; a.p2 = p2; a.mask1 = mask1; a.mask2 = mask2;
    a.N = N; a.M = M; a.chunk_len = p.chunk_len;
    a.dist = dist; a.idx = idx;
    a.part = (double*)(base + l.part); a.flags = (int*)(base + l.flags); a.pairs = (float2*)(base + l.pairs);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(p.qblocks, p.chunks, B), block(CH_THREADS);
    if (D == 3) hipLaunchKernelGGL(chamfer_nn_kernel<3>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(chamfer_nn_kernel<2>, grid, block, 0, s, a);
    if (p.chunks > 1) hipLaunchKernelGGL(chamfer_merge_kernel, dim3(p.qblocks, 1, B), block, 0, s, a, p.chunks);
    hipLaunchKernelGGL(chamfer_final_kernel, dim3(1), block, 0, s, (const double*)a.part, (size_t)B * p.qblocks, loss);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_chamfer_grad_f32(const float* p1, const float* p2, const unsigned char* mask1, const int* idx, const float* grad_loss,
                                     const float* grad_dist, int B, int N, int M, int D, float* grad_p1, float* grad_p2, void* workspace,
                                     omni_stream_t stream)
{
    const char* who = "omni_chamfer_grad_f32";
    if (!p1 || !p2 || !idx) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": null device pointer");
    if (!grad_loss && !grad_dist) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": no upstream gradient (grad_loss and grad_dist are both null)");
    if (!grad_p1 && !grad_p2) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": no gradient requested (grad_p1 and grad_p2 are both null)");
    if (const int rc = ch_check(who, B, N, M, D)) return rc;
    if (grad_p2 && !workspace) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": grad_p2 needs the workspace");
    if ((uintptr_t)workspace & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(CH_THREADS), grid((unsigned)(((size_t)N + CH_THREADS - 1) / CH_THREADS), B);
    const int L = ch_ceil_log2(N);
    unsigned long long* acc = nullptr;
    unsigned *poison = nullptr, *maxbits = nullptr;
    if (grad_p2) {
        const ChWs l = ch_layout(B, N, M, D);
        char* base = (char*)workspace;
        maxbits = (unsigned*)(base + l.hdr); acc = (unsigned long long*)(base + l.acc); poison = (unsigned*)(base + l.poison);
        const size_t n16 = (l.total - l.hdr) / 16;
        hipLaunchKernelGGL(dibr_zero_kernel, dim3((unsigned)std::min<size_t>((n16 + CH_THREADS - 1) / CH_THREADS, 2048)), block, 0, s, (uint4*)(base + l.hdr), n16);
        const unsigned mx = (unsigned)std::min<size_t>(((size_t)N + 1023) / 1024, 64);
        hipLaunchKernelGGL(chamfer_gmax_kernel, dim3(mx, B), block, 0, s, grad_loss, grad_dist, idx, N, maxbits);
    }
    if (D == 3) hipLaunchKernelGGL(chamfer_grad_kernel<3>, grid, block, 0, s, p1, p2, mask1, idx, grad_loss, grad_dist, N, M, L, grad_p1, acc, poison, (const unsigned*)maxbits);
    else hipLaunchKernelGGL(chamfer_grad_kernel<2>, grid, block, 0, s, p1, p2, mask1, idx, grad_loss, grad_dist, N, M, L, grad_p1, acc, poison, (const unsigned*)maxbits);
    if (grad_p2) {
        const size_t n = (size_t)B * M * D;
        const unsigned cb = (unsigned)std::min<size_t>((n + CH_THREADS - 1) / CH_THREADS, 8192);
        hipLaunchKernelGGL(chamfer_convert_kernel, dim3(cb), block, 0, s, (const long long*)acc, (const unsigned*)poison, (const unsigned*)maxbits, n,
                           (size_t)M * D, D, L, grad_p2);
    }
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
