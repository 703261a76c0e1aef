// omni_normals.h — the per-pixel arithmetic of the geometry terms of depth training (util.py:332-382 depth2normal_gpu, :426-451 imgrad /
// imgrad_yx), shared by the stand-alone mirrors and the fused loss kernels of omni_normals.hip so that the two cannot drift apart.
//
// Every function takes an accessor `at(di, dj)` -> float: the map at (row + di, column + dj).  The fused kernels read a tile staged in LDS, the
// mirrors read global memory with bounds checks; the arithmetic, and therefore the bits, are the same.  The library is built with
// -ffp-contract=off: every product and sum below is rounded once, in the order written.
#pragma once
#include "omni_internal.h"

namespace geo {

constexpr float EPS = 1e-12f;                       // F.normalize's eps

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 zero3() { return {0.0f, 0.0f, 0.0f}; }

// The four ray tables of one image size, float32, built on the host from coords2uv / uv2xyz (util.py:159-174): sin / cos of the latitude of
// row i, sin / cos of the longitude of column j.  One device array [sv: H][cv: H][su: W][cu: W].
struct Rays { const float* sv; const float* cv; const float* su; const float* cu; };
__host__ __device__ inline Rays rays_of(const float* tab, int H, int W) { return {tab, tab + H, tab + 2 * (size_t)H, tab + 2 * (size_t)H + W}; }
// uv2xyz: x = cos v sin u, y = cos v cos u, z = sin v, single float32 products (0 <= i < H, 0 <= j < W)
__device__ __forceinline__ V3 ray(const Rays& t, int i, int j) { const float c = t.cv[i]; return {c * t.su[j], c * t.cu[j], t.sv[i]}; }

// V - V' = ray * depth - ray' * depth': the products are exact in double (two float32 factors) and the difference is rounded to float32 once.
// Next to a pole two neighbouring vertices of a row lie cos(lat) * 2 pi / W apart: float32 vertices lose four digits of that difference
// (the reference's own float32 normals are off by 4e-5 in the pole rows of a 70-row map), this form loses none.
__device__ __forceinline__ V3 edge(V3 r, float d, V3 r2, float d2)
{
    const double a = d, b = d2;
    return {(float)((double)r.x * a - (double)r2.x * b), (float)((double)r.y * a - (double)r2.y * b), (float)((double)r.z * a - (double)r2.z * b)};
}

// y = x / max(|x|, eps) and its torch backward: below eps the divisor is the constant eps
__device__ __forceinline__ V3 normalize(V3 x, float& n) { n = sqrtf((x.x * x.x + x.y * x.y) + x.z * x.z); return x / fmaxf(n, EPS); }
__device__ __forceinline__ V3 normalize_bwd(V3 y, float n, V3 gy) { return n < EPS ? gy / EPS : (gy - y * dot(y, gy)) / n; }

// What the backward keeps of one pixel's normal: the four one-sided differences (zero where the neighbour lies outside the image, on all
// four borders, no wrap), the unit cross products, their norms, the sum and the result.
struct Normal {
    V3 v0, v2, v4, v6;          // V - V(right), V - V(below), V - V(left), V - V(above)
    V3 y[4]; float n[4];        // normalize(2x0, 4x2, 6x4, 0x6)
    float ns; V3 out;           // |sum|, normalize(sum)
    bool has_r, has_d, has_l, has_u;
};

template <class At>
__device__ __forceinline__ void normal_at(At at, const Rays& t, int i, int j, int H, int W, Normal& f)
{
    f.has_r = j + 1 < W; f.has_d = i + 1 < H; f.has_l = j >= 1; f.has_u = i >= 1;
    const V3 rc = ray(t, i, j);
    const float dc = at(0, 0);
    f.v0 = f.has_r ? edge(rc, dc, ray(t, i, j + 1), at(0, 1)) : zero3();
    f.v2 = f.has_d ? edge(rc, dc, ray(t, i + 1, j), at(1, 0)) : zero3();
    f.v4 = f.has_l ? edge(rc, dc, ray(t, i, j - 1), at(0, -1)) : zero3();
    f.v6 = f.has_u ? edge(rc, dc, ray(t, i - 1, j), at(-1, 0)) : zero3();
    f.y[0] = normalize(cross(f.v2, f.v0), f.n[0]);
    f.y[1] = normalize(cross(f.v4, f.v2), f.n[1]);
    f.y[2] = normalize(cross(f.v6, f.v4), f.n[2]);
    f.y[3] = normalize(cross(f.v0, f.v6), f.n[3]);
    f.out = normalize(((f.y[0] + f.y[1]) + f.y[2]) + f.y[3], f.ns);
}

// a = dL/d(normal) of the pixel -> what the five depths it read receive: d[0] the pixel itself, d[1..4] its right, lower, left and upper
// neighbour (0 where that neighbour is outside the image)
__device__ __forceinline__ void normal_bwd(const Normal& f, const Rays& t, int i, int j, V3 a, float (&d)[5])
{
    const V3 gs = normalize_bwd(f.out, f.ns, a);
    const V3 g20 = normalize_bwd(f.y[0], f.n[0], gs), g42 = normalize_bwd(f.y[1], f.n[1], gs);
    const V3 g64 = normalize_bwd(f.y[2], f.n[2], gs), g06 = normalize_bwd(f.y[3], f.n[3], gs);
    // c = a x b: dL/da = b x g, dL/db = g x a
    const V3 g0 = cross(g20, f.v2) + cross(f.v6, g06);
    const V3 g2 = cross(f.v0, g20) + cross(g42, f.v4);
    const V3 g4 = cross(f.v2, g42) + cross(g64, f.v6);
    const V3 g6 = cross(f.v4, g64) + cross(g06, f.v0);
    V3 self = zero3();
    d[1] = d[2] = d[3] = d[4] = 0.0f;
    if (f.has_r) { self = self + g0; d[1] = -dot(ray(t, i, j + 1), g0); }
    if (f.has_d) { self = self + g2; d[2] = -dot(ray(t, i + 1, j), g2); }
    if (f.has_l) { self = self + g4; d[3] = -dot(ray(t, i, j - 1), g4); }
    if (f.has_u) { self = self + g6; d[4] = -dot(ray(t, i - 1, j), g6); }
    d[0] = dot(ray(t, i, j), self);
}

// imgrad: the 3x3 Sobel cross-correlations with zero padding (`at` returns 0 outside the image); fx = [[1,0,-1],[2,0,-2],[1,0,-1]],
// fy = [[1,2,1],[0,0,0],[-1,-2,-1]].  Differences of neighbours first: they are (nearly) exact on a smooth map.
template <class At>
__device__ __forceinline__ void sobel_at(At at, float& gy, float& gx)
{
    const float a00 = at(-1, -1), a01 = at(-1, 0), a02 = at(-1, 1), a10 = at(0, -1), a12 = at(0, 1), a20 = at(1, -1), a21 = at(1, 0), a22 = at(1, 1);
    gx = ((a00 - a02) + 2.0f * (a10 - a12)) + (a20 - a22);
    gy = ((a00 - a20) + 2.0f * (a01 - a21)) + (a02 - a22);
}
// the transposes: `wy`, `wx` return dL/dgrad_y, dL/dgrad_x at (row + di, column + dj), 0 outside the image
template <class Wy, class Wx>
__device__ __forceinline__ float sobel_bwd_at(Wy wy, Wx wx)
{
    const float ty = ((wy(1, -1) - wy(-1, -1)) + 2.0f * (wy(1, 0) - wy(-1, 0))) + (wy(1, 1) - wy(-1, 1));
    const float tx = ((wx(-1, 1) - wx(-1, -1)) + 2.0f * (wx(0, 1) - wx(0, -1))) + (wx(1, 1) - wx(1, -1));
    return ty + tx;
}

// the mask the losses use: its value, or with `erode` its value where all eight neighbours are non-zero (`at` returns 1 outside the image)
template <class At>
__device__ __forceinline__ float mask_at(At at, bool erode)
{
    const float m = at(0, 0);
    if (!erode) return m;
    const bool all = at(-1, -1) != 0.0f && at(-1, 0) != 0.0f && at(-1, 1) != 0.0f && at(0, -1) != 0.0f && at(0, 1) != 0.0f &&
                     at(1, -1) != 0.0f && at(1, 0) != 0.0f && at(1, 1) != 0.0f;
    return all ? m : 0.0f;
}

__device__ __forceinline__ float sign0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }      // d|x|/dx, 0 at 0

}  // namespace geo
