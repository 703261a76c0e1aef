// omni_planefit.hip — the plane-fit normals of a depth map (equi_pers/depth2normal.py), their backward, and the normal loss built on them:
//
//   omni_planefit_normals_f32         depth [B,1,H,W] -> unit normals [B,3,H,W]
//   omni_planefit_normals_grad_f32    d <upstream, normals> / d depth for an upstream [B,3,H,W]
//   omni_planefit_loss_f32            1 - mean_b(sum_b(N(pred) . N(gt) mask) / sum(mask)); no normal map is written
//   omni_planefit_loss_grad_f32       (*grad_out) d loss / d pred
//
// A pixel's normal: over the 25 vertices p = ray * depth at offsets {-4,-2,0,2,4}^2 (zero vectors outside the image, no wrap), M = sum p p^T,
// s = sum p; n = M^-1 s where det M >= 1e-5, n = s otherwise; out = n / max(|n|, 1e-12).  M is taken about the origin, so its condition
// number grows as the angular step shrinks: the reference's float32 solve is off by 1e-2 at 512 x 1024.  Here the vertices are the exact
// double products of the float32 ray and the float32 depth, and the moments, the cofactors, the determinant and the solve are float64.
//
// Forward: a block owns a 16 x 64 tile and stages the vertices of the tile plus a 4-pixel halo in LDS as three double planes (41 KB); a
// thread owns four pixels and reads its 25 taps from there.  The loss stages pred, keeps its four normals in registers, then stages gt in
// the same planes; sums go wave -> block -> one double partial per (item, tile), a final block adds them in a fixed order.  No atomics.
// Backward, two kernels: the adjoint kernel recomputes each centre's fit and writes lambda = M^-1 g_n (g_n: the upstream taken through the
// normalisation) and n to a [B,6,H,W] double map in the workspace (n = 0 in the fallback branch: the centre then sends lambda alone); the
// gather kernel stages that map for an 8 x 64 tile plus halo in LDS, sums lambda (1 - p.n) - n (lambda.p) over the 25 centres whose windows
// hold the pixel and multiplies by the pixel's ray.  Nothing is scattered.  Per-centre arithmetic: fit_at / adjoint_of below, shared by all four entries so that their bits cannot drift apart.
#include "omni_normals.h"
#include "omni_reduce.h"

namespace {

using geo::V3;

constexpr int PT_W = 64, PT_H = 16, P_THREADS = 256, P_ROWS = P_THREADS / PT_W, P_PX = PT_H / P_ROWS;
constexpr int P_REACH = 2, P_STEP = 2, P_HALO = P_REACH * P_STEP;               // 5 taps per axis at dilation 2
constexpr int P_SW = PT_W + 2 * P_HALO, P_SH = PT_H + 2 * P_HALO, P_CELLS = P_SH * P_SW;
constexpr double P_DET_MIN = 1e-5, P_EPS = 1e-12;                              // depth2normal.py:43, F.normalize's eps

// The vertices of rows y0 - 4 .. y0 + 16 + 4, columns x0 - 4 .. x0 + 64 + 4 of one depth plane; zero outside the image (unfold's padding).
__device__ __forceinline__ void stage_vertices(const float* __restrict__ depth, const geo::Rays& rays, int H, int W, int y0, int x0,
                                               double* __restrict__ vx, double* __restrict__ vy, double* __restrict__ vz)
{
    for (int k = threadIdx.x; k < P_CELLS; k += P_THREADS) {
        const int r = k / P_SW, c = k - r * P_SW;
        const int i = y0 - P_HALO + r, j = x0 - P_HALO + c;
        double x = 0.0, y = 0.0, z = 0.0;
        if (i >= 0 && i < H && j >= 0 && j < W) {
            const V3 ry = geo::ray(rays, i, j);
            const double d = (double)depth[(size_t)i * W + j];
            x = (double)ry.x * d; y = (double)ry.y * d; z = (double)ry.z * d;
        }
        vx[k] = x; vy[k] = y; vz[k] = z;
    }
}

struct Fit {
    double a00, a01, a02, a11, a12, a22;       // the adjugate of M (symmetric)
    double det;
    bool solved;                               // det >= 1e-5: n = M^-1 s; otherwise n = s (the reference puts the identity in M's place)
    double n[3], len, o[3];                    // n, |n|, n / max(|n|, eps)
};

// o: the centre's cell in the staged planes.  Taps in row-major order; a NaN vertex makes det NaN, the comparison false and n = s = NaN.
__device__ __forceinline__ void fit_at(const double* __restrict__ vx, const double* __restrict__ vy, const double* __restrict__ vz, int o, Fit& f)
{
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int a = -P_REACH; a <= P_REACH; ++a)
#pragma unroll
        for (int b = -P_REACH; b <= P_REACH; ++b) {
            const int q = o + a * P_STEP * P_SW + b * P_STEP;
            const double x = vx[q], y = vy[q], z = vz[q];
            m00 = fma(x, x, m00); m01 = fma(x, y, m01); m02 = fma(x, z, m02);
            m11 = fma(y, y, m11); m12 = fma(y, z, m12); m22 = fma(z, z, m22);
            s0 += x; s1 += y; s2 += z;
        }
    f.a00 = m11 * m22 - m12 * m12; f.a01 = m02 * m12 - m01 * m22; f.a02 = m01 * m12 - m02 * m11;
    f.a11 = m00 * m22 - m02 * m02; f.a12 = m01 * m02 - m00 * m12; f.a22 = m00 * m11 - m01 * m01;
    f.det = (m00 * f.a00 + m01 * f.a01) + m02 * f.a02;
    f.solved = f.det >= P_DET_MIN;
    if (f.solved) {
        f.n[0] = ((f.a00 * s0 + f.a01 * s1) + f.a02 * s2) / f.det;
        f.n[1] = ((f.a01 * s0 + f.a11 * s1) + f.a12 * s2) / f.det;
        f.n[2] = ((f.a02 * s0 + f.a12 * s1) + f.a22 * s2) / f.det;
    } else {
        f.n[0] = s0; f.n[1] = s1; f.n[2] = s2;
    }
    f.len = sqrt((f.n[0] * f.n[0] + f.n[1] * f.n[1]) + f.n[2] * f.n[2]);
    const double d = fmax(f.len, P_EPS);
    f.o[0] = f.n[0] / d; f.o[1] = f.n[1] / d; f.o[2] = f.n[2] / d;
}

// g = dL/d out of the centre -> lam = M^-1 g_n (g_n in the fallback branch), nn = n (0 in the fallback branch)
__device__ __forceinline__ void adjoint_of(const Fit& f, const double (&g)[3], double (&lam)[3], double (&nn)[3])
{
    double gn[3];
    if (f.len < P_EPS) {                                                       // the divisor is the constant eps there
        gn[0] = g[0] / P_EPS; gn[1] = g[1] / P_EPS; gn[2] = g[2] / P_EPS;
    } else {
        const double og = (f.o[0] * g[0] + f.o[1] * g[1]) + f.o[2] * g[2];
        gn[0] = (g[0] - f.o[0] * og) / f.len; gn[1] = (g[1] - f.o[1] * og) / f.len; gn[2] = (g[2] - f.o[2] * og) / f.len;
    }
    if (f.solved) {
        lam[0] = ((f.a00 * gn[0] + f.a01 * gn[1]) + f.a02 * gn[2]) / f.det;
        lam[1] = ((f.a01 * gn[0] + f.a11 * gn[1]) + f.a12 * gn[2]) / f.det;
        lam[2] = ((f.a02 * gn[0] + f.a12 * gn[1]) + f.a22 * gn[2]) / f.det;
        nn[0] = f.n[0]; nn[1] = f.n[1]; nn[2] = f.n[2];
    } else {
        lam[0] = gn[0]; lam[1] = gn[1]; lam[2] = gn[2];
        nn[0] = nn[1] = nn[2] = 0.0;
    }
}

struct MaskAt {                                                                // accessor of geo::mask_at over global memory: 1 outside the image
    const float* p; int i, j, H, W;
    __device__ __forceinline__ float operator()(int di, int dj) const
    {
        const int y = i + di, x = j + dj;
        return (y >= 0 && y < H && x >= 0 && x < W) ? p[(size_t)y * W + x] : 1.0f;
    }
};

// ------------------------------------------------------------------ the map
__global__ __launch_bounds__(P_THREADS) void planefit_normals_kernel(const float* __restrict__ depth, const float* __restrict__ tab, int H, int W, int tiles_x,
                                                                     float* __restrict__ out)
{
    __shared__ double vx[P_CELLS], vy[P_CELLS], vz[P_CELLS];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * PT_H, x0 = (tile % tiles_x) * PT_W;
    const size_t hw = (size_t)H * W;
    stage_vertices(depth + (size_t)b * hw, geo::rays_of(tab, H, W), H, W, y0, x0, vx, vy, vz);
    __syncthreads();
    const int tx = threadIdx.x & (PT_W - 1), ty = threadIdx.x / PT_W;
#pragma unroll
    for (int k = 0; k < P_PX; ++k) {
        const int r = ty + k * P_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        Fit f;
        fit_at(vx, vy, vz, (r + P_HALO) * P_SW + tx + P_HALO, f);
        float* q = out + (size_t)b * 3 * hw + (size_t)i * W + j;
        q[0] = (float)f.o[0]; q[hw] = (float)f.o[1]; q[2 * hw] = (float)f.o[2];
    }
}

// ------------------------------------------------------------------ the loss
// part: [B][ntiles][2] = sum(N(pred) . N(gt) m), sum(m) of the tile; the normals enter as the float32 values the map entry writes
__global__ __launch_bounds__(P_THREADS) void planefit_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                                  const float* __restrict__ tab, int H, int W, int tiles_x, int erode, double* __restrict__ part)
{
    __shared__ double vx[P_CELLS], vy[P_CELLS], vz[P_CELLS];
    __shared__ double red[2][P_THREADS / 64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * PT_H, x0 = (tile % tiles_x) * PT_W;
    const size_t plane = (size_t)b * H * W;
    const geo::Rays rays = geo::rays_of(tab, H, W);
    const int tx = threadIdx.x & (PT_W - 1), ty = threadIdx.x / PT_W;
    float pn[P_PX][3];
    stage_vertices(pred + plane, rays, H, W, y0, x0, vx, vy, vz);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P_PX; ++k) {
        const int r = ty + k * P_ROWS;
        pn[k][0] = pn[k][1] = pn[k][2] = 0.0f;
        if (y0 + r >= H || x0 + tx >= W) continue;
        Fit f;
        fit_at(vx, vy, vz, (r + P_HALO) * P_SW + tx + P_HALO, f);
        pn[k][0] = (float)f.o[0]; pn[k][1] = (float)f.o[1]; pn[k][2] = (float)f.o[2];
    }
    __syncthreads();
    stage_vertices(gt + plane, rays, H, W, y0, x0, vx, vy, vz);
    __syncthreads();
    double s[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < P_PX; ++k) {
        const int r = ty + k * P_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        Fit f;
        fit_at(vx, vy, vz, (r + P_HALO) * P_SW + tx + P_HALO, f);
        const double m = (double)geo::mask_at(MaskAt{mask + plane, i, j, H, W}, erode != 0);
        const double d = ((double)pn[k][0] * (double)(float)f.o[0] + (double)pn[k][1] * (double)(float)f.o[1]) + (double)pn[k][2] * (double)(float)f.o[2];
        s[0] += d * m;
        s[1] += m;
    }
    block_sum<2>(s, red);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)b * gridDim.x + tile) * 2;
        p[0] = s[0]; p[1] = s[1];
    }
}

// One block.  Per item: thread t adds partials t, t + 256, ... in that order, then the fixed tree.  head[0] = sum(mask) of the batch,
// head[1 + b] = sum(N(pred) . N(gt) mask) of item b.  An empty mask divides 0 by 0: NaN, as geometry_final_kernel.
__global__ __launch_bounds__(P_THREADS) void planefit_final_kernel(const double* __restrict__ part, int B, int ntiles, float* __restrict__ head, float* __restrict__ loss)
{
    __shared__ double red[2][P_THREADS / 64];
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double s[2] = {0.0, 0.0};
        for (int k = threadIdx.x; k < ntiles; k += P_THREADS) {
            const double* p = part + ((size_t)b * ntiles + k) * 2;
            s[0] += p[0]; s[1] += p[1];
        }
        __syncthreads();                                                     // (red is reused per item)
        block_sum<2>(s, red);
        if (threadIdx.x == 0) { head[1 + b] = (float)s[0]; total += s[1]; }
    }
    if (threadIdx.x == 0) {
        const float M = (float)total;
        double sum = 0.0;
        for (int b = 0; b < B; ++b) sum += (double)(head[1 + b] / M);
        head[0] = M;
        *loss = 1.0f - (float)(sum / B);
    }
}

// ------------------------------------------------------------------ backward, stage one: lambda and n per centre
// LOSS: the upstream of a centre is -(*up / B) (m / M) N(gt), formed here; otherwise it is read from up [B,3,H,W].
// map: [B][6][H][W] double = lambda x, y, z, n x, y, z
template <bool LOSS>
__global__ __launch_bounds__(P_THREADS) void planefit_adjoint_kernel(const float* __restrict__ depth, const float* __restrict__ gt, const float* __restrict__ mask,
                                                                     const float* __restrict__ tab, const float* __restrict__ up, const float* __restrict__ head,
                                                                     int B, int H, int W, int tiles_x, int erode, double* __restrict__ map)
{
    __shared__ double vx[P_CELLS], vy[P_CELLS], vz[P_CELLS];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * PT_H, x0 = (tile % tiles_x) * PT_W;
    const size_t hw = (size_t)H * W, plane = (size_t)b * hw;
    const geo::Rays rays = geo::rays_of(tab, H, W);
    const int tx = threadIdx.x & (PT_W - 1), ty = threadIdx.x / PT_W;
    double g[P_PX][3];
    if constexpr (LOSS) {
        stage_vertices(gt + plane, rays, H, W, y0, x0, vx, vy, vz);
        __syncthreads();
        const double c = -((double)*up / (double)B) / (double)head[0];
#pragma unroll
        for (int k = 0; k < P_PX; ++k) {
            const int r = ty + k * P_ROWS, i = y0 + r, j = x0 + tx;
            g[k][0] = g[k][1] = g[k][2] = 0.0;
            if (i >= H || j >= W) continue;
            Fit f;
            fit_at(vx, vy, vz, (r + P_HALO) * P_SW + tx + P_HALO, f);
            const double w = c * (double)geo::mask_at(MaskAt{mask + plane, i, j, H, W}, erode != 0);
            g[k][0] = (double)(float)f.o[0] * w; g[k][1] = (double)(float)f.o[1] * w; g[k][2] = (double)(float)f.o[2] * w;
        }
        __syncthreads();
    }
    stage_vertices(depth + plane, rays, H, W, y0, x0, vx, vy, vz);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P_PX; ++k) {
        const int r = ty + k * P_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const size_t o = (size_t)i * W + j;
        if constexpr (!LOSS) {
            const float* u = up + 3 * plane + o;
            g[k][0] = (double)u[0]; g[k][1] = (double)u[hw]; g[k][2] = (double)u[2 * hw];
        }
        Fit f;
        fit_at(vx, vy, vz, (r + P_HALO) * P_SW + tx + P_HALO, f);
        double lam[3], nn[3];
        adjoint_of(f, g[k], lam, nn);
        double* q = map + 6 * plane + o;
        q[0] = lam[0]; q[hw] = lam[1]; q[2 * hw] = lam[2]; q[3 * hw] = nn[0]; q[4 * hw] = nn[1]; q[5 * hw] = nn[2];
    }
}

// ------------------------------------------------------------------ backward, stage two: the gather
// Pixel k receives lambda_c (1 - p_k . n_c) - n_c (lambda_c . p_k) from every centre c = k + {-4,-2,0,2,4}^2 inside the image (the window
// is symmetric: those are the centres whose windows hold k), in row-major order; d depth_k = ray_k . sum.  A block owns an 8 x 64 tile and
// stages the six planes of the map for the tile plus the 4-pixel halo in LDS (54 KB), zero outside the image: a centre that does not exist
// sends nothing.  Straight from memory every pixel would fetch 25 x 48 bytes through the L2; staged, a block fetches 2.25 x its own.
constexpr int PG_H = 8, PG_SH = PG_H + 2 * P_HALO, PG_CELLS = PG_SH * P_SW, PG_PX = PG_H / P_ROWS;

__global__ __launch_bounds__(P_THREADS) void planefit_gather_kernel(const float* __restrict__ depth, const float* __restrict__ tab, const double* __restrict__ map,
                                                                    int H, int W, int tiles_x, float* __restrict__ grad)
{
    __shared__ double sm[6][PG_CELLS];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * PG_H, x0 = (tile % tiles_x) * PT_W;
    const size_t hw = (size_t)H * W, plane = (size_t)b * hw;
    const geo::Rays rays = geo::rays_of(tab, H, W);
    const double* __restrict__ m = map + 6 * plane;
    for (int k = threadIdx.x; k < PG_CELLS; k += P_THREADS) {
        const int r = k / P_SW, c = k - r * P_SW;
        const int i = y0 - P_HALO + r, j = x0 - P_HALO + c;
        const bool in = i >= 0 && i < H && j >= 0 && j < W;
        const double* q = m + (size_t)(in ? i : 0) * W + (in ? j : 0);
#pragma unroll
        for (int v = 0; v < 6; ++v) sm[v][k] = in ? q[v * hw] : 0.0;
    }
    __syncthreads();
    const int tx = threadIdx.x & (PT_W - 1), ty = threadIdx.x / PT_W;
#pragma unroll
    for (int k = 0; k < PG_PX; ++k) {
        const int r = ty + k * P_ROWS, i = y0 + r, j = x0 + tx;
        if (i >= H || j >= W) continue;
        const V3 ry = geo::ray(rays, i, j);
        const double d = (double)depth[plane + (size_t)i * W + j];
        const double px = (double)ry.x * d, py = (double)ry.y * d, pz = (double)ry.z * d;
        const int o = (r + P_HALO) * P_SW + tx + P_HALO;
        double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
        for (int a = -P_REACH; a <= P_REACH; ++a)
#pragma unroll
            for (int c = -P_REACH; c <= P_REACH; ++c) {
                const int q = o + a * P_STEP * P_SW + c * P_STEP;
                const double lx = sm[0][q], ly = sm[1][q], lz = sm[2][q], nx = sm[3][q], ny = sm[4][q], nz = sm[5][q];
                const double res = 1.0 - ((px * nx + py * ny) + pz * nz), lp = (lx * px + ly * py) + lz * pz;
                sx += lx * res - nx * lp; sy += ly * res - ny * lp; sz += lz * res - nz * lp;
            }
        grad[plane + (size_t)i * W + j] = (float)(((double)ry.x * sx + (double)ry.y * sy) + (double)ry.z * sz);
    }
}

// ------------------------------------------------------------------ host side
constexpr int PF_MAX_B = 65535;                                              // gridDim.y

int pf_check(const char* who, int B, int H, int W)
{
    if (B < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": empty batch");
    if (H < 1 || W < 1) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": H, W >= 1 required, got " + std::to_string(H) + " x " + std::to_string(W));
    if (B > PF_MAX_B || (size_t)H * W >= ((size_t)1 << 31)) OMNI_FAIL(OMNI_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 items or 2^31 pixels per item");
    return OMNI_OK;
}

int pf_aligned(const char* who, const void* workspace)
{
    if ((uintptr_t)workspace & 15) OMNI_FAIL(OMNI_ERR_INVALID, std::string(who) + ": the workspace must be 16-byte aligned");
    return OMNI_OK;
}

inline int tiles_x_of(int W) { return (W + PT_W - 1) / PT_W; }
inline int tiles_of(int H, int W) { return tiles_x_of(W) * ((H + PT_H - 1) / PT_H); }
// workspace: float head[1 + B] (the batch's mask sum, the items' dot sums), padded to 64 bytes | double part[B][ntiles][2], padded to 64 bytes |
// double map[B][6][H][W]
inline size_t head_bytes(int B) { return ((sizeof(float) * (1 + (size_t)B) + 63) / 64) * 64; }
inline size_t part_bytes(int B, int H, int W) { return ((sizeof(double) * 2 * (size_t)B * tiles_of(H, W) + 63) / 64) * 64; }
inline double* map_of(const void* workspace, int B, int H, int W) { return (double*)((char*)workspace + head_bytes(B) + part_bytes(B, H, W)); }

void launch_gather(const float* depth, const float* tab, const double* map, int B, int H, int W, float* grad, hipStream_t s)
{
    hipLaunchKernelGGL(planefit_gather_kernel, dim3(tiles_x_of(W) * ((H + PG_H - 1) / PG_H), B), dim3(P_THREADS), 0, s, depth, tab, map, H, W, tiles_x_of(W), grad);
}

}  // namespace

extern "C" size_t omni_planefit_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1 || B > PF_MAX_B || (size_t)H * W >= ((size_t)1 << 31)) return 0;
    return head_bytes(B) + part_bytes(B, H, W) + sizeof(double) * 6 * (size_t)B * H * W;
}

extern "C" int omni_planefit_normals_f32(const float* depth, const float* ray_tables, int B, int H, int W, float* normals, omni_stream_t stream)
{
    if (!depth || !ray_tables || !normals) OMNI_FAIL(OMNI_ERR_INVALID, "omni_planefit_normals_f32: null device pointer");
    if (const int rc = pf_check("omni_planefit_normals_f32", B, H, W)) return rc;
    hipLaunchKernelGGL(planefit_normals_kernel, dim3(tiles_of(H, W), B), dim3(P_THREADS), 0, (hipStream_t)stream, depth, ray_tables, H, W, tiles_x_of(W), normals);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_planefit_normals_grad_f32(const float* depth, const float* ray_tables, const float* grad_normals, int B, int H, int W, void* workspace,
                                              float* grad_depth, omni_stream_t stream)
{
    if (!depth || !ray_tables || !grad_normals || !workspace || !grad_depth) OMNI_FAIL(OMNI_ERR_INVALID, "omni_planefit_normals_grad_f32: null device pointer");
    if (const int rc = pf_check("omni_planefit_normals_grad_f32", B, H, W)) return rc;
    if (const int rc = pf_aligned("omni_planefit_normals_grad_f32", workspace)) return rc;
    double* map = map_of(workspace, B, H, W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((planefit_adjoint_kernel<false>), dim3(tiles_of(H, W), B), dim3(P_THREADS), 0, s, depth, (const float*)nullptr, (const float*)nullptr, ray_tables,
                       grad_normals, (const float*)nullptr, B, H, W, tiles_x_of(W), 0, map);
    launch_gather(depth, ray_tables, map, B, H, W, grad_depth, s);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_planefit_loss_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W, int erode_mask,
                                      void* workspace, float* loss, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !ray_tables || !workspace || !loss) OMNI_FAIL(OMNI_ERR_INVALID, "omni_planefit_loss_f32: null device pointer");
    if (const int rc = pf_check("omni_planefit_loss_f32", B, H, W)) return rc;
    if (const int rc = pf_aligned("omni_planefit_loss_f32", workspace)) return rc;
    float* head = (float*)workspace;
    double* part = (double*)((char*)workspace + head_bytes(B));
    const int ntiles = tiles_of(H, W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(planefit_loss_kernel, dim3(ntiles, B), dim3(P_THREADS), 0, s, pred, gt, mask, ray_tables, H, W, tiles_x_of(W), erode_mask ? 1 : 0, part);
    hipLaunchKernelGGL(planefit_final_kernel, dim3(1), dim3(P_THREADS), 0, s, (const double*)part, B, ntiles, head, loss);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}

extern "C" int omni_planefit_loss_grad_f32(const float* pred, const float* gt, const float* mask, const float* ray_tables, int B, int H, int W, int erode_mask,
                                           void* workspace, const float* grad_out, float* grad_pred, omni_stream_t stream)
{
    if (!pred || !gt || !mask || !ray_tables || !workspace || !grad_out || !grad_pred) OMNI_FAIL(OMNI_ERR_INVALID, "omni_planefit_loss_grad_f32: null device pointer");
    if (const int rc = pf_check("omni_planefit_loss_grad_f32", B, H, W)) return rc;
    if (const int rc = pf_aligned("omni_planefit_loss_grad_f32", workspace)) return rc;
    double* map = map_of(workspace, B, H, W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((planefit_adjoint_kernel<true>), dim3(tiles_of(H, W), B), dim3(P_THREADS), 0, s, pred, gt, mask, ray_tables, grad_out, (const float*)workspace,
                       B, H, W, tiles_x_of(W), erode_mask ? 1 : 0, map);
    launch_gather(pred, ray_tables, map, B, H, W, grad_pred, s);
    OMNI_HIP(hipGetLastError());
    return OMNI_OK;
}
