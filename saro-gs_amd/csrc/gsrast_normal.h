// gsrast_normal.h -- normal consistency (2DGS, gsplat's 2DGS trainer, GOF, RaDe-GS, PGSR): the agreement between the alpha-blended Gaussian
// normals and the normals of the rendered depth surface.  include/gsrast.h (gsrast_gaussian_normals_*, gsrast_depth_normal_*,
// gsrast_normal_loss_*) holds the definitions; in short
//   per Gaussian:  k = argmin(scales) (a tie: the lowest index),  n = +-(column k of R(q / |q|)) rotated into view space, the sign that
//                  faces the camera (n . p_view <= 0);  |q| = 0 or a non-finite q: n = 0
//   per pixel:     u_x = ((2x + 1) / W - 1) tanfovx,  v_y likewise,  P(x, y) = d(x, y) (u_x, v_y, 1)
//                  a = P(x, y+1) - P(x, y-1),  b = P(x+1, y) - P(x-1, y),  c = a x b,  n = c / |c|      (a fronto-parallel plane: (0, 0, -1))
//                  n = 0, with a zero gradient, on the one-pixel border, where one of the four depths is not > 0 (an uncovered pixel, a
//                  NaN), and where c . c < 1e-24
//   the loss:      L = (1 / (H W)) sum_p (1 - w_p <N_p, n_p>),  N the rendered normal map as given, w a weight without a gradient
// The last two rules of the pixel normal are DEVIATIONS from gsplat's depth_to_normal (a torch composition: slices, cross, F.normalize,
// zero padding), which divides by max(|c|, 1e-12) and has no coverage rule: there a hole's edge gets the normal of a cliff down to depth 0,
// and a degenerate stencil a tiny non-unit vector with a gradient of 1e12 per unit.
//
// Kernels:
//   gaussian_normals_fwd_kernel / _bwd_kernel  one lane per Gaussian; the backward recomputes the forward from its inputs and writes
//                              dL/drotations through q / |q| (the argmin and the sign are piecewise constant: no other gradient exists).
//   depth_normal_fwd_kernel    one workgroup per NM_TW x NM_TH pixel tile: the depths with a halo of 1 staged in LDS once, then a wave per row.
//   depth_normal_bwd_kernel    dL/dd(q) is a GATHER over the four pixels whose stencil contains q -- (x, y+-1) and (x+-1, y) --, their cross
//                              products recomputed from the depths of the radius-2 diamond around q (a halo of 2 in LDS); ray(q) factors
//                              out:  dL/dd(q) = ray(q) . (dL/da(x, y-1) - dL/da(x, y+1) + dL/db(x-1, y) - dL/db(x+1, y)).
//   normal_loss_fwd_kernel     the forward's tile with N and w read beside it; the [3][H][W] normals stay in registers; per-lane fp64 sums, a
//                              fixed tree over the wave, the four waves in order: ONE fp64 partial per workgroup, then
//   normal_loss_reduce_kernel  one workgroup sums the partials (lane i: i, i + 256, ... in that order; a fixed tree) and scales by 1 / (H W).
//   normal_loss_bwd_kernel     saves nothing: dL/dN_p = -(upstream / (H W)) w_p n_p pointwise, and dL/dd by the gather above with
//                              g_p = -(upstream / (H W)) w_p N_p formed on the fly.
// One writer per element everywhere and no atomics: every value and gradient is bit-identical from run to run.
// nm_stencil / nm_vjp / nm_gather (the ray, the stencil, the normalisation with its validity rule, the gather) are the one set of device
// functions under depth_normal_* and normal_loss_*.
//
// Arithmetic: the inputs are fp32, the expressions are evaluated in fp64 and every output is rounded ONCE.  c is the cross product of two
// differences of neighbouring surface points: in fp32 its relative error is that of d(x+1) - d(x-1), unbounded on a smooth surface, and on
// a 3 x 3 image there is one pixel to be wrong at.  One sqrt and one division per stencil.  Measured on an MI355X (tools/normal_overhead.py,
// device events, median of 20, 1352 x 1014 / 1920 x 1080, 90 % of the pixels with a normal): depth_normal forward 0.014 / 0.016 ms, backward
// 0.035 / 0.042; loss forward (both launches) 0.018 / 0.021 ms = 1.5 / 2.0 TB/s of its 20 B per pixel, loss backward 0.045 / 0.054 ms = 1.1 /
// 1.4 TB/s of its 36 B per pixel (dL/dN alone 0.018 / 0.021, dL/dd alone 0.039 / 0.047: the gather's four stencils are the cost, not the
// bytes); gaussian_normals forward 0.012 / 0.026 ms at 1 M / 3 M rows (4.4 / 6.1 TB/s of its 52 B per row), backward 0.015 / 0.034.
//
// Tile: a wave owns 64 consecutive pixels of a row (whole 256-byte runs, as gsrast_bilagrid.h), four waves take the rows of the tile in
// turn.  The halo rows are read again by the tiles above and below: NM_TH = 16 reads (16 + 2) / 16 = 1.125 x the depth plane forward and
// (16 + 4) / 16 = 1.25 x in the gather (NM_TH = 4, one row per wave, would read 1.5 x and 2 x; NM_TH = 32 saves 6 % / 11 % of ONE of the
// five to eight planes a call moves and halves the workgroups: 68 x 30 = 2040 at 1920 x 1080 with 16, eight per CU).  The two halo columns
// of a row are its lanes 0 .. 2 HALO - 1's second load.  Out-of-image taps are staged as 0.0 = "not > 0": the border rule is the coverage rule.
//
// Resources (build.py's flags + -Rpass-analysis=kernel-resource-usage, gfx950).  Scratch (private segment) and spills are 0 for every kernel.
//   kernel                          VGPR  AGPR  SGPR  LDS [B]   scratch  occupancy [waves/SIMD]
//   gaussian_normals_fwd_kernel       50     0    28  0               0  8
//   gaussian_normals_bwd_kernel       48     0    28  0               0  8
//   depth_normal_fwd_kernel           36     0    38  4752            0  8
//   depth_normal_bwd_kernel           78     0    46  5440            0  6
//   normal_loss_fwd_kernel            42     0    52  4784            0  8
//   normal_loss_reduce_kernel         10     0    17  2048            0  8
//   normal_loss_bwd_kernel            89     0    62  5440            0  5
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int NM_THREADS = 256;               // four waves
constexpr int NM_TW = 64, NM_TH = 16;         // the pixel tile of a workgroup
constexpr int NM_MAX_SIDE = 32768;            // W, H: 2 x + 1 and H x W fit 31 bits
constexpr double NM_MIN_CC = 1e-24;           // c . c below this: no normal (F.normalize's eps, squared)

// sizes and rays of an image: u_x = (2 x + 1) hx - tx  with hx = tanfovx / W
struct NmImage { int W, H; double tx, ty, hx, hy; };
__host__ inline NmImage nm_image(int W, int H, double tanfovx, double tanfovy) { return NmImage{ W, H, tanfovx, tanfovy, tanfovx / (double)W, tanfovy / (double)H }; }
__device__ __forceinline__ double nm_u(const NmImage& im, int x) { return (double)(2 * x + 1) * im.hx - im.tx; }
__device__ __forceinline__ double nm_v(const NmImage& im, int y) { return (double)(2 * y + 1) * im.hy - im.ty; }

template <int HALO> constexpr int nm_tile_floats() { return (NM_TW + 2 * HALO) * (NM_TH + 2 * HALO); }

// The depths of the workgroup's tile and HALO pixels around it -> tile[(NM_TH + 2 HALO)][(NM_TW + 2 HALO)], 0.0 outside the image.
// Every lane of the workgroup calls it (it holds the barrier).
template <int HALO>
__device__ __forceinline__ void nm_stage(const NmImage& im, const float* __restrict__ depth, float* tile)
{
    constexpr int RW = NM_TW + 2 * HALO;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (int)blockIdx.x * NM_TW, y0 = (int)blockIdx.y * NM_TH;
    for (int r = wave; r < NM_TH + 2 * HALO; r += NM_THREADS / 64) {
        const int y = y0 - HALO + r;
        const bool row = y >= 0 && y < im.H;
        const size_t at = (size_t)(row ? y : 0) * im.W;
        const int x = x0 + lane;
        tile[r * RW + HALO + lane] = row && x < im.W ? depth[at + x] : 0.0f;
        if (lane < 2 * HALO) {
            const int col = lane < HALO ? lane : NM_TW + lane, xh = x0 - HALO + col;
            tile[r * RW + col] = row && xh >= 0 && xh < im.W ? depth[at + xh] : 0.0f;
        }
    }
    __syncthreads();
}

// The stencil of pixel (x, y), tile-local (lx, ly) (each may lie one pixel outside the tile where HALO = 2): a, b, c and 1 / |c|.
// false: the pixel has no normal (a tap that is not > 0 -- the border's taps are staged as 0 --, or c . c < NM_MIN_CC).
struct NmStencil { double a[3], b[3], c[3], inv; };

template <int HALO>
__device__ __forceinline__ bool nm_stencil(const NmImage& im, const float* tile, int lx, int ly, int x, int y, NmStencil& s)
{
    constexpr int RW = NM_TW + 2 * HALO;
    const float* t = tile + (ly + HALO) * RW + lx + HALO;
    const float fu = t[-RW], fd = t[RW], fl = t[-1], fr = t[1];
    if (!(fu > 0.0f && fd > 0.0f && fl > 0.0f && fr > 0.0f)) return false;
    const double du = fu, dd = fd, dl = fl, dr = fr;
    const double u0 = nm_u(im, x), um = nm_u(im, x - 1), up = nm_u(im, x + 1), v0 = nm_v(im, y), vm = nm_v(im, y - 1), vp = nm_v(im, y + 1);
    s.a[0] = dd * u0 - du * u0; s.a[1] = dd * vp - du * vm; s.a[2] = dd - du;
    s.b[0] = dr * up - dl * um; s.b[1] = dr * v0 - dl * v0; s.b[2] = dr - dl;
    s.c[0] = s.a[1] * s.b[2] - s.a[2] * s.b[1];
    s.c[1] = s.a[2] * s.b[0] - s.a[0] * s.b[2];
    s.c[2] = s.a[0] * s.b[1] - s.a[1] * s.b[0];
    const double cc = (s.c[0] * s.c[0] + s.c[1] * s.c[1]) + s.c[2] * s.c[2];
    if (cc < NM_MIN_CC) return false;
    s.inv = 1.0 / sqrt(cc);
    return true;
}

// dL/da and dL/db of a stencil from g = dL/dn:  dL/dc = (g - n (n . g)) / |c|,  dL/da = b x dL/dc,  dL/db = dL/dc x a
__device__ __forceinline__ void nm_vjp(const NmStencil& s, const double g[3], double da[3], double db[3])
{
    const double n[3] = { s.c[0] * s.inv, s.c[1] * s.inv, s.c[2] * s.inv };
    const double ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
    const double dc[3] = { (g[0] - n[0] * ng) * s.inv, (g[1] - n[1] * ng) * s.inv, (g[2] - n[2] * ng) * s.inv };
    da[0] = s.b[1] * dc[2] - s.b[2] * dc[1]; da[1] = s.b[2] * dc[0] - s.b[0] * dc[2]; da[2] = s.b[0] * dc[1] - s.b[1] * dc[0];
    db[0] = dc[1] * s.a[2] - dc[2] * s.a[1]; db[1] = dc[2] * s.a[0] - dc[0] * s.a[2]; db[2] = dc[0] * s.a[1] - dc[1] * s.a[0];
}

// dL/dd(q), q = (x, y) = tile-local (lx, ly), from the four pixels whose stencil contains q, in a fixed order.  upstream(px, py, g) gives
// dL/dn of pixel (px, py); it is called for pixels that have a normal only (they are interior: inside the image).  tile: HALO = 2.
template <class G>
__device__ __forceinline__ double nm_gather(const NmImage& im, const float* tile, int lx, int ly, int x, int y, G&& upstream)
{
    double acc[3] = { 0.0, 0.0, 0.0 };
    NmStencil s;
    double g[3], da[3], db[3];
    if (nm_stencil<2>(im, tile, lx, ly - 1, x, y - 1, s)) {      // q is the lower tap of (x, y - 1): + dL/da
        upstream(x, y - 1, g); nm_vjp(s, g, da, db);
        acc[0] += da[0]; acc[1] += da[1]; acc[2] += da[2];
    }
    if (nm_stencil<2>(im, tile, lx, ly + 1, x, y + 1, s)) {      // the upper tap of (x, y + 1): - dL/da
        upstream(x, y + 1, g); nm_vjp(s, g, da, db);
        acc[0] -= da[0]; acc[1] -= da[1]; acc[2] -= da[2];
    }
    if (nm_stencil<2>(im, tile, lx - 1, ly, x - 1, y, s)) {      // the right tap of (x - 1, y): + dL/db
        upstream(x - 1, y, g); nm_vjp(s, g, da, db);
        acc[0] += db[0]; acc[1] += db[1]; acc[2] += db[2];
    }
    if (nm_stencil<2>(im, tile, lx + 1, ly, x + 1, y, s)) {      // the left tap of (x + 1, y): - dL/db
        upstream(x + 1, y, g); nm_vjp(s, g, da, db);
        acc[0] -= db[0]; acc[1] -= db[1]; acc[2] -= db[2];
    }
    return (nm_u(im, x) * acc[0] + nm_v(im, y) * acc[1]) + acc[2];
}

__global__ void __launch_bounds__(NM_THREADS)
depth_normal_fwd_kernel(const NmImage im, const float* __restrict__ depth, float* __restrict__ normals)
{
    __shared__ float tile[nm_tile_floats<1>()];
    nm_stage<1>(im, depth, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * NM_TW + lane;
    if (x >= im.W) return;
    const size_t plane = (size_t)im.H * im.W;
    for (int ly = wave; ly < NM_TH; ly += NM_THREADS / 64) {
        const int y = (int)blockIdx.y * NM_TH + ly;
        if (y >= im.H) break;
        NmStencil s;
        float n[3] = { 0.0f, 0.0f, 0.0f };
        if (nm_stencil<1>(im, tile, lane, ly, x, y, s)) { n[0] = (float)(s.c[0] * s.inv); n[1] = (float)(s.c[1] * s.inv); n[2] = (float)(s.c[2] * s.inv); }
        const size_t at = (size_t)y * im.W + x;
        normals[at] = n[0]; normals[plane + at] = n[1]; normals[2 * plane + at] = n[2];
    }
}

__global__ void __launch_bounds__(NM_THREADS)
depth_normal_bwd_kernel(const NmImage im, const float* __restrict__ depth, const float* __restrict__ dnormals, float* __restrict__ ddepth)
{
    __shared__ float tile[nm_tile_floats<2>()];
    nm_stage<2>(im, depth, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * NM_TW + lane;
    if (x >= im.W) return;
    const size_t plane = (size_t)im.H * im.W;
    for (int ly = wave; ly < NM_TH; ly += NM_THREADS / 64) {
        const int y = (int)blockIdx.y * NM_TH + ly;
        if (y >= im.H) break;
        ddepth[(size_t)y * im.W + x] = (float)nm_gather(im, tile, lane, ly, x, y, [&](int px, int py, double g[3]) {
            const size_t at = (size_t)py * im.W + px;
            g[0] = dnormals[at]; g[1] = dnormals[plane + at]; g[2] = dnormals[2 * plane + at];
        });
    }
}

// the sum of one double per lane over the workgroup, in a fixed order (a butterfly over the wave, then the four waves one after the
// other); every lane calls it; the result is valid in thread 0
__device__ __forceinline__ double nm_block_sum(double v, double* s_wave)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

__global__ void __launch_bounds__(NM_THREADS)
normal_loss_fwd_kernel(const NmImage im, const float* __restrict__ normal_map, const float* __restrict__ depth, const float* __restrict__ weight,
                       double* __restrict__ partial)
{
    __shared__ float tile[nm_tile_floats<1>()];
    __shared__ double s_wave[NM_THREADS / 64];
    nm_stage<1>(im, depth, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * NM_TW + lane;
    const size_t plane = (size_t)im.H * im.W;
    double sum = 0.0;
    if (x < im.W) {
        for (int ly = wave; ly < NM_TH; ly += NM_THREADS / 64) {
            const int y = (int)blockIdx.y * NM_TH + ly;
            if (y >= im.H) break;
            const size_t at = (size_t)y * im.W + x;
            const double N[3] = { normal_map[at], normal_map[plane + at], normal_map[2 * plane + at] };
            const double w = weight ? (double)weight[at] : 1.0;
            NmStencil s;
            double n[3] = { 0.0, 0.0, 0.0 };
            if (nm_stencil<1>(im, tile, lane, ly, x, y, s)) { n[0] = s.c[0] * s.inv; n[1] = s.c[1] * s.inv; n[2] = s.c[2] * s.inv; }
            sum += 1.0 - w * ((N[0] * n[0] + N[1] * n[1]) + N[2] * n[2]);      // (a pixel without a normal counts 1; a NaN in N or w stays a NaN)
        }
    }
    const double total = nm_block_sum(sum, s_wave);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
normal_loss_reduce_kernel(const double* __restrict__ partial, int n, double inv_count, float* __restrict__ loss)
{
    __shared__ double r[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += partial[i];
    r[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) r[threadIdx.x] += r[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(r[0] * inv_count);
}

__global__ void __launch_bounds__(NM_THREADS)
normal_loss_bwd_kernel(const NmImage im, const float* __restrict__ normal_map, const float* __restrict__ depth, const float* __restrict__ weight,
                       const float* __restrict__ upstream, float* __restrict__ dnormal_map, float* __restrict__ ddepth)
{
    __shared__ float tile[nm_tile_floats<2>()];
    nm_stage<2>(im, depth, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * NM_TW + lane;
    if (x >= im.W) return;
    const size_t plane = (size_t)im.H * im.W;
    const double scale = -(double)*upstream / ((double)im.H * (double)im.W);      // d L / d (w <N, n>) of every pixel
    for (int ly = wave; ly < NM_TH; ly += NM_THREADS / 64) {
        const int y = (int)blockIdx.y * NM_TH + ly;
        if (y >= im.H) break;
        const size_t at = (size_t)y * im.W + x;
        if (dnormal_map) {
            NmStencil s;
            float d[3] = { 0.0f, 0.0f, 0.0f };
            if (nm_stencil<2>(im, tile, lane, ly, x, y, s)) {
                const double sw = scale * (weight ? (double)weight[at] : 1.0) * s.inv;
                d[0] = (float)(sw * s.c[0]); d[1] = (float)(sw * s.c[1]); d[2] = (float)(sw * s.c[2]);
            }
            dnormal_map[at] = d[0]; dnormal_map[plane + at] = d[1]; dnormal_map[2 * plane + at] = d[2];
        }
        if (ddepth) {
            ddepth[at] = (float)nm_gather(im, tile, lane, ly, x, y, [&](int px, int py, double g[3]) {
                const size_t p = (size_t)py * im.W + px;
                const double sw = scale * (weight ? (double)weight[p] : 1.0);
                g[0] = sw * (double)normal_map[p]; g[1] = sw * (double)normal_map[plane + p]; g[2] = sw * (double)normal_map[2 * plane + p];
            });
        }
    }
}

// ---- per-Gaussian normals -------------------------------------------------------------------------------------------------------------
// What the two kernels share: the row's k, q / |q| = (r, x, y, z), 1 / |q|, and the sign (+1: column k as it is, -1: negated) that makes the
// view-space normal face the camera.  false: |q| = 0 or a non-finite q (the row's normal and gradient are 0).  V: the viewmatrix, 16 floats
// in the render's transposed storage (p_view = [mean, 1] V).
struct NmGauss { int k; double q[4], inv_len, sign, n[3]; };

__device__ __forceinline__ void nm_column(int k, const double q[4], double col[3])
{
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    if (k == 0)      { col[0] = 1.0 - 2.0 * (y * y + z * z); col[1] = 2.0 * (x * y + r * z); col[2] = 2.0 * (x * z - r * y); }
    else if (k == 1) { col[0] = 2.0 * (x * y - r * z); col[1] = 1.0 - 2.0 * (x * x + z * z); col[2] = 2.0 * (y * z + r * x); }
    else             { col[0] = 2.0 * (x * z + r * y); col[1] = 2.0 * (y * z - r * x); col[2] = 1.0 - 2.0 * (x * x + y * y); }
}

__device__ __forceinline__ bool nm_gauss(int i, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                                         const float* __restrict__ V, NmGauss& g)
{
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const float s0 = scales[i3], s1 = scales[i3 + 1], s2 = scales[i3 + 2];
    g.k = 0;
    float smin = s0;
    if (s1 < smin) { g.k = 1; smin = s1; }
    if (s2 < smin) g.k = 2;
    const float qf[4] = { rotations[i4], rotations[i4 + 1], rotations[i4 + 2], rotations[i4 + 3] };
    const double qq = ((double)qf[0] * qf[0] + (double)qf[1] * qf[1]) + ((double)qf[2] * qf[2] + (double)qf[3] * qf[3]);      // (exact products: no over- or underflow from fp32)
    if (!(isfinite(qf[0]) && isfinite(qf[1]) && isfinite(qf[2]) && isfinite(qf[3])) || qq == 0.0) return false;
    g.inv_len = 1.0 / sqrt(qq);
#pragma unroll
    for (int j = 0; j < 4; j++) g.q[j] = (double)qf[j] * g.inv_len;
    double col[3];
    nm_column(g.k, g.q, col);
    const double m[3] = { means3D[i3], means3D[i3 + 1], means3D[i3 + 2] };
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        g.n[j] = (col[0] * (double)V[j] + col[1] * (double)V[4 + j]) + col[2] * (double)V[8 + j];
        const double p = ((m[0] * (double)V[j] + m[1] * (double)V[4 + j]) + m[2] * (double)V[8 + j]) + (double)V[12 + j];
        dot += g.n[j] * p;
    }
    g.sign = dot > 0.0 ? -1.0 : 1.0;      // (an exact 0, and a NaN mean, leave the column as it is)
    return true;
}

__global__ void __launch_bounds__(256)
gaussian_normals_fwd_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                            const float* __restrict__ V, float* __restrict__ normals)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    NmGauss g;
    float n[3] = { 0.0f, 0.0f, 0.0f };
    if (nm_gauss(i, means3D, scales, rotations, V, g)) { n[0] = (float)(g.sign * g.n[0]); n[1] = (float)(g.sign * g.n[1]); n[2] = (float)(g.sign * g.n[2]); }
    normals[3 * (size_t)i] = n[0]; normals[3 * (size_t)i + 1] = n[1]; normals[3 * (size_t)i + 2] = n[2];
}

__global__ void __launch_bounds__(256)
gaussian_normals_bwd_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                            const float* __restrict__ V, const float* __restrict__ dnormals, float* __restrict__ drotations)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= P) return;
    NmGauss g;
    float d[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (nm_gauss(i, means3D, scales, rotations, V, g)) {
        const double gv[3] = { dnormals[3 * (size_t)i], dnormals[3 * (size_t)i + 1], dnormals[3 * (size_t)i + 2] };
        double G[3];      // dL / d (column k), world space
#pragma unroll
        for (int r = 0; r < 3; r++) G[r] = g.sign * (((double)V[4 * r] * gv[0] + (double)V[4 * r + 1] * gv[1]) + (double)V[4 * r + 2] * gv[2]);
        const double r = g.q[0], x = g.q[1], y = g.q[2], z = g.q[3];
        double dq[4];     // dL / d (q / |q|)
        if (g.k == 0) {
            dq[0] = 2.0 * (z * G[1] - y * G[2]);
            dq[1] = 2.0 * (y * G[1] + z * G[2]);
            dq[2] = 2.0 * ((x * G[1] - r * G[2]) - 2.0 * y * G[0]);
            dq[3] = 2.0 * ((r * G[1] + x * G[2]) - 2.0 * z * G[0]);
        } else if (g.k == 1) {
            dq[0] = 2.0 * (x * G[2] - z * G[0]);
            dq[1] = 2.0 * ((y * G[0] + r * G[2]) - 2.0 * x * G[1]);
            dq[2] = 2.0 * (x * G[0] + z * G[2]);
            dq[3] = 2.0 * ((y * G[2] - r * G[0]) - 2.0 * z * G[1]);
        } else {
            dq[0] = 2.0 * (y * G[0] - x * G[1]);
            dq[1] = 2.0 * ((z * G[0] - r * G[1]) - 2.0 * x * G[2]);
            dq[2] = 2.0 * ((r * G[0] + z * G[1]) - 2.0 * y * G[2]);
            dq[3] = 2.0 * (x * G[0] + y * G[1]);
        }
        const double qd = (g.q[0] * dq[0] + g.q[1] * dq[1]) + (g.q[2] * dq[2] + g.q[3] * dq[3]);
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = (float)((dq[j] - g.q[j] * qd) * g.inv_len);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) drotations[4 * (size_t)i + j] = d[j];
}

}  // namespace gsrast
