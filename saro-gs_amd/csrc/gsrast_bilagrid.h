// gsrast_bilagrid.h -- per-camera appearance compensation between the render and the loss: a bilateral grid of 3x4 colour matrices
// (gsplat's lib_bilagrid `slice`; upstream 3DGS's "exposure" is its 1 x 1 x 1 case) and its total-variation regulariser.
// include/gsrast.h (gsrast_bilagrid_*) holds the definition; in short, per pixel (px, py) of a [3][H][W] crop at (x0, y0) of a frame:
//   u = (x0 + px + 0.5) (GW - 1) / full_W,  v likewise,  gray = 0.299 r + 0.587 g + 0.114 b,  t = clamp(gray, 0, 1) (L - 1)
//   A[12] = trilinear interpolation of grid [12][L][GH][GW] at (u, v, t)       (grid_sample: bilinear, border, align_corners)
//   out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3]
// Kernels:
//   bilagrid_fwd_kernel        one lane per pixel; a wave owns 64 consecutive pixels of one row (whole 256-byte runs per channel)
//   bilagrid_bwd_pixel_kernel  the same walk; recomputes the weights and A from grid and image, writes dL/dimage (matrix product + the
//                              guidance term through gray; slope 0 where gray is outside (0, 1), as grid_sample's border clip gives it)
//   bilagrid_bwd_grid_kernel   a GATHER: one workgroup per grid vertex column (gx, gy) and slab; it walks the pixels whose u and v lie
//                              within one cell of the vertex in a fixed order, every lane sums w_x w_y w_t dL/dout_c [r, g, b, 1]_k into
//                              L x 12 registers (static indices), then a fixed tree over the wave (bg_wave_sum) and a fixed sum over the four waves.
//                              ONE writer per element, no floating-point atomics: dL/dgrid is bit-identical from run to run for a given
//                              slab count.  With more than one slab per vertex the partials go to scratch and
//   bilagrid_reduce_kernel     sums them in slab order (fp64, rounded once).
//   bilagrid_tv_kernel         the regulariser's value: ONE workgroup (the call has no scratch to meet in), per-lane fp64 sums in a fixed
//                              stride order, a fixed LDS tree, one float.
//   bilagrid_tv_grad_kernel    its gradient, one lane per grid element, scaled by the upstream scalar.
// A wave's pixels almost always share their xy cell (1080p, 16 x 16 x 8: a cell is 128 x 72 px), so the two pixel kernels stage the wave's
// (at most 3) x 2 vertex columns x L x 12 coefficients in LDS once and interpolate from there; a wave that spans more than two cells in x
// (grids finer than 32 px per cell) reads the grid through the cache instead.  Measured on an MI355X against a build without the stage
// (-DGSRAST_BILAGRID_STAGE=0, same bits out), device events, median of 20, 1920 x 1080: 16 x 16 x 8 forward 0.033 ms staged / 0.254 ms
// plain, pixel backward 0.035 / 0.255; 8 x 8 x 4: 0.027 / 0.190; 64 x 64 x 16 (30 px cells: never staged) 0.28 either way.  96 taps per
// pixel at wave-uniform addresses are bound by the load unit, not by bytes; the stage turns them into LDS broadcasts.
// The library is built with -ffp-contract=off: there is no FMA here.
//
// Resources (build.py's flags + -Rpass-analysis=kernel-resource-usage, gfx950).  Scratch (private segment) and spills are 0 for every
// kernel: the L x 12 accumulators of the gather stay in VGPRs.  LDS: static + dynamic.
//   kernel                          VGPR  AGPR  SGPR  LDS [B]                          scratch  occupancy [waves/SIMD]
//   bilagrid_fwd_kernel               54     0    44  0 + 1152 L (9216 at L = 8)             0  8
//   bilagrid_bwd_pixel_kernel         56     0    44  0 + 1152 L                             0  8
//   bilagrid_bwd_grid_kernel<1>       46     0    66  192                                    0  8
//   bilagrid_bwd_grid_kernel<2>       68     0    70  384                                    0  7
//   bilagrid_bwd_grid_kernel<4>       94     0    74  768                                    0  5
//   bilagrid_bwd_grid_kernel<8>      142     0    82  1536                                   0  3
//   bilagrid_bwd_grid_kernel<16>     238     0    98  3072                                   0  2
//   bilagrid_reduce_kernel             8     0    14  0                                      0  8
//   bilagrid_tv_kernel                56     0    36  24576                                  0  8 (one workgroup of 16 waves)
//   bilagrid_tv_grad_kernel           14     0    21  0                                      0  8
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int BG_THREADS = 256;              // four waves: four rows of 64 pixels in the pixel kernels
constexpr int BG_MAX_G = 64, BG_MAX_L = 16;  // the limits of GW, GH and of L
constexpr int BG_MAX_FRAME = 32768;          // full_W, full_H: (p + 0.5) (G - 1) stays exact in fp32, H x W fits 31 bits
constexpr int BG_MAX_SPLITS = 1024;
constexpr int BG_STAGE_NX = 3;               // vertex columns in x a wave stages (two cells)
#ifndef GSRAST_BILAGRID_STAGE
#define GSRAST_BILAGRID_STAGE 1              // 0 (a variant build: build.py -DGSRAST_BILAGRID_STAGE=0): no wave stages, every tap is a cached load
#endif
constexpr int BG_TV_THREADS = 1024, BG_TV_UNROLL = 4;
constexpr int BG_TV_MAX_N = 2048;            // grids per TV call: N x 12 L GH GW stays below 2^31
constexpr float BG_GRAY_R = 0.299f, BG_GRAY_G = 0.587f, BG_GRAY_B = 0.114f;

struct BgArgs { int GW, GH, L, W, H, x0, y0, full_W, full_H; };

// index coordinate of pixel p (frame coordinates) on an axis of n vertices: one rounding (the product is exact below 2^24)
__device__ __forceinline__ float bg_coord(int p, int full, int n) { return (((float)p + 0.5f) * (float)(n - 1)) / (float)full; }

// the lower vertex of coordinate c on an axis of n vertices and the fraction above it.  c is clamped to [0, n - 2] as a FLOAT before the
// conversion (fmaxf drops a NaN: a float -> int conversion of NaN is undefined, and the compiler may then take every `l == l0` for true),
// so the index is in range whatever c is; a NaN c leaves f NaN.  n = 1: index 0, f = c = 0.
__device__ __forceinline__ int bg_cell(float c, int n, float& f)
{
    const float hi = n > 1 ? (float)(n - 2) : 0.0f;
    const int i = (int)fminf(fmaxf(c, 0.0f), hi);      // (truncation is floor: the operand is >= 0)
    f = c - (float)i;
    return i;
}

// t = clamp(gray, 0, 1) (L - 1) written so that a NaN gray stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float bg_t(float gray, int L)
{
    const float g = gray < 0.0f ? 0.0f : (gray > 1.0f ? 1.0f : gray);
    return g * (float)(L - 1);
}

// the bilinear interpolation in xy of the two slices l0 and l1 for the 12 channels: taps at p[(ch L + l) s_cl + jy s_y + jx s_x]
__device__ __forceinline__ void bg_slices(const float* __restrict__ p, int L, int l0, int l1, size_t s_cl, int s_y, int s_x,
                                          const float wxy[4], float B0[12], float B1[12])
{
#pragma unroll
    for (int ch = 0; ch < 12; ch++) {
        const float* q0 = p + (size_t)(ch * L + l0) * s_cl;
        const float* q1 = p + (size_t)(ch * L + l1) * s_cl;
        B0[ch] = ((wxy[0] * q0[0] + wxy[1] * q0[s_x]) + wxy[2] * q0[s_y]) + wxy[3] * q0[s_y + s_x];
        B1[ch] = ((wxy[0] * q1[0] + wxy[1] * q1[s_x]) + wxy[2] * q1[s_y]) + wxy[3] * q1[s_y + s_x];
    }
}

// What the two pixel kernels share: the lane's pixel, its cell and fractions, and the two slices B0, B1 (from LDS where the wave staged
// its vertex columns, from the grid otherwise).  Every lane of the workgroup calls it (it holds the barrier); -> whether the lane has a pixel.
struct BgPixel { int px, py, l0; float fx, fy, ft, r, g, b, gray; size_t at; };

__device__ __forceinline__ bool bg_pixel_setup(const BgArgs& a, const float* __restrict__ grid, const float* __restrict__ image, float* lds,
                                               BgPixel& P, float B0[12], float B1[12])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px_first = (int)blockIdx.x * 64;
    P.px = px_first + lane;
    P.py = (int)blockIdx.y * 4 + wave;
    const bool row = P.py < a.H, active = row && P.px < a.W;
    // the wave's row and its span of vertex columns (the same for all its lanes)
    const int py = row ? P.py : a.H - 1;
    const int gy0 = bg_cell(bg_coord(a.y0 + py, a.full_H, a.GH), a.GH, P.fy);
    const int px_last = px_first + 63 < a.W ? px_first + 63 : a.W - 1;
    float unused;
    const int gx_lo = bg_cell(bg_coord(a.x0 + px_first, a.full_W, a.GW), a.GW, unused);
    const int gx_hi = bg_cell(bg_coord(a.x0 + px_last, a.full_W, a.GW), a.GW, unused) + 1;      // (GW = 1: one past the axis; clamped where read)
    const bool staged = GSRAST_BILAGRID_STAGE != 0 && gx_hi - gx_lo < BG_STAGE_NX;
    float* const mine = lds + (size_t)wave * (12 * a.L * 2 * BG_STAGE_NX);
    if (staged && row) {
        const int n = 12 * a.L * 2 * BG_STAGE_NX;
        for (int i = lane; i < n; i += 64) {
            const int jx = i % BG_STAGE_NX, rest = i / BG_STAGE_NX, jy = rest & 1, cl = rest >> 1;
            const int gx = gx_lo + jx < a.GW ? gx_lo + jx : a.GW - 1, gy = gy0 + jy < a.GH ? gy0 + jy : a.GH - 1;
            mine[i] = grid[((size_t)cl * a.GH + gy) * a.GW + gx];
        }
    }
    __syncthreads();
    if (!active) return false;
    P.at = (size_t)P.py * a.W + P.px;
    const size_t plane = (size_t)a.H * a.W;
    P.r = image[P.at]; P.g = image[plane + P.at]; P.b = image[2 * plane + P.at];
    P.gray = (BG_GRAY_R * P.r + BG_GRAY_G * P.g) + BG_GRAY_B * P.b;
    const int gx0 = bg_cell(bg_coord(a.x0 + P.px, a.full_W, a.GW), a.GW, P.fx);
    P.l0 = bg_cell(bg_t(P.gray, a.L), a.L, P.ft);
    const int l1 = P.l0 + 1 < a.L ? P.l0 + 1 : P.l0;
    const float wx0 = 1.0f - P.fx, wy0 = 1.0f - P.fy;
    const float wxy[4] = { wx0 * wy0, P.fx * wy0, wx0 * P.fy, P.fx * P.fy };
    if (staged) {
        bg_slices(mine + (gx0 - gx_lo), a.L, P.l0, l1, 2 * BG_STAGE_NX, BG_STAGE_NX, 1, wxy, B0, B1);      // (gx0 - gx_lo is 0 or 1: the tap beside it is staged)
    } else {
        const int s_x = gx0 + 1 < a.GW ? 1 : 0, s_y = gy0 + 1 < a.GH ? a.GW : 0;
        bg_slices(grid + (size_t)gy0 * a.GW + gx0, a.L, P.l0, l1, (size_t)a.GH * a.GW, s_y, s_x, wxy, B0, B1);
    }
    return true;
}

// dynamic LDS of the two pixel kernels: 4 waves x 12 L x 2 x BG_STAGE_NX floats (9 KiB at L = 8, 18 KiB at L = 16)
__host__ __device__ inline size_t bg_pixel_lds(int L) { return (size_t)4 * 12 * L * 2 * BG_STAGE_NX * 4; }

__global__ void __launch_bounds__(BG_THREADS)
bilagrid_fwd_kernel(const BgArgs a, const float* __restrict__ grid, const float* __restrict__ image, float* __restrict__ out)
{
    extern __shared__ float4 bg_lds4[];
    BgPixel P; float B0[12], B1[12];
    if (!bg_pixel_setup(a, grid, image, reinterpret_cast<float*>(bg_lds4), P, B0, B1)) return;
    const float wt0 = 1.0f - P.ft;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float A[4];
#pragma unroll
        for (int k = 0; k < 4; k++) A[k] = wt0 * B0[4 * c + k] + P.ft * B1[4 * c + k];
        out[c * plane + P.at] = ((A[0] * P.r + A[1] * P.g) + A[2] * P.b) + A[3];
    }
}

// dL/dimage_k = sum_c dL/dout_c A[c][k]  +  w_k (L - 1) sum_c dL/dout_c sum_k' (B1 - B0)[c][k'] [r, g, b, 1]_k'   (the second term only for
// 0 < gray < 1 and L > 1: outside, the coordinate is clipped and its slope is 0; a NaN gray compares false and takes the second term: NaN)
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_bwd_pixel_kernel(const BgArgs a, const float* __restrict__ grid, const float* __restrict__ image, const float* __restrict__ dout,
                          float* __restrict__ dimage)
{
    extern __shared__ float4 bg_lds4[];
    BgPixel P; float B0[12], B1[12];
    if (!bg_pixel_setup(a, grid, image, reinterpret_cast<float*>(bg_lds4), P, B0, B1)) return;
    const size_t plane = (size_t)a.H * a.W;
    const float wt0 = 1.0f - P.ft;
    const float go[3] = { dout[P.at], dout[plane + P.at], dout[2 * plane + P.at] };
    float d[3] = { 0.0f, 0.0f, 0.0f }, slope = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float A[4], D[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { A[k] = wt0 * B0[4 * c + k] + P.ft * B1[4 * c + k]; D[k] = B1[4 * c + k] - B0[4 * c + k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] += go[c] * A[k];
        slope += go[c] * (((D[0] * P.r + D[1] * P.g) + D[2] * P.b) + D[3]);
    }
    const bool clipped = P.gray <= 0.0f || P.gray >= 1.0f || a.L == 1;
    if (!clipped) {
        const float dgray = slope * (float)(a.L - 1);
        d[0] += BG_GRAY_R * dgray; d[1] += BG_GRAY_G * dgray; d[2] += BG_GRAY_B * dgray;
    }
    dimage[P.at] = d[0]; dimage[plane + P.at] = d[1]; dimage[2 * plane + P.at] = d[2];
}

// the pixels (crop coordinates, inclusive, clamped to [0, n_px - 1]) whose coordinate can lie within one cell of vertex g: a superset by
// two pixels on each side in exact integer arithmetic; the kernel tests every pixel's own cell
__device__ __forceinline__ void bg_vertex_range(int g, int n, int full, int p0, int n_px, int& lo, int& hi)
{
    if (n == 1) { lo = 0; hi = n_px - 1; return; }
    const long long a = ((long long)(g - 1) * full) / (n - 1) - p0 - 2, b = ((long long)(g + 1) * full) / (n - 1) - p0 + 2;
    lo = a < 0 ? 0 : (int)a;
    hi = b > n_px - 1 ? n_px - 1 : (int)b;
}

// the weight of vertex g for a coordinate in cell i0 with fraction f; false: the vertex is not a corner of the cell
__device__ __forceinline__ bool bg_vertex_weight(int g, int i0, float f, float& w)
{
    if (g == i0) { w = 1.0f - f; return true; }
    if (g == i0 + 1) { w = f; return true; }
    return false;
}

// The sum over the 64 lanes of a wave of N = 3 x 2^k values per lane, N <= 192.  While more than 3 values are left, a step over lane
// distance O HALVES them: the lane without bit O keeps the lower half and takes its partner's lower half, the lane with bit O the upper
// halves -- one shuffle per value kept, 2 N of them in all where a butterfly over every value takes 6 N.  The last 3 values finish as a
// butterfly over the distances left.  In the end v[0 .. 2] of a lane hold the wave's sums of the values base .. base + 2.  Static
// register indices throughout; the tree is fixed, so the sums are the same bits every run.
template <int N, int O>
__device__ __forceinline__ void bg_wave_sum(float* v, int lane, int& base)
{
    if constexpr (O > 0) {
        if constexpr (N > 3) {
            constexpr int h = N / 2;
            const bool upper = (lane & O) != 0;
#pragma unroll
            for (int i = 0; i < h; i++) {
                const float send = upper ? v[i] : v[i + h], keep = upper ? v[i + h] : v[i];
                v[i] = keep + __shfl_xor(send, O, 64);
            }
            if (upper) base += h;
            bg_wave_sum<h, O / 2>(v, lane, base);
        } else {
#pragma unroll
            for (int i = 0; i < N; i++) v[i] += __shfl_xor(v[i], O, 64);
            bg_wave_sum<N, O / 2>(v, lane, base);
        }
    }
}

template <int LT>      // the smallest of 1, 2, 4, 8, 16 that is >= L: the accumulators are LT x 12 registers
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_bwd_grid_kernel(const BgArgs a, int splits, const float* __restrict__ image, const float* __restrict__ dout, float* __restrict__ dst)
{
    __shared__ float s_part[BG_THREADS / 64][LT * 12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx = (int)blockIdx.x % a.GW, gy = (int)blockIdx.x / a.GW, slab = (int)blockIdx.y;
    int px_lo, px_hi, py_lo, py_hi;
    bg_vertex_range(gx, a.GW, a.full_W, a.x0, a.W, px_lo, px_hi);
    bg_vertex_range(gy, a.GH, a.full_H, a.y0, a.H, py_lo, py_hi);
    const int rows = py_hi >= py_lo ? py_hi - py_lo + 1 : 0, per = (rows + splits - 1) / splits;
    const int row_first = py_lo + slab * per, row_end = row_first + per < py_hi + 1 ? row_first + per : py_hi + 1;
    const size_t plane = (size_t)a.H * a.W;
    float acc[LT][12];
#pragma unroll
    for (int l = 0; l < LT; l++)
#pragma unroll
        for (int j = 0; j < 12; j++) acc[l][j] = 0.0f;
    for (int py = row_first + wave; py < row_end; py += BG_THREADS / 64) {
        float fy, wy;
        const int gy0 = bg_cell(bg_coord(a.y0 + py, a.full_H, a.GH), a.GH, fy);
        if (!bg_vertex_weight(gy, gy0, fy, wy)) continue;
        for (int px = px_lo + lane; px <= px_hi; px += 64) {
            float fx, wx, ft;
            const int gx0 = bg_cell(bg_coord(a.x0 + px, a.full_W, a.GW), a.GW, fx);
            if (!bg_vertex_weight(gx, gx0, fx, wx)) continue;
            const size_t at = (size_t)py * a.W + px;
            const float rgb1[4] = { image[at], image[plane + at], image[2 * plane + at], 1.0f };
            const float gray = (BG_GRAY_R * rgb1[0] + BG_GRAY_G * rgb1[1]) + BG_GRAY_B * rgb1[2];
            const int l0 = bg_cell(bg_t(gray, a.L), a.L, ft);
            const float wxy = wx * wy, w0 = 1.0f - ft;
            float val[12];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float g = wxy * dout[c * plane + at];
#pragma unroll
                for (int k = 0; k < 4; k++) val[4 * c + k] = g * rgb1[k];
            }
            // two slices take the pixel; the others are NOT multiplied by a zero weight (0 x NaN would spread a bad pixel over all L)
#pragma unroll
            for (int l = 0; l < LT; l++) {
                if (l == l0) {
#pragma unroll
                    for (int j = 0; j < 12; j++) acc[l][j] += w0 * val[j];
                } else if (l == l0 + 1 && l < a.L) {
#pragma unroll
                    for (int j = 0; j < 12; j++) acc[l][j] += ft * val[j];
                }
            }
        }
    }
    // the wave's sums (bg_wave_sum: the same tree every run), then the four waves in order
    int base = 0;
    bg_wave_sum<LT * 12, 32>(&acc[0][0], lane, base);
#pragma unroll
    for (int i = 0; i < 3; i++) s_part[wave][base + i] = acc[0][i];      // (the lanes of a butterfly group hold and store the same bits)
    __syncthreads();
    const int e = threadIdx.x;
    if (e < LT * 12 && e / 12 < a.L) {
        const int l = e / 12, ch = e % 12;
        const float v = ((s_part[0][e] + s_part[1][e]) + s_part[2][e]) + s_part[3][e];
        const size_t n_grid = (size_t)12 * a.L * a.GH * a.GW;
        dst[(size_t)slab * n_grid + (((size_t)ch * a.L + l) * a.GH + gy) * a.GW + gx] = v;
    }
}

__global__ void __launch_bounds__(256)
bilagrid_reduce_kernel(unsigned n, int splits, const float* __restrict__ partial, float* __restrict__ out)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int k = 0; k < splits; k++) s += (double)partial[(size_t)k * n + e];
    out[e] = (float)s;
}

// ---- total variation: sum over the axes W, H, L of mean((forward difference)^2) over [N][12][L][GH][GW] ----
// the number of element pairs along the axes (0: the axis has one vertex and contributes nothing)
struct BgTvCounts { double inv_x, inv_y, inv_l; };      // 1 / count, or 0

// One workgroup: lane i takes the elements i, i + 1024, ... (coalesced), carrying its (x, y, l) position along by the constant step
// instead of dividing (step = the position of element 1024: {1024 % GW, (1024 / GW) % GH, (1024 / GW / GH) % L}).  Differences (exact), squares
// and sums in fp64.  n < 2^31.
struct BgTvStep { int x, y, l; };

__global__ void __launch_bounds__(BG_TV_THREADS)
bilagrid_tv_kernel(unsigned n, int GW, int GH, int L, BgTvStep step, BgTvCounts cnt, const float* __restrict__ g, float* __restrict__ loss)
{
    __shared__ double s_sum[3][BG_TV_THREADS];
    double sx = 0.0, sy = 0.0, sl = 0.0;
    const unsigned sy_stride = (unsigned)GW, sl_stride = (unsigned)(GW * GH);
    int x = (int)(threadIdx.x % (unsigned)GW), y = (int)((threadIdx.x / (unsigned)GW) % (unsigned)GH), l = (int)((threadIdx.x / sl_stride) % (unsigned)L);
    for (unsigned i0 = threadIdx.x; i0 < n; i0 += BG_TV_THREADS * BG_TV_UNROLL) {
        // the indices of BG_TV_UNROLL elements and of their three forward neighbours first, so that all their loads are in flight together
        // (one workgroup has nothing else to hide the latency with).  A neighbour that does not exist, and an element past the end, reads
        // the element itself: difference 0.
        unsigned iv[BG_TV_UNROLL], ix[BG_TV_UNROLL], iy[BG_TV_UNROLL], il[BG_TV_UNROLL];
#pragma unroll
        for (int u = 0; u < BG_TV_UNROLL; u++) {
            const unsigned i = i0 + (unsigned)u * BG_TV_THREADS;
            const bool in = i < n;
            iv[u] = in ? i : 0u;
            ix[u] = in && x + 1 < GW ? i + 1 : iv[u];
            iy[u] = in && y + 1 < GH ? i + sy_stride : iv[u];
            il[u] = in && l + 1 < L ? i + sl_stride : iv[u];
            x += step.x;
            const int cx = x >= GW ? 1 : 0;
            x -= cx ? GW : 0;
            y += step.y + cx;
            const int cy = y >= GH ? 1 : 0;
            y -= cy ? GH : 0;
            l += step.l + cy;
            l -= l >= L ? L : 0;
        }
        float fv[BG_TV_UNROLL], fx[BG_TV_UNROLL], fy[BG_TV_UNROLL], fl[BG_TV_UNROLL];
#pragma unroll
        for (int u = 0; u < BG_TV_UNROLL; u++) { fv[u] = g[iv[u]]; fx[u] = g[ix[u]]; fy[u] = g[iy[u]]; fl[u] = g[il[u]]; }
#pragma unroll
        for (int u = 0; u < BG_TV_UNROLL; u++) {
            const double v = (double)fv[u], dx = (double)fx[u] - v, dy = (double)fy[u] - v, dl = (double)fl[u] - v;
            sx += dx * dx; sy += dy * dy; sl += dl * dl;
        }
    }
    s_sum[0][threadIdx.x] = sx; s_sum[1][threadIdx.x] = sy; s_sum[2][threadIdx.x] = sl;
    __syncthreads();
    for (int o = BG_TV_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 3; k++) s_sum[k][threadIdx.x] += s_sum[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)((s_sum[0][0] * cnt.inv_x + s_sum[1][0] * cnt.inv_y) + s_sum[2][0] * cnt.inv_l);
}

// d tv / d g[i] = sum over the axes of (2 / count) ((g[i] - g[i - 1]) - (g[i + 1] - g[i])), each difference where the neighbour exists
__global__ void __launch_bounds__(256)
bilagrid_tv_grad_kernel(unsigned n, int GW, int GH, int L, BgTvCounts cnt, const float* __restrict__ g, const float* __restrict__ upstream,
                        float* __restrict__ dg)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned sy_stride = (unsigned)GW, sl_stride = (unsigned)(GW * GH);
    const int x = (int)(i % sy_stride), y = (int)((i / sy_stride) % (unsigned)GH), l = (int)((i / sl_stride) % (unsigned)L);
    const double v = (double)g[i];
    double dx = 0.0, dy = 0.0, dl = 0.0;
    if (x > 0) dx += v - (double)g[i - 1];
    if (x + 1 < GW) dx -= (double)g[i + 1] - v;
    if (y > 0) dy += v - (double)g[i - sy_stride];
    if (y + 1 < GH) dy -= (double)g[i + sy_stride] - v;
    if (l > 0) dl += v - (double)g[i - sl_stride];
    if (l + 1 < L) dl -= (double)g[i + sl_stride] - v;
    const double up = upstream ? (double)*upstream : 1.0;
    dg[i] = (float)(up * (2.0 * ((dx * cnt.inv_x + dy * cnt.inv_y) + dl * cnt.inv_l)));
}

}  // namespace gsrast
