// gsrast_filter3d.h -- Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024; its gaussian_model.py): the companion of the render's
// antialiasing (the 2-D screen-space filter).  Functions restated:
//   compute_3D_filter                    the loop over the training cameras: min depth over the cameras that see a row  -> filter3d_sweep_kernel
//   its tail                             rows no camera sees get the largest distance; distance / focal * sqrt(0.2)     -> filter3d_finish_kernel
//   get_scaling_with_3D_filter,
//   get_opacity_with_3D_filter           s_f = sqrt(s^2 + f^2),  o_f = o sqrt(prod s^2 / prod s_f^2)                     -> filter3d_apply_fwd_kernel
//   their autograd                                                                                                      -> filter3d_apply_bwd_kernel
// A camera row is 16 floats: R = viewmatrix[:3,:3] row-major (p_cam = p R + T), T, focal_x, focal_y, W, H.  Per row and camera, in fp32,
// every operation rounded (the library is built with -ffp-contract=off and IEEE division):
//   xc = ((x R00 + y R10) + z R20) + T0, yc, zc likewise;  zz = fmaxf(zc, 0.001);  px = (xc / zz) fx + W / 2,  py = (yc / zz) fy + H / 2
//   seen = zc > near && zz < inf && -(margin W) <= px <= W + margin W && -(margin H) <= py <= H + margin H
//   dist = min over the cameras that see the row of zz;   filter_3D = (seen by any ? dist : max dist over the seen rows) * k
// One lane per row, 256-row workgroups; x, y, z, dist stay in registers across the camera loop; a camera row's address depends on the
// kernel arguments and the loop counter alone, so the 64 B arrive through uniform loads, once per wave.  The maximum is an integer max on
// the bits of positive floats (exact, order-free: gsrast_temporal.h's idiom), the count an integer add, one of each per workgroup of at
// most F3_SWEEP_WGS; no floating-point atomics, one writer per element: bit-identical from run to run and rank to rank.
// The opacity factor is evaluated as (r0 r1) r2 with r_k = s_k / s_f,k: the same number as upstream's sqrt(det1 / det2) without the
// products of three squares, which underflow in fp32 for thin Gaussians (0 / 0 there).
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int F3_RUN = 256;                  // rows per workgroup
constexpr int F3_SWEEP_WGS = 2048;           // the sweep walks the rows in grid strides: at most this many atomic pairs on the two scratch words
constexpr int F3_CAMERA_FLOATS = 16;

// dist [P]: the smallest clamped depth over the cameras that see the row, +inf where none does (the finish launch reads it back from the
// same array).  stats[0]: the bits of the largest finite dist; stats[1]: the number of seen rows.  Both cleared on the stream before.
__global__ void __launch_bounds__(F3_RUN)
filter3d_sweep_kernel(int P, int C, float near, float margin, const float* __restrict__ means3D, const float* __restrict__ table,
                      float* __restrict__ dist, int* __restrict__ stats)
{
    __shared__ int s_max[F3_RUN / 64], s_cnt[F3_RUN / 64];
    int bits = 0, cnt = 0;
    for (size_t i = (size_t)blockIdx.x * F3_RUN + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * F3_RUN) {
        const float x = means3D[3 * i], y = means3D[3 * i + 1], z = means3D[3 * i + 2];
        float d = INFINITY;
        for (int c = 0; c < C; c++) {
            const float* __restrict__ cam = table + (size_t)c * F3_CAMERA_FLOATS;      // (uniform: scalar loads)
            const float zc = ((x * cam[2] + y * cam[5]) + z * cam[8]) + cam[11];
            if (!(zc > near)) continue;      // (not seen whatever px, py are: both divisions skipped, the same bits)
            const float xc = ((x * cam[0] + y * cam[3]) + z * cam[6]) + cam[9];
            const float yc = ((x * cam[1] + y * cam[4]) + z * cam[7]) + cam[10];
            const float zz = fmaxf(zc, 0.001f);
            const float W = cam[14], H = cam[15], mw = margin * W, mh = margin * H;
            const float px = (xc / zz) * cam[12] + W * 0.5f;
            const float py = (yc / zz) * cam[13] + H * 0.5f;
            const bool seen = zz < INFINITY && px >= -mw && px <= W + mw && py >= -mh && py <= H + mh;
            d = seen ? fminf(d, zz) : d;
        }
        dist[i] = d;
        if (d < INFINITY) { const int b = __float_as_int(d); bits = b > bits ? b : bits; cnt++; }      // (d > 0: positive floats order as integers)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_xor(bits, o, 64), n = __shfl_xor(cnt, o, 64);
        bits = b > bits ? b : bits;
        cnt += n;
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = bits; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < F3_RUN / 64; w++) { bits = s_max[w] > bits ? s_max[w] : bits; cnt += s_cnt[w]; }
        if (cnt > 0) {
            if (*reinterpret_cast<volatile int*>(&stats[0]) < bits) atomicMax(&stats[0], bits);      // (the word only grows: a stale read errs on the side of issuing it)
            atomicAdd(&stats[1], cnt);
        }
    }
}

// filter_3D = (seen ? dist : dmax) k, in place over dist; valid (NULL = not wanted) = seen.  No seen row at all: dmax = 0, every value +0.0.
__global__ void __launch_bounds__(F3_RUN)
filter3d_finish_kernel(int P, float k, const int* __restrict__ stats, float* __restrict__ filter_3D, unsigned char* __restrict__ valid)
{
    const size_t i = (size_t)blockIdx.x * F3_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float dmax = stats[1] > 0 ? __int_as_float(stats[0]) : 0.0f;
    const float d = filter_3D[i];
    const bool seen = d < INFINITY;
    filter_3D[i] = (seen ? d : dmax) * k;
    if (valid) valid[i] = seen ? 1 : 0;
}

// what the apply kernels share: s_f, r = s / s_f (1 where s_f == 0) and q = f / s_f (0 there) of one axis
struct F3Axis { float sf, r, q; };
__device__ __forceinline__ F3Axis f3_axis(float s, float f)
{
    F3Axis a;
    a.sf = sqrtf(s * s + f * f);
    const bool zero = a.sf == 0.0f;
    a.r = zero ? 1.0f : s / a.sf;
    a.q = zero ? 0.0f : f / a.sf;
    return a;
}

// scales_f [P][3], opacities_f [P]: one lane per row, the 12-byte rows stored per lane (profiles/project_overhead_stores.json)
__global__ void __launch_bounds__(F3_RUN)
filter3d_apply_fwd_kernel(int P, const float* __restrict__ scales, const float* __restrict__ opacities, const float* __restrict__ filter_3D,
                          float* __restrict__ scales_f, float* __restrict__ opacities_f)
{
    const size_t i = (size_t)blockIdx.x * F3_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float f = filter_3D[i];
    const F3Axis a0 = f3_axis(scales[3 * i], f), a1 = f3_axis(scales[3 * i + 1], f), a2 = f3_axis(scales[3 * i + 2], f);
    scales_f[3 * i] = a0.sf;
    scales_f[3 * i + 1] = a1.sf;
    scales_f[3 * i + 2] = a2.sf;
    opacities_f[i] = opacities[i] * ((a0.r * a1.r) * a2.r);
}

// d s_k = g_s,k r_k + (G prod_{j != k} r_j) (q_k^2 / s_f,k),  G = g_o o;  d o = g_o coef.  Everything recomputed from the three inputs;
// a NULL upstream gradient counts as zero, a NULL output is not written.  No division by s_k: an axis with s_f,k == 0 has q_k = 0 and
// its second term is 0.
__global__ void __launch_bounds__(F3_RUN)
filter3d_apply_bwd_kernel(int P, const float* __restrict__ scales, const float* __restrict__ opacities, const float* __restrict__ filter_3D,
                          const float* __restrict__ d_scales_f, const float* __restrict__ d_opacities_f, float* __restrict__ d_scales,
                          float* __restrict__ d_opacities)
{
    const size_t i = (size_t)blockIdx.x * F3_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float f = filter_3D[i];
    const F3Axis a0 = f3_axis(scales[3 * i], f), a1 = f3_axis(scales[3 * i + 1], f), a2 = f3_axis(scales[3 * i + 2], f);
    const float g_o = d_opacities_f ? d_opacities_f[i] : 0.0f;
    if (d_opacities) d_opacities[i] = g_o * ((a0.r * a1.r) * a2.r);
    if (d_scales) {
        const float G = g_o * opacities[i];
        const float g0 = d_scales_f ? d_scales_f[3 * i] : 0.0f, g1 = d_scales_f ? d_scales_f[3 * i + 1] : 0.0f, g2 = d_scales_f ? d_scales_f[3 * i + 2] : 0.0f;
        const float t0 = a0.sf == 0.0f ? 0.0f : (a0.q * a0.q) / a0.sf;
        const float t1 = a1.sf == 0.0f ? 0.0f : (a1.q * a1.q) / a1.sf;
        const float t2 = a2.sf == 0.0f ? 0.0f : (a2.q * a2.q) / a2.sf;
        d_scales[3 * i] = g0 * a0.r + (G * (a1.r * a2.r)) * t0;
        d_scales[3 * i + 1] = g1 * a1.r + (G * (a0.r * a2.r)) * t1;
        d_scales[3 * i + 2] = g2 * a2.r + (G * (a0.r * a1.r)) * t2;
    }
}

}  // namespace gsrast
