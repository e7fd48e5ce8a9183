// gsrast_distort.h -- the depth-distortion map of one finished forward (Mip-NeRF 360's distortion loss, gsplat's render_distort) and its
// gradients (include/gsrast.h: gsrast_distortion_forward / gsrast_distortion_backward).
//
// Over the pairs that contribute (the replay invariant of gsrast_replay.h), with w = alpha T and z = rec1.z, the view-space depth acc_depth
// sums; no background term:
//   distort[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_{i-1} - D_{i-1}),   A_{i-1} = sum_{j<i} w_j,  D_{i-1} = sum_{j<i} w_j z_j
// in list order (every tile list is in non-decreasing z; ties contribute 0 either way).  The quantity does not change under z -> z - z0:
// both kernels work on depths RELATIVE to z0 = the depth of the tile's first listed Gaussian (tile-uniform, read from the list head by
// both, not stored), so that z A - D does not cancel against the scene's distance from the camera.
//
// distort_fwd_kernel (replay_front_to_back) keeps A, D and the running sum per lane.  Every pixel inside the image is written: the map (0 with
// fewer than two contributors) and the moments [2][H][W] = (A_N, D_N), relative to z0, which the backward cannot recover going back to front.
//
// distort_bwd_kernel (replay_back_to_front) takes g[p] = dL/ddistort.  Per lane the suffix sums over the contributors behind the pair:
// SA = sum w, SD = sum w z, SG = sum G w.  Per pair
//   A_{i-1} = A_N - SA - w     D_{i-1} = D_N - SD - w z
//   dL/dz   = 2 g w (A_{i-1} - SA)
//   G       = dL/dw = 2 g (z (A_{i-1} - SA) + SD - D_{i-1})
//   dL/dalpha = T G - SG / (1 - alpha)
// dL/dalpha goes to floats 0-5 of the Gaussian's record as the walker describes; dL/dz is the walker's value 6 and is ADDED to float 9, where
// the per-Gaussian backward reads dL/d(view-space z) under GSRAST_RENDER_AUX.
//
// Resources (gfx950, tools/kernel_resources.sh distort_; scratch 0 in every instantiation), exp_mode 0 | 1 | 2:
//   distort_fwd_kernel:  VGPR 32 | 32 | 32,  LDS 8192 B
//   distort_bwd_kernel:  VGPR 51 | 51 | 50,  LDS 4352 B
// Both are far from the limits of eight waves per SIMD (64 VGPRs, 20 KiB of LDS per workgroup).
#pragma once
#include "gsrast_common.h"
#include "gsrast_replay.h"

namespace gsrast {

// The tile's depth origin: the first listed Gaussian's (uniform; both directions read the same entry)
__device__ __forceinline__ float distort_z0(const ReplayPixel& p, const uint32_t* __restrict__ point_list, const float4* __restrict__ rec1)
{
    return p.range.y != p.range.x ? rec1[(size_t)REC_STRIDE * point_list[p.range.x]].z : 0.0f;
}

template <int EXPMODE>
__global__ void __launch_bounds__(256)
distort_fwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                   const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                   const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                   float* __restrict__ distort_map /* [H][W] */, float* __restrict__ moments /* [2][H][W]: A_N, D_N (relative to z0) */)
{
    ReplayPixel p;
    if (!replay_pixel(p, ranges, W, H, gx, ntiles, n_contrib, tile_max)) return;
    const float z0 = distort_z0(p, point_list, rec1);
    float A = 0.0f, D = 0.0f, dist = 0.0f;
    replay_front_to_back<EXPMODE>(p, point_list, rec0, rec1, [&](float w, const float4& b) {
        const float zr = b.z - z0;
        dist = __builtin_fmaf(w, __builtin_fmaf(zr, A, -D), dist);      // w (z A_{i-1} - D_{i-1})
        A += w;
        D = __builtin_fmaf(w, zr, D);
    });
    if (p.inside) {
        const size_t plane = (size_t)W * H;
        distort_map[p.pid] = 2.0f * dist;
        moments[p.pid] = A; moments[plane + p.pid] = D;
    }
}

template <int EXPMODE>
__global__ void __launch_bounds__(256)
distort_bwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                   const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                   const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                   const float* __restrict__ moments /* [2][H][W] */, const float* __restrict__ dL_ddistort /* [H][W] */,
                   float* __restrict__ grec /* [P][GREC]: floats 0-5 and 9 are added to */)
{
#pragma clang fp contract(fast)
    constexpr int AS = 8;                         // accumulators per staged instance: six geometric sums, dL/dz, one spare
    ReplayPixel p;
    if (!replay_pixel(p, ranges, W, H, gx, ntiles, n_contrib, tile_max)) return;
    const size_t plane = (size_t)W * H;
    const float g2 = p.inside ? 2.0f * dL_ddistort[p.pid] : 0.0f;        // 2 dL/ddistort of the pixel
    const float AN = p.inside ? moments[p.pid] : 0.0f, DN = p.inside ? moments[plane + p.pid] : 0.0f;
    float SA = 0.0f, SD = 0.0f, SG = 0.0f;                     // sums over the contributors behind the current one
    const float z0 = distort_z0(p, point_list, rec1);
    replay_back_to_front<EXPMODE, AS>(p, point_list, rec0, rec1, final_T, grec,
        [&](const ReplayBackHit& h, float& dz) {
            const float zr = h.b.z - z0;
            const float wz = h.w * zr;
            const float dA = (AN - SA - h.w) - SA;             // A_{i-1} - SA
            const float Dp = DN - SD - wz;                     // D_{i-1}
            const float Gw = g2 * (zr * dA + (SD - Dp));       // dL/dw
            const float dL_dalpha = h.T * Gw - SG * h.rcp1ma;
            dz = g2 * h.w * dA;
            SA += h.w; SD += wz; SG += Gw * h.w;
            return dL_dalpha;
        },
        [&](size_t gid, uint32_t qv, float v) { if (qv == 6u) atomicAdd(grec + gid * GREC + 9u, v); });
}

} // namespace gsrast
