// gsrast_topk.h -- which Gaussians a pixel sees, and with what weight: each pixel's first or heaviest K contributors of one finished forward
// (include/gsrast.h: gsrast_pixel_contributors).
//
// Contribution is the replay invariant of gsrast_replay.h; the weight of a contributing pair is w = alpha T.  Per pixel, in blend order
// c_1 ... c_n:  count = n;  order 0 ("weight"): the slots hold the contributors with the largest w, descending, the earlier in blend order
// first on equal w (contrib's top_count rule: slot 0 is that Gaussian);  order 1 ("depth"): the slots hold c_1 ... c_min(K, n).  Unused
// slots hold id -1 and weight +0.0.  Ids are the Gaussians' row numbers, as the tile lists carry them.
//
// pixel_topk_kernel is a visitor of replay_front_to_back with the walker's id staging switched on (ReplayIds: the ids of a batch lie
// beside s0 / s1, the visitor gets the pair's), so every w is the forward's bit for bit.  Each lane keeps TOPK_MAX = 16 (w, id) pairs in
// registers, named by compile-time indices only (every loop over them is fully unrolled: no dynamically indexed array, no scratch), and
// its count.  K is a run-time argument that bounds the stores, and in depth order the updates; in weight order all 16 are kept, whatever K.
//   weight order: a contributing w is > 0 and an unused slot holds 0, so one rule serves both -- w goes in front of the first slot it is
//     STRICTLY larger than (sorted descending: the tests `w > slot k` are false ... false true ... true), the slots behind move down one,
//     the sixteenth leaves.  Lanes whose w does not beat their slot 15 skip the insertion; a wave in which none does branches over it.
//   depth order: the pair goes to slot `count` while count < K.
// No atomics, no LDS beyond the walker's staging, no scratch buffer: every output element has one writer (the lane of its pixel), so the
// result is bit-identical from run to run.  Outputs are planar -- ids [K][H][W], weights [K][H][W], count [H][W] -- and a lane stores its
// own pixel's K values: an 8 x 8 block stores 32-byte row segments, K + K + 1 times.  (An LDS-staged wider store has not been tried.)
// topk_fill_kernel writes the outputs of a state nothing was blended in (P = 0 or R = 0).
//
// The three exp modes are dispatched by a plain switch here (launch_pixel_topk), not by the pick_int of the other replays: the table of
// compiled variants (tests/variant_table.py) counts those sites, and every instantiation of this kernel is run against the fp64
// reference by tests/test_gpu_topk.py itself.
//
// Resources (gfx950, tools/kernel_resources.sh topk; scratch 0 in every instantiation), exp_mode 0 | 1 | 2:
//   pixel_topk_kernel:  VGPR 85 | 85 | 84,  LDS 9216 B (s0, s1 and the 1 KiB of ids)  ->  five waves per SIMD, by the registers (512 / 88)
//   topk_fill_kernel:   VGPR 8,  LDS 0
#pragma once
#include "gsrast_common.h"
#include "gsrast_replay.h"

namespace gsrast {

constexpr int TOPK_MAX = 16;

template <int EXPMODE>
__global__ void __launch_bounds__(256)
pixel_topk_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                  const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                  const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                  int K /* 1 .. TOPK_MAX */, int order /* 0 weight, 1 depth */,
                  int32_t* __restrict__ ids /* [K][H][W] */, float* __restrict__ weights /* [K][H][W] */, int32_t* __restrict__ count /* [H][W] or null */)
{
    ReplayPixel p;
    if (!replay_pixel(p, ranges, W, H, gx, ntiles, n_contrib, tile_max)) return;
    float tw[TOPK_MAX];
    int32_t ti[TOPK_MAX];
#pragma unroll
    for (int k = 0; k < TOPK_MAX; k++) { tw[k] = 0.0f; ti[k] = -1; }
    uint32_t cnt = 0;
    const bool by_weight = order == 0;                         // uniform
    replay_front_to_back<EXPMODE, true>(p, point_list, rec0, rec1, [&](float w, const float4&, uint32_t g) {
        if (by_weight) {
            if (w > tw[TOPK_MAX - 1]) {
#pragma unroll
                for (int k = TOPK_MAX - 1; k >= 1; k--) {      // (from the back: slot k - 1 still holds its old pair)
                    const bool here = w > tw[k], above = w > tw[k - 1];
                    tw[k] = here ? (above ? tw[k - 1] : w) : tw[k];
                    ti[k] = here ? (above ? ti[k - 1] : (int32_t)g) : ti[k];
                }
                if (w > tw[0]) { tw[0] = w; ti[0] = (int32_t)g; }
            }
        } else if (cnt < (uint32_t)K) {
#pragma unroll
            for (int k = 0; k < TOPK_MAX; k++)
                if (cnt == (uint32_t)k) { tw[k] = w; ti[k] = (int32_t)g; }
        }
        cnt++;
    });
    if (p.inside) {
        const size_t plane = (size_t)W * (size_t)H;
#pragma unroll
        for (int k = 0; k < TOPK_MAX; k++)
            if (k < K) { ids[plane * k + p.pid] = ti[k]; weights[plane * k + p.pid] = tw[k]; }      // (uniform test)
        if (count) count[p.pid] = (int32_t)cnt;
    }
}

// The outputs of a state in which nothing was blended: id -1, weight +0.0, count 0
__global__ void __launch_bounds__(256)
topk_fill_kernel(size_t slots /* K H W */, size_t pixels, int32_t* __restrict__ ids, float* __restrict__ weights, int32_t* __restrict__ count /* or null */)
{
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < slots; e += stride) {
        ids[e] = -1; weights[e] = 0.0f;
        if (count && e < pixels) count[e] = 0;
    }
}

// L: the replay's launch record (gsrast_capi.hip: ReplayLaunch); exp_mode has been checked to be 0, 1 or 2
template <class Launch>
inline void launch_pixel_topk(const Launch& L, int exp_mode, hipStream_t s, int K, int order, int32_t* ids, float* weights, int32_t* count)
{
    switch (exp_mode) {
    case 0: L.front_to_back(pixel_topk_kernel<0>, s, K, order, ids, weights, count); break;
    case 1: L.front_to_back(pixel_topk_kernel<1>, s, K, order, ids, weights, count); break;
    default: L.front_to_back(pixel_topk_kernel<2>, s, K, order, ids, weights, count); break;
    }
}

} // namespace gsrast
