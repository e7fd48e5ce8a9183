// gsrast_contrib.h -- per-Gaussian blend-weight statistics of one finished forward (include/gsrast.h: gsrast_contrib_stats).
//
// Contribution is the replay invariant of gsrast_replay.h; the weight of a contributing pair is w = alpha T.  m_p = pixel_weights[p] clamped to
// [0, 1] (1 without weights); a pixel with m_p = 0 counts in no column.  One row per Gaussian:  [ sum_p m_p w,  max over pixels with
// m_p > 0 of w,  number of pixels with m_p > 0 it contributes to,  number of those pixels whose largest w is this Gaussian's (first in list
// order on a tie) ].
//
// contrib_blend_kernel walks front to back with a body of its own, line for line replay_front_to_back's, in which a pixel with m_p = 0 looks
// at no list position, every lane takes part in the per-pair reductions below and a batch is retired behind a third barrier: written as a
// visitor of that walker it measured 1 - 2 % slower on the MI355X (DESIGN_LOG.md), so a change to the walker's tests or arithmetic has to be
// made here as well.
//
// Accumulation is integer and commutative from the first cross-wave step on, so the result is bit-identical from run to run:
//   * per surviving (wave, staged slot): the masked sum m w by a fixed-order DPP reduction (wave_sum_to_lane63), the maximum of w by the same
//     tree, the number of updating lanes by a scalar popcount -- stored by lane 63 into the WAVE'S OWN row of three LDS arrays (a wave meets a
//     slot once per batch: plain stores, no LDS atomics, no cross-wave ordering);
//   * when the batch is retired, the thread that staged slot t converts each wave's partial sum to fixed point (units of 2^-36: a partial is
//     at most 64, its conversion drops less than one unit; a Gaussian that covers every pixel of a 2^26-pixel image sums to less than 2^62)
//     and issues, only for a slot some wave updated, one 64-bit integer atomicAdd, one 32-bit atomicMax on the float's bits (weights are
//     non-negative: their bit patterns order like their values) and one 32-bit atomicAdd of the count;
//   * each lane keeps its pixel's best (w, Gaussian) in registers and adds 1 to that Gaussian's top count at the end.
// contrib_finish_kernel turns the 20 bytes of accumulators per Gaussian into the float32 row and clears them.
//
// Resources (gfx950, tools/kernel_resources.sh contrib_; scratch 0), exp_mode 0 | 1 | 2:
//   contrib_blend_kernel:  VGPR 65 | 65 | 65,  LDS 21504 B  ->  seven waves per SIMD, by the registers (512 / 72) and by LDS (160 KiB / 21504 B) alike
#pragma once
#include "gsrast_common.h"
#include "gsrast_blend.h"

namespace gsrast {

constexpr float CONTRIB_FIX = 68719476736.0f;             // 2^36: fixed-point units per 1.0 of the summed weight
constexpr double CONTRIB_UNFIX = 1.0 / 68719476736.0;

// Maximum over the 64 lanes of a wave of NON-NEGATIVE values; valid in lane 63 only (the tree of wave_sum_to_lane63: a lane without a source
// reads 0, the neutral element here as there).
template <int CTRL>
__device__ __forceinline__ float dpp_max0(float v)
{
    const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
    return fmaxf(v, __int_as_float(t));
}
__device__ __forceinline__ float wave_max0_to_lane63(float v)
{
    v = dpp_max0<0x111>(v); v = dpp_max0<0x112>(v); v = dpp_max0<0x114>(v); v = dpp_max0<0x118>(v);
    v = dpp_max0<0x142>(v); v = dpp_max0<0x143>(v);
    return v;
}

template <int EXPMODE>
__global__ void __launch_bounds__(256)
contrib_blend_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                     const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                     const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                     const float* __restrict__ pixel_weights /* [H][W] or null = 1 */,
                     unsigned long long* __restrict__ acc_sum, uint32_t* __restrict__ acc_max, uint32_t* __restrict__ acc_cnt, uint32_t* __restrict__ acc_top)
{
    constexpr uint32_t FB = 256, NW = 4;          // instances staged per batch (the forward's), waves
    __shared__ float4 s0[FB];
    __shared__ float4 s1[FB];
    __shared__ uint32_t sid[FB];
    __shared__ float w_sum[NW][FB];               // [wave][staged slot]: valid where w_cnt is non-zero
    __shared__ float w_max[NW][FB];
    __shared__ uint32_t w_cnt[NW][FB];
    const uint32_t tile = xcd_tile(blockIdx.x, ntiles);      // neighbouring tiles share Gaussians: one band of tiles per XCD
    if (tile >= ntiles) return;
    const uint32_t tx = tile % (uint32_t)gx, ty = tile / (uint32_t)gx;
    const uint32_t t = threadIdx.x;
    const unsigned lane = lane_id(), wave = t >> 6;
    const uint32_t bx = (wave & 1u) * 8u, by = (wave >> 1) * 8u;
    const uint32_t px = tx * TILE_X + bx + (lane & 7u), py = ty * TILE_Y + by + (lane >> 3);
    const float sx0 = (float)(tx * TILE_X + bx), sx1 = sx0 + 7.0f;
    const float sy0 = (float)(ty * TILE_Y + by), sy1 = sy0 + 7.0f;
    const bool inside = px < (uint32_t)W && py < (uint32_t)H;
    const float pxf = (float)px, pyf = (float)py;
    const uint2 range = ranges[tile];
    const uint32_t n_all = range.y - range.x, tm = tile_max[tile];
    const uint32_t n = tm < n_all ? tm : n_all;               // list positions >= tile_max were consumed by no pixel
    // the pixel's weight; a pixel with m = 0 (or NaN) is treated like one outside the image
    float mw = 0.0f;
    uint32_t last = 0;
    if (inside) {
        const size_t pid = (size_t)W * py + px;
        mw = pixel_weights ? fminf(fmaxf(pixel_weights[pid], 0.0f), 1.0f) : 1.0f;
        const uint32_t nc = n_contrib[pid];
        last = mw > 0.0f ? (nc < n ? nc : n) : 0u;
    }
    uint32_t wave_last;
    {
        uint32_t m = last;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        wave_last = __builtin_amdgcn_readfirstlane(m);
    }
#pragma unroll
    for (uint32_t w = 0; w < NW; w++) w_cnt[w][t] = 0u;       // (thread t owns column t of the counts between two batches)

    float T = 1.0f, best_w = 0.0f;
    uint32_t best_id = 0xFFFFFFFFu;
    for (uint32_t base = 0; base < n; base += FB) {
        const uint32_t i = base + t;
        uint32_t g = 0xFFFFFFFFu;
        if (i < n) {
            g = point_list[range.x + i];
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g]; sid[t] = g;
        }
        __syncthreads();
        const uint32_t cnt = (n - base) < FB ? (n - base) : FB;
        if (base < wave_last)                                  // (a wave past its block's deepest contributor only helps staging)
#pragma unroll 1
        for (uint32_t r = 0; r < FB / 64u; r++) {
            if (base + r * 64u >= wave_last) break;            // uniform
            const uint32_t slot = r * 64u + lane;
            bool touch = false;
            if (slot < cnt && base + slot < wave_last) {
                const float4 a = s0[slot];
                const float4 b = s1[slot];
                touch = strip_may_touch(a, b.x, b.w, sx0, sx1, sy0, sy1);
            }
            uint64_t mask = __ballot(touch);
            while (mask) {
                const uint32_t j = r * 64u + (uint32_t)__builtin_ctzll(mask);
                mask &= mask - 1;
                const float4 a = s0[j];
                const float4 b = s1[j];
                const uint32_t gj = sid[j];
                const float dx = a.x - pxf, dy = a.y - pyf;
                const float power = gs_power(a.z, a.w, b.x, dx, dy);
                // the forward's nested tests as wave-uniform masks (blend_fwd_cull_body); `alive` there is `position < n_contrib` here
                const uint64_t m_in = __builtin_amdgcn_ballot_w64(base + j < last) & __builtin_amdgcn_ballot_w64(power <= 0.0f) & __builtin_amdgcn_ballot_w64(power >= b.w);
                if (m_in == 0ull) continue;
                float alpha = b.y * gs_exp<EXPMODE, true>(power);
                alpha = alpha < 0.99f ? alpha : 0.99f;
                const float test_T = T * (1.0f - alpha);
                const uint64_t m_contrib = m_in & __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
                const uint64_t m_upd = m_contrib & ~__builtin_amdgcn_ballot_w64(test_T < 0.0001f);
                if (m_upd == 0ull) continue;
                const bool upd = __builtin_amdgcn_inverse_ballot_w64(m_upd);
                const float w = alpha * T;
                const float vs = upd ? mw * w : 0.0f, vm = upd ? w : 0.0f;
                if (upd) {
                    if (w > best_w) { best_w = w; best_id = gj; }      // strict: the first in list order keeps a tie
                    T = test_T;
                }
                const float S = wave_sum_to_lane63(vs), M = wave_max0_to_lane63(vm);
                if (lane == 63u) { w_sum[wave][j] = S; w_max[wave][j] = M; w_cnt[wave][j] = (uint32_t)__popcll(m_upd); }
            }
        }
        __syncthreads();
        // retire the batch: the thread that staged slot t combines the four waves' values in wave order
        if (g != 0xFFFFFFFFu) {
            unsigned long long fs = 0ull; uint32_t fm = 0u, fc = 0u;
#pragma unroll
            for (uint32_t w = 0; w < NW; w++) {
                const uint32_t c = w_cnt[w][t];
                if (c) {
                    fs += (unsigned long long)(w_sum[w][t] * CONTRIB_FIX);
                    const uint32_t mb = __float_as_uint(w_max[w][t]);
                    fm = mb > fm ? mb : fm; fc += c;
                    w_cnt[w][t] = 0u;
                }
            }
            if (fc) { atomicAdd(acc_sum + g, fs); atomicMax(acc_max + g, fm); atomicAdd(acc_cnt + g, fc); }
        }
        // (the next batch's staging writes s0 / s1 / sid behind the barrier above; its waves write the count columns behind the next one)
    }
    if (best_id != 0xFFFFFFFFu) atomicAdd(acc_top + best_id, 1u);
}

// One lane per Gaussian: accumulators -> [sum, max, count, top] (float32; counts are exact up to 2^24 and rounded above), accumulators cleared.
__global__ void __launch_bounds__(256)
contrib_finish_kernel(int P, unsigned long long* __restrict__ acc_sum, uint32_t* __restrict__ acc_max, uint32_t* __restrict__ acc_cnt, uint32_t* __restrict__ acc_top,
                      float4* __restrict__ stats)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const unsigned long long s = acc_sum[i];
    const uint32_t m = acc_max[i], c = acc_cnt[i], k = acc_top[i];
    stats[i] = make_float4((float)((double)s * CONTRIB_UNFIX), __uint_as_float(m), (float)c, (float)k);
    acc_sum[i] = 0ull; acc_max[i] = 0u; acc_cnt[i] = 0u; acc_top[i] = 0u;
}

} // namespace gsrast
