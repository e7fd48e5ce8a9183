// gsrast_features.h -- per-Gaussian feature vectors (1 <= C <= 64 channels) blended with the weights of one finished forward, and the
// gradients of that blend (include/gsrast.h: gsrast_features_forward / gsrast_features_backward).
//
// Over the pairs that contribute (the replay invariant of gsrast_replay.h), with w = alpha T; no background term:
//   feature_map[c][p] = sum_i w_ip f[i][c]                       f: [P][C] row-major, the map: [C][H][W] planar
//
// features_fwd_kernel walks front to back with a body of its own, line for line replay_front_to_back's with the feature rows staged beside
// the records in LDS and CH accumulators per lane: written as a visitor of that walker it measured 1.3 - 2.6 % slower at CH 8, 16 and 32 on
// the MI355X (DESIGN_LOG.md), so a change to the walker's tests or arithmetic has to be made here as well.  Every pixel inside the image is
// written (0 without a contributor).
//
// features_bwd_kernel (replay_back_to_front) takes g[c][p] = dL/dfeature_map: A_c <- alpha f_c + (1 - alpha) A_c behind the pair, and per pair
//   dL/df[i][c] += w g[c][p]                 dL/dalpha = T sum_c g[c][p] (f[i][c] - A_c)
// dL/dalpha goes to floats 0-5 of the Gaussian's record as the walker describes (its value 6 stays 0; floats 6-11 are not touched).  The
// channels' sums go through the same transposing wave reduction eight at a time, lanes 0-7 add the totals into the batch's accumulators
// behind the walker's eight, and the walker's retire step sends each non-zero one to dL_dfeatures.
//
// Channels: the kernels are instantiated for chunks of CH = 4, 8, 16, 32 channels; a call runs passes over [c0, c0 + CH) until C is covered
// (the smallest chunk that holds what is left, 32 at most).  Both directions are additive over chunks: dL/dalpha is a sum over channels, so
// each pass adds its part to the records.  A ragged last chunk is padded with zeros in LDS / registers: no address at or past
// features + P C (or the map's / the gradient's C planes) is formed for a load or a store.
//
// Resources (gfx950, tools/kernel_resources.sh features_; scratch 0 in every instantiation; exp_mode 0 | 1 | 2 agree within 3 VGPRs).  Occupancy in
// waves per SIMD, the smaller of the register file's (512 / VGPRs) and LDS's (160 KiB / workgroup's LDS; a workgroup is one wave per SIMD):
//   features_fwd_kernel  CH =  4 |  8 | 16 | 32:  VGPR 38 | 42 | 73 |  97,  LDS 12288 | 16384 | 24576 | 40960 B  ->  8 | 8 | 6 | 4  (LDS-bound at CH 16 and 32)
//   features_bwd_kernel  CH =  4 |  8 | 16 | 32:  VGPR 54 | 71 | 95 | 140,  LDS  6400 |  8448 | 12544 | 20736 B  ->  8 | 7 | 5 | 3  (register-bound)
// CH = 32 is the widest chunk: 64 channels in one pass would need 2 x 64 registers of per-pixel state in the backward alone (one wave per SIMD, or scratch).
#pragma once
#include "gsrast_common.h"
#include "gsrast_replay.h"

namespace gsrast {

constexpr int FEAT_MAX_C = 64;          // include/gsrast.h: GSRAST_FEATURES_MAX_C

template <int EXPMODE, int CH>
__global__ void __launch_bounds__(256)
features_fwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                    const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                    const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                    const float* __restrict__ features /* [P][C] */, int C, int c0 /* this pass: channels [c0, c0 + CH) */,
                    float* __restrict__ feature_map /* [C][H][W] */)
{
    constexpr uint32_t FB = 256;                  // instances staged per batch (the forward's)
    __shared__ float4 s0[FB];
    __shared__ float4 s1[FB];
    __shared__ __attribute__((aligned(16))) float sf[FB][CH];
    const uint32_t tile = xcd_tile(blockIdx.x, ntiles);
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
    const size_t pid = (size_t)W * py + px;
    uint32_t last = 0;
    if (inside) { const uint32_t nc = n_contrib[pid]; last = nc < n ? nc : n; }
    uint32_t wave_last;
    {
        uint32_t m = last;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        wave_last = __builtin_amdgcn_readfirstlane(m);
    }
    const int cw = (C - c0) < CH ? (C - c0) : CH;             // channels of this pass that exist

    float T = 1.0f;
    float acc[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) acc[k] = 0.0f;
    for (uint32_t base = 0; base < n; base += FB) {
        if (base) __syncthreads();                             // (uniform: the previous batch has been read)
        const uint32_t i = base + t;
        if (i < n) {
            const uint32_t g = point_list[range.x + i];
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g];
        }
        // the feature rows: consecutive lanes take consecutive channels of a row (zeros behind the last channel)
        for (uint32_t e = t; e < FB * (uint32_t)CH; e += 256u) {
            const uint32_t slot = e / (uint32_t)CH, k = e % (uint32_t)CH;
            float v = 0.0f;
            if (base + slot < n && (int)k < cw) v = features[(size_t)point_list[range.x + base + slot] * (size_t)C + (size_t)(c0 + (int)k)];
            sf[slot][k] = v;
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
                if (__builtin_amdgcn_inverse_ballot_w64(m_upd)) {
                    const float w = alpha * T;
#pragma unroll
                    for (int q = 0; q < CH / 4; q++) {
                        const float4 f = *reinterpret_cast<const float4*>(&sf[j][4 * q]);
                        acc[4 * q + 0] = __builtin_fmaf(f.x, w, acc[4 * q + 0]); acc[4 * q + 1] = __builtin_fmaf(f.y, w, acc[4 * q + 1]);
                        acc[4 * q + 2] = __builtin_fmaf(f.z, w, acc[4 * q + 2]); acc[4 * q + 3] = __builtin_fmaf(f.w, w, acc[4 * q + 3]);
                    }
                    T = test_T;
                }
            }
        }
    }
    if (inside) {
        const size_t plane = (size_t)W * H;
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (k < cw) feature_map[(size_t)(c0 + k) * plane + pid] = acc[k];
    }
}

template <int EXPMODE, int CH>
__global__ void __launch_bounds__(256)
features_bwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                    const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                    const float* __restrict__ features /* [P][C] */, int C, int c0 /* this pass: channels [c0, c0 + CH) */,
                    const float* __restrict__ dL_dmap /* [C][H][W] */,
                    float* __restrict__ grec /* [P][GREC]: floats 0-5 are added to */, float* __restrict__ dL_dfeatures /* [P][C]: added to */)
{
#pragma clang fp contract(fast)
    constexpr uint32_t BATCH = 64;                // instances staged per batch (the walker's)
    constexpr int AS = CH + 8;                    // accumulators per staged instance: the walker's eight, CH channels
    __shared__ __attribute__((aligned(16))) float sf[BATCH][CH];
    ReplayPixel p;
    if (!replay_pixel(p, ranges, W, H, gx, ntiles, n_contrib, tile_max)) return;
    const size_t plane = (size_t)W * H;
    const int cw = (C - c0) < CH ? (C - c0) : CH;             // channels of this pass that exist
    float gp[CH], A[CH];                                       // dL/dfeature_map of the pixel; the blend behind the current contributor
#pragma unroll
    for (int k = 0; k < CH; k++) { gp[k] = (p.inside && k < cw) ? dL_dmap[(size_t)(c0 + k) * plane + p.pid] : 0.0f; A[k] = 0.0f; }
    replay_back_to_front<EXPMODE, AS>(p, point_list, rec0, rec1, final_T, grec,
        [&](const ReplayBackHit& h, float&) {
            const float om = 1.0f - h.alpha;
            float dL_dalpha = 0.f;
#pragma unroll
            for (int q4 = 0; q4 < CH / 4; q4++) {
                const float4 f = *reinterpret_cast<const float4*>(&sf[h.j][4 * q4]);
                const float fk[4] = { f.x, f.y, f.z, f.w };
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int k = 4 * q4 + i;
                    dL_dalpha += (fk[i] - A[k]) * gp[k];
                    A[k] = h.alpha * fk[i] + om * A[k];
                }
            }
            return dL_dalpha * h.T;
        },
        [&](size_t gid, uint32_t qv, float v) {
            if (qv >= 8u && (int)(qv - 8u) < cw) atomicAdd(dL_dfeatures + gid * (size_t)C + (size_t)(c0 + (int)(qv - 8u)), v);
        },
        [&](uint32_t j, float w, float* acc_j) {
#pragma unroll
            for (int q8 = 0; q8 < CH / 8 + (CH % 8 ? 1 : 0); q8++) {
                if (8 * q8 >= cw) break;                       // uniform: nothing but padding from here on
                float v8[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v8[i] = (8 * q8 + i < CH) ? w * gp[(8 * q8 + i) < CH ? (8 * q8 + i) : 0] : 0.f;
                const float tot = wave_sum8_transposed(v8, p.lane);
                if (p.lane < 8u && 8u * (uint32_t)q8 + p.lane < (uint32_t)CH && tot != 0.f) lds_add_f32(&acc_j[8 + 8 * q8 + p.lane], tot);
            }
        },
        [&](uint32_t base) {
#pragma unroll
            for (uint32_t e = p.t; e < BATCH * (uint32_t)CH; e += 256u) {
                const uint32_t slot = e / (uint32_t)CH, k = e % (uint32_t)CH;
                float v = 0.0f;
                if (base + slot < p.n && (int)k < cw) v = features[(size_t)point_list[p.range.x + (p.n - 1 - (base + slot))] * (size_t)C + (size_t)(c0 + (int)k)];
                sf[slot][k] = v;
            }
        });
}

} // namespace gsrast
