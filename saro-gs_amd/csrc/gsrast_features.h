// gsrast_features.h -- per-Gaussian feature vectors (1 <= C <= 64 channels) blended with the weights of one finished forward, and the
// gradients of that blend (include/gsrast.h: gsrast_features_forward / gsrast_features_backward).
//
// A pair (pixel p, Gaussian i) CONTRIBUTES exactly as in gsrast_contrib.h: i's position in the tile's list in force is below n_contrib[p] and
// the pair passes the forward's nested tests (power <= 0 && power >= threshold; alpha = min(0.99, o exp(power)) >= 1/255; T (1 - alpha) >=
// 1e-4).  Its weight is w = alpha T, o the opacity the state carries (anti-aliasing compensation included).  No background term.
//   feature_map[c][p] = sum_i w_ip f[i][c]                       f: [P][C] row-major, the map: [C][H][W] planar
//
// features_fwd_kernel replays blend_fwd_cull_kernel front to back like contrib_blend_kernel: one tile per workgroup (xcd_tile), four wave64
// on an 8 x 8 block each, rec0 / rec1 staged 256 instances per batch, strip_may_touch culling, gs_power, gs_exp<EXPMODE, true>, the
// forward's association for T, last = min(n_contrib, tile_max, list length).  The staged instances' feature rows lie beside their records
// in LDS, every lane keeps CH accumulators.  Every pixel inside the image is written (0 without a contributor).
//
// features_bwd_kernel takes g[c][p] = dL/dfeature_map and goes back to front from final_T and n_contrib like the colour's blend backward
// (blend_bwd_cull_t_kernel): T <- T / (1 - alpha) by the same v_rcp, A_c <- alpha f_c + (1 - alpha) A_c behind the pair, and per pair
//   dL/df[i][c] += w g[c][p]                 dL/dalpha = T sum_c g[c][p] (f[i][c] - A_c)
// From dL/dalpha: the sums for means2D (2), the conic (3) and the opacity (1) by the formulas, units, clamp conventions and commit_scale of
// floats 0-5 of the gradient record (the 0.99 clamp straight through, dL/dG = o dL/dalpha, dL/do = G dL/dalpha), ADDED to floats 0-5 of the
// Gaussian's record (GeomLayout::grec); floats 6-11 are not touched.  Cross-lane: the six geometric sums in one transposing wave reduction
// (wave_sum8_transposed), the channels eight at a time in the same; lanes 0-7 add the totals into the batch's LDS accumulators, and when
// the batch is retired ONE global float atomic per (workgroup, instance, value) leaves -- none per pixel, none for a zero sum.
//
// Channels: the kernels are instantiated for chunks of CH = 4, 8, 16, 32 channels; a call runs passes over [c0, c0 + CH) until C is covered
// (the smallest chunk that holds what is left, 32 at most).  Both directions are additive over chunks: dL/dalpha is a sum over channels, so
// each pass adds its part to the records.  A ragged last chunk is padded with zeros in LDS / registers: no address at or past
// features + P C (or the map's / the gradient's C planes) is formed for a load or a store.
//
// Which Gaussians receive adds: a wave only looks at list positions below its block's largest n_contrib (and the workgroup below tile_max)
// -- positions at which the forward's lanes were alive, the invariant gsrast_contrib.h states.  So only Gaussians whose `untouched` byte
// the forward cleared are added to, in the records and in dL_dfeatures alike: the sparse zeroing of the records and the sparse / grouped
// preprocess_bwd stay valid.
//
// Every __syncthreads() sits on a workgroup-uniform path; the batch loops' trip counts derive from n = min(tile_max, list length) alone.
//
// Resources (gfx950, tools/kernel_resources.sh features_; scratch 0 in every instantiation; exp_mode 0 | 1 | 2 agree within 3 VGPRs).  Occupancy in
// waves per SIMD, the smaller of the register file's (512 / VGPRs) and LDS's (160 KiB / workgroup's LDS; a workgroup is one wave per SIMD):
//   features_fwd_kernel  CH =  4 |  8 | 16 | 32:  VGPR 38 | 42 | 73 |  97,  LDS 12288 | 16384 | 24576 | 40960 B  ->  8 | 8 | 6 | 4  (LDS-bound at CH 16 and 32)
//   features_bwd_kernel  CH =  4 |  8 | 16 | 32:  VGPR 60 | 71 | 98 | 141,  LDS  6400 |  8448 | 12544 | 20736 B  ->  8 | 7 | 4 | 3  (register-bound)
// CH = 32 is the widest chunk: 64 channels in one pass would need 2 x 64 registers of per-pixel state in the backward alone (one wave per SIMD, or scratch).
#pragma once
#include "gsrast_common.h"
#include "gsrast_blend.h"

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
    constexpr uint32_t BATCH = 64;                // instances staged per batch (the colour backward's)
    constexpr int AS = CH + 8;                    // accumulators per staged instance: six geometric sums (two spare), CH channels
    __shared__ float4 s0[BATCH];
    __shared__ float4 s1[BATCH];
    __shared__ uint32_t sid[BATCH];
    __shared__ __attribute__((aligned(16))) float sf[BATCH][CH];
    __shared__ __attribute__((aligned(16))) float acc[BATCH][AS];      // shared by the four waves (LDS float adds)
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
    const uint32_t n = tm < n_all ? tm : n_all;               // instances at list position >= n touch no pixel
    const size_t plane = (size_t)W * H;
    const size_t pid = (size_t)W * py + px;
    const int cw = (C - c0) < CH ? (C - c0) : CH;             // channels of this pass that exist
    float T = inside ? final_T[pid] : 0.0f;
    uint32_t last = 0;
    if (inside) { const uint32_t nc = n_contrib[pid]; last = nc < n ? nc : n; }
    float gp[CH], A[CH];                                       // dL/dfeature_map of the pixel; the blend behind the current contributor
#pragma unroll
    for (int k = 0; k < CH; k++) { gp[k] = (inside && k < cw) ? dL_dmap[(size_t)(c0 + k) * plane + pid] : 0.0f; A[k] = 0.0f; }
    uint32_t strip_last;
    {
        uint32_t m = last;                                     // deepest position the block needs (wave-uniform)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        strip_last = __builtin_amdgcn_readfirstlane(m);
    }
    // factor applied by lane l when it adds value l & 7: {mean.x, mean.y, conic a, b, c, opacity, -, -} (the colour backward's)
    const unsigned kind = lane & 7u;
    const float commit_scale = kind == 0u ? -0.5f * (float)W : kind == 1u ? -0.5f * (float)H : (kind >= 2u && kind <= 4u) ? -0.5f : 1.0f;

    // list position `pos` (0-based from the FRONT of the tile's list) is visited from n - 1 down to 0
    for (uint32_t base = 0; base < n; base += BATCH) {
        if (base) __syncthreads();                             // (uniform: the previous batch has been committed)
        if (t < BATCH && base + t < n) {
            const uint32_t g = point_list[range.x + (n - 1 - (base + t))];
            sid[t] = g;
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g];
        }
#pragma unroll
        for (uint32_t e = t; e < BATCH * (uint32_t)CH; e += 256u) {
            const uint32_t slot = e / (uint32_t)CH, k = e % (uint32_t)CH;
            float v = 0.0f;
            if (base + slot < n && (int)k < cw) v = features[(size_t)point_list[range.x + (n - 1 - (base + slot))] * (size_t)C + (size_t)(c0 + (int)k)];
            sf[slot][k] = v;
        }
        for (uint32_t e = t; e < BATCH * (uint32_t)AS / 4u; e += 256u) reinterpret_cast<float4*>(&acc[0][0])[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const uint32_t cnt = (n - base) < BATCH ? (n - base) : BATCH;
        uint64_t mk;
        {
            const uint32_t spos = n - 1 - (base + lane);      // list position of this lane's instance (only used when lane < cnt)
            const bool valid = lane < cnt;
            const float4 a = valid ? s0[lane] : make_float4(0.f, 0.f, 1.f, 0.f);
            const float czv = valid ? s1[lane].x : 1.f;
            const float thr = valid ? s1[lane].w : 1.f;
            mk = __ballot(valid && spos < strip_last && strip_may_touch(a, czv, thr, sx0, sx1, sy0, sy1));
        }
        while (mk) {
            const uint32_t j = (uint32_t)__builtin_ctzll(mk);
            mk &= mk - 1;
            const uint32_t pos = n - 1 - (base + j);
            const float4 a = s0[j];
            const float4 b = s1[j];
            const float dx = a.x - pxf, dy = a.y - pyf;
            const float q = __builtin_fmaf(b.x * dy, dy, (a.z * dx) * dx);
            const float power = __builtin_fmaf(-0.5f, q, -((a.w * dx) * dy));
            const uint64_t m_in = __builtin_amdgcn_ballot_w64(pos < last) & __builtin_amdgcn_ballot_w64(power <= 0.0f) &
                                  __builtin_amdgcn_ballot_w64(power >= b.w);
            if (m_in == 0ull) continue;
            const float G = gs_exp<EXPMODE, true>(power);
            float alpha = b.y * G;
            alpha = alpha < 0.99f ? alpha : 0.99f;
            const uint64_t m_ok = m_in & __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
            if (m_ok == 0ull) continue;
            float u = 0.f, dch = 0.f;                          // G dL/dalpha, alpha T: zero where the pair does not contribute
            if (__builtin_amdgcn_inverse_ballot_w64(m_ok)) {
                const float om = 1.0f - alpha;
                const float rcp1ma = __builtin_amdgcn_rcpf(om);
                T = T * rcp1ma;
                float dL_dalpha = 0.f;
#pragma unroll
                for (int q4 = 0; q4 < CH / 4; q4++) {
                    const float4 f = *reinterpret_cast<const float4*>(&sf[j][4 * q4]);
                    const float fk[4] = { f.x, f.y, f.z, f.w };
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int k = 4 * q4 + i;
                        dL_dalpha += (fk[i] - A[k]) * gp[k];
                        A[k] = alpha * fk[i] + om * A[k];
                    }
                }
                dL_dalpha *= T;
                dch = alpha * T; u = G * dL_dalpha;
            }
            {
                const float gxv = (u * b.y) * dx, gyv = (u * b.y) * dy;        // dL/dG = o dL/dalpha, times G d(..): sign and 0.5 W / 0.5 H / 0.5 in commit_scale
                const float v8[8] = { gxv * a.z + gyv * a.w, gyv * b.x + gxv * a.w, gxv * dx, gxv * dy, gyv * dy, u, 0.f, 0.f };
                const float tot = wave_sum8_transposed(v8, lane);
                if (lane < 6u && tot != 0.f) lds_add_f32(&acc[j][lane], tot * commit_scale);
            }
#pragma unroll
            for (int q8 = 0; q8 < CH / 8 + (CH % 8 ? 1 : 0); q8++) {
                if (8 * q8 >= cw) break;                       // uniform: nothing but padding from here on
                float v8[8];
#pragma unroll
                for (int i = 0; i < 8; i++) v8[i] = (8 * q8 + i < CH) ? dch * gp[(8 * q8 + i) < CH ? (8 * q8 + i) : 0] : 0.f;
                const float tot = wave_sum8_transposed(v8, lane);
                if (lane < 8u && 8u * (uint32_t)q8 + lane < (uint32_t)CH && tot != 0.f) lds_add_f32(&acc[j][8 + 8 * q8 + lane], tot);
            }
        }
        __syncthreads();
        // retire the batch: one global atomic per (instance, value) whose sum is not zero
        for (uint32_t e = t; e < cnt * (uint32_t)AS; e += 256u) {
            const uint32_t slot = e / (uint32_t)AS, qv = e % (uint32_t)AS;
            const float v = acc[slot][qv];
            if (v != 0.f) {
                const size_t gid = sid[slot];
                if (qv < 6u) atomicAdd(grec + gid * GREC + qv, v);
                else if (qv >= 8u && (int)(qv - 8u) < cw) atomicAdd(dL_dfeatures + gid * (size_t)C + (size_t)(c0 + (int)(qv - 8u)), v);
            }
        }
    }
}

} // namespace gsrast
