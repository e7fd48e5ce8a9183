// gsrast_distort.h -- the depth-distortion map of one finished forward (Mip-NeRF 360's distortion loss, gsplat's render_distort) and its
// gradients (include/gsrast.h: gsrast_distortion_forward / gsrast_distortion_backward).
//
// A pair (pixel p, Gaussian i) CONTRIBUTES exactly as in gsrast_contrib.h: i's position in the tile's list in force is below n_contrib[p] and
// the pair passes the forward's nested tests (power <= 0 && power >= threshold; alpha = min(0.99, o exp(power)) >= 1/255; T (1 - alpha) >=
// 1e-4).  Its weight is w = alpha T, o the opacity the state carries (anti-aliasing compensation included); its depth z is rec1.z, the
// view-space depth acc_depth sums.  No background term.
//   distort[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_{i-1} - D_{i-1}),   A_{i-1} = sum_{j<i} w_j,  D_{i-1} = sum_{j<i} w_j z_j
// in list order (every tile list is in non-decreasing z; ties contribute 0 either way).  The quantity does not change under z -> z - z0:
// both kernels work on depths RELATIVE to z0 = the depth of the tile's first listed Gaussian (tile-uniform, read from the list head by
// both, not stored), so that z A - D does not cancel against the scene's distance from the camera.
//
// distort_fwd_kernel replays blend_fwd_cull_kernel front to back like features_fwd_kernel: one tile per workgroup (xcd_tile), four wave64
// on an 8 x 8 block each, rec0 / rec1 staged 256 instances per batch, strip_may_touch culling, gs_power, gs_exp<EXPMODE, true>, the
// forward's association for T, last = min(n_contrib, tile_max, list length).  Per lane: T, A, D and the running sum.  Every pixel inside the
// image is written: the map (0 with fewer than two contributors) and the moments [2][H][W] = (A_N, D_N), relative to z0, which the backward
// cannot recover going back to front.
//
// distort_bwd_kernel takes g[p] = dL/ddistort and goes back to front from final_T and n_contrib like features_bwd_kernel (T <- T / (1 - alpha)
// by the same v_rcp).  Per lane the suffix sums over the contributors behind the pair: SA = sum w, SD = sum w z, SG = sum G w.  Per pair
//   A_{i-1} = A_N - SA - w     D_{i-1} = D_N - SD - w z
//   dL/dz   = 2 g w (A_{i-1} - SA)
//   G       = dL/dw = 2 g (z (A_{i-1} - SA) + SD - D_{i-1})
//   dL/dalpha = T G - SG / (1 - alpha)
// From dL/dalpha: the sums for means2D (2), the conic (3) and the opacity (1) by the formulas, units, clamp conventions and commit_scale of
// floats 0-5 of the gradient record (the 0.99 clamp straight through, dL/dG = o dL/dalpha, dL/do = G dL/dalpha), ADDED to floats 0-5 of the
// Gaussian's record (GeomLayout::grec); dL/dz is ADDED to float 9, where the per-Gaussian backward reads dL/d(view-space z) under
// GSRAST_RENDER_AUX.  Nothing else of the record is touched.  Cross-lane: the seven sums in ONE transposing wave reduction
// (wave_sum8_transposed, eight slots); lanes 0-6 add the totals into the batch's LDS accumulators, and when the batch is retired ONE global
// float atomic per (workgroup, instance, value) leaves -- none per pixel, none for a zero sum.
//
// Which Gaussians receive adds: a wave only looks at list positions below its block's largest n_contrib (and the workgroup below tile_max)
// -- positions at which the forward's lanes were alive, the invariant gsrast_contrib.h states.  So only Gaussians whose `untouched` byte
// the forward cleared are added to: the sparse zeroing of the records and the sparse / grouped preprocess_bwd stay valid.
//
// Every __syncthreads() sits on a workgroup-uniform path; the batch loops' trip counts derive from n = min(tile_max, list length) alone.
//
// Resources (gfx950, tools/kernel_resources.sh distort_; scratch 0 in every instantiation), exp_mode 0 | 1 | 2:
//   distort_fwd_kernel:  VGPR 32 | 32 | 32,  LDS 8192 B
//   distort_bwd_kernel:  VGPR 51 | 51 | 50,  LDS 4352 B
// Both are far from the limits of eight waves per SIMD (64 VGPRs, 20 KiB of LDS per workgroup).
#pragma once
#include "gsrast_common.h"
#include "gsrast_blend.h"

namespace gsrast {

template <int EXPMODE>
__global__ void __launch_bounds__(256)
distort_fwd_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, int W, int H, int gx, uint32_t ntiles,
                   const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                   const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max,
                   float* __restrict__ distort_map /* [H][W] */, float* __restrict__ moments /* [2][H][W]: A_N, D_N (relative to z0) */)
{
    constexpr uint32_t FB = 256;                  // instances staged per batch (the forward's)
    __shared__ float4 s0[FB];
    __shared__ float4 s1[FB];
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
    // the tile's depth origin: the first listed Gaussian's (uniform; the backward reads the same entry)
    const float z0 = n_all ? rec1[(size_t)REC_STRIDE * point_list[range.x]].z : 0.0f;

    float T = 1.0f, A = 0.0f, D = 0.0f, dist = 0.0f;
    for (uint32_t base = 0; base < n; base += FB) {
        if (base) __syncthreads();                             // (uniform: the previous batch has been read)
        const uint32_t i = base + t;
        if (i < n) {
            const uint32_t g = point_list[range.x + i];
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g];
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
                    const float zr = b.z - z0;
                    dist = __builtin_fmaf(w, __builtin_fmaf(zr, A, -D), dist);      // w (z A_{i-1} - D_{i-1})
                    A += w;
                    D = __builtin_fmaf(w, zr, D);
                    T = test_T;
                }
            }
        }
    }
    if (inside) {
        const size_t plane = (size_t)W * H;
        distort_map[pid] = 2.0f * dist;
        moments[pid] = A; moments[plane + pid] = D;
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
    constexpr uint32_t BATCH = 64;                // instances staged per batch (the colour backward's)
    constexpr int AS = 8;                         // accumulators per staged instance: six geometric sums, dL/dz, one spare
    __shared__ float4 s0[BATCH];
    __shared__ float4 s1[BATCH];
    __shared__ uint32_t sid[BATCH];
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
    float T = inside ? final_T[pid] : 0.0f;
    uint32_t last = 0;
    if (inside) { const uint32_t nc = n_contrib[pid]; last = nc < n ? nc : n; }
    const float g2 = inside ? 2.0f * dL_ddistort[pid] : 0.0f;            // 2 dL/ddistort of the pixel
    const float AN = inside ? moments[pid] : 0.0f, DN = inside ? moments[plane + pid] : 0.0f;
    float SA = 0.0f, SD = 0.0f, SG = 0.0f;                     // sums over the contributors behind the current one
    uint32_t strip_last;
    {
        uint32_t m = last;                                     // deepest position the block needs (wave-uniform)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        strip_last = __builtin_amdgcn_readfirstlane(m);
    }
    const float z0 = n_all ? rec1[(size_t)REC_STRIDE * point_list[range.x]].z : 0.0f;      // the forward's depth origin
    // factor applied by lane l when it adds value l & 7: {mean.x, mean.y, conic a, b, c, opacity, z, -} (the colour backward's)
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
        if (t < BATCH * (uint32_t)AS / 4u) reinterpret_cast<float4*>(&acc[0][0])[t] = make_float4(0.f, 0.f, 0.f, 0.f);
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
            float u = 0.f, dz = 0.f;                           // G dL/dalpha, dL/dz: zero where the pair does not contribute
            if (__builtin_amdgcn_inverse_ballot_w64(m_ok)) {
                const float om = 1.0f - alpha;
                const float rcp1ma = __builtin_amdgcn_rcpf(om);
                T = T * rcp1ma;                                // the transmittance in front of the pair
                const float w = alpha * T;
                const float zr = b.z - z0;
                const float wz = w * zr;
                const float dA = (AN - SA - w) - SA;           // A_{i-1} - SA
                const float Dp = DN - SD - wz;                 // D_{i-1}
                const float Gw = g2 * (zr * dA + (SD - Dp));   // dL/dw
                const float dL_dalpha = T * Gw - SG * rcp1ma;
                dz = g2 * w * dA;
                SA += w; SD += wz; SG += Gw * w;
                u = G * dL_dalpha;
            }
            {
                const float gxv = (u * b.y) * dx, gyv = (u * b.y) * dy;        // dL/dG = o dL/dalpha, times G d(..): sign and 0.5 W / 0.5 H / 0.5 in commit_scale
                const float v8[8] = { gxv * a.z + gyv * a.w, gyv * b.x + gxv * a.w, gxv * dx, gxv * dy, gyv * dy, u, dz, 0.f };
                const float tot = wave_sum8_transposed(v8, lane);
                if (lane < 7u && tot != 0.f) lds_add_f32(&acc[j][lane], tot * commit_scale);
            }
        }
        __syncthreads();
        // retire the batch: one global atomic per (instance, value) whose sum is not zero
        for (uint32_t e = t; e < cnt * (uint32_t)AS; e += 256u) {
            const uint32_t slot = e / (uint32_t)AS, qv = e % (uint32_t)AS;
            const float v = acc[slot][qv];
            if (v != 0.f && qv < 7u) atomicAdd(grec + (size_t)sid[slot] * GREC + (qv < 6u ? qv : 9u), v);
        }
    }
}

} // namespace gsrast
