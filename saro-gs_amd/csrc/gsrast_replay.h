// gsrast_replay.h -- the blend of one finished forward, walked again: what gsrast_contrib.h, gsrast_features.h, gsrast_distort.h and
// gsrast_topk.h share (contrib_blend_kernel and features_fwd_kernel share the invariant and keep a body of their own: their headers say why).
//
// THE REPLAY INVARIANT.  A pair (pixel p, Gaussian i) CONTRIBUTES when the forward blended it: i's position in the tile's list in force is
// below n_contrib[p] and the pair passes the forward's nested tests (power <= 0 && power >= threshold; alpha = min(0.99, o exp(power)) >=
// 1/255; T (1 - alpha) >= 1e-4 -- the terminating entry does not contribute).  Its weight is w = alpha T, T the transmittance in front of
// it, o the opacity the state carries (anti-aliasing compensation included).  The walkers below replay blend_fwd_cull_body (gsrast_blend.h)
// from the state it left behind: the same geometry (one tile per workgroup by xcd_tile, four wave64, each an 8 x 8 block), the same
// wave-level culling (strip_may_touch), the same arithmetic (gs_power, gs_exp<EXPMODE, true>, the forward's association) and the same
// nested tests, so that every pixel's alpha and T are the forward's bit for bit at every step.  What the forward decided by carrying `alive`
// lanes they decide from the stored n_contrib: a lane looks at list positions below last = min(n_contrib, tile_max, list length), a wave at
// those below its block's maximum of last, the workgroup at those below n = min(tile_max, list length) -- at every such position the
// forward's lanes were alive, so the replayed pair sees the operands the forward saw.  rec2 (the colour) is never staged.
//   front to back: T starts at 1 and follows the forward, T <- T (1 - alpha) on a contributing pair; rec0 / rec1 staged 256 per batch.
//   back to front: T starts at final_T and is undone, T <- T v_rcp(1 - alpha), as the colour's blend backward (blend_bwd_cull_t_kernel)
//   undoes it; the list is staged reversed, 64 per batch, and the pairs' gradient sums leave as described at replay_back_to_front.
//
// WHICH GAUSSIANS RECEIVE ADDS.  A wave only looks at list positions below its block's largest n_contrib (and the workgroup below tile_max),
// positions at which the forward's lanes were alive.  So only Gaussians whose `untouched` byte the forward cleared are added to, in the
// gradient records and in a visitor's own outputs alike: the sparse zeroing of the records and the sparse / grouped preprocess_bwd stay valid.
//
// Every __syncthreads() sits on a workgroup-uniform path; the batch loops' trip counts derive from n alone.  A kernel is a prologue
// (replay_pixel), its per-pixel registers, one walker call with lambdas that capture those registers by reference, and its stores.
#pragma once
#include "gsrast_common.h"
#include "gsrast_blend.h"

namespace gsrast {

// A lane's pixel and its workgroup's tile
struct ReplayPixel {
    uint2 range;                    // the tile's list in force (into point_list)
    uint32_t n;                     // min(tile_max, list length): list positions >= tile_max were consumed by no pixel
    uint32_t last;                  // min(n_contrib, n) of a pixel inside the image, else 0
    uint32_t t;                     // threadIdx.x
    unsigned lane;
    float sx0, sx1, sy0, sy1;       // the wave's 8 x 8 block (pixel centres), the box strip_may_touch culls against
    float pxf, pyf;
    bool inside;
    size_t pid;                     // W * py + px (an address only where `inside`)
    int W, H;
};

// The deepest position the wave's block needs (wave-uniform)
__device__ __forceinline__ uint32_t replay_wave_last(uint32_t last)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(last, d, 64); last = o > last ? o : last; }
    return __builtin_amdgcn_readfirstlane(last);
}

// False for a workgroup of the padded grid that has no tile (uniform).
__device__ __forceinline__ bool replay_pixel(ReplayPixel& p, const uint2* __restrict__ ranges, int W, int H, int gx, uint32_t ntiles,
                                             const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ tile_max)
{
    const uint32_t tile = xcd_tile(blockIdx.x, ntiles);      // neighbouring tiles share Gaussians: one band of tiles per XCD
    if (tile >= ntiles) return false;
    const uint32_t tx = tile % (uint32_t)gx, ty = tile / (uint32_t)gx;
    p.t = threadIdx.x; p.lane = lane_id(); p.W = W; p.H = H;
    const unsigned wave = p.t >> 6;
    const uint32_t bx = (wave & 1u) * 8u, by = (wave >> 1) * 8u;
    const uint32_t px = tx * TILE_X + bx + (p.lane & 7u), py = ty * TILE_Y + by + (p.lane >> 3);
    p.sx0 = (float)(tx * TILE_X + bx); p.sx1 = p.sx0 + 7.0f;
    p.sy0 = (float)(ty * TILE_Y + by); p.sy1 = p.sy0 + 7.0f;
    p.inside = px < (uint32_t)W && py < (uint32_t)H;
    p.pxf = (float)px; p.pyf = (float)py;
    p.range = ranges[tile];
    const uint32_t n_all = p.range.y - p.range.x, tm = tile_max[tile];
    p.n = tm < n_all ? tm : n_all;
    p.pid = (size_t)W * py + px;
    p.last = 0;
    if (p.inside) { const uint32_t nc = n_contrib[p.pid]; p.last = nc < p.n ? nc : p.n; }
    return true;
}

// The staged Gaussians' ids beside s0 / s1: 1 KiB of LDS that only an instantiation with IDS has
template <bool IDS, uint32_t FB>
__device__ __forceinline__ uint32_t* replay_staged_ids()
{
    if constexpr (IDS) { __shared__ uint32_t sid[FB]; return sid; }
    else return nullptr;
}

// pair(w, b) is called in the lanes whose pixel blended the pair: w = alpha T, T in front of the pair; b its rec1.  A batch is two phases,
// staging and walk; the barrier that separates a batch's walk from the next batch's staging sits in front of the staging.
// IDS (opt-in, compile time): the batch's Gaussian ids are staged too and the visitor is pair(w, b, id); without it nothing of that is
// compiled and an instantiation is what it was before the switch existed.
template <int EXPMODE, bool IDS = false, class Pair>
__device__ __forceinline__ void replay_front_to_back(const ReplayPixel& p, const uint32_t* __restrict__ point_list,
                                                     const float4* __restrict__ rec0, const float4* __restrict__ rec1, Pair&& pair)
{
    constexpr uint32_t FB = 256;                  // instances staged per batch (the forward's)
    __shared__ float4 s0[FB];
    __shared__ float4 s1[FB];
    uint32_t* const sid = replay_staged_ids<IDS, FB>();
    const uint32_t t = p.t, n = p.n, last = p.last;
    const unsigned lane = p.lane;
    const uint32_t wave_last = replay_wave_last(last);
    float T = 1.0f;
    for (uint32_t base = 0; base < n; base += FB) {
        if (base) __syncthreads();                             // (uniform: the previous batch has been read)
        const uint32_t i = base + t;
        if (i < n) {
            const uint32_t g = point_list[p.range.x + i];
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g];
            if constexpr (IDS) sid[t] = g;
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
                touch = strip_may_touch(a, b.x, b.w, p.sx0, p.sx1, p.sy0, p.sy1);
            }
            uint64_t mask = __ballot(touch);
            while (mask) {
                const uint32_t j = r * 64u + (uint32_t)__builtin_ctzll(mask);
                mask &= mask - 1;
                const float4 a = s0[j];
                const float4 b = s1[j];
                const float dx = a.x - p.pxf, dy = a.y - p.pyf;
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
                    if constexpr (IDS) pair(alpha * T, b, sid[j]);
                    else pair(alpha * T, b);
                    T = test_T;
                }
            }
        }
    }
}

struct ReplayNoHook { template <class... A> __device__ __forceinline__ void operator()(A...) const {} };

// One pair that contributes in this lane, back to front
struct ReplayBackHit {
    uint32_t j;                     // its staged slot
    float4 b;                       // its rec1
    float alpha, rcp1ma;            // v_rcp(1 - alpha)
    float T, w;                     // the transmittance in front of the pair, alpha T
};

// The pairs of replay_front_to_back, last first, and the gradient their dL/dalpha sends to floats 0-5 of the Gaussians' records.
//   pair(const ReplayBackHit&, float& extra) is called by the lanes in which the pair contributes and returns dL/dalpha; from G dL/dalpha the
//     walker forms the sums for means2D (2), the conic (3) and the opacity (1) by the formulas, units, clamp conventions and commit_scale of
//     the colour's blend backward (the 0.99 clamp straight through, dL/dG = o dL/dalpha, dL/do = G dL/dalpha).  `extra` (0 unless set) is
//     summed beside them, unscaled, as value 6.
//   more(j, w, acc_j) is called by ALL lanes behind that (w = 0 in a lane in which the pair does not contribute): further wave sums of the
//     visitor's own, added into acc_j[8 ...).
//   stage(base) runs with the batch's staging in front of the barrier (staged slot k holds list position n - 1 - (base + k)).
// Cross-lane: the seven sums in ONE transposing wave reduction (wave_sum8_transposed); lanes 0-6 add the non-zero totals into the batch's LDS
// accumulators acc[64][AS] (shared by the four waves), and when the batch is retired ONE global float atomic per (workgroup, instance,
// value) leaves -- none per pixel, none for a zero sum: values 0-5 into floats 0-5 of the record (GeomLayout::grec), every other one
// through retire(Gaussian, value index, sum).  Nothing else of the record is touched.
// Floating-point contraction is on for this body as it is for the colour's blend backward; a visitor written inside a kernel takes the
// kernel's own setting.
template <int EXPMODE, int AS, class Pair, class Retire, class More = ReplayNoHook, class Stage = ReplayNoHook>
__device__ __forceinline__ void replay_back_to_front(const ReplayPixel& p, const uint32_t* __restrict__ point_list,
                                                     const float4* __restrict__ rec0, const float4* __restrict__ rec1,
                                                     const float* __restrict__ final_T, float* __restrict__ grec,
                                                     Pair&& pair, Retire&& retire, More&& more = More(), Stage&& stage = Stage())
{
#pragma clang fp contract(fast)
    constexpr uint32_t BATCH = 64;                // instances staged per batch (the colour backward's)
    __shared__ float4 s0[BATCH];
    __shared__ float4 s1[BATCH];
    __shared__ uint32_t sid[BATCH];
    __shared__ __attribute__((aligned(16))) float acc[BATCH][AS];
    const uint32_t t = p.t, n = p.n, last = p.last;
    const unsigned lane = p.lane;
    float T = p.inside ? final_T[p.pid] : 0.0f;
    const uint32_t strip_last = replay_wave_last(last);
    // factor applied by lane l when it adds value l & 7: {mean.x, mean.y, conic a, b, c, opacity, extra, -} (the colour backward's)
    const unsigned kind = lane & 7u;
    const float commit_scale = kind == 0u ? -0.5f * (float)p.W : kind == 1u ? -0.5f * (float)p.H : (kind >= 2u && kind <= 4u) ? -0.5f : 1.0f;

    // list position `pos` (0-based from the FRONT of the tile's list) is visited from n - 1 down to 0
    for (uint32_t base = 0; base < n; base += BATCH) {
        if (base) __syncthreads();                             // (uniform: the previous batch has been committed)
        if (t < BATCH && base + t < n) {
            const uint32_t g = point_list[p.range.x + (n - 1 - (base + t))];
            sid[t] = g;
            s0[t] = rec0[(size_t)REC_STRIDE * g]; s1[t] = rec1[(size_t)REC_STRIDE * g];
        }
        stage(base);
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
            mk = __ballot(valid && spos < strip_last && strip_may_touch(a, czv, thr, p.sx0, p.sx1, p.sy0, p.sy1));
        }
        while (mk) {
            const uint32_t j = (uint32_t)__builtin_ctzll(mk);
            mk &= mk - 1;
            const uint32_t pos = n - 1 - (base + j);
            const float4 a = s0[j];
            const float4 b = s1[j];
            const float dx = a.x - p.pxf, dy = a.y - p.pyf;
            const float power = gs_power(a.z, a.w, b.x, dx, dy);
            const uint64_t m_in = __builtin_amdgcn_ballot_w64(pos < last) & __builtin_amdgcn_ballot_w64(power <= 0.0f) &
                                  __builtin_amdgcn_ballot_w64(power >= b.w);
            if (m_in == 0ull) continue;
            const float G = gs_exp<EXPMODE, true>(power);
            float alpha = b.y * G;
            alpha = alpha < 0.99f ? alpha : 0.99f;
            const uint64_t m_ok = m_in & __builtin_amdgcn_ballot_w64(!(alpha < 1.0f / 255.0f));
            if (m_ok == 0ull) continue;
            float u = 0.f, extra = 0.f, w = 0.f;              // G dL/dalpha, the visitor's value 6, alpha T: zero where the pair does not contribute
            if (__builtin_amdgcn_inverse_ballot_w64(m_ok)) {
                const float rcp1ma = __builtin_amdgcn_rcpf(1.0f - alpha);
                T = T * rcp1ma;                                // the transmittance in front of the pair
                w = alpha * T;
                u = G * pair(ReplayBackHit{ j, b, alpha, rcp1ma, T, w }, extra);
            }
            {
                const float gxv = (u * b.y) * dx, gyv = (u * b.y) * dy;        // dL/dG = o dL/dalpha, times G d(..): sign and 0.5 W / 0.5 H / 0.5 in commit_scale
                const float v8[8] = { gxv * a.z + gyv * a.w, gyv * b.x + gxv * a.w, gxv * dx, gxv * dy, gyv * dy, u, extra, 0.f };
                const float tot = wave_sum8_transposed(v8, lane);
                if (lane < 7u && tot != 0.f) lds_add_f32(&acc[j][lane], tot * commit_scale);
            }
            more(j, w, &acc[j][0]);
        }
        __syncthreads();
        // retire the batch: one global atomic per (instance, value) whose sum is not zero
        for (uint32_t e = t; e < cnt * (uint32_t)AS; e += 256u) {
            const uint32_t slot = e / (uint32_t)AS, qv = e % (uint32_t)AS;
            const float v = acc[slot][qv];
            if (v != 0.f) {
                const size_t gid = sid[slot];
                if (qv < 6u) atomicAdd(grec + gid * GREC + qv, v);
                else retire(gid, qv, v);
            }
        }
    }
}

} // namespace gsrast
