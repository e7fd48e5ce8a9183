// gsrast_densify.h -- densification on the device: clone / split / prune of every per-Gaussian array together with its Adam
// moments, plus the per-iteration statistics update.  Reference behaviour restated (paths relative to the reference's root):
//   scene/saro_gaussian.py:705-736  densify_pruneclone: grads = accum / denom (NaN -> 0) * inv_intergral_fordensify; clone; split; prune
//   scene/saro_gaussian.py:685-701  densify_and_clone:   g >= thr and max(exp(scaling)) <= percent_dense * extent: the row is appended once
//   scene/saro_gaussian.py:646-682  densify_and_splitv2: g >= thr and max(exp(scaling)) >  percent_dense * extent: N copies are appended,
//                                   xyz + R(q) (noise * exp(scaling)), scaling = log(exp(scaling) / (0.8 N)); the sources are removed
//   scene/saro_gaussian.py:555-640  _prune_optimizer / cat_tensors_to_optimizer: every group's exp_avg / exp_avg_sq follow (new rows: zeros)
//   train.py:282-292, scene/saro_gaussian.py:745-750   the statistics the criterion reads (stats_update_kernel)
// Two launches for the plan (classify, then the scan of the workgroup sums; the apply redoes the 256-wide scan in LDS) and one launch
// that moves every group.  Output layout:
//   [ originals !split && !pruned | clones of clone && !pruned | split copy 0 of split && !pruned | copy 1 | ... | copy N-1 ]
// every part in source order.  The noise row of copy k of source i is noise[k * n_split_all + rank of i among ALL split-selected sources],
// pruned or not (the reference draws its samples before it prunes).  No atomics: every count comes from a scan, every destination row
// has exactly one writer, so the result is the same bits on every run and every rank.
#pragma once
#include "gsrast_gaussian.h"

namespace gsrast {

constexpr int DN_RUN = 256;              // consecutive sources per workgroup (classify and apply alike: the scan's first level)
constexpr int DN_MAX_GROUPS = 16, DN_MAX_WIDTH = 64, DN_MAX_N = 4;
constexpr unsigned char DN_KEEP = 1, DN_CLONE = 2, DN_SPLIT = 4, DN_SPLIT_ALL = 8;      // class bits (KEEP: the original row survives)
constexpr int DN_ROLE_COPY = 0, DN_ROLE_XYZ = 1, DN_ROLE_SCALING = 2;

struct DnCount { uint32_t kept, clone, split, split_all; };
__device__ __forceinline__ DnCount dn_add(DnCount a, DnCount b) { return DnCount{ a.kept + b.kept, a.clone + b.clone, a.split + b.split, a.split_all + b.split_all }; }
__device__ __forceinline__ DnCount dn_of(unsigned char c)
{
    return DnCount{ (c & DN_KEEP) ? 1u : 0u, (c & DN_CLONE) ? 1u : 0u, (c & DN_SPLIT) ? 1u : 0u, (c & DN_SPLIT_ALL) ? 1u : 0u };
}

// Exclusive scan of one DnCount per thread over a 256-thread workgroup; *total = the workgroup's sum.  `wsum`: 4 entries of LDS.
__device__ __forceinline__ DnCount dn_block_excl_scan(DnCount v, DnCount* total, DnCount* wsum)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    DnCount inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        DnCount t{ __shfl_up(inc.kept, d, 64), __shfl_up(inc.clone, d, 64), __shfl_up(inc.split, d, 64), __shfl_up(inc.split_all, d, 64) };
        if (lane >= (unsigned)d) inc = dn_add(inc, t);
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    DnCount base{ 0, 0, 0, 0 }, tot{ 0, 0, 0, 0 };
#pragma unroll
    for (int w = 0; w < 4; w++) { const DnCount s = wsum[w]; if (w < (int)wave) base = dn_add(base, s); tot = dn_add(tot, s); }
    __syncthreads();
    *total = tot;
    return DnCount{ base.kept + inc.kept - v.kept, base.clone + inc.clone - v.clone, base.split + inc.split - v.split, base.split_all + inc.split_all - v.split_all };
}

// One source per thread: its class byte, and the workgroup's four counts into sums[0..3][blockIdx] (four arrays of `nb` words).
__global__ void __launch_bounds__(DN_RUN)
densify_classify_kernel(int P, const float* __restrict__ accum, const float* __restrict__ denom, const float* __restrict__ grad_scale,
                        const float* __restrict__ scaling, const float* __restrict__ opacity_logit, const unsigned char* __restrict__ prune_src,
                        float thr, int select /* 0: nothing is cloned or split (thr = +inf) */, float tau, float min_opacity,
                        unsigned char* __restrict__ cls, uint32_t* __restrict__ sums, uint32_t nb)
{
    __shared__ DnCount wsum[4];
    const int i = blockIdx.x * DN_RUN + threadIdx.x;
    unsigned char c = 0;
    if (i < P) {
        bool pruned = prune_src && prune_src[i] != 0;
        if (min_opacity > 0.0f) pruned = pruned || (1.0f / (1.0f + expf(-opacity_logit[i]))) < min_opacity;
        bool sel = false, big = false;
        if (select) {
            float g = accum ? accum[i] / denom[i] : 0.0f;
            if (g != g) g = 0.0f;
            if (grad_scale) g *= grad_scale[i];
            sel = g >= thr;
            const float smax = fmaxf(fmaxf(expf(scaling[3 * (size_t)i]), expf(scaling[3 * (size_t)i + 1])), expf(scaling[3 * (size_t)i + 2]));
            big = smax > tau;
        }
        const bool split_all = sel && big, clone = sel && !big && !pruned;
        c = (unsigned char)((!split_all && !pruned ? DN_KEEP : 0) | (clone ? DN_CLONE : 0) | (split_all && !pruned ? DN_SPLIT : 0) | (split_all ? DN_SPLIT_ALL : 0));
        cls[i] = c;
    }
    DnCount tot;
    (void)dn_block_excl_scan(dn_of(c), &tot, wsum);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tot.kept; sums[nb + blockIdx.x] = tot.clone; sums[2 * (size_t)nb + blockIdx.x] = tot.split; sums[3 * (size_t)nb + blockIdx.x] = tot.split_all;
    }
}

// Single workgroup: the four arrays of workgroup sums become exclusive prefixes in place (256 sums per turn, with a carry), and
// counts[5] = { n_kept, n_clone, n_split, n_split_all, P' = n_kept + n_clone + N * n_split }.  nb = 0 (P = 0): counts are zeros.
__global__ void __launch_bounds__(DN_RUN)
densify_scan_kernel(uint32_t* __restrict__ sums, uint32_t nb, int N, uint32_t* __restrict__ counts)
{
    __shared__ DnCount wsum[4];
    DnCount carry{ 0, 0, 0, 0 };
    for (uint32_t c0 = 0; c0 < nb; c0 += DN_RUN) {
        const uint32_t b = c0 + threadIdx.x;
        DnCount v{ 0, 0, 0, 0 };
        if (b < nb) v = DnCount{ sums[b], sums[nb + b], sums[2 * (size_t)nb + b], sums[3 * (size_t)nb + b] };
        DnCount tot;
        const DnCount ex = dn_add(dn_block_excl_scan(v, &tot, wsum), carry);
        if (b < nb) { sums[b] = ex.kept; sums[nb + b] = ex.clone; sums[2 * (size_t)nb + b] = ex.split; sums[3 * (size_t)nb + b] = ex.split_all; }
        carry = dn_add(carry, tot);
    }
    if (threadIdx.x == 0) {
        counts[0] = carry.kept; counts[1] = carry.clone; counts[2] = carry.split; counts[3] = carry.split_all;
        counts[4] = carry.kept + carry.clone + (uint32_t)N * carry.split;
    }
}

struct DnGroup { const float *src, *src_m, *src_v; float *dst, *dst_m, *dst_v; int width, role; };
struct DnApplyArgs {
    DnGroup grp[DN_MAX_GROUPS];
    int n_groups, P, N;
    uint32_t n_kept, n_clone, n_split, n_split_all, p_new, nb;
    const unsigned char* cls; const uint32_t* sums;
    const float *rotation, *scaling, *noise;
};

// Component c of  R(q / |q|) (noise * exp(scaling))  (utils/general_utils.py:127-148 build_rotation, q = (r, x, y, z)).
__device__ __forceinline__ float dn_split_offset(const float* __restrict__ rotation, const float* __restrict__ scaling, const float* __restrict__ noise,
                                                 size_t src, size_t nrow, int c)
{
    float r = rotation[4 * src], x = rotation[4 * src + 1], y = rotation[4 * src + 2], z = rotation[4 * src + 3];
    const float norm = sqrtf(r * r + x * x + y * y + z * z);
    r /= norm; x /= norm; y /= norm; z /= norm;
    const float s0 = noise[3 * nrow] * expf(scaling[3 * src]), s1 = noise[3 * nrow + 1] * expf(scaling[3 * src + 1]), s2 = noise[3 * nrow + 2] * expf(scaling[3 * src + 2]);
    const float q[4] = { r, x, y, z };
    M3 R;
    quat_to_R(q, R);
    if (c == 0) return R.m[0][0] * s0 + R.m[0][1] * s1 + R.m[0][2] * s2;
    if (c == 1) return R.m[1][0] * s0 + R.m[1][1] * s1 + R.m[1][2] * s2;
    return R.m[2][0] * s0 + R.m[2][1] * s1 + R.m[2][2] * s2;
}

// A workgroup takes DN_RUN consecutive sources: class and destination rows into LDS, then every group's run x width floats with
// consecutive lanes on consecutive floats (the reads are coalesced; the kept rows' writes are wherever survivors are dense).
__global__ void __launch_bounds__(DN_RUN)
densify_apply_kernel(DnApplyArgs a)
{
    __shared__ DnCount wsum[4];
    __shared__ unsigned char s_cls[DN_RUN];
    __shared__ uint32_t s_keep[DN_RUN], s_new[DN_RUN], s_noise[DN_RUN];      // kept row | clone row or split copy 0's row | noise rank
    const uint32_t blk = blockIdx.x;
    const size_t first = (size_t)blk * DN_RUN;
    const int run = (int)((size_t)a.P - first < (size_t)DN_RUN ? (size_t)a.P - first : (size_t)DN_RUN);
    {
        const unsigned char c = (int)threadIdx.x < run ? a.cls[first + threadIdx.x] : (unsigned char)0;
        DnCount tot;
        const DnCount ex = dn_block_excl_scan(dn_of(c), &tot, wsum);
        s_cls[threadIdx.x] = c;
        s_keep[threadIdx.x] = a.sums[blk] + ex.kept;
        s_new[threadIdx.x] = (c & DN_SPLIT) ? a.n_kept + a.n_clone + a.sums[2 * (size_t)a.nb + blk] + ex.split : a.n_kept + a.sums[a.nb + blk] + ex.clone;
        s_noise[threadIdx.x] = a.sums[3 * (size_t)a.nb + blk] + ex.split_all;
    }
    __syncthreads();
    for (int gi = 0; gi < a.n_groups; gi++) {
        const DnGroup G = a.grp[gi];
        const int w = G.width, total = run * w, qstep = DN_RUN / w, rstep = DN_RUN % w;
        const float div = (float)(0.8 * (double)a.N);
        int r = (int)threadIdx.x / w, c = (int)threadIdx.x % w;
        for (int e = threadIdx.x; e < total; e += DN_RUN) {
            const unsigned char k = s_cls[r];
            if (k & (DN_KEEP | DN_SPLIT)) {                              // (a cloned row is a kept row too)
                const size_t so = (first + r) * (size_t)w + c;
                const float v = G.src[so];
                if (k & DN_KEEP) {
                    const uint32_t row = s_keep[r];
                    if (row < a.n_kept) {                                // (always, for the scratch of this plan: a guard against a foreign one)
                        const size_t o = (size_t)row * w + c;
                        G.dst[o] = v;
                        if (G.dst_m) G.dst_m[o] = G.src_m[so];
                        if (G.dst_v) G.dst_v[o] = G.src_v[so];
                    }
                    if (k & DN_CLONE) {
                        const uint32_t crow = s_new[r];
                        if (crow < a.n_kept + a.n_clone) {
                            const size_t o = (size_t)crow * w + c;
                            G.dst[o] = v;
                            if (G.dst_m) G.dst_m[o] = 0.0f;
                            if (G.dst_v) G.dst_v[o] = 0.0f;
                        }
                    }
                } else {
                    float base = v;
                    if (G.role == DN_ROLE_SCALING) base = logf(expf(v) / div);
                    for (int n = 0; n < a.N; n++) {
                        const uint32_t row = s_new[r] + (uint32_t)n * a.n_split;
                        if (row >= a.p_new || s_noise[r] >= a.n_split_all) continue;
                        float out = base;
                        if (G.role == DN_ROLE_XYZ)
                            out = v + dn_split_offset(a.rotation, a.scaling, a.noise, first + r, (size_t)n * a.n_split_all + s_noise[r], c);
                        const size_t o = (size_t)row * w + c;
                        G.dst[o] = out;
                        if (G.dst_m) G.dst_m[o] = 0.0f;
                        if (G.dst_v) G.dst_v[o] = 0.0f;
                    }
                }
            }
            r += qstep; c += rstep;
            if (c >= w) { c -= w; r++; }
        }
    }
}

// The transpose of a prune-only apply (gsrast_densify_scatter): the same workgroup-to-run mapping and the same LDS scan, but the walk is over
// the DESTINATION's run x width floats: a kept row loads its floats from row s_keep of the compact source (survivors keep index order, so a
// run reads one contiguous span), every other element stores +0.0f.  One writer per element, nothing read from an unselected row.
constexpr uint32_t DN_NO_ROW = 0xFFFFFFFFu;
constexpr int DN_SCATTER_UNROLL = 4;
__global__ void __launch_bounds__(DN_RUN)
densify_scatter_kernel(DnApplyArgs a)
{
    __shared__ DnCount wsum[4];
    __shared__ uint32_t s_keep[DN_RUN];                                  // the kept row, or DN_NO_ROW
    const uint32_t blk = blockIdx.x;
    const size_t first = (size_t)blk * DN_RUN;
    const int run = (int)((size_t)a.P - first < (size_t)DN_RUN ? (size_t)a.P - first : (size_t)DN_RUN);
    {
        const unsigned char c = (int)threadIdx.x < run ? a.cls[first + threadIdx.x] : (unsigned char)0;
        DnCount tot;
        const DnCount ex = dn_block_excl_scan(dn_of(c), &tot, wsum);
        const uint32_t row = a.sums[blk] + ex.kept;
        s_keep[threadIdx.x] = ((c & DN_KEEP) && row < a.n_kept) ? row : DN_NO_ROW;      // (row < n_kept: always, for the scratch of this plan)
    }
    __syncthreads();
    for (int gi = 0; gi < a.n_groups; gi++) {
        const DnGroup G = a.grp[gi];
        const int w = G.width, total = run * w, qstep = DN_RUN / w, rstep = DN_RUN % w;
        int r = (int)threadIdx.x / w, c = (int)threadIdx.x % w;
        // four elements per turn, the loads in front of the stores: src and dst may alias as far as the compiler knows, so a load behind a
        // store waits for it, and one load in flight per wave leaves the kernel bound by latency
        for (int e = threadIdx.x; e < total; e += DN_SCATTER_UNROLL * DN_RUN) {
            float v[DN_SCATTER_UNROLL];
            size_t o[DN_SCATTER_UNROLL];
#pragma unroll
            for (int u = 0; u < DN_SCATTER_UNROLL; u++) {
                v[u] = 0.0f;
                o[u] = (first + r) * (size_t)w + c;
                if (e + u * DN_RUN < total) {                            // (behind the run's end r may pass DN_RUN: nothing is read there)
                    const uint32_t row = s_keep[r];
                    if (row != DN_NO_ROW) v[u] = G.src[(size_t)row * w + c];
                }
                r += qstep; c += rstep;
                if (c >= w) { c -= w; r++; }
            }
#pragma unroll
            for (int u = 0; u < DN_SCATTER_UNROLL; u++)
                if (e + u * DN_RUN < total) G.dst[o[u]] = v[u];
        }
    }
}

// train.py:282-292 + add_densification_stats_grad (scene/saro_gaussian.py:745-750), where visibility_count[i] > 0:
//   accum += grad_is_mean ? grad[i] : grad[i] / visibility_count[i];  denom += 1;  max_radii = max(max_radii, radii)
__global__ void __launch_bounds__(256)
densify_stats_update_kernel(int P, const float* __restrict__ grad, const float* __restrict__ visibility_count, const float* __restrict__ radii,
                            float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_radii, int grad_is_mean)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float n = visibility_count[i];
    if (!(n > 0.0f)) return;
    accum[i] += grad_is_mean ? grad[i] : grad[i] / n;
    denom[i] += 1.0f;
    if (max_radii) max_radii[i] = fmaxf(max_radii[i], radii[i]);
}

} // namespace gsrast
