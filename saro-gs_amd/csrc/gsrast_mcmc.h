// gsrast_mcmc.h -- the second densification policy on the device: 3DGS-MCMC ("3D Gaussian Splatting as Markov Chain Monte Carlo") as
// gsplat's MCMCStrategy runs it.  Functions restated (gsplat/strategy/ops.py, gsplat/relocation.py):
//   relocate                   dead Gaussians become copies of alive ones sampled by opacity          -> mcmc_weights / _scan / _sample / _values / _apply<false>
//   sample_add                 n more Gaussians, copies of rows sampled by opacity                    -> the same chain with nothing dead, _apply<true>
//   compute_relocation         the opacity and scale a source and its copies share (N_MAX = 51)       -> mcmc_values_kernel
//   inject_noise_to_position   xyz += covariance-shaped noise, gated by opacity                       -> mcmc_noise_kernel
// Sampling is integer arithmetic from the fixed-point weights on: q_i = max(1, floor(sigmoid(opacity_i) * 2^24)) for an alive row, 0 for a
// dead one; draw d in [0, 2^62) targets t = floor(d * W / 2^62), W = sum q, and selects the smallest i whose inclusive prefix of q exceeds
// t.  Prefixes come from two-level scans (a 256-source run per workgroup, a single-workgroup carry pass), so a zero-weight row is never
// selected and the same draws select the same rows on every run and every rank.  No floating-point atomics; the one atomic is an integer
// add on the per-source draw count, whose result does not depend on order.  Every row of every group has exactly one writer.
// The ONE deliberate difference from gsplat's arithmetic: compute_relocation's alternating sum  denom = sum_i sum_k C(i-1, k) (-1)^k /
// sqrt(k+1) o'^(k+1)  is accumulated in fp64 over an fp64 binomial table (gsplat: an fp32 loop over an fp32 table).  Its terms reach
// about 10 where the result is about 0.1 (r = 51, o = 0.99): two digits in fp32, nothing in fp64.
// Moments: the sampled sources' exp_avg / exp_avg_sq become 0; a relocated dead row KEEPS its own moments -- the 3DGS-MCMC code and
// gsplat both reset the optimizer state at the sampled indices only, and this file leaves it that way.
#pragma once
#include "gsrast_gaussian.h"
#include <cfloat>

namespace gsrast {

constexpr int MC_RUN = 256;                  // consecutive rows per workgroup: the scans' first level, the sampler's inner search
constexpr int MC_MAX_GROUPS = 16, MC_MAX_WIDTH = 64;
constexpr int MC_N_MAX = 51;                 // gsplat/relocation.py: N_MAX
constexpr int MC_ROLE_COPY = 0, MC_ROLE_OPACITY = 1, MC_ROLE_SCALING = 2;
constexpr uint32_t MC_HDR_WORDS = 4;         // scratch header = counts: { n_dead, n_alive, W_lo, W_hi }

// Pascal's triangle up to row 51, exact in fp64 (C(51, 25) < 2^48), built at compile time.
struct McBinom { double c[MC_N_MAX + 1][MC_N_MAX + 1]; };
constexpr McBinom mc_make_binom()
{
    McBinom b{};
    for (int n = 0; n <= MC_N_MAX; n++) {
        b.c[n][0] = 1.0;
        for (int k = 1; k <= n; k++) b.c[n][k] = b.c[n - 1][k - 1] + (k <= n - 1 ? b.c[n - 1][k] : 0.0);
    }
    return b;
}
__constant__ const McBinom kMcBinom = mc_make_binom();

// Exclusive scan of one value per thread over a 256-thread workgroup; *total = the workgroup's sum.  `wsum`: 4 entries of LDS.
template <typename T>
__device__ __forceinline__ T mc_block_excl_scan(T v, T* total, T* wsum)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(inc, d, 64);
        if (lane >= (unsigned)d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const T s = wsum[w]; if (w < (int)wave) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// (a) One row per thread: dead flag, fixed-point weight, the weight's exclusive prefix inside the run (< 255 * 2^24: 32 bits), and the
// workgroup's two sums (the weights' in 64 bits: 256 rows of 2^24 are 2^32).  A NaN opacity is dead.
__global__ void __launch_bounds__(MC_RUN)
mcmc_weights_kernel(int P, const float* __restrict__ opacity_logit, const unsigned char* __restrict__ dead_src, float min_opacity,
                    uint32_t* __restrict__ weights_out, uint32_t* __restrict__ run_prefix, unsigned char* __restrict__ dead,
                    unsigned long long* __restrict__ wg_weight, uint32_t* __restrict__ wg_dead)
{
    __shared__ unsigned long long s64[4];
    __shared__ uint32_t s32[4];
    const size_t i = (size_t)blockIdx.x * MC_RUN + threadIdx.x;
    uint32_t q = 0, d = 0;
    if (i < (size_t)P) {
        const float o = 1.0f / (1.0f + expf(-opacity_logit[i]));
        d = (!(o > min_opacity) || (dead_src && dead_src[i] != 0)) ? 1u : 0u;
        if (!d) { q = (uint32_t)floorf(o * 16777216.0f); if (q < 1u) q = 1u; }
        weights_out[i] = q;
        dead[i] = (unsigned char)d;
    }
    unsigned long long tq; uint32_t td;
    const unsigned long long eq = mc_block_excl_scan<unsigned long long>(q, &tq, s64);
    (void)mc_block_excl_scan<uint32_t>(d, &td, s32);
    if (i < (size_t)P) run_prefix[i] = (uint32_t)eq;
    if (threadIdx.x == 0) { wg_weight[blockIdx.x] = tq; wg_dead[blockIdx.x] = td; }
}

// Single workgroup: both arrays of workgroup sums become exclusive prefixes in place (256 sums per turn, with a carry);
// counts = hdr = { n_dead, n_alive, W_lo, W_hi }.  nb = 0 (P = 0): zeros.
__global__ void __launch_bounds__(MC_RUN)
mcmc_scan_kernel(unsigned long long* __restrict__ wg_weight, uint32_t* __restrict__ wg_dead, uint32_t nb, uint32_t P,
                 uint32_t* __restrict__ hdr, uint32_t* __restrict__ counts)
{
    __shared__ unsigned long long s64[4];
    __shared__ uint32_t s32[4];
    unsigned long long cw = 0; uint32_t cd = 0;
    for (uint32_t c0 = 0; c0 < nb; c0 += MC_RUN) {
        const uint32_t b = c0 + threadIdx.x;
        const unsigned long long w = b < nb ? wg_weight[b] : 0ull;
        const uint32_t d = b < nb ? wg_dead[b] : 0u;
        unsigned long long tw; uint32_t td;
        const unsigned long long ew = mc_block_excl_scan<unsigned long long>(w, &tw, s64);
        const uint32_t ed = mc_block_excl_scan<uint32_t>(d, &td, s32);
        if (b < nb) { wg_weight[b] = cw + ew; wg_dead[b] = cd + ed; }
        cw += tw; cd += td;
    }
    if (threadIdx.x == 0) {
        const uint32_t lo = (uint32_t)(cw & 0xFFFFFFFFull), hi = (uint32_t)(cw >> 32);
        hdr[0] = cd; hdr[1] = P - cd; hdr[2] = lo; hdr[3] = hi;
        counts[0] = cd; counts[1] = P - cd; counts[2] = lo; counts[3] = hi;
    }
}

// (b) One draw per thread.  t = floor(d * W / 2^62) < W is the high word of the 128-bit product (d << 2) * W.  The workgroup holding t is
// the LAST one whose exclusive prefix is <= t (a workgroup of weight 0 shares its prefix with its successor, so it is never the last);
// the same rule inside the run finds the row.  W = 0: no row can be selected, src = -1.
__global__ void __launch_bounds__(MC_RUN)
mcmc_sample_kernel(int P, int n, const long long* __restrict__ draws, const uint32_t* __restrict__ hdr,
                   const unsigned long long* __restrict__ wg_prefix, uint32_t nb, const uint32_t* __restrict__ run_prefix,
                   int* __restrict__ src, uint32_t* __restrict__ count)
{
    const size_t j = (size_t)blockIdx.x * MC_RUN + threadIdx.x;
    if (j >= (size_t)n) return;
    const unsigned long long W = (unsigned long long)hdr[2] | ((unsigned long long)hdr[3] << 32);
    if (W == 0ull || nb == 0u) { src[j] = -1; return; }
    const unsigned long long d = (unsigned long long)draws[j] & ((1ull << 62) - 1ull);      // (in range by contract; the mask keeps a foreign value in bounds)
    const unsigned long long t = __umul64hi(d << 2, W);
    uint32_t lo = 0, hi = nb - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (wg_prefix[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const uint32_t r = (uint32_t)(t - wg_prefix[lo]);                                      // < the workgroup's weight <= 2^32
    const size_t first = (size_t)lo * MC_RUN;
    const uint32_t len = (uint32_t)((size_t)P - first < (size_t)MC_RUN ? (size_t)P - first : (size_t)MC_RUN);
    uint32_t a = 0, b = len - 1;
    while (a < b) {
        const uint32_t mid = a + (b - a + 1) / 2;
        if (run_prefix[first + mid] <= r) a = mid; else b = mid - 1;
    }
    const size_t i = first + a;
    src[j] = (int)i;
    atomicAdd(&count[i], 1u);
}

// (c) compute_relocation for every source with count > 0, from the pre-call opacity and scaling, in fp64:
//   r = min(count + 1, 51);  o' = 1 - (1 - o)^(1/r);  denom = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1)
//   s' = (o / denom) exp(scaling);  o' clamped to [min_opacity, 1 - FLT_EPSILON];  vals[i] = { logit(o'), log(s'_0), log(s'_1), log(s'_2) }
// The double sum is taken with k outside: sum_{i=k+1..r} C(i-1, k) = C(r, k+1), an integer the table holds exactly, so the r(r+1)/2 terms
// of the formula are r multiply-adds.
__global__ void __launch_bounds__(MC_RUN)
mcmc_values_kernel(int P, const uint32_t* __restrict__ count, const float* __restrict__ opacity_logit, const float* __restrict__ scaling,
                   float min_opacity, float* __restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * MC_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const uint32_t n = count[i];
    if (n == 0u) return;
    const int r = n + 1u < (uint32_t)MC_N_MAX ? (int)(n + 1u) : MC_N_MAX;
    const double o = 1.0 / (1.0 + exp(-(double)opacity_logit[i]));
    double on = -expm1(log1p(-o) / (double)r);
    double denom = 0.0, pw = on;                    // pw = (-1)^k o'^(k+1)
    for (int k = 0; k < r; k++) {
        denom += kMcBinom.c[r][k + 1] * (pw / sqrt((double)(k + 1)));
        pw *= -on;
    }
    const double coeff = o / denom;
    on = fmin(fmax(on, (double)min_opacity), 1.0 - (double)FLT_EPSILON);
    vals[4 * i] = (float)log(on / (1.0 - on));
#pragma unroll
    for (int c = 0; c < 3; c++) vals[4 * i + 1 + c] = (float)log(coeff * exp((double)scaling[3 * i + c]));
}

struct McGroup { const float *src, *src_m, *src_v; float *dst, *dst_m, *dst_v; int width, role; };
struct McApplyArgs {
    McGroup grp[MC_MAX_GROUPS];
    int n_groups, P, n;
    const int* src;                  // [n] sampled source per draw
    const uint32_t* count;           // [P] draws per source
    const float* vals;               // [P][4] new opacity logit and log-scales of the sources
    const unsigned char* dead;       // [P]                          (relocate)
    const uint32_t* wg_dead;         // [nb] exclusive dead prefixes (relocate)
};

// (d) GROW = false, in place (dst only): the j-th dead row in index order becomes a copy of row src[j], with the source's new opacity and
// scaling; a sampled source takes its new opacity and scaling and zero moments; every other row is left alone.  A dead row reads only
// what no thread writes (an alive row's COPY groups, and `vals`), so the result does not depend on the order of the workgroups.
// (e) GROW = true, src -> dst of P + n rows: rows [0, P) are copies with their moments, sampled sources with the new opacity and scaling;
// row P + j is a copy of the updated row src[j] with zero moments.
// A workgroup takes MC_RUN consecutive destination rows; consecutive lanes take consecutive floats of a group's run.
template <bool GROW>
__global__ void __launch_bounds__(MC_RUN)
mcmc_apply_kernel(McApplyArgs a)
{
    __shared__ uint32_t s32[4];
    __shared__ int s_from[MC_RUN];           // the row this one copies (-1: none)
    __shared__ unsigned char s_kind[MC_RUN]; // 0 untouched | 1 copy of s_from, own moments kept / zero (GROW) | 2 sampled source | 3 plain copy (GROW)
    const size_t first = (size_t)blockIdx.x * MC_RUN;
    const size_t rows = (size_t)a.P + (GROW ? (size_t)a.n : 0);
    const int run = (int)(rows - first < (size_t)MC_RUN ? rows - first : (size_t)MC_RUN);
    {
        const size_t i = first + threadIdx.x;
        int from = -1; unsigned char kind = 0;
        if (GROW) {
            if ((int)threadIdx.x < run) {
                if (i < (size_t)a.P) { from = (int)i; kind = a.count[i] > 0u ? 2 : 3; }
                else { from = a.src[i - (size_t)a.P]; kind = 1; }
            }
        } else {
            const uint32_t d = ((int)threadIdx.x < run && a.dead[i]) ? 1u : 0u;
            uint32_t td;
            const uint32_t j = a.wg_dead[blockIdx.x] + mc_block_excl_scan<uint32_t>(d, &td, s32);
            if (d) { if (j < (uint32_t)a.n) { from = a.src[j]; kind = 1; } }
            else if ((int)threadIdx.x < run && a.count[i] > 0u) { from = (int)i; kind = 2; }
        }
        if (kind == 1 && (uint32_t)from >= (uint32_t)a.P) { from = -1; kind = 0; }      // (never, for the src of this plan: a guard against a foreign one)
        s_from[threadIdx.x] = from; s_kind[threadIdx.x] = kind;
    }
    __syncthreads();
    for (int gi = 0; gi < a.n_groups; gi++) {
        const McGroup G = a.grp[gi];
        const int w = G.width, total = run * w, qstep = MC_RUN / w, rstep = MC_RUN % w;
        int r = (int)threadIdx.x / w, c = (int)threadIdx.x % w;
        for (int e = threadIdx.x; e < total; e += MC_RUN) {
            const unsigned char k = s_kind[r];
            if (k != 0) {
                const size_t from = (size_t)s_from[r];
                const size_t o = (first + r) * (size_t)w + c, so = from * (size_t)w + c;
                const bool fresh = G.role != MC_ROLE_COPY && k != 3;          // the value comes from `vals`
                if (fresh) G.dst[o] = a.vals[4 * from + (G.role == MC_ROLE_OPACITY ? 0 : 1 + c)];
                else if (GROW || k == 1) G.dst[o] = G.src[so];
                if (GROW) {
                    if (G.dst_m) G.dst_m[o] = k == 1 ? 0.0f : G.src_m[so];
                    if (G.dst_v) G.dst_v[o] = k == 1 ? 0.0f : G.src_v[so];
                } else if (k == 2) {
                    if (G.dst_m) G.dst_m[o] = 0.0f;
                    if (G.dst_v) G.dst_v[o] = 0.0f;
                }
            }
            r += qstep; c += rstep;
            if (c >= w) { c -= w; r++; }
        }
    }
}

// (f) inject_noise_to_position, one Gaussian per thread, in place:
//   xyz += Sigma (noise * gate * scale [* row_scale]),  Sigma = R diag(exp(scaling))^2 R^T,  R = R(q / |q|) as dn_split_offset builds it,
//   gate = 1 / (1 + exp(-k ((1 - o) - x0))),  1 - o = 1 / (1 + exp(opacity_logit)).
// 56 B read and 12 B written per row; the quaternion is one 16-byte load.
__global__ void __launch_bounds__(MC_RUN)
mcmc_noise_kernel(int P, float* __restrict__ xyz, const float4* __restrict__ rotation, const float* __restrict__ scaling,
                  const float* __restrict__ opacity_logit, const float* __restrict__ noise, const float* __restrict__ row_scale,
                  float scale, float k, float x0)
{
    const size_t i = (size_t)blockIdx.x * MC_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float4 q4 = rotation[i];
    float r = q4.x, x = q4.y, y = q4.z, z = q4.w;
    const float norm = sqrtf(r * r + x * x + y * y + z * z);
    r /= norm; x /= norm; y /= norm; z /= norm;
    const float qn[4] = { r, x, y, z };
    M3 R;
    quat_to_R(qn, R);      // R.m[i][j]: row i, column j of build_rotation
    const float one_minus_o = 1.0f / (1.0f + expf(opacity_logit[i]));
    float g = scale / (1.0f + expf(-k * (one_minus_o - x0)));
    if (row_scale) g *= row_scale[i];
    const float v0 = noise[3 * i] * g, v1 = noise[3 * i + 1] * g, v2 = noise[3 * i + 2] * g;
    const float e0 = expf(scaling[3 * i]), e1 = expf(scaling[3 * i + 1]), e2 = expf(scaling[3 * i + 2]);
    const float t0 = (R.m[0][0] * v0 + R.m[1][0] * v1 + R.m[2][0] * v2) * (e0 * e0);      // diag(s)^2 R^T v
    const float t1 = (R.m[0][1] * v0 + R.m[1][1] * v1 + R.m[2][1] * v2) * (e1 * e1);
    const float t2 = (R.m[0][2] * v0 + R.m[1][2] * v1 + R.m[2][2] * v2) * (e2 * e2);
    xyz[3 * i] += R.m[0][0] * t0 + R.m[0][1] * t1 + R.m[0][2] * t2;
    xyz[3 * i + 1] += R.m[1][0] * t0 + R.m[1][1] * t1 + R.m[1][2] * t2;
    xyz[3 * i + 2] += R.m[2][0] * t0 + R.m[2][1] * t1 + R.m[2][2] * t2;
}

} // namespace gsrast
