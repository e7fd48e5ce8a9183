// gsrast_adam.h -- Adam step for the per-Gaussian parameter groups with a PER-ROW learning rate, all groups in one
// launch (third item).  Reference behaviour restated (paths relative to /root/reference/):
//   scene/saro_gaussian.py:306-323  param groups xyz / f_dc / f_rest / opacity / scaling / rotation / temporal_pos,
//                                   torch.optim.Adam(l, lr=0.0, eps=1e-15, fused=True)
//   scene/saro_gaussian.py:345-398  update_learning_rate: param_group['lr'] = lr * self.inv_intergral -- a [P,1] tensor,
//                                   i.e. one learning rate per Gaussian (row)
// torch.optim.Adam (amsgrad=False, maximize=False, weight_decay=0), step t = 1, 2, ...:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// Traffic per element: p, g, m, v in, p, m, v out = 28 B; 60 floats per Gaussian = 1.68 kB per Gaussian and step.
//
// adam_step_visible_kernel: the same step for the rows a mask names (upstream 3DGS's SparseGaussianAdam, gsplat's SelectiveAdam,
// torch.optim.SparseAdam): a row nobody saw keeps p, m, v bit for bit, and neither its g nor its lr_rows entry is loaded.  A wave owns 64
// consecutive rows of a group, ballots their mask entries into one 64-bit word and leaves at once when it is zero -- an unseen run of 64
// rows costs its 64 mask entries.  Otherwise the wave walks the run's 64 x width floats, consecutive lanes on consecutive float4s, every
// load and store predicated on the row's bit.  Requests are 128 B: a narrow group (width 1-4: 8-32 rows per line) at a random 22 %
// visibility still touches nearly every line; the saving is f_rest's (180 B per row, 75 % of the bytes) and that of whole unseen runs.
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int ADAM_MAX_GROUPS = 8;
struct AdamGroup {
    float* p; const float* g; float* m; float* v;
    const float* lr_rows;       // [rows] per-row learning rate, or null
    float lr;                   // scalar learning rate (multiplied with lr_rows[i] when that is given)
    unsigned width;             // floats per row
    unsigned long long n;       // rows * width
    unsigned long long first_block, n_blocks;   // this group's slice of the grid
};
struct AdamArgs { AdamGroup grp[ADAM_MAX_GROUPS]; int n_groups; float b1, b2, omb1, omb2, eps, inv_bc1, inv_sqrt_bc2; };   // omb = 1 - beta, rounded once from fp64 (1 - 0.999f is off by 5e-5)

constexpr int ADAM_THREADS = 256, ADAM_PER_THREAD = 4;
constexpr int ADAM_VIS_ROWS = 64;                                   // rows per wave of adam_step_visible_kernel: one bit each of the ballot
constexpr int ADAM_VIS_ROWS_PER_BLOCK = ADAM_VIS_ROWS * (ADAM_THREADS / 64);
constexpr unsigned ADAM_VIS_MAX_WIDTH = 1u << 24;                   // 64 x width stays a 32-bit index inside a run

// one element's update, shared by both kernels (an all-true mask reproduces the dense step bit for bit); row indexes lr_rows
__device__ __forceinline__ void adam_update(const AdamArgs& a, float lr, const float* lr_rows, unsigned long long row, float& p, float g, float& m, float& v)
{
    if (lr_rows) lr *= lr_rows[row];
    m = a.b1 * m + a.omb1 * g;
    v = a.b2 * v + a.omb2 * g * g;
    const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    p -= (lr * a.inv_bc1) * (m / denom);
}

__global__ void __launch_bounds__(ADAM_THREADS)
adam_step_kernel(AdamArgs a)
{
    int gi = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MAX_GROUPS; k++) if (k < a.n_groups && blockIdx.x >= a.grp[k].first_block) gi = k;
    const AdamGroup G = a.grp[gi];
    const unsigned long long e0 = ((unsigned long long)(blockIdx.x - G.first_block) * ADAM_THREADS + threadIdx.x) * ADAM_PER_THREAD;
    if (e0 >= G.n) return;
    const bool vec = e0 + ADAM_PER_THREAD <= G.n && ((((uintptr_t)G.p | (uintptr_t)G.g | (uintptr_t)G.m | (uintptr_t)G.v) & 15) == 0);
    float p[4], g[4], m[4], v[4];
    const int cnt = (int)((G.n - e0) < (unsigned long long)ADAM_PER_THREAD ? (G.n - e0) : ADAM_PER_THREAD);
    if (vec) {
        const float4 P4 = *reinterpret_cast<const float4*>(G.p + e0), G4 = *reinterpret_cast<const float4*>(G.g + e0);
        const float4 M4 = *reinterpret_cast<const float4*>(G.m + e0), V4 = *reinterpret_cast<const float4*>(G.v + e0);
        p[0] = P4.x; p[1] = P4.y; p[2] = P4.z; p[3] = P4.w; g[0] = G4.x; g[1] = G4.y; g[2] = G4.z; g[3] = G4.w;
        m[0] = M4.x; m[1] = M4.y; m[2] = M4.z; m[3] = M4.w; v[0] = V4.x; v[1] = V4.y; v[2] = V4.z; v[3] = V4.w;
    } else {
        for (int k = 0; k < cnt; k++) { p[k] = G.p[e0 + k]; g[k] = G.g[e0 + k]; m[k] = G.m[e0 + k]; v[k] = G.v[e0 + k]; }
    }
#pragma unroll
    for (int k = 0; k < ADAM_PER_THREAD; k++) {
        if (k >= cnt) break;
        adam_update(a, G.lr, G.lr_rows, G.lr_rows ? (e0 + k) / G.width : 0ull, p[k], g[k], m[k], v[k]);
    }
    if (vec) {
        *reinterpret_cast<float4*>(G.p + e0) = make_float4(p[0], p[1], p[2], p[3]);
        *reinterpret_cast<float4*>(G.m + e0) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(G.v + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < cnt; k++) { G.p[e0 + k] = p[k]; G.m[e0 + k] = m[k]; G.v[e0 + k] = v[k]; }
    }
}

// visible: [rows] bytes (non-zero = visible) or int32 (> 0 = visible: a render's radii), elem_bytes 1 or 4.  Grid: per group
// ceil(rows / ADAM_VIS_ROWS_PER_BLOCK) blocks (AdamGroup::first_block); every group has `rows` rows and width <= ADAM_VIS_MAX_WIDTH.
__global__ void __launch_bounds__(ADAM_THREADS)
adam_step_visible_kernel(AdamArgs a, const void* __restrict__ visible, int elem_bytes, unsigned rows)
{
    int gi = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MAX_GROUPS; k++) if (k < a.n_groups && blockIdx.x >= a.grp[k].first_block) gi = k;
    const AdamGroup& G = a.grp[gi];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long r0l = ((unsigned long long)(blockIdx.x - G.first_block) * (ADAM_THREADS / 64) + (threadIdx.x >> 6)) * ADAM_VIS_ROWS;
    if (r0l >= rows) return;
    const unsigned r0 = (unsigned)r0l;
    bool vis = false;
    if (r0 + lane < rows)
        vis = elem_bytes == 4 ? reinterpret_cast<const int*>(visible)[r0 + lane] > 0 : reinterpret_cast<const unsigned char*>(visible)[r0 + lane] != 0;
    const unsigned long long mask = __ballot(vis);       // bit r: row r0 + r is visible (wave-uniform)
    if (mask == 0) return;

    const unsigned width = G.width;
    const unsigned n_run = (rows - r0 < (unsigned)ADAM_VIS_ROWS ? rows - r0 : (unsigned)ADAM_VIS_ROWS) * width;      // floats of this wave's run
    // the run starts r0 * width floats in, a multiple of 64 floats: a float4 inside it is aligned whenever the pointers are (the dense kernel's condition)
    const bool aligned = ((((uintptr_t)G.p | (uintptr_t)G.g | (uintptr_t)G.m | (uintptr_t)G.v) & 15) == 0);
    const unsigned long long base = (unsigned long long)r0 * width;
    float* __restrict__ const P = G.p + base; const float* __restrict__ const Gr = G.g + base;
    float* __restrict__ const M = G.m + base; float* __restrict__ const V = G.v + base;
    const float* const lr_rows = G.lr_rows ? G.lr_rows + r0 : nullptr;
    // (row, rem) of element j = lane * 4 + 256 * iteration inside the run, advanced without a division per element
    const unsigned dq = (64 * ADAM_PER_THREAD) / width, dr = (64 * ADAM_PER_THREAD) % width;
    unsigned row = (lane * ADAM_PER_THREAD) / width, rem = lane * ADAM_PER_THREAD - row * width;
    for (unsigned j = lane * ADAM_PER_THREAD; j < n_run; j += 64 * ADAM_PER_THREAD) {
        const unsigned cnt = n_run - j < (unsigned)ADAM_PER_THREAD ? n_run - j : (unsigned)ADAM_PER_THREAD;
        unsigned rk[ADAM_PER_THREAD], bits = 0;
        {
            unsigned r = row, m_ = rem;
#pragma unroll
            for (int k = 0; k < ADAM_PER_THREAD; k++) {
                rk[k] = r;
                if ((unsigned)k < cnt) bits |= (unsigned)((mask >> r) & 1ull) << k;      // (k < cnt: r < 64)
                if (++m_ == width) { m_ = 0; r++; }
            }
        }
        if (bits == 15u && aligned) {
            const float4 P4 = *reinterpret_cast<const float4*>(P + j), G4 = *reinterpret_cast<const float4*>(Gr + j);
            const float4 M4 = *reinterpret_cast<const float4*>(M + j), V4 = *reinterpret_cast<const float4*>(V + j);
            float p[4] = { P4.x, P4.y, P4.z, P4.w }, g[4] = { G4.x, G4.y, G4.z, G4.w }, m[4] = { M4.x, M4.y, M4.z, M4.w }, v[4] = { V4.x, V4.y, V4.z, V4.w };
#pragma unroll
            for (int k = 0; k < ADAM_PER_THREAD; k++) adam_update(a, G.lr, lr_rows, rk[k], p[k], g[k], m[k], v[k]);
            *reinterpret_cast<float4*>(P + j) = make_float4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<float4*>(M + j) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4*>(V + j) = make_float4(v[0], v[1], v[2], v[3]);
        } else if (bits) {
            // a float4 that straddles a visible and an invisible row, the run's tail, or unaligned pointers: element by element, invisible ones untouched
#pragma unroll
            for (int k = 0; k < ADAM_PER_THREAD; k++) {
                if (!((bits >> k) & 1u)) continue;
                float p = P[j + k], m = M[j + k], v = V[j + k];
                adam_update(a, G.lr, lr_rows, rk[k], p, Gr[j + k], m, v);
                P[j + k] = p; M[j + k] = m; V[j + k] = v;
            }
        }
        row += dq; rem += dr;
        if (rem >= width) { rem -= width; row++; }
    }
}

} // namespace gsrast
