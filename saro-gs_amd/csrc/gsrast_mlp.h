// gsrast_mlp.h -- the deformation heads of the dynamic stage as ONE kernel each way: Linear -> ReLU -> Linear -> ReLU -> Linear [-> Sigmoid]
// over N rows, fp32 throughout, on the f32-input matrix instruction v_mfma_f32_32x32x2_f32 (an exact k-ordered fmaf chain: the numerics of
// an fp32 nn.Linear, in another summation order).  Shapes: D_in = D_x + D_tail in [1, 64], H1, H2 in {32, 64, 96, 128}, D_out in [1, 64];
// weights in nn.Linear's [out][in] layout.
//
// Orientation.  Every product is computed TRANSPOSED, rows of the batch on the lanes:  H1^T [H1 x rows] = W1 [H1 x D_in] . X^T [D_in x rows].
// The weight is the A operand (lane l holds A[l & 31][k]), the activation the B operand (lane l holds B[k][l & 31], l & 31 = the row of the
// batch), and the 32 x 32 result has the row of the batch on the lane and 16 features in the registers (feature = (r & 3) + 8 (r >> 2) +
// 4 (l >> 5)).  Within a block of 8 k the lane half h = l >> 5 takes k = 4 h + t at step t, for both operands: a permutation of the sum's
// order that lets a lane fetch its four weights of the block as one 16-byte load.
//
// Tile and work split.  A workgroup (256 threads, 4 waves) loops over tiles of 64 rows: tile = blockIdx.x, blockIdx.x + gridDim.x, ...
// A layer's output [features x 64] is cut into 32 x 32 items (feature tile, row half); the items go round the 4 waves.
//
// LDS budget (160 KiB per CU, one workgroup per CU).  The three weight matrices are at most 128 KB and an activation tile is 32.5 KB per
// 128 features, so both do not fit beside the backward's five tiles.  What stays on chip is what is WRITTEN: the activation tiles, as
// [feature][64 rows + 1] fp32 images (stride 65: a lane per row reads a k-row without bank conflicts, and a lane per feature -- the weight
// gradient's operands -- reads along the rows without conflicts too).  What is only READ streams: the weights come from L2 / L1 straight
// into the A operand's register (at most 128 KB, resident in L2 for the whole launch), one block of 8 k ahead of the MFMAs that use it.
//   forward    x 8 ceil(D_in / 8) x 65 + h1 128 x 65 + h2 128 x 65 floats                           <= 83 200 B
//              (79 040 B at D_in = 41: two workgroups per CU, 2 waves per SIMD; the forward launches two workgroups per CU)
//   backward   x 64 x 65 + dz 64 x 65 + h1 128 x 65 + h2 128 x 65 (dh1 reuses it) + dh2 128 x 65    = 133 120 B
// h1 and h2 never reach global memory, in either direction.
//
// The backward RECOMPUTES h1 and h2 from x.  Saving them would be N x (H1 + H2) x 4 B = 1 GB per evaluation at 1 M rows x 128 x 2, and the
// reference evaluates up to seven heads per view; recomputing is 2 x 1 M x (41 x 128 + 128 x 128) = 43 GFLOP (55 GFLOP with the sigmoid
// head's third layer), about 0.3 ms at the 155 TFLOP/s f32-MFMA peak -- what writing 1 GB and reading it back costs at 6-7 TB/s, without
// the 1 GB.  The sigmoid head reads y (N x D_out) instead of recomputing the third layer.
//
// ONE kernel does the whole backward (the single-kernel form, as a chain of launches): per tile, h1, h2, dz = dy [* y (1 - y)],
// dh2 = (W3^T dz) [h2 > 0], dh1 = (W2^T dh2) [h1 > 0], dx = (W1^T dh1)[:D_x], and dW3 += dz h2^T, dW2 += dh2 h1^T, dW1 += dh1 x^T,
// db_l += sum over rows.  The weight gradients stay in the accumulator registers across all of the workgroup's tiles of a launch: dW2 is
// 16 items of 32 x 32 = 4 per wave, dW1 and dW3 at most 8 = 2 per wave, 128 registers per lane of the 512 a wave has at one wave per SIMD.
// A launch covers at most 8 tiles (512 rows) per workgroup and stores (the launches behind the first: adds) each workgroup's accumulators
// to its slab of scratch, so no fp32 chain is longer than 512 rows; the host issues ceil(N / (512 workgroups)) launches -- 8 at 1 M rows
// on 256 workgroups; the count grows with N, and with a forced small workgroup count (a test's device) it grows large.
// mlp3_reduce_kernel sums the slabs in workgroup order, in fp64: no floating-point atomics, and with the same workgroup count the weight
// gradients are bit-identical from run to run.  Scratch = workgroups x (|W1| + |b1| + |W2| + |b2| + |W3| + |b3|) floats, independent of N.
//
// NaN: a ReLU passes a NaN pre-activation on (v < 0 ? 0 : v) and its backward passes the gradient where the activation is NaN
// (h <= 0 ? 0 : g), as torch.relu and its threshold_backward do: a diverged head shows NaN where the nn.Sequential would.
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int MLP_TR = 64;                   // rows of the batch per tile
constexpr int MLP_LD = MLP_TR + 1;           // floats per feature row of an LDS image
constexpr int MLP_THREADS = 256;
constexpr int MLP_FLUSH_TILES = 8;           // backward: tiles per workgroup and launch (the length of a weight-gradient accumulator's chain)
constexpr int MLP_MAX_IO = 64, MLP_MAX_H = 128;
constexpr int MLP_FWD_LDS = (MLP_MAX_IO + 2 * MLP_MAX_H) * MLP_LD * 4;
constexpr int MLP_BWD_LDS = (2 * MLP_MAX_IO + 3 * MLP_MAX_H) * MLP_LD * 4;
constexpr int MLP_NEED_DX = 1, MLP_NEED_L1 = 2, MLP_NEED_L2 = 4, MLP_NEED_L3 = 8;      // Mlp3Args::need

typedef float mlp_f32x16 __attribute__((ext_vector_type(16)));

struct Mlp3Args {
    long long n;
    int d_x, d_tail, d_in, h1, h2, d_out, sigmoid, need;
    const float *x, *x_tail, *w1, *b1, *w2, *b2, *w3, *b3;
    float* y;             // forward: written; backward (sigmoid head): read
    const float* dy;
    float* dx;
    float* partial;       // backward: [workgroups][mlp3_param_floats]
    long long tile0, tile_end;      // backward: this launch's tiles
    int add;              // backward: 0 = store the partial, 1 = add onto it (a launch behind the first)
};

__host__ __device__ inline size_t mlp3_param_floats(int d_in, int h1, int h2, int d_out)
{
    return (size_t)h1 * d_in + h1 + (size_t)h2 * h1 + h2 + (size_t)d_out * h2 + d_out;
}

__device__ __forceinline__ int mlp_feat(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }      // row of the 32 x 32 result in register r of lane half h

// acc [32 x 32] = A [m0 .. m0 + 32) x [0, K) . S [K][64-row image](:, col0 .. col0 + 32), A(m, k) = TRANS ? W[k * ld + m] : W[m * ld + k],
// 0 where m >= M or k >= K.  S rows [K, round-up-to-8 K) must hold finite values.  The loads are unconditional from a clamped address and
// masked afterwards (a branch round each load would wait for every one of them singly).
template <bool TRANS>
__device__ __forceinline__ void mlp_load_a(float (&a)[4], const float* __restrict__ W, int ld, int M, int K, int m, int k0, bool vec)
{
    const int mc = min(m, M - 1);
    if (!TRANS && vec) {      // (K a multiple of 8, rows 16-byte aligned: the whole block of 4 is inside the row)
        const float4 v = *reinterpret_cast<const float4*>(W + (size_t)mc * ld + k0);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int kc = min(k0 + t, K - 1);
            a[t] = TRANS ? W[(size_t)kc * ld + mc] : W[(size_t)mc * ld + kc];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) a[t] = (m < M && k0 + t < K) ? a[t] : 0.0f;
}

template <bool TRANS>
__device__ __forceinline__ mlp_f32x16 mlp_gemm_w(const float* __restrict__ W, int ld, int M, int K, int m0, const float* S, int col0, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const int m = m0 + i;
    const bool vec = !TRANS && (K & 7) == 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    const int Kp = (K + 7) & ~7;
    mlp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    float a[4], an[4];
    mlp_load_a<TRANS>(a, W, ld, M, K, m, 4 * h, vec);
    for (int kb = 0; kb < Kp; kb += 8) {
        const int kn = kb + 8 < Kp ? kb + 8 : kb;      // (the last block loads itself again: no branch round the loads)
        mlp_load_a<TRANS>(an, W, ld, M, K, m, kn + 4 * h, vec);
        const float* s = S + (kb + 4 * h) * MLP_LD + col0 + i;
#pragma unroll
        for (int t = 0; t < 4; t++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], s[t * MLP_LD], acc, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; t++) a[t] = an[t];
    }
    return acc;
}

// acc [32 x 32] += G [g0 .. g0 + 32)(:, 64 rows) . A [a0 .. a0 + 32)(:, 64 rows)^T: the sum over the tile's rows (both operands from LDS images).
__device__ __forceinline__ void mlp_wgrad(mlp_f32x16& acc, const float* G, int g0, const float* A, int a0, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const float* g = G + (g0 + i) * MLP_LD + h;
    const float* a = A + (a0 + i) * MLP_LD + h;
#pragma unroll 8
    for (int k = 0; k < MLP_TR; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g[k], a[k], acc, 0, 0, 0);
}

// x (and the tail behind its columns) of one tile -> S[f][r]; rows past n are 0
__device__ __forceinline__ void mlp_stage_rows(float* S, const float* __restrict__ src, int width, int f0, long long row0, long long n, int tid)
{
    const long long base = row0 * width, end = n * width;
    for (int idx = tid; idx < MLP_TR * width; idx += MLP_THREADS) {
        const int r = idx / width, f = idx - r * width;
        S[(f0 + f) * MLP_LD + r] = base + idx < end ? src[base + idx] : 0.0f;
    }
}

// hidden layer: Sout[f][row] = relu(W . Sin + b)
__device__ __forceinline__ void mlp_hidden(const float* __restrict__ W, const float* __restrict__ b, int M, int K, const float* Sin, float* Sout, int wave, int lane)
{
    const int n_items = (M >> 5) * 2;
    for (int q = wave; q < n_items; q += 4) {
        const int m0 = (q >> 1) * 32, col0 = (q & 1) * 32;
        const mlp_f32x16 acc = mlp_gemm_w<false>(W, K, M, K, m0, Sin, col0, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = m0 + mlp_feat(r, lane >> 5);
            const float v = acc[r] + b[f];
            Sout[f * MLP_LD + col0 + (lane & 31)] = v < 0.0f ? 0.0f : v;      // (a NaN stays a NaN, as torch.relu)
        }
    }
}

// dSout[f][row] = (W^T . Sg)[f][row] where Sh[f][row] > 0, else 0  (W [K_out][M] row-major: the layer's own weight)
__device__ __forceinline__ void mlp_dgrad_hidden(const float* __restrict__ W, int M, int K, const float* Sg, const float* Sh, float* Sout, int wave, int lane)
{
    const int n_items = (M >> 5) * 2;
    for (int q = wave; q < n_items; q += 4) {
        const int m0 = (q >> 1) * 32, col0 = (q & 1) * 32;
        const mlp_f32x16 acc = mlp_gemm_w<true>(W, M, M, K, m0, Sg, col0, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int at = (m0 + mlp_feat(r, lane >> 5)) * MLP_LD + col0 + (lane & 31);
            Sout[at] = Sh[at] <= 0.0f ? 0.0f : acc[r];      // (h = NaN passes the gradient, as threshold_backward)
        }
    }
}

__device__ __forceinline__ void mlp_zero(float* S, int floats, int tid)
{
    for (int k = tid; k < floats; k += MLP_THREADS) S[k] = 0.0f;
}

__global__ void __launch_bounds__(MLP_THREADS) mlp3_fwd_kernel(const Mlp3Args a)
{
    extern __shared__ float mlp_lds[];
    const int kx = (a.d_in + 7) & ~7;
    float* Sx = mlp_lds;                                   // [kx][65]   (rows d_in .. kx - 1 stay 0)
    float* Sh1 = Sx + kx * MLP_LD;                         // [h1][65]
    float* Sh2 = Sh1 + a.h1 * MLP_LD;                      // [h2][65]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_tiles = (a.n + MLP_TR - 1) / MLP_TR;
    mlp_zero(Sx, kx * MLP_LD, tid);
    __syncthreads();
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * MLP_TR;
        mlp_stage_rows(Sx, a.x, a.d_x, 0, row0, a.n, tid);
        if (a.d_tail) mlp_stage_rows(Sx, a.x_tail, a.d_tail, a.d_x, row0, a.n, tid);
        __syncthreads();
        mlp_hidden(a.w1, a.b1, a.h1, a.d_in, Sx, Sh1, wave, lane);
        __syncthreads();
        mlp_hidden(a.w2, a.b2, a.h2, a.h1, Sh1, Sh2, wave, lane);
        __syncthreads();
        const int n_items = ((a.d_out + 31) >> 5) * 2;
        for (int q = wave; q < n_items; q += 4) {
            const int m0 = (q >> 1) * 32, col0 = (q & 1) * 32;
            const mlp_f32x16 acc = mlp_gemm_w<false>(a.w3, a.h2, a.d_out, a.h2, m0, Sh2, col0, lane);
            const long long row = row0 + col0 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int f = m0 + mlp_feat(r, lane >> 5);
                if (f < a.d_out && row < a.n) {
                    float v = acc[r] + a.b3[f];
                    if (a.sigmoid) v = 1.0f / (1.0f + expf(-v));
                    a.y[row * a.d_out + f] = v;
                }
            }
        }
        // (the next tile's staging writes Sx, last read before the previous barrier; Sh1 / Sh2 are rewritten behind later barriers)
    }
}

// one wave's share of a weight gradient's 32 x 32 items: item q = wave + 4 t covers (q / n_i, q % n_i)
template <int T>
__device__ __forceinline__ void mlp_wgrad_items(mlp_f32x16 (&acc)[T], int n_o, int n_i, const float* G, const float* A, int wave, int lane)
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int q = wave + 4 * t;
        if (q < n_o * n_i) mlp_wgrad(acc[t], G, (q / n_i) * 32, A, (q % n_i) * 32, lane);
    }
}

// acc -> the workgroup's partial (add: onto what an earlier launch left there; the same lane owns the same element every time)
template <int T>
__device__ __forceinline__ void mlp_flush_partial(mlp_f32x16 (&acc)[T], int n_o, int n_i, int M, int K, float* out, bool add, int wave, int lane)
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int q = wave + 4 * t;
        if (q < n_o * n_i) {
            const int in = (q % n_i) * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int o = (q / n_i) * 32 + mlp_feat(r, lane >> 5);
                if (o < M && in < K) {
                    float* at = out + (size_t)o * K + in;
                    *at = add ? *at + acc[t][r] : acc[t][r];
                }
            }
        }
    }
}

// The bias gradients are plain sums over all rows, terms of either sign: they are kept in fp64 (192 adds per thread and tile beside ~500 MFMAs
// per wave) and rounded once, into the workgroup's partial.
__device__ __forceinline__ double mlp_row_sum(const float* S, int f)
{
    double s = 0.0;
    for (int r = 0; r < MLP_TR; r++) s += (double)S[f * MLP_LD + r];
    return s;
}

__global__ void __launch_bounds__(MLP_THREADS) mlp3_bwd_kernel(const Mlp3Args a)
{
    extern __shared__ float mlp_lds[];
    float* Sx = mlp_lds;                                   // [64][65]   x^T            (rows d_in .. 63 stay 0)
    float* Sdz = Sx + MLP_MAX_IO * MLP_LD;                 // [64][65]   dz^T           (rows d_out .. 63 stay 0)
    float* Sh1 = Sdz + MLP_MAX_IO * MLP_LD;                // [h1][65]
    float* Sh2 = Sh1 + a.h1 * MLP_LD;                      // [h2][65]   h2^T, then dh1^T ([h1][65]) in the same place: sized for the larger
    float* Sdh2 = Sh2 + max(a.h1, a.h2) * MLP_LD;          // [h2][65]
    float* Sdh1 = Sh2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool l1 = (a.need & MLP_NEED_L1) != 0, l2 = (a.need & MLP_NEED_L2) != 0, l3 = (a.need & MLP_NEED_L3) != 0, want_dx = (a.need & MLP_NEED_DX) != 0;
    const bool want_dh1 = l1 || want_dx, want_dh2 = l2 || want_dh1;
    const int n1o = a.h1 >> 5, n1i = (a.d_in + 31) >> 5, n2o = a.h2 >> 5, n2i = a.h1 >> 5, n3o = (a.d_out + 31) >> 5, n3i = a.h2 >> 5;

    mlp_f32x16 acc1[2], acc2[4], acc3[2];
#pragma unroll
    for (int r = 0; r < 16; r++) { acc1[0][r] = acc1[1][r] = acc3[0][r] = acc3[1][r] = 0.0f; acc2[0][r] = acc2[1][r] = acc2[2][r] = acc2[3][r] = 0.0f; }
    double db1 = 0.0, db2 = 0.0, db3 = 0.0;      // thread f < 128: the bias gradient of feature f

    // The accumulators are fp32 chains over the rows.  A launch gives a workgroup at most MLP_FLUSH_TILES tiles (512 rows); the launches
    // behind the first ADD onto the workgroup's partial, so no chain is longer than that whatever N and the workgroup count (a chain's
    // rounding error grows with the square root of its length: one chain over 4099 rows measured 1.2e-6 of the largest entry, 5 x torch's
    // blocked sums).
    float* const p1 = a.partial + (size_t)blockIdx.x * mlp3_param_floats(a.d_in, a.h1, a.h2, a.d_out);
    float* const p2 = p1 + (size_t)a.h1 * a.d_in + a.h1;
    float* const p3 = p2 + (size_t)a.h2 * a.h1 + a.h2;

    mlp_zero(Sx, 2 * MLP_MAX_IO * MLP_LD, tid);
    __syncthreads();
    for (long long tile = a.tile0 + blockIdx.x; tile < a.tile_end; tile += gridDim.x) {
        const long long row0 = tile * MLP_TR;
        mlp_stage_rows(Sx, a.x, a.d_x, 0, row0, a.n, tid);
        if (a.d_tail) mlp_stage_rows(Sx, a.x_tail, a.d_tail, a.d_x, row0, a.n, tid);
        {   // dz = dy, or dy y (1 - y) behind the sigmoid; rows past n are 0, so they add nothing to any gradient
            const long long base = row0 * a.d_out, end = a.n * a.d_out;
            for (int idx = tid; idx < MLP_TR * a.d_out; idx += MLP_THREADS) {
                const int r = idx / a.d_out, f = idx - r * a.d_out;
                float g = 0.0f;
                if (base + idx < end) {
                    g = a.dy[base + idx];
                    if (a.sigmoid) { const float yv = a.y[base + idx]; g = (g * (1.0f - yv)) * yv; }      // (torch's order of the two products)
                }
                Sdz[f * MLP_LD + r] = g;
            }
        }
        __syncthreads();
        mlp_hidden(a.w1, a.b1, a.h1, a.d_in, Sx, Sh1, wave, lane);
        __syncthreads();
        mlp_hidden(a.w2, a.b2, a.h2, a.h1, Sh1, Sh2, wave, lane);
        __syncthreads();
        // layer 3: dh2 = (W3^T dz) [h2 > 0];  dW3 += dz h2^T;  db3 += sum dz
        if (want_dh2) mlp_dgrad_hidden(a.w3, a.h2, a.d_out, Sdz, Sh2, Sdh2, wave, lane);
        if (l3) {
            mlp_wgrad_items<2>(acc3, n3o, n3i, Sdz, Sh2, wave, lane);
            if (tid < a.d_out) db3 += mlp_row_sum(Sdz, tid);
        }
        __syncthreads();
        // layer 2: dh1 = (W2^T dh2) [h1 > 0] (into h2's image: its readers are behind the barrier);  dW2 += dh2 h1^T;  db2 += sum dh2
        if (want_dh1) mlp_dgrad_hidden(a.w2, a.h1, a.h2, Sdh2, Sh1, Sdh1, wave, lane);
        if (l2) {
            mlp_wgrad_items<4>(acc2, n2o, n2i, Sdh2, Sh1, wave, lane);
            if (tid < a.h2) db2 += mlp_row_sum(Sdh2, tid);
        }
        __syncthreads();
        // layer 1: dx = (W1^T dh1)[:d_x];  dW1 += dh1 x^T;  db1 += sum dh1
        if (want_dx) {
            const int n_items = ((a.d_x + 31) >> 5) * 2;
            for (int q = wave; q < n_items; q += 4) {
                const int m0 = (q >> 1) * 32, col0 = (q & 1) * 32;
                const mlp_f32x16 acc = mlp_gemm_w<true>(a.w1, a.d_in, a.d_x, a.h1, m0, Sdh1, col0, lane);
                const long long row = row0 + col0 + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = m0 + mlp_feat(r, lane >> 5);
                    if (f < a.d_x && row < a.n) a.dx[row * a.d_x + f] = acc[r];
                }
            }
        }
        if (l1) {
            mlp_wgrad_items<2>(acc1, n1o, n1i, Sdh1, Sx, wave, lane);
            if (tid < a.h1) db1 += mlp_row_sum(Sdh1, tid);
        }
        __syncthreads();      // the next tile's staging writes Sx / Sdz
    }
    if (l1) mlp_flush_partial<2>(acc1, n1o, n1i, a.h1, a.d_in, p1, a.add != 0, wave, lane);
    if (l2) mlp_flush_partial<4>(acc2, n2o, n2i, a.h2, a.h1, p2, a.add != 0, wave, lane);
    if (l3) mlp_flush_partial<2>(acc3, n3o, n3i, a.d_out, a.h2, p3, a.add != 0, wave, lane);
    if (l1 && tid < a.h1) { float* at = p1 + (size_t)a.h1 * a.d_in + tid; *at = (float)(a.add ? (double)*at + db1 : db1); }
    if (l2 && tid < a.h2) { float* at = p2 + (size_t)a.h2 * a.h1 + tid; *at = (float)(a.add ? (double)*at + db2 : db2); }
    if (l3 && tid < a.d_out) { float* at = p3 + (size_t)a.d_out * a.h2 + tid; *at = (float)(a.add ? (double)*at + db3 : db3); }
}

struct Mlp3Reduce {
    const float* partial; int n_partials; unsigned total;
    unsigned seg_end[6];      // exclusive ends of dW1, db1, dW2, db2, dW3, db3 inside one partial
    float* out[6];            // NULL: not wanted (and not computed)
};

// out[e] = partial[0][e] + partial[1][e] + ...: in workgroup order, one thread per parameter
__global__ void __launch_bounds__(256) mlp3_reduce_kernel(const Mlp3Reduce a)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= a.total) return;
    int seg = 0;
    while (e >= a.seg_end[seg]) seg++;
    if (!a.out[seg]) return;
    double s = 0.0;      // (fp64: the order is still the workgroups', the sum of up to a few hundred partials is rounded once)
    for (int g = 0; g < a.n_partials; g++) s += (double)a.partial[(size_t)g * a.total + e];
    a.out[seg][e - (seg ? a.seg_end[seg - 1] : 0u)] = (float)s;
}

}  // namespace gsrast
