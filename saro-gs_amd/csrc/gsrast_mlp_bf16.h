// gsrast_mlp_bf16.h -- the fused 3-layer head of gsrast_mlp.h on the bf16 matrix instruction v_mfma_f32_32x32x16_bf16 (fp32 accumulate):
// the opt-in reduced-precision path (GSRAST_MLP_BF16).  Same shapes, same descriptor, same scratch, fp32 tensors on both sides.
//
// Rounding model (what tests/mlp_bf16_math.py restates and tests/test_gpu_mlp_bf16.py holds the kernels to).  bf(.) is round-to-nearest-even
// to bfloat16; a NaN stays a NaN.  Behaviour on fp32 DENORMALS is unspecified (the conversion instruction may flush them, and a denormal
// activation that rounds to 0 closes its ReLU gate).
//   forward    x~ = bf([x | x_tail]),  W~k = bf(Wk),  biases fp32
//              a1 = W~1 x~ + b1,   h~1 = bf(relu(a1))
//              a2 = W~2 h~1 + b2,  h~2 = bf(relu(a2))
//              y  = W~3 h~2 + b3   [-> sigmoid]
//              products bf16 x bf16, accumulated in fp32; bias add, ReLU, Sigmoid and y in fp32
//   backward   recomputes a1, a2, h~1, h~2 exactly as the forward formed them
//              g3 = dy, or dy y (1 - y);       g~3 = bf(g3);   dW3 = sum_rows g~3 (x) h~2
//              g2 = (W~3^T g~3) [a2 > 0];      g~2 = bf(g2);   dW2 = sum_rows g~2 (x) h~1
//              g1 = (W~2^T g~2) [a1 > 0];      g~1 = bf(g1);   dW1 = sum_rows g~1 (x) x~;     dx = (W~1^T g~1)[:d_x]
//              db_k = sum_rows of the UNROUNDED fp32 g_k, in fp64
//              the weight gradients are the fp32 master weights' (the rounding is straight-through, as under autocast); all gradients fp32
// The weights are converted inside each launch, into LDS: no bf16 copy of anything outlives a call, none reaches global memory.
//
// Orientation: as gsrast_mlp.h, every product is transposed -- the weight is the A operand, the row of the batch sits on the lane.  A wave
// owns 32 rows of the batch through ALL layers: a layer's 32 x 32 accumulators (row of the batch = lane & 31, feature = mlp_feat(r, lane >> 5)),
// biased, clamped and packed pairwise with v_cvt_pk_bf16_f32, ARE the next layer's B operand -- no LDS, no lane movement, no barrier.
// Registers 8 s .. 8 s + 7 of feature tile T make the fragment of k-step S = 2 T + s, whose element j of lane half h is feature
//     k(S, h, j) = 16 S + 8 (j >> 2) + 4 h + (j & 3);
// every other operand follows this k order: x and dy are fetched from global memory in it, the weight fragments are read from the LDS
// images in it (two 8-byte reads per fragment).  The data gradients take the TRANSPOSED weight (A[m][k] = W[k][m]) from the same image with
// ds_read_b64_tr_b16: one image per weight serves both directions.
//
// The weight gradients sum over the rows of the batch, the lane index of everything above, so they need the transposed images: each wave
// writes its packed fragments (8-byte stores) into two [128 rows][features] bf16 images P (g~) and Q (the activation), and after a barrier
// the 32 x 32 items of dW go round the four waves as in gsrast_mlp.h, both operands read with ds_read_b64_tr_b16.  Three phases per tile
// (layer 3, 2, 1) reuse the two images.  The accumulators stay in registers over a launch's tiles: at most MLPB_FLUSH_TILES x 128 = 512
// rows per workgroup and launch, then stored (later launches: added) to the workgroup's slab; mlp3_reduce_kernel sums the slabs in fp64 in
// workgroup order.  No floating-point atomics, run-to-run bit-identical for one workgroup count, scratch independent of N: the fp32 path's
// guarantees, its partial layout and its reduction kernel.
// Bias gradients: the unrounded fp32 g tile goes through a wave-private [32][33] fp32 slab, each lane sums 16 rows of one feature in fp64
// and keeps the sum over the launch's tiles; the 8 sums per feature (4 waves x 2 halves) are added in that fixed order at the end.
//
// LDS (bytes): W1 [128][68] 17 408 | W2 [128][132] 33 792 | W3 [64][132] 16 896 | biases 1 280 = 69 376 (forward: two workgroups per CU)
//              backward adds P, Q [128][132] 2 x 33 792 and the four bias slabs 16 896 = 153 856 (one workgroup per CU).
// Row strides of 136 / 264 bytes: a lane per row reads or writes 8 bytes without bank conflicts, and every row is 8-byte aligned for the
// transposed reads.  Every transposed read runs with all 64 lanes active (wave-uniform control flow only) and inside the images: padding
// rows and columns hold zeros or finite leftovers whose products land in elements the flush discards.
#pragma once
#include "gsrast_mlp.h"

namespace gsrast {

constexpr int MLPB_ROWS = 128;              // rows of the batch per tile: 32 per wave
constexpr int MLPB_FLUSH_TILES = 4;         // backward: tiles per workgroup and launch (512 rows: the longest fp32 chain of a weight gradient)
constexpr int MLPB_LDN = 64 + 4;            // bf16 elements per row of a 64-column image
constexpr int MLPB_LDW = 128 + 4;           //                              128-column image
constexpr int MLPB_OFF_W1 = 0;
constexpr int MLPB_OFF_W2 = MLPB_OFF_W1 + MLP_MAX_H * MLPB_LDN * 2;
constexpr int MLPB_OFF_W3 = MLPB_OFF_W2 + MLP_MAX_H * MLPB_LDW * 2;
constexpr int MLPB_OFF_B = MLPB_OFF_W3 + MLP_MAX_IO * MLPB_LDW * 2;
constexpr int MLPB_FWD_LDS = MLPB_OFF_B + (2 * MLP_MAX_H + MLP_MAX_IO) * 4;
constexpr int MLPB_OFF_P = MLPB_FWD_LDS;
constexpr int MLPB_OFF_Q = MLPB_OFF_P + MLPB_ROWS * MLPB_LDW * 2;
constexpr int MLPB_OFF_SLAB = MLPB_OFF_Q + MLPB_ROWS * MLPB_LDW * 2;
constexpr int MLPB_SLAB = 32 * 33;          // floats of one wave's bias slab
constexpr int MLPB_BWD_LDS = MLPB_OFF_SLAB + 4 * MLPB_SLAB * 4;
constexpr int MLPB_NB = 2 * MLP_MAX_H + MLP_MAX_IO;      // bias gradients of one head
static_assert(MLPB_OFF_W2 % 16 == 0 && MLPB_OFF_W3 % 16 == 0 && MLPB_OFF_B % 16 == 0 && MLPB_OFF_P % 16 == 0 && MLPB_OFF_Q % 16 == 0 && MLPB_OFF_SLAB % 16 == 0, "LDS images 16-byte aligned");
static_assert(MLPB_BWD_LDS <= 160 * 1024 && 2 * MLPB_FWD_LDS <= 160 * 1024, "LDS budget");
static_assert(8 * MLPB_NB * 8 <= MLPB_ROWS * MLPB_LDW * 2, "the bias gradients' last sum fits in P");

typedef unsigned short mlpb_u16;
typedef __bf16 mlpb_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mlpb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mlpb_f32x2 __attribute__((ext_vector_type(2)));
typedef short mlpb_s16x4 __attribute__((ext_vector_type(4)));
struct MlpbFrag { unsigned u[4]; };         // 8 bf16: one lane's share of an A or B operand of one k-step

__device__ __forceinline__ unsigned mlpb_pk(float lo, float hi)      // bf(lo) | bf(hi) << 16  (v_cvt_pk_bf16_f32: RNE, a NaN stays a NaN)
{
    const mlpb_f32x2 v = { lo, hi };
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, mlpb_bf16x2));
}

__device__ __forceinline__ mlp_f32x16 mlpb_mfma(const MlpbFrag& a, const MlpbFrag& b, mlp_f32x16 acc)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mlpb_bf16x8, a), __builtin_bit_cast(mlpb_bf16x8, b), acc, 0, 0, 0);
}

__device__ __forceinline__ mlp_f32x16 mlpb_zero16()
{
    mlp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    return acc;
}

// W [M][K] fp32 (global) -> img [rows][cols] bf16 with row stride ld, 0 outside M x K
__device__ __forceinline__ void mlpb_stage_w(mlpb_u16* img, int ld, int rows, int cols, const float* __restrict__ W, int M, int K, int tid)
{
    const int half = cols >> 1;
    for (int idx = tid; idx < rows * half; idx += MLP_THREADS) {
        const int m = idx / half, k = 2 * (idx - m * half);
        const float lo = (m < M && k < K) ? W[(size_t)m * K + k] : 0.0f;
        const float hi = (m < M && k + 1 < K) ? W[(size_t)m * K + k + 1] : 0.0f;
        *reinterpret_cast<unsigned*>(img + m * ld + k) = mlpb_pk(lo, hi);
    }
}

// the three weight images and the biases of one launch
__device__ __forceinline__ void mlpb_stage_params(unsigned char* lds, const Mlp3Args& a, int tid)
{
    mlpb_stage_w(reinterpret_cast<mlpb_u16*>(lds + MLPB_OFF_W1), MLPB_LDN, a.h1, MLP_MAX_IO, a.w1, a.h1, a.d_in, tid);
    mlpb_stage_w(reinterpret_cast<mlpb_u16*>(lds + MLPB_OFF_W2), MLPB_LDW, a.h2, MLP_MAX_H, a.w2, a.h2, a.h1, tid);
    mlpb_stage_w(reinterpret_cast<mlpb_u16*>(lds + MLPB_OFF_W3), MLPB_LDW, MLP_MAX_IO, MLP_MAX_H, a.w3, a.d_out, a.h2, tid);
    float* Sb = reinterpret_cast<float*>(lds + MLPB_OFF_B);
    for (int k = tid; k < MLPB_NB; k += MLP_THREADS)
        Sb[k] = k < MLP_MAX_H ? (k < a.h1 ? a.b1[k] : 0.0f) : k < 2 * MLP_MAX_H ? (k - MLP_MAX_H < a.h2 ? a.b2[k - MLP_MAX_H] : 0.0f)
                                                                               : (k - 2 * MLP_MAX_H < a.d_out ? a.b3[k - 2 * MLP_MAX_H] : 0.0f);
}

// A fragment of k-step S, rows m0 .. m0 + 31 of a weight image: element j = img[m0 + (lane & 31)][k(S, lane >> 5, j)]
__device__ __forceinline__ MlpbFrag mlpb_a(const mlpb_u16* img, int ld, int m0, int S, int lane)
{
    const mlpb_u16* p = img + (m0 + (lane & 31)) * ld + 16 * S + 4 * (lane >> 5);
    const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 8);
    return MlpbFrag{ { lo.x, lo.y, hi.x, hi.y } };
}

// The transposed fragment: element j = img[k(S, lane >> 5, j)][c0 + (lane & 31)].  Per group of 16 lanes ds_read_b64_tr_b16 takes a block of
// 4 rows x 16 columns: lane 4 q + p of the group gives the address of row q, columns 4 p .. 4 p + 3, and receives column (lane & 15) of
// the four rows.  Block t (j >> 2 = t) has rows 16 S + 8 t + 4 h + q; the group's columns start at c0 + 16 ((lane >> 4) & 1).
// All 64 lanes must be active.
__device__ __forceinline__ MlpbFrag mlpb_at(const mlpb_u16* img, int ld, int c0, int S, int lane)
{
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const mlpb_u16* at = img + (16 * S + 4 * (lane >> 5) + q) * ld + c0 + 16 * ((lane >> 4) & 1) + 4 * p;
    typedef __attribute__((address_space(3))) mlpb_s16x4 lds_s16x4;
    const mlpb_s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)at);
    const mlpb_s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(at + 8 * ld));
    const uint2 lo = __builtin_bit_cast(uint2, t0), hi = __builtin_bit_cast(uint2, t1);
    return MlpbFrag{ { lo.x, lo.y, hi.x, hi.y } };
}

// one lane's fragment -> its row of a [row of the batch][feature] image: features k(S, h, 0..3) and k(S, h, 4..7), 8 bytes each
__device__ __forceinline__ void mlpb_store_frag(mlpb_u16* img, int row, int S, const MlpbFrag& f, int lane)
{
    mlpb_u16* p = img + row * MLPB_LDW + 16 * S + 4 * (lane >> 5);
    *reinterpret_cast<uint2*>(p) = make_uint2(f.u[0], f.u[1]);
    *reinterpret_cast<uint2*>(p + 8) = make_uint2(f.u[2], f.u[3]);
}

// acc [32 features m0.. x 32 rows of the batch] = sum over k-steps S < n_ks of A(S) . b[S]; A from the image, TR: its transpose
template <bool TR, int NB>
__device__ __forceinline__ mlp_f32x16 mlpb_gemm(const mlpb_u16* img, int ld, int m0, int n_ks, const MlpbFrag (&b)[NB], int lane)
{
    mlp_f32x16 acc = mlpb_zero16();
#pragma unroll
    for (int S = 0; S < NB; S++)
        if (S < n_ks) acc = mlpb_mfma(TR ? mlpb_at(img, ld, m0, S, lane) : mlpb_a(img, ld, m0, S, lane), b[S], acc);
    return acc;
}

// the 16 fp32 values of feature tile T -> the two fragments S = 2 T, 2 T + 1
__device__ __forceinline__ void mlpb_pack(const mlp_f32x16& v, MlpbFrag& f0, MlpbFrag& f1)
{
#pragma unroll
    for (int jj = 0; jj < 4; jj++) {
        f0.u[jj] = mlpb_pk(v[2 * jj], v[2 * jj + 1]);
        f1.u[jj] = mlpb_pk(v[8 + 2 * jj], v[8 + 2 * jj + 1]);
    }
}

// hidden layer: out[2 T], out[2 T + 1] = bf(relu(W . in + b)) for the feature tiles T < n_mt
template <int NB>
__device__ __forceinline__ void mlpb_hidden(MlpbFrag (&out)[8], const mlpb_u16* img, int ld, const float* bias, int n_mt, int n_ks, const MlpbFrag (&in)[NB], int lane)
{
#pragma unroll
    for (int T = 0; T < 4; T++) {
        if (T < n_mt) {
            mlp_f32x16 acc = mlpb_gemm<false>(img, ld, 32 * T, n_ks, in, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float v = acc[r] + bias[32 * T + mlp_feat(r, lane >> 5)];
                acc[r] = v < 0.0f ? 0.0f : v;      // (a NaN stays a NaN, as torch.relu)
            }
            mlpb_pack(acc, out[2 * T], out[2 * T + 1]);
        } else {
#pragma unroll
            for (int jj = 0; jj < 4; jj++) out[2 * T].u[jj] = out[2 * T + 1].u[jj] = 0u;
        }
    }
}

// x~ in the fragments' k order: element j of xb[S] = bf([x | x_tail][row][k(S, h, j)]), 0 past D_in columns or for a row past n
__device__ __forceinline__ void mlpb_load_x(MlpbFrag (&xb)[4], const Mlp3Args& a, long long row, int lane)
{
    const bool live = row < a.n;
    const int n_ks = (a.d_in + 15) >> 4, h4 = 4 * (lane >> 5);
    // the lane half's 4 columns go into the row pointers and the two limits: every element is then a constant offset and a constant compared
    const float* xr = a.x + (live ? row : 0) * a.d_x + h4;                                          // [c] is column c + h4 < d_x
    const float* tr = (a.d_tail ? a.x_tail + (live ? row : 0) * a.d_tail : a.x) + (h4 - a.d_x);     // [c] is column d_x <= c + h4 < d_in
    const int x_left = live ? a.d_x - h4 : 0, in_left = live ? a.d_in - h4 : 0;
#pragma unroll
    for (int S = 0; S < 4; S++) {
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            float v[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int c = 16 * S + 8 * (jj >> 1) + 2 * (jj & 1) + e;
                v[e] = 0.0f;
                if (S < n_ks) {
                    if (c < x_left) v[e] = xr[c];
                    else if (c < in_left) v[e] = tr[c];
                }
            }
            xb[S].u[jj] = mlpb_pk(v[0], v[1]);
        }
    }
}

// 32 x 32 results -> out[row][f], f = m0 + feature < width
__device__ __forceinline__ void mlpb_store_rows(float* __restrict__ out, int width, int m0, const mlp_f32x16& v, long long row, long long n, int lane)
{
    if (row >= n) return;
    float* o = out + row * width + m0 + 4 * (lane >> 5);
    const int left = width - m0 - 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int f = (r & 3) + 8 * (r >> 2);      // (mlp_feat without the lane half: a constant offset from o)
        if (f < left) o[f] = v[r];
    }
}

// N1, N2: H1 / 32 and H2 / 32 as compile-time constants (the loops over feature tiles and k-steps then have no branches), or 0: read from a
template <int N1, int N2>
__global__ void __launch_bounds__(MLP_THREADS) mlp3_bf16_fwd_kernel(const Mlp3Args a)
{
    const int n1 = N1 ? N1 : a.h1 >> 5, n2 = N2 ? N2 : a.h2 >> 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char mlpb_lds[];
    const mlpb_u16* W1 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W1);
    const mlpb_u16* W2 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W2);
    const mlpb_u16* W3 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W3);
    const float* Sb = reinterpret_cast<const float*>(mlpb_lds + MLPB_OFF_B);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mlpb_stage_params(mlpb_lds, a, tid);
    __syncthreads();
    const long long n_tiles = (a.n + MLPB_ROWS - 1) / MLPB_ROWS;
    const int n_ks1 = (a.d_in + 15) >> 4, n_mt3 = (a.d_out + 31) >> 5;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long row0 = tile * MLPB_ROWS + 32 * wave;
        if (row0 >= a.n) continue;      // (the whole wave: no barrier below)
        const long long row = row0 + (lane & 31);
        MlpbFrag xb[4], h1f[8], h2f[8];
        mlpb_load_x(xb, a, row, lane);
        mlpb_hidden(h1f, W1, MLPB_LDN, Sb, n1, n_ks1, xb, lane);
        mlpb_hidden(h2f, W2, MLPB_LDW, Sb + MLP_MAX_H, n2, 2 * n1, h1f, lane);
#pragma unroll
        for (int T = 0; T < 2; T++) {
            if (T < n_mt3) {
                mlp_f32x16 acc = mlpb_gemm<false>(W3, MLPB_LDW, 32 * T, 2 * n2, h2f, lane);
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    float v = acc[r] + Sb[2 * MLP_MAX_H + 32 * T + mlp_feat(r, lane >> 5)];
                    if (a.sigmoid) v = 1.0f / (1.0f + expf(-v));
                    acc[r] = v;
                }
                mlpb_store_rows(a.y, a.d_out, 32 * T, acc, row, a.n, lane);
            }
        }
    }
}

// db += this wave's 32 rows of the unrounded tile v, by feature: lane l sums rows 16 (l >> 5) .. + 15 of feature l & 31 (tile-local) in fp64
__device__ __forceinline__ void mlpb_bias_rows(float* slab, const mlp_f32x16& v, double& db, int lane)
{
#pragma unroll
    for (int r = 0; r < 16; r++) slab[mlp_feat(r, lane >> 5) * 33 + (lane & 31)] = v[r];
    __builtin_amdgcn_wave_barrier();      // (one wave's LDS accesses complete in order: no wait, only no reordering by the compiler)
    const float* s = slab + (lane & 31) * 33 + 16 * (lane >> 5);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) sum += (double)s[k];
    db += sum;
    __builtin_amdgcn_wave_barrier();
}

// g = acc where the packed activation of the same (feature, row) is not +-0, else 0  (h~ = NaN passes the gradient, as threshold_backward)
__device__ __forceinline__ void mlpb_mask(mlp_f32x16& acc, const MlpbFrag& f0, const MlpbFrag& f1)
{
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const unsigned u = (r < 8 ? f0 : f1).u[(r & 7) >> 1];
        const unsigned bits = (r & 1) ? (u >> 16) : (u & 0xffffu);
        acc[r] = (bits & 0x7fffu) == 0u ? 0.0f : acc[r];
    }
}

// one wave's share of a weight gradient's 32 x 32 items over the tile's 128 rows: item q = wave + 4 t covers (q / n_i, q % n_i)
template <int T>
__device__ __forceinline__ void mlpb_wgrad_items(mlp_f32x16 (&acc)[T], int n_o, int n_i, const mlpb_u16* P, const mlpb_u16* Q, int wave, int lane)
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int q = wave + 4 * t;
        if (q < n_o * n_i) {      // (wave-uniform: the transposed reads keep all lanes)
            const int o0 = (q / n_i) * 32, i0 = (q % n_i) * 32;
#pragma unroll
            for (int S = 0; S < MLPB_ROWS / 16; S++)
                acc[t] = mlpb_mfma(mlpb_at(P, MLPB_LDW, o0, S, lane), mlpb_at(Q, MLPB_LDW, i0, S, lane), acc[t]);
        }
    }
}

template <int N1, int N2>
__global__ void __launch_bounds__(MLP_THREADS) mlp3_bf16_bwd_kernel(const Mlp3Args a)
{
    const int n1 = N1 ? N1 : a.h1 >> 5, n2 = N2 ? N2 : a.h2 >> 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char mlpb_lds[];
    const mlpb_u16* W1 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W1);
    const mlpb_u16* W2 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W2);
    const mlpb_u16* W3 = reinterpret_cast<const mlpb_u16*>(mlpb_lds + MLPB_OFF_W3);
    const float* Sb = reinterpret_cast<const float*>(mlpb_lds + MLPB_OFF_B);
    mlpb_u16* P = reinterpret_cast<mlpb_u16*>(mlpb_lds + MLPB_OFF_P);
    mlpb_u16* Q = reinterpret_cast<mlpb_u16*>(mlpb_lds + MLPB_OFF_Q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* slab = reinterpret_cast<float*>(mlpb_lds + MLPB_OFF_SLAB) + wave * MLPB_SLAB;
    const bool l1 = (a.need & MLP_NEED_L1) != 0, l2 = (a.need & MLP_NEED_L2) != 0, l3 = (a.need & MLP_NEED_L3) != 0, want_dx = (a.need & MLP_NEED_DX) != 0;
    const bool want_g1 = l1 || want_dx, want_g2 = l2 || want_g1;
    const int n1o = n1, n1i = (a.d_in + 31) >> 5, n2o = n2, n2i = n1, n3o = (a.d_out + 31) >> 5, n3i = n2;
    const int n_ks1 = (a.d_in + 15) >> 4, n_ks3 = (a.d_out + 15) >> 4;

    mlp_f32x16 acc1[2], acc2[4], acc3[2];
#pragma unroll
    for (int t = 0; t < 4; t++) { acc2[t] = mlpb_zero16(); if (t < 2) { acc1[t] = mlpb_zero16(); acc3[t] = mlpb_zero16(); } }
    double db1[4] = { 0.0, 0.0, 0.0, 0.0 }, db2[4] = { 0.0, 0.0, 0.0, 0.0 }, db3[2] = { 0.0, 0.0 };      // feature 32 T + (lane & 31), rows of lane half lane >> 5

    mlpb_stage_params(mlpb_lds, a, tid);
    __syncthreads();
    const int lane_id = lane;
    for (long long tile = a.tile0 + blockIdx.x; tile < a.tile_end; tile += gridDim.x) {
        // The lane index is made opaque once per tile: everything derived from it (LDS addresses, column limits, byte offsets) is then
        // recomputed per tile -- a few dozen integer instructions -- where hoisting it out of the loop held 160 registers and spilled them.
        int lane = lane_id;
        asm volatile("" : "+v"(lane));
        const int lrow = 32 * wave + (lane & 31);                  // this lane's row of the tile (and of P, Q)
        const long long row = tile * MLPB_ROWS + lrow;
        const bool live = row < a.n;                               // rows past n: x = 0 and g3 = 0, so every g~ is 0 and they add nothing
        MlpbFrag xb[4], h1f[8], h2f[8], g3f[4], g2f[8], g1f[8];
        const float* dyr = a.dy + (live ? row : 0) * a.d_out + 4 * (lane >> 5);
        const float* yr = a.sigmoid ? a.y + (live ? row : 0) * a.d_out + 4 * (lane >> 5) : dyr;
        const int dy_left = live ? a.d_out - 4 * (lane >> 5) : 0;
        mlpb_load_x(xb, a, row, lane);
        mlpb_hidden(h1f, W1, MLPB_LDN, Sb, n1, n_ks1, xb, lane);
        mlpb_hidden(h2f, W2, MLPB_LDW, Sb + MLP_MAX_H, n2, 2 * n1, h1f, lane);
        // g3 = dy, or dy y (1 - y) behind the sigmoid, in the fragments' k order
#pragma unroll
        for (int T = 0; T < 2; T++) {
            mlp_f32x16 g = mlpb_zero16();
            if (T < n3o) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int f = 32 * T + (r & 3) + 8 * (r >> 2);      // (mlp_feat without the lane half: inside dyr, yr and dy_left)
                    if (f < dy_left) {
                        float v = dyr[f];
                        if (a.sigmoid) { const float yv = yr[f]; v = (v * (1.0f - yv)) * yv; }      // (torch's order of the two products)
                        g[r] = v;
                    }
                }
                if (l3) mlpb_bias_rows(slab, g, db3[T], lane);
            }
            mlpb_pack(g, g3f[2 * T], g3f[2 * T + 1]);
        }
        // layer 3: dW3 += g~3 (x) h~2 over the tile's rows
        if (l3) {
#pragma unroll
            for (int S = 0; S < 4; S++) if (S < n_ks3) mlpb_store_frag(P, lrow, S, g3f[S], lane);
#pragma unroll
            for (int S = 0; S < 8; S++) if (S < 2 * n2) mlpb_store_frag(Q, lrow, S, h2f[S], lane);
        }
        __syncthreads();
        if (l3) mlpb_wgrad_items<2>(acc3, n3o, n3i, P, Q, wave, lane);
        // g2 = (W~3^T g~3) [a2 > 0]
        if (want_g2) {
#pragma unroll
            for (int T = 0; T < 4; T++) {
                mlp_f32x16 g = mlpb_zero16();
                if (T < n2o) {
                    g = mlpb_gemm<true>(W3, MLPB_LDW, 32 * T, n_ks3, g3f, lane);
                    mlpb_mask(g, h2f[2 * T], h2f[2 * T + 1]);
                    if (l2) mlpb_bias_rows(slab, g, db2[T], lane);
                }
                mlpb_pack(g, g2f[2 * T], g2f[2 * T + 1]);
            }
        }
        __syncthreads();      // layer 3's items have read P and Q
        // layer 2: dW2 += g~2 (x) h~1
        if (l2) {
#pragma unroll
            for (int S = 0; S < 8; S++) {
                if (S < 2 * n2) mlpb_store_frag(P, lrow, S, g2f[S], lane);
                if (S < 2 * n1) mlpb_store_frag(Q, lrow, S, h1f[S], lane);
            }
        }
        __syncthreads();
        if (l2) mlpb_wgrad_items<4>(acc2, n2o, n2i, P, Q, wave, lane);
        // g1 = (W~2^T g~2) [a1 > 0]
        if (want_g1) {
#pragma unroll
            for (int T = 0; T < 4; T++) {
                mlp_f32x16 g = mlpb_zero16();
                if (T < n1o) {
                    g = mlpb_gemm<true>(W2, MLPB_LDW, 32 * T, 2 * n2, g2f, lane);
                    mlpb_mask(g, h1f[2 * T], h1f[2 * T + 1]);
                    if (l1) mlpb_bias_rows(slab, g, db1[T], lane);
                }
                mlpb_pack(g, g1f[2 * T], g1f[2 * T + 1]);
            }
        }
        __syncthreads();
        // layer 1: dW1 += g~1 (x) x~;  dx = (W~1^T g~1)[:d_x]
        if (l1) {
#pragma unroll
            for (int S = 0; S < 8; S++) if (S < 2 * n1) mlpb_store_frag(P, lrow, S, g1f[S], lane);
#pragma unroll
            for (int S = 0; S < 4; S++) mlpb_store_frag(Q, lrow, S, xb[S], lane);      // (all 64 columns: the fragments past D_in are 0)
        }
        __syncthreads();
        if (l1) mlpb_wgrad_items<2>(acc1, n1o, n1i, P, Q, wave, lane);
        if (want_dx) {
#pragma unroll
            for (int T = 0; T < 2; T++) {
                if (T < ((a.d_x + 31) >> 5)) {
                    const mlp_f32x16 g = mlpb_gemm<true>(W1, MLPB_LDN, 32 * T, 2 * n1, g1f, lane);
                    mlpb_store_rows(a.dx, a.d_x, 32 * T, g, row, a.n, lane);
                }
            }
        }
        __syncthreads();      // the next tile's phase 3 writes P and Q
    }

    float* const p1 = a.partial + (size_t)blockIdx.x * mlp3_param_floats(a.d_in, a.h1, a.h2, a.d_out);
    float* const p2 = p1 + (size_t)a.h1 * a.d_in + a.h1;
    float* const p3 = p2 + (size_t)a.h2 * a.h1 + a.h2;
    if (l1) mlp_flush_partial<2>(acc1, n1o, n1i, a.h1, a.d_in, p1, a.add != 0, wave, lane);
    if (l2) mlp_flush_partial<4>(acc2, n2o, n2i, a.h2, a.h1, p2, a.add != 0, wave, lane);
    if (l3) mlp_flush_partial<2>(acc3, n3o, n3i, a.d_out, a.h2, p3, a.add != 0, wave, lane);
    // bias gradients: the 8 fp64 sums of a feature (wave, lane half) added in that order (P is free behind the loop's last barrier)
    double* red = reinterpret_cast<double*>(P) + (2 * wave + (lane >> 5)) * MLPB_NB;
#pragma unroll
    for (int T = 0; T < 4; T++) {
        red[32 * T + (lane & 31)] = db1[T];
        red[MLP_MAX_H + 32 * T + (lane & 31)] = db2[T];
        if (T < 2) red[2 * MLP_MAX_H + 32 * T + (lane & 31)] = db3[T];
    }
    __syncthreads();
    for (int k = tid; k < MLPB_NB; k += MLP_THREADS) {
        const int layer = k < MLP_MAX_H ? 1 : k < 2 * MLP_MAX_H ? 2 : 3, f = k - (layer - 1) * MLP_MAX_H;
        const bool on = layer == 1 ? (l1 && f < a.h1) : layer == 2 ? (l2 && f < a.h2) : (l3 && f < a.d_out);
        if (!on) continue;
        double s = 0.0;
        for (int g = 0; g < 8; g++) s += reinterpret_cast<const double*>(P)[g * MLPB_NB + k];
        float* at = layer == 1 ? p1 + (size_t)a.h1 * a.d_in + f : layer == 2 ? p2 + (size_t)a.h2 * a.h1 + f : p3 + (size_t)a.d_out * a.h2 + f;
        *at = (float)(a.add ? (double)*at + s : s);
    }
}

}  // namespace gsrast
