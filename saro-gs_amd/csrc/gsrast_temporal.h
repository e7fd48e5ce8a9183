// gsrast_temporal.h -- the temporal lifespan of the 4-D model (scene/saro_gaussian.py of the reference): what makes a Gaussian appear and
// fade around its temporal centre.  Functions restated:
//   get_deformation :782-795       lifespan from the opacity head, distance, survival state (Eq. 9), time_emb(distance)  -> temporal_gate_fwd_kernel
//   its autograd                   d state, d lifespan -> d head, d temporal_pos (the embedding is detached at the cat)  -> temporal_gate_bwd_kernel
//   get_deformation_eval :878      state > 0.001 (the `dead` output; the rows are moved by gsrast_densify_apply)         -> temporal_gate_fwd_kernel
//   get_intergral :761-777         Eq. 22's integral                                                                     -> temporal_integral_kernel
//   update_learning_rate :350-356  valid mask, inv_intergral = (1/I) / min(1/I) = I_max / I                              -> temporal_integral_kernel + temporal_inv_kernel
// Per row, with head = the opacity head's output after its Sigmoid, c = temporal_pos (sigmoid(temporal_pos) under sigmoid_center) and
// ms = min_interval / duration:
//   L = (1 - ms) (1 - head) + ms;   d = t - c;   state = exp(-4 (d / L)^2)
//   time_emb = [d, sin d, cos d, sin 2d, cos 2d, ..., sin 2^(m-1) d, cos 2^(m-1) d]      (the reference's Embedder: include_input, log-sampled)
//   Q(x) = 1 / (1 + exp(-(a1 x^3 + a2 x)));   I = L (sqrt(pi) / 2) (Q(2 sqrt2 (end - c) / L) - Q(2 sqrt2 (start - c) / L))
// Q is written as a sigmoid: the reference's 1 - 1 / (1 + e^z) is the same number but cancels to 0 for very negative z.
// One lane per row, 256-row workgroups, every output element one writer.  No floating-point atomics: the integral's maximum is an integer
// max on the bits of positive floats (exact, order-free), its count an integer add, one of each per workgroup of at most 1024.  expf / sinf / cosf and
// IEEE division throughout; the library is built with -ffp-contract=off, so there is no FMA here.
#pragma once
#include "gsrast_common.h"

namespace gsrast {

constexpr int TP_RUN = 256;                  // rows per workgroup
constexpr int TP_MAX_MULTIRES = 8;           // time_emb rows of at most 17 floats: 17 KiB of LDS per workgroup
constexpr float TP_Q_A1 = 0.070565902f, TP_Q_A2 = 1.5976f;
constexpr float TP_TWO_SQRT2 = 2.8284271247461903f, TP_HALF_SQRT_PI = 0.886226925452758f;

__device__ __forceinline__ float tp_centre(float c, int sigmoid_center) { return sigmoid_center ? 1.0f / (1.0f + expf(-c)) : c; }
__device__ __forceinline__ float tp_lifespan(float head, float min_scale) { return (1.0f - min_scale) * (1.0f - head) + min_scale; }

// Forward.  The embedding is 2m+1 floats per row -- four fifths of the bytes written at m = 4 and no multiple of 16 B -- so the workgroup
// stages its rows in LDS (row stride 2m+1: odd, the lanes of a wave hit distinct banks) and stores its contiguous 256 (2m+1) floats as
// coalesced float4; only the last workgroup can have a scalar tail.  The workgroup's first float is 256 (2m+1) blockIdx floats behind a
// 16-byte aligned base: aligned as well.
__global__ void __launch_bounds__(TP_RUN)
temporal_gate_fwd_kernel(int P, int multires, int sigmoid_center, float t, float min_scale, float dead_threshold,
                         const float* __restrict__ head, const float* __restrict__ center, float* __restrict__ lifespan,
                         float* __restrict__ state, float* __restrict__ time_emb, unsigned char* __restrict__ dead)
{
    extern __shared__ float4 tp_stage4[];      // TP_RUN * (2 multires + 1) floats when time_emb is wanted, nothing otherwise
    float* const stage = reinterpret_cast<float*>(tp_stage4);
    const size_t first = (size_t)blockIdx.x * TP_RUN, i = first + threadIdx.x;
    const int W = 2 * multires + 1;
    if (i < (size_t)P) {
        const float L = tp_lifespan(head[i], min_scale);
        const float d = t - tp_centre(center[i], sigmoid_center);
        const float u = d / L;
        const float st = expf(-4.0f * (u * u));
        lifespan[i] = L;
        state[i] = st;
        if (dead) dead[i] = st > dead_threshold ? 0 : 1;      // (a NaN state is dead)
        if (time_emb) {
            float* row = stage + (size_t)threadIdx.x * W;
            row[0] = d;
            float f = 1.0f;
            for (int k = 0; k < multires; k++, f *= 2.0f) {
                const float a = d * f;
                row[1 + 2 * k] = sinf(a);
                row[2 + 2 * k] = cosf(a);
            }
        }
    }
    if (!time_emb) return;
    __syncthreads();
    const size_t rows = (size_t)P - first < (size_t)TP_RUN ? (size_t)P - first : (size_t)TP_RUN;
    const unsigned n = (unsigned)rows * (unsigned)W, n4 = n >> 2;
    float* const out = time_emb + first * (size_t)W;
    float4* const out4 = reinterpret_cast<float4*>(out);
    for (unsigned j = threadIdx.x; j < n4; j += TP_RUN) out4[j] = tp_stage4[j];
    const unsigned j = (n4 << 2) + threadIdx.x;
    if (j < n) out[j] = stage[j];
}

// Backward: L, d and state are recomputed from the 8 B per row of inputs.
//   u = d / L;  g_d = d_state (-8 u state / L);  g_L = d_lifespan + d_state (8 u^2 state / L);  d_head = -(1 - ms) g_L;  d_center = -g_d [sigma'(center)]
// A state that underflowed to 0 multiplies a finite u: gradient 0.
__global__ void __launch_bounds__(TP_RUN)
temporal_gate_bwd_kernel(int P, int sigmoid_center, float t, float min_scale, const float* __restrict__ head, const float* __restrict__ center,
                         const float* __restrict__ d_lifespan, const float* __restrict__ d_state, float* __restrict__ d_head, float* __restrict__ d_center)
{
    const size_t i = (size_t)blockIdx.x * TP_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float L = tp_lifespan(head[i], min_scale);
    const float c = tp_centre(center[i], sigmoid_center);
    const float d = t - c;
    const float u = d / L;
    const float st = expf(-4.0f * (u * u));
    const float ds = d_state ? d_state[i] : 0.0f, dl = d_lifespan ? d_lifespan[i] : 0.0f;
    const float k = 8.0f * u * st / L;      // -d state / d d
    if (d_head) d_head[i] = -(1.0f - min_scale) * (dl + ds * (k * u));
    if (d_center) {
        const float g = ds * k;             // -g_d
        d_center[i] = sigmoid_center ? g * (c * (1.0f - c)) : g;
    }
}

__device__ __forceinline__ float tp_Q(float x) { return 1.0f / (1.0f + expf(-(TP_Q_A1 * (x * x * x) + TP_Q_A2 * x))); }

// Integral, valid mask and the two statistics.  stats (zeroed before the launch) = { bits of the largest valid I, number of valid rows }:
// a valid I exceeds min_integral >= 0, so it is positive and its bits order as the floats do.  At most TP_INTEGRAL_WGS workgroups walk
// the rows in grid strides and each ends with one integer atomic pair: atomics on one address serialise (with a pair per 256 rows the
// call measured 0.101 / 0.284 ms at 1 M / 3 M rows on an MI355X, this way 0.032 / 0.068 ms).  The max is skipped where a plain read already shows a value as large -- the word
// only grows, so a stale read errs on the side of issuing it.
constexpr int TP_INTEGRAL_WGS = 1024;
__global__ void __launch_bounds__(TP_RUN)
temporal_integral_kernel(int P, int sigmoid_center, float start, float end, float min_scale, float min_integral, const float* __restrict__ head,
                         const float* __restrict__ center, float* __restrict__ integral, unsigned char* __restrict__ dead, int* __restrict__ stats)
{
    __shared__ int s_max[TP_RUN / 64], s_cnt[TP_RUN / 64];
    int bits = 0, cnt = 0;
    for (size_t i = (size_t)blockIdx.x * TP_RUN + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * TP_RUN) {
        const float L = tp_lifespan(head[i], min_scale);
        const float c = tp_centre(center[i], sigmoid_center);
        const float p1 = tp_Q(TP_TWO_SQRT2 * (end - c) / L), p2 = tp_Q(TP_TWO_SQRT2 * (start - c) / L);
        const float I = L * TP_HALF_SQRT_PI * (p1 - p2);
        const bool valid = I > min_integral;      // (a NaN integral is dead)
        integral[i] = I;
        dead[i] = valid ? 0 : 1;
        if (valid) { const int b = __float_as_int(I); bits = b > bits ? b : bits; cnt++; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int b = __shfl_xor(bits, o, 64), n = __shfl_xor(cnt, o, 64);
        bits = b > bits ? b : bits;
        cnt += n;
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = bits; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TP_RUN / 64; w++) { bits = s_max[w] > bits ? s_max[w] : bits; cnt += s_cnt[w]; }
        if (cnt > 0) {
            if (*reinterpret_cast<volatile int*>(&stats[0]) < bits) atomicMax(&stats[0], bits);
            atomicAdd(&stats[1], cnt);
        }
    }
}

// inv = I_max / I on a valid row, 0 on a dead one: the reference's (1/I) / min(1/I) with one rounding less.  No valid row: all zeros.
__global__ void __launch_bounds__(TP_RUN)
temporal_inv_kernel(int P, const float* __restrict__ integral, const unsigned char* __restrict__ dead, const int* __restrict__ stats, float* __restrict__ inv)
{
    const size_t i = (size_t)blockIdx.x * TP_RUN + threadIdx.x;
    if (i >= (size_t)P) return;
    const float imax = __int_as_float(stats[0]);
    inv[i] = dead[i] ? 0.0f : imax / integral[i];
}

}  // namespace gsrast
