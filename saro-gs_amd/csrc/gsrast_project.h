// gsrast_project.h -- the renderer's per-Gaussian projection as a call of its own (include/gsrast.h: gsrast_project_forward / _backward;
// gsplat's fully_fused_projection): pixel centre, view-space depth, dilated conic, integer radius and, with the anti-aliasing flag, the
// opacity compensation -- what preprocess_fwd_kernel keeps inside the geometry state -- as differentiable outputs.  This file holds the
// load helper and the two kernels; the arithmetic is gsrast_gaussian.h's, the very functions the renderer's kernels call.
//
// Forward.  project_head + project_row per row, as in preprocess_fwd_kernel: the bits are the renderer's, and so is the rule for a
// visible row.  A culled row reads +0.0 / radius 0.
//
// Backward.  Recomputes the forward from the inputs (nothing is saved), then project_backward and cov3d_backward, as in
// preprocess_bwd_kernel; dL/dscales is the gradient of scale_modifier * scale.  What differs from that kernel is the upstream side:
// dL/dmeans2D arrives in PIXELS (x 0.5 W, 0.5 H gives the ndc units of the renderer's means2D), dL/dconics is the plain gradient of the
// three stored numbers (c, -b, a) / det (the chain takes half of the middle one, as the renderer's record carries it), dL/ddepths goes
// to t.z, dL/dcompensation stands where the renderer has dL/dopacity_eff * opacity.
//
// One lane per Gaussian, 256-lane workgroups, no LDS, no scratch, no atomics, one writer per output element.  Rows of 2 and 4 floats leave
// as one 8- / 16-byte store per lane (contiguous over the wave).  Rows of 3 and 6 floats (conics, dL/dmeans3D, dL/dscales, dL/dcov3D) are
// 12- / 24-byte strides per lane and are stored per lane, float by float: parking them in LDS so that the workgroup's contiguous run
// leaves as float4 (as gsrast_temporal.h does for its embedding rows) was built and measured beside this on an MI355X and was no faster
// -- forward 0.0189 against 0.0185 ms at 1 M rows, 0.0426 against 0.0413 ms at 3 M; backward 0.0327 / 0.0322 and 0.0813 / 0.0809 ms
// (profiles/project_overhead_stores.json: "staged" beside "lane") -- so the simpler form stays.
#pragma once
#include "gsrast_gaussian.h"

namespace gsrast {

constexpr int PJ_THREADS = 256;                 // rows per workgroup

// Row i of W floats to dst [P][W].
template <int W>
__device__ __forceinline__ void project_store_row(float* __restrict__ dst, size_t i, const float row[W])
{
#pragma unroll
    for (int k = 0; k < W; k++) dst[i * W + k] = row[k];
}

// Every per-row input, requested up front with a clamped index (lanes past P load a valid element and never use it).
struct ProjIn { float p[3], s[3], c6[6]; float4 q; };
__device__ __forceinline__ void project_load(int P, size_t i, const float* __restrict__ means3D, const float* __restrict__ scales,
                                             const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, ProjIn& in)
{
    const size_t ic = i < (size_t)P ? i : (size_t)P - 1;
#pragma unroll
    for (int k = 0; k < 3; k++) in.p[k] = means3D[3 * ic + k];
    if (cov3D_precomp) {                      // uniform
#pragma unroll
        for (int k = 0; k < 6; k++) in.c6[k] = cov3D_precomp[6 * ic + k];
        in.s[0] = in.s[1] = in.s[2] = 0.0f; in.q = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) in.s[k] = scales[3 * ic + k];
        in.q = reinterpret_cast<const float4*>(rotations)[ic];
    }
}

template <bool AA>
__global__ void __launch_bounds__(PJ_THREADS)
project_fwd_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                   const float* __restrict__ cov3D_precomp, CamArgs cam_args, float* __restrict__ means2D, float* __restrict__ depths,
                   float* __restrict__ conics, int* __restrict__ radii, float* __restrict__ compensation)
{
    const size_t i = (size_t)blockIdx.x * PJ_THREADS + threadIdx.x;
    ProjIn in;
    project_load(P, i, means3D, scales, rotations, cov3D_precomp, in);
    const Cam cam = load_cam(cam_args);
    if (i >= (size_t)P) return;
    if (!cov3D_precomp) {
        const float q[4] = { in.q.x, in.q.y, in.q.z, in.q.w };
        M3 Mm;
        cov3d_from_scale_rot(in.s, cam.scale_mod, q, in.c6, Mm);
    }
    Cov2D cv;
    ProjHead h;
    ProjRow r;
    const bool vis = project_head(in.p, cam, h) && project_row<AA>(in.p, h, in.c6, cam, cv, r);
    const float con[3] = { vis ? r.con0 : 0.0f, vis ? r.con1 : 0.0f, vis ? r.con2 : 0.0f };
    reinterpret_cast<float2*>(means2D)[i] = vis ? make_float2(r.px, r.py) : make_float2(0.0f, 0.0f);
    depths[i] = vis ? h.t[2] : 0.0f;
    project_store_row<3>(conics, i, con);
    radii[i] = vis ? r.rad : 0;
    if (AA) compensation[i] = vis ? r.comp : 0.0f;
}

template <bool AA>
__global__ void __launch_bounds__(PJ_THREADS)
project_bwd_kernel(int P, const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
                   const float* __restrict__ cov3D_precomp, CamArgs cam_args,
                   const float* __restrict__ g_means2D, const float* __restrict__ g_depths, const float* __restrict__ g_conics,
                   const float* __restrict__ g_comp /* each: or null = zero */,
                   float* __restrict__ d_means3D, float* __restrict__ d_scales, float* __restrict__ d_rot, float* __restrict__ d_cov3D /* each: or null = not wanted */)
{
    const size_t i = (size_t)blockIdx.x * PJ_THREADS + threadIdx.x;
    const size_t ic = i < (size_t)P ? i : (size_t)P - 1;
    ProjIn in;
    project_load(P, i, means3D, scales, rotations, cov3D_precomp, in);
    float2 gm = make_float2(0.0f, 0.0f);
    float gz = 0.0f, gk = 0.0f, gc[3] = { 0.0f, 0.0f, 0.0f };
    if (g_means2D) gm = reinterpret_cast<const float2*>(g_means2D)[ic];      // (uniform, each of the four)
    if (g_depths) gz = g_depths[ic];
    if (AA && g_comp) gk = g_comp[ic];
    if (g_conics) { gc[0] = g_conics[3 * ic]; gc[1] = g_conics[3 * ic + 1]; gc[2] = g_conics[3 * ic + 2]; }      // (the last request: the compiler halves gc[1] right behind its load, and waits for it there)
    const Cam cam = load_cam(cam_args);
    const float q[4] = { in.q.x, in.q.y, in.q.z, in.q.w };
    M3 Mm;
    Cov2D cv;
    ProjHead h;
    ProjRow r;
    if (i >= (size_t)P) return;
    if (!cov3D_precomp) cov3d_from_scale_rot(in.s, cam.scale_mod, q, in.c6, Mm);
    const bool vis = project_head(in.p, cam, h) && project_row<AA>(in.p, h, in.c6, cam, cv, r);
    ProjGrad g;
#pragma unroll
    for (int k = 0; k < 3; k++) g.dmean[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; k++) g.dcov[k] = 0.0f;
    float ds[3] = { 0.0f, 0.0f, 0.0f };
    float4 dq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vis) {
        // comp = sqrt(rho):  dL/dcomp comp 0.5 is the weight of d(ln rho);  depths is t.z itself
        project_backward(in.p, cam, cv, r.det, gc[0], 0.5f * gc[1], gc[2], AA && r.rho > AA_FLOOR, gk * r.comp * 0.5f,
                         0.5f * (float)cam.W * gm.x, 0.5f * (float)cam.H * gm.y, true, gz, g);
        if (!cov3D_precomp) {
            const float sm[3] = { cam.scale_mod * in.s[0], cam.scale_mod * in.s[1], cam.scale_mod * in.s[2] };
            cov3d_backward(q, sm, Mm, g.dcov, ds, dq);
        }
    }
    if (d_means3D) project_store_row<3>(d_means3D, i, g.dmean);      // (uniform, each of the four)
    if (d_scales) project_store_row<3>(d_scales, i, ds);
    if (d_rot) reinterpret_cast<float4*>(d_rot)[i] = dq;
    if (d_cov3D) project_store_row<6>(d_cov3D, i, g.dcov);
}

}  // namespace gsrast
