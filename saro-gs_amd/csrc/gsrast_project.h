// gsrast_project.h -- the renderer's per-Gaussian projection as a call of its own (include/gsrast.h: gsrast_project_forward / _backward;
// gsplat's fully_fused_projection): pixel centre, view-space depth, dilated conic, integer radius and, with the anti-aliasing flag, the
// opacity compensation -- what preprocess_fwd_kernel keeps inside the geometry state -- as differentiable outputs.
//
// Forward.  Per row exactly what preprocess_fwd_kernel evaluates (gsrast_preprocess.h, the non-RAW branch), through the same device
// functions (xform4x4, xform4x3, cov3d_from_scale_rot, cov2d_eval, aa_rho, aa_comp, ndc2pix, tile_rect) on the same operands in the same
// order: the unit is built with -ffp-contract=off and correctly rounded divide / sqrt, so the bits are the renderer's.  A row is visible
// iff  view z > 0.2,  det != 0  and its tile rectangle has non-zero area -- the renderer's rule.  A culled row reads +0.0 / radius 0.
//
// Backward.  Recomputes the forward from the inputs (nothing is saved) and applies, written anew here, the chain preprocess_bwd_kernel
// applies to its gradient record (reference backward.cu:144-274 computeCov2DCUDA, :346-396 preprocessCUDA, :278-341 computeCov3D), with the
// reference's conventions:  a frustum-clamped t.x / t.z, t.y / t.z enters J as a constant;  d conic / d cov2D uses 1 / (det^2 + 1e-7);
// dL/dscales is the gradient of scale_modifier * scale;  the compensation has no gradient where rho sits on its floor.  What differs from
// that kernel is the upstream side: dL/dmeans2D arrives in PIXELS (x 0.5 W, 0.5 H gives the ndc units of the renderer's means2D), dL/dconics
// is the plain gradient of the three stored numbers (c, -b, a) / det, dL/ddepths goes to t.z, dL/dcompensation stands where the
// renderer has dL/dopacity_eff * opacity.
//
// One lane per Gaussian, 256-lane workgroups, no LDS, no scratch, no atomics, one writer per output element.  Rows of 2 and 4 floats leave
// as one 8- / 16-byte store per lane (contiguous over the wave).  Rows of 3 and 6 floats (conics, dL/dmeans3D, dL/dscales, dL/dcov3D) are
// 12- / 24-byte strides per lane and are stored per lane, float by float: parking them in LDS so that the workgroup's contiguous run
// leaves as float4 (as gsrast_temporal.h does for its embedding rows) was built and measured beside this on an MI355X and was no faster
// -- forward 0.0189 against 0.0185 ms at 1 M rows, 0.0426 against 0.0413 ms at 3 M; backward 0.0327 / 0.0322 and 0.0813 / 0.0809 ms
// (profiles/project_overhead_stores.json: "staged" beside "lane") -- so the simpler form stays.
#pragma once
#include "gsrast_preprocess.h"

namespace gsrast {

constexpr int PJ_THREADS = 256;                 // rows per workgroup

struct ProjRow { float px, py, z, con0, con1, con2, det, comp, rho; int rad; };

// One row of the forward.  c6: the 3-D covariance (from scale / rotation, or the caller's).  Returns whether the row is visible; cv is
// filled whenever view z > 0.2 (the backward reads it on visible rows only).
template <bool AA>
__device__ __forceinline__ bool project_row(const float p[3], const float c6[6], const Cam& cam, Cov2D& cv, ProjRow& o)
{
    float ph[4], pv[3];
    xform4x4(p, cam.proj, ph);
    const float pw = 1.0f / (ph[3] + 0.0000001f);
    const float pp0 = ph[0] * pw, pp1 = ph[1] * pw;
    xform4x3(p, cam.view, pv);
    if (!(pv[2] > 0.2f)) return false;
    cov2d_eval(p, cam, c6, cv);
    const float det = cv.a * cv.c - cv.b * cv.b;
    if (!(det != 0.0f)) return false;
    const float det_inv = 1.0f / det;
    o.con0 = cv.c * det_inv; o.con1 = -cv.b * det_inv; o.con2 = cv.a * det_inv;
    const float mid = 0.5f * (cv.a + cv.c);
    float disc = mid * mid - det; disc = disc < 0.1f ? 0.1f : disc;
    const float l1 = mid + sqrtf(disc), l2 = mid - sqrtf(disc);
    const float lmax = l1 < l2 ? l2 : l1;
    const float my_radius = ceilf(3.0f * sqrtf(lmax));
    o.px = ndc2pix(pp0, cam.W); o.py = ndc2pix(pp1, cam.H);
    o.rad = (int)my_radius;
    int rmin[2], rmax[2];
    tile_rect(o.px, o.py, o.rad, cam.gx, cam.gy, rmin, rmax);
    const int area = (rmax[0] - rmin[0]) * (rmax[1] - rmin[1]);
    if (area == 0) return false;
    o.z = pv[2]; o.det = det;
    o.rho = AA ? aa_rho(cv, det) : 1.0f;
    o.comp = AA ? aa_comp(o.rho) : 1.0f;
    return true;
}

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
    ProjRow r;
    const bool vis = project_row<AA>(in.p, in.c6, cam, cv, r);
    const float con[3] = { vis ? r.con0 : 0.0f, vis ? r.con1 : 0.0f, vis ? r.con2 : 0.0f };
    reinterpret_cast<float2*>(means2D)[i] = vis ? make_float2(r.px, r.py) : make_float2(0.0f, 0.0f);
    depths[i] = vis ? r.z : 0.0f;
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
    if (g_conics) { gc[0] = g_conics[3 * ic]; gc[1] = g_conics[3 * ic + 1]; gc[2] = g_conics[3 * ic + 2]; }
    if (AA && g_comp) gk = g_comp[ic];
    const Cam cam = load_cam(cam_args);
    const float q[4] = { in.q.x, in.q.y, in.q.z, in.q.w };
    M3 Mm;
    Cov2D cv;
    ProjRow r;
    if (i >= (size_t)P) return;
    if (!cov3D_precomp) cov3d_from_scale_rot(in.s, cam.scale_mod, q, in.c6, Mm);
    const bool vis = project_row<AA>(in.p, in.c6, cam, cv, r);
    float dmean[3] = { 0.0f, 0.0f, 0.0f }, ds[3] = { 0.0f, 0.0f, 0.0f }, dcov[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    float4 dq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vis) {
        // a frustum-clamped axis: the clamped value is a constant of J, and t.x / t.y get no direct gradient
        const float xgm = (cv.txtz < -cv.limx || cv.txtz > cv.limx) ? 0.0f : 1.0f;
        const float ygm = (cv.tytz < -cv.limy || cv.tytz > cv.limy) ? 0.0f : 1.0f;
        const float a = cv.a, b = cv.b, c = cv.c, det = r.det;
        const M3& T = cv.T; const M3& V = cv.V; const M3& Wm = cv.Wm;
        // conic = (c, -b, a) / det  ->  the covariance's three numbers (b: the scalar c01), with 1 / (det^2 + 1e-7) for 1 / det^2
        const float det2inv = 1.0f / ((det * det) + 0.0000001f);
        float dL_da = 0.0f, dL_db = 0.0f, dL_dc = 0.0f;
        if (det2inv != 0.0f) {
            dL_da = det2inv * (-c * c * gc[0] + b * c * gc[1] + (det - a * c) * gc[2]);
            dL_dc = det2inv * (-a * a * gc[2] + a * b * gc[1] + (det - a * c) * gc[0]);
            dL_db = det2inv * (2.0f * b * c * gc[0] - (det + 2.0f * b * b) * gc[1] + 2.0f * a * b * gc[2]);
            if (AA && r.rho > AA_FLOOR) {      // comp = sqrt(rho):  d comp = comp 0.5 d(ln rho),  rho = (c00 c11 - b^2) / det
                const float w = gk * r.comp * 0.5f;
                const float icov = 1.0f / (cv.c00 * cv.c11 - b * b), ih = 1.0f / det;
                dL_da = dL_da + w * (cv.c11 * icov - c * ih);
                dL_dc = dL_dc + w * (cv.c00 * icov - a * ih);
                dL_db = dL_db + w * (2.0f * b * ih - 2.0f * b * icov);
            }
            // cov2D = T Sigma T^T (rows 0, 1 of T)  ->  Sigma's six numbers (off-diagonal ones stand for both entries)
            dcov[0] = T.m[0][0] * T.m[0][0] * dL_da + T.m[0][0] * T.m[1][0] * dL_db + T.m[1][0] * T.m[1][0] * dL_dc;
            dcov[3] = T.m[0][1] * T.m[0][1] * dL_da + T.m[0][1] * T.m[1][1] * dL_db + T.m[1][1] * T.m[1][1] * dL_dc;
            dcov[5] = T.m[0][2] * T.m[0][2] * dL_da + T.m[0][2] * T.m[1][2] * dL_db + T.m[1][2] * T.m[1][2] * dL_dc;
            dcov[1] = 2.0f * T.m[0][0] * T.m[0][1] * dL_da + (T.m[0][0] * T.m[1][1] + T.m[0][1] * T.m[1][0]) * dL_db + 2.0f * T.m[1][0] * T.m[1][1] * dL_dc;
            dcov[2] = 2.0f * T.m[0][0] * T.m[0][2] * dL_da + (T.m[0][0] * T.m[1][2] + T.m[0][2] * T.m[1][0]) * dL_db + 2.0f * T.m[1][0] * T.m[1][2] * dL_dc;
            dcov[4] = 2.0f * T.m[0][2] * T.m[0][1] * dL_da + (T.m[0][1] * T.m[1][2] + T.m[0][2] * T.m[1][1]) * dL_db + 2.0f * T.m[1][1] * T.m[1][2] * dL_dc;
        }
        // ... -> T = J W  ->  the four non-constant entries of J  ->  the view-space mean t
        float dT[2][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float r0 = T.m[0][0] * V.m[k][0] + T.m[0][1] * V.m[k][1] + T.m[0][2] * V.m[k][2];
            const float r1 = T.m[1][0] * V.m[k][0] + T.m[1][1] * V.m[k][1] + T.m[1][2] * V.m[k][2];
            dT[0][k] = 2.0f * r0 * dL_da + r1 * dL_db;
            dT[1][k] = 2.0f * r1 * dL_dc + r0 * dL_db;
        }
        const float dJ00 = Wm.m[0][0] * dT[0][0] + Wm.m[0][1] * dT[0][1] + Wm.m[0][2] * dT[0][2];
        const float dJ02 = Wm.m[2][0] * dT[0][0] + Wm.m[2][1] * dT[0][1] + Wm.m[2][2] * dT[0][2];
        const float dJ11 = Wm.m[1][0] * dT[1][0] + Wm.m[1][1] * dT[1][1] + Wm.m[1][2] * dT[1][2];
        const float dJ12 = Wm.m[2][0] * dT[1][0] + Wm.m[2][1] * dT[1][1] + Wm.m[2][2] * dT[1][2];
        const float tz = 1.0f / cv.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
        const float dtx = xgm * -cam.fx * tz2 * dJ02;
        const float dty = ygm * -cam.fy * tz2 * dJ12;
        float dtz = -cam.fx * tz2 * dJ00 - cam.fy * tz2 * dJ11 + (2.0f * cam.fx * cv.t[0]) * tz3 * dJ02 + (2.0f * cam.fy * cv.t[1]) * tz3 * dJ12;
        dtz += gz;                                     // depths is t.z itself
        dmean[0] = cam.view[0] * dtx + cam.view[1] * dty + cam.view[2] * dtz;
        dmean[1] = cam.view[4] * dtx + cam.view[5] * dty + cam.view[6] * dtz;
        dmean[2] = cam.view[8] * dtx + cam.view[9] * dty + cam.view[10] * dtz;
        // the pixel centre: pix = ((ndc + 1) S - 1) / 2,  ndc = hom.xy / (hom.w + 1e-7)
        const float g2x = 0.5f * (float)cam.W * gm.x, g2y = 0.5f * (float)cam.H * gm.y;
        float mh[4];
        xform4x4(in.p, cam.proj, mh);
        const float mw = 1.0f / (mh[3] + 0.0000001f);
        const float* pj = cam.proj;
        const float mul1 = mh[0] * mw * mw, mul2 = mh[1] * mw * mw;
        dmean[0] += (pj[0] * mw - pj[3] * mul1) * g2x + (pj[1] * mw - pj[3] * mul2) * g2y;
        dmean[1] += (pj[4] * mw - pj[7] * mul1) * g2x + (pj[5] * mw - pj[7] * mul2) * g2y;
        dmean[2] += (pj[8] * mw - pj[11] * mul1) * g2x + (pj[9] * mw - pj[11] * mul2) * g2y;
        if (!cov3D_precomp) {                          // Sigma = M^T M, M = S R  ->  scale_modifier * scale, and the quaternion as given
            M3 R;
            quat_to_R(q, R);
            const float sm[3] = { cam.scale_mod * in.s[0], cam.scale_mod * in.s[1], cam.scale_mod * in.s[2] };
            M3 dSig, dM;
            dSig.m[0][0] = dcov[0]; dSig.m[0][1] = 0.5f * dcov[1]; dSig.m[0][2] = 0.5f * dcov[2];
            dSig.m[1][0] = 0.5f * dcov[1]; dSig.m[1][1] = dcov[3]; dSig.m[1][2] = 0.5f * dcov[4];
            dSig.m[2][0] = 0.5f * dcov[2]; dSig.m[2][1] = 0.5f * dcov[4]; dSig.m[2][2] = dcov[5];
#pragma unroll
            for (int cc = 0; cc < 3; cc++)
#pragma unroll
                for (int rr = 0; rr < 3; rr++)
                    dM.m[cc][rr] = 2.0f * Mm.m[0][rr] * dSig.m[cc][0] + 2.0f * Mm.m[1][rr] * dSig.m[cc][1] + 2.0f * Mm.m[2][rr] * dSig.m[cc][2];
#pragma unroll
            for (int k = 0; k < 3; k++) ds[k] = R.m[0][k] * dM.m[0][k] + R.m[1][k] * dM.m[1][k] + R.m[2][k] * dM.m[2][k];
#define PJ_D(cc, rr) (dM.m[rr][cc] * sm[cc])
            const float qr = q[0], x = q[1], y = q[2], z = q[3];
            dq.x = 2.0f * z * (PJ_D(0, 1) - PJ_D(1, 0)) + 2.0f * y * (PJ_D(2, 0) - PJ_D(0, 2)) + 2.0f * x * (PJ_D(1, 2) - PJ_D(2, 1));
            dq.y = 2.0f * y * (PJ_D(1, 0) + PJ_D(0, 1)) + 2.0f * z * (PJ_D(2, 0) + PJ_D(0, 2)) + 2.0f * qr * (PJ_D(1, 2) - PJ_D(2, 1)) - 4.0f * x * (PJ_D(2, 2) + PJ_D(1, 1));
            dq.z = 2.0f * x * (PJ_D(1, 0) + PJ_D(0, 1)) + 2.0f * qr * (PJ_D(2, 0) - PJ_D(0, 2)) + 2.0f * z * (PJ_D(1, 2) + PJ_D(2, 1)) - 4.0f * y * (PJ_D(2, 2) + PJ_D(0, 0));
            dq.w = 2.0f * qr * (PJ_D(0, 1) - PJ_D(1, 0)) + 2.0f * x * (PJ_D(2, 0) + PJ_D(0, 2)) + 2.0f * y * (PJ_D(1, 2) + PJ_D(2, 1)) - 4.0f * z * (PJ_D(1, 1) + PJ_D(0, 0));
#undef PJ_D
        }
    }
    if (d_means3D) project_store_row<3>(d_means3D, i, dmean);      // (uniform, each of the four)
    if (d_scales) project_store_row<3>(d_scales, i, ds);
    if (d_rot) reinterpret_cast<float4*>(d_rot)[i] = dq;
    if (d_cov3D) project_store_row<6>(d_cov3D, i, dcov);
}

}  // namespace gsrast
