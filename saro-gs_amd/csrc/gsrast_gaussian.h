// gsrast_gaussian.h -- the per-Gaussian maths, once: camera constants, R(q), the 3-D and the screen-space covariance, the anti-aliasing
// ratio, one row of the forward projection and the backward chain behind it.  Device functions and small structs only, no kernel, so that
// both translation units take it: the renderer (gsrast_preprocess.h) and the projection call (gsrast_project.h) run the same row and the
// same chain, densification and the MCMC noise (gsrast_densify.h, gsrast_mcmc.h) the same R(q).  fp32 in a fixed evaluation order: the
// units are built with -ffp-contract=off and correctly rounded divide / sqrt, so a caller of these functions gets the same bits as any other.
//
// Reference behaviour restated here (RST = reference cuda_rasterizer/):
//   forward : RST/forward.cu:155-256 preprocessCUDA, :74-113 computeCov2D, :118-152 computeCov3D, RST/auxiliary.h:41-56 ndc2Pix/getRect
//   backward: RST/backward.cu:144-274 computeCov2DCUDA, :346-396 preprocessCUDA, :278-341 computeCov3D
#pragma once
#include "gsrast_common.h"

namespace gsrast {

struct Cam {            // per-call constants, passed by value in kernarg (SGPRs)
    float view[16];     // transposed storage: view[4*c + r] = V[r][c]
    float proj[16];
    float campos[3];
    float tanx, tany, fx, fy, scale_mod;
    int W, H, gx, gy;
};

// What the host passes: the three camera arrays stay in HBM (no D2H copy, no sync); every lane
// reads them through uniform (scalar) loads at kernel entry.
struct CamArgs {
    const float* view; const float* proj; const float* campos;
    float tanx, tany, fx, fy, scale_mod;
    int W, H, gx, gy;
};
__device__ __forceinline__ Cam load_cam(const CamArgs& a)
{
    Cam c;
#pragma unroll
    for (int k = 0; k < 16; k++) { c.view[k] = a.view[k]; c.proj[k] = a.proj[k]; }
    if (a.campos) { c.campos[0] = a.campos[0]; c.campos[1] = a.campos[1]; c.campos[2] = a.campos[2]; }
    else { c.campos[0] = c.campos[1] = c.campos[2] = 0.0f; }
    c.tanx = a.tanx; c.tany = a.tany; c.fx = a.fx; c.fy = a.fy; c.scale_mod = a.scale_mod;
    c.W = a.W; c.H = a.H; c.gx = a.gx; c.gy = a.gy;
    return c;
}

struct M3 { float m[3][3]; };  // m[c][r], column-major like the reference's glm::mat3

__device__ __forceinline__ void xform4x3(const float p[3], const float* M, float o[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = M[r] * p[0] + M[4 + r] * p[1] + M[8 + r] * p[2] + M[12 + r];
}
__device__ __forceinline__ void xform4x4(const float p[3], const float* M, float o[4])
{
#pragma unroll
    for (int r = 0; r < 4; r++) o[r] = M[r] * p[0] + M[4 + r] * p[1] + M[8 + r] * p[2] + M[12 + r];
}
__device__ __forceinline__ float ndc2pix(float v, int S)
{ // evaluated in double like the reference (1.0 / 0.5 literals), then narrowed
    return (float)((((double)v + 1.0) * S - 1.0) * 0.5);
}
__device__ __forceinline__ void tile_rect(float px, float py, int rad, int gx, int gy, int rmin[2], int rmax[2])
{
    int a;
    a = (int)((px - rad) / TILE_X); a = a > 0 ? a : 0; rmin[0] = gx < a ? gx : a;
    a = (int)((py - rad) / TILE_Y); a = a > 0 ? a : 0; rmin[1] = gy < a ? gy : a;
    a = (int)((px + rad + TILE_X - 1) / TILE_X); a = a > 0 ? a : 0; rmax[0] = gx < a ? gx : a;
    a = (int)((py + rad + TILE_Y - 1) / TILE_Y); a = a > 0 ? a : 0; rmax[1] = gy < a ? gy : a;
}

__device__ __forceinline__ void quat_to_R(const float q[4], M3& R)
{
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R.m[0][0] = 1.0f - 2.0f * (y * y + z * z); R.m[0][1] = 2.0f * (x * y - r * z); R.m[0][2] = 2.0f * (x * z + r * y);
    R.m[1][0] = 2.0f * (x * y + r * z); R.m[1][1] = 1.0f - 2.0f * (x * x + z * z); R.m[1][2] = 2.0f * (y * z - r * x);
    R.m[2][0] = 2.0f * (x * z - r * y); R.m[2][1] = 2.0f * (y * z + r * x); R.m[2][2] = 1.0f - 2.0f * (x * x + y * y);
}
// Sigma = (S R)^T (S R), upper triangle; M = S*R returned for the backward.
__device__ __forceinline__ void cov3d_from_scale_rot(const float s_in[3], float mod, const float q[4], float c6[6], M3& M)
{
    M3 R; quat_to_R(q, R);
    const float s[3] = { mod * s_in[0], mod * s_in[1], mod * s_in[2] };
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) M.m[c][r] = s[r] * R.m[c][r];
#define GS_SIG(c, r) (M.m[r][0] * M.m[c][0] + M.m[r][1] * M.m[c][1] + M.m[r][2] * M.m[c][2])
    c6[0] = GS_SIG(0, 0); c6[1] = GS_SIG(0, 1); c6[2] = GS_SIG(0, 2);
    c6[3] = GS_SIG(1, 1); c6[4] = GS_SIG(1, 2); c6[5] = GS_SIG(2, 2);
#undef GS_SIG
}

// a, b, c: the screen-space covariance with the 0.3 px^2 dilation (b = c01); c00, c11: its diagonal BEFORE the dilation, for the
// anti-aliasing filter (aa_rho below) -- not recovered as a - 0.3f, which would add a rounding error to the quantity that cancels.
// (Dead in the plain kernels: nothing reads them there.)
struct Cov2D { float t[3]; float txtz, tytz, limx, limy; M3 T, Wm, V; float a, b, c; float c00, c11; };

__device__ __forceinline__ void cov2d_eval(const float mean[3], const Cam& cam, const float c6[6], Cov2D& o)
{
    float t[3];
    xform4x3(mean, cam.view, t);
    o.limx = 1.3f * cam.tanx; o.limy = 1.3f * cam.tany;
    o.txtz = t[0] / t[2]; o.tytz = t[1] / t[2];
    float cx = o.txtz < -o.limx ? -o.limx : o.txtz; cx = o.limx < cx ? o.limx : cx;
    float cy = o.tytz < -o.limy ? -o.limy : o.tytz; cy = o.limy < cy ? o.limy : cy;
    t[0] = cx * t[2]; t[1] = cy * t[2];
    o.t[0] = t[0]; o.t[1] = t[1]; o.t[2] = t[2];
    const float J00 = cam.fx / t[2], J02 = -(cam.fx * t[0]) / (t[2] * t[2]);
    const float J11 = cam.fy / t[2], J12 = -(cam.fy * t[1]) / (t[2] * t[2]);
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) o.Wm.m[c][r] = cam.view[4 * r + c];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o.T.m[0][r] = o.Wm.m[0][r] * J00 + o.Wm.m[2][r] * J02;
        o.T.m[1][r] = o.Wm.m[1][r] * J11 + o.Wm.m[2][r] * J12;
        o.T.m[2][r] = 0.0f;
    }
    o.V.m[0][0] = c6[0]; o.V.m[0][1] = c6[1]; o.V.m[0][2] = c6[2];
    o.V.m[1][0] = c6[1]; o.V.m[1][1] = c6[3]; o.V.m[1][2] = c6[4];
    o.V.m[2][0] = c6[2]; o.V.m[2][1] = c6[4]; o.V.m[2][2] = c6[5];
    float A[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int r = 0; r < 2; r++)
            A[k][r] = o.T.m[r][0] * o.V.m[0][k] + o.T.m[r][1] * o.V.m[1][k] + o.T.m[r][2] * o.V.m[2][k];
    const float c00 = A[0][0] * o.T.m[0][0] + A[1][0] * o.T.m[0][1] + A[2][0] * o.T.m[0][2];
    const float c01 = A[0][1] * o.T.m[0][0] + A[1][1] * o.T.m[0][1] + A[2][1] * o.T.m[0][2];
    const float c11 = A[0][1] * o.T.m[1][0] + A[1][1] * o.T.m[1][1] + A[2][1] * o.T.m[1][2];
    o.a = c00 + 0.3f; o.b = c01; o.c = c11 + 0.3f;
    o.c00 = c00; o.c11 = c11;
}

// ---- anti-aliasing: the 2-D Mip filter of Mip-Splatting (Yu et al., CVPR 2024), as upstream 3DGS's `antialiasing` ----------------
// The 0.3 px^2 dilation above widens every footprint; with AA the opacity is scaled by the ratio of the two footprints' areas so that a
// small or distant Gaussian keeps its energy:  rho = det(cov2D) / det(cov2D + 0.3 I),  comp = sqrt(max(AA_FLOOR, rho)),  o_eff = o * comp.
// o_eff replaces o in every downstream use (rec1.y, the skip threshold, the predicted cut's mass); conic, radius and tiles do not change.
// det_h is the forward's `det` (the backward's `denom`): the same expression on the same operands.  rho <= 0 (fp32 cancellation of a
// needle) lands on the floor, where the covariance term of the backward is zero.
constexpr float AA_FLOOR = 0.000025f;      // upstream's literal
__device__ __forceinline__ float aa_rho(const Cov2D& cv, float det_h)
{
    const float det_cov = cv.c00 * cv.c11 - cv.b * cv.b;
    return det_cov / det_h;
}
__device__ __forceinline__ float aa_comp(float rho) { return sqrtf(fmaxf(AA_FLOOR, rho)); }

// ---- one row of the forward -------------------------------------------------------------------------------------------------------
// In two halves, because the 3-D covariance stands between them and the renderer builds it (and exports it for "debug_state") only for a
// row in front of the near plane.  A row is visible iff  view z > 0.2  (project_head),  det != 0  and its tile rectangle has non-zero
// area (project_row) -- the reference's rule.
struct ProjHead { float pp0, pp1, t[3]; };      // the centre in ndc, the view-space mean (t[2]: the depth)
__device__ __forceinline__ bool project_head(const float p[3], const Cam& cam, ProjHead& h)
{
    float ph[4];
    xform4x4(p, cam.proj, ph);
    const float pw = 1.0f / (ph[3] + 0.0000001f);
    h.pp0 = ph[0] * pw; h.pp1 = ph[1] * pw;
    xform4x3(p, cam.view, h.t);
    return h.t[2] > 0.2f;
}

// rmin, rmax: the tile rectangle (tile_rect); comp, rho: 1 without AA.
struct ProjRow { float px, py, con0, con1, con2, det, comp, rho; int rad, rmin[2], rmax[2]; };

// c6: the 3-D covariance (from scale / rotation, or the caller's).  Returns whether the row is visible; cv is filled either way (the
// backward reads it on visible rows only).
template <bool AA>
__device__ __forceinline__ bool project_row(const float p[3], const ProjHead& h, const float c6[6], const Cam& cam, Cov2D& cv, ProjRow& o)
{
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
    o.px = ndc2pix(h.pp0, cam.W); o.py = ndc2pix(h.pp1, cam.H);
    o.rad = (int)my_radius;
    tile_rect(o.px, o.py, o.rad, cam.gx, cam.gy, o.rmin, o.rmax);
    const int area = (o.rmax[0] - o.rmin[0]) * (o.rmax[1] - o.rmin[1]);
    if (area == 0) return false;
    o.det = det;
    o.rho = AA ? aa_rho(cv, det) : 1.0f;
    o.comp = AA ? aa_comp(o.rho) : 1.0f;
    return true;
}

// ---- the backward chain of a visible row -------------------------------------------------------------------------------------------
// With the reference's conventions:  a frustum-clamped t.x / t.z, t.y / t.z enters J as a constant;  d conic / d cov2D uses
// 1 / (det^2 + 1e-7);  the compensation has no gradient where rho sits on its floor.  Every intermediate comes back: the renderer's
// camera-pose sums read dT, dtx / dty / dtz, tz, tz2, mh and mw.
struct ProjGrad {
    float dL_da, dL_db, dL_dc;      // dL / d(a, b, c) of Cov2D (b: the scalar c01)
    float dcov[6];                  // dL / d(the 3-D covariance's six numbers); an off-diagonal one stands for both entries
    float dT[2][3];
    float dtx, dty, dtz, tz, tz2;   // dL / d(view-space mean);  1 / t.z and its square
    float mh[4], mw;                // [mean, 1] @ proj;  1 / (mh[3] + 1e-7)
    float dmean[3];
};

// det: the forward's.  dcx, dcy, dcz: dL / d(conic), the MIDDLE one halved -- the stored middle conic counts for both off-diagonal entries
// and the renderer's gradient record carries half of its gradient.  aa_on / aa_w: above AA_FLOOR, the weight of d(ln rho) -- dL / d(comp)
// * comp * 0.5.  g2x, g2y: dL / d(centre) in ndc units.  has_gz / gz: dL / d(view z) from outside the chain.
__device__ __forceinline__ void project_backward(const float mean[3], const Cam& cam, const Cov2D& cv, float det, float dcx, float dcy, float dcz,
                                                 bool aa_on, float aa_w, float g2x, float g2y, bool has_gz, float gz, ProjGrad& g)
{
    // a frustum-clamped axis: the clamped value is a constant of J, and t.x / t.y get no direct gradient
    const float xgm = (cv.txtz < -cv.limx || cv.txtz > cv.limx) ? 0.0f : 1.0f;
    const float ygm = (cv.tytz < -cv.limy || cv.tytz > cv.limy) ? 0.0f : 1.0f;
    const float a = cv.a, b = cv.b, c = cv.c;
    const M3& T = cv.T; const M3& V = cv.V; const M3& Wm = cv.Wm;
    // conic = (c, -b, a) / det  ->  the covariance's three numbers, with 1 / (det^2 + 1e-7) for 1 / det^2
    const float det2inv = 1.0f / ((det * det) + 0.0000001f);
    float dL_da = 0, dL_db = 0, dL_dc = 0;
    float dcov[6];
    if (det2inv != 0) {
        dL_da = det2inv * (-c * c * dcx + 2.0f * b * c * dcy + (det - a * c) * dcz);
        dL_dc = det2inv * (-a * a * dcz + 2.0f * a * b * dcy + (det - a * c) * dcx);
        dL_db = det2inv * 2.0f * (b * c * dcx - (det + 2.0f * b * b) * dcy + a * b * dcz);
        if (aa_on) {      // comp = sqrt(rho):  d comp = comp 0.5 d(ln rho),  rho = (c00 c11 - b^2) / det
            const float icov = 1.0f / (cv.c00 * cv.c11 - b * b), ih = 1.0f / det;
            dL_da = dL_da + aa_w * (cv.c11 * icov - c * ih);
            dL_dc = dL_dc + aa_w * (cv.c00 * icov - a * ih);
            dL_db = dL_db + aa_w * (2.0f * b * ih - 2.0f * b * icov);
        }
        // cov2D = T Sigma T^T (rows 0, 1 of T)  ->  Sigma's six numbers
        dcov[0] = (T.m[0][0] * T.m[0][0] * dL_da + T.m[0][0] * T.m[1][0] * dL_db + T.m[1][0] * T.m[1][0] * dL_dc);
        dcov[3] = (T.m[0][1] * T.m[0][1] * dL_da + T.m[0][1] * T.m[1][1] * dL_db + T.m[1][1] * T.m[1][1] * dL_dc);
        dcov[5] = (T.m[0][2] * T.m[0][2] * dL_da + T.m[0][2] * T.m[1][2] * dL_db + T.m[1][2] * T.m[1][2] * dL_dc);
        dcov[1] = 2.0f * T.m[0][0] * T.m[0][1] * dL_da + (T.m[0][0] * T.m[1][1] + T.m[0][1] * T.m[1][0]) * dL_db + 2.0f * T.m[1][0] * T.m[1][1] * dL_dc;
        dcov[2] = 2.0f * T.m[0][0] * T.m[0][2] * dL_da + (T.m[0][0] * T.m[1][2] + T.m[0][2] * T.m[1][0]) * dL_db + 2.0f * T.m[1][0] * T.m[1][2] * dL_dc;
        dcov[4] = 2.0f * T.m[0][2] * T.m[0][1] * dL_da + (T.m[0][1] * T.m[1][2] + T.m[0][2] * T.m[1][1]) * dL_db + 2.0f * T.m[1][1] * T.m[1][2] * dL_dc;
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) dcov[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) g.dcov[k] = dcov[k];
    g.dL_da = dL_da; g.dL_db = dL_db; g.dL_dc = dL_dc;
    // ... -> T = J W  ->  the four non-constant entries of J  ->  the view-space mean t
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float r0 = T.m[0][0] * V.m[k][0] + T.m[0][1] * V.m[k][1] + T.m[0][2] * V.m[k][2];
        const float r1 = T.m[1][0] * V.m[k][0] + T.m[1][1] * V.m[k][1] + T.m[1][2] * V.m[k][2];
        g.dT[0][k] = 2.0f * r0 * dL_da + r1 * dL_db;
        g.dT[1][k] = 2.0f * r1 * dL_dc + r0 * dL_db;
    }
    const float dJ00 = Wm.m[0][0] * g.dT[0][0] + Wm.m[0][1] * g.dT[0][1] + Wm.m[0][2] * g.dT[0][2];
    const float dJ02 = Wm.m[2][0] * g.dT[0][0] + Wm.m[2][1] * g.dT[0][1] + Wm.m[2][2] * g.dT[0][2];
    const float dJ11 = Wm.m[1][0] * g.dT[1][0] + Wm.m[1][1] * g.dT[1][1] + Wm.m[1][2] * g.dT[1][2];
    const float dJ12 = Wm.m[2][0] * g.dT[1][0] + Wm.m[2][1] * g.dT[1][1] + Wm.m[2][2] * g.dT[1][2];
    const float tz = 1.0f / cv.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    g.tz = tz; g.tz2 = tz2;
    g.dtx = xgm * -cam.fx * tz2 * dJ02;
    g.dty = ygm * -cam.fy * tz2 * dJ12;
    g.dtz = -cam.fx * tz2 * dJ00 - cam.fy * tz2 * dJ11 + (2.0f * cam.fx * cv.t[0]) * tz3 * dJ02 + (2.0f * cam.fy * cv.t[1]) * tz3 * dJ12;
    if (has_gz) g.dtz += gz;          // (not added at all without one: -0.0f + 0.0f is +0.0f)
    g.dmean[0] = cam.view[0] * g.dtx + cam.view[1] * g.dty + cam.view[2] * g.dtz;
    g.dmean[1] = cam.view[4] * g.dtx + cam.view[5] * g.dty + cam.view[6] * g.dtz;
    g.dmean[2] = cam.view[8] * g.dtx + cam.view[9] * g.dty + cam.view[10] * g.dtz;
    // the centre through the perspective divide: ndc = hom.xy / (hom.w + 1e-7)
    xform4x4(mean, cam.proj, g.mh);
    g.mw = 1.0f / (g.mh[3] + 0.0000001f);
    const float mw = g.mw;
    const float* pj = cam.proj;
    const float mul1 = g.mh[0] * mw * mw, mul2 = g.mh[1] * mw * mw;
    g.dmean[0] += (pj[0] * mw - pj[3] * mul1) * g2x + (pj[1] * mw - pj[3] * mul2) * g2y;
    g.dmean[1] += (pj[4] * mw - pj[7] * mul1) * g2x + (pj[5] * mw - pj[7] * mul2) * g2y;
    g.dmean[2] += (pj[8] * mw - pj[11] * mul1) * g2x + (pj[9] * mw - pj[11] * mul2) * g2y;
}

// Sigma = M^T M, M = S R  ->  ds = dL / d(sm) and dq = dL / d(q), the quaternion as given.  sm: scale_modifier * scale; Mm: cov3d_from_scale_rot's.
__device__ __forceinline__ void cov3d_backward(const float q[4], const float sm[3], const M3& Mm, const float dcov[6], float ds[3], float4& dq)
{
    M3 R;
    quat_to_R(q, R);
    M3 dSig, dM;
    dSig.m[0][0] = dcov[0]; dSig.m[0][1] = 0.5f * dcov[1]; dSig.m[0][2] = 0.5f * dcov[2];
    dSig.m[1][0] = 0.5f * dcov[1]; dSig.m[1][1] = dcov[3]; dSig.m[1][2] = 0.5f * dcov[4];
    dSig.m[2][0] = 0.5f * dcov[2]; dSig.m[2][1] = 0.5f * dcov[4]; dSig.m[2][2] = dcov[5];
#pragma unroll
    for (int cc = 0; cc < 3; cc++)
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
            dM.m[cc][rr] = 2.0f * Mm.m[0][rr] * dSig.m[cc][0] + 2.0f * Mm.m[1][rr] * dSig.m[cc][1] + 2.0f * Mm.m[2][rr] * dSig.m[cc][2];
    // Rt[k][j] = R[j][k], dMt[k][j] = dM[j][k]
#pragma unroll
    for (int k = 0; k < 3; k++) ds[k] = R.m[0][k] * dM.m[0][k] + R.m[1][k] * dM.m[1][k] + R.m[2][k] * dM.m[2][k];
#define D_(cc, rr) (dM.m[rr][cc] * sm[cc])
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    dq.x = 2.0f * z * (D_(0, 1) - D_(1, 0)) + 2.0f * y * (D_(2, 0) - D_(0, 2)) + 2.0f * x * (D_(1, 2) - D_(2, 1));
    dq.y = 2.0f * y * (D_(1, 0) + D_(0, 1)) + 2.0f * z * (D_(2, 0) + D_(0, 2)) + 2.0f * r * (D_(1, 2) - D_(2, 1)) - 4.0f * x * (D_(2, 2) + D_(1, 1));
    dq.z = 2.0f * x * (D_(1, 0) + D_(0, 1)) + 2.0f * r * (D_(2, 0) - D_(0, 2)) + 2.0f * z * (D_(1, 2) + D_(2, 1)) - 4.0f * y * (D_(2, 2) + D_(0, 0));
    dq.w = 2.0f * r * (D_(0, 1) - D_(1, 0)) + 2.0f * x * (D_(2, 0) + D_(0, 2)) + 2.0f * y * (D_(1, 2) + D_(2, 1)) - 4.0f * z * (D_(1, 1) + D_(0, 0));
#undef D_
}

}  // namespace gsrast
