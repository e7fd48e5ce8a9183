// gsrast_train.hip -- the training kernels' half of the C ABI declared in include/gsrast.h: the entry points that never read the renderer's
// state buffers.  Each is argument checks, a scratch layout and launches.  Errors, launch checks, option words and profile timers are the
// process's one set (gsrast_host.h, defined in gsrast_capi.hip), as are the two radix sorts k-NN and hexplane call.
#include "gsrast_host.h"
#include "gsrast_loss.h"
#include "gsrast_epilogue.h"
#include "gsrast_adam.h"
#include "gsrast_densify.h"
#include "gsrast_mcmc.h"
#include "gsrast_mlp.h"
#include "gsrast_mlp_bf16.h"
#include "gsrast_temporal.h"
#include "gsrast_bilagrid.h"
#include "gsrast_normal.h"
#include "gsrast_filter3d.h"
#include "gsrast_knn.h"
#include "gsrast_knn_query.h"
#include "gsrast_hexplane.h"
#include <algorithm>
#include <cmath>

using namespace gsrast;

extern "C" {

int gsrast_activate_forward(int P, int M, const float* xyz, const float* motion_res, const float* rotation,
                            const float* rot_res, const float* scaling, const float* opacity_logit, const float* trbf,
                            const float* features_dc, const float* features_rest, const float* shs_res,
                            float* motion, float* rot, float* scale, float* opacity, float* shs, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || M < 1) return fail(GSRAST_E_ARG, "activate_forward: bad sizes");
    if (P == 0) return GSRAST_OK;
    if (!xyz || !rotation || !scaling || !opacity_logit || !features_dc || (M > 1 && !features_rest) ||
        !motion || !rot || !scale || !opacity || !shs) return fail(GSRAST_E_ARG, "activate_forward: NULL required pointer");
    if (((uintptr_t)rotation | (uintptr_t)rot) & 15) return fail(GSRAST_E_ARG, "activate_forward: rotation / rot must be 16-byte aligned");
    epilogue_small_fwd_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, xyz, motion_res, rotation, rot_res, scaling, opacity_logit, trbf,
                                                             motion, rot, scale, opacity);
    GS_LAUNCHED("epilogue_small_fwd");
    const int row = 3 * M;
    const size_t n = (size_t)P * row;
    if ((row & 3) == 0 && (((uintptr_t)shs | (uintptr_t)shs_res) & 15) == 0) {
        const size_t nq = n / 4;
        epilogue_sh_fwd_kernel<<<(unsigned)((nq + 255) / 256), 256, 0, s>>>(nq, row, features_dc, features_rest, shs_res, shs);
    } else {
        epilogue_sh_fwd_scalar_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, row, features_dc, features_rest, shs_res, shs);
    }
    GS_LAUNCHED("epilogue_sh_fwd");
    return GSRAST_OK;
}

int gsrast_activate_backward(int P, const float* rotation, const float* rot_res, const float* scale, const float* opacity_logit,
                             const float* trbf, const float* d_rot, const float* d_scale, const float* d_opacity,
                             float* d_rotation, float* d_scaling, float* d_rot_res, float* d_opacity_logit, float* d_trbf,
                             void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "activate_backward: bad sizes");
    if (P == 0) return GSRAST_OK;
    if (!rotation || !scale || !opacity_logit || !d_rotation || !d_scaling || !d_opacity_logit)
        return fail(GSRAST_E_ARG, "activate_backward: NULL required pointer");
    if (((uintptr_t)rotation | (uintptr_t)d_rot | (uintptr_t)d_rotation) & 15)
        return fail(GSRAST_E_ARG, "activate_backward: rotation / d_rot / d_rotation must be 16-byte aligned");
    epilogue_small_bwd_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, rotation, rot_res, scale, opacity_logit, trbf, d_rot, d_scale, d_opacity,
                                                             d_rotation, d_scaling, d_rot_res, d_opacity_logit, d_trbf);
    GS_LAUNCHED("epilogue_small_bwd");
    return GSRAST_OK;
}

int gsrast_adam_step(int n_groups, const gsrast_adam_group* groups, double beta1, double beta2, double eps, int step, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_groups < 0 || n_groups > ADAM_MAX_GROUPS || (n_groups > 0 && !groups) || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(GSRAST_E_ARG, "adam_step: bad arguments (at most 8 groups, step >= 1, betas in [0, 1))");
    AdamArgs a{};
    unsigned long long blocks = 0;
    for (int k = 0; k < n_groups; k++) {
        const gsrast_adam_group& g = groups[k];
        if (g.rows < 0 || g.width < 1) return fail(GSRAST_E_ARG, "adam_step: bad group shape");
        const unsigned long long n = (unsigned long long)g.rows * (unsigned long long)g.width;
        if (n && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)) return fail(GSRAST_E_ARG, "adam_step: NULL tensor");
        AdamGroup& o = a.grp[a.n_groups];
        if (n == 0) continue;
        o.p = g.param; o.g = g.grad; o.m = g.exp_avg; o.v = g.exp_avg_sq; o.lr_rows = g.lr_rows; o.lr = g.lr; o.width = (unsigned)g.width;
        o.n = n; o.first_block = blocks; o.n_blocks = (n + ADAM_THREADS * ADAM_PER_THREAD - 1) / (ADAM_THREADS * ADAM_PER_THREAD);
        blocks += o.n_blocks;
        a.n_groups++;
    }
    if (blocks == 0) return GSRAST_OK;
    if (blocks > 0x7FFFFFFFull) return fail(GSRAST_E_OVERFLOW, "adam_step: too many elements for one launch");
    a.b1 = (float)beta1; a.b2 = (float)beta2; a.eps = (float)eps;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);      // as torch: the subtraction in fp64, one rounding
    a.inv_bc1 = (float)(1.0 / (1.0 - std::pow(beta1, (double)step)));
    a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)step)));
    adam_step_kernel<<<(unsigned)blocks, ADAM_THREADS, 0, s>>>(a);
    GS_LAUNCHED("adam_step");
    return GSRAST_OK;
}

int gsrast_adam_step_visible(int n_groups, const gsrast_adam_group* groups, const void* visible, int visible_elem_bytes, long long rows,
                             double beta1, double beta2, double eps, int step, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_groups < 0 || n_groups > ADAM_MAX_GROUPS || (n_groups > 0 && !groups) || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(GSRAST_E_ARG, "adam_step_visible: bad arguments (at most 8 groups, step >= 1, betas in [0, 1))");
    if (visible_elem_bytes != 1 && visible_elem_bytes != 4) return fail(GSRAST_E_ARG, "adam_step_visible: visible_elem_bytes must be 1 or 4");
    if (rows < 0 || rows > 0x7FFFFFFFll) return fail(GSRAST_E_ARG, "adam_step_visible: rows out of range");
    if (rows > 0 && !visible) return fail(GSRAST_E_ARG, "adam_step_visible: NULL visible");
    AdamArgs a{};
    const unsigned long long per_group = ((unsigned long long)rows + ADAM_VIS_ROWS_PER_BLOCK - 1) / ADAM_VIS_ROWS_PER_BLOCK;      // (<= 2^23 blocks per group: the grid cannot overflow)
    unsigned long long blocks = 0;
    for (int k = 0; k < n_groups; k++) {
        const gsrast_adam_group& g = groups[k];
        if (g.rows < 0 || g.width < 1 || (unsigned)g.width > ADAM_VIS_MAX_WIDTH) return fail(GSRAST_E_ARG, "adam_step_visible: bad group shape");
        if (g.rows != rows) return fail(GSRAST_E_ARG, "adam_step_visible: a group's rows differ from the mask's length");
        if (rows && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)) return fail(GSRAST_E_ARG, "adam_step_visible: NULL tensor");
        if (rows == 0) continue;
        AdamGroup& o = a.grp[a.n_groups++];
        o.p = g.param; o.g = g.grad; o.m = g.exp_avg; o.v = g.exp_avg_sq; o.lr_rows = g.lr_rows; o.lr = g.lr; o.width = (unsigned)g.width;
        o.n = (unsigned long long)rows * (unsigned long long)g.width; o.first_block = blocks; o.n_blocks = per_group;
        blocks += per_group;
    }
    if (blocks == 0) return GSRAST_OK;
    a.b1 = (float)beta1; a.b2 = (float)beta2; a.eps = (float)eps;
    a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2);
    a.inv_bc1 = (float)(1.0 / (1.0 - std::pow(beta1, (double)step)));
    a.inv_sqrt_bc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)step)));
    ProfScope ps(K_ADAM_VISIBLE, s);
    adam_step_visible_kernel<<<(unsigned)blocks, ADAM_THREADS, 0, s>>>(a, visible, visible_elem_bytes, (unsigned)rows);
    GS_LAUNCHED("adam_step_visible");
    return GSRAST_OK;
}

// scratch: class byte per source | four arrays of workgroup sums (kept, clone, split, split_all), scanned in place by the plan
namespace {
struct DensifyLayout { size_t cls, sums, total; uint32_t nb; };
DensifyLayout densify_layout(size_t P)
{
    DensifyLayout L; Carver c;
    L.nb = (uint32_t)((P + DN_RUN - 1) / DN_RUN);
    L.cls = c.take(P ? P : 1); L.sums = c.take((size_t)4 * (L.nb ? L.nb : 1) * 4);
    L.total = c.o + 256;
    return L;
}
}
size_t gsrast_densify_scratch_bytes(int P) { return densify_layout(P > 0 ? (size_t)P : 0).total; }

int gsrast_densify_plan(int P, int N, const float* accum, const float* denom, const float* grad_scale, const float* scaling,
                        const float* opacity_logit, const unsigned char* prune_src, float grad_threshold, float size_threshold,
                        float min_opacity, char* scratch, unsigned* counts, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "densify_plan: negative P");
    if (N < 1 || N > DN_MAX_N) return fail(GSRAST_E_ARG, "densify_plan: N (copies per split source) must be in [1, 4]");
    if (!(grad_threshold > 0.0f)) return fail(GSRAST_E_ARG, "densify_plan: grad_threshold must be > 0 (+inf: prune only); with a threshold <= 0 the reference splits its fresh clones");
    if (!scratch || !counts) return fail(GSRAST_E_ARG, "densify_plan: NULL scratch / counts");
    const bool select = grad_threshold < INFINITY;
    if (P > 0 && select && (!scaling || (accum != nullptr) != (denom != nullptr))) return fail(GSRAST_E_ARG, "densify_plan: a finite threshold needs scaling, and accum and denom together");
    if (P > 0 && min_opacity > 0.0f && !opacity_logit) return fail(GSRAST_E_ARG, "densify_plan: min_opacity > 0 without opacity_logit");
    const DensifyLayout L = densify_layout((size_t)P);
    uint32_t* sums = at<uint32_t>(scratch, L.sums);
    if (L.nb) {
        ProfScope ps(K_DENSIFY_CLASSIFY, s);
        densify_classify_kernel<<<L.nb, DN_RUN, 0, s>>>(P, accum, denom, grad_scale, scaling, opacity_logit, prune_src, grad_threshold, select ? 1 : 0,
                                                       size_threshold, min_opacity, at<unsigned char>(scratch, L.cls), sums, L.nb);
        GS_LAUNCHED("densify_classify");
    }
    {
        ProfScope ps(K_DENSIFY_SCAN, s);
        densify_scan_kernel<<<1, DN_RUN, 0, s>>>(sums, L.nb, N, counts);
        GS_LAUNCHED("densify_scan");
    }
    return GSRAST_OK;
}

int gsrast_densify_apply(int P, int N, const char* scratch, const unsigned* counts_host, int n_groups, const gsrast_densify_group* groups,
                         const float* rotation, const float* scaling, const float* noise, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "densify_apply: negative P");
    if (N < 1 || N > DN_MAX_N) return fail(GSRAST_E_ARG, "densify_apply: N (copies per split source) must be in [1, 4]");
    if (n_groups < 0 || n_groups > DN_MAX_GROUPS) return fail(GSRAST_E_ARG, "densify_apply: at most 16 groups");
    if (!scratch || !counts_host || (n_groups > 0 && !groups)) return fail(GSRAST_E_ARG, "densify_apply: NULL scratch / counts / groups");
    const unsigned n_kept = counts_host[0], n_clone = counts_host[1], n_split = counts_host[2], n_split_all = counts_host[3], p_new = counts_host[4];
    if (n_kept > (unsigned)P || n_clone > n_kept || n_split > n_split_all || (unsigned long long)n_kept + n_split_all > (unsigned long long)P ||
        (unsigned long long)p_new != (unsigned long long)n_kept + n_clone + (unsigned long long)N * n_split)
        return fail(GSRAST_E_ARG, "densify_apply: counts are not those of a plan for this P and N");
    DnApplyArgs a{};
    for (int k = 0; k < n_groups; k++) {
        const gsrast_densify_group& g = groups[k];
        if (g.width < 1 || g.width > DN_MAX_WIDTH) return fail(GSRAST_E_ARG, "densify_apply: group width must be in [1, 64]");
        if (g.role != GSRAST_DENSIFY_COPY && g.role != GSRAST_DENSIFY_XYZ && g.role != GSRAST_DENSIFY_SCALING) return fail(GSRAST_E_ARG, "densify_apply: unknown group role");
        if ((g.src_m && !g.dst_m) || (g.src_v && !g.dst_v)) return fail(GSRAST_E_ARG, "densify_apply: src_m / src_v given without dst_m / dst_v");
        if ((g.dst_m && !g.src_m) || (g.dst_v && !g.src_v)) return fail(GSRAST_E_ARG, "densify_apply: dst_m / dst_v given without src_m / src_v");
        if ((P > 0 && !g.src) || (p_new > 0 && !g.dst)) return fail(GSRAST_E_ARG, "densify_apply: NULL src / dst");
        if (g.role == GSRAST_DENSIFY_XYZ && g.width != 3) return fail(GSRAST_E_ARG, "densify_apply: the xyz role needs width 3");
        if (g.role == GSRAST_DENSIFY_XYZ && n_split > 0 && (!rotation || !scaling || !noise)) return fail(GSRAST_E_ARG, "densify_apply: the xyz role needs rotation, scaling and noise while n_split > 0");
        a.grp[k] = DnGroup{ g.src, g.src_m, g.src_v, g.dst, g.dst_m, g.dst_v, g.width, g.role };
    }
    if (P == 0 || n_groups == 0) return GSRAST_OK;
    const DensifyLayout L = densify_layout((size_t)P);
    a.n_groups = n_groups; a.P = P; a.N = N;
    a.n_kept = n_kept; a.n_clone = n_clone; a.n_split = n_split; a.n_split_all = n_split_all; a.p_new = p_new; a.nb = L.nb;
    a.cls = at<unsigned char>(scratch, L.cls); a.sums = at<uint32_t>(scratch, L.sums);
    a.rotation = rotation; a.scaling = scaling; a.noise = noise;
    ProfScope ps(K_DENSIFY_APPLY, s);
    densify_apply_kernel<<<L.nb, DN_RUN, 0, s>>>(a);
    GS_LAUNCHED("densify_apply");
    return GSRAST_OK;
}

int gsrast_densify_scatter(int P, const char* scratch, const unsigned* counts_host, int n_groups, const gsrast_densify_group* groups, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "densify_scatter: negative P");
    if (n_groups < 0 || n_groups > DN_MAX_GROUPS) return fail(GSRAST_E_ARG, "densify_scatter: at most 16 groups");
    if (P > 0 && (!scratch || !counts_host || !groups)) return fail(GSRAST_E_ARG, "densify_scatter: NULL scratch / counts / groups");
    if (P == 0) return GSRAST_OK;
    const unsigned n_kept = counts_host[0];
    if (counts_host[1] || counts_host[2] || counts_host[3] || counts_host[4] != n_kept)
        return fail(GSRAST_E_ARG, "densify_scatter: counts are not those of a prune-only plan (clones or split copies have no transpose)");
    if (n_kept > (unsigned)P) return fail(GSRAST_E_ARG, "densify_scatter: n_kept exceeds P");
    DnApplyArgs a{};
    for (int k = 0; k < n_groups; k++) {
        const gsrast_densify_group& g = groups[k];
        if (g.width < 1 || g.width > DN_MAX_WIDTH) return fail(GSRAST_E_ARG, "densify_scatter: group width must be in [1, 64]");
        if (g.role != GSRAST_DENSIFY_COPY) return fail(GSRAST_E_ARG, "densify_scatter: only the COPY role has a transpose");
        if (g.src_m || g.src_v || g.dst_m || g.dst_v) return fail(GSRAST_E_ARG, "densify_scatter: moments are not scattered (src_m / src_v / dst_m / dst_v must be NULL)");
        if (n_kept > 0 && !g.src) return fail(GSRAST_E_ARG, "densify_scatter: NULL src while n_kept > 0");
        if (!g.dst) return fail(GSRAST_E_ARG, "densify_scatter: NULL dst");
        a.grp[k] = DnGroup{ g.src, nullptr, nullptr, g.dst, nullptr, nullptr, g.width, g.role };
    }
    if (n_groups == 0) return GSRAST_OK;
    const DensifyLayout L = densify_layout((size_t)P);
    a.n_groups = n_groups; a.P = P; a.N = 1;
    a.n_kept = n_kept; a.p_new = n_kept; a.nb = L.nb;
    a.cls = at<unsigned char>(scratch, L.cls); a.sums = at<uint32_t>(scratch, L.sums);
    densify_scatter_kernel<<<L.nb, DN_RUN, 0, s>>>(a);      // (no timer of its own: the profile table is the plan's and the apply's)
    GS_LAUNCHED("densify_scatter");
    return GSRAST_OK;
}

int gsrast_densify_stats_update(int P, const float* grad, const float* visibility_count, const float* radii,
                                float* accum, float* denom, float* max_radii, int grad_is_mean, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "densify_stats_update: negative P");
    if (P == 0) return GSRAST_OK;
    if (!grad || !visibility_count || !accum || !denom || ((max_radii != nullptr) != (radii != nullptr)))
        return fail(GSRAST_E_ARG, "densify_stats_update: NULL pointer (max_radii and radii go together)");
    ProfScope ps(K_DENSIFY_STATS, s);
    densify_stats_update_kernel<<<(unsigned)(((size_t)P + 255) / 256), 256, 0, s>>>(P, grad, visibility_count, radii, accum, denom, max_radii, grad_is_mean ? 1 : 0);
    GS_LAUNCHED("densify_stats_update");
    return GSRAST_OK;
}

// ---- MCMC densification (gsrast_mcmc.h) ----------------------------------------------------------------------------
// scratch: header = counts (4 words) | in-run weight prefix per row | dead byte per row | workgroup weight sums (64 bit) and dead sums,
//          scanned in place by the plan | draws per source | the sources' new values [P][4]
namespace {
struct McmcLayout { size_t hdr, run_prefix, dead, wg_weight, wg_dead, count, vals, total; uint32_t nb; };
McmcLayout mcmc_layout(size_t P)
{
    McmcLayout L; Carver c;
    const size_t Pp = P ? P : 1;
    L.nb = (uint32_t)((P + MC_RUN - 1) / MC_RUN);
    const size_t nbp = L.nb ? L.nb : 1;
    L.hdr = c.take(MC_HDR_WORDS * 4); L.run_prefix = c.take(Pp * 4); L.dead = c.take(Pp); L.wg_weight = c.take(nbp * 8); L.wg_dead = c.take(nbp * 4);
    L.count = c.take(Pp * 4); L.vals = c.take(Pp * 16);
    L.total = c.o + 256;
    return L;
}
// what relocate and grow share: the argument checks, the values pass and the apply launch
int mcmc_apply(const char* who, bool grow, int P, int n, const int* src, char* scratch, const unsigned* counts_host, float min_opacity,
               int n_groups, const gsrast_densify_group* groups, hipStream_t s)
{
    if (P < 0 || n < 0) return refuse(who, "negative P / n");
    if ((long long)P + (long long)n > 0x7FFFFFFFll) return refuse(who, "P + n exceeds 2^31 - 1");
    if (!(min_opacity >= 0.0f && min_opacity < 1.0f)) return refuse(who, "min_opacity must be in [0, 1)");
    if (n_groups < 0 || n_groups > MC_MAX_GROUPS) return refuse(who, "at most 16 groups");
    if (!scratch || (n_groups > 0 && !groups) || (n > 0 && !src)) return refuse(who, "NULL scratch / groups / src");
    if (!grow && !counts_host) return refuse(who, "NULL counts");
    if (P == 0 && n > 0) return refuse(who, "n > 0 draws from an empty model");
    if (counts_host) {
        const unsigned long long W = (unsigned long long)counts_host[2] | ((unsigned long long)counts_host[3] << 32);
        if ((unsigned long long)counts_host[0] + counts_host[1] != (unsigned long long)P || W > ((unsigned long long)counts_host[1] << 24) || (counts_host[1] > 0 && W < counts_host[1]))
            return refuse(who, "counts are not those of a plan for this P");
        if (n > 0 && W == 0) return refuse(who, "n > 0 draws from a total weight of 0 (no alive row)");
        if (!grow && (unsigned)n > counts_host[0]) return refuse(who, "n exceeds the number of dead rows");
    }
    McApplyArgs a{};
    const float *opacity = nullptr, *scaling = nullptr;
    for (int k = 0; k < n_groups; k++) {
        const gsrast_densify_group& g = groups[k];
        if (g.width < 1 || g.width > MC_MAX_WIDTH) return refuse(who, "group width must be in [1, 64]");
        if (g.role != GSRAST_MCMC_COPY && g.role != GSRAST_MCMC_OPACITY && g.role != GSRAST_MCMC_SCALING) return refuse(who, "unknown group role");
        if (g.role == GSRAST_MCMC_OPACITY && g.width != 1) return refuse(who, "the opacity role needs width 1");
        if (g.role == GSRAST_MCMC_SCALING && g.width != 3) return refuse(who, "the scaling role needs width 3");
        if ((g.role == GSRAST_MCMC_OPACITY && opacity) || (g.role == GSRAST_MCMC_SCALING && scaling)) return refuse(who, "more than one opacity / scaling group");
        if (grow) {
            if ((g.src_m && !g.dst_m) || (g.src_v && !g.dst_v) || (g.dst_m && !g.src_m) || (g.dst_v && !g.src_v)) return refuse(who, "src_m / src_v and dst_m / dst_v go together");
            if ((P > 0 && !g.src) || (P + n > 0 && !g.dst)) return refuse(who, "NULL src / dst");
        } else {
            if ((g.src && g.src != g.dst) || (g.src_m && g.src_m != g.dst_m) || (g.src_v && g.src_v != g.dst_v)) return refuse(who, "in place: src / src_m / src_v must be NULL or equal dst / dst_m / dst_v");
            if (P > 0 && !g.dst) return refuse(who, "NULL dst");
        }
        a.grp[k] = grow ? McGroup{ g.src, g.src_m, g.src_v, g.dst, g.dst_m, g.dst_v, g.width, g.role }
                        : McGroup{ g.dst, g.dst_m, g.dst_v, g.dst, g.dst_m, g.dst_v, g.width, g.role };
        if (g.role == GSRAST_MCMC_OPACITY) opacity = a.grp[k].src;
        if (g.role == GSRAST_MCMC_SCALING) scaling = a.grp[k].src;
    }
    if (n > 0 && P > 0 && (!opacity || !scaling)) return refuse(who, "one opacity and one scaling group are required");
    if (P == 0 || n_groups == 0 || (!grow && n == 0)) return GSRAST_OK;
    const McmcLayout L = mcmc_layout((size_t)P);
    a.n_groups = n_groups; a.P = P; a.n = n; a.src = src;
    a.count = at<uint32_t>(scratch, L.count); a.vals = at<float>(scratch, L.vals);
    a.dead = at<unsigned char>(scratch, L.dead); a.wg_dead = at<uint32_t>(scratch, L.wg_dead);
    ProfScope ps(K_MCMC_APPLY, s);
    if (n > 0) {
        mcmc_values_kernel<<<L.nb, MC_RUN, 0, s>>>(P, a.count, opacity, scaling, min_opacity, at<float>(scratch, L.vals));
        GS_LAUNCHED("mcmc_values");
    }
    if (grow) {
        mcmc_apply_kernel<true><<<(unsigned)(((size_t)P + (size_t)n + MC_RUN - 1) / MC_RUN), MC_RUN, 0, s>>>(a);
        GS_LAUNCHED("mcmc_grow");
    } else {
        mcmc_apply_kernel<false><<<L.nb, MC_RUN, 0, s>>>(a);
        GS_LAUNCHED("mcmc_relocate");
    }
    return GSRAST_OK;
}
}
size_t gsrast_mcmc_scratch_bytes(int P, int n) { (void)n; return mcmc_layout(P > 0 ? (size_t)P : 0).total; }

int gsrast_mcmc_plan(int P, const float* opacity_logit, const unsigned char* dead_src, float min_opacity, unsigned* weights_out,
                     char* scratch, unsigned* counts, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "mcmc_plan: negative P");
    if (!(min_opacity >= 0.0f && min_opacity < 1.0f)) return fail(GSRAST_E_ARG, "mcmc_plan: min_opacity must be in [0, 1)");
    if (!scratch || !counts) return fail(GSRAST_E_ARG, "mcmc_plan: NULL scratch / counts");
    if (P > 0 && (!opacity_logit || !weights_out)) return fail(GSRAST_E_ARG, "mcmc_plan: NULL opacity_logit / weights_out");
    const McmcLayout L = mcmc_layout((size_t)P);
    ProfScope ps(K_MCMC_PLAN, s);
    if (L.nb) {
        mcmc_weights_kernel<<<L.nb, MC_RUN, 0, s>>>(P, opacity_logit, dead_src, min_opacity, weights_out, at<uint32_t>(scratch, L.run_prefix),
                                                   at<unsigned char>(scratch, L.dead), at<unsigned long long>(scratch, L.wg_weight), at<uint32_t>(scratch, L.wg_dead));
        GS_LAUNCHED("mcmc_weights");
    }
    mcmc_scan_kernel<<<1, MC_RUN, 0, s>>>(at<unsigned long long>(scratch, L.wg_weight), at<uint32_t>(scratch, L.wg_dead), L.nb, (uint32_t)P,
                                          at<uint32_t>(scratch, L.hdr), counts);
    GS_LAUNCHED("mcmc_scan");
    return GSRAST_OK;
}

int gsrast_mcmc_sample(int P, int n, const long long* draws, char* scratch, int* src_out, unsigned* count_out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || n < 0) return fail(GSRAST_E_ARG, "mcmc_sample: negative P / n");
    if (!scratch) return fail(GSRAST_E_ARG, "mcmc_sample: NULL scratch");
    if (n > 0 && (!draws || !src_out)) return fail(GSRAST_E_ARG, "mcmc_sample: NULL draws / src_out");
    if (P == 0 && n == 0) return GSRAST_OK;
    const McmcLayout L = mcmc_layout((size_t)P);
    uint32_t* count = at<uint32_t>(scratch, L.count);
    ProfScope ps(K_MCMC_SAMPLE, s);
    if (P > 0) GS_HIP(hipMemsetAsync(count, 0, (size_t)P * 4, s));
    if (n > 0) {
        mcmc_sample_kernel<<<(unsigned)(((size_t)n + MC_RUN - 1) / MC_RUN), MC_RUN, 0, s>>>(P, n, draws, at<uint32_t>(scratch, L.hdr), at<unsigned long long>(scratch, L.wg_weight),
                                                                                          L.nb, at<uint32_t>(scratch, L.run_prefix), src_out, count);
        GS_LAUNCHED("mcmc_sample");
    }
    if (count_out && P > 0) GS_HIP(hipMemcpyAsync(count_out, count, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
    return GSRAST_OK;
}

int gsrast_mcmc_relocate(int P, int n, const int* src, char* scratch, const unsigned* counts_host, float min_opacity, int n_groups,
                         const gsrast_densify_group* groups, void* stream)
{
    return mcmc_apply("mcmc_relocate", false, P, n, src, scratch, counts_host, min_opacity, n_groups, groups, (hipStream_t)stream);
}

int gsrast_mcmc_grow(int P, int n, const int* src, char* scratch, const unsigned* counts_host, float min_opacity, int n_groups,
                     const gsrast_densify_group* groups, void* stream)
{
    return mcmc_apply("mcmc_grow", true, P, n, src, scratch, counts_host, min_opacity, n_groups, groups, (hipStream_t)stream);
}

int gsrast_mcmc_noise(int P, float* xyz, const float* rotation, const float* scaling, const float* opacity_logit, const float* noise,
                      const float* row_scale, float scale, float k, float x0, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "mcmc_noise: negative P");
    if (P == 0) return GSRAST_OK;
    if (!xyz || !rotation || !scaling || !opacity_logit || !noise) return fail(GSRAST_E_ARG, "mcmc_noise: NULL pointer");
    if (((uintptr_t)rotation & 15) != 0) return fail(GSRAST_E_ARG, "mcmc_noise: rotation must be 16-byte aligned");
    ProfScope ps(K_MCMC_NOISE, s);
    mcmc_noise_kernel<<<(unsigned)(((size_t)P + MC_RUN - 1) / MC_RUN), MC_RUN, 0, s>>>(P, xyz, reinterpret_cast<const float4*>(rotation), scaling, opacity_logit, noise, row_scale, scale, k, x0);
    GS_LAUNCHED("mcmc_noise");
    return GSRAST_OK;
}

// ---- temporal lifespan (gsrast_temporal.h) --------------------------------------------------------------------------
// Not in the profile kernel-name table: tools/temporal_overhead.py times these calls with device events of its own.
namespace {
// the refusals the three entry points share; 0 or GSRAST_E_ARG
int temporal_check(const char* who, int P, int sigmoid_center, float min_scale)
{
    if (P < 0) return refuse(who, "negative P");
    if (sigmoid_center != 0 && sigmoid_center != 1) return refuse(who, "sigmoid_center must be 0 or 1");
    if (!(min_scale > 0.0f && min_scale <= 1.0f)) return refuse(who, "min_scale must be in (0, 1]");
    return GSRAST_OK;
}
unsigned temporal_grid(int P) { return (unsigned)(((size_t)P + TP_RUN - 1) / TP_RUN); }
}  // namespace

int gsrast_temporal_gate_forward(int P, int multires, int sigmoid_center, float t, float min_scale, float dead_threshold, const float* head,
                                 const float* center, float* lifespan, float* state, float* time_emb, unsigned char* dead, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = temporal_check("temporal_gate_forward", P, sigmoid_center, min_scale)) return rc;
    if (multires < 0 || multires > TP_MAX_MULTIRES) return fail(GSRAST_E_ARG, "temporal_gate_forward: multires must be in [0, 8]");
    if (!std::isfinite(t)) return fail(GSRAST_E_ARG, "temporal_gate_forward: t must be finite");
    if (P == 0) return GSRAST_OK;
    if (!head || !center || !lifespan || !state) return fail(GSRAST_E_ARG, "temporal_gate_forward: NULL required pointer");
    if (((uintptr_t)time_emb & 15) != 0) return fail(GSRAST_E_ARG, "temporal_gate_forward: time_emb must be 16-byte aligned");
    const size_t lds = time_emb ? (size_t)TP_RUN * (2 * multires + 1) * 4 : 0;
    temporal_gate_fwd_kernel<<<temporal_grid(P), TP_RUN, lds, s>>>(P, multires, sigmoid_center, t, min_scale, dead_threshold, head, center, lifespan, state, time_emb, dead);
    GS_LAUNCHED("temporal_gate_fwd");
    return GSRAST_OK;
}

int gsrast_temporal_gate_backward(int P, int sigmoid_center, float t, float min_scale, const float* head, const float* center, const float* d_lifespan,
                                  const float* d_state, float* d_head, float* d_center, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = temporal_check("temporal_gate_backward", P, sigmoid_center, min_scale)) return rc;
    if (!std::isfinite(t)) return fail(GSRAST_E_ARG, "temporal_gate_backward: t must be finite");
    if (P == 0) return GSRAST_OK;
    if (!head || !center) return fail(GSRAST_E_ARG, "temporal_gate_backward: NULL required pointer");
    if (!d_head && !d_center) return GSRAST_OK;
    temporal_gate_bwd_kernel<<<temporal_grid(P), TP_RUN, 0, s>>>(P, sigmoid_center, t, min_scale, head, center, d_lifespan, d_state, d_head, d_center);
    GS_LAUNCHED("temporal_gate_bwd");
    return GSRAST_OK;
}

int gsrast_temporal_integral(int P, int sigmoid_center, float start, float end, float min_scale, float min_integral, const float* head, const float* center,
                             float* integral, unsigned char* dead, float* inv, int* stats, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = temporal_check("temporal_integral", P, sigmoid_center, min_scale)) return rc;
    if (!std::isfinite(start) || !std::isfinite(end)) return fail(GSRAST_E_ARG, "temporal_integral: start and end must be finite");
    if (end < start) return fail(GSRAST_E_ARG, "temporal_integral: end < start");
    if (!(min_integral >= 0.0f) || !std::isfinite(min_integral)) return fail(GSRAST_E_ARG, "temporal_integral: min_integral must be finite and >= 0 (the maximum is taken on the bits of positive floats)");
    if (P == 0) return GSRAST_OK;
    if (!head || !center || !integral || !dead || !stats) return fail(GSRAST_E_ARG, "temporal_integral: NULL required pointer");
    GS_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int), s));
    temporal_integral_kernel<<<std::min(temporal_grid(P), (unsigned)TP_INTEGRAL_WGS), TP_RUN, 0, s>>>(P, sigmoid_center, start, end, min_scale, min_integral, head, center, integral, dead, stats);
    GS_LAUNCHED("temporal_integral");
    if (inv) {      // (a launch of its own: the maximum must exist before the division)
        temporal_inv_kernel<<<temporal_grid(P), TP_RUN, 0, s>>>(P, integral, dead, stats, inv);
        GS_LAUNCHED("temporal_inv");
    }
    return GSRAST_OK;
}

// ---- bilateral-grid colour correction (gsrast_bilagrid.h) -----------------------------------------------------------
// Not in the profile kernel-name table: tools/bilagrid_overhead.py times these calls with device events of its own.
// scratch: `splits` slabs of 12 L GH GW floats when a vertex column has more than one slab, nothing otherwise
namespace {
int bilagrid_check(const char* who, const gsrast_bilagrid* d)
{
    if (!d) return refuse(who, "NULL descriptor");
    if (d->GW < 1 || d->GW > BG_MAX_G || d->GH < 1 || d->GH > BG_MAX_G) return refuse(who, "GW and GH must be in [1, 64]");
    if (d->L < 1 || d->L > BG_MAX_L) return refuse(who, "L must be in [1, 16]");
    if (d->W < 1 || d->H < 1) return refuse(who, "W and H must be >= 1");
    if (d->full_W < 1 || d->full_H < 1 || d->full_W > BG_MAX_FRAME || d->full_H > BG_MAX_FRAME) return refuse(who, "full_W and full_H must be in [1, 32768]");
    if (d->x0 < 0 || d->y0 < 0 || (long long)d->x0 + d->W > d->full_W || (long long)d->y0 + d->H > d->full_H) return refuse(who, "the window must lie inside the frame");
    if (d->splits < 0 || d->splits > BG_MAX_SPLITS) return refuse(who, "splits must be in [0, 1024] (0: the library's choice)");
    return GSRAST_OK;
}
// slabs per vertex column: as asked, or enough for about 2048 workgroups while a slab keeps at least four pixel rows (one per wave).
// A function of the descriptor alone, never of the device.
int bilagrid_splits(const gsrast_bilagrid* d)
{
    if (d->splits > 0) return d->splits;
    const int want = (2048 + d->GW * d->GH - 1) / (d->GW * d->GH);
    const int rows = d->GH == 1 ? d->H : std::min(d->H, 2 * ((d->full_H + d->GH - 2) / (d->GH - 1)) + 4);      // of a vertex's rectangle, at most
    return std::max(1, std::min(want, rows / 4));
}
BgArgs bilagrid_args(const gsrast_bilagrid* d) { return BgArgs{ d->GW, d->GH, d->L, d->W, d->H, d->x0, d->y0, d->full_W, d->full_H }; }
size_t bilagrid_floats(const gsrast_bilagrid* d) { return (size_t)12 * d->L * d->GH * d->GW; }
#define BILAGRID_PIXEL_GRID(d) dim3((unsigned)(((d)->W + 63) / 64), (unsigned)(((d)->H + 3) / 4))      /* a wave per 64 pixels of a row, four rows per workgroup */
}  // namespace

size_t gsrast_bilagrid_scratch_bytes(const gsrast_bilagrid* d)
{
    if (bilagrid_check("bilagrid_scratch_bytes", d) != GSRAST_OK) return 0;
    const int splits = bilagrid_splits(d);
    return (splits > 1 ? align256((size_t)splits * bilagrid_floats(d) * 4) : 0) + 256;
}

int gsrast_bilagrid_forward(const gsrast_bilagrid* d, const float* grid, const float* image, float* out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = bilagrid_check("bilagrid_forward", d)) return rc;
    if (!grid || !image || !out) return fail(GSRAST_E_ARG, "bilagrid_forward: NULL required pointer");
    bilagrid_fwd_kernel<<<BILAGRID_PIXEL_GRID(d), BG_THREADS, bg_pixel_lds(d->L), s>>>(bilagrid_args(d), grid, image, out);
    GS_LAUNCHED("bilagrid_fwd");
    return GSRAST_OK;
}

int gsrast_bilagrid_backward(const gsrast_bilagrid* d, const float* grid, const float* image, const float* dL_dout, float* dL_dimage,
                             float* dL_dgrid, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = bilagrid_check("bilagrid_backward", d)) return rc;
    if (!grid || !image || !dL_dout) return fail(GSRAST_E_ARG, "bilagrid_backward: NULL required pointer");
    if (!dL_dimage && !dL_dgrid) return fail(GSRAST_E_ARG, "bilagrid_backward: dL_dimage and dL_dgrid are both NULL");
    const int splits = bilagrid_splits(d);
    if (dL_dgrid && splits > 1 && !scratch) return fail(GSRAST_E_ARG, "bilagrid_backward: NULL scratch");
    const BgArgs a = bilagrid_args(d);
    if (dL_dimage) {
        bilagrid_bwd_pixel_kernel<<<BILAGRID_PIXEL_GRID(d), BG_THREADS, bg_pixel_lds(d->L), s>>>(a, grid, image, dL_dout, dL_dimage);
        GS_LAUNCHED("bilagrid_bwd_pixel");
    }
    if (dL_dgrid) {
        float* const dst = splits > 1 ? reinterpret_cast<float*>(scratch) : dL_dgrid;
        const dim3 g((unsigned)(d->GW * d->GH), (unsigned)splits);
        pick_int<1, 2, 4, 8, 16>(d->L <= 1 ? 1 : d->L <= 2 ? 2 : d->L <= 4 ? 4 : d->L <= 8 ? 8 : 16, [&](auto lt) {
            bilagrid_bwd_grid_kernel<decltype(lt)::value><<<g, BG_THREADS, 0, s>>>(a, splits, image, dL_dout, dst);
        });
        GS_LAUNCHED("bilagrid_bwd_grid");
        if (splits > 1) {
            const unsigned n = (unsigned)bilagrid_floats(d);
            bilagrid_reduce_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, splits, dst, dL_dgrid);
            GS_LAUNCHED("bilagrid_reduce");
        }
    }
    return GSRAST_OK;
}

int gsrast_bilagrid_tv(int N, int GW, int GH, int L, const float* grids, float* loss_out, const float* upstream, float* dL_dgrids, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (N < 1 || N > BG_TV_MAX_N) return fail(GSRAST_E_ARG, "bilagrid_tv: N must be in [1, 2048]");
    if (GW < 1 || GW > BG_MAX_G || GH < 1 || GH > BG_MAX_G) return fail(GSRAST_E_ARG, "bilagrid_tv: GW and GH must be in [1, 64]");
    if (L < 1 || L > BG_MAX_L) return fail(GSRAST_E_ARG, "bilagrid_tv: L must be in [1, 16]");
    if (!grids) return fail(GSRAST_E_ARG, "bilagrid_tv: NULL required pointer");
    if (!loss_out && !dL_dgrids) return fail(GSRAST_E_ARG, "bilagrid_tv: loss_out and dL_dgrids are both NULL");
    const unsigned n = (unsigned)N * 12u * (unsigned)(L * GH * GW);      // (< 2^31: N <= 2048, 12 L GH GW <= 786432)
    const double rows = (double)N * 12.0;
    const auto inv = [](double pairs) { return pairs > 0.0 ? 1.0 / pairs : 0.0; };
    const BgTvCounts cnt{ inv(rows * L * GH * (GW - 1)), inv(rows * L * (GH - 1) * GW), inv(rows * (L - 1) * GH * GW) };
    if (loss_out) {
        const int rows_step = BG_TV_THREADS / GW;
        const BgTvStep step{ BG_TV_THREADS % GW, rows_step % GH, (rows_step / GH) % L };
        bilagrid_tv_kernel<<<1, BG_TV_THREADS, 0, s>>>(n, GW, GH, L, step, cnt, grids, loss_out);
        GS_LAUNCHED("bilagrid_tv");
    }
    if (dL_dgrids) {
        bilagrid_tv_grad_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, GW, GH, L, cnt, grids, upstream, dL_dgrids);
        GS_LAUNCHED("bilagrid_tv_grad");
    }
    return GSRAST_OK;
}

// ---- fused 3-layer MLP (gsrast_mlp.h) -------------------------------------------------------------------------------
namespace {
int mlp3_default_workgroups()     // one workgroup per CU (its LDS images leave room for one)
{
    static const int n = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return cus;
    }();
    return n;
}
// the checks every entry point shares; 0 or the refusal's code
int mlp3_check(const char* who, const gsrast_mlp3* d, int workgroups)
{
    if (!d) return refuse(who, "NULL descriptor");
    if (d->n < 0) return refuse(who, "negative N");
    if (workgroups < 0 || workgroups > 65535) return refuse(who, "workgroups must be in [0, 65535]");
    if (d->d_x < 1 || d->d_tail < 0) return refuse(who, "D_x must be >= 1 and D_tail >= 0");
    if ((long long)d->d_x + d->d_tail > MLP_MAX_IO) return refuse(who, "D_in = D_x + D_tail must be in [1, 64]");
    for (int h : { d->h1, d->h2 }) if (h != 32 && h != 64 && h != 96 && h != 128) return refuse(who, "H1 and H2 must be one of 32, 64, 96, 128");
    if (d->d_out < 1 || d->d_out > MLP_MAX_IO) return refuse(who, "D_out must be in [1, 64]");
    if (d->sigmoid != 0 && d->sigmoid != 1) return refuse(who, "sigmoid must be 0 or 1");
    if (!d->w1 || !d->b1 || !d->w2 || !d->b2 || !d->w3 || !d->b3) return refuse(who, "NULL weight / bias pointer");
    if (d->n > 0 && (!d->x || (d->d_tail > 0 && !d->x_tail))) return refuse(who, "NULL x / x_tail");
    return GSRAST_OK;
}
Mlp3Args mlp3_args(const gsrast_mlp3* d)
{
    Mlp3Args a{};
    a.n = d->n; a.d_x = d->d_x; a.d_tail = d->d_tail; a.d_in = d->d_x + d->d_tail; a.h1 = d->h1; a.h2 = d->h2; a.d_out = d->d_out; a.sigmoid = d->sigmoid;
    a.x = d->x; a.x_tail = d->x_tail; a.w1 = d->w1; a.b1 = d->b1; a.w2 = d->w2; a.b2 = d->b2; a.w3 = d->w3; a.b3 = d->b3;
    a.y = d->y; a.dy = d->dy; a.dx = d->dx;
    return a;
}
int mlp3_grid(const gsrast_mlp3* d, int workgroups, int per_cu)      // never more workgroups than tiles; default: per_cu workgroups per CU
{
    const long long tiles = ((long long)d->n + MLP_TR - 1) / MLP_TR;
    return (int)std::min<long long>(workgroups ? workgroups : per_cu * mlp3_default_workgroups(), tiles);
}
}  // namespace

size_t gsrast_mlp3_scratch_bytes(const gsrast_mlp3* d, int workgroups)
{
    gsrast_mlp3 probe{};
    if (d) { probe = *d; probe.n = 0; }
    static const float one = 0.0f;
    probe.w1 = probe.b1 = probe.w2 = probe.b2 = probe.w3 = probe.b3 = &one;      // (only the dims are looked at)
    if (mlp3_check("mlp3_scratch_bytes", d ? &probe : nullptr, workgroups) != GSRAST_OK) return 0;
    const size_t g = workgroups ? (size_t)workgroups : (size_t)mlp3_default_workgroups();
    return align256(g * mlp3_param_floats(d->d_x + d->d_tail, d->h1, d->h2, d->d_out) * 4) + 256;
}

int gsrast_mlp3_forward(const gsrast_mlp3* d, int workgroups, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mlp3_check("mlp3_forward", d, workgroups)) return rc;
    if (d->n > 0 && !d->y) return fail(GSRAST_E_ARG, "mlp3_forward: NULL y");
    if (d->n == 0) return GSRAST_OK;
    const Mlp3Args a = mlp3_args(d);
    const size_t lds = (size_t)(((a.d_in + 7) & ~7) + a.h1 + a.h2) * MLP_LD * 4;
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(mlp3_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MLP_FWD_LDS);
    if (attr != hipSuccess) return fail(GSRAST_E_DEVICE, "mlp3_forward: hipFuncSetAttribute", attr);
    ProfScope ps(K_MLP_FWD, s);
    mlp3_fwd_kernel<<<mlp3_grid(d, workgroups, 2), MLP_THREADS, lds, s>>>(a);      // (its LDS images leave room for two per CU up to D_in = 48)
    GS_LAUNCHED("mlp3_fwd");
    return GSRAST_OK;
}

int gsrast_mlp3_backward(const gsrast_mlp3* d, int workgroups, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mlp3_check("mlp3_backward", d, workgroups)) return rc;
    if (d->n > 0 && !d->dy) return fail(GSRAST_E_ARG, "mlp3_backward: NULL dy");
    if (d->n > 0 && d->sigmoid && !d->y) return fail(GSRAST_E_ARG, "mlp3_backward: the sigmoid head needs y");
    Mlp3Args a = mlp3_args(d);
    a.need = (d->dx ? MLP_NEED_DX : 0) | (d->dw1 || d->db1 ? MLP_NEED_L1 : 0) | (d->dw2 || d->db2 ? MLP_NEED_L2 : 0) | (d->dw3 || d->db3 ? MLP_NEED_L3 : 0);
    if (a.need == 0) return GSRAST_OK;
    const bool params = (a.need & ~MLP_NEED_DX) != 0;
    if (params && !scratch) return fail(GSRAST_E_ARG, "mlp3_backward: NULL scratch");
    a.partial = reinterpret_cast<float*>(scratch);
    const int grid = mlp3_grid(d, workgroups, 1);
    ProfScope ps(K_MLP_BWD, s);
    if (grid > 0) {
        const size_t lds = (size_t)(2 * MLP_MAX_IO + a.h1 + std::max(a.h1, a.h2) + a.h2) * MLP_LD * 4;
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(mlp3_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MLP_BWD_LDS);
        if (attr != hipSuccess) return fail(GSRAST_E_DEVICE, "mlp3_backward: hipFuncSetAttribute", attr);
        const long long tiles = ((long long)d->n + MLP_TR - 1) / MLP_TR, per_launch = (long long)grid * MLP_FLUSH_TILES;
        for (a.tile0 = 0; a.tile0 < tiles; a.tile0 += per_launch) {      // (gsrast_mlp.h: no accumulator chain longer than 512 rows)
            a.tile_end = std::min(tiles, a.tile0 + per_launch);
            a.add = a.tile0 > 0;
            mlp3_bwd_kernel<<<(unsigned)std::min<long long>(grid, a.tile_end - a.tile0), MLP_THREADS, lds, s>>>(a);
            GS_LAUNCHED("mlp3_bwd");
        }
    }
    if (params) {      // (N = 0: no partial, every wanted gradient is written as 0)
        Mlp3Reduce r{};
        r.partial = a.partial; r.n_partials = grid; r.total = (unsigned)mlp3_param_floats(a.d_in, a.h1, a.h2, a.d_out);
        const unsigned sizes[6] = { (unsigned)(a.h1 * a.d_in), (unsigned)a.h1, (unsigned)(a.h2 * a.h1), (unsigned)a.h2, (unsigned)(a.d_out * a.h2), (unsigned)a.d_out };
        float* const outs[6] = { d->dw1, d->db1, d->dw2, d->db2, d->dw3, d->db3 };
        unsigned end = 0;
        for (int k = 0; k < 6; k++) { end += sizes[k]; r.seg_end[k] = end; r.out[k] = outs[k]; }
        mlp3_reduce_kernel<<<(r.total + 255) / 256, 256, 0, s>>>(r);
        GS_LAUNCHED("mlp3_reduce");
    }
    return GSRAST_OK;
}

// ---- the same head with the precision chosen per call (gsrast_mlp_bf16.h); GSRAST_MLP_FP32 IS the calls above ----
namespace {
int mlp3_precision_check(const char* who, int precision)
{
    if (precision != GSRAST_MLP_FP32 && precision != GSRAST_MLP_BF16) return refuse(who, "precision must be GSRAST_MLP_FP32 (0) or GSRAST_MLP_BF16 (1)");
    return GSRAST_OK;
}
// the kernels with the hidden widths of the reference's heads (128 / 128, 128 / 64) compiled in, or the general one
typedef void (*mlp3_bf16_kernel_t)(const Mlp3Args);
mlp3_bf16_kernel_t mlp3_bf16_pick(const gsrast_mlp3* d, mlp3_bf16_kernel_t both128, mlp3_bf16_kernel_t second64, mlp3_bf16_kernel_t general)
{
    return d->h1 == 128 && d->h2 == 128 ? both128 : d->h1 == 128 && d->h2 == 64 ? second64 : general;
}
int mlp3_bf16_grid(const gsrast_mlp3* d, int workgroups, int per_cu)
{
    const long long tiles = ((long long)d->n + MLPB_ROWS - 1) / MLPB_ROWS;
    return (int)std::min<long long>(workgroups ? workgroups : per_cu * mlp3_default_workgroups(), tiles);
}
}  // namespace

size_t gsrast_mlp3_scratch_bytes_p(const gsrast_mlp3* d, int precision, int workgroups)
{
    if (mlp3_precision_check("mlp3_scratch_bytes", precision) != GSRAST_OK) return 0;
    return gsrast_mlp3_scratch_bytes(d, workgroups);      // (bf16: the same slabs, one per workgroup, the same default count)
}

int gsrast_mlp3_forward_p(const gsrast_mlp3* d, int precision, int workgroups, void* stream)
{
    if (int rc = mlp3_precision_check("mlp3_forward", precision)) return rc;
    if (precision == GSRAST_MLP_FP32) return gsrast_mlp3_forward(d, workgroups, stream);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mlp3_check("mlp3_forward", d, workgroups)) return rc;
    if (d->n > 0 && !d->y) return fail(GSRAST_E_ARG, "mlp3_forward: NULL y");
    if (d->n == 0) return GSRAST_OK;
    const Mlp3Args a = mlp3_args(d);
    const auto kernel = mlp3_bf16_pick(d, &mlp3_bf16_fwd_kernel<4, 4>, &mlp3_bf16_fwd_kernel<4, 2>, &mlp3_bf16_fwd_kernel<0, 0>);
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MLPB_FWD_LDS);
    if (attr != hipSuccess) return fail(GSRAST_E_DEVICE, "mlp3_forward: hipFuncSetAttribute", attr);
    ProfScope ps(K_MLP_FWD, s);
    kernel<<<mlp3_bf16_grid(d, workgroups, 2), MLP_THREADS, MLPB_FWD_LDS, s>>>(a);
    GS_LAUNCHED("mlp3_bf16_fwd");
    return GSRAST_OK;
}

int gsrast_mlp3_backward_p(const gsrast_mlp3* d, int precision, int workgroups, char* scratch, void* stream)
{
    if (int rc = mlp3_precision_check("mlp3_backward", precision)) return rc;
    if (precision == GSRAST_MLP_FP32) return gsrast_mlp3_backward(d, workgroups, scratch, stream);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = mlp3_check("mlp3_backward", d, workgroups)) return rc;
    if (d->n > 0 && !d->dy) return fail(GSRAST_E_ARG, "mlp3_backward: NULL dy");
    if (d->n > 0 && d->sigmoid && !d->y) return fail(GSRAST_E_ARG, "mlp3_backward: the sigmoid head needs y");
    Mlp3Args a = mlp3_args(d);
    a.need = (d->dx ? MLP_NEED_DX : 0) | (d->dw1 || d->db1 ? MLP_NEED_L1 : 0) | (d->dw2 || d->db2 ? MLP_NEED_L2 : 0) | (d->dw3 || d->db3 ? MLP_NEED_L3 : 0);
    if (a.need == 0) return GSRAST_OK;
    const bool params = (a.need & ~MLP_NEED_DX) != 0;
    if (params && !scratch) return fail(GSRAST_E_ARG, "mlp3_backward: NULL scratch");
    a.partial = reinterpret_cast<float*>(scratch);
    const int grid = mlp3_bf16_grid(d, workgroups, 1);
    ProfScope ps(K_MLP_BWD, s);
    if (grid > 0) {
        const auto kernel = mlp3_bf16_pick(d, &mlp3_bf16_bwd_kernel<4, 4>, &mlp3_bf16_bwd_kernel<4, 2>, &mlp3_bf16_bwd_kernel<0, 0>);
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MLPB_BWD_LDS);
        if (attr != hipSuccess) return fail(GSRAST_E_DEVICE, "mlp3_backward: hipFuncSetAttribute", attr);
        const long long tiles = ((long long)d->n + MLPB_ROWS - 1) / MLPB_ROWS, per_launch = (long long)grid * MLPB_FLUSH_TILES;
        for (a.tile0 = 0; a.tile0 < tiles; a.tile0 += per_launch) {      // (gsrast_mlp_bf16.h: no accumulator chain longer than 512 rows)
            a.tile_end = std::min(tiles, a.tile0 + per_launch);
            a.add = a.tile0 > 0;
            kernel<<<(unsigned)std::min<long long>(grid, a.tile_end - a.tile0), MLP_THREADS, MLPB_BWD_LDS, s>>>(a);
            GS_LAUNCHED("mlp3_bf16_bwd");
        }
    }
    if (params) {      // (N = 0: no partial, every wanted gradient is written as 0)
        Mlp3Reduce r{};
        r.partial = a.partial; r.n_partials = grid; r.total = (unsigned)mlp3_param_floats(a.d_in, a.h1, a.h2, a.d_out);
        const unsigned sizes[6] = { (unsigned)(a.h1 * a.d_in), (unsigned)a.h1, (unsigned)(a.h2 * a.h1), (unsigned)a.h2, (unsigned)(a.d_out * a.h2), (unsigned)a.d_out };
        float* const outs[6] = { d->dw1, d->db1, d->dw2, d->db2, d->dw3, d->db3 };
        unsigned end = 0;
        for (int k = 0; k < 6; k++) { end += sizes[k]; r.seg_end[k] = end; r.out[k] = outs[k]; }
        mlp3_reduce_kernel<<<(r.total + 255) / 256, 256, 0, s>>>(r);
        GS_LAUNCHED("mlp3_reduce");
    }
    return GSRAST_OK;
}

// scratch: bbox (8 words) | codes A/B | index A/B | radix histogram | scan scratch | boxes
namespace {
struct KnnLayout { size_t bbox, cA, cB, iA, iB, hist, scan, boxes, total; };
KnnLayout knn_layout(size_t P)
{
    KnnLayout L; Carver c;
    const size_t Pp = P ? P : 1;
    L.bbox = c.take(32); L.cA = c.take(Pp * 4); L.cB = c.take(Pp * 4); L.iA = c.take(Pp * 4); L.iB = c.take(Pp * 4);
    const size_t hist_n = 256 * rs_blocks_n(Pp, GSRAST_DEPTH_ITEMS);
    L.hist = c.take(hist_n * 4); L.scan = c.take(scan_tmp_elems(hist_n) * 4);
    L.boxes = c.take(((Pp + KNN_BOX - 1) / KNN_BOX) * 6 * 4);
    L.total = c.o + 256;
    return L;
}
}
size_t gsrast_knn_scratch_bytes(int P) { return knn_layout(P > 0 ? (size_t)P : 0).total; }

int gsrast_knn3_mean_dist2(int P, const float* points, float* mean_dist2, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "knn3: bad size");
    if (P == 0) return GSRAST_OK;
    if (!points || !mean_dist2 || !scratch) return fail(GSRAST_E_ARG, "knn3: NULL pointer");
    const KnnLayout L = knn_layout((size_t)P);
    unsigned* bbox = at<unsigned>(scratch, L.bbox);
    uint32_t *cA = at<uint32_t>(scratch, L.cA), *cB = at<uint32_t>(scratch, L.cB);
    uint32_t *iA = at<uint32_t>(scratch, L.iA), *iB = at<uint32_t>(scratch, L.iB);
    const int nb = (P + 255) / 256;
    knn_init_kernel<<<1, 64, 0, s>>>(bbox);
    GS_LAUNCHED("knn_init");
    knn_bbox_kernel<<<nb, 256, 0, s>>>(P, points, bbox);
    GS_LAUNCHED("knn_bbox");
    knn_morton_kernel<<<nb, 256, 0, s>>>(P, points, bbox, cA, iA);
    GS_LAUNCHED("knn_morton");
    int rc = sort_pairs_small(cA, iA, cB, iB, (uint32_t)P, 30, at<uint32_t>(scratch, L.hist), at<uint32_t>(scratch, L.scan), s);
    if (rc != GSRAST_OK) return rc;
    const uint32_t* order = (radix_passes(30) & 1) ? iB : iA;
    const int nboxes = (P + KNN_BOX - 1) / KNN_BOX;
    float* boxes = at<float>(scratch, L.boxes);
    knn_boxes_kernel<<<nboxes, 256, 0, s>>>(P, points, order, boxes);
    GS_LAUNCHED("knn_boxes");
    knn_search_kernel<<<nb, 256, 0, s>>>(P, points, order, boxes, nboxes, mean_dist2);
    GS_LAUNCHED("knn_search");
    return GSRAST_OK;
}

// ---- exact k-NN query with indices (gsrast_knn_query.h) ----------------------------------------------------------
// scratch: the reference's part as knn_layout's (bbox | codes A/B | index A/B), the sort's histogram and scan scratch sized for the larger
// of the two sets | boxes | the Morton-ordered records | the queries' codes A/B and index A/B
namespace {
struct KnnQueryLayout { size_t bbox, cA, cB, iA, iB, hist, scan, boxes, rec, qcA, qcB, qiA, qiB, total; };
KnnQueryLayout knn_query_layout(size_t n_ref, size_t n_query)
{
    KnnQueryLayout L; Carver c;
    const size_t R = n_ref ? n_ref : 1, Q = n_query ? n_query : 1, S = R > Q ? R : Q;
    L.bbox = c.take(32); L.cA = c.take(R * 4); L.cB = c.take(R * 4); L.iA = c.take(R * 4); L.iB = c.take(R * 4);
    const size_t hist_n = 256 * rs_blocks_n(S, GSRAST_DEPTH_ITEMS);
    L.hist = c.take(hist_n * 4); L.scan = c.take(scan_tmp_elems(hist_n) * 4);
    L.boxes = c.take(((R + KNN_BOX - 1) / KNN_BOX) * 6 * 4);
    L.rec = c.take(R * 16);
    L.qcA = c.take(Q * 4); L.qcB = c.take(Q * 4); L.qiA = c.take(Q * 4); L.qiB = c.take(Q * 4);
    L.total = c.o + 256;
    return L;
}
}
size_t gsrast_knn_query_scratch_bytes(int n_ref, int n_query) { return knn_query_layout(n_ref > 0 ? (size_t)n_ref : 0, n_query > 0 ? (size_t)n_query : 0).total; }

int gsrast_knn_query(int n_ref, const float* ref, int n_query, const float* query, int k, int32_t* idx, float* dist2, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n_ref < 0 || n_query < 0) return fail(GSRAST_E_ARG, "knn_query: bad size");
    if (k < 1 || k > KNNQ_MAX_K) return fail(GSRAST_E_ARG, "knn_query: k must be in 1..32");
    if (n_query == 0) return GSRAST_OK;
    if (!idx) return fail(GSRAST_E_ARG, "knn_query: NULL idx");
    if (n_ref == 0) {
        const size_t slots = (size_t)k * (size_t)n_query;
        knnq_fill_kernel<<<(unsigned)std::min<size_t>((slots + 255) / 256, 4096), 256, 0, s>>>(slots, idx, dist2);
        GS_LAUNCHED("knnq_fill");
        return GSRAST_OK;
    }
    if (!ref || !scratch) return fail(GSRAST_E_ARG, "knn_query: NULL pointer");
    if (!query && n_query != n_ref) return fail(GSRAST_E_ARG, "knn_query: a NULL query is the reference querying itself: n_query must be n_ref");
    const KnnQueryLayout L = knn_query_layout((size_t)n_ref, (size_t)n_query);
    unsigned* bbox = at<unsigned>(scratch, L.bbox);
    uint32_t *cA = at<uint32_t>(scratch, L.cA), *cB = at<uint32_t>(scratch, L.cB);
    uint32_t *iA = at<uint32_t>(scratch, L.iA), *iB = at<uint32_t>(scratch, L.iB);
    uint32_t *hist = at<uint32_t>(scratch, L.hist), *scan = at<uint32_t>(scratch, L.scan);
    const bool inB = radix_passes(30) & 1;
    const int nb = (n_ref + 255) / 256;
    // the reference: Morton order, boxes of KNN_BOX consecutive points (the kernels of gsrast_knn.h, as they are), the permuted copy
    knn_init_kernel<<<1, 64, 0, s>>>(bbox);
    GS_LAUNCHED("knn_init");
    knn_bbox_kernel<<<nb, 256, 0, s>>>(n_ref, ref, bbox);
    GS_LAUNCHED("knn_bbox");
    knn_morton_kernel<<<nb, 256, 0, s>>>(n_ref, ref, bbox, cA, iA);
    GS_LAUNCHED("knn_morton");
    int rc = sort_pairs_small(cA, iA, cB, iB, (uint32_t)n_ref, 30, hist, scan, s);
    if (rc != GSRAST_OK) return rc;
    const uint32_t *order = inB ? iB : iA, *codes = inB ? cB : cA;
    const int nboxes = (n_ref + KNN_BOX - 1) / KNN_BOX;
    float* boxes = at<float>(scratch, L.boxes);
    knn_boxes_kernel<<<nboxes, 256, 0, s>>>(n_ref, ref, order, boxes);
    GS_LAUNCHED("knn_boxes");
    float4* rec = at<float4>(scratch, L.rec);
    knnq_records_kernel<<<nb, 256, 0, s>>>(n_ref, ref, order, rec);
    GS_LAUNCHED("knnq_records");
    // the queries: Morton order on the reference's grid (codes clamped to it); the reference's own order when it queries itself
    const uint32_t *qorder = nullptr, *qcodes = nullptr;
    const int nqb = (n_query + 255) / 256;
    if (query) {
        uint32_t *qcA = at<uint32_t>(scratch, L.qcA), *qcB = at<uint32_t>(scratch, L.qcB);
        uint32_t *qiA = at<uint32_t>(scratch, L.qiA), *qiB = at<uint32_t>(scratch, L.qiB);
        knn_morton_kernel<<<nqb, 256, 0, s>>>(n_query, query, bbox, qcA, qiA);
        GS_LAUNCHED("knn_morton");
        rc = sort_pairs_small(qcA, qiA, qcB, qiB, (uint32_t)n_query, 30, hist, scan, s);
        if (rc != GSRAST_OK) return rc;
        qorder = inB ? qiB : qiA; qcodes = inB ? qcB : qcA;
    }
    // the smallest capacity that holds k.  (A plain chain, as launch_pixel_topk's switch: the table of compiled variants, tests/variant_table.py,
    // counts the selection sites of the render kernels, and every instantiation here is run against the fp64 brute force by tests/test_gpu_knn_query.py.)
#define KNNQ_LAUNCH(CAP) knnq_search_kernel<CAP><<<nqb, 256, 0, s>>>(n_ref, rec, codes, boxes, nboxes, n_query, query, qorder, qcodes, k, idx, dist2)
    if (k <= 2) KNNQ_LAUNCH(2); else if (k <= 4) KNNQ_LAUNCH(4); else if (k <= 8) KNNQ_LAUNCH(8); else if (k <= 16) KNNQ_LAUNCH(16); else KNNQ_LAUNCH(32);
#undef KNNQ_LAUNCH
    GS_LAUNCHED("knnq_search");
    return GSRAST_OK;
}

// ---- mip-mapped feature-plane lookup (gsrast_hexplane.h) ---------------------------------------------------------
// scratch: value stacks (levels >= 1) of every plane | gradient stacks of every plane, each 256-byte aligned
namespace {
struct HexLayout { size_t mips[HEX_MAX_PLANES], gmips[HEX_MAX_PLANES], gmips_begin, gmips_end, kA, kB, vA, vB, pairs, hist, scan, total; int levels[HEX_MAX_PLANES]; int cell_bits, key_bits; };
// number of levels above 0 the published op builds: halve while an extent is > 1 and the limit allows; -1 = odd extent
int hex_levels(int W, int H, int limit)
{
    int w = W, h = H, l = 0;
    while ((w > 1 || h > 1) && l < limit) {
        if ((w > 1 && (w & 1)) || (h > 1 && (h & 1))) return -1;
        w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; l++;
    }
    return l;
}
// F < 0: the caller does not know the row width (gsrast_hexplane_scratch_bytes); everything that needs none is still checked
const char* hex_check(int n_planes, const gsrast_plane* planes, int C, int D, int F)
{
    if (n_planes < 1 || n_planes > HEX_MAX_PLANES || !planes) return "hexplane: 1..24 planes";
    if (C < 4 || C > 64 || (C & (C - 1))) return "hexplane: channels must be a power of two in [4, 64]";
    if (D < 2 || D > 8 || (F >= 0 && (F < C || (F & 3)))) return "hexplane: 2..8 coordinates per point, feature rows a multiple of 4 floats";
    for (int p = 0; p < n_planes; p++) {
        const gsrast_plane& g = planes[p];
        if (g.W < 1 || g.H < 1 || (long long)g.W * g.H > (1ll << 26)) return "hexplane: bad plane extent";
        if (g.cu < 0 || g.cu >= D || g.cv < 0 || g.cv >= D) return "hexplane: coordinate column outside the point row";
        if (g.max_mip_level < 0) return "hexplane: negative max_mip_level";
        if (g.out_offset < 0 || (g.out_offset & 3) || (F >= 0 && g.out_offset > F - C)) return "hexplane: feature block outside the row";
        if (hex_levels(g.W, g.H, g.max_mip_level) < 0) return "hexplane: a mip level has an odd extent > 1 (limit max_mip_level)";
        if (hex_levels(g.W, g.H, g.max_mip_level) >= HEX_MAX_LEVELS) return "hexplane: too many mip levels";
        // the forward sums a block in registers over ADJACENT planes and stores it once: an equal offset further back, or a block
        // that covers part of another, would be overwritten, and the backward would differentiate a sum that was never formed
        for (int q = 0; q < p; q++) {
            const int o = planes[q].out_offset;
            if (o == g.out_offset ? planes[p - 1].out_offset != g.out_offset : (o < g.out_offset + C && g.out_offset < o + C))
                return "hexplane: planes sharing a feature block must be adjacent, and blocks must be equal or disjoint";
        }
    }
    return nullptr;
}
HexLayout hex_layout(int n_planes, const gsrast_plane* planes, int C, size_t N)
{
    HexLayout L{}; Carver c;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) L.gmips_begin = c.o;
        for (int p = 0; p < n_planes; p++) {
            const int nl = hex_levels(planes[p].W, planes[p].H, planes[p].max_mip_level);
            L.levels[p] = nl;
            const size_t texels = hex_level_offset(planes[p].W, planes[p].H, nl + 1);
            (pass ? L.gmips[p] : L.mips[p]) = c.take(texels * (size_t)C * 4);
        }
    }
    L.gmips_end = c.o;
    // sorted-run backward: (key, point) pairs of every plane, double-buffered, + the radix sort's tables
    size_t widest = 1;
    for (int p = 0; p < n_planes; p++)
        widest = std::max(widest, (size_t)planes[p].W * planes[p].H + hex_level_offset(planes[p].W, planes[p].H, L.levels[p] + 1));
    L.cell_bits = 1; while (((size_t)1 << L.cell_bits) < widest) L.cell_bits++;
    int pb = 0; while ((1 << pb) < n_planes) pb++;
    L.key_bits = L.cell_bits + pb;
    const size_t E = std::max<size_t>((size_t)n_planes * N, 1);
    L.kA = c.take(E * 4); L.kB = c.take(E * 4); L.vA = c.take(E * 4); L.vB = c.take(E * 4); L.pairs = c.take(E * sizeof(HexPair));
    const size_t hist_n = 256 * rs_blocks_n(E, RS_ITEMS);
    L.hist = c.take(hist_n * 4); L.scan = c.take(scan_tmp_elems(hist_n) * 4);
    L.total = c.o + 256;
    return L;
}
void hex_fill(HexArgs& a, const HexLayout& L, int N, int D, int C, int F, int n_planes, const gsrast_plane* planes, char* scratch, bool backward)
{
    a.n_planes = n_planes; a.C = C; a.N = N; a.D = D; a.F = F;
    for (int p = 0; p < n_planes; p++) {
        HexPlane& P = a.pl[p];
        P.tex = planes[p].tex; P.grad = planes[p].grad_tex;
        P.mips = at<float>(scratch, L.mips[p]); P.gmips = at<float>(scratch, L.gmips[p]);
        P.W = planes[p].W; P.H = planes[p].H; P.cu = planes[p].cu; P.cv = planes[p].cv;
        P.n_levels = L.levels[p]; P.out_offset = planes[p].out_offset;
    }
}
int hex_build_mips(const HexArgs& a, hipStream_t s)
{
    int top = 0; unsigned long long widest[HEX_MAX_LEVELS + 1] = {0};
    for (int p = 0; p < a.n_planes; p++) {
        top = std::max(top, a.pl[p].n_levels);
        for (int l = 1; l <= a.pl[p].n_levels; l++)
            widest[l] = std::max(widest[l], (unsigned long long)hex_extent(a.pl[p].W, l) * hex_extent(a.pl[p].H, l) * (a.C >> 2));
    }
    for (int l = 1; l <= top; l++) {
        hex_mip_build_kernel<<<dim3((unsigned)((widest[l] + 255) / 256), (unsigned)a.n_planes), 256, 0, s>>>(a, l);
        GS_LAUNCHED("hex_mip_build");
    }
    return GSRAST_OK;
}
}  // namespace

size_t gsrast_hexplane_scratch_bytes(int n_planes, const gsrast_plane* planes, int C, int N)
{
    // no row width is passed: whether a block fits its row is for forward / backward to say.  0 = refused, gsrast_last_error() has the text
    if (N < 0) { fail(GSRAST_E_ARG, "hexplane_scratch_bytes: bad size"); return 0; }
    if (const char* e = hex_check(n_planes, planes, C, 8, -1)) { fail(GSRAST_E_ARG, e); return 0; }
    return hex_layout(n_planes, planes, C, (size_t)N).total;
}

int gsrast_hexplane_forward(int N, int D, int C, int F, int n_planes, const gsrast_plane* planes, const float* pts, const float* levels,
                            float* features, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (N < 0) return fail(GSRAST_E_ARG, "hexplane_forward: bad size");
    if (const char* e = hex_check(n_planes, planes, C, D, F)) return fail(GSRAST_E_ARG, e);
    for (int p = 0; p < n_planes; p++) if (!planes[p].tex) return fail(GSRAST_E_ARG, "hexplane_forward: NULL plane");
    if (!scratch || (N > 0 && (!pts || !levels || !features))) return fail(GSRAST_E_ARG, "hexplane_forward: NULL pointer");
    const HexLayout L = hex_layout(n_planes, planes, C, (size_t)N);
    HexArgs a{};
    hex_fill(a, L, N, D, C, F, n_planes, planes, scratch, false);
    if (int rc = hex_build_mips(a, s)) return rc;
    if (N == 0) return GSRAST_OK;
    const unsigned long long lanes = (unsigned long long)N * (C >> 2);
    hex_sample_fwd_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(a, pts, levels, features);
    GS_LAUNCHED("hex_sample_fwd");
    return GSRAST_OK;
}

int gsrast_hexplane_backward(int N, int D, int C, int F, int n_planes, const gsrast_plane* planes, const float* pts, const float* levels,
                             const float* d_features, float* d_pts, float* d_levels, int mips_built, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (N < 0) return fail(GSRAST_E_ARG, "hexplane_backward: bad size");
    if (const char* e = hex_check(n_planes, planes, C, D, F)) return fail(GSRAST_E_ARG, e);
    for (int p = 0; p < n_planes; p++) if (!planes[p].tex || !planes[p].grad_tex) return fail(GSRAST_E_ARG, "hexplane_backward: NULL plane or gradient");
    if (!scratch || (N > 0 && (!pts || !levels || !d_features))) return fail(GSRAST_E_ARG, "hexplane_backward: NULL pointer");
    const HexLayout L = hex_layout(n_planes, planes, C, (size_t)N);
    HexArgs a{};
    hex_fill(a, L, N, D, C, F, n_planes, planes, scratch, true);
    for (int p = 0; p < n_planes; p++) GS_HIP(hipMemsetAsync(planes[p].grad_tex, 0, (size_t)planes[p].W * planes[p].H * C * 4, s));
    if (N == 0) return GSRAST_OK;
    int top = 0;
    for (int p = 0; p < n_planes; p++) top = std::max(top, a.pl[p].n_levels);
    if (top) GS_HIP(hipMemsetAsync(scratch + L.gmips_begin, 0, L.gmips_end - L.gmips_begin, s));
    const unsigned long long E = (unsigned long long)n_planes * N;
    if (g_opt.hexplane_scatter.load() == 0 && L.key_bits <= 32 && E < 0xFFFFFFFFull && (unsigned long long)N * F < 0xFFFFFFFFull) {
        uint32_t *kA = at<uint32_t>(scratch, L.kA), *kB = at<uint32_t>(scratch, L.kB), *vA = at<uint32_t>(scratch, L.vA), *vB = at<uint32_t>(scratch, L.vB);
        hex_keys_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)n_planes), 256, 0, s>>>(a, L.cell_bits, pts, levels, kA, vA, at<HexPair>(scratch, L.pairs));
        GS_LAUNCHED("hex_keys");
        if (int rc = sort_pairs_large(kA, vA, kB, vB, (uint32_t)E, L.key_bits, at<uint32_t>(scratch, L.hist), at<uint32_t>(scratch, L.scan), s)) return rc;
        const bool inB = radix_passes(L.key_bits) & 1;
        const uint32_t *ks = inB ? kB : kA, *vs = inB ? vB : vA;
        const unsigned long long groups = (E + HEX_RUN_CHUNK - 1) / HEX_RUN_CHUNK;
        pick_int<4, 8, 16, 32, 64>(C, [&](auto channels) {
            constexpr int CH = decltype(channels)::value;
            hex_grad_tex_sorted_kernel<CH><<<(unsigned)((groups * CH + 255) / 256), 256, 0, s>>>(a, L.cell_bits, (unsigned)E, ks, vs, at<HexPair>(scratch, L.pairs), pts, levels, d_features, g_opt.ablate.load());
        });
        GS_LAUNCHED("hex_grad_tex_sorted");
    } else {
        const unsigned long long lanes = (unsigned long long)N * C;
        hex_grad_tex_global_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(a, pts, levels, d_features);
        GS_LAUNCHED("hex_grad_tex_global");
    }
    for (int l = top; l >= 1; l--) {
        unsigned long long widest = 0;
        for (int p = 0; p < n_planes; p++) if (a.pl[p].n_levels >= l)
            widest = std::max(widest, (unsigned long long)hex_extent(a.pl[p].W, l) * hex_extent(a.pl[p].H, l) * (C >> 2));
        hex_mip_pull_kernel<<<dim3((unsigned)((widest + 255) / 256), (unsigned)n_planes), 256, 0, s>>>(a, l);
        GS_LAUNCHED("hex_mip_pull");
    }
    if (d_pts || d_levels) {
        if (!mips_built) if (int rc = hex_build_mips(a, s)) return rc;
        const unsigned long long lanes = (unsigned long long)N * (C >> 2);
        hex_grad_uv_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(a, pts, levels, d_features, d_pts, d_levels);
        GS_LAUNCHED("hex_grad_uv");
    }
    return GSRAST_OK;
}

// ---- normal consistency (gsrast_normal.h) -----------------------------------------------------------------------------
// Not in the profile kernel-name table: tools/normal_overhead.py times these calls with device events of its own.
// scratch of the loss: one fp64 partial per workgroup of the forward
namespace {
// the refusals the image calls share; 0 or GSRAST_E_ARG
int normal_image_check(const char* who, int W, int H, double tanfovx, double tanfovy)
{
    if (W < 1 || H < 1) return refuse(who, "W and H must be >= 1");
    if (W > NM_MAX_SIDE || H > NM_MAX_SIDE) return refuse(who, "W and H must be at most 32768");
    if (!std::isfinite(tanfovx) || !std::isfinite(tanfovy) || !(tanfovx > 0.0) || !(tanfovy > 0.0)) return refuse(who, "tanfovx and tanfovy must be finite and > 0");
    return GSRAST_OK;
}
#define NORMAL_GRID(W, H) dim3((unsigned)(((W) + NM_TW - 1) / NM_TW), (unsigned)(((H) + NM_TH - 1) / NM_TH))      /* a workgroup per NM_TW x NM_TH pixel tile */
}  // namespace

int gsrast_gaussian_normals_forward(int P, const float* means3D, const float* scales, const float* rotations, const float* viewmatrix,
                                    float* normals, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "gaussian_normals_forward: negative P");
    if (P == 0) return GSRAST_OK;
    if (!means3D || !scales || !rotations || !viewmatrix || !normals) return fail(GSRAST_E_ARG, "gaussian_normals_forward: NULL required pointer");
    gaussian_normals_fwd_kernel<<<(unsigned)(((size_t)P + 255) / 256), 256, 0, s>>>(P, means3D, scales, rotations, viewmatrix, normals);
    GS_LAUNCHED("gaussian_normals_fwd");
    return GSRAST_OK;
}

int gsrast_gaussian_normals_backward(int P, const float* means3D, const float* scales, const float* rotations, const float* viewmatrix,
                                     const float* dL_dnormals, float* dL_drotations, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return fail(GSRAST_E_ARG, "gaussian_normals_backward: negative P");
    if (!dL_drotations) return fail(GSRAST_E_ARG, "gaussian_normals_backward: dL_drotations is NULL (it is the only gradient)");
    if (P == 0) return GSRAST_OK;
    if (!means3D || !scales || !rotations || !viewmatrix || !dL_dnormals) return fail(GSRAST_E_ARG, "gaussian_normals_backward: NULL required pointer");
    gaussian_normals_bwd_kernel<<<(unsigned)(((size_t)P + 255) / 256), 256, 0, s>>>(P, means3D, scales, rotations, viewmatrix, dL_dnormals, dL_drotations);
    GS_LAUNCHED("gaussian_normals_bwd");
    return GSRAST_OK;
}

int gsrast_depth_normal_forward(int W, int H, double tanfovx, double tanfovy, const float* depth, float* normals, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = normal_image_check("depth_normal_forward", W, H, tanfovx, tanfovy)) return rc;
    if (!depth || !normals) return fail(GSRAST_E_ARG, "depth_normal_forward: NULL required pointer");
    depth_normal_fwd_kernel<<<NORMAL_GRID(W, H), NM_THREADS, 0, s>>>(nm_image(W, H, tanfovx, tanfovy), depth, normals);
    GS_LAUNCHED("depth_normal_fwd");
    return GSRAST_OK;
}

int gsrast_depth_normal_backward(int W, int H, double tanfovx, double tanfovy, const float* depth, const float* dL_dnormals, float* dL_ddepth,
                                 void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = normal_image_check("depth_normal_backward", W, H, tanfovx, tanfovy)) return rc;
    if (!depth || !dL_dnormals) return fail(GSRAST_E_ARG, "depth_normal_backward: NULL required pointer");
    if (!dL_ddepth) return fail(GSRAST_E_ARG, "depth_normal_backward: dL_ddepth is NULL (it is the only gradient)");
    depth_normal_bwd_kernel<<<NORMAL_GRID(W, H), NM_THREADS, 0, s>>>(nm_image(W, H, tanfovx, tanfovy), depth, dL_dnormals, dL_ddepth);
    GS_LAUNCHED("depth_normal_bwd");
    return GSRAST_OK;
}

size_t gsrast_normal_loss_scratch_bytes(int W, int H)
{
    if (normal_image_check("normal_loss_scratch_bytes", W, H, 1.0, 1.0) != GSRAST_OK) return 0;
    const dim3 g = NORMAL_GRID(W, H);
    return align256((size_t)g.x * g.y * sizeof(double)) + 256;
}

int gsrast_normal_loss_forward(int W, int H, double tanfovx, double tanfovy, const float* normal_map, const float* depth, const float* weight,
                               float* loss, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = normal_image_check("normal_loss_forward", W, H, tanfovx, tanfovy)) return rc;
    if (!normal_map || !depth || !loss) return fail(GSRAST_E_ARG, "normal_loss_forward: NULL required pointer");
    if (!scratch) return fail(GSRAST_E_ARG, "normal_loss_forward: NULL scratch");
    const dim3 g = NORMAL_GRID(W, H);
    double* const partial = reinterpret_cast<double*>(scratch);
    normal_loss_fwd_kernel<<<g, NM_THREADS, 0, s>>>(nm_image(W, H, tanfovx, tanfovy), normal_map, depth, weight, partial);
    GS_LAUNCHED("normal_loss_fwd");
    normal_loss_reduce_kernel<<<1, 256, 0, s>>>(partial, (int)(g.x * g.y), 1.0 / ((double)H * (double)W), loss);
    GS_LAUNCHED("normal_loss_reduce");
    return GSRAST_OK;
}

int gsrast_normal_loss_backward(int W, int H, double tanfovx, double tanfovy, const float* normal_map, const float* depth, const float* weight,
                                const float* upstream, float* dL_dnormal_map, float* dL_ddepth, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (int rc = normal_image_check("normal_loss_backward", W, H, tanfovx, tanfovy)) return rc;
    if (!normal_map || !depth || !upstream) return fail(GSRAST_E_ARG, "normal_loss_backward: NULL required pointer");
    if (!dL_dnormal_map && !dL_ddepth) return fail(GSRAST_E_ARG, "normal_loss_backward: dL_dnormal_map and dL_ddepth are both NULL");
    normal_loss_bwd_kernel<<<NORMAL_GRID(W, H), NM_THREADS, 0, s>>>(nm_image(W, H, tanfovx, tanfovy), normal_map, depth, weight, upstream, dL_dnormal_map, dL_ddepth);
    GS_LAUNCHED("normal_loss_bwd");
    return GSRAST_OK;
}

// ---- Mip-Splatting's 3-D smoothing filter (gsrast_filter3d.h) ---------------------------------------------------------
// Not in the profile kernel-name table: tools/filter3d_overhead.py times these calls with device events of its own.
// scratch of the sweep: two ints (the bits of the largest distance, the number of seen rows), cleared on the stream by every call
namespace {
unsigned filter3d_grid(int P) { return (unsigned)(((size_t)P + F3_RUN - 1) / F3_RUN); }
}  // namespace

size_t gsrast_filter3d_scratch_bytes(int P, int C)
{
    if (P < 0) { refuse("filter3d_scratch_bytes", "negative P"); return 0; }
    if (C < 1) { refuse("filter3d_scratch_bytes", "C must be >= 1"); return 0; }
    return 256;
}

int gsrast_filter3d_compute(int P, int C, const float* means3D, const float* table, double near, double margin, double variance, double focal_max,
                            float* filter_3D, unsigned char* valid, void* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const char* who = "filter3d_compute";
    if (P < 0) return refuse(who, "negative P");
    if (C < 1) return refuse(who, "C must be >= 1");
    if (!std::isfinite(near) || !(near > 0.0)) return refuse(who, "near must be finite and > 0");
    if (!std::isfinite(margin) || !(margin >= 0.0)) return refuse(who, "margin must be finite and >= 0");
    if (!std::isfinite(variance) || !(variance > 0.0)) return refuse(who, "variance must be finite and > 0");
    if (!std::isfinite(focal_max) || !(focal_max > 0.0)) return refuse(who, "focal_max must be finite and > 0");
    if (P == 0) return GSRAST_OK;
    if (!means3D || !table || !filter_3D) return refuse(who, "NULL required pointer");
    if (!scratch) return refuse(who, "NULL scratch");
    const float k = (float)(std::sqrt((double)(float)variance) / focal_max);      // near, margin, variance rounded to fp32 once; k in fp64, rounded once
    int* const stats = reinterpret_cast<int*>(scratch);
    GS_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int), s));
    filter3d_sweep_kernel<<<std::min(filter3d_grid(P), (unsigned)F3_SWEEP_WGS), F3_RUN, 0, s>>>(P, C, (float)near, (float)margin, means3D, table, filter_3D, stats);
    GS_LAUNCHED("filter3d_sweep");
    filter3d_finish_kernel<<<filter3d_grid(P), F3_RUN, 0, s>>>(P, k, stats, filter_3D, valid);      // (a launch of its own: the maximum must exist first)
    GS_LAUNCHED("filter3d_finish");
    return GSRAST_OK;
}

int gsrast_filter3d_apply_forward(int P, const float* scales, const float* opacities, const float* filter_3D, float* scales_f, float* opacities_f,
                                  void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return refuse("filter3d_apply_forward", "negative P");
    if (P == 0) return GSRAST_OK;
    if (!scales || !opacities || !filter_3D || !scales_f || !opacities_f) return refuse("filter3d_apply_forward", "NULL required pointer");
    filter3d_apply_fwd_kernel<<<filter3d_grid(P), F3_RUN, 0, s>>>(P, scales, opacities, filter_3D, scales_f, opacities_f);
    GS_LAUNCHED("filter3d_apply_fwd");
    return GSRAST_OK;
}

int gsrast_filter3d_apply_backward(int P, const float* scales, const float* opacities, const float* filter_3D, const float* d_scales_f,
                                   const float* d_opacities_f, float* d_scales, float* d_opacities, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0) return refuse("filter3d_apply_backward", "negative P");
    if (!d_scales && !d_opacities) return refuse("filter3d_apply_backward", "d_scales and d_opacities are both NULL");
    if (P == 0) return GSRAST_OK;
    if (!scales || !opacities || !filter_3D) return refuse("filter3d_apply_backward", "NULL required pointer");
    filter3d_apply_bwd_kernel<<<filter3d_grid(P), F3_RUN, 0, s>>>(P, scales, opacities, filter_3D, d_scales_f, d_opacities_f, d_scales, d_opacities);
    GS_LAUNCHED("filter3d_apply_bwd");
    return GSRAST_OK;
}

// ---- fused L1 + D-SSIM loss (gsrast_loss.h) ---------------------------------------------------
namespace {
LossWin make_window()
{   // utils/loss_utils.py:25-27: exp() in double, stored as fp32, divided (fp32) by the fp32 sum.  That sum is the correctly
    // rounded one in the reference (torch's CPU reduction; a sequential fp32 sum lands 1 ulp lower): summed in double here,
    // then rounded -- checked bit for bit against the reference's own window (tests/golden/loss_vectors.npz: ref_window_1d)
    LossWin w; double dsum = 0.0;
    for (int i = 0; i < LW; i++) { w.w[i] = (float)exp(-(double)((i - LW / 2) * (i - LW / 2)) / (2.0 * 1.5 * 1.5)); dsum += (double)w.w[i]; }
    const float sum = (float)dsum;
    for (int i = 0; i < LW; i++) w.w[i] = w.w[i] / sum;
    return w;
}
struct LossLayout { size_t d_mu, d_e11, d_e12, partial, total; int nblk; };
LossLayout loss_layout(int C, int H, int W)
{
    LossLayout L; Carver c;
    const size_t n = (size_t)C * H * W;
    L.nblk = C * ((W + LT - 1) / LT) * ((H + LT - 1) / LT);
    L.d_mu = c.take(n * 4); L.d_e11 = c.take(n * 4); L.d_e12 = c.take(n * 4); L.partial = c.take((size_t)L.nblk * 8);
    L.total = c.o + 256;
    return L;
}
} // namespace

size_t gsrast_loss_scratch_bytes(int C, int H, int W) { return (C > 0 && H > 0 && W > 0) ? loss_layout(C, H, W).total : 256; }

int gsrast_loss_forward(int C, int H, int W, const float* img, const float* gt, float lambda_dssim, float* out3,
                        char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !out3 || !scratch) return fail(GSRAST_E_ARG, "loss_forward: bad argument");
    const LossLayout L = loss_layout(C, H, W);
    ProfScope ps(K_LOSS_FWD, s);
    loss_fwd_kernel<<<L.nblk, 256, 0, s>>>(C, H, W, img, gt, make_window(), at<float>(scratch, L.d_mu), at<float>(scratch, L.d_e11),
                                           at<float>(scratch, L.d_e12), at<float2>(scratch, L.partial));
    GS_LAUNCHED("loss_fwd");
    loss_reduce_kernel<<<1, 256, 0, s>>>(at<float2>(scratch, L.partial), L.nblk, 1.0f / ((float)C * (float)H * (float)W), lambda_dssim, out3);
    GS_LAUNCHED("loss_reduce");
    return GSRAST_OK;
}

int gsrast_loss_backward(int C, int H, int W, const float* img, const float* gt, float lambda_dssim, const float* dL_dloss,
                         const char* scratch, float* dL_dimg, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (C <= 0 || H <= 0 || W <= 0 || !img || !gt || !dL_dimg || !scratch) return fail(GSRAST_E_ARG, "loss_backward: bad argument");
    const LossLayout L = loss_layout(C, H, W);
    ProfScope ps(K_LOSS_BWD, s);
    loss_bwd_kernel<<<L.nblk, 256, 0, s>>>(C, H, W, img, gt, make_window(), at<float>(scratch, L.d_mu), at<float>(scratch, L.d_e11),
                                           at<float>(scratch, L.d_e12), lambda_dssim, 1.0f / ((float)C * (float)H * (float)W), dL_dloss, dL_dimg);
    GS_LAUNCHED("loss_bwd");
    return GSRAST_OK;
}

} // extern "C"
