// gsrast_capi.hip -- the renderer's host orchestration + its half of the C ABI declared in include/gsrast.h: everything that reads the
// renderer's state buffers (forward, backward, the post-render passes, mark-visible, debug export), the gradient exchange (its kernels
// build on gsrast_preprocess.h), and the one definition of what gsrast_host.h declares (errors, option table, profile timers, the sort
// drivers).  The training kernels' calls -- activations, Adam, densify, MCMC, temporal, MLP, k-NN, hexplane, loss -- are gsrast_train.hip.
// Built with the flags of build.py (FLAGS), one object per unit, linked into one library.
//
// Host side: forward_impl / backward_impl run the stages of one ForwardRun / BackwardRun; what a call does is decided once, at its top, by
// plan_forward / plan_backward (gsrast_policy.h).  The process-wide words of gsrast_set_option live in one table (kOptions).  What a context
// owns on a device -- streams, gate, tables, hints -- is one record (DeviceState), which a call resolves once, at its top (current_device).
// Launch plan of the default path (every launch on the caller's stream except the colour kernel):
//   forward : preprocess_fwd (geometry; claims the pose's launch-order hint slot) -> depth_bucket_scatter -> depth_bucket_sort
//             -> [fork: preprocess_color on the context's side stream] -> emit_column_runs (workgroup 0: totals -> pinned host memory,
//             the host spins on them while the rest is enqueued speculatively) -> run sort by column (hist, rowscan, scatter)
//             -> run_hist_rows -> rowscan -> run_scatter_rows -> tile_ranges_from_runs -> [join] -> blend_fwd_cull (also zero-fills
//             the gradient records, writes the pose's hints and the backward's launch order)
//   backward: blend_bwd_cull_t -> preprocess_bwd (reference K6 + K7 fused; RAW: + the activations' chain rule)
// Fallbacks: radix depth sort (+ scan) after a bucket overflow or with options.depth_sort = 1; instance-level binning with
// options.binning = 1; repeated binning + blend with exact sizes when the speculative capacities did not fit.
#include "gsrast_host.h"
#include "gsrast_common.h"
#include "gsrast_policy.h"
#include "gsrast_preprocess.h"
#include "gsrast_binning.h"
#include "gsrast_blend.h"
#include "gsrast_contrib.h"
#include "gsrast_features.h"
#include "gsrast_distort.h"
#include "gsrast_topk.h"
#include "gsrast_project.h"
#include "gsrast_exchange.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <thread>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <dlfcn.h>
#ifndef GSRAST_LATE_FILL_WGS
#define GSRAST_LATE_FILL_WGS 256      // workgroups of late_rows_zero_kernel beside the blend backward: as few as finish under it -- 3 M views/s with 64 / 128 / 256 / 512 / 1024 / 4096: 676 (too slow: the per-Gaussian backward waits) / 803-806 / 790-813 / 806-808 / 801-804 / 797; 2 M: 883 / 935 / 953
#endif
#include <mutex>
#include <string>
#include <vector>
#include <unordered_map>

using namespace gsrast;

namespace {

thread_local std::string g_err;
// ---- every process-wide word gsrast_set_option addresses: ONE table -- name, word, default, how a value is taken ------------------------
// Per-call behaviour lives in a gsrast_options value: the *_ex entry points take one, the reference-shaped entry points snapshot the
// process defaults (the rows with a `field`) once at entry, so a call never sees a half-changed set and two host threads driving
// different streams / devices with different options cannot disturb each other.  The other rows are process-wide diagnostics and A/B
// switches, not per-call behaviour: a render call loads each of them ONCE, at its top (snapshot_switches).
// The words themselves (OptionWords g_opt) are declared in gsrast_host.h -- the training unit reads two of them -- and defined below.
enum OptionKind { OPT_FLAG /* non-zero means 1 */, OPT_ONE_OF /* bit v of `a` set: v is accepted; else GSRAST_E_ARG */, OPT_CLAMP /* to [a, b] */, OPT_WORD /* stored as given */ };
struct OptionRow { const char* name; std::atomic<int>* word; int def; OptionKind kind; int a, b; int gsrast_options::* field /* the per-call option this word is the process default of */; };
constexpr int OPT_01 = 0b11, OPT_012 = 0b111, OPT_PPL = 0b10111 /* 0 auto, 1 / 2 / 4 */, OPT_MAX = 0x7FFFFFFF;
constexpr OptionRow kOptions[] = {
    { "exp_mode", &g_opt.exp_mode, 0, OPT_ONE_OF, OPT_012, 0, &gsrast_options::exp_mode },
    { "binning", &g_opt.binning, 0, OPT_ONE_OF, OPT_01, 0, &gsrast_options::binning },
    { "tile_clip", &g_opt.tile_clip, 1, OPT_FLAG, 0, 0, &gsrast_options::tile_clip },
    { "cull", &g_opt.cull, 1, OPT_FLAG, 0, 0, &gsrast_options::cull },
    { "lpt", &g_opt.lpt, 1, OPT_FLAG, 0, 0, &gsrast_options::lpt },      // heaviest-tile-first launch order
    { "speculative", &g_opt.speculative, 1, OPT_FLAG, 0, 0, &gsrast_options::speculative },
    { "fwd_pixels_per_lane", &g_opt.fwd_pixels_per_lane, 0, OPT_ONE_OF, OPT_PPL, 0, &gsrast_options::fwd_pixels_per_lane },
    { "bwd_pixels_per_lane", &g_opt.bwd_pixels_per_lane, 0, OPT_ONE_OF, OPT_PPL, 0, &gsrast_options::bwd_pixels_per_lane },
    { "sh_grad_factors", &g_opt.sh_grad_factors, 0, OPT_FLAG, 0, 0, &gsrast_options::sh_grad_factors },
    { "side_stream", &g_opt.side_stream, 1, OPT_FLAG, 0, 0, &gsrast_options::side_stream },
    { "depth_sort", &g_opt.depth_sort, 0, OPT_ONE_OF, OPT_01, 0, &gsrast_options::depth_sort },
    { "forward_only", &g_opt.forward_only, 0, OPT_FLAG, 0, 0, &gsrast_options::forward_only },
    { "no_order_hint", &g_opt.no_order_hint, 0, OPT_FLAG, 0, 0, &gsrast_options::no_order_hint },
    { "dense_backward", &g_opt.dense_backward, 0, OPT_FLAG, 0, 0, &gsrast_options::dense_backward },
    { "no_list_cut", &g_opt.no_list_cut, 0, OPT_FLAG, 0, 0, &gsrast_options::no_list_cut },
    { "profile", &g_opt.profile, 0, OPT_WORD, 0, 0, nullptr },                    // bit k = time kernel id k; -1 = all
    { "debug_sync", &g_opt.debug_sync, 0, OPT_FLAG, 0, 0, nullptr },
    { "debug_state", &g_opt.debug_state, 0, OPT_FLAG, 0, 0, nullptr },            // forwards also store what only gsrast_debug_export reads (cov3D)
    { "ablate", &g_opt.ablate, 0, OPT_WORD, 0, 0, nullptr },                      // experiments only
    { "mutate", &g_opt.mutate, 0, OPT_WORD, 0, 0, nullptr },                      // tests only: a deliberately WRONG backward (mutate_drop_front_batch_kernel) -- proves that a parity bar bites
    { "list_cut_always", &g_opt.list_cut_always, 0, OPT_FLAG, 0, 0, nullptr },    // the list cut also where it does not pay (tests)
    { "chain_gate", &g_opt.chain_gate, 1, OPT_FLAG, 0, 0, nullptr },              // 1: the completion pass of the list cut runs on its own stream behind a gate (ChainGate); 0: inline, eleven predicated launches on the caller's stream
    { "touch_bits", &g_opt.touch_bits, 1, OPT_FLAG, 0, 0, nullptr },              // 1: the forward blend keeps GeomLayout::untouched for the backward; 0: only the list cut's late bits serve it (A/B switch)
    { "sparse_grec", &g_opt.sparse_grec, 1, OPT_FLAG, 0, 0, nullptr },            // 1: a forward that keeps those bits zeroes only the consumed Gaussians' gradient records (A/B switch)
    { "late_fill_min_p", &g_opt.late_fill_min_p, 750000, OPT_CLAMP, 0, OPT_MAX, nullptr },      // scenes of at least this many Gaussians write their zero rows beside the blend backward
    { "tau_sample", &g_opt.tau_sample, 1, OPT_CLAMP, 0, 6, nullptr },             // the predicted cut's opacity mass comes from one wave in 2^this of preprocess_fwd
    { "tau_cut", &g_opt.tau_cut, 1, OPT_FLAG, 0, 0, nullptr },                    // 1: a pose without (trustworthy) remembered cut depths gets PREDICTED ones from this call's own opacity mass (gsrast_common.h); 0: only poses with remembered cut depths are cut
    { "two_level", &g_opt.two_level, 1, OPT_FLAG, 0, 0, nullptr },                // 1: the bucket scatter as two launches, coarse + refine (gsrast_binning.h; A/B switch)
    { "two_level_min_p", &g_opt.two_level_min_p, 2500000, OPT_CLAMP, 0, OPT_MAX, nullptr },     // measured (kernel times, one box): 0.3 M 16.1 us in one launch against 15.8 + 5.7 in two, 1 M 41.0 against 36.6 + 9.1, 3 M 88.2 against 60.5 + 19.9: the second launch only pays where the scattered stores dominate
    { "sort_hint", &g_opt.sort_hint, 1, OPT_FLAG, 0, 0, nullptr },                // 1: enqueue three depth-sort passes when the context's last forward had short keys (A/B switch)
    { "bwd_transposed", &g_opt.bwd_transposed, 1, OPT_FLAG, 0, 0, nullptr },      // 1: blend_bwd_cull_t_kernel for one pixel per lane (default); 0: blend_bwd_cull_kernel<.., 1> (A/B switch)
    { "hexplane_scatter", &g_opt.hexplane_scatter, 0, OPT_ONE_OF, OPT_01, 0, nullptr },         // hexplane backward to the texels: 0 = sorted runs, 1 = direct global atomics
};
const OptionRow* option_row(const char* name)
{
    for (const OptionRow& r : kOptions) if (!strcmp(name, r.name)) return &r;
    return nullptr;
}
// what a row stores for `value`; false: the value is refused
bool option_take(const OptionRow& r, int value, int* stored)
{
    *stored = r.kind == OPT_FLAG ? (value ? 1 : 0) : r.kind == OPT_CLAMP ? std::min(std::max(value, r.a), r.b) : value;
    return r.kind != OPT_ONE_OF || (value >= 0 && value < 31 && ((r.a >> value) & 1) != 0);
}
PlanSwitches snapshot_switches()      // one load of every switch a render call's plan depends on
{
    const OptionWords& g = g_opt;
    return PlanSwitches{ g.list_cut_always.load() != 0, g.tau_cut.load() != 0, g.touch_bits.load() != 0, g.sparse_grec.load() != 0, g.two_level.load() != 0, g.chain_gate.load() != 0,
                         g.sort_hint.load() != 0, g.debug_state.load() != 0, g.two_level_min_p.load(), g.tau_sample.load(), g.bwd_transposed.load() != 0, g.late_fill_min_p.load(),
                         g.ablate.load(), g.mutate.load() };
}

// ---- per-kernel device timing (option "profile") -------------------------------------------
// (the ids: KernelId, gsrast_host.h)
const char* const kKernelNames[K_COUNT] = { "preprocess_fwd", "sort_depth", "scan_tiles", "emit_instances",
                                            "sort_tile", "tile_ranges", "blend_fwd", "blend_bwd",
                                            "preprocess_bwd", "mark_visible", "loss_fwd", "loss_bwd", "preprocess_color", "sh_dir_derivs",
                                            "cut_redo" /* list cut: the predicated second binning + blend behind the forward blend, as ONE stage */,
                                            "late_rows_zero" /* list cut: the late Gaussians' zero rows, on the side stream beside the blend backward */,
                                            "grec_zero_touched" /* the consumed Gaussians' gradient records zeroed behind the forward's last blend */,
                                            "densify_classify", "densify_scan", "densify_apply", "densify_stats_update" /* csrc/gsrast_densify.h */,
                                            "contrib_blend", "contrib_finish" /* csrc/gsrast_contrib.h: gsrast_contrib_stats */,
                                            "features_fwd", "features_bwd" /* csrc/gsrast_features.h: gsrast_features_forward / _backward (one entry per call: all its passes) */,
                                            "distort_fwd", "distort_bwd" /* csrc/gsrast_distort.h: gsrast_distortion_forward / _backward */,
                                            "adam_step_visible" /* csrc/gsrast_adam.h: gsrast_adam_step_visible */,
                                            "mcmc_plan" /* csrc/gsrast_mcmc.h: gsrast_mcmc_plan (weights + scan) */, "mcmc_sample" /* gsrast_mcmc_sample */,
                                            "mcmc_apply" /* gsrast_mcmc_relocate / _grow (values + apply) */, "mcmc_noise" /* gsrast_mcmc_noise */,
                                            "mlp_fwd" /* csrc/gsrast_mlp.h: gsrast_mlp3_forward */, "mlp_bwd" /* gsrast_mlp3_backward (the kernel + the partial-sum reduction) */ };
thread_local int t_prof_off = 0;      // > 0: the stages below are part of an enclosing one (cut_redo) and not recorded on their own
struct Pending { int id; hipEvent_t a, b; };
std::mutex g_prof_mu;
std::vector<Pending> g_pending;
double g_total_ms[K_COUNT];
long long g_launches[K_COUNT];

// roctx ranges (the stages as named ranges in a rocprofv3 --marker-trace): only with GSRAST_ROCTX set in the environment, the
// marker library looked up at run time (no link-time dependency).  A range brackets the host's ENQUEUE of a stage, as ranges do.
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx()
    {
        if (!getenv("GSRAST_ROCTX")) return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
const Roctx& roctx() { static const Roctx r; return r; }
} // namespace

// ---- what gsrast_host.h declares without a body: the one definition of each ------------------------------------------------------------
namespace gsrast {
OptionWords g_opt;
OptionWords::OptionWords() { for (const OptionRow& r : kOptions) r.word->store(r.def); }
gsrast_options snapshot_defaults()
{
    gsrast_options o{};
    for (const OptionRow& r : kOptions) if (r.field) o.*r.field = r.word->load();
    return o;
}

int fail(int code, const char* what, hipError_t e)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

RoctxRange::RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) (void)roctx().push(name); }
RoctxRange::~RoctxRange() { if (on) (void)roctx().pop(); }

ProfScope::ProfScope(int id_, hipStream_t s_) : id(id_), s(s_), on((id_ < 32 ? ((g_opt.profile.load() >> id_) & 1) != 0 : g_opt.profile.load() == -1) && (t_prof_off == 0 || id_ == K_CUT_REDO)), range(kKernelNames[id_])
{
    if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
}
ProfScope::~ProfScope()
{
    if (on) {
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_pending.push_back({ id, a, b });
    }
}

int post_launch(const char* what, hipStream_t s)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GSRAST_E_DEVICE, what, e);
    static const bool env_sync = getenv("GSRAST_DEBUG_SYNC") != nullptr;      // (diagnostics: localise a faulting launch)
    if (g_opt.debug_sync.load() || env_sync) {
        if (env_sync) fprintf(stderr, "[gsrast] %s\n", what);
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GSRAST_E_DEVICE, what, e);
    }
    return GSRAST_OK;
}
} // namespace gsrast

namespace {
// ---- scan / sort drivers --------------------------------------------------------------------
// dst[i] = scan of (idx ? src[idx[i]] : src[i]); two levels (single-block scan of block sums).
// `aux` (optional, n entries): only summed; its 64-bit total goes to aux_lo / aux_hi.
int scan_u32(const uint32_t* src, const uint32_t* idx, uint32_t n, uint32_t* dst, bool inclusive,
             uint32_t* tmp, uint32_t* total_out, hipStream_t s, const uint2* runs = nullptr,
             const uint32_t* aux = nullptr, uint32_t* aux_lo = nullptr, uint32_t* aux_hi = nullptr)
{
    if (n == 0) return GSRAST_OK;
    const uint32_t nb = (n + SC_CHUNK - 1) / SC_CHUNK;
    if (nb == 1 && !aux) {
        scan_apply_kernel<<<1, 256, 0, s>>>(src, idx, runs, n, nullptr, dst, inclusive ? 1 : 0, total_out);
        GS_LAUNCHED("scan_apply");
        return GSRAST_OK;
    }
    scan_block_sums_kernel<<<nb, 256, 0, s>>>(src, idx, runs, n, tmp, aux, tmp + nb);
    GS_LAUNCHED("scan_block_sums");
    scan_single_block_kernel<<<1, 256, 0, s>>>(tmp, nb, aux ? tmp + nb : nullptr, aux_lo, aux_hi);
    GS_LAUNCHED("scan_single_block");
    scan_apply_kernel<<<nb, 256, 0, s>>>(src, idx, runs, n, tmp, dst, inclusive ? 1 : 0, total_out);
    GS_LAUNCHED("scan_apply");
    return GSRAST_OK;
}

// Stable sort of n (key,value) pairs on the low `bits` key bits, in ceil(bits/8) passes of (nearly)
// equal digit width (13 bits -> 7 + 6: narrower digits mean fewer bins per block, i.e. longer
// contiguous runs in the scatter's write-out).  Result ends in (kA,vA) if the pass count is even,
// else in (kB,vB).
// ITEMS = elements per lane: a workgroup sorts 256 * ITEMS consecutive elements.  The R-sized sort wants 16 (long
// contiguous runs in the write-out); the P- and Q-sized ones have too few elements to fill 256 CUs with 4096-element
// chunks (1 M Gaussians = 245 workgroups) and run faster with smaller ones.
// Device-side pass-count adaptation of the 32-bit depth sort (gsrast_binning.h: RA_*): a third buffer pair, the per-block
// key minima / maxima of pass 0, and the word that receives the number of significant key bits.
template <typename KeyT, typename ValT> struct SortAdapt { KeyT* kC; ValT* vC; uint32_t* block_minmax; uint32_t* sig; bool assume_short; };

template <typename KeyT, typename ValT = uint32_t, int ITEMS = RS_ITEMS>
int radix_sort(KeyT* kA, ValT* vA, KeyT* kB, ValT* vB, uint32_t n, int bits,
               uint32_t* hist, uint32_t* scan_tmp, hipStream_t s,
               const uint2* gather_rect = nullptr, uint32_t* gather_tiles = nullptr, uint32_t* gather_width = nullptr,
               const uint32_t* n_dev = nullptr /* n is a capacity, the real count is on the device (dev_count) */,
               const SortAdapt<KeyT, ValT>* ad = nullptr, const uint32_t* pred = nullptr /* predicated launch (list cut): only on the plain path below */)
{
    if (n == 0) return GSRAST_OK;
    const uint32_t nblk = (n + RS_THREADS * ITEMS - 1) / (RS_THREADS * ITEMS);
    const int passes = radix_passes(bits);
    if (ad && passes == 4 && bits == 32 && nblk > RS_SELF_SCAN_BLOCKS) {
        // A -> B -> (short ? C : A) -> (short ? A : B) -> [A]: see RA_* in gsrast_binning.h.  The result is in (kA, vA).
        const uint32_t mask = 255u;
        const int as = ad->assume_short ? RA_ASSUME : 0;
        for (int p = 0; p < (ad->assume_short ? 3 : 4); p++) {
            const int shift = 8 * p;
            const KeyT* kin = (p & 1) ? kB : kA; const ValT* vin = (p & 1) ? vB : vA;      // the long sort's ping-pong
            KeyT* kout = (p & 1) ? kA : kB; ValT* vout = (p & 1) ? vA : vB;
            const int hmode = (p == 0 ? RA_MINMAX : p == 2 ? RA_IN_ALT : p == 3 ? RA_SKIP : 0) | as;
            const int smode = (p == 1 ? RA_OUT_ALT : p == 2 ? (RA_IN_ALT | RA_OUT_ALT | RA_LAST_IF_SHORT) : p == 3 ? RA_SKIP : 0) | as;
            radix_hist_kernel<KeyT, ITEMS><<<nblk, RS_THREADS, 0, s>>>(kin, n, n_dev, shift, mask, hist, nblk, ad->kC, p ? ad->sig : nullptr, hmode, ad->block_minmax);
            GS_LAUNCHED("radix_hist");
            radix_rowscan_kernel<<<mask + 1 + (p == 0 ? 1 : 0), 256, 0, s>>>(hist, nblk, scan_tmp, ad->sig, (p == 0 ? RA_MINMAX : p == 3 ? RA_SKIP : 0) | as, ad->block_minmax, mask + 1);
            GS_LAUNCHED("radix_rowscan");
            // pass 1 writes C when short; pass 2 reads C and writes A when short (and gathers: it is then the last pass)
            radix_scatter_kernel<KeyT, ValT, ITEMS><<<nblk, RS_THREADS, 0, s>>>(kin, vin, kout, vout, n, n_dev, shift, mask, hist, scan_tmp, nblk,
                                                                         p >= 2 ? gather_rect : nullptr, gather_tiles, gather_width,
                                                                         ad->kC, ad->vC, p == 1 ? ad->kC : kA, p == 1 ? ad->vC : vA, ad->sig, smode);
            GS_LAUNCHED("radix_scatter");
        }
        return GSRAST_OK;
    }
    int shift = 0;
    for (int p = 0; p < passes; p++) {
        const int w = (bits - shift + (passes - p) - 1) / (passes - p);   // remaining bits spread evenly (7+6 == 6+7 measured)
        const uint32_t mask = (1u << w) - 1u;
        radix_hist_kernel<KeyT, ITEMS><<<nblk, RS_THREADS, 0, s>>>(kA, n, n_dev, shift, mask, hist, nblk, nullptr, nullptr, 0, nullptr, pred);
        GS_LAUNCHED("radix_hist");
        const bool self_scan = nblk <= RS_SELF_SCAN_BLOCKS;      // the scatter blocks sum the few block counts themselves
        if (!self_scan) {
            radix_rowscan_kernel<<<mask + 1, 256, 0, s>>>(hist, nblk, scan_tmp, nullptr, 0, nullptr, 0, pred);     // one workgroup per digit value in use
            GS_LAUNCHED("radix_rowscan");
        }
        const bool last = p == passes - 1;
        radix_scatter_kernel<KeyT, ValT, ITEMS><<<nblk, RS_THREADS, 0, s>>>(kA, vA, kB, vB, n, n_dev, shift, mask, hist,
                                                                     self_scan ? nullptr : scan_tmp, nblk,
                                                                     last ? gather_rect : nullptr, gather_tiles, gather_width,
                                                                     nullptr, nullptr, nullptr, nullptr, nullptr, 0, pred);
        GS_LAUNCHED("radix_scatter");
        std::swap(kA, kB); std::swap(vA, vB);
        shift += w;
    }
    return GSRAST_OK;
}

} // namespace
namespace gsrast {
int radix_passes(int bits) { int p = (bits + 7) / 8; return p ? p : 1; }
// the sorts of the training unit (gsrast_host.h): k-NN's Morton codes (P elements, sized as the depth sort), the hexplane backward's texel keys
int sort_pairs_small(uint32_t* kA, uint32_t* vA, uint32_t* kB, uint32_t* vB, uint32_t n, int bits, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s) { return radix_sort<uint32_t, uint32_t, GSRAST_DEPTH_ITEMS>(kA, vA, kB, vB, n, bits, hist, scan_tmp, s); }
int sort_pairs_large(uint32_t* kA, uint32_t* vA, uint32_t* kB, uint32_t* vB, uint32_t n, int bits, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s) { return radix_sort<uint32_t, uint32_t, RS_ITEMS>(kA, vA, kB, vB, n, bits, hist, scan_tmp, s); }
} // namespace gsrast
namespace {

// Low-latency readback of one device word: async copy into pinned host memory, then spin on an event
// (hipStreamSynchronize may sleep; the GPU is idle while we wait, so every microsecond counts).
struct Readback {     // 64 pinned bytes + one event per (host thread, device); deliberately never freed: the destructor of a
    uint32_t* pinned = nullptr; hipEvent_t ev = nullptr;   // thread_local would call into the HIP runtime at thread / process exit,
    uint32_t* dev_alias = nullptr;                         // possibly after the runtime itself has been torn down
    uint32_t seq = 0;       // dev_alias: the same 64 bytes as the device sees them (a kernel stores the counts there itself: read_flag_*)
    uint32_t fb_seen = 0;   // list cut: sequence number of the last fallback this thread has taken note of (word RB_FALLBACK)
    bool prepared = false;  // read_flag_prepare has run for the forward in progress (the pose-found word is waited for before the counts)
};
// 64-bit words of the pinned buffer (128 bytes): the counts of depth_bucket_totals (kReadbackWord, gsrast_common.h), then RB_FOUND, RB_FALLBACK
constexpr size_t RB_BYTES = 128;
constexpr int kCountWords = SC_BUCKET_OVER + 1;      // the words of GeomLayout::scalars a forward's host reads back (ForwardRun::counts): SC_R_LO ... SC_BUCKET_OVER
static_assert([] { for (int w : kReadbackWord) if (w >= kCountWords) return false; return true; }(), "a read-back word the host's copy has no room for");
constexpr int kMaxDevices = 32;      // devices a context keeps a record for (DeviceState) and a host thread a read-back buffer: THE bound, spelt nowhere else
thread_local Readback t_readback[kMaxDevices];     // one per (host thread, device): events belong to a device
// The calling thread's current device, or -1: none (no runtime, or an exotic topology beyond kMaxDevices) -- such a call has no side stream,
// no gate, no hints, its own tables, and a blocking copy for the read-back.  A render call asks ONCE, at its top.
int current_device()
{
    int device = 0;
    return (hipGetDevice(&device) == hipSuccess && device >= 0 && device < kMaxDevices) ? device : -1;
}
// begin: enqueue the copy + event; finish: spin until it landed.  Work enqueued between the two runs on the GPU while
// the host waits (speculative launch in gsrast_forward).
int read_u32_begin(int device, const uint32_t* dev, hipStream_t s, int nwords, Readback** handle)
{
    *handle = nullptr;
    if (device < 0) return GSRAST_OK;      // no device record: finish() does a blocking copy
    Readback& rb = t_readback[device];
    if (!rb.pinned) {
        GS_HIP(hipHostMalloc((void**)&rb.pinned, RB_BYTES, hipHostMallocPortable | hipHostMallocMapped));
        GS_HIP(hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming));
        if (hipHostGetDevicePointer((void**)&rb.dev_alias, rb.pinned, 0) != hipSuccess) rb.dev_alias = nullptr;
        memset(rb.pinned, 0, RB_BYTES);
    }
    GS_HIP(hipMemcpyAsync(rb.pinned, dev, sizeof(uint32_t) * nwords, hipMemcpyDeviceToHost, s));
    GS_HIP(hipEventRecord(rb.ev, s));
    *handle = &rb;
    return GSRAST_OK;
}
int read_u32_finish(Readback* rb, const uint32_t* dev, hipStream_t s, uint32_t* out, int nwords)
{
    if (!rb) {
        GS_HIP(hipMemcpyAsync(out, dev, sizeof(uint32_t) * nwords, hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        return GSRAST_OK;
    }
    hipError_t e;
    while ((e = hipEventQuery(rb->ev)) == hipErrorNotReady) { }
    if (e != hipSuccess) return fail(GSRAST_E_DEVICE, "read_u32", e);
    for (int k = 0; k < nwords; k++) out[k] = rb->pinned[k];
    return GSRAST_OK;
}
// The read-back without a copy: the producing kernel stores the (12) words into the pinned buffer itself and then the sequence number
// into word 15 (depth_bucket_totals).  prepare: the buffer's device alias and this call's sequence number, or nullptr if mapped host
// memory is not to be had (the caller then uses the copy).  finish: spin on word 15; should it not arrive within two seconds the stream
// is drained and the counts are copied the slow way (a failed launch surfaces there).
Readback* read_flag_prepare(int device, uint32_t** dev_alias, uint32_t* seq)
{
    if (device < 0) return nullptr;
    Readback& rb = t_readback[device];
    if (!rb.pinned) {
        if (hipHostMalloc((void**)&rb.pinned, RB_BYTES, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { rb.pinned = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipHostGetDevicePointer((void**)&rb.dev_alias, rb.pinned, 0) != hipSuccess) rb.dev_alias = nullptr;
        memset(rb.pinned, 0, RB_BYTES);
    }
    if (!rb.dev_alias) return nullptr;
    rb.seq = rb.seq + 1u ? rb.seq + 1u : 1u;
    for (int k = 0; k <= RB_FOUND; k++) reinterpret_cast<volatile unsigned long long*>(rb.pinned)[k] = 0ull;      // (no stale word may carry this number)
    std::atomic_thread_fence(std::memory_order_seq_cst);
    *dev_alias = rb.dev_alias; *seq = rb.seq;
    return &rb;
}
int read_flag_finish(Readback* rb, const uint32_t* dev, hipStream_t s, uint32_t* out /* [kCountWords] */)
{
    constexpr int nwords = kCountWords;
    // RB_WORDS 64-bit words {value, sequence number} (depth_bucket_totals): each is valid as soon as its upper half carries this call's number
    volatile unsigned long long* p = reinterpret_cast<volatile unsigned long long*>(rb->pinned);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long w[RB_WORDS];
    for (int k = 0; k < RB_WORDS; k++) {
        for (uint64_t spins = 1; (uint32_t)((w[k] = p[k]) >> 32) != rb->seq; spins++) {
            if ((spins & 0xFFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
                GS_HIP(hipStreamSynchronize(s));
                if ((uint32_t)((w[k] = p[k]) >> 32) == rb->seq) break;
                GS_HIP(hipMemcpy(out, dev, sizeof(uint32_t) * nwords, hipMemcpyDeviceToHost));
                return GSRAST_OK;
            }
        }
    }
    for (int k = 0; k < nwords; k++) out[k] = 0u;
    for (int k = 0; k < RB_WORDS; k++) out[kReadbackWord[k]] = (uint32_t)w[k];      // (the kernel's own order: one list, gsrast_common.h)
    return GSRAST_OK;
}
// the pose-found word of preprocess_fwd (RB_FOUND): 1 / 0, or 0 ("size the launches as for an unknown pose": all column runs, the safe
// sizing) if it does not arrive within 200 ms
bool read_found(Readback* rb)
{
    volatile unsigned long long* p = reinterpret_cast<volatile unsigned long long*>(rb->pinned) + RB_FOUND;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long w;
    for (uint64_t spins = 1; (uint32_t)((w = *p) >> 32) != rb->seq; spins++)
        if ((spins & 0xFFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
    return (uint32_t)w != 0u;
}
// has the device reported a completion pass of the list cut this thread has not taken note of yet (RB_FALLBACK)?  Returns the number
// of column runs of that pass's candidates (0: nothing new).
uint32_t take_fallback_event(int device)
{
    if (device < 0) return 0u;
    Readback& rb = t_readback[device];
    if (!rb.pinned) return 0u;
    const unsigned long long w = reinterpret_cast<volatile unsigned long long*>(rb.pinned)[RB_FALLBACK];
    const uint32_t sq = (uint32_t)(w >> 32);
    if (sq == 0u || sq == rb.fb_seen) return 0u;
    rb.fb_seen = sq;
    return (uint32_t)w ? (uint32_t)w : 1u;
}
int read_u32(int device, const uint32_t* dev, hipStream_t s, uint32_t* out, int nwords = 1)
{
    Readback* rb = nullptr;
    int rc = read_u32_begin(device, dev, s, nwords, &rb);
    if (rc != GSRAST_OK) return rc;
    return read_u32_finish(rb, dev, s, out, nwords);
}
// Instances of the previous forward call: the binning buffer is requested for 1.25x that many BEFORE
// the host waits for the real count, so the (Python) allocation callback runs while the GPU is still
// busy with preprocess / depth sort instead of in the idle gap after the readback.
// These hints (and the counts of the last call) belong to a gsrast_context: one per caller that renders a sequence of similar
// views.  The reference-shaped entry points use a context private to the calling host thread.
} // namespace
struct SideStream { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr; };
// The list cut's completion pass OFF the critical path (round 4).  Its eleven predicated launches used to sit between the forward blend and
// whatever the caller enqueues next: 55-80 us of dependent-launch latency in the steady state, where every one of them returns at once.
// Now the blend's LAST workgroup (gsrast_blend.h, GateArgs) copies the blend's verdict into a word of the context's own (`pred`: the chain's predicate; the
// forward's buffers may be gone by the time the chain's no-ops run) and, if the verdict is "nothing to complete", releases the caller's
// stream at once (`done` = the call's sequence number, waited for with hipStreamWaitValue32); the chain runs on a second stream behind
// the blend and, if it had work to do, releases the caller's stream at its end.  Deadlock-free on in-order hardware queues however HIP
// maps streams onto them: everything the wait can be released by is SUBMITTED before the wait (gate kernel, event, chain, last the wait).
// The release / predicate words are a ring of GATE_RING slots indexed by the call's sequence number.  A slot may only be claimed again once
// every launch that can still read it has run: the host records an event behind each chain (`tail`) and claims sequence number n only
// if the chain of n - GATE_RING / 2 has completed (hipEventQuery, no wait) -- otherwise that call runs its completion pass inline on the
// caller's stream, the round-3 form, which needs no slot.  So at most GATE_RING / 2 chains are ever pending and no slot is rewritten
// under a chain (the gate stream has the lowest priority and nothing else bounded its backlog).
// A profiler that collects hardware counters SERIALISES the device's kernels: the caller's stream would sit in its wait while the chain that
// releases it cannot start (round 5: every rocprofv3 --pmc pass of bench.py hung until its timeout).  rocprofv3 announces counter collection
// in the environment of the process it launches; the completion pass then runs inline on the caller's stream, as with option chain_gate = 0.
static bool counter_collection_env()
{
    static const bool on = getenv("ROCPROF_COUNTERS") != nullptr || getenv("ROCPROF_COUNTER_GROUPS") != nullptr || getenv("GSRAST_SERIALIZED_KERNELS") != nullptr;
    return on;
}
constexpr uint32_t GATE_RING = 64;
struct ChainGate { hipStream_t stream = nullptr; hipEvent_t ev = nullptr; uint32_t* words = nullptr /* [64] done | [64] pred */; uint32_t seq = 0; bool failed = false;
                   hipEvent_t tail[GATE_RING] = {}; uint32_t tail_seq[GATE_RING] = {} /* sequence number whose chain the slot's event follows; 0 = none */; uint32_t inline_calls = 0 /* forwards that found the ring's older half still pending (diagnostic) */; };
__global__ void chain_done_kernel(const uint32_t* __restrict__ pred_copy, uint32_t* __restrict__ done, uint32_t seq)
{
    if (*pred_copy != 0u) __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ---- what a context owns on ONE device (gsrast_context::dev[current_device()]): every piece created on first use, by the member that hands
// it out, under the context's mutex `mu`.  A call resolves its record once, at its top, and every stage uses that pointer. ----
namespace {
struct DeviceState {
    SideStream side;                  // the stream the colour kernel runs on beside the sort
    ChainGate gate;                   // the completion pass's own stream and release words
    uint32_t* tau = nullptr; size_t tau_words = 0; bool tau_dirty = false;      // the predicted cut's opacity-mass table [TAU_COPIES][T][TAU_BINS] (ImgLayout::tau_hist's twin), kept ZERO between
                                                                                // forwards: filled by preprocess_fwd, read by tau_cut_kernel, zeroed again by the bucket sort behind it -- no memset launch per forward
    uint32_t* zhist = nullptr;        // the sampled depth histogram of the bucket depth sort [ZH_COPIES][ZH_BINS] -- filled by preprocess_fwd, read by the
                                      // scatter, zeroed again by the bucket sort behind it (no memset launch per forward).  Two forwards of one context in flight on two
                                      // streams mix their samples: the bucket map stays monotone whatever the histogram holds (gsrast_common.h), only the balance suffers
    struct Hints { HintTable* table = nullptr; uint32_t T = 0; uint64_t used = 0; } hints[4];   // launch-order hints of the forward blend (gsrast_common.h), device memory: one table per image size in use, up to four (train / eval resolutions alternate)
    uint64_t hints_clock = 0;         // ... and their least-recently-used clock

    // The side stream (lowest priority: its bandwidth-heavy kernels should fill the gaps the critical path leaves, not compete with it for
    // compute units).  nullptr if it cannot be had.
    SideStream* side_stream(std::mutex& mu)
    {
        std::lock_guard<std::mutex> lk(mu);
        SideStream& x = side;
        if (!x.stream) {
            int prio_least = 0, prio_greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
            if (hipStreamCreateWithPriority(&x.stream, hipStreamNonBlocking, prio_least) != hipSuccess) { x.stream = nullptr; return nullptr; }
            if (hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&x.join2, hipEventDisableTiming) != hipSuccess) {
                if (x.fork) (void)hipEventDestroy(x.fork);          // all or nothing: the next call tries again
                if (x.join) (void)hipEventDestroy(x.join);
                if (x.join2) (void)hipEventDestroy(x.join2);
                (void)hipStreamDestroy(x.stream);
                x = SideStream{};
                return nullptr;
            }
        }
        return &x;
    }
    // The completion pass's gate; nullptr if the device cannot wait on a memory word, or once anything about the gate has failed (`failed` latches)
    ChainGate* chain_gate(std::mutex& mu, int device)
    {
        int can = 0;
        std::lock_guard<std::mutex> lk(mu);
        ChainGate& g = gate;
        if (g.failed) return nullptr;
        if (!g.stream) {
            g.failed = true;                      // (until everything below has worked)
            if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess || !can) return nullptr;
            int prio_least = 0, prio_greatest = 0;      // (lowest priority: the pass's no-ops run beside the backward and must not stand in its workgroups' way)
            (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
            if (hipMalloc((void**)&g.words, 128 * sizeof(uint32_t)) != hipSuccess) { g.words = nullptr; return nullptr; }
            if (hipMemset(g.words, 0, 128 * sizeof(uint32_t)) != hipSuccess ||
                hipStreamCreateWithPriority(&g.stream, hipStreamNonBlocking, prio_least) != hipSuccess) { (void)hipFree(g.words); g = ChainGate{}; g.failed = true; return nullptr; }
            if (hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(g.stream); (void)hipFree(g.words); g = ChainGate{}; g.failed = true; return nullptr; }
            for (uint32_t k = 0; k < GATE_RING; k++)
                if (hipEventCreateWithFlags(&g.tail[k], hipEventDisableTiming) != hipSuccess) {
                    for (uint32_t j = 0; j < k; j++) (void)hipEventDestroy(g.tail[j]);
                    (void)hipEventDestroy(g.ev); (void)hipStreamDestroy(g.stream); (void)hipFree(g.words); g = ChainGate{}; g.failed = true; return nullptr;
                }
            g.failed = false;
        }
        return &g;
    }
    // The hint table for a T-tile image (allocated on first use, cleared when T changes); nullptr if it cannot be had -- the forward
    // then orders its blend by list length, as a first-seen pose does.
    HintTable* hint_table(std::mutex& mu, uint32_t T, hipStream_t s)
    {
        std::lock_guard<std::mutex> lk(mu);
        // one table per tile count, up to four per device (train and eval resolutions, mixed camera sizes: each keeps its poses); a fifth
        // size takes over the least recently used table's place (rare: drain, then start over)
        Hints* hp = nullptr;
        for (auto& c : hints) if (c.table && c.T == T) hp = &c;
        if (!hp) {
            for (auto& c : hints) if (!c.table) { hp = &c; break; }
            if (!hp) {
                hp = &hints[0];
                for (auto& c : hints) if (c.used < hp->used) hp = &c;
                (void)hipStreamSynchronize(s); (void)hipFree(hp->table); hp->table = nullptr;
            }
        }
        auto& h = *hp;
        h.used = ++hints_clock;
        if (!h.table) {
            if (hipMalloc((void**)&h.table, hint_table_bytes(T)) != hipSuccess) { h.table = nullptr; return nullptr; }
            h.T = T;
            if (hipMemsetAsync(h.table, 0, hint_zcut_offset(T), s) != hipSuccess ||
                hipMemsetAsync(reinterpret_cast<char*>(h.table) + hint_zcut_offset(T), 0xFF, (size_t)HINT_SLOTS * T * 4, s) != hipSuccess) { (void)hipFree(h.table); h.table = nullptr; return nullptr; }
        }
        return h.table;
    }
    // The depth histogram, zero; nullptr if no memory is to be had (the call then uses its own table and a memset)
    uint32_t* depth_hist(std::mutex& mu)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!zhist) {
            uint32_t* z = nullptr;
            if (hipMalloc((void**)&z, ZH_COPIES * ZH_BINS * sizeof(uint32_t)) == hipSuccess) {
                if (hipMemset(z, 0, ZH_COPIES * ZH_BINS * sizeof(uint32_t)) == hipSuccess) zhist = z; else (void)hipFree(z);
            }
        }
        return zhist;
    }
    // The opacity-mass table of at least `words` words, zero on `s` and marked dirty (the bucket sort that zeroes it again clears the mark);
    // nullptr if it cannot be had or zeroed (the call then uses its own table and a memset, which reports what is wrong with the stream)
    uint32_t* mass_table(std::mutex& mu, size_t words, hipStream_t s)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (tau_words < words) {
            if (tau) { (void)hipFree(tau); tau = nullptr; tau_words = 0; }
            uint32_t* z = nullptr;
            if (hipMalloc((void**)&z, words * sizeof(uint32_t)) == hipSuccess) { tau = z; tau_words = words; tau_dirty = true; }
        }
        if (!tau) return nullptr;
        // (a fresh table, or a forward that filled it and never reached its bucket sort: zeroed here)
        if (tau_dirty && hipMemsetAsync(tau, 0, tau_words * sizeof(uint32_t), s) != hipSuccess) return nullptr;
        tau_dirty = true;
        return tau;
    }
    // gsrast_context_destroy: the streams are drained before they are destroyed
    void release()
    {
        for (auto& h : hints) if (h.table) (void)hipFree(h.table);
        if (gate.stream) { (void)hipStreamSynchronize(gate.stream); (void)hipStreamDestroy(gate.stream); }
        if (gate.ev) (void)hipEventDestroy(gate.ev);
        for (hipEvent_t e : gate.tail) if (e) (void)hipEventDestroy(e);
        if (gate.words) (void)hipFree(gate.words);
        if (zhist) (void)hipFree(zhist);
        if (tau) (void)hipFree(tau);
        if (side.stream) { (void)hipStreamSynchronize(side.stream); (void)hipStreamDestroy(side.stream); }
        if (side.fork) (void)hipEventDestroy(side.fork);
        if (side.join) (void)hipEventDestroy(side.join);
        if (side.join2) (void)hipEventDestroy(side.join2);
    }
};
} // namespace
struct gsrast_context {
    std::atomic<uint32_t> R_hint{0}, Q_hint{0}, last_R{0}, last_Q{0}, last_late{0}, last_Qe{0};
    std::atomic<uint32_t> Qe_hint{0};  // list cut: column runs of the early Gaussians in recent forwards (sizes the launches over the cut lists)
    std::atomic<uint32_t> Qe_hint_tau{0};  // ... of the forwards that ran under PREDICTED cut depths (they keep more: their own hint)
    CutPolicy pol;                     // list cut: when it is applied, paused, widened (gsrast_policy.h)
    // a HINT, nothing more: "the last forward whose view matrix lived at this device address found its pose in the table".  Callers keep
    // a camera's matrices in one tensor for its lifetime (scene/cameras.py:90-101), so a forward can tell BEFORE it launches anything
    // whether it will need predicted cut depths: a pose the table knows skips the opacity-mass histogram and its kernel.  A wrong guess
    // costs one forward its cut (an address reused for another camera: the snapshot finds no slot, nothing is predicted), never a result.
    std::unordered_map<const void*, uint8_t> pose_seen;
    // equalised depth buckets (gsrast_common.h): the key range the depth histogram's bins cover, learned from the previous forwards
    DepthRange zrange;                 // (gsrast_policy.h) klo / shift: the histogram's bins; khi: the range's un-rounded upper end (the predicted cut's bins span [klo, khi])
    std::atomic<uint32_t> last_prologue_ns{0};   // host time of the last forward from entry to the launch of its first kernel (diagnostic: tools/sync_probe.py)
    std::atomic<int> redo_count{0};   // forwards whose speculative launch did not fit and was repeated with exact sizes
    DepthSortPolicy zsort;            // the bucket depth sort's back-off after an overflow ("bucket_skip"), the radix sort's pass-count hint (gsrast_policy.h)
    DeviceState dev[kMaxDevices];     // per device: streams, gate, tables, hints
    std::mutex mu;
    DeviceState* device_state(int device) { return device >= 0 ? &dev[device] : nullptr; }      // (device: current_device())
};
namespace {
// TESTS ONLY (option "mutate"): a backward that is wrong on purpose, so that a test can show its tolerance would catch it (the
// full-size gradient bar let an all-zero dL/dsh pass).  bit 0: the blend backward of ONE tile -- the image's centre tile -- does not see the 64
// front-most entries of the tile's list (one staged batch dropped: the tile's range, its pixels' n_contrib and its tile_max are shifted by a
// small kernel in front of the blend backward; every other (pixel, Gaussian) pair gets exactly what it gets without the mutation).
// bit 1: the background term of dL/dalpha (backward.cu:531-534) is dropped (the blend backward is handed a zero background).
__global__ void mutate_drop_front_batch_kernel(uint2* ranges, uint32_t* n_contrib, uint32_t* tile_max, uint32_t tile, int W, int H, int gx)
{
    const uint32_t tx = tile % (uint32_t)gx, ty = tile / (uint32_t)gx;
    const uint32_t px = tx * TILE_X + (threadIdx.x & 15u), py = ty * TILE_Y + (threadIdx.x >> 4);
    const uint2 r = ranges[tile];
    const uint32_t drop = (r.y - r.x) < 64u ? (r.y - r.x) : 64u;
    __syncthreads();
    if (px < (uint32_t)W && py < (uint32_t)H) { const size_t pid = (size_t)W * py + px; const uint32_t c = n_contrib[pid]; n_contrib[pid] = c > drop ? c - drop : 0u; }
    if (threadIdx.x == 0) { ranges[tile] = make_uint2(r.x + drop, r.y); const uint32_t m = tile_max[tile]; tile_max[tile] = m > drop ? m - drop : 0u; }
}
gsrast_context* thread_context()
{   // deliberately leaked at thread exit -- the host words AND the device pose tables it has grown (12.5 MB per image size at 1080p, include/gsrast.h):
    // see Readback above for why nothing here has a destructor; a host thread that renders and exits should use gsrast_context_create / _destroy
    thread_local gsrast_context* c = new gsrast_context();
    return c;
}

CamArgs make_cam(const float* view, const float* proj, const float* campos, float tanx, float tany,
                 float scale_mod, int W, int H)
{
    CamArgs c;
    c.view = view; c.proj = proj; c.campos = campos;
    c.tanx = tanx; c.tany = tany;
    c.fy = H / (2.0f * tany);   // reference rasterizer_impl.cu:222-223
    c.fx = W / (2.0f * tanx);
    c.scale_mod = scale_mod;
    c.W = W; c.H = H; c.gx = (W + TILE_X - 1) / TILE_X; c.gy = (H + TILE_Y - 1) / TILE_Y;
    return c;
}

__global__ void __launch_bounds__(256)
export_geom_kernel(int P, const float4* __restrict__ rec0,
                   const float4* __restrict__ rec1, const float4* __restrict__ rec2,
                   const float* __restrict__ cov3D_in, const unsigned char* __restrict__ clamped_in,
                   const uint32_t* __restrict__ tiles_in, float* depths, float* means2D, float* cov3D,
                   float* conic_opacity, float* rgb, unsigned char* clamped, uint32_t* tiles)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const bool vis = tiles_in[i] != 0;
    const float4 a = rec0[(size_t)REC_STRIDE * i], b = rec1[(size_t)REC_STRIDE * i], c = rec2[(size_t)REC_STRIDE * i];
    if (depths) depths[i] = vis ? b.z : 0.0f;
    if (means2D) { means2D[2 * i] = vis ? a.x : 0.f; means2D[2 * i + 1] = vis ? a.y : 0.f; }
    if (cov3D) for (int k = 0; k < 6; k++) cov3D[6 * i + k] = cov3D_in[6 * i + k];
    if (conic_opacity) {
        conic_opacity[4 * i] = vis ? a.z : 0.f; conic_opacity[4 * i + 1] = vis ? a.w : 0.f;
        conic_opacity[4 * i + 2] = vis ? b.x : 0.f; conic_opacity[4 * i + 3] = vis ? b.y : 0.f;
    }
    if (rgb) { rgb[3 * i] = vis ? c.x : 0.f; rgb[3 * i + 1] = vis ? c.y : 0.f; rgb[3 * i + 2] = vis ? c.z : 0.f; }
    if (clamped) {
        const unsigned cl = vis ? clamped_in[i] : 0u;
        clamped[3 * i] = cl & 1u; clamped[3 * i + 1] = (cl >> 1) & 1u; clamped[3 * i + 2] = (cl >> 2) & 1u;
    }
    if (tiles) tiles[i] = tiles_in[i];
}

__global__ void __launch_bounds__(256) iota_kernel(uint32_t* __restrict__ v, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) v[i] = i;
}

// one workgroup per tile: the 64-bit keys of the reference, rebuilt from the tile's range
__global__ void __launch_bounds__(256)
export_keys_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ vals_sorted,
                   const float4* __restrict__ rec1 /* .z = depth */, uint64_t* keys, uint32_t* point_list, uint32_t R /* entries of the two output arrays */)
{
    const uint2 r = ranges[blockIdx.x];
    // (a tile the list cut's completion pass listed again has its range in the point list's second half, past R: not exported -- the
    // entry-by-entry comparisons run with tile_clip = 0, i.e. without the cut)
    for (uint32_t i = r.x + threadIdx.x; i < r.y && i < R; i += 256) {
        const uint32_t g = vals_sorted[i];
        if (keys) keys[i] = ((uint64_t)blockIdx.x << 32) | (uint64_t)__float_as_uint(rec1[(size_t)REC_STRIDE * g].z);
        if (point_list) point_list[i] = g;
    }
}

struct BlendArgs {
    uint32_t* bcnt = nullptr; uint16_t* blist = nullptr; int from_buckets = 0;   // launch order from the work buckets (ImgLayout)
    const uint2* ranges; const uint32_t* plist; const uint32_t* order; int W, H, gx; uint32_t T; const float4 *r0, *r1, *r2; const float* bg;
    float *oc, *od, *fT; uint32_t *nc, *tm;                       // forward outputs (fT / nc / tm: inputs of backward)
    const float* dpix; float* grec;                              // backward
    float4* zero4 = nullptr; uint32_t n_zero4 = 0;               // forward (culling kernel): the gradient records to zero-fill
    HintTable* hints = nullptr; const uint32_t* hint_sel = nullptr;   // forward: the context's launch-order hints, this call's slot
    const uint32_t* zcut_used = nullptr; uint32_t* cut_scalars = nullptr; const uint32_t* pred = nullptr;   // forward: list cut (gsrast_common.h)
    unsigned char* tile_flags = nullptr;                         // forward: tiles the completion pass lists and blends again
    GateArgs gate{};                                             // forward, list cut's first pass: the completion pass's gate (ChainGate)
    uint32_t cut_margin_x4 = 6;                                  // forward: the next cut depth's margin (gsrast_context::cut_margin)
    unsigned char* untouched = nullptr;                          // forward (culling kernel): GeomLayout::untouched
    float *oad = nullptr, *oal = nullptr;                        // forward (culling kernel), aux: acc_depth / alpha -- non-null selects AUX
    const float *dad = nullptr, *dal = nullptr;                  // backward, aux: dL/dacc_depth / dL/dalpha (either may be null)
};

// blend forward: <exp_mode> x (culled: <aux> | un-culled: <pixels per lane>)
void launch_blend_fwd(int exp_mode, bool cull, int ppl, uint32_t grid, hipStream_t s, const BlendArgs& a)
{
    pick_int<0, 1, 2>(exp_mode, [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        if (cull) pick_bool(a.oad != nullptr, [&](auto aux) {
            constexpr bool AUX = decltype(aux)::value;
            blend_fwd_cull_kernel<MODE, AUX><<<grid, 256, 0, s>>>(a.ranges, a.plist, a.order, a.W, a.H, a.gx, a.T, a.r0, a.r1, a.r2, a.bg, a.oc, a.od, a.fT, a.nc, a.tm,
                                                                  a.bcnt, a.blist, a.from_buckets, a.zero4, a.n_zero4, a.hints, a.hint_sel, a.zcut_used, a.cut_scalars, a.pred, a.tile_flags, a.gate, a.cut_margin_x4, a.untouched,
                                                                  AUX ? a.oad : nullptr, AUX ? a.oal : nullptr);
        });
        else pick_int<4, 2, 1>(ppl, [&](auto lanes) {
            constexpr int PPL = decltype(lanes)::value;
            blend_fwd_kernel<MODE, PPL><<<grid, 256 / PPL, 0, s>>>(a.ranges, a.plist, a.W, a.H, a.gx, a.T, a.r0, a.r1, a.r2, a.bg, a.oc, a.od, a.fT, a.nc, a.tm, a.bcnt, a.blist);
        });
    });
}

// blend backward: ablation | <exp_mode> x (transposed: <aux, abs> | culled: <pixels per lane> | un-culled: <pixels per lane>)
void launch_blend_bwd(int exp_mode, const BlendBwdPick& k, uint32_t grid, hipStream_t s, const BlendArgs& a)
{
    const uint32_t* bcnt = a.from_buckets ? a.bcnt : nullptr;
    auto uncull = [&](auto mode, auto lanes, auto abl) {
        constexpr int PPL = decltype(lanes)::value;
        blend_bwd_kernel<decltype(mode)::value, PPL, decltype(abl)::value><<<grid, 256 / PPL, 0, s>>>(a.ranges, a.plist, a.W, a.H, a.gx, a.T, a.r0, a.r1, a.r2, a.bg, a.fT, a.nc, a.tm, a.dpix, a.grec);
    };
    if (k.ablate) return pick_int<1, 2>(k.ablate, [&](auto abl) { uncull(int_c<0>{}, int_c<4>{}, abl); });
    pick_int<0, 1, 2>(exp_mode, [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        if (k.transposed) pick_bool(k.aux, [&](auto aux) { pick_bool(k.abs, [&](auto abs_c) {
            constexpr bool AUX = decltype(aux)::value, ABS = decltype(abs_c)::value;
            blend_bwd_cull_t_kernel<MODE, AUX, ABS><<<grid, 256, 0, s>>>(a.ranges, a.plist, a.order, a.W, a.H, a.gx, a.T, a.r0, a.r1, a.r2, a.bg, a.fT, a.nc, a.tm, a.dpix, a.grec,
                                                                         bcnt, a.blist, AUX ? a.dad : nullptr, AUX ? a.dal : nullptr);
        }); });
        else if (k.cull) pick_int<4, 2, 1>(k.ppl, [&](auto lanes) {
            constexpr int PPL = decltype(lanes)::value;
            blend_bwd_cull_kernel<MODE, PPL><<<grid, 256 / PPL, 0, s>>>(a.ranges, a.plist, a.order, a.W, a.H, a.gx, a.T, a.r0, a.r1, a.r2, a.bg, a.fT, a.nc, a.tm, a.dpix, a.grec, bcnt, a.blist);
        });
        else pick_int<4, 2, 1>(k.ppl, [&](auto lanes) { uncull(mode, lanes, int_c<0>{}); });
    });
}

// ---- the replays of a finished forward (gsrast_replay.h): what their five launches take from the forward's state -----------------------
struct ReplayLaunch {
    int W, H, gx; uint32_t T; unsigned grid;      // one workgroup per tile, the grid padded to xcd_tile's eight bands
    // the list in force, resolved as the blend backward resolves it: the tile's range (a tile the list cut's completion pass listed again has
    // its range in the point list's second half) into the point list at offset 0 of the binning buffer
    const uint2* ranges; const uint32_t* point_list;
    const float4 *rec0, *rec1; const float* final_T; const uint32_t *n_contrib, *tile_max;
    size_t grec;                                  // GeomLayout::grec: where the two backwards add
    ReplayLaunch(int P, int width, int height, const char* geom, const char* binning, const char* image)
    {
        const GeomLayout GL = geom_layout((size_t)P);
        const ImgLayout IL = img_layout((size_t)width, (size_t)height);
        W = width; H = height; gx = (width + TILE_X - 1) / TILE_X;
        T = (uint32_t)gx * (uint32_t)((height + TILE_Y - 1) / TILE_Y); grid = ((T + 7) / 8) * 8;
        ranges = at<uint2>(image, IL.ranges); point_list = at<uint32_t>(binning, 0);
        rec0 = at<float4>(geom, GL.rec0); rec1 = at<float4>(geom, GL.rec1); grec = GL.grec;
        final_T = at<float>(image, IL.final_T); n_contrib = at<uint32_t>(image, IL.n_contrib); tile_max = at<uint32_t>(image, IL.tile_max);
    }
    // the kernels' common leading arguments, then the kernel's own
    template <class K, class... A> void front_to_back(K kernel, hipStream_t s, A... own) const
    { kernel<<<grid, 256, 0, s>>>(ranges, point_list, W, H, gx, T, rec0, rec1, n_contrib, tile_max, own...); }
    template <class K, class... A> void back_to_front(K kernel, hipStream_t s, A... own) const
    { kernel<<<grid, 256, 0, s>>>(ranges, point_list, W, H, gx, T, rec0, rec1, final_T, n_contrib, tile_max, own...); }
};

} // namespace

extern "C" {

int gsrast_abi_version(void) { return GSRAST_ABI_VERSION; }
const char* gsrast_last_error(void) { return g_err.c_str(); }

void gsrast_options_init(gsrast_options* o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    for (const OptionRow& r : kOptions) if (r.field) o->*r.field = r.def;
}
gsrast_context* gsrast_context_create(void) { return new (std::nothrow) gsrast_context(); }
void gsrast_context_destroy(gsrast_context* c)
{
    if (!c) return;
    for (DeviceState& d : c->dev) d.release();
    delete c;
}
int gsrast_context_query(const gsrast_context* c, const char* name)
{
    if (!name) return GSRAST_E_ARG;
    if (!c) c = thread_context();
    if (!strcmp(name, "last_instances")) return (int)c->last_R.load();   // num_rendered / column runs of the context's last forward call
    if (!strcmp(name, "last_runs")) return (int)c->last_Q.load();
    if (!strcmp(name, "last_prologue_ns")) return (int)c->last_prologue_ns.load();
    if (!strcmp(name, "redo_count")) return c->redo_count.load();
    if (!strcmp(name, "bucket_skip")) return c->zsort.skip.load();
    if (!strcmp(name, "last_late")) return (int)c->last_late.load();
    if (!strcmp(name, "last_early_runs")) return (int)c->last_Qe.load();
    if (!strcmp(name, "completion_passes")) return (int)c->pol.passes_reported.load();
    if (!strcmp(name, "tau_req")) return c->pol.tau_req.load();
    if (!strcmp(name, "tau_force")) return c->pol.tau_force.load();
    if (!strcmp(name, "cut_margin_x4")) return c->pol.margin.load();      // the list cut's current margin, in quarters (6 = 1.5 x)
    if (!strcmp(name, "gate_inline_calls")) {     // cut forwards that ran their completion pass inline because the gate's ring was half full
        const int device = current_device();
        return device < 0 ? 0 : (int)c->dev[device].gate.inline_calls;
    }
    if (!strcmp(name, "cut_pause")) return c->pol.pause.load();      // forwards the list cut still sits out (too little saved, or its lists kept failing)
    if (!strcmp(name, "cut_fallbacks")) {       // a device counter in the hint table of the current device (diagnostic: waits for the device)
        const int device = current_device();
        if (device < 0) return 0;
        if (hipDeviceSynchronize() != hipSuccess) return GSRAST_E_DEVICE;
        uint32_t sum = 0;                       // (over the device's tables: one per image size)
        for (const auto& h : c->dev[device].hints) {
            uint32_t v = 0;
            if (h.table && hipMemcpy(&v, &h.table->cut_fallbacks, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return GSRAST_E_DEVICE;
            sum += v;
        }
        return (int)sum;
    }
    return GSRAST_E_ARG;
}

int gsrast_policy_event(gsrast_context* c, const char* what, int a, int b, int c3)
{
    if (!what) return GSRAST_E_ARG;
    if (!c) c = thread_context();
    CutPolicy& pol = c->pol;
    if (!strcmp(what, "begin")) {
        pol.begin_forward((uint32_t)a);
        c->last_R = (uint32_t)a;       // (the P the "counts" / "pass" events below refer to)
        const bool pays = pol.pays((uint32_t)b, c3 != 0);
        if (!pays) pol.sits_out();
        return pays ? 1 : 0;
    }
    if (!strcmp(what, "counts")) { pol.forward_counts((c3 & 1) != 0, (c3 & 2) ? 1u : 0u, (uint32_t)a, (uint32_t)b, c->last_R.load(), false); return pol.pause.load(); }
    if (!strcmp(what, "pass")) return pol.completion_pass((uint32_t)a, (uint32_t)b, c->last_R.load(), false, c3 != 0);
    if (!strcmp(what, "clean")) { pol.clean_cut_forward(); return pol.fb_score.load(); }
    if (!strcmp(what, "size")) return (int)early_launch_runs((uint32_t)a, (uint32_t)b, c3 != 0);
    if (!strcmp(what, "grow")) return (int)grow_capacity((uint32_t)a);
    if (!strcmp(what, "follow")) return (int)follow_hint((uint32_t)a, (uint32_t)b, c3);
    if (!strcmp(what, "depth_sort")) {      // a forward's outcome for the bucket depth sort's back-off: a = 0 radix (the bucket sort was asked for), 1 clean bucket sort, 2 overflow (b = 1: the table held every key)
        if (a == 0) c->zsort.radix_forward(); else if (a == 1) c->zsort.clean_forward(); else if (a == 2) (void)c->zsort.overflow(b != 0); else return GSRAST_E_ARG;
        return c->zsort.skip.load();
    }
    if (!strcmp(what, "reset")) { c->pol.~CutPolicy(); new (&c->pol) CutPolicy(); c->zsort.~DepthSortPolicy(); new (&c->zsort) DepthSortPolicy(); return 0; }      // (tests: fresh policies, whatever earlier calls left)
    if (!strcmp(what, "tau_min")) { pol.tau_min = std::max(1, a); pol.tau_req = std::max(1, a); return a; }      // (experiments: the predicted cut's requirement and its floor)
    if (!strcmp(what, "zrange")) {      // a = first | last << 16 occupied bin of a forward that used the context's current table -> the next table's shift (| 256 if that table had held every key)
        const uint32_t k = c->zrange.klo.load(); const int sh = c->zrange.shift.load();
        const bool held = c->zrange.learn((uint32_t)a, k, sh);
        return c->zrange.shift.load() | (held ? 256 : 0);
    }
    if (!strcmp(what, "zget")) return a == 0 ? (int)(c->zrange.klo.load() >> 8) : a == 1 ? c->zrange.shift.load() : (int)(c->zrange.khi.load() >> 8);      // (keys / 256: they do not fit an int)
    if (!strcmp(what, "get")) {
        switch (a) { case 0: return pol.pause.load(); case 1: return pol.fb_score.load(); case 2: return pol.margin.load(); case 3: return pol.tau_req.load();
                     case 4: return pol.tau_force.load(); case 5: return pol.fb_pause.load();
                     case 6: return c->zsort.skip.load(); case 7: return c->zsort.backoff.load(); case 8: return c->zsort.clean.load(); default: return GSRAST_E_ARG; }
    }
    return GSRAST_E_ARG;
}

int gsrast_debug_forward_plan(gsrast_context* c, const gsrast_options* options, unsigned flags, int P, int W, int H, const int* words)
{
    if (!options || !words) return fail(GSRAST_E_ARG, "debug_forward_plan: NULL argument");
    if (!c) c = thread_context();
    ForwardPlan p = plan_forward(*options, PlanInputs{ flags, P, W, H, words[4] >> 4, (words[4] & 1) != 0, (words[4] & 2) != 0, words[0], (uint32_t)words[1], (uint32_t)words[2], words[3] != 0 }, snapshot_switches());
    if (p.refusal) return fail(GSRAST_E_ARG, p.refusal);
    p.policy_answer(c->pol.pays(p.last_Q, p.list_cut_always), words[5] != 0);
    const bool bits[] = { p.runbin, p.buckets_ok, p.bucket_sort, p.two_level, p.culled, p.ordered, p.want_hints, p.cut_base, p.tau_mode, p.zero_in_blend, p.zero_touched,
                          p.keep_untouched, p.clip, p.want_shd, p.spec_eligible, p.adaptive_sort, p.assume_short, p.cut_pays, p.cut };
    int v = 0;
    for (size_t k = 0; k < sizeof bits / sizeof bits[0]; k++) v |= bits[k] ? 1 << k : 0;
    return v;
}

int gsrast_debug_backward_plan(const gsrast_options* options, unsigned flags, const int* words, int* grids)
{
    if (!options || !words) return fail(GSRAST_E_ARG, "debug_backward_plan: NULL argument");
    const int in = words[5];
    BackwardInputs bi{ flags, words[0], words[1], words[2], words[3], words[4], (in & 1) != 0, (in & 2) != 0, (in & 4) != 0, (in & 8) != 0, (in & 16) != 0 };
    bi.known_flags = backward_known_flags((in & 32) ? sizeof(gsrast_backward_call) : GSRAST_BACKWARD_CALL_MIN);
    bi.pose_out = (in & 64) != 0; bi.pose_scratch = (in & 128) != 0; bi.abs_sink = (in & 256) != 0;
    BackwardPlan p = plan_backward(*options, bi, snapshot_switches());
    if (p.refusal) return fail(GSRAST_E_ARG, p.refusal);
    p.side_answer(p.wants_side() && words[6] != 0);
    if (grids) { grids[0] = p.derivs_grid; grids[1] = p.per_gaussian_grid; }
    const bool bits[] = { p.aux, p.aa, p.do_blend, p.do_geom, p.zero_records, p.derivs, p.derivs_on_side, p.late_fill_wanted, p.late_fill, p.skip_zero_rows, p.join_late,
                          p.blend, p.pick.cull, p.pick.transposed, p.pick.aux, p.from_buckets, p.tile_order, p.sh_factor, p.factors != 0, p.sparse, p.grouped };
    int v = 0;
    for (size_t k = 0; k < sizeof bits / sizeof bits[0]; k++) v |= bits[k] ? 1 << k : 0;
    return v | p.pick.ppl << 21 | p.pick.ablate << 24 | (p.mutate & 3) << 26 | (p.pose ? 1 << 28 : 0);
}

// A lookup in kOptions, plus the names that are not plain words: "pixels_per_lane" writes both directions and reads the forward's, "word_fork"
// (word forks were removed, DESIGN_LOG.md; bench.py still reads the name) reads 0 and accepts only 0, the context's words are read-only.
int gsrast_set_option(const char* name, int value)
{
    if (!name) return GSRAST_E_ARG;
    if (!strcmp(name, "word_fork")) return value == 0 ? 0 : GSRAST_E_ARG;
    const bool both = !strcmp(name, "pixels_per_lane");
    const OptionRow* r = option_row(both ? "fwd_pixels_per_lane" : name);
    int stored = 0;
    if (!r || !option_take(*r, value, &stored)) return GSRAST_E_ARG;
    r->word->store(stored);
    if (both) g_opt.bwd_pixels_per_lane = stored;
    return 0;
}
int gsrast_get_option(const char* name)
{
    if (!name) return GSRAST_E_ARG;
    if (!strcmp(name, "word_fork")) return 0;
    for (const char* word : { "last_instances", "last_runs", "redo_count", "bucket_skip" }) if (!strcmp(name, word)) return gsrast_context_query(nullptr, name);
    const OptionRow* r = option_row(!strcmp(name, "pixels_per_lane") ? "fwd_pixels_per_lane" : name);
    return r ? r->word->load() : GSRAST_E_ARG;
}

int gsrast_profile_kernel_count(void) { return K_COUNT; }
const char* gsrast_profile_kernel_name(int id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : ""; }
int gsrast_profile_collect(void)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& p : g_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            g_total_ms[p.id] += ms; g_launches[p.id] += 1;
        }
        (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b);
    }
    g_pending.clear();
    return 0;
}
int gsrast_profile_read(int id, double* total_ms, long long* launches)
{
    if (id < 0 || id >= K_COUNT) return GSRAST_E_ARG;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (total_ms) *total_ms = g_total_ms[id];
    if (launches) *launches = g_launches[id];
    return 0;
}
void gsrast_profile_reset(void)
{
    gsrast_profile_collect();
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < K_COUNT; i++) { g_total_ms[i] = 0; g_launches[i] = 0; }
}

size_t gsrast_geometry_bytes(int P) { return geom_layout((size_t)(P > 0 ? P : 0)).total; }
size_t gsrast_binning_bytes(int R, int, int) { return bin_layout((size_t)(R > 0 ? R : 0)).total; }
size_t gsrast_image_bytes(int W, int H) { return img_layout((size_t)(W > 0 ? W : 0), (size_t)(H > 0 ? H : 0)).total; }
void* gsrast_alloc_prealloc(void* ctx, size_t bytes)
{
    gsrast_prealloc* p = static_cast<gsrast_prealloc*>(ctx);
    if (!p) return nullptr;
    p->requested = bytes;
    return bytes <= p->capacity ? p->ptr : nullptr;
}

int gsrast_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                        unsigned char* present, void* stream)
{
    (void)projmatrix;
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail(GSRAST_E_ARG, "mark_visible: NULL argument");
    if (P == 0) return GSRAST_OK;
    ProfScope ps(K_MARK_VISIBLE, s);
    mark_visible_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, means3D, viewmatrix, present);
    GS_LAUNCHED("mark_visible");
    return GSRAST_OK;
}

static int prefilter_verdict(const uint32_t* word, hipStream_t s)
{
    uint32_t v = 0;
    GS_HIP(hipMemcpyAsync(&v, word, sizeof v, hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    return v ? fail(GSRAST_E_ARG, "forward: a Gaussian passed as prefiltered was culled by the near plane (the reference traps: auxiliary.h:156-160)") : GSRAST_OK;
}

static const char* raw_inputs_check(int P, int M, const gsrast_raw_inputs* in)
{
    if (!in) return "raw: NULL inputs";
    if (P == 0) return nullptr;
    if (!in->xyz || !in->rotation || !in->scaling || !in->opacity_logit || !in->features_dc || (M > 1 && !in->features_rest)) return "raw: NULL required input";
    if (M < 1 || M * 3 > PP_SH_MAX || ((M * 3) & 3)) return "raw: M must be 4 or 16 (SH rows of a multiple of 16 bytes, at most 16 coefficients)";
    if (((uintptr_t)in->rotation | (uintptr_t)in->features_dc | (uintptr_t)in->features_rest | (uintptr_t)in->shs_res) & 15) return "raw: rotation / features_dc / features_rest / shs_res must be 16-byte aligned";
    return nullptr;
}

extern "C++" { namespace {      // (C++ linkage: a member template lives here)
// ---- the two binning kernels with long argument lists: one record each, filled by name, the positional list written once ----
struct BucketSortArgs {      // depth_bucket_sort_kernel
    const uint4* slab; const uint32_t* gcount; uint32_t nb; const uint32_t* bkey; uint32_t *border, *bwincl; uint4* binfo; uint32_t* bwsum;
    uint4* binfo_all = nullptr;                                                        // list cut, early-only mode: the totals over ALL Gaussians
    const uint32_t* pred = nullptr; const unsigned long long* keep_bits = nullptr;     // completion pass: its predicate, the candidates
    uint32_t* zero_words = nullptr; uint32_t n_zero_words = 0; uint4* zero_quads = nullptr; uint32_t n_zero_quads = 0;   // the context's tables, zeroed for its next forward
};
void launch_bucket_sort(hipStream_t s, const BucketSortArgs& a)
{
    depth_bucket_sort_kernel<<<(a.nb + BK_WAVES - 1) / BK_WAVES, 64 * BK_WAVES, 0, s>>>(a.slab, a.gcount, a.nb, a.bkey, a.border, a.bwincl, a.binfo, a.bwsum, a.binfo_all, a.pred, a.keep_bits,
                                                                                   a.zero_words, a.n_zero_words, a.zero_quads, a.n_zero_quads);
}
struct EmitArgs {            // emit_column_runs_kernel
    uint32_t grid; int P; const uint32_t *order, *woffsets; const float4* binrec; int W, H, clip; uint32_t capQ; uint16_t* run_keys; uint2* run_vals;
    const float4 *rec0, *rec1; const uint2* rect;
    const uint4* binfo = nullptr; const uint32_t* bwsum = nullptr; uint32_t nbuckets = 0;      // bucket depth sort: one workgroup per bucket
    uint32_t* scalars = nullptr; uint32_t* host_out = nullptr; uint32_t host_seq = 0;           // the totals, on the device and in pinned host memory
    const uint4* binfo_all = nullptr; const uint32_t* pred = nullptr;                           // list cut: the set over all Gaussians; the completion pass's predicate
    uint32_t* redo_bucket_cnt = nullptr; int n_redo_cnt = 0; HintTable* redo_hints = nullptr; unsigned long long* host_fallback = nullptr; uint32_t host_fb_seq = 0;
    const unsigned char* need2 = nullptr; int gx_tiles = 0; uint32_t* pass2_counts = nullptr;   // completion pass: the tiles listed again
};
void launch_emit(hipStream_t s, const EmitArgs& a)
{
    emit_column_runs_kernel<<<a.grid, 256, 0, s>>>(a.P, a.order, a.woffsets, a.binrec, a.W, a.H, a.clip, a.capQ, a.run_keys, a.run_vals, a.binfo, a.bwsum, a.nbuckets, a.scalars,
                                               a.host_out, a.host_seq, a.binfo_all, a.pred, a.redo_bucket_cnt, a.n_redo_cnt, a.redo_hints, a.host_fallback, a.host_fb_seq,
                                               a.need2, a.gx_tiles, a.pass2_counts, a.rec0, a.rec1, a.rect);
}
bool trace_on() { static const bool on = getenv("GSRAST_TRACE") != nullptr; return on; }

// One forward call's state and its stages (forward_impl below is the order they run in).  Every stage that launches is told its stream
// -- `stream` is the caller's and is never re-aimed -- and, where it has one, its predicate word.
// c: the call's record (include/gsrast.h: gsrast_forward_call).  Raw family: `raw` replaces the dense inputs (which are null), prefiltered is 0.
struct ForwardRun {
    gsrast_context* const ctx; const gsrast_forward_call& c; const gsrast_options o; const std::chrono::steady_clock::time_point t_entry; const hipStream_t stream;
    const int device; DeviceState* const dev;      // the calling thread's device (current_device(); indexes t_readback) and the context's record on it; -1 / nullptr: none
    ForwardPlan plan;
    const float *means3D, *shs, *opacities, *scales, *rotations;      // as the kernels see them (raw family: the model's leaves)
    const gsrast_raw_inputs* rawin = nullptr; RawArgs raw{};
    float *out_acc_depth = nullptr, *out_alpha = nullptr;
    int P = 0, W = 0, H = 0; uint32_t T = 0, nbk = 0; CamArgs cam;
    // the three state buffers and their typed pointers, resolved once
    GeomLayout GL; ImgLayout IL; char *geom = nullptr, *img = nullptr, *bin = nullptr; uint32_t cap = 0, capQ = 0;
    float4 *rec0, *rec1, *rec2, *binrec, *grec; uint32_t* tiles; uint2* rect; uint32_t *kA, *kB, *vA, *vB, *offsets, *woffsets, *hist, *scan_tmp, *scalars, *hint_sel, *prefilter_word;
    uint4 *bk_slab, *bk_info, *bk_info_e; uint32_t *bk_count, *bk_key, *bk_order, *bk_wincl, *bk_base, *bk_order_e, *bk_wincl_e, *bk_base_e;
    unsigned long long *color_skip, *cand_bits; unsigned char *untouched = nullptr, *tile_flags; uint32_t* bucket_cnt; uint16_t* bucket_list; uint2* ranges;
    uint32_t *zcut_used = nullptr, *tau_hist = nullptr, *zhist_call = nullptr; TauBins tau_bins{};
    HintTable* hints = nullptr;
    uint32_t zh_klo = 0, zh_wave_mask = 0; int zh_shift = 0;      // equalised depth buckets: the histogram's bins (range hint of this context), the sampled waves
    uint32_t *zhist_ctx = nullptr, *tau_ctx = nullptr;             // non-null: the depth histogram / the opacity-mass table this call fills is the context's (DeviceState), zeroed again by the bucket sort
    // Every exit after the fork must order the caller's stream behind the side stream: the colour kernel and the zero-fill write
    // into the geometry buffer, which the caller is free to release (on its stream) as soon as this function has returned -- an error
    // return (allocation failure, overflow, a failed launch) included: those drain the side stream.  The normal path enqueues the
    // two waits itself (in front of / behind the blend) and disarms the guard.
    struct SideJoinGuard {
        SideStream* side = nullptr; bool launched = false /* the colour kernel is enqueued */, joined = false;
        ~SideJoinGuard() { if (launched && side && !joined) (void)hipStreamSynchronize(side->stream); }    // error path: cost is irrelevant
    } fork;
    bool bucketed = false;          // the order in force comes from the bucket sort (per-bucket slot ranges) rather than vA
    bool totals_pending = false;    // ... and nobody has summed the buckets' totals (R, Q, overflow verdict) into `scalars` yet
    bool sort_redone = false;
    // read-back handles: the pose-found word (RB_FOUND), the counts by the emission's own store (flag) or by a copy (rb)
    Readback *rb_pre = nullptr, *rb_flag = nullptr, *rb = nullptr; uint32_t *pre_alias = nullptr, *flag_alias = nullptr; uint32_t pre_seq = 0, flag_seq = 0;
    // the completion pass's gate (ChainGate): claimed when the cut forward's blend is launched -- its last workgroup is the gate
    ChainGate* gate = nullptr; uint32_t gseq = 0, *gdone = nullptr, *gpred = nullptr;
    // the host's copy of the count block's first words, indexed by their names (gsrast_common.h: SC_R_LO ... SC_BUCKET_OVER)
    uint32_t counts[kCountWords] = { 0 }; uint32_t nQ1 = 0;
    std::chrono::steady_clock::time_point t0, t1;

    ForwardRun(gsrast_context* ctx_, const gsrast_options* options, const gsrast_forward_call& c_, std::chrono::steady_clock::time_point t)
        : ctx(ctx_ ? ctx_ : thread_context()), c(c_), o(options ? *options : snapshot_defaults()), t_entry(t), stream((hipStream_t)c_.stream),
          device(current_device()), dev(ctx->device_state(device)), means3D(c_.means3D), shs(c_.shs), opacities(c_.opacities), scales(c_.scales), rotations(c_.rotations) {}

    // ---- the plan, and the checks every entry point shares (before any device work or allocator callback) ----
    int check_and_plan(hipStream_t s)
    {
        P = c.P; W = c.width; H = c.height;
        const bool raw_family = c.family == GSRAST_FAMILY_RAW;
        plan = plan_forward(o, PlanInputs{ c.flags, P, W, H, c.D, (raw_family ? c.raw && c.raw->features_dc : c.shs != nullptr), c.colors_precomp != nullptr,
                                           ctx->zsort.skip.load(), ctx->R_hint.load(), ctx->last_Q.load(), ctx->zsort.depth_short.load() != 0 }, snapshot_switches());
        if (plan.refusal) return fail(GSRAST_E_ARG, plan.refusal);
        if (plan.aux) { out_acc_depth = c.out_acc_depth; out_alpha = c.out_alpha; }
        if (plan.aux && (!out_acc_depth || !out_alpha)) return fail(GSRAST_E_ARG, "forward: NULL acc_depth / alpha output");
        if (raw_family) {
            rawin = c.raw;
            if (const char* e = raw_inputs_check(P, c.M, rawin)) return fail(GSRAST_E_ARG, e);
            means3D = rawin->xyz; shs = rawin->features_dc /* "there are SH coefficients" */; opacities = rawin->opacity_logit; scales = rawin->scaling; rotations = rawin->rotation;
            raw.motion_res = rawin->motion_res; raw.rot_res = rawin->rot_res; raw.trbf = rawin->trbf; raw.opacity_logit = rawin->opacity_logit;
            raw.features_dc = rawin->features_dc; raw.features_rest = rawin->features_rest; raw.shs_res = rawin->shs_res;
        }
        if (P < 0 || W <= 0 || H <= 0 || c.D < 0 || c.D > 3) return fail(GSRAST_E_ARG, "forward: bad P / image size / SH degree");
        if (!c.geometry_alloc || !c.binning_alloc || !c.image_alloc) return fail(GSRAST_E_ARG, "forward: NULL allocator");
        if (!c.out_color || !c.out_depth || !c.background) return fail(GSRAST_E_ARG, "forward: NULL output / background");
        const size_t N = (size_t)W * H;
        if (P == 0) { // reference rasterize_points.cu:81 -- nothing is rendered, outputs stay zero
            GS_HIP(hipMemsetAsync(c.out_color, 0, 3 * N * sizeof(float), s));
            GS_HIP(hipMemsetAsync(c.out_depth, 0, N * sizeof(float), s));
            if (plan.aux) { GS_HIP(hipMemsetAsync(out_acc_depth, 0, N * sizeof(float), s)); GS_HIP(hipMemsetAsync(out_alpha, 0, N * sizeof(float), s)); }
            return 0;
        }
        if (!means3D || !opacities || !c.viewmatrix || !c.projmatrix || !c.radii) return fail(GSRAST_E_ARG, "forward: NULL required input");
        if (!shs && !c.colors_precomp) return fail(GSRAST_E_ARG, "forward: need shs or colors_precomp");
        if (!c.cov3D_precomp && (!scales || !rotations)) return fail(GSRAST_E_ARG, "forward: need scales+rotations or cov3D_precomp");
        if (shs && !c.colors_precomp && (!c.cam_pos || c.M < (c.D + 1) * (c.D + 1))) return fail(GSRAST_E_ARG, "forward: SH path needs campos and M >= (D+1)^2");
        return GSRAST_OK;
    }

    // ---- the geometry and image buffers (allocator callbacks), their typed pointers, the side stream ----
    int buffers(hipStream_t s)
    {
        cam = make_cam(c.viewmatrix, c.projmatrix, c.cam_pos, c.tan_fovx, c.tan_fovy, c.scale_modifier, W, H);
        T = plan.T;
        GL = geom_layout((size_t)P);
        geom = (char*)c.geometry_alloc(c.geometry_ctx, GL.total);
        if (!geom) return fail(GSRAST_E_ALLOC, "forward: geometry allocation failed");
        IL = img_layout((size_t)W, (size_t)H);
        img = (char*)c.image_alloc(c.image_ctx, IL.total);
        if (!img) return fail(GSRAST_E_ALLOC, "forward: image allocation failed");
        rec0 = at<float4>(geom, GL.rec0); rec1 = at<float4>(geom, GL.rec1); rec2 = at<float4>(geom, GL.rec2); grec = at<float4>(geom, GL.grec);
        tiles = at<uint32_t>(geom, GL.tiles); rect = at<uint2>(geom, GL.rect);
        kA = at<uint32_t>(geom, GL.keyA); kB = at<uint32_t>(geom, GL.keyB); vA = at<uint32_t>(geom, GL.valA); vB = at<uint32_t>(geom, GL.valB);
        offsets = at<uint32_t>(geom, GL.offsets); woffsets = at<uint32_t>(geom, GL.woffsets); hist = at<uint32_t>(geom, GL.hist); scan_tmp = at<uint32_t>(geom, GL.scan_tmp);
        scalars = at<uint32_t>(geom, GL.scalars); hint_sel = scalars + HINT_SEL;
        bk_slab = at<uint4>(geom, GL.bk_slab); bk_info = at<uint4>(geom, GL.bk_info); bk_info_e = at<uint4>(geom, GL.bk_info_e);
        bk_count = at<uint32_t>(geom, GL.bk_count); bk_key = at<uint32_t>(geom, GL.bk_key);
        bk_order = at<uint32_t>(geom, GL.bk_order); bk_wincl = at<uint32_t>(geom, GL.bk_wincl); bk_base = at<uint32_t>(geom, GL.bk_base);
        bk_order_e = at<uint32_t>(geom, GL.bk_order_e); bk_wincl_e = at<uint32_t>(geom, GL.bk_wincl_e); bk_base_e = at<uint32_t>(geom, GL.bk_base_e);
        color_skip = at<unsigned long long>(geom, GL.color_skip); cand_bits = at<unsigned long long>(geom, GL.cand_bits);
        tile_flags = at<unsigned char>(img, IL.tile_flags); bucket_cnt = at<uint32_t>(img, IL.bucket_cnt); bucket_list = at<uint16_t>(img, IL.bucket_list);
        ranges = at<uint2>(img, IL.ranges);
        // `prefiltered` is the caller's promise that no Gaussian will be culled by the near plane; the reference prints and traps when one is
        // (auxiliary.h:156-160).  Here preprocess_fwd raises a word and this call returns GSRAST_E_ARG after it has waited for the device
        // (SaRO-GS always passes False, renderer/__init__.py:63: the promise costs a synchronisation, nobody makes it on a hot path).
        prefilter_word = c.prefiltered ? scalars + SC_PREFILTER : nullptr;
        if (prefilter_word) GS_HIP(hipMemsetAsync(prefilter_word, 0, sizeof(uint32_t), s));
        nbk = depth_buckets_host((size_t)P);
        // equalised depth buckets: which waves of preprocess_fwd are sampled (512-1024 of them)
        zh_klo = ctx->zrange.klo.load(); zh_shift = ctx->zrange.shift.load();
        while ((((size_t)P + 63) / 64) / ((size_t)zh_wave_mask + 1) > 1024) zh_wave_mask = 2u * zh_wave_mask + 1u;
        // Colour half of the per-Gaussian forward (SH -> RGB: most of its bytes) on the context's side stream, forked off the
        // caller's stream behind the depth sort and joined in front of the blend: it overlaps the binning.
        // Where it forks matters little: its 200 MB of traffic stretches whatever latency-bound kernel runs beside it by about as much as
        // it hides (measured: beside the geometry kernel + depth sort +55 us, beside the run emission + run sort +45 / +65 us, beside the
        // LDS-bound run_scatter_rows it starves itself and delays the blend) -- round 2 forked it at entry, the best of those by ~20 us.
        // The 64 B / Gaussian zero-fill of the backward's gradient records follows on the side stream, under the VALU-bound forward blend.
        if (o.side_stream && dev) fork.side = dev->side_stream(ctx->mu);
        return GSRAST_OK;
    }

    // ---- the pose table, the policy's answer, the plan's second phase ----
    // List cut (gsrast_common.h): whether THIS pose has cut depths is decided on the device; whether the cut pays, by CutPolicy (gsrast_policy.h).
    int begin_policy(hipStream_t s)
    {
        // launch-order hints of the forward blend: per context, device and camera pose (gsrast_common.h)
        hints = plan.want_hints && dev ? dev->hint_table(ctx->mu, T, s) : nullptr;
        CutPolicy& pol = ctx->pol;          // (the decisions: gsrast_policy.h)
        if (pol.begin_forward((uint32_t)P)) {     // (what was learned belongs to the scene it was learned on: a context that moves on to a scene of another size starts afresh)
            // keys, stamps, clock: every slot free again, ordered in front of this call's lookup -- of EVERY image size's table of this device (round 6,
            // the other resolutions' tables kept the old scene's cut depths, running maxima that take eight visits to fade)
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (hints)      // (a table was handed out: there is a record)
                for (auto& h : dev->hints) if (h.table) GS_HIP(hipMemsetAsync(h.table, 0, sizeof(HintTable) /* everything in front of work[] */, s));
            ctx->pose_seen.clear(); ctx->Qe_hint = 0; ctx->Qe_hint_tau = 0;
        }
        // The cut does not need the pose table.  With remembered cut depths (a pose the table knows) the first pass lists what lies in front
        // of them; WITHOUT -- a first-seen pose, the table switched off -- it lists what lies in front of PREDICTED ones (tau_cut_kernel), and
        // the completion pass behind the blend lists the rest into the tiles that did not saturate.  Either way the result is exact, and a
        // pause (the passes did not pay) stops both.
        plan.policy_answer(pol.pays(plan.last_Q, plan.list_cut_always), hints != nullptr);
        // the 32-byte binning records (everything the run emission needs of a Gaussian in one line) are written where the emission gathers
        // EVERY visible Gaussian; under the list cut it gathers one in eight, from the blend's records, and preprocess_fwd writes 96 MB less at 3 M
        binrec = plan.cut ? nullptr : at<float4>(geom, GL.binrec);
        if (!plan.cut && !o.no_list_cut) pol.sits_out();
        const bool forced = plan.cut && plan.tau_mode && pol.forced_prediction();
        bool pose_expected = false;         // (see gsrast_context::pose_seen)
        if (plan.cut && plan.tau_mode && hints && !forced) { std::lock_guard<std::mutex> lk(ctx->mu); auto it = ctx->pose_seen.find(c.viewmatrix); pose_expected = it != ctx->pose_seen.end() && it->second != 0; }
        plan.prediction_answer(forced, pose_expected);
        tau_hist = plan.tau_on ? at<uint32_t>(img, IL.tau_hist) : nullptr;
        tau_bins = TauBins{0u, 0.0f, 0.0f, plan.tau_sample_mask};      // (scale 0: the context has not learned a depth range yet -- no prediction in this call)
        {   const uint32_t klo = ctx->zrange.klo.load(), khi = ctx->zrange.khi.load();
            if (plan.tau_on && khi > klo + (uint32_t)TAU_BINS) { tau_bins.lo = klo; tau_bins.scale = (float)TAU_BINS / (float)(khi - klo); tau_bins.inv_scale = (float)(khi - klo) / (float)TAU_BINS; } }
        zcut_used = plan.cut ? at<uint32_t>(img, IL.zcut_used) : nullptr;
        untouched = plan.keep_untouched ? at<unsigned char>(geom, GL.untouched) : nullptr;
        // list cut: the device says at once whether the pose has a slot in the table (RB_FOUND); the launches over the cut lists of a pose
        // that has none -- everything is early -- are sized for all column runs, not for the early runs of recent forwards (a launch
        // that turned out too small cost a first-seen pose a whole second forward: 1.35 instead of 1.05 ms forward-only at 3 M)
        if (plan.cut) rb_pre = read_flag_prepare(device, &pre_alias, &pre_seq);
        return GSRAST_OK;
    }

    // ---- the geometry half of the per-Gaussian forward, and the predicted cut depths ----
    int preprocess(hipStream_t s)
    {
        ProfScope ps(K_PREPROCESS_FWD, s);
        const int pf_grid = (P + PF_THREADS - 1) / PF_THREADS;
        float* cov_dbg = plan.debug_state ? at<float>(geom, GL.cov3D) : nullptr;     // 24 B / Gaussian nobody but gsrast_debug_export reads
        if (plan.bucket_sort) {      // the context's depth histogram on this device, zeroed again by the bucket sort (no memset launch per forward)
            zhist_call = zhist_ctx = dev ? dev->depth_hist(ctx->mu) : nullptr;
            if (!zhist_call) {      // (no context memory to be had: the call's own table and a memset, as before)
                zhist_call = at<uint32_t>(geom, GL.zhist);
                GS_HIP(hipMemsetAsync(zhist_call, 0, ZH_COPIES * ZH_BINS * sizeof(uint32_t), s));
            }
        }
        if (tau_hist) {      // the context's opacity-mass table where the bucket sort will zero it again behind tau_cut_kernel; else the call's own and a memset
            const size_t words = (size_t)TAU_COPIES * T * TAU_BINS;
            if (plan.bucket_sort && zhist_ctx && !plan.debug_state /* (diagnostics read the table back from the image buffer: tools/tau_debug.py) */ && (words & 3) == 0 && words / 4 <= 0xFFFFFFFFull)
                tau_ctx = dev->mass_table(ctx->mu, words, s);
            if (tau_ctx) tau_hist = tau_ctx; else GS_HIP(hipMemsetAsync(tau_hist, 0, words * sizeof(uint32_t), s));
        }
        const int nzero = plan.bucket_sort ? (int)nbk * BK_XCD + BK_XCD * BK_NBC_MAX : 0;      // (fine counters + the two-launch scatter's coarse ones, contiguous)
        unsigned long long* host_found = rb_pre ? reinterpret_cast<unsigned long long*>(pre_alias) + RB_FOUND : nullptr;
        pick_bool(rawin != nullptr, [&](auto raw_c) { pick_bool(plan.aa, [&](auto aa_c) {       // <RAW, AA>
            preprocess_fwd_kernel<decltype(raw_c)::value, decltype(aa_c)::value><<<pf_grid, PF_THREADS, 0, s>>>(
                P, means3D, scales, rotations, opacities, raw, c.cov3D_precomp, cam, c.radii, rec0, rec1, cov_dbg,
                tiles, rect, binrec, kA, plan.bucket_sort ? nullptr : vA, plan.clip ? 1 : 0, bucket_cnt, zhist_call, zh_klo, zh_shift, zh_wave_mask, bk_count, nzero, hints, hint_sel,
                zcut_used, T, scalars, host_found, pre_seq, prefilter_word, untouched, tau_hist, tau_bins);
        }); });
        GS_LAUNCHED("preprocess_fwd");
        ctx->last_prologue_ns = (uint32_t)std::min<long long>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_entry).count(), 0xFFFFFFFFll);
        if (tau_hist) {       // the predicted cut depths of a pose without remembered ones (a no-op for a pose the table knows, unless forced)
            const dim3 tg((unsigned)((cam.gx + TAU_TILE - 1) / TAU_TILE), (unsigned)((cam.gy + TAU_TILE - 1) / TAU_TILE));
            tau_cut_kernel<<<tg, TAU_BLK * TAU_BLK, 0, s>>>(tau_hist, T, cam.gx, cam.gy, tau_bins, (uint32_t)ctx->pol.tau_req.load() * 256u, hints ? hint_sel : nullptr, plan.tau_forced ? 1 : 0,
                                              zcut_used, tau_bins.scale > 0.0f ? 0 : 1);
            GS_LAUNCHED("tau_cut");
        }
        return GSRAST_OK;
    }

    BucketSortArgs whole_buckets() const { return BucketSortArgs{ bk_slab, bk_count, nbk, bk_key, bk_order, bk_wincl, bk_info, bk_base }; }
    // ---- depth order of the Gaussians: the bucket sort (gsrast_binning.h), or the radix passes and the scan of the widths ----
    int sort_and_scan(hipStream_t s, bool assume, bool buckets)
    {
        bucketed = buckets; totals_pending = false;
        if (buckets) {      // three launches instead of the radix passes and the scan
            ProfScope ps(K_SORT_DEPTH, s);
            const int items = depth_scatter_items((size_t)P);       // (elements per lane: whatever makes the launch ONE round of workgroups)
            // two-launch form (gsrast_binning.h, round 6; from two_level_min_p Gaussians on): coarse scatter, then the refine kernel
            const bool two = plan.two_level;
            auto scatter = two ? (items == BK_ITEMS_WIDE ? depth_bucket_scatter_kernel<BK_ITEMS_WIDE, true> : depth_bucket_scatter_kernel<BK_ITEMS, true>)
                               : (items == BK_ITEMS_WIDE ? depth_bucket_scatter_kernel<BK_ITEMS_WIDE, false> : depth_bucket_scatter_kernel<BK_ITEMS, false>);
            // (the coarse slab: the gradient records' memory -- 64 B per Gaussian, nobody's until this forward's last blend; whoever zeroes or reads the records does so behind it)
            uint4* cslab = reinterpret_cast<uint4*>(grec);
            const uint32_t ccap = depth_coarse_cap((size_t)P, nbk);
            uint32_t* gccount = at<uint32_t>(geom, GL.bk_ccount);
            scatter<<<(P + 256 * items - 1) / (256 * items), 256, 0, s>>>(kA, rect, tiles, (uint32_t)P, zhist_call, zh_klo, zh_shift, nbk, two ? gccount : bk_count, two ? cslab : bk_slab, bk_key, scalars + SC_ZBINS,
                                                                           zcut_used, T, (uint32_t)cam.gx, scalars + SC_N_LATE, plan.cut ? color_skip : nullptr, (uint32_t)plan.cut_cs, ccap);
            GS_LAUNCHED("depth_bucket_scatter");
            if (two) {
                depth_bucket_refine_kernel<<<(nbk >> BK_CSHIFT) * BK_XCD, 256, 0, s>>>(cslab, gccount, nbk, bk_count, bk_slab, ccap);
                GS_LAUNCHED("depth_bucket_refine");
            }
            // list cut: only the bucket's EARLY Gaussians are sorted (into the early set); the late ones count into bk_info's totals
            BucketSortArgs a = whole_buckets();
            if (plan.cut) { a.border = bk_order_e; a.bwincl = bk_wincl_e; a.binfo = bk_info_e; a.bwsum = bk_base_e; a.binfo_all = bk_info; }
            a.zero_words = zhist_ctx; a.n_zero_words = ZH_COPIES * ZH_BINS;
            if (tau_ctx) { a.zero_quads = reinterpret_cast<uint4*>(tau_ctx); a.n_zero_quads = (uint32_t)((size_t)TAU_COPIES * T * TAU_BINS / 4); }
            launch_bucket_sort(s, a);
            GS_LAUNCHED("depth_bucket_sort");
            if (a.zero_quads) { std::lock_guard<std::mutex> lk(ctx->mu); dev->tau_dirty = false; }
            totals_pending = true;      // by the run emission's last workgroup, or by depth_bucket_scan_kernel if the host needs them first
            return GSRAST_OK;
        }
        {   ProfScope ps(K_SORT_DEPTH, s);      // (the radix-sorted sequence ends in (kA, vA) under every pass count)
            if (plan.bucket_sort) {      // the geometry kernel left the values to the bucket sort (which overflowed): the identity, now
                iota_kernel<<<(P + 255) / 256, 256, 0, s>>>(vA, (uint32_t)P);
                GS_LAUNCHED("iota");
            }
            // the last pass also writes rectangle widths (and, for the instance-level binning, tile counts) in depth order
            const SortAdapt<uint32_t, uint32_t> ad{ at<uint32_t>(geom, GL.keyC), at<uint32_t>(geom, GL.valC), at<uint32_t>(geom, GL.sort_minmax), scalars + SC_SIG, assume };
            int rc = radix_sort<uint32_t, uint32_t, GSRAST_DEPTH_ITEMS>(kA, vA, kB, vB, (uint32_t)P, 32, hist, scan_tmp, s, rect, plan.runbin ? nullptr : offsets, woffsets, nullptr, &ad);
            if (rc != GSRAST_OK) return rc;
        }
        ProfScope ps(K_SCAN_TILES, s);
        if (plan.runbin)   // only the widths are scanned (-> run offsets, Q); num_rendered is just the sum of the tile counts
            return scan_u32(woffsets, nullptr, (uint32_t)P, woffsets, true, scan_tmp, scalars + SC_Q, s, nullptr, tiles, scalars + SC_R_LO, scalars + SC_R_HI);
        int rc = scan_u32(offsets, nullptr, (uint32_t)P, offsets, true, scan_tmp, scalars + SC_R_LO, s);
        if (rc != GSRAST_OK) return rc;
        return scan_u32(woffsets, nullptr, (uint32_t)P, woffsets, true, scan_tmp, scalars + SC_Q, s);   // column runs
    }

    // ---- plan, second phase: the device's word on the pose (written at the very start of preprocess_fwd, long before this point) ----
    void learn_pose()
    {
        plan.pose_answer(!(plan.cut && rb_pre && hints) || read_found(rb_pre));
        if (plan.cut && plan.tau_mode && hints && rb_pre) {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (ctx->pose_seen.size() > 4096) ctx->pose_seen.clear();
            ctx->pose_seen[c.viewmatrix] = plan.pose_known ? 1 : 0;
        }
    }
    size_t bin_bytes() const { return plan.runbin ? runbin_layout((size_t)cap, (size_t)capQ).total : bin_layout((size_t)cap).total; }
    // ---- the binning buffer of the speculative launch: requested for 1.25 x the hints BEFORE the host knows the counts ----
    int speculative_buffer(hipStream_t s)
    {
        // reference rasterizer_impl.cu:311 (the run-compressed path writes every tile's range itself, empty ones included)
        if (!plan.runbin) GS_HIP(hipMemsetAsync(ranges, 0, (size_t)T * sizeof(uint2), s));
        t0 = std::chrono::steady_clock::now();
        if (plan.R_hint) {
            cap = grow_capacity(plan.R_hint); capQ = grow_capacity(ctx->Q_hint.load());
            bin = (char*)c.binning_alloc(c.binning_ctx, bin_bytes());
            if (!bin) cap = capQ = 0;
        }
        t1 = std::chrono::steady_clock::now();
        plan.binning_answer(bin != nullptr);
        return GSRAST_OK;
    }

    // ---- the colour half.  List cut: early_only = only the Gaussians the bucket scatter did not mark culled or late (the compacting
    // kernel: a Gaussian found late is in no list, its colour is not evaluated -- 3 M cube: 87 % of them); pred = the predicated launch ----
    int color_kernels(hipStream_t cs, bool early_only, const uint32_t* pred)
    {
        ProfScope ps(K_COLOR, cs);
        const float* const colors_precomp = c.colors_precomp; const float* const cam_pos = c.cam_pos; const int D = c.D, M = c.M;
        // d(colour)/d(view direction) for the backward (36 B / Gaussian), unless the caller said that no backward will follow
        float4 *sA = plan.want_shd ? at<float4>(geom, GL.shdA) : nullptr, *sB = plan.want_shd ? at<float4>(geom, GL.shdB) : nullptr; float* sC = plan.want_shd ? at<float>(geom, GL.shdC) : nullptr;
        const float* sh_in = colors_precomp ? nullptr : shs;
        unsigned char* cl = at<unsigned char>(geom, GL.clamped);
        float4* gz = (fork.side || plan.zero_in_blend) ? nullptr : grec;
        const bool staged = sh_in && M * 3 <= PP_SH_MAX && ((M * 3) & 3) == 0 && ((uintptr_t)sh_in & 15) == 0;
        const int grid = (P + PP_THREADS - 1) / PP_THREADS;
        if (early_only) {       // list cut: Gaussians the bucket scatter found culled or late are skipped (gsrast_preprocess.h)
            // (with `pred`: the completion pass -- the colours of the late Gaussians that are listed after all, GeomLayout::skip2)
            const unsigned char* skip = at<unsigned char>(geom, pred ? GL.skip2 : GL.color_skip);
            const int cgrid = (P + PCC_IDS - 1) / PCC_IDS;
            if (rawin) preprocess_color_compact_kernel<true><<<cgrid, 64 * PCC_WAVES, 0, cs>>>(P, D, M, means3D, nullptr, nullptr, raw, cam_pos, rec2, cl, sA, sB, sC, skip, pred);
            else preprocess_color_compact_kernel<false><<<cgrid, 64 * PCC_WAVES, 0, cs>>>(P, D, M, means3D, sh_in, colors_precomp, raw, cam_pos, rec2, cl, sA, sB, sC, skip, pred);
        } else if (rawin) {        // (raw_inputs_check has checked M and the alignment of the three SH arrays)
            if (M * 3 == PP_SH_MAX) preprocess_color_kernel<PP_SH_MAX, true><<<grid, PP_THREADS, 0, cs>>>(P, D, M, means3D, nullptr, raw, cam_pos, rec2, cl, gz, sA, sB, sC, pred);
            else preprocess_color_kernel<0, true><<<grid, PP_THREADS, 0, cs>>>(P, D, M, means3D, nullptr, raw, cam_pos, rec2, cl, gz, sA, sB, sC, pred);
        } else if (staged && M * 3 == PP_SH_MAX)
            preprocess_color_kernel<PP_SH_MAX, false><<<grid, PP_THREADS, 0, cs>>>(P, D, M, means3D, sh_in, raw, cam_pos, rec2, cl, gz, sA, sB, sC, pred);
        else if (staged)
            preprocess_color_kernel<0, false><<<grid, PP_THREADS, 0, cs>>>(P, D, M, means3D, sh_in, raw, cam_pos, rec2, cl, gz, sA, sB, sC, pred);
        else
            preprocess_color_direct_kernel<<<(P + 255) / 256, 256, 0, cs>>>(P, D, M, means3D, sh_in, colors_precomp, cam_pos, rec2, cl, gz, sA, sB, sC, pred);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(GSRAST_E_DEVICE, "preprocess_color", e);
        return GSRAST_OK;
    }
    // The colour kernel forks off `s` behind the geometry kernel and the depth sort (round 3; rounds 1-2: at entry): the geometry kernel
    // is as bandwidth-bound as the colours are (running both at once is the sum of their times) and the bucket scatter's returning
    // atomics are what the colour traffic hurts most (70 -> 150 us at 3 M); the gather-bound run emission and the run sort that now
    // run beside it stretch less.  Two alternating runs each, views/s, entry -> here: 3 M 609 -> 619, 2 M 745 -> 753, 1 M 1059 -> 1082,
    // 0.3 M 1504 -> 1551, 0.1 M 1878 -> 1894, shell 1 M 884 -> 917, cfg2 2692 -> 2787.  Behind the geometry kernel only: 3 M -3.8 %
    // (the scatter beside the colours); behind the run emission: 3 M -4 % (the colours end after the binning, the blend waits).
    int launch_color(hipStream_t s)
    {
        if (fork.launched) return GSRAST_OK;
        fork.launched = true;
        SideStream* const side = fork.side;
        if (side) {
            GS_HIP(hipEventRecord(side->fork, s));             // the inputs (and the buffers just handed out) are ordered on s
            GS_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
        }
        { int rc = color_kernels(side ? side->stream : s, plan.cut_colors, nullptr); if (rc != GSRAST_OK) return rc; }
        // The backward's gradient records (64 B / Gaussian) are zero-filled by the forward: inside the default (culling) blend kernel; by a
        // memset behind the colour kernel (side stream) / by the colour kernel itself (no side stream) when another blend kernel runs.
        if (side) {
            GS_HIP(hipEventRecord(side->join, side->stream));
            if (!plan.zero_in_blend) {
                GS_HIP(hipMemsetAsync(grec, 0, (size_t)P * GREC * sizeof(float), side->stream));
                GS_HIP(hipEventRecord(side->join2, side->stream));
            }
        }
        return GSRAST_OK;
    }

    // ---- run-compressed binning on the buffer in force; nQ / cap are either exact counts (counts_dev == nullptr) or capacities with the
    // real counts read on the device (speculative launch: grids and histogram strides follow the capacities) ----
    // mode (list cut): 0 = all Gaussians (as ever); 1 = the EARLY Gaussians only (counts_dev = scalars + SC_EARLY_COUNTS); 2 = all
    // Gaussians again behind a blend over cut lists, every kernel predicated on *pred (counts_dev = scalars + SC_PASS2)
    int run_binning(hipStream_t s, uint32_t nQ, const uint32_t* counts_dev, int mode, const uint32_t* pred, bool readback_after_emit)
    {
        const RunBinLayout RL = runbin_layout((size_t)cap, (size_t)capQ);
        uint16_t *rkA = at<uint16_t>(bin, RL.rkeyA), *rkB = at<uint16_t>(bin, RL.rkeyB);
        uint2 *rvA = at<uint2>(bin, RL.rvalA), *rvB = at<uint2>(bin, RL.rvalB);
        uint32_t *hist_x = at<uint32_t>(bin, RL.hist_x), *hist_y = at<uint32_t>(bin, RL.hist_y), *rscan = at<uint32_t>(bin, RL.scan_tmp), *plist_w = at<uint32_t>(bin, RL.point_list);
        const uint32_t* Q_dev = counts_dev ? counts_dev + SC_Q : nullptr;
        const int xbits = tile_bits((size_t)cam.gx);
        {   ProfScope ps(K_EMIT, s);
            EmitArgs e{};
            e.grid = nbk + 1; e.P = P; e.order = bk_order; e.woffsets = bk_wincl; e.binrec = binrec; e.W = W; e.H = H; e.clip = o.tile_clip; e.capQ = capQ; e.run_keys = rkA; e.run_vals = rvA;
            e.rec0 = rec0; e.rec1 = rec1; e.rect = rect;
            if (bucketed) { e.binfo = bk_info; e.bwsum = bk_base; e.nbuckets = nbk; }
            if (bucketed && mode == 1) {
                e.order = bk_order_e; e.woffsets = bk_wincl_e; e.binfo = bk_info_e; e.bwsum = bk_base_e; e.binfo_all = bk_info;
                e.scalars = scalars; e.host_out = flag_alias; e.host_seq = flag_seq;
            } else if (bucketed && mode == 2) {
                // COMPLETION pass: only the CANDIDATES -- the Gaussians, early or late, whose rectangle touches a tile flagged by the
                // blend -- are sorted (the buckets' non-early arrays are free) and listed, and only into flagged tiles
                BucketSortArgs a = whole_buckets(); a.pred = pred; a.keep_bits = cand_bits;
                launch_bucket_sort(s, a);
                e.pred = pred; e.redo_bucket_cnt = bucket_cnt; e.n_redo_cnt = XCD_GROUPS * WORK_BUCKETS /* (the forward's order only: the backward's keeps the tiles that are final) */; e.redo_hints = hints;
                e.host_fallback = rb_pre ? reinterpret_cast<unsigned long long*>(pre_alias) + RB_FALLBACK : nullptr; e.host_fb_seq = pre_seq;
                e.need2 = tile_flags; e.gx_tiles = cam.gx; e.pass2_counts = scalars + SC_PASS2;
            } else if (bucketed) {
                if (plan.cut) {      // (a list-cut forward sorted the early Gaussians only, and now everything is listed after all: the buckets are sorted again, whole)
                    launch_bucket_sort(s, whole_buckets());
                    GS_LAUNCHED("depth_bucket_sort");
                }
                e.scalars = scalars; e.host_out = flag_alias; e.host_seq = flag_seq;
            } else { e.grid = (uint32_t)((P + 255) / 256); e.order = vA; e.woffsets = woffsets; }
            launch_emit(s, e);
            GS_LAUNCHED("emit_column_runs"); }
        if (bucketed && mode != 2) totals_pending = false;
        if (readback_after_emit) { int rc = read_u32_begin(device, scalars, s, kCountWords, &rb); if (rc != GSRAST_OK) return rc; }
        const uint32_t nblk = (nQ + RUNS_PER_BLOCK - 1) / RUNS_PER_BLOCK;
        ProfScope ps(K_SORT_TILE, s);
        int rc = radix_sort<uint16_t, uint2, GSRAST_RUN_SORT_ITEMS>(rkA, rvA, rkB, rvB, nQ, xbits, hist_x, rscan, s, nullptr, nullptr, nullptr, Q_dev, nullptr, pred);   // runs by column
        if (rc != GSRAST_OK) return rc;
        if (radix_passes(xbits) & 1) { std::swap(rkA, rkB); std::swap(rvA, rvB); }                   // sorted runs now in (rkA, rvA)
        run_hist_rows_kernel<<<nblk, 256, 0, s>>>(rvA, nQ, Q_dev, hist_y, nblk, (uint32_t)cam.gy, pred);
        GS_LAUNCHED("run_hist_rows");
        radix_rowscan_kernel<<<cam.gy, 256, 0, s>>>(hist_y, nblk, rscan, nullptr, 0, nullptr, 0, pred);     // one workgroup per tile row
        GS_LAUNCHED("radix_rowscan");
        // the row pass and the tile ranges in one launch (gsrast_binning.h)
        rows_and_ranges_kernel<<<nblk + (uint32_t)cam.gx, RS_THREADS, 0, s>>>(rkA, rvA, nQ, counts_dev, cap, tile_bits((size_t)cam.gy), cam.gx, cam.gy, hist_y, rscan, nblk,
                                                                             mode == 2 ? plist_w + cap : plist_w, scalars + (mode == 2 ? SC_PASS2 : 0) + SC_LISTED, ranges,
                                                                             plan.buckets_ok ? bucket_cnt : nullptr, bucket_list, hints, hint_sel, pred,
                                                                             mode == 2 ? tile_flags : nullptr, mode == 2 ? cap : 0u,
                                                                             (mode == 1 && plan.tau_on) ? zcut_used : nullptr);
        GS_LAUNCHED("rows_and_ranges");
        return GSRAST_OK;
    }
    // ---- instance-level binning (options.binning = 1, or an image too large for the run-compressed scheme) ----
    // Tile ids fit 16 bits up to 65 536 tiles (4096 x 4096 pixels): the R-sized key streams are then half as wide (the key buffers are
    // sized for 32-bit ids either way).
    template <typename KeyT> int instance_binning(hipStream_t s, uint32_t R)
    {
        const BinLayout BL = bin_layout((size_t)cap);
        uint32_t *tkA = at<uint32_t>(bin, BL.keyA), *tkB = at<uint32_t>(bin, BL.keyB);
        uint32_t *tvA = at<uint32_t>(bin, BL.valA), *tvB = at<uint32_t>(bin, BL.valB);
        if (tile_passes(T) & 1) { std::swap(tkA, tkB); std::swap(tvA, tvB); }   // odd pass count: start in B, finish in A
        KeyT *hA = reinterpret_cast<KeyT*>(tkA), *hB = reinterpret_cast<KeyT*>(tkB);
        { ProfScope ps(K_EMIT, s);
          emit_instances_kernel<KeyT><<<(P + 255) / 256, 256, 0, s>>>(P, vA, offsets, tiles, rect, cam.gx, hA, tvA);
          GS_LAUNCHED("emit_instances"); }
        { ProfScope ps(K_SORT_TILE, s);
          int rc = radix_sort<KeyT>(hA, tvA, hB, tvB, R, tile_bits(T), at<uint32_t>(bin, BL.hist), at<uint32_t>(bin, BL.scan_tmp), s);
          if (rc != GSRAST_OK) return rc; }
        ProfScope ps(K_RANGES, s);
        tile_ranges_kernel<KeyT><<<(R + 255) / 256, 256, 0, s>>>(R, nullptr, reinterpret_cast<const KeyT*>(at<uint32_t>(bin, BL.keyA)), ranges);
        GS_LAUNCHED("tile_ranges");
        return GSRAST_OK;
    }

    // claims the completion pass's gate for the blend about to be launched; without one (gate == nullptr) the pass runs inline
    void claim_gate()
    {
        if (!plan.chain_gate || counter_collection_env() || !dev || (gate = dev->chain_gate(ctx->mu, device)) == nullptr) return;
        std::lock_guard<std::mutex> lk(ctx->mu);
        uint32_t n = gate->seq + 1u; if (n == 0u) n = 1u;
        // the slot of n was last used by n - GATE_RING; it is free once the chain of n - GATE_RING / 2 (enqueued later on the same
        // in-order stream) has run.  Not yet?  Then this call does without the gate (inline chain).
        // (a call that claimed a number but never enqueued a chain recorded no event: the youngest recorded chain among
        // n - GATE_RING / 2 ... n - GATE_RING answers for all older ones)
        bool free_slot = true;
        for (uint32_t back = GATE_RING / 2u; back <= GATE_RING; back++) {
            const uint32_t k = n - back;
            if (k != 0u && gate->tail_seq[k % GATE_RING] == k) { free_slot = hipEventQuery(gate->tail[k % GATE_RING]) == hipSuccess; break; }
        }
        if (!free_slot) { gate->inline_calls++; gate = nullptr; return; }
        gate->seq = n; gseq = n; gate->tail_seq[n % GATE_RING] = 0u;
        gdone = gate->words + (gseq % GATE_RING); gpred = gate->words + GATE_RING + (gseq % GATE_RING);
    }
    // ---- the forward blend over `plist`; mode as run_binning (2: predicated on *pred) ----
    int blend(hipStream_t s, const uint32_t* plist, bool fwd_lists_built, int mode, const uint32_t* pred)
    {
        { int rc = launch_color(s); if (rc != GSRAST_OK) return rc; }  // the other binning scheme / nothing to bin: not forked yet
        SideStream* const side = fork.side;
        if (side) { GS_HIP(hipStreamWaitEvent(s, side->join, 0)); if (plan.zero_in_blend) fork.joined = true; }       // the colours (rec2) are the blend's input
        ProfScope ps(K_BLEND_FWD, s);
        uint32_t grid = ((T + 7) / 8) * 8;
        BlendArgs ba{};
        ba.ranges = ranges; ba.plist = plist; ba.W = W; ba.H = H; ba.gx = cam.gx; ba.T = T; ba.r0 = rec0; ba.r1 = rec1; ba.r2 = rec2;
        ba.bg = c.background; ba.oc = c.out_color; ba.od = c.out_depth; ba.fT = at<float>(img, IL.final_T); ba.nc = at<uint32_t>(img, IL.n_contrib); ba.tm = at<uint32_t>(img, IL.tile_max);
        ba.oad = out_acc_depth; ba.oal = out_alpha;           // (every launch: the first pass, the completion pass, a redo)
        if (plan.zero_in_blend && !plan.zero_touched && !o.forward_only && mode != 2) { ba.zero4 = grec; ba.n_zero4 = (uint32_t)((size_t)P * 4); }
        if (fwd_lists_built) { ba.hints = hints; ba.hint_sel = hint_sel; }      // (the slot is only claimed on the work-bucket path)
        ba.cut_margin_x4 = (uint32_t)ctx->pol.margin.load();
        ba.untouched = untouched;
        if (mode == 1) { ba.zcut_used = zcut_used; ba.cut_scalars = scalars; ba.tile_flags = tile_flags; }
        if (mode == 1 && plan.culled) claim_gate();
        if (mode == 1 && gate) ba.gate = GateArgs{ bucket_cnt + (XCD_GROUPS + 1) * WORK_BUCKETS, gpred, gdone, gseq };
        if (mode == 2) ba.pred = pred;
        if (plan.buckets_ok) { ba.bcnt = bucket_cnt; ba.blist = bucket_list; }   // backward order: always appended
        if (plan.ordered) {
            if (plan.buckets_ok && fwd_lists_built) { ba.from_buckets = 1; grid = (uint32_t)(XCD_GROUPS * xcd_group_tiles_host((size_t)cam.gx, (size_t)cam.gy)); }   // the tile-range kernel already bucketed the tiles
            else {
                uint32_t* ord = at<uint32_t>(img, IL.order_fwd);
                tile_order_kernel<<<1, 1024, 0, s>>>(T, ranges, nullptr, ord);
                GS_LAUNCHED("tile_order");
                ba.order = ord;
            }
        }
        launch_blend_fwd(o.exp_mode, plan.culled, o.fwd_pixels_per_lane ? o.fwd_pixels_per_lane : 1 /* the un-culled template is fastest with one pixel per lane */, grid, s, ba);
        GS_LAUNCHED("blend_fwd");
        if (side && !plan.zero_in_blend) { GS_HIP(hipStreamWaitEvent(s, side->join2, 0)); fork.joined = true; }      // the gradient records are zero before anything after this forward
        return GSRAST_OK;
    }

    // ---- the counts' read-back is begun; with a buffer sized from the previous call, binning and blend are enqueued BEFORE the host knows
    // R and Q (the kernels read the counts on the device), so the GPU never idles on the read-back.  If the counts turn out not to fit,
    // the device published empty ranges and the two pieces are simply launched again with exact sizes (exact_redo). ----
    int speculative_launch(hipStream_t s)
    {
        if (!(plan.speculative && totals_pending)) {       // (with the bucket sort the totals come out of the speculative run emission: read back right behind it)
            if (totals_pending) {
                ProfScope ps(K_SCAN_TILES, s);
                depth_bucket_scan_kernel<<<1, 256, 0, s>>>(bk_info, nbk, scalars);
                GS_LAUNCHED("depth_bucket_scan");
                totals_pending = false;
            }
            int rc = read_u32_begin(device, scalars, s, kCountWords, &rb); if (rc != GSRAST_OK) return rc;
        }
        if (!plan.speculative) return GSRAST_OK;
        const bool late = totals_pending;      // the counts arrive by the emission kernel's own store into pinned memory (no copy enqueued)
        if (late) { if (rb_pre) { rb_flag = rb_pre; flag_alias = pre_alias; flag_seq = pre_seq; } else rb_flag = read_flag_prepare(device, &flag_alias, &flag_seq); }
        // (list cut: the sorts over the cut lists are sized for the early runs of recent forwards, not for all runs)
        // (the early set differs from pose to pose -- 0.98 M / 1.29 M column runs at two neighbouring poses of the 3 M cube --, a launch
        // sized too small costs a whole second forward, one sized too large a few empty workgroups: half again as much as the largest of
        // the recent forwards)
        if (plan.cut) nQ1 = early_launch_runs(early_hint().load(), capQ, plan.pose_known || plan.tau_on);
        int rc = run_binning(s, plan.cut ? nQ1 : capQ, plan.cut ? scalars + SC_EARLY_COUNTS : scalars, plan.cut ? 1 : 0, nullptr, late && !rb_flag);
        flag_alias = nullptr;                    // (a repeated emission reads its counts back the ordinary way)
        if (rc == GSRAST_OK) rc = blend(s, at<uint32_t>(bin, 0), true, plan.cut ? 1 : 0, nullptr);
        return rc;
    }
    // (a forward under predicted cut depths keeps two or three times the early set of one under remembered ones: each kind is sized by its own history)
    std::atomic<uint32_t>& early_hint() const { return (plan.tau_on && (plan.tau_forced || !plan.pose_known || !hints)) ? ctx->Qe_hint_tau : ctx->Qe_hint; }

    int sort_again(hipStream_t s)      // with all four radix passes; everything enqueued so far used a wrong order, as after an undersized speculative launch
    {
        ctx->redo_count++;
        int rc = sort_and_scan(s, false, false);
        if (rc == GSRAST_OK) rc = read_u32(device, scalars, s, counts, kCountWords);
        sort_redone = true;
        return rc;
    }
    // ---- the counts arrive; what they say about the depth sort: the histogram's range, the bucket sort's back-off, a sort to be repeated ----
    int absorb_depth_sort(hipStream_t s)
    {
        { int rc = rb_flag ? read_flag_finish(rb_flag, scalars, s, counts) : read_u32_finish(rb, scalars, s, counts, kCountWords); if (rc != GSRAST_OK) return rc; }
        DepthSortPolicy& zs = ctx->zsort;      // (the decisions: gsrast_policy.h)
        if (!plan.bucket_sort && o.depth_sort == 0) zs.radix_forward();
        if (plan.bucket_sort) {
            if (counts[SC_BUCKET_OVER] == 0) zs.clean_forward();
            else {      // more Gaussians at (nearly) one depth than a bucket holds: sort again with the radix passes
                // (the histogram's range is learned from this call either way; whether its table was up to the view decides about a pause)
                zs.overflow(ctx->zrange.learn(counts[SC_ZBINS], zh_klo, zh_shift));
                int rc = sort_again(s); if (rc != GSRAST_OK) return rc;
                if (plan.adaptive_sort) zs.radix_key_bits(counts[SC_KEY_BITS]);
            }
        } else if (plan.adaptive_sort) {
            if (plan.assume_short && counts[SC_SHORT_WRONG] != 0) { int rc = sort_again(s); if (rc != GSRAST_OK) return rc; }      // the scene's depth range widened
            zs.radix_key_bits(counts[SC_KEY_BITS]);
        }
        if (plan.runbin && counts[SC_R_HI] != 0) return fail(GSRAST_E_OVERFLOW, "forward: more than 2^31-1 instances");
        return GSRAST_OK;
    }
    // ---- what the counts teach the context: capacity hints, the early set's size, the cut's policy (gsrast_policy.h) ----
    int absorb_counts()
    {
        const auto t2 = std::chrono::steady_clock::now();
        CutPolicy& pol = ctx->pol;
        if (trace_on()) fprintf(stderr, "[gsrast] alloc(spec) %.1f us, readback wait %.1f us, cap %u R %u Q %u%s | cut %d (pays %d: last_Q %u pause %d) late %u Q_early %u nQ1 %u capQ %u bucket_sort %d (over %u) hints %d zh %08x >> %d bins %u-%u\n",
                               std::chrono::duration<double, std::micro>(t1 - t0).count(), std::chrono::duration<double, std::micro>(t2 - t1).count(), cap, counts[SC_R_LO], counts[SC_Q],
                               plan.speculative ? " (speculative)" : "", (int)plan.cut, (int)plan.cut_pays, ctx->last_Q.load(), pol.pause.load(), counts[SC_N_LATE], counts[SC_Q_EARLY], nQ1, capQ,
                               (int)plan.bucket_sort, counts[SC_BUCKET_OVER], hints ? 1 : 0, zh_klo, zh_shift, counts[SC_ZBINS] & 0xFFFFu, counts[SC_ZBINS] >> 16);
        if (counts[SC_R_LO] > 0x7FFFFFFFu) return fail(GSRAST_E_OVERFLOW, "forward: more than 2^31-1 instances");
        const uint32_t R = counts[SC_R_LO], Q = counts[SC_Q];
        if (plan.bucket_sort && !sort_redone) (void)ctx->zrange.learn(counts[SC_ZBINS], zh_klo, zh_shift);
        // capacity hints decay slowly: consecutive calls render different views, a buffer sized for the largest recent one
        // keeps the speculative launch valid
        ctx->R_hint = follow_hint(ctx->R_hint.load(), R, 4); ctx->Q_hint = follow_hint(ctx->Q_hint.load(), Q, 4);
        ctx->last_R = R; ctx->last_Q = Q;
        ctx->last_late = plan.cut ? counts[SC_N_LATE] : 0u; ctx->last_Qe = plan.cut ? counts[SC_Q_EARLY] : Q;
        // (a cut forward that removed too little to pay for itself; round 5: FOUR in a row before the context sits out)
        if (plan.cut) pol.forward_counts(plan.tau_on, counts[SC_N_LATE], Q, counts[SC_Q_EARLY], (uint32_t)P, plan.list_cut_always);
        if (plan.cut && plan.speculative && !sort_redone) { std::atomic<uint32_t>& hint = early_hint(); hint = follow_hint(hint.load(), counts[SC_Q_EARLY], 5); }
        // fallbacks of this thread's earlier cut forwards, as the device reported them (everything enqueued before this forward's counts has run)
        // (a completion pass over a few tiles is cheap and expected; its cost grows with the tiles it lists again: one over an eighth of
        // the image counts like rounds 3's whole second forward, smaller ones in proportion)
        if (const uint32_t q2 = take_fallback_event(device)) {       // (the column runs of the pass's candidates)
            const int before = pol.fb_score.load();
            const int pts = pol.completion_pass(q2, ctx->last_Q.load(), (uint32_t)P, plan.list_cut_always, plan.tau_mode);
            if (trace_on()) fprintf(stderr, "[gsrast] completion pass reported: %u column runs of %u, %d points on a score of %d; margin %d / 4, tau_req %d, pause %d\n", q2, ctx->last_Q.load(), pts, before,
                                   pol.margin.load(), pol.tau_req.load(), pol.pause.load());
        } else if (plan.cut && counts[SC_N_LATE] != 0u) pol.clean_cut_forward();
        return GSRAST_OK;
    }

    // ---- List cut: the lists in flight hold the early Gaussians only.  The blend verified them; behind it, a COMPLETION pass (round 4), every
    // kernel predicated on the blend's verdict (gsrast_common.h): the Gaussians that touch a flagged tile -- the candidates --, their missing
    // colours, their column runs through flagged tiles, and the flagged tiles' blend from their full lists.  Nothing of this runs in the
    // steady state.  The pass runs on its own stream behind a gate (ChainGate above), unless that cannot be had: then on the caller's. ----
    int completion_pass(hipStream_t s_caller)
    {
        if (gate) {      // (claimed with the blend's launch: its last workgroup has copied the verdict and, if there is nothing to do, released us)
            GS_HIP(hipEventRecord(gate->ev, s_caller));
            GS_HIP(hipStreamWaitEvent(gate->stream, gate->ev, 0));
        }
        const hipStream_t s = gate ? gate->stream : s_caller;
        const uint32_t* const pred = gate ? gpred : scalars + SC_REDO_PRED;      // (the gate's copy of the predicate: the forward's buffers may be gone when the chain's no-ops run)
        ProfScope ps(K_CUT_REDO, s);           // (on the stream the pass runs on: its events bracket the chain, not an empty interval of the caller's stream)
        struct Off { Off() { t_prof_off++; } ~Off() { t_prof_off--; } } off;
        cut_candidates_kernel<<<std::min((P + 255) / 256, 2048), 256, 0, s>>>((uint32_t)P, tiles, rect, tile_flags, T, (uint32_t)cam.gx, color_skip, cand_bits, at<unsigned long long>(geom, GL.skip2), pred);
        int rc = post_launch("cut_candidates", s);
        if (rc == GSRAST_OK && plan.cut_colors) rc = color_kernels(s, true, pred);      // (the late candidates' colours)
        if (rc == GSRAST_OK) rc = run_binning(s, capQ, scalars + SC_PASS2, 2, pred, false);
        if (rc == GSRAST_OK) rc = blend(s, at<uint32_t>(bin, 0), true, 2, pred);
        if (gate) {
            // (also after an error above: the caller's stream must not wait for a release nobody sends)
            chain_done_kernel<<<1, 1, 0, gate->stream>>>(pred, gdone, gseq);
            const hipError_t e1 = hipGetLastError();
            {   std::lock_guard<std::mutex> lk(ctx->mu);      // the chain's tail: whoever wants this slot's successor asks this event
                if (hipEventRecord(gate->tail[gseq % GATE_RING], gate->stream) == hipSuccess) gate->tail_seq[gseq % GATE_RING] = gseq; }
            const hipError_t e2 = hipStreamWaitValue32(s_caller, gdone, gseq, hipStreamWaitValueEq, 0xFFFFFFFFu);
            if (e1 != hipSuccess || e2 != hipSuccess) {     // no gate after all: an ordinary join behind the chain, and never again
                { std::lock_guard<std::mutex> lk(ctx->mu); gate->failed = true; }
                (void)hipEventRecord(gate->ev, gate->stream);
                (void)hipStreamWaitEvent(s_caller, gate->ev, 0);
            }
        }
        return rc;
    }
    // ---- the end of every successful forward: the consumed Gaussians' gradient records, the prefilter promise's verdict ----
    int finish(hipStream_t s, uint32_t R)
    {
        if (plan.zero_touched) {
            ProfScope ps(K_GREC_ZERO, s);
            grec_zero_touched_kernel<<<(unsigned)(((size_t)P + 256 * GZ_PER - 1) / (256 * GZ_PER)), 256, 0, s>>>(P, untouched, grec, scalars);
            GS_LAUNCHED("grec_zero_touched");
        }
        if (prefilter_word) { int rc = prefilter_verdict(prefilter_word, s); if (rc != GSRAST_OK) return rc; }
        return (int)R;
    }
    // ---- binning + blend with exact sizes: no speculative launch, or one whose capacities (or order) did not fit ----
    int exact_redo(hipStream_t s, uint32_t R, uint32_t Q)
    {
        if (plan.speculative && !sort_redone) ctx->redo_count++;
        if (plan.cut) GS_HIP(hipMemsetAsync(scalars + SC_N_LATE, 0, sizeof(uint32_t), s));      // (the backward must not take a late Gaussian's rows for zero: below it is listed)
        if (plan.cut_colors && fork.launched) {     // everything from here on lists ALL Gaussians: the colours the list cut left out are evaluated now
            if (fork.side) GS_HIP(hipStreamWaitEvent(s, fork.side->join, 0));
            int rc = color_kernels(s, false, nullptr);
            if (rc != GSRAST_OK) return rc;
        }
        if (plan.speculative)    // redo: the truncated pass already appended every tile to the work buckets once
            GS_HIP(hipMemsetAsync(bucket_cnt, 0, (XCD_GROUPS + 1) * WORK_BUCKETS * sizeof(uint32_t), s));
        if (!bin || R > cap || Q > capQ) {   // first call, or the scene grew by more than 25 %: ask again (the callback's last answer counts)
            cap = R; capQ = Q;
            bin = (char*)c.binning_alloc(c.binning_ctx, bin_bytes());
            if (!bin) return fail(GSRAST_E_ALLOC, "forward: binning allocation failed");
        }
        // The layout inside the buffer follows its CAPACITY; the sorted Gaussian ids (point_list) always end in the
        // array at offset 0, whatever the capacity, the pass count and the binning scheme -- all the backward needs.
        if (plan.runbin && (R == 0 || Q == 0)) GS_HIP(hipMemsetAsync(ranges, 0, (size_t)T * sizeof(uint2), s));
        int rc = GSRAST_OK;
        if (R > 0 && Q > 0 && plan.runbin) rc = run_binning(s, Q, nullptr, 0, nullptr, false);
        else if (R > 0 && !plan.runbin) rc = T <= 65536u ? instance_binning<uint16_t>(s, R) : instance_binning<uint32_t>(s, R);
        if (rc == GSRAST_OK) rc = blend(s, at<uint32_t>(bin, 0), plan.runbin && R > 0 && Q > 0, 0, nullptr);
        return rc == GSRAST_OK ? finish(s, R) : rc;
    }
};
} } // namespace

// The one forward.  Dense: the inputs are the activated arrays.  Raw family: means3D / opacities / scales / rotations are the model's raw
// leaves, shs a non-null placeholder, and the per-Gaussian kernels run as their RAW instantiations.
// checks -> plan -> preprocess -> sort -> speculative binning + blend -> read-back -> (sort redo) -> accept, completion pass, or exact redo
static int forward_impl(gsrast_context* ctx, const gsrast_options* options, const gsrast_forward_call& c)
{
    const auto t_entry = std::chrono::steady_clock::now();
    RoctxRange range_fwd(c.family == GSRAST_FAMILY_RAW ? "gsrast_forward" "_raw" : "gsrast_forward");      // (the range names are the ones profiles have always been read by)
    ForwardRun r(ctx, options, c, t_entry);
    const hipStream_t s = r.stream;
    int rc = r.check_and_plan(s);
    if (rc != GSRAST_OK || c.P == 0) return rc;
    if ((rc = r.buffers(s)) != GSRAST_OK || (rc = r.begin_policy(s)) != GSRAST_OK) return rc;
    if ((rc = r.preprocess(s)) != GSRAST_OK || (rc = r.sort_and_scan(s, r.plan.assume_short, r.plan.bucket_sort)) != GSRAST_OK) return rc;
    r.learn_pose();
    // Everything that does not depend on num_rendered is enqueued / prepared before the host waits: the colour kernels, beside the binning
    if ((rc = r.speculative_buffer(s)) != GSRAST_OK || (rc = r.launch_color(s)) != GSRAST_OK || (rc = r.speculative_launch(s)) != GSRAST_OK) return rc;
    if ((rc = r.absorb_depth_sort(s)) != GSRAST_OK || (rc = r.absorb_counts()) != GSRAST_OK) return rc;
    const ForwardPlan& plan = r.plan;
    const uint32_t R = r.counts[SC_R_LO], Q = r.counts[SC_Q];
    const bool early_fits = !plan.cut || r.counts[SC_Q_EARLY] <= r.nQ1;
    if (!(plan.speculative && !r.sort_redone && R <= r.cap && Q <= r.capQ && early_fits)) return r.exact_redo(s, R, Q);
    // everything is already in flight
    if (plan.cut && r.counts[SC_N_LATE] != 0u && (rc = r.completion_pass(s)) != GSRAST_OK) return rc;
    return r.finish(s, R);
}

// A call record as the library sees it: struct_size bytes of the caller's in a zeroed record of its own, so that fields the caller's header
// did not have are null (include/gsrast.h: how the records grow).  The refusals of the record itself, before any check of its contents.
static const char* take_record(void* own, size_t own_size, const void* call, size_t min_size)
{
    if (!call) return "call record: NULL";
    size_t n;
    memcpy(&n, call, sizeof n);      // (struct_size is the first field of both records)
    if (n < min_size || n > own_size) return "call record: struct_size is not one this library knows";
    memset(own, 0, own_size);
    memcpy(own, call, n);
    return nullptr;
}
static bool family_known(int family) { return family == GSRAST_FAMILY_DENSE || family == GSRAST_FAMILY_RAW; }

// ---- the exported forwards: the record call, and the reference-shaped positional one that fills a record by name ----
int gsrast_render_forward(gsrast_context* ctx, const gsrast_options* options, const gsrast_forward_call* call)
{
    gsrast_forward_call c;
    if (const char* e = take_record(&c, sizeof c, call, GSRAST_FORWARD_CALL_MIN)) return fail(GSRAST_E_ARG, e);
    if (!family_known(c.family)) return fail(GSRAST_E_ARG, "call record: unknown family");
    if (c.family == GSRAST_FAMILY_DENSE ? c.raw != nullptr
                                        : c.means3D || c.shs || c.colors_precomp || c.opacities || c.scales || c.rotations || c.cov3D_precomp || c.prefiltered)
        return fail(GSRAST_E_ARG, "call record: dense family with raw set, or raw family with a dense input / prefiltered set");
    return forward_impl(ctx, options, c);
}

int gsrast_forward(gsrast_alloc_fn geometry_alloc, void* geometry_ctx, gsrast_alloc_fn binning_alloc,
                   void* binning_ctx, gsrast_alloc_fn image_alloc, void* image_ctx, int P, int D, int M,
                   const float* background, int width, int height, const float* means3D, const float* shs,
                   const float* colors_precomp, const float* opacities, const float* scales,
                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                   const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                   float tan_fovy, int prefiltered, float* out_color, float* out_depth, int* radii, void* stream)
{
    gsrast_forward_call c{};
    c.struct_size = sizeof c; c.family = GSRAST_FAMILY_DENSE;
    c.geometry_alloc = geometry_alloc; c.geometry_ctx = geometry_ctx; c.binning_alloc = binning_alloc; c.binning_ctx = binning_ctx;
    c.image_alloc = image_alloc; c.image_ctx = image_ctx;
    c.P = P; c.D = D; c.M = M; c.background = background; c.width = width; c.height = height;
    c.means3D = means3D; c.shs = shs; c.colors_precomp = colors_precomp; c.opacities = opacities; c.scales = scales;
    c.rotations = rotations; c.cov3D_precomp = cov3D_precomp; c.scale_modifier = scale_modifier;
    c.viewmatrix = viewmatrix; c.projmatrix = projmatrix; c.cam_pos = cam_pos; c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy;
    c.prefiltered = prefiltered; c.out_color = out_color; c.out_depth = out_depth; c.radii = radii; c.stream = stream;
    return forward_impl(nullptr, nullptr, c);
}

__global__ void __launch_bounds__(256)
touched_rows_kernel(int P, const unsigned char* __restrict__ untouched, const uint32_t* __restrict__ scalars, unsigned char* __restrict__ flags)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    flags[i] = scalars[SC_TOUCH_VALID] != 0u ? (unsigned char)(untouched[i] ? 0 : 1) : (unsigned char)1;
}
int gsrast_touched_rows(int P, const char* geom_buffer, unsigned char* flags, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || (P > 0 && (!geom_buffer || !flags))) return fail(GSRAST_E_ARG, "touched_rows: bad arguments");
    if (P == 0) return GSRAST_OK;
    const GeomLayout GL = geom_layout((size_t)P);
    touched_rows_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, at<unsigned char>(geom_buffer, GL.untouched), at<uint32_t>(geom_buffer, GL.scalars), flags);
    GS_LAUNCHED("touched_rows");
    return GSRAST_OK;
}

// ---- per-Gaussian blend-weight statistics of a finished forward (gsrast_contrib.h) ---------------------------------------------------
namespace {
struct ContribLayout { size_t sum, max, cnt, top, total; };
ContribLayout contrib_layout(size_t P)
{
    ContribLayout L; Carver c;
    const size_t Pp = P ? P : 1;
    L.sum = c.take(Pp * 8); L.max = c.take(Pp * 4); L.cnt = c.take(Pp * 4); L.top = c.take(Pp * 4);      // 20 bytes per Gaussian
    L.total = c.o;
    return L;
}
} // namespace

size_t gsrast_contrib_scratch_bytes(int P) { return contrib_layout(P > 0 ? (size_t)P : 0).total; }

int gsrast_contrib_stats(const gsrast_options* options, int P, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                         const char* image_buffer, const float* pixel_weights, float* stats, char* scratch, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || R < 0) return fail(GSRAST_E_ARG, "contrib_stats: negative P or R");
    if (width <= 0 || height <= 0) return fail(GSRAST_E_ARG, "contrib_stats: zero-size image");
    if (P == 0) return GSRAST_OK;
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail(GSRAST_E_ARG, "contrib_stats: NULL state buffer");
    if (!stats) return fail(GSRAST_E_ARG, "contrib_stats: NULL stats");
    if (!scratch) return fail(GSRAST_E_ARG, "contrib_stats: NULL scratch");
    if (((uintptr_t)stats & 15) || ((uintptr_t)scratch & 15)) return fail(GSRAST_E_ARG, "contrib_stats: stats / scratch must be 16-byte aligned");
    const gsrast_options o = options ? *options : snapshot_defaults();
    if (o.exp_mode < 0 || o.exp_mode > 2) return fail(GSRAST_E_ARG, "contrib_stats: exp_mode must be 0, 1 or 2");
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    const ContribLayout CL = contrib_layout((size_t)P);
    unsigned long long* const a_sum = at<unsigned long long>(scratch, CL.sum);
    uint32_t* const a_max = at<uint32_t>(scratch, CL.max); uint32_t* const a_cnt = at<uint32_t>(scratch, CL.cnt); uint32_t* const a_top = at<uint32_t>(scratch, CL.top);
    GS_HIP(hipMemsetAsync(scratch, 0, CL.total, s));      // (the caller owes nothing: whatever the scratch held)
    {
        ProfScope ps(K_CONTRIB_BLEND, s);
        pick_int<0, 1, 2>(o.exp_mode, [&](auto mode) { L.front_to_back(contrib_blend_kernel<decltype(mode)::value>, s, pixel_weights, a_sum, a_max, a_cnt, a_top); });
        GS_LAUNCHED("contrib_blend");
    }
    {
        ProfScope ps(K_CONTRIB_FINISH, s);
        contrib_finish_kernel<<<(P + 255) / 256, 256, 0, s>>>(P, a_sum, a_max, a_cnt, a_top, reinterpret_cast<float4*>(stats));
        GS_LAUNCHED("contrib_finish");
    }
    return GSRAST_OK;
}

// ---- per-Gaussian feature vectors through the blend of a finished forward, and back (gsrast_features.h) ------------------------------
namespace {
// What the two calls refuse alike, before any device work (one text each); fwd: the text names features_forward, else features_backward
const char* features_refusal(bool fwd, int P, int R, int C, int width, int height)
{
    if (C < 1 || C > GSRAST_FEATURES_MAX_C) return fwd ? "features_forward: C must be 1..64" : "features_backward: C must be 1..64";
    if (P < 0 || R < 0) return fwd ? "features_forward: negative P or R" : "features_backward: negative P or R";
    if (width <= 0 || height <= 0) return fwd ? "features_forward: zero-size image" : "features_backward: zero-size image";
    return nullptr;
}
// The chunk of the pass that starts at channel c0: the smallest instantiated width that holds what is left, 32 at most
inline int features_chunk(int C, int c0) { const int rem = C - c0; return rem > 16 ? 32 : rem > 8 ? 16 : rem > 4 ? 8 : 4; }
} // namespace

int gsrast_features_forward(const gsrast_options* options, int P, int R, int C, int width, int height, const char* geom_buffer,
                            const char* binning_buffer, const char* image_buffer, const float* features, float* feature_map, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = features_refusal(true, P, R, C, width, height)) return fail(GSRAST_E_ARG, e);
    if (!feature_map) return fail(GSRAST_E_ARG, "features_forward: NULL feature_map");
    if (P > 0 && (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer))) return fail(GSRAST_E_ARG, "features_forward: NULL state buffer");
    if (P > 0 && !features) return fail(GSRAST_E_ARG, "features_forward: NULL features");
    const gsrast_options o = options ? *options : snapshot_defaults();
    if (o.exp_mode < 0 || o.exp_mode > 2) return fail(GSRAST_E_ARG, "features_forward: exp_mode must be 0, 1 or 2");
    // (no Gaussian, or no instance: nothing was blended)
    if (P == 0 || R == 0) { GS_HIP(hipMemsetAsync(feature_map, 0, (size_t)C * (size_t)width * (size_t)height * sizeof(float), s)); return GSRAST_OK; }
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    ProfScope ps(K_FEATURES_FWD, s);
    for (int c0 = 0; c0 < C;) {
        const int ch = features_chunk(C, c0);
        pick_int<0, 1, 2>(o.exp_mode, [&](auto mode) { pick_int<4, 8, 16, 32>(ch, [&](auto chunk) {
            L.front_to_back(features_fwd_kernel<decltype(mode)::value, decltype(chunk)::value>, s, features, C, c0, feature_map);
        }); });
        GS_LAUNCHED("features_fwd");
        c0 += ch;
    }
    return GSRAST_OK;
}

int gsrast_features_backward(const gsrast_options* options, int P, int R, int C, int width, int height, char* geom_buffer,
                             const char* binning_buffer, const char* image_buffer, const float* features, const float* dL_dfeature_map,
                             float* dL_dfeatures, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = features_refusal(false, P, R, C, width, height)) return fail(GSRAST_E_ARG, e);
    if (!dL_dfeature_map) return fail(GSRAST_E_ARG, "features_backward: NULL dL_dfeature_map");
    if (P > 0 && (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer))) return fail(GSRAST_E_ARG, "features_backward: NULL state buffer");
    if (P > 0 && !features) return fail(GSRAST_E_ARG, "features_backward: NULL features");
    if (P > 0 && !dL_dfeatures) return fail(GSRAST_E_ARG, "features_backward: NULL dL_dfeatures");
    const gsrast_options o = options ? *options : snapshot_defaults();
    if (o.exp_mode < 0 || o.exp_mode > 2) return fail(GSRAST_E_ARG, "features_backward: exp_mode must be 0, 1 or 2");
    if (P == 0) return GSRAST_OK;
    GS_HIP(hipMemsetAsync(dL_dfeatures, 0, (size_t)P * (size_t)C * sizeof(float), s));
    if (R == 0) return GSRAST_OK;             // (no instance: nothing was blended)
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    ProfScope ps(K_FEATURES_BWD, s);
    for (int c0 = 0; c0 < C;) {
        const int ch = features_chunk(C, c0);
        pick_int<0, 1, 2>(o.exp_mode, [&](auto mode) { pick_int<4, 8, 16, 32>(ch, [&](auto chunk) {
            L.back_to_front(features_bwd_kernel<decltype(mode)::value, decltype(chunk)::value>, s, features, C, c0, dL_dfeature_map, at<float>(geom_buffer, L.grec), dL_dfeatures);
        }); });
        GS_LAUNCHED("features_bwd");
        c0 += ch;
    }
    return GSRAST_OK;
}

// ---- the depth-distortion map of a finished forward, and back (gsrast_distort.h) -------------------------------------------------------
namespace {
// What the two calls refuse alike, before any device work (one text each); fwd: the text names distortion_forward, else distortion_backward
const char* distortion_refusal(bool fwd, const gsrast_options* options, int P, int R, int width, int height, const void* geom, const void* binning, const void* image,
                               const void* map_or_grad, const void* moments)
{
    if (P < 0 || R < 0) return fwd ? "distortion_forward: negative P or R" : "distortion_backward: negative P or R";
    if (width <= 0 || height <= 0) return fwd ? "distortion_forward: zero-size image" : "distortion_backward: zero-size image";
    if (P > 0 && (!geom || !image || (R > 0 && !binning))) return fwd ? "distortion_forward: NULL state buffer" : "distortion_backward: NULL state buffer";
    if ((fwd || P > 0) && !map_or_grad) return fwd ? "distortion_forward: NULL distort_map" : "distortion_backward: NULL dL_ddistort";
    if ((fwd || P > 0) && !moments) return fwd ? "distortion_forward: NULL moments" : "distortion_backward: NULL moments";
    const int mode = options ? options->exp_mode : snapshot_defaults().exp_mode;
    if (mode < 0 || mode > 2) return fwd ? "distortion_forward: exp_mode must be 0, 1 or 2" : "distortion_backward: exp_mode must be 0, 1 or 2";
    return nullptr;
}
} // namespace

int gsrast_distortion_forward(const gsrast_options* options, int P, int R, int width, int height, const char* geom_buffer,
                              const char* binning_buffer, const char* image_buffer, float* distort_map, float* moments, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = distortion_refusal(true, options, P, R, width, height, geom_buffer, binning_buffer, image_buffer, distort_map, moments)) return fail(GSRAST_E_ARG, e);
    const gsrast_options o = options ? *options : snapshot_defaults();
    const size_t N = (size_t)width * (size_t)height;
    // (no Gaussian, or no instance: nothing was blended)
    if (P == 0 || R == 0) { GS_HIP(hipMemsetAsync(distort_map, 0, N * sizeof(float), s)); GS_HIP(hipMemsetAsync(moments, 0, 2 * N * sizeof(float), s)); return GSRAST_OK; }
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    ProfScope ps(K_DISTORT_FWD, s);
    pick_int<0, 1, 2>(o.exp_mode, [&](auto mode) { L.front_to_back(distort_fwd_kernel<decltype(mode)::value>, s, distort_map, moments); });
    GS_LAUNCHED("distort_fwd");
    return GSRAST_OK;
}

int gsrast_distortion_backward(const gsrast_options* options, int P, int R, int width, int height, char* geom_buffer,
                               const char* binning_buffer, const char* image_buffer, const float* moments, const float* dL_ddistort, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = distortion_refusal(false, options, P, R, width, height, geom_buffer, binning_buffer, image_buffer, dL_ddistort, moments)) return fail(GSRAST_E_ARG, e);
    const gsrast_options o = options ? *options : snapshot_defaults();
    if (P == 0 || R == 0) return GSRAST_OK;      // (no Gaussian, or no instance: nothing was blended, nothing is added)
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    ProfScope ps(K_DISTORT_BWD, s);
    pick_int<0, 1, 2>(o.exp_mode, [&](auto mode) { L.back_to_front(distort_bwd_kernel<decltype(mode)::value>, s, moments, dL_ddistort, at<float>(geom_buffer, L.grec)); });
    GS_LAUNCHED("distort_bwd");
    return GSRAST_OK;
}

// ---- each pixel's first or heaviest K contributors of a finished forward (gsrast_topk.h) -------------------------------------------------
int gsrast_pixel_contributors(const gsrast_options* options, int P, int R, int width, int height, const char* geom_buffer,
                              const char* binning_buffer, const char* image_buffer, int K, int order, int32_t* ids, float* weights,
                              int32_t* count, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || R < 0) return fail(GSRAST_E_ARG, "pixel_contributors: negative P or R");
    if (width <= 0 || height <= 0) return fail(GSRAST_E_ARG, "pixel_contributors: zero-size image");
    if (K < 1 || K > TOPK_MAX) return fail(GSRAST_E_ARG, "pixel_contributors: K must be 1..16");
    if (order != 0 && order != 1) return fail(GSRAST_E_ARG, "pixel_contributors: order must be 0 (weight) or 1 (depth)");
    const gsrast_options o = options ? *options : snapshot_defaults();
    if (o.exp_mode < 0 || o.exp_mode > 2) return fail(GSRAST_E_ARG, "pixel_contributors: exp_mode must be 0, 1 or 2");
    if (P > 0 && R > 0 && (!geom_buffer || !image_buffer || !binning_buffer)) return fail(GSRAST_E_ARG, "pixel_contributors: NULL state buffer");
    if (!ids) return fail(GSRAST_E_ARG, "pixel_contributors: NULL ids");
    if (!weights) return fail(GSRAST_E_ARG, "pixel_contributors: NULL weights");
    if (P == 0 || R == 0) {                       // (no Gaussian, or no instance: nothing was blended, no state is read)
        const size_t pixels = (size_t)width * (size_t)height, slots = pixels * (size_t)K;
        const size_t groups = (slots + 255) / 256;
        topk_fill_kernel<<<(unsigned)(groups < 4096 ? groups : 4096), 256, 0, s>>>(slots, pixels, ids, weights, count);
        GS_LAUNCHED("topk_fill");
        return GSRAST_OK;
    }
    const ReplayLaunch L(P, width, height, geom_buffer, binning_buffer, image_buffer);
    launch_pixel_topk(L, o.exp_mode, s, K, order, ids, weights, count);
    GS_LAUNCHED("pixel_topk");
    return GSRAST_OK;
}

// ---- the projection as a call of its own (gsrast_project.h) -----------------------------------------------------------------------------
namespace {
// What the two calls refuse alike, before any device work (one text each, behind the call's name)
const char* project_refusal(const gsrast_project* d)
{
    if (!d) return "NULL descriptor";
    if (d->P < 0) return "negative P";
    if (d->width <= 0 || d->height <= 0) return "zero-size image";
    if (!(d->tanfovx > 0.0f) || !(d->tanfovy > 0.0f)) return "tanfovx / tanfovy must be positive";
    if (!d->means3D) return "NULL means3D";
    if (!d->viewmatrix || !d->projmatrix) return "NULL viewmatrix / projmatrix";
    if ((d->scales != nullptr) != (d->rotations != nullptr)) return "scales and rotations go together";
    if ((d->scales != nullptr) == (d->cov3D_precomp != nullptr)) return "exactly one of (scales, rotations) and cov3D_precomp";
    if (((uintptr_t)d->rotations & 15) || ((uintptr_t)d->dL_drotations & 15)) return "rotations / dL_drotations must be 16-byte aligned";
    if (d->flags & ~GSRAST_PROJECT_ANTIALIAS) return "flags: unknown bits";
    return nullptr;
}
} // namespace

int gsrast_project_forward(const gsrast_project* d, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = project_refusal(d)) return refuse("project_forward", e);
    const bool aa = (d->flags & GSRAST_PROJECT_ANTIALIAS) != 0;
    if (!d->means2D || !d->depths || !d->conics || !d->radii) return refuse("project_forward", "NULL means2D / depths / conics / radii");
    if (aa != (d->compensation != nullptr)) return refuse("project_forward", aa ? "NULL compensation with GSRAST_PROJECT_ANTIALIAS" : "compensation without GSRAST_PROJECT_ANTIALIAS");
    if (d->P == 0) return GSRAST_OK;
    const CamArgs cam = make_cam(d->viewmatrix, d->projmatrix, nullptr, d->tanfovx, d->tanfovy, d->scale_modifier, d->width, d->height);
    const unsigned grid = ((unsigned)d->P + PJ_THREADS - 1) / PJ_THREADS;
    pick_bool(aa, [&](auto AA) {
        project_fwd_kernel<decltype(AA)::value><<<grid, PJ_THREADS, 0, s>>>(d->P, d->means3D, d->scales, d->rotations, d->cov3D_precomp, cam,
                                                                                     d->means2D, d->depths, d->conics, d->radii, d->compensation);
    });
    GS_LAUNCHED("project_fwd");
    return GSRAST_OK;
}

int gsrast_project_backward(const gsrast_project* d, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (const char* e = project_refusal(d)) return refuse("project_backward", e);
    const bool aa = (d->flags & GSRAST_PROJECT_ANTIALIAS) != 0;
    if (d->dL_dcompensation && !aa) return refuse("project_backward", "dL_dcompensation without GSRAST_PROJECT_ANTIALIAS");
    if (!d->dL_dmeans3D && !d->dL_dscales && !d->dL_drotations && !d->dL_dcov3D) return refuse("project_backward", "no gradient output");
    if (d->P == 0) return GSRAST_OK;
    const CamArgs cam = make_cam(d->viewmatrix, d->projmatrix, nullptr, d->tanfovx, d->tanfovy, d->scale_modifier, d->width, d->height);
    const unsigned grid = ((unsigned)d->P + PJ_THREADS - 1) / PJ_THREADS;
    pick_bool(aa && d->dL_dcompensation, [&](auto AA) {      // (without its upstream gradient the compensation adds nothing: the plain kernel)
        project_bwd_kernel<decltype(AA)::value><<<grid, PJ_THREADS, 0, s>>>(d->P, d->means3D, d->scales, d->rotations, d->cov3D_precomp, cam,
                                                                                     d->dL_dmeans2D, d->dL_ddepths, d->dL_dconics, d->dL_dcompensation,
                                                                                     d->dL_dmeans3D, d->dL_dscales, d->dL_drotations, d->dL_dcov3D);
    });
    GS_LAUNCHED("project_bwd");
    return GSRAST_OK;
}

static int rows_pack_impl(bool pack, long long n, const long long* idx, int n_arrays, float* const* arrays, const int* widths, float* packed, void* stream)
{
    if (n < 0 || n_arrays < 1 || n_arrays > 8 || !arrays || !widths) return fail(GSRAST_E_ARG, "rows_pack: bad arguments");
    if (n == 0) return GSRAST_OK;
    RowArrays a{}; a.n = n_arrays;
    for (int k = 0; k < n_arrays; k++) {
        if (!arrays[k] || widths[k] < 1) return fail(GSRAST_E_ARG, "rows_pack: NULL array or width < 1");
        a.ptr[k] = arrays[k]; a.width[k] = widths[k]; a.total += widths[k];
    }
    if (!idx || !packed || n * a.total > 0x7FFFFFFFll * 256) return fail(GSRAST_E_ARG, "rows_pack: NULL index / packed array, or too large");
    const unsigned blocks = (unsigned)((n * a.total + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (pack) rows_pack_kernel<true><<<blocks, 256, 0, s>>>(n, idx, a, packed);
    else rows_pack_kernel<false><<<blocks, 256, 0, s>>>(n, idx, a, packed);
    GS_LAUNCHED("rows_pack");
    return GSRAST_OK;
}
int gsrast_rows_pack(long long n, const long long* idx, int n_arrays, const float* const* arrays, const int* widths, float* packed, void* stream)
{ return rows_pack_impl(true, n, idx, n_arrays, const_cast<float* const*>(arrays), widths, packed, stream); }
int gsrast_rows_unpack(long long n, const long long* idx, int n_arrays, float* const* arrays, const int* widths, const float* packed, void* stream)
{ return rows_pack_impl(false, n, idx, n_arrays, arrays, widths, const_cast<float*>(packed), stream); }

// ---- the all-gather gradient exchange (gsrast_exchange.h) ----
static int grow_arrays(GradRowArrays& a, float* const* dense, int M, float* dL_dsh, float* d_dc, float* d_rest, const char* who, bool need_dense = true)
{
    for (int k = 0; k < 4; k++) {
        if (need_dense && (!dense || !dense[k])) return fail(GSRAST_E_ARG, who);
        a.dense[k] = dense ? dense[k] : nullptr;
    }
    a.sh = dL_dsh; a.dc = d_dc; a.rest = d_rest; a.M = M;
    if (dL_dsh || d_dc) {
        if (M < 1 || M * 3 > PP_SH_MAX || ((M * 3) & 3) || ((uintptr_t)dL_dsh & 15) || (d_dc && M > 1 && !d_rest)) return fail(GSRAST_E_ARG, who);
    }
    return GSRAST_OK;
}
int gsrast_grad_rows_pack(int P, const unsigned char* touched, float* const* dense, const float* factor, uint32_t* rows, uint32_t cap, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || (P > 0 && (!touched || !factor || !rows))) return fail(GSRAST_E_ARG, "grad_rows_pack: bad arguments");
    if (P == 0) return GSRAST_OK;
    GradRowArrays a{};
    if (int rc = grow_arrays(a, dense, 0, nullptr, nullptr, nullptr, "grad_rows_pack: four dense arrays are required")) return rc;
    grad_rows_pack_kernel<<<(P + GROW_PACK - 1) / GROW_PACK, 256, 0, s>>>(P, touched, a, factor, rows, cap);
    GS_LAUNCHED("grad_rows_pack");
    return GSRAST_OK;
}
int gsrast_grad_rows_clear(int P, const uint32_t* chunks, int n_chunks, size_t chunk_words, uint32_t cap, float* const* dense, int M, float* dL_dsh,
                           float* d_features_dc, float* d_features_rest, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || n_chunks < 0 || (n_chunks > 0 && cap > 0 && !chunks) || chunk_words < (size_t)(1 + (size_t)cap) * GROW_WORDS) return fail(GSRAST_E_ARG, "grad_rows_clear: bad arguments");
    if (n_chunks == 0 || cap == 0) return GSRAST_OK;
    const int what = (dense ? 1 : 0) | ((dL_dsh || d_features_dc) ? 2 : 0);
    if (!what) return GSRAST_OK;
    GradRowArrays a{};
    if (int rc = grow_arrays(a, dense, M, dL_dsh, d_features_dc, d_features_rest, "grad_rows_clear: bad arrays", dense != nullptr)) return rc;
    const size_t lanes = (size_t)n_chunks * cap * 16;
    if (lanes > 0x7FFFFFFFull * 256) return fail(GSRAST_E_ARG, "grad_rows_clear: too many rows");
    grad_rows_clear_kernel<<<(unsigned)((lanes + 255) / 256), 256, 0, s>>>(chunks, n_chunks, chunk_words, cap, a, what, (uint32_t)P);
    GS_LAUNCHED("grad_rows_clear");
    return GSRAST_OK;
}
int gsrast_grad_rows_add(int P, const uint32_t* chunk, uint32_t cap, float* const* dense, int D, int M, const float* means3D, float scale, float* dL_dsh,
                         float* d_features_dc, float* d_features_rest, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (cap == 0 || P == 0) return GSRAST_OK;
    if (P < 0 || !chunk || !means3D || D < 0 || D > 3 || ((dL_dsh || d_features_dc) && (D + 1) * (D + 1) > M)) return fail(GSRAST_E_ARG, "grad_rows_add: bad arguments");
    GradRowArrays a{};
    if (int rc = grow_arrays(a, dense, M, dL_dsh, d_features_dc, d_features_rest, "grad_rows_add: bad arrays")) return rc;
    grad_rows_add_kernel<<<(cap + PP_THREADS - 1) / PP_THREADS, PP_THREADS, 0, s>>>(chunk, cap, a, means3D, D, scale, (uint32_t)P);
    GS_LAUNCHED("grad_rows_add");
    return GSRAST_OK;
}

int gsrast_sh_grad_combine(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride,
                           float scale, float* dL_dsh, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || N < 1 || M < 1 || D < 0 || D > 3 || (D + 1) * (D + 1) > M) return fail(GSRAST_E_ARG, "sh_grad_combine: bad sizes");
    if (P == 0) return GSRAST_OK;
    if (!means3D || !chunks || !dL_dsh || chunk_stride < (size_t)3 * P + 3) return fail(GSRAST_E_ARG, "sh_grad_combine: NULL or short buffer");
    sh_grad_combine_kernel<<<(P + PP_THREADS - 1) / PP_THREADS, PP_THREADS, 0, s>>>(P, D, M, N, means3D, chunks, chunk_stride, scale, dL_dsh, P, nullptr, nullptr, nullptr);
    GS_LAUNCHED("sh_grad_combine");
    return GSRAST_OK;
}

int gsrast_sh_grad_combine_rows(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride, int rows,
                                const int* row_of, float scale, float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || N < 1 || M < 1 || D < 0 || D > 3 || (D + 1) * (D + 1) > M || rows < 0 || rows > P || (!row_of && rows != P))
        return fail(GSRAST_E_ARG, "sh_grad_combine_rows: bad sizes");
    if (P == 0) return GSRAST_OK;
    if (!means3D || !chunks || chunk_stride < (size_t)3 * rows + 3) return fail(GSRAST_E_ARG, "sh_grad_combine_rows: NULL or short buffer");
    if (!dL_dsh && !d_features_dc) return fail(GSRAST_E_ARG, "sh_grad_combine_rows: no output array");
    if (d_features_dc && M > 1 && !d_features_rest) return fail(GSRAST_E_ARG, "sh_grad_combine_rows: d_features_dc without d_features_rest");
    if (d_features_dc && (M * 3 > PP_SH_MAX || ((M * 3) & 3) || (((uintptr_t)d_features_dc | (uintptr_t)d_features_rest) & 15)))
        return fail(GSRAST_E_ARG, "sh_grad_combine_rows: the split outputs need M = 4 or 16 and 16-byte aligned arrays");
    sh_grad_combine_kernel<<<(P + PP_THREADS - 1) / PP_THREADS, PP_THREADS, 0, s>>>(P, D, M, N, means3D, chunks, chunk_stride, scale, dL_dsh, rows, row_of,
                                                                                   d_features_dc, d_features_rest);
    GS_LAUNCHED("sh_grad_combine_rows");
    return GSRAST_OK;
}

int gsrast_sh_grad_combine_union(int P, int D, int M, int N, const float* means3D, const float* chunks, size_t chunk_stride, int rows,
                                 const long long* idx, float scale, float* dL_dsh, float* d_features_dc, float* d_features_rest, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P < 0 || N < 1 || M < 1 || D < 0 || D > 3 || (D + 1) * (D + 1) > M || rows < 0 || rows > P)
        return fail(GSRAST_E_ARG, "sh_grad_combine_union: bad sizes");
    if (P == 0 || rows == 0) return GSRAST_OK;
    if (!means3D || !chunks || !idx || chunk_stride < (size_t)3 * rows + 3) return fail(GSRAST_E_ARG, "sh_grad_combine_union: NULL or short buffer");
    if (!dL_dsh && !d_features_dc) return fail(GSRAST_E_ARG, "sh_grad_combine_union: no output array");
    if (d_features_dc && !d_features_rest) return fail(GSRAST_E_ARG, "sh_grad_combine_union: d_features_dc without d_features_rest");
    if (M * 3 > PP_SH_MAX || ((M * 3) & 3) || ((uintptr_t)dL_dsh & 15))
        return fail(GSRAST_E_ARG, "sh_grad_combine_union: needs M = 4, 8, 12 or 16 and a 16-byte aligned dL_dsh");
    sh_grad_combine_union_kernel<<<(rows + PP_THREADS - 1) / PP_THREADS, PP_THREADS, 0, s>>>(rows, idx, D, M, N, means3D, chunks, chunk_stride, scale,
                                                                                          dL_dsh, d_features_dc, d_features_rest);
    GS_LAUNCHED("sh_grad_combine_union");
    return GSRAST_OK;
}

// One backward call's state and its stages (backward_impl below is the order they run in).  What the call does is decided once, by
// plan_backward (gsrast_policy.h), from one snapshot of the options and the process-wide switches; the stages only check pointers and enqueue.
// c: the call's record (include/gsrast.h: gsrast_backward_call).  Raw family: `raw` / `raw_grads` replace the dense inputs and gradient outputs (null in
// the record): the dense pointers become the model's raw leaves and their gradients, taken from the two structs in check_and_plan.
namespace {
struct BackwardRun {
    gsrast_backward_call c; const bool raw_family;      // (a copy: the raw family's leaves and gradient arrays take the dense pointers' places)
    gsrast_options o; const hipStream_t s;
    DeviceState* const dev;      // the calling thread's context's record on its current device (the backward's side stream); nullptr: none
    BackwardPlan plan;
    const gsrast_raw_inputs* rawin = nullptr; RawArgs raw{}; RawGrads rawg{};
    CamArgs cam; GeomLayout GL; ImgLayout IL; char *geom = nullptr, *img = nullptr;
    // per-Gaussian gradient records: the only memory the backward accumulates into (64 B / Gaussian, in the geometry buffer)
    // (the forward leaves them zero: a caller that knows this is the first backward on this state says so and saves the fill)
    float* grec = nullptr;
    struct SideJoinGuard {      // an error exit must not leave side-stream work running on the caller's arrays
        SideStream* side = nullptr; bool joined = false;
        ~SideJoinGuard() { if (side && !joined) (void)hipStreamSynchronize(side->stream); }
    } fork;

    BackwardRun(const gsrast_options* options, const gsrast_backward_call& c_) : c(c_), raw_family(c_.family == GSRAST_FAMILY_RAW), o(options ? *options : snapshot_defaults()), s((hipStream_t)c_.stream),
          dev(thread_context()->device_state(current_device())) {}

    // ---- the plan, and the checks every entry point shares (before any device work) ----
    int check_and_plan()
    {
        const int P = c.P, M = c.M;
        if (raw_family) o.sh_grad_factors = (c.raw_grads && c.raw_grads->d_sh_factor) ? 1 : 0;      // the SH leaves' gradient leaves as its [P][3] factor (multi-GPU exchange)
        plan = plan_backward(o, BackwardInputs{ c.flags, P, c.D, c.R, c.width, c.height, raw_family, (raw_family ? c.raw && c.raw->features_dc : c.shs != nullptr),
                                                c.colors_precomp != nullptr, c.cov3D_precomp != nullptr, c.dL_dacc_depth != nullptr || c.dL_dalpha != nullptr,
                                                backward_known_flags(c.struct_size), c.dL_dmean2D_abs != nullptr, c.dL_dcamera != nullptr, c.pose_scratch != nullptr }, snapshot_switches());
        if (plan.refusal) return fail(GSRAST_E_ARG, plan.refusal);
        if (raw_family) {
            rawin = c.raw;
            const gsrast_raw_grads* const out = c.raw_grads;
            if (const char* e = raw_inputs_check(P, M, rawin)) return fail(GSRAST_E_ARG, e);
            if (!out) return fail(GSRAST_E_ARG, "backward_raw: NULL gradient set");
            if (P == 0) return GSRAST_OK;
            if (!out->dL_dmean2D || !out->d_xyz || !out->d_rotation || !out->d_scaling || !out->d_opacity_logit) return fail(GSRAST_E_ARG, "backward_raw: NULL required gradient output");
            if ((rawin->rot_res != nullptr) != (out->d_rot_res != nullptr) && rawin->rot_res == nullptr) return fail(GSRAST_E_ARG, "backward_raw: d_rot_res without rot_res");
            if (out->d_shs_res && !rawin->shs_res) return fail(GSRAST_E_ARG, "backward_raw: d_shs_res without shs_res");
            const bool fac = out->d_sh_factor != nullptr;
            if (fac && (rawin->shs_res || out->d_shs_res)) return fail(GSRAST_E_ARG, "backward_raw: d_sh_factor cannot be combined with shs_res / d_shs_res");
            if ((out->d_features_dc != nullptr) != (M > 1 ? out->d_features_rest != nullptr : out->d_features_dc != nullptr) || (!fac && !out->d_shs_res && !out->d_features_dc))
                return fail(GSRAST_E_ARG, "backward_raw: give d_features_dc + d_features_rest and / or (with shs_res) d_shs_res, whose rows hold both");
            if (((uintptr_t)out->d_rotation | (uintptr_t)out->d_features_dc | (uintptr_t)out->d_features_rest | (uintptr_t)out->d_shs_res) & 15)
                return fail(GSRAST_E_ARG, "backward_raw: d_rotation / d_features_dc / d_features_rest / d_shs_res must be 16-byte aligned");
            c.means3D = rawin->xyz; c.shs = rawin->features_dc; c.scales = rawin->scaling; c.rotations = rawin->rotation;
            c.dL_dmean2D = out->dL_dmean2D; c.dL_dopacity = out->d_opacity_logit; c.dL_dmean3D = out->d_xyz; c.dL_dscale = out->d_scaling; c.dL_drot = out->d_rotation;
            c.dL_dsh = fac ? out->d_sh_factor : (out->d_shs_res ? out->d_shs_res : out->d_features_dc);      // (a marker, but for the factor)
            raw.motion_res = rawin->motion_res; raw.rot_res = rawin->rot_res; raw.trbf = rawin->trbf; raw.opacity_logit = rawin->opacity_logit;
            raw.features_dc = rawin->features_dc; raw.features_rest = rawin->features_rest; raw.shs_res = rawin->shs_res;
            rawg.d_rot_res = out->d_rot_res; rawg.d_trbf = out->d_trbf; rawg.d_shs_res = out->d_shs_res;
            if (!fac) { rawg.d_dc = out->d_features_dc; rawg.d_rest = out->d_features_rest; }     // (factor: not written, the caller completes them after the exchange)
        }
        if (P < 0 || c.R < 0 || c.width <= 0 || c.height <= 0) return fail(GSRAST_E_ARG, "backward: bad sizes");
        if (P == 0) return GSRAST_OK;
        if (!c.geom_buffer || !c.image_buffer || (c.R > 0 && !c.binning_buffer)) return fail(GSRAST_E_ARG, "backward: NULL state buffer");
        if (!c.means3D || !c.radii || !c.viewmatrix || !c.projmatrix || !c.dL_dpix || !c.background) return fail(GSRAST_E_ARG, "backward: NULL required input");
        if (!c.dL_dmean2D || !c.dL_dopacity || !c.dL_dmean3D) return fail(GSRAST_E_ARG, "backward: NULL gradient output");
        if (c.colors_precomp && !c.dL_dcolor) return fail(GSRAST_E_ARG, "backward: colors_precomp path needs dL_dcolor");
        if (c.dL_dconic && ((uintptr_t)c.dL_dconic & 15)) return fail(GSRAST_E_ARG, "backward: dL_dconic must be 16-byte aligned");
        if (c.rotations && (((uintptr_t)c.rotations | (uintptr_t)c.dL_drot) & 15)) return fail(GSRAST_E_ARG, "backward: rotations / dL_drot must be 16-byte aligned");
        if (c.cov3D_precomp && !c.dL_dcov3D) return fail(GSRAST_E_ARG, "backward: cov3D_precomp path needs dL_dcov3D");
        if (plan.use_sh && (!c.dL_dsh || !c.campos)) return fail(GSRAST_E_ARG, "backward: SH path needs dL_dsh and campos");
        if (plan.use_sr && (!c.scales || !c.rotations || !c.dL_dscale || !c.dL_drot)) return fail(GSRAST_E_ARG, "backward: scale/rotation path needs their gradients");
        if (plan.pose && ((uintptr_t)c.pose_scratch & 15)) return fail(GSRAST_E_ARG, "backward: pose_scratch must be 16-byte aligned");
        cam = make_cam(c.viewmatrix, c.projmatrix, c.campos, c.tan_fovx, c.tan_fovy, c.scale_modifier, c.width, c.height);
        GL = geom_layout((size_t)P); IL = img_layout((size_t)c.width, (size_t)c.height);
        geom = c.geom_buffer; img = c.image_buffer; grec = at<float>(geom, GL.grec);
        return GSRAST_OK;
    }
    int zero_records()
    {
        if (plan.zero_records) GS_HIP(hipMemsetAsync(grec, 0, (size_t)c.P * GREC * sizeof(float), s));
        return GSRAST_OK;
    }
    // What the per-Gaussian backward needs of the SH coefficients -- d(colour)/d(view direction), 36 B instead of 12*M -- depends on
    // nothing the blend backward produces: evaluated on the side stream of the calling thread's context WHILE the VALU-bound blend
    // backward runs, joined in front of preprocess_bwd (or at the end of phase 1 of a two-phase backward).
    // Round 3: the forward's colour kernel leaves those nine floats per Gaussian while it has the coefficient block in LDS
    // (preprocess_color_kernel), so this kernel only runs for a state whose forward was told that no backward would follow
    // (options.forward_only, passed to both calls by a caller that changed its mind).
    // The side stream is forked here, for the zero rows below as well, and the plan gets its answer: inline and ungrouped if it cannot be had.
    int fork_derivs()
    {
        if (plan.derivs && rawin) return fail(GSRAST_E_ARG, "backward_raw: the forward was run with forward_only");
        if (plan.wants_side() && dev && (fork.side = dev->side_stream(thread_context()->mu))) { GS_HIP(hipEventRecord(fork.side->fork, s)); GS_HIP(hipStreamWaitEvent(fork.side->stream, fork.side->fork, 0)); }
        plan.side_answer(fork.side != nullptr);
        if (!plan.derivs) return GSRAST_OK;
        const hipStream_t ds = plan.derivs_on_side ? fork.side->stream : s;
        {
            ProfScope ps(K_SH_DERIVS, ds);
            sh_dir_derivs_kernel<<<plan.derivs_grid, 64, 0, ds>>>(c.P, c.D, c.M, c.means3D, c.shs, c.campos, c.radii,
                                                                  at<float4>(geom, GL.shdA), at<float4>(geom, GL.shdB), at<float>(geom, GL.shdC));
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(GSRAST_E_DEVICE, "sh_dir_derivs", e);
        }
        if (plan.derivs_on_side) GS_HIP(hipEventRecord(fork.side->join, fork.side->stream));
        return GSRAST_OK;
    }
    // List cut (gsrast_common.h): the zero rows of the Gaussians the forward left out are written on the side stream, beside the blend
    // backward; preprocess_bwd then neither reads nor writes them.  Both kernels check on the device that the forward's cut was in force
    // and held.  Only where it pays for the two events (large scenes), with the sparse per-Gaussian backward, in the call that runs it
    // (a one-phase call, or phase 2 of two: a backward with a feature or distortion gradient takes the grouped form like any other).
    int fork_zero_rows()
    {
        if (!plan.late_fill) return GSRAST_OK;
        LateRowsArgs la{}; int n = 0;
        auto add = [&](float* p, int rl) { if (p && rl > 0) { la.ptr[n] = p; la.rowlen[n] = rl; n++; } };
        add(c.dL_dmean2D, 3); add(c.dL_dopacity, 1); add(c.dL_dmean3D, 3); add(c.dL_dconic, 4); add(c.dL_dcolor, 3); add(c.dL_dcov3D, 6);
        if (plan.abs) add(c.dL_dmean2D_abs, 2);
        if (rawin || plan.use_sr) { add(c.dL_dscale, 3); add(c.dL_drot, 4); }
        if (rawin) { add(rawg.d_rot_res, 7); add(rawg.d_trbf, 1); add(rawg.d_shs_res, c.M * 3); add(rawg.d_dc, 3); add(rawg.d_rest, c.M * 3 - 3); }
        else if (plan.use_sh && !o.sh_grad_factors) add(c.dL_dsh, c.M * 3);
        la.n = n;
        if (!plan.skip_zero_rows) {      // (experiments only: the step without the zero rows -- what a caller with persistent outputs could save)
            ProfScope ps(K_LATE_ZERO, fork.side->stream);
            late_rows_zero_kernel<<<GSRAST_LATE_FILL_WGS, 256, 0, fork.side->stream>>>(c.P, at<unsigned long long>(geom, GL.color_skip), at<uint32_t>(geom, GL.scalars), la, at<unsigned char>(geom, GL.untouched));
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(GSRAST_E_DEVICE, "late_rows_zero", e);
        GS_HIP(hipEventRecord(fork.side->join, fork.side->stream));
        return GSRAST_OK;
    }
    int blend()
    {
        if (!plan.blend) return GSRAST_OK;
        ProfScope ps(K_BLEND_BWD, s);
        const uint32_t T = plan.T, grid = ((T + 7) / 8) * 8;
        uint2* ranges = at<uint2>(img, IL.ranges); uint32_t* tm = at<uint32_t>(img, IL.tile_max);
        BlendArgs ba{};
        ba.ranges = ranges; ba.plist = at<uint32_t>(c.binning_buffer, 0) /* BinLayout: point_list lives at offset 0 */; ba.W = c.width; ba.H = c.height; ba.gx = cam.gx; ba.T = T;
        ba.r0 = at<float4>(geom, GL.rec0); ba.r1 = at<float4>(geom, GL.rec1); ba.r2 = at<float4>(geom, GL.rec2);
        ba.bg = c.background; ba.fT = at<float>(img, IL.final_T); ba.nc = at<uint32_t>(img, IL.n_contrib); ba.tm = tm;
        ba.dpix = c.dL_dpix; ba.grec = grec;
        if (plan.aux) { ba.dad = c.dL_dacc_depth; ba.dal = c.dL_dalpha; }      // (either may be null = zero)
        if (plan.mutate & 1) {      // tests only: see mutate_drop_front_batch_kernel
            mutate_drop_front_batch_kernel<<<1, 256, 0, s>>>(ranges, ba.nc, tm, (uint32_t)(cam.gy / 2) * (uint32_t)cam.gx + (uint32_t)(cam.gx / 2), c.width, c.height, cam.gx);
            GS_LAUNCHED("mutate_drop_front_batch");
        }
        if (plan.mutate & 2) {
            static float* zero_bg = nullptr;      // (never freed: a test-only path)
            if (!zero_bg) { GS_HIP(hipMalloc((void**)&zero_bg, 16)); GS_HIP(hipMemset(zero_bg, 0, 16)); }
            ba.bg = zero_bg;
        }
        if (plan.from_buckets) {
            ba.bcnt = at<uint32_t>(img, IL.bucket_cnt); ba.blist = at<uint16_t>(img, IL.bucket_list);
            ba.from_buckets = 1;
        } else if (plan.tile_order) {
            uint32_t* ord = at<uint32_t>(img, IL.order_bwd);
            tile_order_kernel<<<1, 1024, 0, s>>>(T, ranges, tm, ord);
            GS_LAUNCHED("tile_order");
            ba.order = ord;
        }
        launch_blend_bwd(o.exp_mode, plan.pick, grid, s, ba);
        GS_LAUNCHED("blend_bwd");
        return GSRAST_OK;
    }
    int sh_factor()      // dL_dsh is [P][3] in this mode: the factor, final after the blend backward
    {
        if (!plan.sh_factor) return GSRAST_OK;
        sh_factor_kernel<<<(c.P + 255) / 256, 256, 0, s>>>(c.P, c.radii, at<unsigned char>(geom, GL.clamped), reinterpret_cast<const float4*>(grec), c.dL_dsh, at<uint32_t>(geom, GL.scalars), at<unsigned char>(geom, GL.untouched));
        GS_LAUNCHED("sh_factor");
        return GSRAST_OK;
    }
    // In front of the per-Gaussian backward -- or, when the zero rows are all the side stream carries, BEHIND it (plan.join_late): that kernel
    // neither waits for the last zero row nor pays the join's latency in front of it (the table-off step showed it waiting 18 us for a
    // fill that had started later than the blend backward)
    int join()
    {
        if (fork.side) { GS_HIP(hipStreamWaitEvent(s, fork.side->join, 0)); fork.joined = true; }
        return GSRAST_OK;
    }
    int per_gaussian()
    {
        if (!plan.do_geom) return GSRAST_OK;
        ProfScope ps(K_PREPROCESS_BWD, s);
        const int P = c.P;
        const float* cov = c.cov3D_precomp ? c.cov3D_precomp : at<float>(geom, GL.cov3D);
        const float* sh_in = rawin ? c.shs : (plan.use_sh ? c.shs : nullptr);
        const float* sc_in = rawin ? c.scales : (plan.use_sr ? c.scales : nullptr);
        const float* ro_in = rawin ? c.rotations : (plan.use_sr ? c.rotations : nullptr);
        // <RAW, SPARSE, GROUPED, AA, POSE> (aa, pose: the kernel's own instantiations -- the plain ones are the same code as before the flags existed)
        float* const pose_rows = plan.pose ? reinterpret_cast<float*>(c.pose_scratch) : nullptr;
        pick_bool(rawin != nullptr, [&](auto raw_c) { pick_bool(plan.aa, [&](auto aa_c) { pick_bool(plan.pose, [&](auto pose_c) {
            auto launch = [&](auto sparse_c, auto grouped_c) {
                preprocess_bwd_kernel<decltype(raw_c)::value, decltype(sparse_c)::value, decltype(grouped_c)::value, decltype(aa_c)::value, decltype(pose_c)::value><<<plan.per_gaussian_grid, PP_THREADS, 0, s>>>(
                    P, c.D, c.M, c.means3D, c.radii, raw, rawg, sh_in, at<unsigned char>(geom, GL.clamped), at<float4>(geom, GL.shdA), at<float4>(geom, GL.shdB),
                    at<float>(geom, GL.shdC), sc_in, ro_in, cov, cam, reinterpret_cast<const float4*>(grec), c.dL_dmean2D, c.dL_dconic, c.dL_dopacity, c.dL_dcolor,
                    c.dL_dmean3D, c.dL_dcov3D, c.dL_dsh, c.dL_dscale, c.dL_drot, plan.factors, (plan.late_fill ? at<unsigned long long>(geom, GL.color_skip) : nullptr), at<uint32_t>(geom, GL.scalars), at<unsigned char>(geom, GL.untouched),
                    plan.aux ? 1 : 0, at<float4>(geom, GL.rec1), plan.abs ? c.dL_dmean2D_abs : nullptr, pose_rows);
            };
            // (grouped implies sparse)
            if (plan.grouped) launch(std::true_type{}, std::true_type{});
            else pick_bool(plan.sparse, [&](auto sparse_c) { launch(sparse_c, std::false_type{}); });
        }); }); });
        GS_LAUNCHED("preprocess_bwd");
        if (plan.pose) {      // the workgroups' rows -> dL_dcamera, one workgroup, a fixed order (inside the kernel timer: it is part of the per-Gaussian backward)
            pose_grad_reduce_kernel<<<1, 1024, 0, s>>>(plan.per_gaussian_grid, pose_rows, c.dL_dcamera);
            GS_LAUNCHED("pose_grad_reduce");
        }
        return GSRAST_OK;
    }
};
} // namespace

// The one backward: checks -> plan -> zero-fill -> [fork: direction derivatives, zero rows] -> blend backward -> factor -> join and
// per-Gaussian backward, in the order the plan says
static int backward_impl(const gsrast_options* options, const gsrast_backward_call& c)
{
    RoctxRange range_bwd(c.family == GSRAST_FAMILY_RAW ? "gsrast_backward" "_raw" : "gsrast_backward");
    BackwardRun r(options, c);
    int rc = r.check_and_plan();
    if (rc == GSRAST_OK && c.P == 0 && r.plan.pose && r.o.backward_phase != 1 && hipMemsetAsync(c.dL_dcamera, 0, POSE_OUT * sizeof(float), r.s) != hipSuccess)
        return fail(GSRAST_E_DEVICE, "backward: dL_dcamera of an empty scene");      // (no Gaussian: the camera's gradient is zero, written like any other)
    if (rc != GSRAST_OK || c.P == 0) return rc;
    if ((rc = r.zero_records()) != GSRAST_OK || (rc = r.fork_derivs()) != GSRAST_OK || (rc = r.fork_zero_rows()) != GSRAST_OK) return rc;
    if ((rc = r.blend()) != GSRAST_OK || (rc = r.sh_factor()) != GSRAST_OK) return rc;
    if (!r.plan.join_late && (rc = r.join()) != GSRAST_OK) return rc;
    if ((rc = r.per_gaussian()) != GSRAST_OK) return rc;
    return r.plan.join_late ? r.join() : GSRAST_OK;
}

// ---- the exported backwards: the record call, and the reference-shaped positional one that fills a record by name ----
int gsrast_render_backward(const gsrast_options* options, const gsrast_backward_call* call)
{
    gsrast_backward_call c;
    if (const char* e = take_record(&c, sizeof c, call, GSRAST_BACKWARD_CALL_MIN)) return fail(GSRAST_E_ARG, e);
    if (!family_known(c.family)) return fail(GSRAST_E_ARG, "call record: unknown family");
    if (c.family == GSRAST_FAMILY_DENSE ? c.raw || c.raw_grads
                                        : c.means3D || c.shs || c.colors_precomp || c.scales || c.rotations || c.cov3D_precomp || c.dL_dmean2D || c.dL_dconic ||
                                          c.dL_dopacity || c.dL_dcolor || c.dL_dmean3D || c.dL_dcov3D || c.dL_dsh || c.dL_dscale || c.dL_drot)
        return fail(GSRAST_E_ARG, "call record: dense family with raw / raw_grads set, or raw family with a dense input / gradient output set");
    return backward_impl(options, c);
}

int gsrast_backward(int P, int D, int M, int R, const float* background, int width, int height,
                    const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                    float scale_modifier, const float* rotations, const float* cov3D_precomp,
                    const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                    float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                    const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, void* stream)
{
    gsrast_backward_call c{};
    c.struct_size = GSRAST_BACKWARD_CALL_MIN; c.family = GSRAST_FAMILY_DENSE;
    c.P = P; c.D = D; c.M = M; c.R = R; c.background = background; c.width = width; c.height = height;
    c.means3D = means3D; c.shs = shs; c.colors_precomp = colors_precomp; c.scales = scales; c.rotations = rotations; c.cov3D_precomp = cov3D_precomp;
    c.scale_modifier = scale_modifier; c.viewmatrix = viewmatrix; c.projmatrix = projmatrix; c.campos = campos; c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy;
    c.radii = radii; c.geom_buffer = geom_buffer; c.binning_buffer = binning_buffer; c.image_buffer = image_buffer; c.dL_dpix = dL_dpix;
    c.dL_dmean2D = dL_dmean2D; c.dL_dconic = dL_dconic; c.dL_dopacity = dL_dopacity; c.dL_dcolor = dL_dcolor; c.dL_dmean3D = dL_dmean3D;
    c.dL_dcov3D = dL_dcov3D; c.dL_dsh = dL_dsh; c.dL_dscale = dL_dscale; c.dL_drot = dL_drot; c.stream = stream;
    return backward_impl(nullptr, c);
}

// One row of POSE_ROW floats per workgroup of the per-Gaussian backward, sized for its larger grid (the plain form: PP_THREADS Gaussians each)
size_t gsrast_pose_scratch_bytes(int P) { return P > 0 ? (((size_t)P + PP_THREADS - 1) / PP_THREADS) * POSE_ROW * sizeof(float) : (size_t)POSE_ROW * sizeof(float); }

int gsrast_debug_export(int P, int R, int width, int height, const char* geom_buffer, const char* binning_buffer,
                        const char* image_buffer, float* depths, float* means2D, float* cov3D, float* conic_opacity,
                        float* rgb, unsigned char* clamped, uint32_t* tiles_touched, uint64_t* keys_sorted,
                        uint32_t* point_list, uint32_t* ranges, float* final_T, uint32_t* n_contrib, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (P <= 0 || !geom_buffer) return fail(GSRAST_E_ARG, "debug_export: bad arguments");
    if (cov3D && !g_opt.debug_state.load()) return fail(GSRAST_E_ARG, "debug_export: cov3D is only kept by forwards run with gsrast_set_option(\"debug_state\", 1)");
    const GeomLayout GL = geom_layout((size_t)P);
    const ImgLayout IL = img_layout((size_t)width, (size_t)height);
    const uint32_t T = (uint32_t)((width + TILE_X - 1) / TILE_X) * (uint32_t)((height + TILE_Y - 1) / TILE_Y);
    export_geom_kernel<<<(P + 255) / 256, 256, 0, s>>>(
        P, at<float4>(geom_buffer, GL.rec0), at<float4>(geom_buffer, GL.rec1),
        at<float4>(geom_buffer, GL.rec2), at<float>(geom_buffer, GL.cov3D), at<unsigned char>(geom_buffer, GL.clamped),
        at<uint32_t>(geom_buffer, GL.tiles), depths, means2D, cov3D, conic_opacity, rgb, clamped, tiles_touched);
    GS_LAUNCHED("export_geom");
    if (R > 0 && binning_buffer && image_buffer && (keys_sorted || point_list)) {
        export_keys_kernel<<<T, 256, 0, s>>>(at<uint2>(image_buffer, IL.ranges), at<uint32_t>(binning_buffer, 0),
                                             at<float4>(geom_buffer, GL.rec1), keys_sorted, point_list, (uint32_t)R);
        GS_LAUNCHED("export_keys");
    }
    if (image_buffer) {
        const size_t N = (size_t)width * height;
        if (ranges) GS_HIP(hipMemcpyAsync(ranges, image_buffer + IL.ranges, (size_t)T * 8, hipMemcpyDeviceToDevice, s));
        if (final_T) GS_HIP(hipMemcpyAsync(final_T, image_buffer + IL.final_T, N * 4, hipMemcpyDeviceToDevice, s));
        if (n_contrib) GS_HIP(hipMemcpyAsync(n_contrib, image_buffer + IL.n_contrib, N * 4, hipMemcpyDeviceToDevice, s));
    }
    return GSRAST_OK;
}

} // extern "C"

#ifdef GSRAST_SCATTER_TIMING
extern "C" int gsrast_debug_scatter_timing(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gsrast::g_scat), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; z[14] = ~0ull; if (hipMemcpyToSymbol(HIP_SYMBOL(gsrast::g_scat), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
#if defined(GSRAST_DEBUG_COUNTERS) || defined(GSRAST_DEBUG_TIMING)
extern "C" int gsrast_debug_counters(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gsrast::g_dbg), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; z[11] = ~0ull /* (a minimum) */; if (hipMemcpyToSymbol(HIP_SYMBOL(gsrast::g_dbg), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif
