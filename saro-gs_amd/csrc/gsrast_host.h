// gsrast_host.h -- what every entry point of the C ABI needs on the host, whichever unit it lives in (gsrast_capi.hip: the renderer;
// gsrast_train.hip: the training kernels' calls).  Whatever is declared here without a body is defined ONCE, in gsrast_capi.hip: the process
// has one error text per thread, one option table, one timer table, one roctx lookup.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include <type_traits>
#include "../../include/gsrast.h"

namespace gsrast {

// the offsets of a state / scratch layout: every array starts on a 256-byte boundary
struct Carver {
    size_t o = 0;      // the next free offset
    size_t take(size_t bytes) { const size_t r = o; o = (o + bytes + 255) & ~(size_t)255; return r; }
};

// ---- errors (the text gsrast_last_error returns), launch checks ----
int fail(int code, const char* what, hipError_t e = hipSuccess);
inline int refuse(const char* who, const char* what)      // GSRAST_E_ARG with the text "<who>: <what>": the checks several entry points share
{
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return fail(GSRAST_E_ARG, msg);
}
#define GS_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) return ::gsrast::fail(GSRAST_E_DEVICE, #call, e_);      \
    } while (0)
int post_launch(const char* what, hipStream_t s);      // the launch's error; with option debug_sync (or GSRAST_DEBUG_SYNC in the environment) also a wait for the stream
#define GS_LAUNCHED(what)                                 \
    do {                                                  \
        int rc_ = ::gsrast::post_launch(what, s);         \
        if (rc_ != GSRAST_OK) return rc_;                 \
    } while (0)

// ---- the process-wide words of gsrast_set_option (the table that names them: kOptions, gsrast_capi.hip) ----
struct OptionWords {
    std::atomic<int> exp_mode, binning, tile_clip, cull, lpt, speculative, fwd_pixels_per_lane, bwd_pixels_per_lane, sh_grad_factors, side_stream, depth_sort, forward_only,
                     no_order_hint, dense_backward, no_list_cut, profile, debug_sync, debug_state, ablate, mutate, list_cut_always, chain_gate, touch_bits, sparse_grec,
                     late_fill_min_p, tau_sample, tau_cut, two_level, two_level_min_p, sort_hint, bwd_transposed, hexplane_scatter;
    OptionWords();      // (stores the table's defaults)
};
extern OptionWords g_opt;
gsrast_options snapshot_defaults();      // the per-call options of an entry point that was handed none: the process defaults, loaded once

// ---- per-kernel device timing (option "profile"; read with gsrast_profile_read) ----
enum KernelId { K_PREPROCESS_FWD, K_SORT_DEPTH, K_SCAN_TILES, K_EMIT, K_SORT_TILE, K_RANGES, K_BLEND_FWD,
                K_BLEND_BWD, K_PREPROCESS_BWD, K_MARK_VISIBLE, K_LOSS_FWD, K_LOSS_BWD, K_COLOR, K_SH_DERIVS, K_CUT_REDO, K_LATE_ZERO, K_GREC_ZERO,
                K_DENSIFY_CLASSIFY, K_DENSIFY_SCAN, K_DENSIFY_APPLY, K_DENSIFY_STATS, K_CONTRIB_BLEND, K_CONTRIB_FINISH, K_FEATURES_FWD, K_FEATURES_BWD, K_DISTORT_FWD, K_DISTORT_BWD, K_ADAM_VISIBLE,
                K_MCMC_PLAN, K_MCMC_SAMPLE, K_MCMC_APPLY, K_MCMC_NOISE, K_MLP_FWD, K_MLP_BWD, K_COUNT };
// option "profile" is one 32-bit word, a bit per kernel id: ids 0 .. 31 have a bit of their own, the ids behind them are timed when the word is -1 (all)
static_assert(K_MCMC_NOISE == 31, "the ids with a bit of their own");
struct RoctxRange { bool on; explicit RoctxRange(const char* name); ~RoctxRange(); };      // a named range around the host's ENQUEUE of a stage (GSRAST_ROCTX)
struct ProfScope {      // a stage of kernel id `id` on stream `s`: its roctx range, and a pair of events around it when the id's profile bit is set
    int id; hipStream_t s; hipEvent_t a = nullptr, b = nullptr; bool on; RoctxRange range;
    ProfScope(int id_, hipStream_t s_);
    ~ProfScope();
};

template <typename T> T* at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }
template <typename T> const T* at(const char* base, size_t off) { return reinterpret_cast<const T*>(base + off); }

// ---- kernel selection: a runtime value -> the template instantiation.  f is called with the std::integral_constant of the V that equals v
// (of the last V if none does); a generic lambda instantiates its kernel only for the constants it is called with. ----
template <int V> using int_c = std::integral_constant<int, V>;
template <int V, int... Vs, class F>
void pick_int(int v, F&& f)
{
    if constexpr (sizeof...(Vs) == 0) f(int_c<V>{});
    else if (v == V) f(int_c<V>{});
    else pick_int<Vs...>(v, f);
}
template <class F>
void pick_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// ---- the radix sort (gsrast_capi.hip: radix_sort) of uint32 (key, value) pairs for callers outside the renderer's unit: its kernels live in
// gsrast_binning.h, which that unit alone includes.  The result is in (kA, vA) if radix_passes(bits) is even, else in (kB, vB). ----
int radix_passes(int bits);
int sort_pairs_small(uint32_t* kA, uint32_t* vA, uint32_t* kB, uint32_t* vB, uint32_t n, int bits, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s);   // GSRAST_DEPTH_ITEMS elements per lane (k-NN: Morton codes)
int sort_pairs_large(uint32_t* kA, uint32_t* vA, uint32_t* kB, uint32_t* vB, uint32_t n, int bits, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s);   // RS_ITEMS elements per lane (hexplane: texel keys)

} // namespace gsrast
