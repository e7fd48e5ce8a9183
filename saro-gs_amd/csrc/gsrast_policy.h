// gsrast_policy.h -- the HOST-side decisions of a render call, free of any HIP call: when the list cut is applied, paused and widened, how
// the speculative launch is sized, how the depth histogram's range follows the scene, when the bucket depth sort backs off to the radix passes, which path a call takes (ForwardPlan, BackwardPlan).  gsrast_capi.hip
// enqueues; this file decides.  Everything here runs on a CPU box: tests/test_policy.py drives it through gsrast_policy_event(),
// gsrast_debug_forward_plan() and gsrast_debug_backward_plan() (include/gsrast.h), which touch no device.  No result of a call depends on any of it -- only how much work the call enqueues.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include "../../include/gsrast.h"   // (gsrast_options, GSRAST_RENDER_*)
#include "gsrast_common.h"     // (the depth histogram's bin geometry: ZH_*, zh_bin_start)
#include "gsrast_preprocess.h" // (the per-Gaussian backward's workgroup sizes: PP_THREADS, PB_GROUP)

namespace gsrast {

// counters of "that many forwards go without ..." shared by the lanes of a view-parallel caller: never below zero
inline void dec_to_zero(std::atomic<int>& a) { int v = a.load(); while (v > 0 && !a.compare_exchange_weak(v, v - 1)) { } }

// ---- the list cut's policy (gsrast_common.h: LIST CUT, PREDICTED CUT) ----------------------------------------------------------------
// The cut costs ~80 us per forward (the late test in the scatter, the compacting colour kernel, the predicated launches behind the blend)
// and saves ~50 us per million column runs it removes (measured with the cut forced on: 1 M-Gaussian shell -7 %, 0.3 M cube -3 %, 0.1 M cube -8 %; 1 M cube +8 %, 3 M cube +16 %).
struct CutPolicy {
    static constexpr uint32_t MIN_RUNS = 1500000u;     // it is applied when the context's last forward had at least this many column runs
    static constexpr int PAUSE = 64;                   // forwards a context sits out after SMALL_STREAK cut forwards that removed fewer than MIN_RUNS
    static constexpr int SMALL_STREAK = 4;
    static constexpr int MARGIN_MIN = 6, MARGIN_MAX = 16;   // the next remembered cut sits (margin / 4) x as deep as the deepest entry consumed: 1.5 x ... 4 x
    static constexpr int TAU_MIN = 10, TAU_MAX = 96;        // mean optical depth a tile must have gathered in front of a PREDICTED cut (T < 1e-4 needs 9.2 at EVERY pixel; measured on
                                                            // the 3 M cube, 8 poses: no completion pass down to 8 -- the far bin edge and the 3 x 3 maximum are the slack --, passes at 4)
    static constexpr int TAU_FORCE = 512;                   // forwards that use predicted cut depths for every pose after a remembered one failed widely

    std::atomic<int> pause{0};             // > 0: that many forwards go without the cut ...
    std::atomic<uint32_t> pause_P{0};      // ... in a scene of this many Gaussians (another scene: the pause is void)
    // A cut list that turns out too short is completed by the pass behind the blend; the device reports each pass with its size.  Small
    // passes (up to an eighth of all column runs) are what the speculation is expected to cost; a quarter and more counts like a whole
    // second forward (8 points), in between in proportion.  16 points pause the cut -- 64 forwards, twice as long each further time (at
    // most 1024; after a pause the score restarts at 8: ONE more large pass pauses again), 64 cut forwards without a pass forget.
    std::atomic<int> fb_score{0}, fb_pause{0}, ok_streak{0}, small_streak{0};
    // Every reported pass widens the remembered cut's margin by half a step and raises the predicted cut's requirement by 8; 128 (64) cut
    // forwards without one take a quarter step (2) back.  A pass of 2 points or more while predicted cuts are available switches every
    // pose to them for TAU_FORCE forwards: the scene is another one at every visit, its remembered cuts are not to be trusted.
    std::atomic<int> margin{MARGIN_MIN}, margin_streak{0}, tau_req{TAU_MIN}, tau_force{0}, tau_streak{0}, tau_min{TAU_MIN};
    // ... and so does a RUN of small ones: every pass, whatever its size, is a chain of a dozen dependent launches the caller's stream waits
    // for (~0.1 ms); +8 per pass, -1 per clean cut forward, 24 = roughly one pass in six forwards for a while
    std::atomic<int> pass_rate{0};
    std::atomic<uint32_t> passes_reported{0};

    std::atomic<uint32_t> scene_P{0};      // the size of the scene the adaptive state above was learned on
    // start of a forward over P Gaussians: what the policy has learned belongs to the scene (size) it learned it on -- a pause, a widened
    // margin, a raised requirement, a switch to predicted cuts earned on one scene are void on another (a context that moves from a 3 M scene
    // to a 1 M one must not render the second with the first's scars: bench.py's sweep, a caller with several models)
    // Returns true when the scene is another one than the last forward's (the caller then also forgets the pose table's entries: cut
    // depths remembered for a pose of the OLD scene are running maxima and would take eight visits to fade).
    bool begin_forward(uint32_t P)
    {
        const uint32_t pp = pause_P.load();
        if (pause.load() > 0 && (pp > P ? pp - P : P - pp) > pp / 8) pause = 0;
        const uint32_t sp = scene_P.load();
        if (sp == 0u) { scene_P = P; return false; }
        if ((sp > P ? sp - P : P - sp) > sp / 8) {
            scene_P = P;
            fb_score = 0; fb_pause = 0; ok_streak = 0; small_streak = 0; margin = MARGIN_MIN; margin_streak = 0;
            tau_req = tau_min.load(); tau_force = 0; tau_streak = 0; pass_rate = 0;
            return true;
        }
        return false;
    }
    bool pays(uint32_t last_Q, bool always) const { return always || (last_Q >= MIN_RUNS && pause.load() == 0); }
    void sits_out() { dec_to_zero(pause); }             // a forward without the cut serves one forward of a pause
    bool forced_prediction() { const bool f = tau_force.load() > 0; dec_to_zero(tau_force); return f; }
    // the counts of a cut forward: Q column runs in all, Q_early listed
    void forward_counts(bool predicted_available, uint32_t n_late, uint32_t Q, uint32_t Q_early, uint32_t P, bool always)
    {
        if (always) return;
        if ((n_late != 0u || predicted_available) && Q - Q_early < MIN_RUNS) {
            if (++small_streak >= SMALL_STREAK) { small_streak = 0; pause = PAUSE; pause_P = P; }
        } else small_streak = 0;
    }
    static int pass_points(uint32_t q2, uint32_t qall)
    {
        qall = std::max(qall, 8u);
        const uint32_t lo = qall / 8u;
        return q2 <= lo ? 0 : (int)std::min<uint64_t>(8u, ((uint64_t)(q2 - lo) * 8u + lo - 1u) / lo);
    }
    // the device reported a completion pass over q2 column runs of candidates (of qall in the forward); returns its points
    int completion_pass(uint32_t q2, uint32_t qall, uint32_t P, bool always, bool predicted_available)
    {
        const int pts = pass_points(q2, qall);
        passes_reported++;
        if (pts == 0 && fb_score.load() > 0) fb_score--;
        if (pts >= 4) ok_streak = 0;
        { const int m = margin.load(); if (m < MARGIN_MAX) margin = std::min(MARGIN_MAX, m + 2); margin_streak = 0; }
        { const int r = tau_req.load(); if (r < TAU_MAX) tau_req = std::min(TAU_MAX, r + 8); tau_streak = 0; }
        if (predicted_available && (pts >= 2 || (pass_rate += 8) >= 24)) { tau_force = TAU_FORCE; pass_rate = 0; }
        if ((fb_score += pts) >= 16 && !always) {
            const int prev = fb_pause.load(), len = prev <= 0 ? 64 : (prev >= 512 ? 1024 : prev * 2);
            fb_pause = len; pause = len; pause_P = P; fb_score = 8;
        }
        return pts;
    }
    // a cut forward (late Gaussians > 0) behind which no pass was reported
    void clean_cut_forward()
    {
        if (fb_score.load() > 0) fb_score--;
        dec_to_zero(pass_rate);
        if (++ok_streak >= 64) fb_pause = 0;
        if (++margin_streak >= 128) { margin_streak = 0; const int m = margin.load(); if (m > MARGIN_MIN) margin = m - 1; }
        if (++tau_streak >= 64) { tau_streak = 0; const int r = tau_req.load(), lo = tau_min.load(); if (r > lo) tau_req = std::max(lo, r - 2); }
    }
};

// ---- the depth histogram's key range (gsrast_common.h: equalised depth buckets; the predicted cut's bins) ------------------------------
// The MIDDLE of the next forward's histogram covers this one's occupied key range padded by an eighth on either side (the tails beyond take
// a view a whole range away); the range widens at once and narrows by an eighth of the gap per forward (consecutive forwards render
// different views).  khi is the upper end BEFORE the bins' width is rounded up to a power of two: the predicted cut's 32 bins span [klo, khi].
struct DepthRange {
    std::atomic<uint32_t> klo{ZH_KLO_DEFAULT}; std::atomic<int> shift{ZH_SHIFT_DEFAULT}; std::atomic<uint32_t> khi{0};
    bool coarse() const { return shift.load() == ZH_SHIFT_DEFAULT && klo.load() == ZH_KLO_DEFAULT; }      // nothing learned yet: 4 bins per octave over every finite float
    // zb = first | last << 16 occupied bin of the histogram a forward filled with the table (call_klo, call_shift); 0xFFFFFFFF: no sample.
    // Returns whether that table was a learned one that held every key (an overflow of the depth buckets is then the scene's doing).
    bool learn(uint32_t zb, uint32_t call_klo, int call_shift)
    {
        if (zb == 0xFFFFFFFFu) return true;
        const uint32_t first = zb & 0xFFFFu, last = zb >> 16;
        const long long top = ZH_KEY_TOP, bot = ZH_KLO_DEFAULT;
        long long kmin = std::max(zh_bin_start(first, call_klo, call_shift), bot), kmax = std::min(zh_bin_start(last + 1u, call_klo, call_shift), top);
        if (kmax <= kmin) kmax = kmin + 1;
        const long long span = kmax - kmin;
        const bool was_coarse = call_shift == ZH_SHIFT_DEFAULT && call_klo == ZH_KLO_DEFAULT;
        const bool clipped = first == 0u || last >= (uint32_t)ZH_BINS - 1u;          // keys may lie beyond the table's tails
        const long long pad_lo = first == 0u ? 4 * span : span / 8 + 1, pad_hi = last >= (uint32_t)ZH_BINS - 1u ? 4 * span : span / 8 + 1;
        long long lo = std::max(kmin - pad_lo, bot), hi = std::min(kmax + pad_hi, top);
        if (!was_coarse) {      // (against the previous range -- its UN-rounded upper end if known: measured against the rounded one the range never narrowed below half the table)
            const uint32_t khi_prev = khi.load();
            const long long plo = call_klo, phi = khi_prev > call_klo ? (long long)khi_prev : (long long)call_klo + ((long long)ZH_MID << call_shift);
            lo = lo < plo ? lo : plo + (lo - plo) / 8;
            hi = hi > phi ? hi : phi - (phi - hi) / 8;
        }
        int sh = 0;
        while (((hi - lo) >> sh) >= (long long)ZH_MID) sh++;
        klo = (uint32_t)lo; shift = sh; khi = (uint32_t)hi;
        return !was_coarse && !clipped;
    }
};

// ---- the bucket depth sort's back-off (gsrast_binning.h: a bucket overflowed -- more Gaussians at (nearly) one depth than it holds) ----
// An ISOLATED overflow (32 clean forwards before it: one pose of a cycle whose depth profile has a hard edge inside a histogram bin, which
// doubles a few buckets' share and now and then tips one over) costs that forward its repeat and nothing else.  Overflows in quick
// succession start with the radix passes for a while -- exponential back-off: 16 radix forwards, twice as many after each further one (a
// scene whose depths pile up for good pays the discarded speculative launch ever more rarely), capped at 4096 -- unless the histogram
// behind the bucket map was not up to the view (a context's first forward: four bins per octave; a depth range that has moved out of the
// table): the range is learned from that call, the next forward tries again at once.  64 clean forwards forget the length.
struct DepthSortPolicy {
    std::atomic<int> skip{0};         // > 0: that many forwards go straight to the radix sort ("bucket_skip")
    std::atomic<int> backoff{0}, clean{0};   // length of the last such pause (doubles per overflow), bucket-sorted forwards without an overflow since (saturates at 1024)
    std::atomic<int> depth_short{0};  // the last radix-sorted forward's depth keys spanned < 2^24: the next one enqueues three sort passes, not four
    // a forward that went to the radix sort although the caller asked for the bucket sort serves one forward of the pause
    void radix_forward() { dec_to_zero(skip); }
    void clean_forward() { if (clean.load() < 1024 && ++clean >= 64) backoff = 0; }      // the scene changed: forget
    // table_held: the histogram's table was a learned one that held every key (DepthRange::learn's return).  Returns the pause.
    int overflow(bool table_held)
    {
        const int clean_before = clean.exchange(0);
        if (table_held && (clean_before < 32 || backoff.load() > 0)) {
            const int prev = backoff.load(), next = prev <= 0 ? 16 : (prev >= 2048 ? 4096 : prev * 2);
            backoff = next; skip = next;
        }
        depth_short = 0;   // the radix path's pass-count hint is stale (not refreshed on the bucket path): assume four passes
        return skip.load();
    }
    void radix_key_bits(uint32_t bits) { depth_short = bits <= 24u ? 1 : 0; }      // after a radix sort with adaptive pass count
};

// ---- capacities of the speculative launch --------------------------------------------------------------------------------------------
// The binning buffer is requested for 1.25 x (+ 4096) the hint BEFORE the host knows the counts; a hint follows the largest recent count
// and decays by 1 / 2^shift per forward (consecutive forwards render different views).
inline uint32_t grow_capacity(uint32_t v) { const uint64_t w = (uint64_t)v + v / 4 + 4096; return w > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)w; }
inline uint32_t follow_hint(uint32_t hint, uint32_t now, int shift) { const uint32_t d = hint - (hint >> shift); return now > d ? now : d; }
// column runs the launches over the CUT lists are sized for: half again as much as the largest early set of recent forwards of the same kind
// (remembered / predicted cut depths), all runs when nothing is known about this call's early set
inline uint32_t early_launch_runs(uint32_t qe_hint, uint32_t capQ, bool early_set_expected)
{
    if (!qe_hint || !early_set_expected) return capQ;
    return (uint32_t)std::min<uint64_t>(capQ, (uint64_t)qe_hint + qe_hint / 2 + 4096);
}

// ---- the forward's plan ----------------------------------------------------------------------------------------------------------------
// Every decision of a forward call that follows from its options, flags and shape, the context's remembered words and the process-wide
// switches: made ONCE, at the top of the call, from one snapshot of them (plan_forward).  What needs an answer from the policy or the device
// is a second-phase field, written by the one *_answer function below.  tests/test_policy.py reads the plan through gsrast_debug_forward_plan.
inline bool options_valid(const gsrast_options& o)
{
    auto ppl_ok = [](int v) { return v == 0 || v == 1 || v == 2 || v == 4; };
    return o.exp_mode >= 0 && o.exp_mode <= 2 && (o.binning == 0 || o.binning == 1) && ppl_ok(o.fwd_pixels_per_lane) && ppl_ok(o.bwd_pixels_per_lane) &&
           o.backward_phase >= 0 && o.backward_phase <= 2 && (o.depth_sort == 0 || o.depth_sort == 1) && (o.dense_backward == 0 || o.dense_backward == 1);
}
// "the culled blend kernel runs".  Forward: a forced pixels-per-lane selects the un-culled template; backward: it picks among the culled ones.
inline bool culled_blend(const gsrast_options& o, bool backward) { return o.cull != 0 && (backward || o.fwd_pixels_per_lane == 0); }
struct PlanSwitches { bool list_cut_always, tau_cut, touch_bits, sparse_grec, two_level, chain_gate, sort_hint, debug_state; int two_level_min_p, tau_sample;      // the process-wide A/B switches, read once per call
                      bool bwd_transposed; int late_fill_min_p, ablate, mutate; };                                                                                  // ... the backward's
struct PlanInputs { unsigned flags; int P, W, H, D; bool sh, colors_precomp; int bucket_skip; uint32_t R_hint, last_Q; bool depth_short; };      // the call's shape; the context's words
struct ForwardPlan {
    const char* refusal = nullptr;      // GSRAST_E_ARG with this text: unknown flags, a bad option value, aux without the culled kernel (in this order)
    bool aux = false, aa = false;
    bool runbin = false, buckets_ok = false;          // run-compressed binning (one 8-bit pass over tile rows, 16-bit tile ids); the blends' launch order from work buckets (u16 tile ids)
    bool bucket_sort = false, two_level = false;      // depth order by the bucket sort (else radix); its scatter as two launches, coarse + refine
    bool culled = false, ordered = false;             // the culled blend kernel runs; ... heaviest tiles first
    bool want_hints = false, cut_base = false;        // the context's launch-order hints are asked for; list cut: everything it needs but the policy's and the pose table's answer
    bool tau_mode = false;                            // predicted cut depths for a pose without remembered ones
    bool zero_in_blend = false, zero_touched = false; // the gradient records are zeroed inside the blend / only the consumed Gaussians', behind it
    bool keep_untouched = false, clip = false, want_shd = false;      // GeomLayout::untouched is kept for the backward; clipped tile rectangles; d(colour)/d(view direction) stored
    bool spec_eligible = false;                       // binning + blend may be enqueued before the counts are known
    bool adaptive_sort = false, assume_short = false; // the radix depth sort adapts its pass count on the device; three passes are enqueued
    bool list_cut_always = false, chain_gate = false, debug_state = false; uint32_t tau_sample_mask = 0, T = 0, R_hint = 0, last_Q = 0; int cut_cs = 0;
    // second phase: the policy's answer; prediction; the device's word on the pose (only the early Gaussians' colours are evaluated); the binning buffer
    bool cut_pays = false, cut = false, tau_forced = false, tau_on = false, pose_known = true, cut_colors = false, speculative = false;
    void policy_answer(bool pays, bool hints_acquired) { cut_pays = pays; cut = cut_base && pays && (hints_acquired || tau_mode); }
    void prediction_answer(bool forced, bool pose_expected) { tau_forced = forced; tau_on = cut && tau_mode && !pose_expected; }
    // (a pose without a slot has no cut depths: unless predicted ones stand in, every visible Gaussian is early and the plain colour kernel
    // evaluates them; not under debug_state: gsrast_debug_export shows every Gaussian's colour)
    void pose_answer(bool known) { pose_known = known; cut_colors = cut && zero_in_blend && !debug_state && (known || tau_on); }
    void binning_answer(bool have_buffer) { speculative = spec_eligible && have_buffer; }
};
inline ForwardPlan plan_forward(const gsrast_options& o, const PlanInputs& in, const PlanSwitches& g)
{
    ForwardPlan p;
    p.aux = (in.flags & GSRAST_RENDER_AUX) != 0; p.aa = (in.flags & GSRAST_RENDER_ANTIALIAS) != 0;
    p.culled = culled_blend(o, false);
    if (in.flags & ~(unsigned)(GSRAST_RENDER_AUX | GSRAST_RENDER_ANTIALIAS)) p.refusal = "flags: unknown bits";      // (GSRAST_RENDER_ABSGRAD is a backward's bit)
    else if (!options_valid(o)) p.refusal = "forward: bad option value";
    else if (p.aux && !p.culled) p.refusal = "forward: acc_depth / alpha need the culled blend kernel (options.cull != 0, fwd_pixels_per_lane == 0)";
    if (p.refusal || in.P <= 0 || in.W <= 0 || in.H <= 0) return p;      // (the shape is refused, or nothing is rendered)
    p.list_cut_always = g.list_cut_always; p.tau_mode = g.tau_cut; p.chain_gate = g.chain_gate; p.debug_state = g.debug_state;
    p.tau_sample_mask = (1u << g.tau_sample) - 1u; p.R_hint = in.R_hint; p.last_Q = in.last_Q;
    const size_t P = (size_t)in.P, gx = ((size_t)in.W + TILE_X - 1) / TILE_X, gy = ((size_t)in.H + TILE_Y - 1) / TILE_Y;
    p.T = (uint32_t)gx * (uint32_t)gy;
    p.runbin = o.binning == 0 && gy <= 256 && p.T <= 65536u;
    p.buckets_ok = p.T <= BUCKET_MAX_TILES;
    p.bucket_sort = p.runbin && o.depth_sort == 0 && P >= BUCKET_SORT_MIN_P && in.bucket_skip == 0;
    p.two_level = p.bucket_sort && g.two_level && P >= (size_t)g.two_level_min_p;
    p.ordered = p.culled && o.lpt != 0;
    const bool bucket_order = p.runbin && p.buckets_ok && p.ordered;
    p.want_hints = bucket_order && !o.no_order_hint;
    // (the cut lists are blended by the speculative launch: a capacity hint is needed; the verified fallback is enqueued behind it)
    p.cut_cs = cut_cell_shift(gx, gy);
    p.cut_base = bucket_order && p.bucket_sort && o.tile_clip != 0 && !o.no_list_cut && p.cut_cs != 0 && o.speculative != 0 && in.R_hint != 0;
    p.zero_in_blend = p.culled && P * 4 <= 0xFFFFFFFFull;
    p.keep_untouched = p.culled && !o.forward_only && g.touch_bits;      // ... unless no backward will follow
    p.zero_touched = p.keep_untouched && p.zero_in_blend && g.sparse_grec;
    p.clip = p.runbin && o.tile_clip != 0;
    p.want_shd = in.sh && !in.colors_precomp && in.D > 0 && !o.forward_only;
    p.spec_eligible = p.runbin && o.speculative != 0;
    p.adaptive_sort = rs_blocks_n(P, GSRAST_DEPTH_ITEMS) > RS_SELF_SCAN_BLOCKS;      // see radix_sort
    p.assume_short = p.adaptive_sort && g.sort_hint && in.depth_short;
    return p;
}

// ---- the backward's plan ---------------------------------------------------------------------------------------------------------------
// The same for a backward call: everything that follows from its options, flags and shape, the kind of its inputs and the one snapshot of the
// switches (plan_backward).  Whether the context's side stream could be had is the one second-phase answer (side_answer).
// tests/test_policy.py reads the plan through gsrast_debug_backward_plan.
struct BackwardInputs { unsigned flags; int P, D, R, W, H; bool raw_family, sh, colors_precomp, cov3D_precomp, aux_grads /* dL_dacc_depth or dL_dalpha is given */;
                        unsigned known_flags = GSRAST_RENDER_AUX | GSRAST_RENDER_ANTIALIAS;      // backward_known_flags(the record's struct_size)
                        bool abs_sink = false, pose_out = false, pose_scratch = false; };        // dL_dmean2D_abs / dL_dcamera / pose_scratch is not NULL
// The flag bits a backward record of struct_size bytes knows: a bit whose fields lie beyond struct_size is an unknown bit (include/gsrast.h)
inline unsigned backward_known_flags(size_t struct_size)
{
    return GSRAST_RENDER_AUX | GSRAST_RENDER_ANTIALIAS | (struct_size >= GSRAST_BACKWARD_CALL_ABS ? GSRAST_RENDER_ABSGRAD : 0u) |
           (struct_size >= sizeof(gsrast_backward_call) ? GSRAST_RENDER_POSEGRAD : 0u);
}
// Which blend backward runs.  transposed: blend_bwd_cull_t_kernel<.., aux, abs>; ablate 1 / 2: blend_bwd_kernel<0, 4, ablate> (experiments), else 0
struct BlendBwdPick { int ppl = 1; bool cull = false, transposed = false, aux = false; int ablate = 0; bool abs = false; };
struct BackwardPlan {
    const char* refusal = nullptr;      // GSRAST_E_ARG with this text: unknown flags, a bad option value, aux without the culled kernels (in this order)
    bool aux = false, aa = false;                     // an aux gradient is given (both NULL is the plain backward); the state comes from an anti-aliased forward
    bool abs = false;                                 // GSRAST_RENDER_ABSGRAD: the blend backward sums |dL/dmean2D| per pixel, the per-Gaussian backward writes dL_dmean2D_abs
    bool pose = false;                                // GSRAST_RENDER_POSEGRAD: preprocess_bwd<.., POSE> sums the camera's gradient, pose_grad_reduce_kernel writes dL_dcamera (with do_geom)
    bool do_blend = false, do_geom = false;           // options.backward_phase: the blend backward / the per-Gaussian backward is part of this call
    bool use_sh = false, use_sr = false;              // colours from SH coefficients; covariances from scales + rotations
    bool zero_records = false;                        // the gradient records are zero-filled (the caller does not vouch for them, or the forward was told no backward would follow)
    bool derivs = false, derivs_side_wanted = false;  // sh_dir_derivs runs (a forward_only state); ... beside the blend backward
    bool late_fill_wanted = false;                    // the untouched Gaussians' zero rows beside the blend backward (phase 2 of two: beside preprocess_bwd): sparse call with the per-Gaussian backward, large scene (or list_cut_always)
    bool skip_zero_rows = false, join_in_front = false;   // experiments only (ablate 3: late fill without its kernel; 5: the join never moves behind preprocess_bwd)
    bool blend = false, from_buckets = false, tile_order = false;     // the blend backward runs (R > 0); its launch order from the forward's work buckets / from tile_order_kernel
    BlendBwdPick pick; uint32_t T = 0; int P = 0;
    bool sh_factor = false; int factors = 0;          // sh_factor_kernel runs (dL_dsh is the [P][3] factor); preprocess_bwd leaves dL_dsh to it
    bool sparse = false;                              // preprocess_bwd does not read Gaussians whose gradient record is all zero
    int mutate = 0;                                   // tests only: a backward that is wrong on purpose (bit 0: one tile's front batch dropped, bit 1: zero background)
    // second phase: what the side stream carries; preprocess_bwd<.., GROUPED, ..>; the join behind preprocess_bwd; the grids that follow
    bool derivs_on_side = false, late_fill = false, grouped = false, join_late = false; int derivs_grid = 0, per_gaussian_grid = 0;
    bool wants_side() const { return derivs_side_wanted || late_fill_wanted; }
    void side_answer(bool acquired)
    {
        derivs_on_side = derivs_side_wanted && acquired; late_fill = late_fill_wanted && acquired; grouped = late_fill;
        // The zero rows and the per-Gaussian backward write DISJOINT rows: when they are all the side stream carries, it is joined BEHIND preprocess_bwd
        join_late = late_fill && !derivs_on_side && !join_in_front;
        // two waves per compute unit, grid-stride: enough loads in flight for ~1.5 TB/s, few enough not to push the blend kernel's
        // workgroups off the chip (an unthrottled launch slowed the blend backward by 20 %, this one by 2 %)
        derivs_grid = !derivs ? 0 : derivs_on_side ? std::min((P + 63) / 64, 512) : (P + 63) / 64;
        // grouped: PB_GROUP Gaussians per workgroup, the ones late_rows_zero_kernel does not write compacted
        per_gaussian_grid = !do_geom ? 0 : grouped ? (P + PB_GROUP - 1) / PB_GROUP : (P + PP_THREADS - 1) / PP_THREADS;
    }
};
inline BackwardPlan plan_backward(const gsrast_options& o, const BackwardInputs& in, const PlanSwitches& g)
{
    BackwardPlan p;
    const bool aux_flag = (in.flags & GSRAST_RENDER_AUX) != 0;
    p.aux = aux_flag && in.aux_grads; p.aa = (in.flags & GSRAST_RENDER_ANTIALIAS) != 0;
    p.abs = (in.flags & GSRAST_RENDER_ABSGRAD) != 0;
    p.pose = (in.flags & GSRAST_RENDER_POSEGRAD) != 0;
    p.pick.cull = culled_blend(o, true);
    // (GSRAST_RENDER_ABSGRAD on a record without its sink is refused further down, where it always was, with a text of its own)
    if (in.flags & ~(in.known_flags | GSRAST_RENDER_ABSGRAD)) p.refusal = "flags: unknown bits";
    else if (!options_valid(o)) p.refusal = "backward: bad option value";
    else if (aux_flag && !p.pick.cull) p.refusal = "backward: acc_depth / alpha gradients need the culled blend kernels (options.cull != 0)";
    else if (p.abs && !(in.known_flags & GSRAST_RENDER_ABSGRAD)) p.refusal = "flags: unknown bits (GSRAST_RENDER_ABSGRAD is known only to a call record whose struct_size covers dL_dmean2D_abs)";
    else if (p.abs && !in.abs_sink) p.refusal = "backward: GSRAST_RENDER_ABSGRAD with a NULL dL_dmean2D_abs";
    else if (!p.abs && in.abs_sink) p.refusal = "backward: dL_dmean2D_abs without GSRAST_RENDER_ABSGRAD";
    else if (p.abs && (!p.pick.cull || g.ablate == 1 || g.ablate == 2))
        p.refusal = "backward: GSRAST_RENDER_ABSGRAD needs the transposed blend backward (options.cull != 0, no ablation kernel)";
    else if (p.pose && !in.pose_out) p.refusal = "backward: GSRAST_RENDER_POSEGRAD with a NULL dL_dcamera";
    else if (p.pose && !in.pose_scratch) p.refusal = "backward: GSRAST_RENDER_POSEGRAD with a NULL pose_scratch";
    else if (!p.pose && (in.pose_out || in.pose_scratch)) p.refusal = "backward: dL_dcamera / pose_scratch without GSRAST_RENDER_POSEGRAD";
    if (p.refusal || in.P <= 0 || in.R < 0 || in.W <= 0 || in.H <= 0) return p;      // (the shape is refused, or there is nothing to do)
    p.P = in.P; p.do_blend = o.backward_phase != 2; p.do_geom = o.backward_phase != 1;
    p.use_sh = in.sh && !in.colors_precomp; p.use_sr = !in.cov3D_precomp;
    p.zero_records = p.do_blend && (!o.grads_zeroed || o.forward_only);
    p.derivs = p.do_blend && p.use_sh && in.D > 0 && o.forward_only;
    p.derivs_side_wanted = p.derivs && o.side_stream && in.R > 0;
    // (with the per-Gaussian backward: a one-phase call, or phase 2 of two -- whose side stream then carries the zero rows beside preprocess_bwd alone)
    p.late_fill_wanted = p.do_geom && in.R > 0 && !o.dense_backward && o.side_stream && (in.P >= g.late_fill_min_p || g.list_cut_always);
    p.skip_zero_rows = g.ablate == 3; p.join_in_front = g.ablate == 5;
    p.T = (uint32_t)((in.W + TILE_X - 1) / TILE_X) * (uint32_t)((in.H + TILE_Y - 1) / TILE_Y);
    // Pixels per lane, measured on MI355X (profiles/): with per-wave accumulator slices the backward is within 2 % for 1, 2 and 4 at 1080p
    // and above; fewer win for small images (more waves) and small Gaussians (finer culling), more win at 4K.
    const int forced = o.bwd_pixels_per_lane;
    p.pick.ppl = forced ? forced : p.T >= 32768 ? 4 : (p.T >= 8192 ? 2 : 1);
    p.pick.aux = p.aux; p.pick.abs = p.abs;
    p.pick.ablate = (!p.aux && (g.ablate == 1 || g.ablate == 2)) ? g.ablate : 0;
    // aux, abs: always the transposed kernel, whatever the pixels per lane and the A/B switch say
    p.pick.transposed = p.aux || p.abs || (p.pick.cull && !p.pick.ablate && p.pick.ppl == 1 && g.bwd_transposed);
    p.blend = p.do_blend && in.R > 0;
    const bool ordered = p.blend && p.pick.cull && o.lpt != 0;
    p.from_buckets = ordered && p.T <= BUCKET_MAX_TILES;      // the forward blend appended every tile to the backward work buckets
    p.tile_order = ordered && !p.from_buckets;
    p.factors = (p.use_sh && o.sh_grad_factors) ? 1 : 0;
    p.sh_factor = p.do_blend && p.factors;      // the factor is final after the blend backward
    p.sparse = !o.dense_backward;
    p.mutate = p.blend ? g.mutate : 0;
    return p;
}

}  // namespace gsrast
