"""CPU: the host-side decisions of a gsrast_context and of a render call (saro-gs_amd/csrc/gsrast_policy.h) driven through gsrast_policy_event,
gsrast_debug_forward_plan and gsrast_debug_backward_plan -- no device is touched: when the list cut is applied, paused and put on probation, how its margin and the predicted cut's requirement follow the
completion passes the device reports, how the speculative launch is sized."""
import pytest


@pytest.fixture()
def ctx(rast):
    c = rast._C.Context()
    yield c
    c.close()


P, Q = 3_000_000, 8_700_000
PAUSE, SCORE, MARGIN, TAU_REQ, TAU_FORCE, FB_PAUSE = range(6)


def test_cut_pays_only_in_large_scenes_and_outside_a_pause(ctx):
    ev = ctx.policy_event
    assert ev("begin", P, 1_499_999, 0) == 0            # the previous forward had too few column runs: the cut does not pay
    assert ev("begin", P, 1_500_000, 0) == 1
    assert ev("begin", 10_000, 0, 1) == 1               # option list_cut_always (tests)
    assert ev("begin", P, Q, 0) == 1
    # four cut forwards in a row that removed fewer than 1.5 M column runs: the context sits out 64 forwards -- not after one, two or three
    for k in range(3):
        assert ev("counts", Q, Q - 1_000_000, 2) == 0, k
    assert ev("counts", Q, Q - 2_000_000, 2) == 0       # (one that paid: the streak starts again)
    for k in range(3):
        assert ev("counts", Q, Q - 1_000_000, 2) == 0
    assert ev("counts", Q, Q - 1_000_000, 2) == 64
    served = 0
    while ev("begin", P, Q, 0) == 0:                    # every forward without the cut serves one forward of the pause
        served += 1
    assert served == 64 and ev("get", PAUSE) == 0


def test_a_pause_belongs_to_the_scene_that_earned_it(ctx):
    ev = ctx.policy_event
    ev("begin", 1_000_000, Q, 0)
    for _ in range(4):
        ev("counts", Q, Q - 100, 2)
    assert ev("get", PAUSE) == 64
    assert ev("begin", 1_050_000, Q, 0) == 0            # about the same scene: the pause holds
    assert ev("begin", 3_000_000, Q, 0) == 1            # another scene: void


def test_what_was_learned_on_one_scene_is_void_on_another(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    for _ in range(6):
        ev("pass", Q // 5, Q, 1)
    assert ev("get", MARGIN) == 16 and ev("get", TAU_REQ) > 40 and ev("get", TAU_FORCE) == 512
    ev("begin", P + P // 20, Q, 0)                      # the same scene after a densification step: kept
    assert ev("get", MARGIN) == 16
    ev("begin", 1_000_000, Q, 0)                        # another scene: a fresh policy
    assert ev("get", MARGIN) == 6 and ev("get", TAU_REQ) == 10 and ev("get", TAU_FORCE) == 0 and ev("get", SCORE) == 0


def test_completion_passes_are_scored_by_size(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    assert ev("pass", Q // 8, Q, 0) == 0                # up to an eighth of all column runs: what the speculation is expected to cost
    assert ev("pass", Q // 4, Q, 0) == 8                # a quarter and more: like a whole second forward
    assert 3 <= ev("pass", 3 * Q // 16, Q, 0) <= 5      # in between in proportion
    assert ev("pass", Q, Q, 0) == 8


def test_two_large_passes_pause_the_cut_then_probation_doubles(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    ev("pass", Q // 2, Q, 0)
    assert ev("get", PAUSE) == 0 and ev("get", SCORE) == 8
    ev("pass", Q // 2, Q, 0)
    assert ev("get", PAUSE) == 64 and ev("get", SCORE) == 8 and ev("get", FB_PAUSE) == 64      # on probation: the score restarts at half the bar
    while ev("begin", P, Q, 0) == 0:
        pass
    ev("pass", Q // 2, Q, 0)                            # ONE more large pass: paused again, twice as long
    assert ev("get", PAUSE) == 128
    for want in (256, 512, 1024, 1024):
        while ev("begin", P, Q, 0) == 0:
            pass
        ev("pass", Q // 2, Q, 0)
        assert ev("get", PAUSE) == want
    while ev("begin", P, Q, 0) == 0:
        pass
    for _ in range(64):                                 # 64 cut forwards without a pass: forgotten
        ev("clean")
    assert ev("get", FB_PAUSE) == 0 and ev("get", SCORE) == 0
    ev("pass", Q // 2, Q, 0)
    assert ev("get", PAUSE) == 0


def test_small_passes_do_not_pause(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    for _ in range(200):
        assert ev("pass", Q // 50, Q, 0) == 0
    assert ev("get", PAUSE) == 0 and ev("get", SCORE) == 0


def test_margin_and_requirement_widen_with_passes_and_narrow_slowly(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    assert ev("get", MARGIN) == 6 and ev("get", TAU_REQ) == 10
    ev("pass", Q // 50, Q, 1)
    assert ev("get", MARGIN) == 8 and ev("get", TAU_REQ) == 18
    for _ in range(20):
        ev("pass", Q // 50, Q, 1)
    assert ev("get", MARGIN) == 16 and ev("get", TAU_REQ) == 96          # 4 x the deepest consumed entry / 96 of mean alpha mass: the ends
    for _ in range(127):
        ev("clean")
    assert ev("get", MARGIN) == 16
    ev("clean")
    assert ev("get", MARGIN) == 15 and ev("get", TAU_REQ) == 92           # a quarter step per 128, 2 per 64 clean cut forwards
    for _ in range(128 * 12):
        ev("clean")
    assert ev("get", MARGIN) == 6 and ev("get", TAU_REQ) == 44


def test_a_wide_failure_switches_to_predicted_cut_depths(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    ev("pass", Q // 2, Q, 0)                            # no predicted cut available (option tau_cut 0): nothing to switch to
    assert ev("get", TAU_FORCE) == 0
    ev("pass", Q // 50, Q, 1)                           # a small pass: the remembered cuts are fine
    assert ev("get", TAU_FORCE) == 0
    ev("pass", Q // 5, Q, 1)
    assert ev("get", TAU_FORCE) == 512


def test_frequent_small_passes_switch_to_predicted_cut_depths_too(ctx):
    ev = ctx.policy_event
    ev("begin", P, Q, 0)
    for _ in range(40):                                 # one small pass in twenty forwards: the price of the speculation
        ev("pass", Q // 50, Q, 1)
        for _ in range(19):
            ev("clean")
    assert ev("get", TAU_FORCE) == 0
    for k in range(12):                                 # one in five: every pass is a chain of launches the caller waits for
        ev("pass", Q // 50, Q, 1)
        for _ in range(4):
            ev("clean")
    assert ev("get", TAU_FORCE) == 512


def test_speculative_launch_sizes(ctx):
    ev = ctx.policy_event
    assert ev("grow", 1_000_000) == 1_254_096           # 1.25 x + 4096
    assert ev("grow", 2_000_000_000) == 0x7FFFFFFF
    assert ev("follow", 1600, 2000, 4) == 2000          # a hint follows a larger count at once ...
    assert ev("follow", 1600, 100, 4) == 1500           # ... and decays by a sixteenth per forward otherwise
    assert ev("size", 0, 5_000_000, 1) == 5_000_000     # nothing known about the early set: all column runs
    assert ev("size", 1_000_000, 5_000_000, 0) == 5_000_000
    assert ev("size", 1_000_000, 5_000_000, 1) == 1_504_096
    assert ev("size", 4_000_000, 5_000_000, 1) == 5_000_000
    with pytest.raises(ValueError):
        ev("no_such_event")


def test_depth_range_widens_at_once_and_narrows_slowly(ctx):
    """gsrast_policy.h: DepthRange -- the key range the depth histogram's middle bins (and the predicted cut's 32 bins) cover."""
    ev = ctx.policy_event
    ZH_TAIL, ZH_MID, ZH_BINS = 64, 896, 1024
    klo0, sh0 = ev("zget", 0), ev("zget", 1)
    assert sh0 == 21 and ev("zget", 2) == 0              # nothing learned: 4 bins per octave over every finite float, no upper end
    # a context's first forward (coarse table): the scene occupies bins 78-83 = depths 2.4 ... 6.7 -- not "held" (the table was not a learned one)
    r = ev("zrange", 78 | (83 << 16))
    assert not (r & 256)
    sh1, klo1, khi1 = ev("zget", 1), ev("zget", 0), ev("zget", 2)
    assert sh1 < sh0 and klo1 > klo0 and khi1 > klo1     # the table now resolves the scene: finer bins, a range around it
    span1 = khi1 - klo1
    # the same scene seen through the learned table occupies the middle (an eighth of padding on either side): held, and the range stays put
    first = ZH_TAIL + ZH_MID // 10
    last = ZH_TAIL + int(0.9 * ((span1 * 256) >> sh1))       # (zget returns keys / 256)
    r = ev("zrange", first | (last << 16))
    assert r & 256
    # a view whose keys reach the table's last bin: clipped (not held), the range widens AT ONCE, far beyond the old end
    r = ev("zrange", first | ((ZH_BINS - 1) << 16))
    assert not (r & 256) and ev("zget", 2) > khi1
    wide = ev("zget", 2) - ev("zget", 0)
    # ... and narrows by an eighth of the gap per forward once the views are narrow again
    prev = wide
    for _ in range(40):
        sh = ev("zget", 1)
        ev("zrange", (ZH_TAIL + 100) | ((ZH_TAIL + 200) << 16))
        now = ev("zget", 2) - ev("zget", 0)
        assert now <= prev
        prev = now
    assert prev < wide // 4


# ---- the bucket depth sort's back-off (gsrast_policy.h: DepthSortPolicy): "depth_sort" a = RADIX / CLEAN / OVERFLOW, b = 1: the table held every key ----
RADIX, CLEAN, OVERFLOW = range(3)
BUCKET_SKIP, BUCKET_BACKOFF, BUCKET_CLEAN = 6, 7, 8


def test_an_isolated_bucket_overflow_is_free(ctx):
    ev = ctx.policy_event
    for n in (32, 33, 63):          # 32 or more clean forwards before it, no length remembered: this forward's repeat and nothing else
        for _ in range(n):
            assert ev("depth_sort", CLEAN) == 0
        assert ev("depth_sort", OVERFLOW, 1) == 0, n
        assert ev("get", BUCKET_SKIP) == 0 and ev("get", BUCKET_BACKOFF) == 0 and ev("get", BUCKET_CLEAN) == 0


def test_bucket_overflows_in_quick_succession_back_off_and_double(ctx):
    ev = ctx.policy_event
    for _ in range(31):
        ev("depth_sort", CLEAN)
    assert ev("depth_sort", OVERFLOW, 1) == 16          # fewer than 32 clean forwards before it: 16 radix forwards
    assert ev("get", BUCKET_SKIP) == 16 and ev("get", BUCKET_BACKOFF) == 16
    for left in range(15, -1, -1):                      # every radix forward serves one forward of the pause
        assert ev("depth_sort", RADIX) == left
    assert ev("depth_sort", RADIX) == 0                 # (never below zero)
    want = 32
    for _ in range(12):                                 # every further overflow: twice the remembered length, 4096 at most -- however many clean forwards (< 64) lie between
        for _ in range(40):
            ev("depth_sort", CLEAN)
        assert ev("depth_sort", OVERFLOW, 1) == want
        assert ev("get", BUCKET_BACKOFF) == want
        want = min(want * 2, 4096)
    assert want == 4096 and ev("get", BUCKET_SKIP) == 4096


def test_64_clean_forwards_forget_the_back_off_length(ctx):
    ev = ctx.policy_event
    assert ev("depth_sort", OVERFLOW, 1) == 16 and ev("depth_sort", OVERFLOW, 1) == 32
    for _ in range(32):
        ev("depth_sort", RADIX)
    assert ev("get", BUCKET_SKIP) == 0 and ev("get", BUCKET_BACKOFF) == 32
    for k in range(63):
        ev("depth_sort", CLEAN)
        assert ev("get", BUCKET_BACKOFF) == 32, k
    ev("depth_sort", CLEAN)
    assert ev("get", BUCKET_BACKOFF) == 0 and ev("get", BUCKET_CLEAN) == 64
    assert ev("depth_sort", OVERFLOW, 1) == 0           # the next isolated overflow is free again
    assert ev("get", BUCKET_BACKOFF) == 0


def test_an_overflow_under_a_table_that_did_not_hold_every_key_never_pauses(ctx):
    ev = ctx.policy_event
    for _ in range(5):                                  # b = 0: the histogram was not up to the view; its range is learned, the next forward tries again
        assert ev("depth_sort", OVERFLOW, 0) == 0
    assert ev("get", BUCKET_BACKOFF) == 0
    assert ev("depth_sort", OVERFLOW, 1) == 16          # ... also while a length is remembered and a pause is being served: neither grows
    assert ev("depth_sort", OVERFLOW, 0) == 16
    assert ev("get", BUCKET_SKIP) == 16 and ev("get", BUCKET_BACKOFF) == 16 and ev("get", BUCKET_CLEAN) == 0


def test_the_clean_count_saturates_and_reset_clears_the_back_off(ctx):
    ev = ctx.policy_event
    for _ in range(1100):
        ev("depth_sort", CLEAN)
    assert ev("get", BUCKET_CLEAN) == 1024
    assert ev("depth_sort", OVERFLOW, 1) == 0 and ev("get", BUCKET_CLEAN) == 0
    assert ev("depth_sort", OVERFLOW, 1) == 16 and ev("depth_sort", CLEAN) == 16
    assert (ev("get", BUCKET_SKIP), ev("get", BUCKET_BACKOFF), ev("get", BUCKET_CLEAN)) == (16, 16, 1)
    assert ev("reset") == 0
    assert (ev("get", BUCKET_SKIP), ev("get", BUCKET_BACKOFF), ev("get", BUCKET_CLEAN)) == (0, 0, 0)
    with pytest.raises(ValueError):                     # (an unknown outcome is refused)
        ev("depth_sort", 3)


# ---- the forward's plan (gsrast_policy.h: ForwardPlan) through gsrast_debug_forward_plan: what a forward WOULD decide, no device involved ----
(RUNBIN, BUCKETS, BUCKET_SORT, TWO_LEVEL, CULLED, ORDERED, HINTS, CUT_BASE, TAU_MODE, ZERO_IN_BLEND, ZERO_TOUCHED, UNTOUCHED, CLIP, SH_DERIVS,
 SPECULATIVE, ADAPTIVE, ASSUME_SHORT, PAYS, CUT) = (1 << k for k in range(19))
AUX = 1


@pytest.fixture()
def plan(rast, ctx):
    import ctypes as C
    L = rast._C.lib()
    fn = C.CDLL(rast._C.LIB_PATH).gsrast_debug_forward_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    switched = {}

    def run(P=3_000_000, W=1920, H=1080, flags=0, bucket_skip=0, R_hint=9_000_000, last_Q=Q, depth_short=0, sh=1, precomp=0, D=3, table=1, switches=None, **opts):
        for name, v in (switches or {}).items():
            switched.setdefault(name, L.gsrast_get_option(name.encode()))
            assert L.gsrast_set_option(name.encode(), v) == 0
        o = rast._C.OptionsStruct()
        L.gsrast_options_init(C.byref(o))
        for k, v in opts.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        words = (C.c_int * 6)(bucket_skip, R_hint, last_Q, depth_short, sh | precomp << 1 | D << 4, table)
        try:
            return fn(ctx.handle, C.byref(o), flags, P, W, H, words)
        finally:
            for name, v in switched.items():
                assert L.gsrast_set_option(name.encode(), v) == 0 and L.gsrast_get_option(name.encode()) == v
    run.error = lambda: L.gsrast_last_error().decode()
    return run


def test_plan_of_the_default_path(plan):
    v = plan()
    want = (RUNBIN | BUCKETS | BUCKET_SORT | TWO_LEVEL | CULLED | ORDERED | HINTS | CUT_BASE | TAU_MODE | ZERO_IN_BLEND | ZERO_TOUCHED | UNTOUCHED | CLIP
            | SH_DERIVS | SPECULATIVE | ADAPTIVE | PAYS | CUT)
    assert v == want, bin(v ^ want)


@pytest.mark.parametrize("opt", [dict(fwd_pixels_per_lane=2), dict(cull=0), dict(lpt=0)])
def test_plan_without_the_ordered_culled_kernel_has_no_hints_and_no_cut(plan, opt):
    v = plan(**opt)
    assert not v & (HINTS | CUT_BASE | CUT | ORDERED)
    if "lpt" in opt:      # the culled kernel still runs, in tile order: it zeroes the records and keeps the bits
        assert v & CULLED and v & ZERO_IN_BLEND and v & UNTOUCHED
    else:
        assert not v & (CULLED | ZERO_IN_BLEND | ZERO_TOUCHED | UNTOUCHED)
    assert v & RUNBIN and v & BUCKET_SORT and v & SPECULATIVE


@pytest.mark.parametrize("kw", [dict(binning=1), dict(W=1920, H=16 * 257), dict(W=16 * 300, H=16 * 256)])
def test_plan_without_run_compressed_binning(plan, kw):
    v = plan(**kw)      # binning = 1; more than 256 tile rows; more than 65536 tiles
    assert not v & (RUNBIN | BUCKET_SORT | TWO_LEVEL | HINTS | CUT_BASE | CUT | CLIP | SPECULATIVE)
    assert v & CULLED and v & ZERO_IN_BLEND
    assert bool(v & BUCKETS) == (kw.get("W", 1920) // 16 * (kw.get("H", 1080) // 16) <= 65535)


def test_plan_depth_sort_selection(plan):
    assert plan() & BUCKET_SORT
    for kw in (dict(depth_sort=1), dict(bucket_skip=3), dict(P=32767)):      # the caller, a recent overflow, a small scene: radix
        v = plan(**kw)
        assert not v & (BUCKET_SORT | TWO_LEVEL | CUT_BASE | CUT) and v & RUNBIN and v & HINTS, kw
    assert plan(P=32768) & BUCKET_SORT
    # the scatter as two launches from two_level_min_p Gaussians on, unless switched off
    assert not plan(P=2_499_999) & TWO_LEVEL and plan(P=2_500_000) & TWO_LEVEL
    assert not plan(switches=dict(two_level=0)) & TWO_LEVEL
    assert plan(P=100_000, switches=dict(two_level_min_p=100_000)) & TWO_LEVEL
    # the radix sort adapts its pass count above 64 blocks of 2048; three passes are assumed after a forward with short keys
    assert not plan(P=64 * 2048) & ADAPTIVE and plan(P=64 * 2048 + 1) & ADAPTIVE
    assert plan(depth_short=1) & ASSUME_SHORT and not plan(depth_short=1, P=100_000) & ASSUME_SHORT
    assert not plan(depth_short=1, switches=dict(sort_hint=0)) & ASSUME_SHORT


def test_plan_list_cut_conditions(plan, ctx):
    assert plan() & CUT
    for kw in (dict(tile_clip=0), dict(speculative=0), dict(R_hint=0), dict(no_list_cut=1)):
        v = plan(**kw)
        assert not v & (CUT_BASE | CUT) and v & PAYS, kw
    v = plan(last_Q=1_499_999)      # pays(): too few column runs in the last forward ...
    assert v & CUT_BASE and not v & (PAYS | CUT)
    assert plan(last_Q=1_499_999, switches=dict(list_cut_always=1)) & CUT
    ctx.policy_event("begin", 3_000_000, Q, 0)
    for _ in range(4):
        ctx.policy_event("counts", Q, Q - 100, 2)
    assert not plan() & (PAYS | CUT)      # ... or a pause
    ctx.policy_event("reset")
    # without the pose table the cut needs predicted depths
    assert plan(table=0) & CUT and plan(no_order_hint=1, table=0) & CUT and not plan(no_order_hint=1) & HINTS
    v = plan(table=0, switches=dict(tau_cut=0))
    assert v & CUT_BASE and not v & (CUT | TAU_MODE)
    assert plan(table=1, switches=dict(tau_cut=0)) & CUT


def test_plan_gradient_records_and_derivatives(plan):
    v = plan(forward_only=1)
    assert not v & (UNTOUCHED | ZERO_TOUCHED | SH_DERIVS) and v & ZERO_IN_BLEND
    v = plan(switches=dict(touch_bits=0))
    assert not v & (UNTOUCHED | ZERO_TOUCHED) and v & ZERO_IN_BLEND
    v = plan(switches=dict(sparse_grec=0))
    assert v & UNTOUCHED and not v & ZERO_TOUCHED
    assert not plan(D=0) & SH_DERIVS and not plan(precomp=1) & SH_DERIVS and not plan(sh=0, precomp=1) & SH_DERIVS
    assert not plan(tile_clip=0) & CLIP


def test_plan_refusals_keep_their_texts(plan):
    assert plan(flags=AUX) & CULLED
    for kw in (dict(cull=0), dict(fwd_pixels_per_lane=1)):
        assert plan(flags=AUX, **kw) == -1
        assert plan.error() == "forward: acc_depth / alpha need the culled blend kernel (options.cull != 0, fwd_pixels_per_lane == 0)"
    assert plan(flags=8) == -1 and plan.error() == "flags: unknown bits"
    assert plan(fwd_pixels_per_lane=3) == -1 and plan.error() == "forward: bad option value"
    assert plan(flags=8, fwd_pixels_per_lane=3) == -1 and plan.error() == "flags: unknown bits"      # (the order of the checks)


# ---- the backward's plan (gsrast_policy.h: BackwardPlan) through gsrast_debug_backward_plan: what a backward WOULD decide, no device involved ----
(B_AUX, B_AA, B_DO_BLEND, B_DO_GEOM, B_ZERO_RECORDS, B_DERIVS, B_DERIVS_ON_SIDE, B_LATE_FILL_WANTED, B_LATE_FILL, B_SKIP_ZERO_ROWS, B_JOIN_LATE, B_BLEND, B_CULL,
 B_TRANSPOSED, B_PICK_AUX, B_BUCKETS, B_TILE_ORDER, B_SH_FACTOR, B_FACTORS, B_SPARSE, B_GROUPED) = (1 << k for k in range(21))
ANTIALIAS = 2


class BwdPlan(int):
    ppl = property(lambda v: v >> 21 & 7)
    ablate = property(lambda v: v >> 24 & 3)
    mutate = property(lambda v: v >> 26 & 3)


@pytest.fixture()
def bplan(rast):
    import ctypes as C
    L = rast._C.lib()
    fn = C.CDLL(rast._C.LIB_PATH).gsrast_debug_backward_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    switched = {}

    def run(P=3_000_000, D=3, R=40_000_000, W=1920, H=1080, flags=0, raw=0, sh=1, precomp=0, cov3D=0, aux_grads=0, side=1, switches=None, **opts):
        for name, v in (switches or {}).items():
            switched.setdefault(name, L.gsrast_get_option(name.encode()))
            assert L.gsrast_set_option(name.encode(), v) == 0
        o = rast._C.OptionsStruct()
        L.gsrast_options_init(C.byref(o))
        for k, v in opts.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        words = (C.c_int * 7)(P, D, R, W, H, raw | sh << 1 | precomp << 2 | cov3D << 3 | aux_grads << 4, side)
        grids = (C.c_int * 2)(-1, -1)
        try:
            v = fn(C.byref(o), flags, words, grids)
            run.grids = tuple(grids)
            return BwdPlan(v) if v >= 0 else v
        finally:
            for name, v in switched.items():
                assert L.gsrast_set_option(name.encode(), v) == 0 and L.gsrast_get_option(name.encode()) == v
    run.error = lambda: L.gsrast_last_error().decode()
    return run


B_DEFAULT = (B_DO_BLEND | B_DO_GEOM | B_ZERO_RECORDS | B_LATE_FILL_WANTED | B_LATE_FILL | B_JOIN_LATE | B_BLEND | B_CULL | B_TRANSPOSED | B_BUCKETS
             | B_SPARSE | B_GROUPED)


def test_backward_plan_of_the_default_path(bplan):
    """3 M Gaussians at 1080p: transposed blend from the work buckets, zero rows beside it, grouped sparse preprocess_bwd, join behind it."""
    v = bplan()
    assert v & (1 << 21) - 1 == B_DEFAULT, bin(v ^ B_DEFAULT)
    assert (v.ppl, v.ablate, v.mutate) == (1, 0, 0)
    assert bplan.grids == (0, (3_000_000 + 1023) // 1024)      # no sh_dir_derivs; PB_GROUP = 1024 Gaussians per workgroup
    assert bplan(flags=ANTIALIAS) == v | B_AA


def test_backward_plan_late_fill_conditions(bplan):
    lost = B_LATE_FILL_WANTED | B_LATE_FILL | B_JOIN_LATE | B_GROUPED
    for kw in (dict(dense_backward=1), dict(side_stream=0), dict(backward_phase=1), dict(R=0), dict(P=749_999)):
        v = bplan(**kw)
        assert not v & lost, kw
        assert bool(v & B_SPARSE) == ("dense_backward" not in kw)
        if v & B_DO_GEOM:
            assert bplan.grids[1] == (kw.get("P", 3_000_000) + 127) // 128, kw      # ungrouped: PP_THREADS = 128 Gaussians per workgroup
    assert bplan(P=750_000) & lost == lost
    assert bplan(P=749_999, switches=dict(late_fill_min_p=0)) & lost == lost
    assert bplan(P=1000, switches=dict(list_cut_always=1)) & lost == lost      # regained
    for kw in (dict(dense_backward=1), dict(side_stream=0), dict(backward_phase=1), dict(R=0)):
        assert not bplan(P=1000, switches=dict(list_cut_always=1), **kw) & lost, kw
    # the phases: the zero rows and the grouped form belong to the call that runs the per-Gaussian backward -- phase 2 of two (a backward with a
    # feature or distortion gradient) as well as the one-phase call, under the same conditions
    v = bplan(backward_phase=1)
    assert v & B_DO_BLEND and v & B_BLEND and v & B_ZERO_RECORDS and not v & B_DO_GEOM and bplan.grids == (0, 0)
    v = bplan(backward_phase=2)
    assert v & B_DO_GEOM and not v & (B_DO_BLEND | B_BLEND | B_ZERO_RECORDS | B_BUCKETS | B_SH_FACTOR)
    assert v & lost == lost and v & B_SPARSE and bplan.grids == (0, (3_000_000 + 1023) // 1024)
    assert bplan(P=749_999, backward_phase=2, switches=dict(late_fill_min_p=0)) & lost == lost
    assert bplan(P=1000, backward_phase=2, switches=dict(list_cut_always=1)) & lost == lost
    for kw in (dict(dense_backward=1), dict(side_stream=0), dict(R=0), dict(P=749_999)):
        v = bplan(backward_phase=2, **kw)
        assert not v & lost and bplan.grids[1] == (kw.get("P", 3_000_000) + 127) // 128, kw
    v = bplan(backward_phase=2, side=0)      # no side stream to be had: wanted, not had, the ungrouped sparse kernel
    assert v & B_LATE_FILL_WANTED and v & B_SPARSE and not v & (B_LATE_FILL | B_GROUPED | B_JOIN_LATE)
    v = bplan(R=0)
    assert v & B_DO_BLEND and v & B_ZERO_RECORDS and not v & (B_BLEND | B_BUCKETS | B_TILE_ORDER)


def test_backward_plan_without_a_side_stream(bplan):
    v = bplan(side=0)      # side_stream_of returned null: late fill wanted and not had, the ungrouped sparse kernel
    assert v & B_LATE_FILL_WANTED and v & B_SPARSE and not v & (B_LATE_FILL | B_GROUPED | B_JOIN_LATE)
    assert bplan.grids == (0, (3_000_000 + 127) // 128)
    v = bplan(side=0, forward_only=1)      # ... and sh_dir_derivs inline with the full grid
    assert v & B_DERIVS and not v & (B_DERIVS_ON_SIDE | B_LATE_FILL | B_GROUPED | B_JOIN_LATE)
    assert bplan.grids == ((3_000_000 + 63) // 64, (3_000_000 + 127) // 128)


def test_backward_plan_of_a_forward_only_state(bplan):
    v = bplan(forward_only=1, grads_zeroed=1)      # the forward has not zeroed the records, whatever the caller says
    assert v & B_ZERO_RECORDS and v & B_DERIVS and v & B_DERIVS_ON_SIDE and v & B_LATE_FILL and v & B_GROUPED
    assert not v & B_JOIN_LATE      # the side stream carries derivatives preprocess_bwd reads: joined in front
    assert bplan.grids[0] == 512
    assert bplan(P=10_000, forward_only=1) & B_DERIVS_ON_SIDE and bplan.grids[0] == (10_000 + 63) // 64
    for kw in (dict(side_stream=0), dict(R=0)):      # inline
        v = bplan(forward_only=1, **kw)
        assert v & B_DERIVS and not v & B_DERIVS_ON_SIDE and bplan.grids[0] == (3_000_000 + 63) // 64, kw
    for kw in (dict(D=0), dict(precomp=1), dict(sh=0, precomp=1), dict(backward_phase=2)):      # nothing to differentiate / not this phase
        assert not bplan(forward_only=1, **kw) & (B_DERIVS | B_DERIVS_ON_SIDE), kw
    v = bplan(forward_only=1, backward_phase=1)      # phase 1 of two: derivatives beside the blend, no zero rows
    assert v & B_DERIVS_ON_SIDE and not v & (B_LATE_FILL | B_JOIN_LATE)
    assert not bplan() & B_DERIVS


def test_backward_plan_grads_zeroed(bplan):
    assert bplan() & B_ZERO_RECORDS and not bplan(grads_zeroed=1) & B_ZERO_RECORDS
    assert not bplan(backward_phase=2) & B_ZERO_RECORDS and not bplan(grads_zeroed=1, backward_phase=1) & B_ZERO_RECORDS


def test_backward_plan_launch_order(bplan):
    assert bplan(W=16 * 255, H=16 * 257) & B_BUCKETS and not bplan(W=16 * 255, H=16 * 257) & B_TILE_ORDER      # 65535 tiles: BUCKET_MAX_TILES
    v = bplan(W=16 * 256, H=16 * 256)                                                                         # 65536
    assert v & B_TILE_ORDER and not v & B_BUCKETS
    for kw in (dict(lpt=0), dict(cull=0)):
        assert not bplan(**kw) & (B_BUCKETS | B_TILE_ORDER), kw
        assert not bplan(W=16 * 256, H=16 * 256, **kw) & (B_BUCKETS | B_TILE_ORDER), kw


def test_backward_plan_blend_kernel(bplan):
    # pixels per lane by tile count: 1 below 8192 tiles, 2 from there, 4 from 32768; forced
    for W, H, ppl in ((1920, 1080, 1), (16 * 128, 16 * 64 - 1, 2), (16 * 128 - 1, 16 * 64, 2), (16 * 127, 16 * 64, 1), (16 * 256, 16 * 128, 4), (16 * 256, 16 * 127, 2)):
        v = bplan(W=W, H=H)
        assert v.ppl == ppl and v & B_CULL and bool(v & B_TRANSPOSED) == (ppl == 1), (W, H)
    for forced in (1, 2, 4):
        for W, H in ((1920, 1080), (3840, 2160), (16 * 256, 16 * 128)):
            v = bplan(W=W, H=H, bwd_pixels_per_lane=forced)
            assert v.ppl == forced and v & B_CULL and bool(v & B_TRANSPOSED) == (forced == 1), (forced, W)
    assert bplan(fwd_pixels_per_lane=2).ppl == 1      # the forward's is not the backward's
    v = bplan(switches=dict(bwd_transposed=0))
    assert v & B_CULL and not v & B_TRANSPOSED and v.ppl == 1
    v = bplan(cull=0)
    assert not v & (B_CULL | B_TRANSPOSED | B_BUCKETS) and v.ppl == 1
    # aux forces the transposed kernel, whatever the pixels per lane and the A/B switch say
    for kw in (dict(), dict(bwd_pixels_per_lane=4), dict(W=3840, H=2160), dict(switches=dict(bwd_transposed=0))):
        v = bplan(flags=AUX, aux_grads=1, **kw)
        assert v & B_AUX and v & B_PICK_AUX and v & B_TRANSPOSED, kw
    v = bplan(flags=AUX, aux_grads=0)      # both aux gradients NULL: the plain backward
    assert v == bplan() and not v & (B_AUX | B_PICK_AUX)
    assert not bplan(flags=0, aux_grads=1) & (B_AUX | B_PICK_AUX)      # without the flag the pointers are not looked at


def test_backward_plan_ablate_and_mutate(bplan):
    for a in (1, 2):
        v = bplan(switches=dict(ablate=a))
        assert v.ablate == a and not v & B_TRANSPOSED and v & B_LATE_FILL and v & B_JOIN_LATE
        v = bplan(flags=AUX, aux_grads=1, switches=dict(ablate=a))      # ignored under aux
        assert v.ablate == 0 and v & B_TRANSPOSED and v & B_PICK_AUX
    v = bplan(switches=dict(ablate=3))      # late fill without its kernel: everything else as if the rows had been written
    assert v & B_SKIP_ZERO_ROWS and v & B_LATE_FILL and v & B_GROUPED and v & B_JOIN_LATE and v.ablate == 0 and v & B_TRANSPOSED
    v = bplan(switches=dict(ablate=5))      # the join in front
    assert v & B_LATE_FILL and v & B_GROUPED and not v & (B_JOIN_LATE | B_SKIP_ZERO_ROWS) and v.ablate == 0
    assert bplan(switches=dict(ablate=4)) == bplan() and bplan(switches=dict(ablate=-1)) == bplan()
    for m in (1, 2, 3):
        assert bplan(switches=dict(mutate=m)).mutate == m
    assert bplan(switches=dict(mutate=3), backward_phase=2).mutate == 0 and bplan(switches=dict(mutate=3), R=0).mutate == 0      # no blend backward to mutate
    assert bplan().mutate == 0      # (the fixture restored the switch)


def test_backward_plan_sh_grad_factors(bplan):
    v = bplan(sh_grad_factors=1)
    assert v & B_SH_FACTOR and v & B_FACTORS and v & B_LATE_FILL
    assert not bplan() & (B_SH_FACTOR | B_FACTORS)
    v = bplan(sh_grad_factors=1, backward_phase=1)      # the factor is final after the blend backward: all a multi-GPU caller needs to start its exchange
    assert v & B_SH_FACTOR and v & B_FACTORS
    v = bplan(sh_grad_factors=1, backward_phase=2)
    assert v & B_FACTORS and not v & B_SH_FACTOR
    for kw in (dict(precomp=1), dict(sh=0, precomp=1)):
        assert not bplan(sh_grad_factors=1, **kw) & (B_SH_FACTOR | B_FACTORS), kw
    assert bplan(sh_grad_factors=1, raw=1) & B_SH_FACTOR


def test_backward_plan_refusals_keep_their_texts(bplan):
    assert bplan(flags=AUX, aux_grads=1) & B_AUX and bplan(flags=AUX, aux_grads=1, bwd_pixels_per_lane=2) & B_AUX
    for aux_grads in (0, 1):      # the rule is checked first: also with both gradients NULL
        assert bplan(flags=AUX, aux_grads=aux_grads, cull=0) == -1
        assert bplan.error() == "backward: acc_depth / alpha gradients need the culled blend kernels (options.cull != 0)"
    assert bplan(flags=8) == -1 and bplan.error() == "flags: unknown bits"
    for kw in (dict(bwd_pixels_per_lane=3), dict(backward_phase=3), dict(dense_backward=2), dict(exp_mode=3)):
        assert bplan(**kw) == -1 and bplan.error() == "backward: bad option value", kw
    assert bplan(flags=8, bwd_pixels_per_lane=3) == -1 and bplan.error() == "flags: unknown bits"      # (the order of the checks)
    assert bplan(flags=AUX, cull=0, bwd_pixels_per_lane=3) == -1 and bplan.error() == "backward: bad option value"
