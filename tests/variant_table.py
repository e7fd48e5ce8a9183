"""The inventory of the run-time template dispatch of the renderer -- a helper of the tests, not a test.

saro-gs_amd/csrc/gsrast_capi.hip picks its hot kernels' instantiations at run time with pick_int<...> / pick_bool (gsrast_host.h).  ROWS holds
one row per instantiation of the dispatch sites below: the site, the template arguments, the switches (rast._C.set_option names: per-call
options and process-wide A/B switches alike) and the Python keywords that select it, and the -m gpu test that runs it against a reference.
tests/test_variants_host.py parses the two translation units and asserts that the value lists found there are exactly this table's, and
that the switches select what the row says (gsrast_debug_forward_plan / gsrast_debug_backward_plan); tests/test_gpu_variants.py runs the rows.

The forward's colour half dispatches with a plain if / else, which no pick shows: COLOR_LAUNCHES and COLOR_CALLS below list its seven launch
sites and the three calls of color_kernels, each with the case of tests/test_gpu_cut_colours.py that reaches it; test_variants_host.py
asserts that the source holds exactly these.

The two `ablate` instantiations of blend_bwd_kernel and the `mutate` kernel are experiments and have no row (OUT_OF_SCOPE names their
dispatch, and the standalone projection's, whose two instantiations tests/test_gpu_project.py runs)."""
import contextlib
import itertools
import re
from collections import namedtuple

Row = namedtuple("Row", "site args switches keywords test")
Site = namedtuple("Site", "name file anchor axes values")

CAPI, TRAIN = "saro-gs_amd/csrc/gsrast_capi.hip", "saro-gs_amd/csrc/gsrast_train.hip"
MODES, PPLS, BOOLS, CHUNKS = (0, 1, 2), (4, 2, 1), (False, True), (4, 8, 16, 32)
GPU = "tests/test_gpu_variants.py::"

# site: the text whose enclosing pick_int / pick_bool calls (outermost first) are the site's axes, and the values each may take
SITES = (
    Site("blend_fwd_cull", CAPI, "blend_fwd_cull_kernel<MODE, AUX><<<", ("MODE", "AUX"), (MODES, BOOLS)),
    Site("blend_fwd", CAPI, "blend_fwd_kernel<MODE, PPL><<<", ("MODE", "PPL"), (MODES, PPLS)),
    Site("blend_bwd_cull_t", CAPI, "blend_bwd_cull_t_kernel<MODE, AUX, ABS><<<", ("MODE", "AUX", "ABS"), (MODES, BOOLS, BOOLS)),
    Site("blend_bwd_cull", CAPI, "blend_bwd_cull_kernel<MODE, PPL><<<", ("MODE", "PPL"), (MODES, PPLS)),
    Site("blend_bwd", CAPI, "uncull(mode, lanes, int_c<0>{})", ("MODE", "PPL"), (MODES, PPLS)),
    Site("preprocess_fwd", CAPI, "preprocess_fwd_kernel<", ("RAW", "AA"), (BOOLS, BOOLS)),
    # (SPARSE, GROUPED) is no pick of its own: the launch lambda is called as (true, true) when grouped, else as (sparse, false)
    Site("preprocess_bwd", CAPI, "preprocess_bwd_kernel<", ("RAW", "AA", "POSE"), (BOOLS, BOOLS, BOOLS)),
    Site("features_fwd", CAPI, "features_fwd_kernel<", ("MODE", "CH"), (MODES, CHUNKS)),
    Site("features_bwd", CAPI, "features_bwd_kernel<", ("MODE", "CH"), (MODES, CHUNKS)),
    Site("contrib_blend", CAPI, "contrib_blend_kernel<", ("MODE",), (MODES,)),
    Site("distort_fwd", CAPI, "distort_fwd_kernel<", ("MODE",), (MODES,)),
    Site("distort_bwd", CAPI, "distort_bwd_kernel<", ("MODE",), (MODES,)),
    Site("bilagrid_bwd_grid", TRAIN, "bilagrid_bwd_grid_kernel<", ("L",), ((1, 2, 4, 8, 16),)),
    Site("hex_grad_tex_sorted", TRAIN, "hex_grad_tex_sorted_kernel<CH><<<", ("C",), ((4, 8, 16, 32, 64),)),
)
PREPROCESS_BWD_LAUNCHES = ("launch(std::true_type{}, std::true_type{})", "launch(sparse_c, std::false_type{})")      # grouped (=> sparse) | <sparse, not grouped>
PREPROCESS_BWD_SHAPES = dict(dense=(False, False), sparse=(True, False), grouped=(True, True))                      # name: (SPARSE, GROUPED)
# picks that are no row: (file, the text they enclose)
OUT_OF_SCOPE = ((CAPI, "uncull(int_c<0>{}, int_c<4>{}, abl)"), (CAPI, "project_fwd_kernel<"), (CAPI, "project_bwd_kernel<"))

# the switches' defaults (what `switched` restores): the per-call options of rast._C._OPTION_DEFAULTS and the library's process-wide words
DEFAULTS = dict(exp_mode=0, cull=1, fwd_pixels_per_lane=0, bwd_pixels_per_lane=0, dense_backward=0, bwd_transposed=1, late_fill_min_p=750000)

# feature widths of tests/test_gpu_variants.py: every chunk as a first pass, and every chunk as the last pass behind a full 32
FEATURE_WIDTHS = (4, 5, 8, 9, 16, 17, 32, 33, 36, 37, 40, 41, 48, 49, 63)
# (C, k) of its split test, run forward and backward in every exp_mode on F, F[:, :k] and F[:, k:]: passes [16] | [4] + [8], [16] | [8] + [8],
# [32, 8] | [8] + [32], [32, 16] | [16] + [32] -- every chunk, which is what holds the rows of modes 1 and 2
FEATURE_SPLITS = ((12, 4), (13, 5), (40, 8), (48, 16))


def features_chunk(C, c0):
    """gsrast_capi.hip: features_chunk -- the channels of the pass that starts at channel c0 of C."""
    rem = C - c0
    return 32 if rem > 16 else 16 if rem > 8 else 8 if rem > 4 else 4


def feature_passes(C):
    out, c0 = [], 0
    while c0 < C:
        out.append(features_chunk(C, c0))
        c0 += out[-1]
    return out


def fwd_switches(kind):
    """The forward's switches of tests/test_gpu_variants.py: "culled", or the un-culled template at 1 / 2 / 4 pixels per lane."""
    return dict(cull=1, fwd_pixels_per_lane=0) if kind == "culled" else dict(fwd_pixels_per_lane=int(kind))


BACKWARDS = ("transposed", "culled1", "culled2", "culled4", "unculled1", "unculled2", "unculled4")


def bwd_switches(kind):
    if kind == "transposed":
        return dict(cull=1, bwd_pixels_per_lane=0, bwd_transposed=1)
    ppl = int(kind[-1])
    if kind.startswith("culled"):
        return dict(cull=1, bwd_pixels_per_lane=ppl, **(dict(bwd_transposed=0) if ppl == 1 else {}))
    return dict(cull=0, bwd_pixels_per_lane=ppl)


def _rows():
    rows = []
    add = lambda *a: rows.append(Row(*a))      # noqa: E731
    for m in MODES:
        e = dict(exp_mode=m)
        for aux in BOOLS:
            add("blend_fwd_cull", (m, aux), dict(e, **fwd_switches("culled")), dict(return_aux=aux),
                GPU + ("test_transposed_backward_with_aux_and_absgrad" if aux else "test_blend_grid"))
        for ppl in PPLS:
            add("blend_fwd", (m, ppl), dict(e, cull=1, **fwd_switches(ppl)), {}, GPU + "test_blend_grid")
        for aux, ab in itertools.product(BOOLS, BOOLS):
            add("blend_bwd_cull_t", (m, aux, ab), dict(e, **bwd_switches("transposed")), dict(return_aux=aux, absgrad=ab),
                GPU + ("test_transposed_backward_with_aux_and_absgrad" if aux or ab else "test_blend_grid"))
        for ppl in PPLS:
            add("blend_bwd_cull", (m, ppl), dict(e, **bwd_switches(f"culled{ppl}")), {}, GPU + "test_blend_grid")
            add("blend_bwd", (m, ppl), dict(e, **bwd_switches(f"unculled{ppl}")), {}, GPU + "test_blend_grid")
        for ch in CHUNKS:
            for site in ("features_fwd", "features_bwd"):      # features: the smallest width whose first pass is this chunk
                add(site, (m, ch), e, dict(features=ch), GPU + ("test_feature_chunks_against_fp64" if m == 0 else "test_feature_columns_do_not_depend_on_their_chunk"))
        add("contrib_blend", (m,), e, dict(contrib=True), GPU + "test_replays_on_unculled_states")
        add("distort_fwd", (m,), e, dict(distortion=True), GPU + "test_replays_on_unculled_states")
        add("distort_bwd", (m,), e, dict(distortion=True), GPU + "test_replays_on_unculled_states")
    for raw, aa in itertools.product(BOOLS, BOOLS):
        add("preprocess_fwd", (raw, aa), {}, dict(raw=raw, antialiasing=aa), GPU + "test_preprocess_bwd_in_every_shape")
        for pose in BOOLS:
            for shape, (sparse, grouped) in PREPROCESS_BWD_SHAPES.items():
                sw = dict(dense=dict(dense_backward=1), sparse=dict(dense_backward=0), grouped=dict(dense_backward=0, late_fill_min_p=0))[shape]
                add("preprocess_bwd", (raw, sparse, grouped, aa, pose), sw, dict(raw=raw, antialiasing=aa, camera_grads=pose), GPU + "test_preprocess_bwd_in_every_shape")
    # the two dispatch sites of gsrast_train.hip: every value is reached by a test the suite already has
    for L in (1, 2, 4, 8, 16):      # bilagrid_math.GRIDS has L = 1, 2, 4, 8; test_gpu_bilagrid.GRIDS adds (64, 64, 16)
        add("bilagrid_bwd_grid", (L,), {}, dict(L=L), "tests/test_gpu_bilagrid.py::test_forward_and_backward_against_fp64")
    for C in (4, 8, 16, 32, 64):    # its parametrisation has C = 32, 16, 32, 4, 8, 64, each with scatter = 0 (the sorted-run kernel)
        add("hex_grad_tex_sorted", (C,), {}, dict(C=C), "tests/test_hexplane.py::test_single_plane_against_oracle")
    return tuple(rows)


ROWS = _rows()

# ---- the colour half of the forward: no pick, a seven-way if / else (gsrast_capi.hip: color_kernels) -------------------------------------------------
# One row per launch text inside color_kernels, in source order: the text, what selects it, and the -m gpu test id that runs it against the oracle.
# The two compacting launches run under the list cut only (plan.cut_colors: never under debug_state); the other five are what a forward
# without a cut takes -- visit 0 of every case of tests/test_gpu_cut_colours.py -- and what colours the whole set after a redo.
ColorLaunch = namedtuple("ColorLaunch", "launch when test")
ColorCall = namedtuple("ColorCall", "args what test")
CUT = "tests/test_gpu_cut_colours.py::"
COLOR_LAUNCHES = (
    ColorLaunch("preprocess_color_compact_kernel<true>", "list cut, raw leaves", CUT + "test_cut_colours_against_the_oracle[raw_M4_deg1_shs_res]"),
    ColorLaunch("preprocess_color_compact_kernel<false>", "list cut, shs or colors_precomp", CUT + "test_cut_colours_against_the_oracle[shs_M16_deg3]"),
    ColorLaunch("preprocess_color_kernel<PP_SH_MAX, true>", "raw leaves, M = 16", "tests/test_gpu_raw.py::test_raw_rasterizer_against_epilogue_then_rasterizer_and_the_oracles"),
    ColorLaunch("preprocess_color_kernel<0, true>", "raw leaves, M < 16", CUT + "test_cut_colours_against_the_oracle[raw_M4_deg1]"),
    ColorLaunch("preprocess_color_kernel<PP_SH_MAX, false>", "shs, M = 16, aligned", CUT + "test_cut_colours_against_the_oracle[shs_M16_deg0]"),
    ColorLaunch("preprocess_color_kernel<0, false>", "shs, M < 16, rows a multiple of four floats, aligned", CUT + "test_cut_colours_against_the_oracle[shs_M4_deg1]"),
    ColorLaunch("preprocess_color_direct_kernel", "colors_precomp, M > 16, rows no multiple of four floats, an unaligned base",
                CUT + "test_cut_colours_against_the_oracle[shs_M16_deg3_unaligned]"),
)
# the calls of color_kernels(stream, early_only, pred), in source order
COLOR_CALLS = (
    ColorCall("side ? side->stream : s, plan.cut_colors, nullptr", "the forward's colour launch: the early Gaussians only under a cut", CUT + "test_cut_colours_against_the_oracle[colors_precomp]"),
    ColorCall("s, true, pred", "the completion pass: the late candidates' colours, predicated, over skip2", CUT + "test_fallback_colours_the_late_gaussians[shs_M25_deg3]"),
    ColorCall("s, false, nullptr", "in front of a redo (exact_redo) under cut_colors: every Gaussian, the plain kernels", CUT + "test_redo_colours_every_gaussian[colors_precomp]"),
)
COLOR_KERNELS_SIGNATURE = "hipStream_t cs, bool early_only, const uint32_t* pred"


def rows_of(site):
    return [r for r in ROWS if r.site == site]


@contextlib.contextmanager
def switched(rast, switches):
    """Set `switches` (a row's, or any dict of DEFAULTS' names) through rast._C.set_option; the defaults are back on the way out."""
    assert set(switches) <= set(DEFAULTS), set(switches) - set(DEFAULTS)
    try:
        for k, v in switches.items():
            rast._C.set_option(k, v)
        yield
    finally:
        for k in switches:
            rast._C.set_option(k, DEFAULTS[k])


# ---- the parse of the translation units (tests/test_variants_host.py) ---------------------------------------------------------------------
_PICK = re.compile(r"\bpick_(int<([^>]*)>|bool)\s*\(")


def strip_comments(text):
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def picks_of(text):
    """[(start, end, values)] of every pick_int<...>(...) / pick_bool(...) call in `text` (comments stripped by the caller): the span of the
    whole call, and the values its lambda may receive."""
    out = []
    for m in _PICK.finditer(text):
        depth, k = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[k], 0)
            k += 1
        out.append((m.start(), k, BOOLS if m.group(1) == "bool" else tuple(int(v) for v in m.group(2).split(","))))
    return out


def enclosing(picks, pos):
    """The values of the picks whose call encloses position `pos`, outermost first."""
    return tuple(v for a, b, v in sorted(picks) if a < pos < b)
