"""CPU: tests/variant_table.py against the sources and against the host-side plans -- no device is touched.

* The table is complete: every pick_int<...> / pick_bool( of saro-gs_amd/csrc/gsrast_capi.hip and gsrast_train.hip is found, the values of
  the picks around each dispatch site are the table's, every product of values is a row and every row is such a product.  A new
  instantiation without a row, and a row without an instantiation, turn this red (as tests/test_capi_abi.py pins the signature table).
* The colour half's if / else dispatch (color_kernels) holds exactly the launch sites and calls of the table's COLOR_LAUNCHES / COLOR_CALLS.
* The switches select what the row says: gsrast_debug_forward_plan / gsrast_debug_backward_plan under the row's switches
  (tests/test_policy.py drives the same two calls).
* The feature widths of tests/test_gpu_variants.py visit every chunk as a first pass and as the last pass behind a full 32.
* The refusals an un-culled state meets, each with its text."""
import ctypes as C
import itertools
import os
import re

import pytest

import variant_table as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUX, ANTIALIAS, ABSGRAD, POSEGRAD = 1, 2, 4, 8                                       # include/gsrast.h: the flags word
IN_RAW, IN_SH, IN_AUX_GRADS, IN_FULL_RECORD, IN_POSE_OUT, IN_POSE_SCRATCH, IN_ABS_SINK = 1, 2, 16, 32, 64, 128, 256      # gsrast_debug_backward_plan: words[5]
F_CULLED = 1 << 4
B_AUX, B_AA, B_CULL, B_TRANSPOSED, B_PICK_AUX, B_SPARSE, B_GROUPED, B_POSE = (1 << k for k in (0, 1, 12, 13, 14, 19, 20, 28))
B_ALL = B_AUX | B_AA | B_CULL | B_TRANSPOSED | B_PICK_AUX | B_SPARSE | B_GROUPED | B_POSE
P, W, H = 1532, 70, 45     # the per-Gaussian rows' scene (posegrad_math case a) at the blend rows' image


@pytest.fixture(scope="module")
def sources():
    out = {}
    for f in (vt.CAPI, vt.TRAIN):
        with open(os.path.join(ROOT, f)) as fh:
            out[f] = vt.strip_comments(fh.read())
    return out


# ---- 1. the table is complete ----------------------------------------------------------------------------------------------------------------
def _expected_args(site):
    prod = list(itertools.product(*site.values))
    if site.name == "preprocess_bwd":      # <RAW, SPARSE, GROUPED, AA, POSE>
        return [(raw, sp, gr, aa, pose) for raw, aa, pose in prod for sp, gr in vt.PREPROCESS_BWD_SHAPES.values()]
    return prod


def test_every_pick_of_the_sources_belongs_to_a_site(sources):
    claimed = {f: set() for f in sources}
    anchors = [(s.file, s.anchor) for s in vt.SITES] + list(vt.OUT_OF_SCOPE) + [(vt.CAPI, vt.PREPROCESS_BWD_LAUNCHES[1])]
    for f, anchor in anchors:
        text = sources[f]
        assert text.count(anchor) == 1, (f, anchor, text.count(anchor))
        pos = text.index(anchor)
        claimed[f] |= {(a, b) for a, b, _ in vt.picks_of(text) if a < pos < b}
    for f, text in sources.items():
        picks = vt.picks_of(text)
        assert picks, f
        loose = [text[a:a + 80].split("\n")[0] for a, b, _ in picks if (a, b) not in claimed[f]]
        assert not loose, (f, "a dispatch without a site in tests/variant_table.py", loose)
    assert sum(len(vt.picks_of(t)) for t in sources.values()) == 26      # (24 in gsrast_capi.hip, 2 in gsrast_train.hip)


@pytest.mark.parametrize("site", vt.SITES, ids=[s.name for s in vt.SITES])
def test_the_values_of_a_site_are_the_tables(site, sources):
    text = sources[site.file]
    found = vt.enclosing(vt.picks_of(text), text.index(site.anchor))
    assert found == site.values, (site.name, found)
    rows = vt.rows_of(site.name)
    want = _expected_args(site)
    assert sorted(r.args for r in rows) == sorted(want), (site.name, set(want) ^ {r.args for r in rows})
    assert len(rows) == len(set(r.args for r in rows)) == len(want)


def test_the_per_gaussian_backward_has_three_shapes(sources):
    """(SPARSE, GROUPED) is no pick of its own: the launch lambda is called twice, as <true, true> and as <sparse, false>."""
    text = sources[vt.CAPI]
    a = text.index("int per_gaussian()")
    body = text[a:text.index("GS_LAUNCHED(\"preprocess_bwd\")", a)]
    assert len(re.findall(r"\blaunch\(", body)) == 2 and all(body.count(c) == 1 for c in vt.PREPROCESS_BWD_LAUNCHES)
    assert "if (plan.grouped) " + vt.PREPROCESS_BWD_LAUNCHES[0] in body
    assert vt.enclosing(vt.picks_of(text), text.index(vt.PREPROCESS_BWD_LAUNCHES[1]))[-1] == vt.BOOLS
    assert sorted(vt.PREPROCESS_BWD_SHAPES.values()) == [(False, False), (True, False), (True, True)]


def test_the_table_has_no_row_without_a_site_and_names_tests_that_exist():
    sites = {s.name for s in vt.SITES}
    counts = dict(blend_fwd_cull=6, blend_fwd=9, blend_bwd_cull_t=12, blend_bwd_cull=9, blend_bwd=9, preprocess_fwd=4, preprocess_bwd=24, features_fwd=12,
                  features_bwd=12, contrib_blend=3, distort_fwd=3, distort_bwd=3, bilagrid_bwd_grid=5, hex_grad_tex_sorted=5)
    assert {s: len(vt.rows_of(s)) for s in sites} == counts and len(vt.ROWS) == sum(counts.values())
    texts = {}
    for r in vt.ROWS:
        assert r.site in sites and set(r.switches) <= set(vt.DEFAULTS), r
        path, name = r.test.split("::")
        if path not in texts:
            with open(os.path.join(ROOT, path)) as fh:
                texts[path] = fh.read()
        assert re.search(rf"^def {name}\(", texts[path], re.M), r.test
        assert "pytest.mark.gpu" in texts[path]
    # the train sites' values are those of the tests the rows name
    import bilagrid_math as bm
    assert {L for _, _, L in bm.GRIDS} | {16} == {r.args[0] for r in vt.rows_of("bilagrid_bwd_grid")} and "GRIDS = bm.GRIDS + [(64, 64, 16)]" in texts["tests/test_gpu_bilagrid.py"]
    m = re.search(r'parametrize\("W,H,C,mm", \[(.*?)\]\)\n@pytest.mark.parametrize\("scatter", \[0, 1\]\)\ndef test_single_plane_against_oracle', texts["tests/test_hexplane.py"], re.S)
    assert {int(t.split(",")[2]) for t in re.findall(r"\(([^()]*)\)", m.group(1))} == {r.args[0] for r in vt.rows_of("hex_grad_tex_sorted")}


def test_the_colour_dispatch_is_the_tables(sources):
    """color_kernels (gsrast_capi.hip) is a seven-way if / else, no pick: its launch texts, in source order, and the calls of color_kernels are
    exactly variant_table.COLOR_LAUNCHES / COLOR_CALLS -- a new launch site or call cannot appear without a row -- no colour kernel is
    launched anywhere else, and every row names a test case that exists."""
    text = sources[vt.CAPI]
    launch = re.compile(r"\b(preprocess_color_\w*kernel(?:<[^<>]*>)?)\s*<<<")
    head = "int color_kernels(" + vt.COLOR_KERNELS_SIGNATURE + ")"
    assert text.count(head) == 1
    a = text.index(head)
    b = text.index("int launch_color(", a)
    body = text[a:b]
    assert body.rstrip().endswith("}") and body.count("{") == body.count("}"), "color_kernels no longer ends where this test cuts it"
    assert tuple(launch.findall(body)) == tuple(r.launch for r in vt.COLOR_LAUNCHES)
    assert len(launch.findall(text)) == len(vt.COLOR_LAUNCHES), "a colour kernel is launched outside color_kernels"
    calls = re.findall(r"\bcolor_kernels\(([^()]*)\)", text)
    assert tuple(calls) == (vt.COLOR_KERNELS_SIGNATURE,) + tuple(r.args for r in vt.COLOR_CALLS)
    assert text.count("color_kernels") == len(calls), "color_kernels is named somewhere this test does not parse"
    # no other source file launches a colour kernel or calls color_kernels
    csrc = os.path.join(ROOT, os.path.dirname(vt.CAPI))
    for f in sorted(os.listdir(csrc)):
        if os.path.join(os.path.dirname(vt.CAPI), f) == vt.CAPI:
            continue
        with open(os.path.join(csrc, f)) as fh:
            other = vt.strip_comments(fh.read())
        assert not launch.search(other) and "color_kernels(" not in other, f
    # the kernels the launches name are the ones gsrast_preprocess.h defines: none is defined without a launch
    with open(os.path.join(csrc, "gsrast_preprocess.h")) as fh:
        defined = set(re.findall(r"^(preprocess_color_\w*kernel)\(", vt.strip_comments(fh.read()), re.M))
    assert defined == {r.launch.split("<")[0] for r in vt.COLOR_LAUNCHES}
    # every row names a test function, and a parametrisation id, that the named file holds
    texts = {}
    for r in vt.COLOR_LAUNCHES + vt.COLOR_CALLS:
        path, name = r.test.split("::")
        if path not in texts:
            with open(os.path.join(ROOT, path)) as fh:
                texts[path] = fh.read()
        m = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", name)
        assert m and re.search(rf"^def {m.group(1)}\(", texts[path], re.M) and "pytest.mark.gpu" in texts[path], r.test
        if m.group(2) is not None:      # the id is one of the names the test itself is parametrised with
            p = re.search(rf'parametrize\("name", (\w+|list\(CASES\))\)\ndef {m.group(1)}\(', texts[path])
            assert p, r.test
            ids = re.search(r"^CASES = \{(.*?)^\}", texts[path], re.M | re.S) if p.group(1) == "list(CASES)" else re.search(rf"^{p.group(1)} = \((.*?)\)$", texts[path], re.M)
            assert ids and f'"{m.group(2)}"' in ids.group(1), r.test
    assert len({r.launch for r in vt.COLOR_LAUNCHES}) == 7 and len({r.args for r in vt.COLOR_CALLS}) == 3


# ---- 2. the switches select what the row says ----------------------------------------------------------------------------------------------
@pytest.fixture()
def plans(rast):
    L = rast._C.lib()

    def forward(flags=0):
        words = (C.c_int * 6)(0, 0, 0, 0, 1 | 3 << 4, 0)
        return L.gsrast_debug_forward_plan(None, C.byref(rast._C._options_struct()), flags, P, W, H, words)

    def backward(flags=0, inputs=0):
        words = (C.c_int * 7)(P, 3, 5000, W, H, inputs | IN_SH, 1)
        return L.gsrast_debug_backward_plan(C.byref(rast._C._options_struct()), flags, words, None)
    return forward, backward, lambda: L.gsrast_last_error().decode()


def test_switches_of_the_blend_rows(rast, plans):
    forward, backward, _ = plans
    assert forward() & F_CULLED and backward() & (B_CULL | B_TRANSPOSED) == B_CULL | B_TRANSPOSED      # the defaults
    for r in vt.ROWS:
        if not r.site.startswith("blend_"):
            continue
        with vt.switched(rast, r.switches):
            o = rast._C._options_struct()
            assert o.exp_mode == r.args[0], r
            if r.site == "blend_fwd_cull":
                v = forward(AUX if r.args[1] else 0)
                assert v >= 0 and v & F_CULLED and o.fwd_pixels_per_lane == 0, r
            elif r.site == "blend_fwd":
                v = forward()
                assert v >= 0 and not v & F_CULLED and o.fwd_pixels_per_lane == r.args[1], r
            else:
                aux, ab = (r.args[1], r.args[2]) if r.site == "blend_bwd_cull_t" else (False, False)
                v = backward((AUX if aux else 0) | (ABSGRAD if ab else 0), (IN_AUX_GRADS if aux else 0) | (IN_FULL_RECORD | IN_ABS_SINK if ab else 0))
                assert v >= 0, r
                # bits 0, 1, 12, 13, 14, 19, 20, 28 and the pixels per lane in 21-23: at this size the per-Gaussian backward is the sparse, ungrouped one
                want = dict(blend_bwd_cull_t=B_CULL | B_TRANSPOSED, blend_bwd_cull=B_CULL, blend_bwd=0)[r.site] | (B_AUX | B_PICK_AUX if aux else 0) | B_SPARSE
                assert v & B_ALL == want, (r, bin(v))
                assert v >> 21 & 7 == (1 if r.site == "blend_bwd_cull_t" else r.args[1]), r
        assert rast._C._options_struct().exp_mode == 0 and rast._C.get_option("bwd_transposed") == 1      # (the defaults are back)
    # the grid of tests/test_gpu_variants.py: the forward reads its own pixels per lane, the backward its own
    for f, b in itertools.product(("culled", 1, 2, 4), vt.BACKWARDS):
        with vt.switched(rast, dict(vt.fwd_switches(f), **vt.bwd_switches(b))):
            v = backward()
            assert bool(v & B_CULL) == (not b.startswith("unculled")) and bool(v & B_TRANSPOSED) == (b == "transposed") and v >> 21 & 7 == int(b[-1] if b[-1].isdigit() else 1)
            # (an un-culled backward takes options.cull = 0, which the forward reads as well: behind a culled forward the test hands the backward its own options)
            assert bool(forward() & F_CULLED) == (f == "culled" and not b.startswith("unculled")), (f, b)


def test_switches_of_the_per_gaussian_rows(rast, plans):
    _, backward, _ = plans
    for r in vt.rows_of("preprocess_bwd"):
        raw, sparse, grouped, aa, pose = r.args
        flags = (ANTIALIAS if aa else 0) | (POSEGRAD if pose else 0)
        inputs = (IN_RAW if raw else 0) | (IN_FULL_RECORD | IN_POSE_OUT | IN_POSE_SCRATCH if pose else 0)
        with vt.switched(rast, r.switches):
            v = backward(flags, inputs)
        assert v >= 0, r
        want = (B_AA if aa else 0) | (B_SPARSE if sparse else 0) | (B_GROUPED if grouped else 0) | (B_POSE if pose else 0)
        assert v & B_ALL == want | B_CULL | B_TRANSPOSED and v >> 21 & 7 == 1, (r, bin(v))      # (behind the default blend backward)
    # late fill does not apply to the dense form, whatever late_fill_min_p says: the plan bit says so
    with vt.switched(rast, dict(dense_backward=1, late_fill_min_p=0)):
        assert not backward() & (B_SPARSE | B_GROUPED)
    assert backward() & (B_SPARSE | B_GROUPED) == B_SPARSE and rast._C.get_option("late_fill_min_p") == vt.DEFAULTS["late_fill_min_p"]


def test_the_defaults_are_the_librarys(rast):
    for k, v in vt.DEFAULTS.items():
        assert rast._C.get_option(k) == v, k


# ---- 3. the features rows ---------------------------------------------------------------------------------------------------------------------
def test_feature_widths_visit_every_chunk_first_and_last(sources):
    assert "inline int features_chunk(int C, int c0) { const int rem = C - c0; return rem > 16 ? 32 : rem > 8 ? 16 : rem > 4 ? 8 : 4; }" in sources[vt.CAPI]
    for C_, want in ((1, [4]), (4, [4]), (5, [8]), (8, [8]), (9, [16]), (16, [16]), (17, [32]), (32, [32]), (33, [32, 4]), (36, [32, 4]), (37, [32, 8]), (40, [32, 8]),
                     (41, [32, 16]), (48, [32, 16]), (49, [32, 32]), (63, [32, 32]), (64, [32, 32])):
        assert vt.feature_passes(C_) == want, C_
    passes = [vt.feature_passes(c) for c in vt.FEATURE_WIDTHS]
    assert {p[0] for p in passes if len(p) == 1} == set(vt.CHUNKS)
    assert {p[1] for p in passes if len(p) == 2 and p[0] == 32} == set(vt.CHUNKS)
    for c in vt.CHUNKS:      # both edges of every chunk: its full width and one channel past the next smaller one
        assert c in vt.FEATURE_WIDTHS and 32 + c in vt.FEATURE_WIDTHS + (64,)
    # the widths of the test a row names produce the row's chunk: mode 0 by FEATURE_WIDTHS, modes 1 and 2 by the split test, which runs the
    # forward AND the backward on F, F[:, :k] and F[:, k:] -- both read from the GPU file's own parametrisation
    with open(os.path.join(ROOT, "tests/test_gpu_variants.py")) as fh:
        gpu = fh.read()
    assert re.search(r'parametrize\("C", vt\.FEATURE_WIDTHS\)\n@pytest\.mark\.parametrize\("name", list\(cm\.CASES\)\)\ndef test_feature_chunks_against_fp64\(', gpu)
    assert re.search(r'parametrize\("C,k", vt\.FEATURE_SPLITS\)\n@pytest\.mark\.parametrize\("name", list\(cm\.CASES\)\)\n@pytest\.mark\.parametrize\("exp_mode", \[0, 1, 2\]\)\n'
                     r'def test_feature_columns_do_not_depend_on_their_chunk\(', gpu)
    split_passes = {p for c, k in vt.FEATURE_SPLITS for w in (c, k, c - k) for p in vt.feature_passes(w)}
    assert split_passes == set(vt.CHUNKS) and vt.FEATURE_SPLITS[1:] == ((13, 5), (40, 8), (48, 16))
    reached = {"test_feature_chunks_against_fp64": {p for c in vt.FEATURE_WIDTHS for p in vt.feature_passes(c)}, "test_feature_columns_do_not_depend_on_their_chunk": split_passes}
    for r in vt.rows_of("features_fwd") + vt.rows_of("features_bwd"):
        assert vt.feature_passes(r.keywords["features"]) == [r.args[1]]
        assert r.args[1] in reached[r.test.split("::")[1]] and (r.args[0] == 0) == r.test.endswith("test_feature_chunks_against_fp64"), r
    import features_math as fm
    assert fm.CHANNELS == (1, 3, 19, 64) and {p for c in fm.CHANNELS for p in vt.feature_passes(c)} == {4, 32}      # (what the older matrix reaches)


# ---- 4. refusals, each with its text ----------------------------------------------------------------------------------------------------------
def test_refusals_of_an_unculled_state_keep_their_texts(rast, plans):
    forward, backward, error = plans
    aux_text = "forward: acc_depth / alpha need the culled blend kernel (options.cull != 0, fwd_pixels_per_lane == 0)"
    for sw in (dict(cull=0), dict(fwd_pixels_per_lane=1), dict(fwd_pixels_per_lane=2), dict(fwd_pixels_per_lane=4)):
        with vt.switched(rast, sw):
            assert forward(AUX) == -1 and error() == aux_text, sw
            assert forward() >= 0
    with vt.switched(rast, dict(cull=0)):
        assert backward(ABSGRAD, IN_FULL_RECORD | IN_ABS_SINK) == -1
        assert error() == "backward: GSRAST_RENDER_ABSGRAD needs the transposed blend backward (options.cull != 0, no ablation kernel)"
        assert backward(AUX, IN_AUX_GRADS) == -1 and error() == "backward: acc_depth / alpha gradients need the culled blend kernels (options.cull != 0)"
        with pytest.raises(RuntimeError) as e:
            rast._C._distortion_aux((None, None), None, None, H, W, None, None)
        assert str(e.value) == "distortion=True: the gradient of the distortion map needs the culled blend kernels (options.cull != 0)"
        with pytest.raises(RuntimeError, match="distortion=True: the gradient"):      # ... and with the options a forward stored
            rast._C._distortion_aux((None, None), None, None, H, W, None, dict(rast._C.current_options()))
        assert rast._C._distortion_aux(None, None, None, H, W, None, None) is None      # (without the keyword: nothing to refuse)
    for ppl in (1, 2, 4):      # a forced forward template is no refusal of the backward's: absgrad and the distortion gradient run behind it
        with vt.switched(rast, dict(fwd_pixels_per_lane=ppl)):
            v = backward(ABSGRAD, IN_FULL_RECORD | IN_ABS_SINK)
            assert v >= 0 and v & B_TRANSPOSED
            v = backward(AUX, IN_AUX_GRADS)
            assert v >= 0 and v & B_PICK_AUX
    assert backward(ABSGRAD, IN_FULL_RECORD | IN_ABS_SINK) >= 0 and forward(AUX) & F_CULLED
