"""-m gpu: every instantiation of the renderer's run-time template dispatch (tests/variant_table.py: one row each) run against a reference.

Scenes: contrib_math.CASES a and b, 70 x 45 = 5 x 3 ragged tiles (a: a tile list longer than two 256-entry batches, an opaque stack, culled
Gaussians; b: 2000 sparse Gaussians, two empty tiles) -- the smallest in the tree that cross every staged batch size of the table (64, 128,
256); absgrad_math case a / d for the ABS kernels, posegrad_math's cases for the per-Gaussian backward.  Upstream gradients are zero on the
fp64 reference's own fp32-ambiguous pixels (under 5 % of each case, asserted).  That a family ran is read from the profile table's launch
counts in a window around the call; WHICH instantiation the switches select is pinned by tests/test_variants_host.py on the host-side plans.
Every test prints its worst err / bar.

(a) Feature chunks.  Map bar: 4 x the fp32 restatement's own error (features_math.restate32) as a max|ref| + r |ref|, measured on the CPU
over cases a and b, plain, C in {4, 5, 8, 9, 13, 16, 17, 19, 32, 33, 36, 37, 40, 41, 48, 49, 63} by distort_math.map_bar_terms:
    a = 1.671e-6 (case b, C = 40)      r = 2.629e-5 (case b, C = 8)      MAP_BAR = (1.68e-6, 2.63e-5)
(tests/test_gpu_features.py's pair, 1.42e-6 / 1.85e-5, was measured over C in {1, 3, 19, 64} and is a little below it).  Gradients:
conftest.grad_tol(ref64, ref32).  In every exp_mode the map's columns are held bit for bit under a permutation of the channels and under a
split of F: channels accumulate independently (one fma chain per pixel and channel), so a column's bits may not depend on the chunk or the
slot it lands in.  dL/dfeatures is a sum over pixels and is NOT such a chain: features_bwd_kernel sums the 64 lanes of a wave with
wave_sum8_transposed, whose association order depends on the slot (lane & 7: the row's four quads are added as (q0 + q4) + (q8 + q12) in slots
0-3 and as (q4 + q8) + (q12 + q0) in slots 4-7), then the four waves through LDS float atomics and the tiles through global ones.  So the permuted
call's dL/dfeatures is held to the permuted gradient at grad_tol of the fp64 gradient, like the geometry leaves (float atomics), and the
test prints how many of its entries differ in their bits; the two parts of a split run their backward too, each dL/dfeatures held to the
full call's columns at the same bar (measured on the MI355X: 0.7 % - 4.3 % of the entries, in every mode, mode 0
included; worst err / bar of the permuted call against the unpermuted one under 0.1).

(b) The blend grid: exp_mode x forward {culled, un-culled at 1 / 2 / 4 pixels per lane} x backward {transposed, culled 1 / 2 / 4, un-culled
1 / 2 / 4}, colour loss, through gpu_harness.run_hip.  options.cull is read by both directions and the autograd node hands the backward the
forward's options, so an un-culled backward behind a CULLED forward gets its own options the way a C caller passes them: per call
(_backward_options).  Gradient reference in modes 1 and 2: see GRADIENT_REFERENCE below.

(c) The replays (contrib, features, distortion) on the state an un-culled forward left.  (d) preprocess_bwd_kernel in its 24 shapes.
(e) blend_bwd_cull_t_kernel<MODE, AUX, ABS> with the absgrad sink in every mode."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import absgrad_math as am
import contrib_math as cm
import distort_math as dm
import features_math as fm
import math_renderer as mr
import posegrad_math as pm
import variant_table as vt
from conftest import grad_tol, settings_from
from gpu_harness import bits, run_hip

pytestmark = pytest.mark.gpu

MAP_BAR = (1.68e-6, 2.63e-5)      # (a, r): the map's bar is 4 x (a max|ref| + r |ref|), measured for vt.FEATURE_WIDTHS (module docstring)
# Which reference the gradients of a mode are held to at conftest.grad_tol(o64, o32) of the fp64 oracle's gradient.  "fp64": the fp64 oracle
# itself (upstream zero on the ambiguous pixels).  "default": the same mode's default kernels (culled forward, transposed backward), device
# against device -- for a mode whose default kernels do not meet the fp64 bar because another exp flips decisions the mask does not cover.
# Measured on the MI355X, default kernels against fp64, worst err / bar over the six gradient tensors (test_blend_grid prints it):
#     exp_mode 0: case a 0.024, case b 0.193      exp_mode 1: case a 0.026, case b 0.226      exp_mode 2: case a 0.029, case b 0.129
# The default kernels of modes 1 and 2 meet the fp64 bar with the margin mode 0 has, so every variant of every mode is held to fp64; the
# absgrad sink of (e) likewise (worst err / bar 0.009 in every mode), and so are the replays' feature and distortion gradients of (c), whose
# default forward is asserted against fp64 in every mode before its variants are (measured, worst err / bar of the default forward: features
# 0.129 / 0.129 / 0.130 and distortion 0.120 / 0.124 / 0.124 in modes 0 / 1 / 2, all case b).
GRADIENT_REFERENCE = {0: "fp64", 1: "fp64", 2: "fp64"}
GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations")
FORWARDS = ("culled", 1, 2, 4)


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _np(x):
    return x.detach().double().cpu().numpy()


@contextlib.contextmanager
def _launches(rast):
    """The profile table's launch counts of the window: the dict is filled on the way out."""
    _C = rast._C
    counts = {}
    _C.set_option("profile", -1)
    try:
        _C.profile_reset()
        yield counts
        counts.update({k: v[1] for k, v in _C.profile_read().items()})
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()


@contextlib.contextmanager
def _backward_options(rast, override):
    """The backwards inside run with `override` on top of the options their forward stored (per-call options only): what a C caller does
    by passing another gsrast_options to gsrast_render_backward."""
    _C = rast._C
    if not override:
        yield
        return
    assert set(override) <= set(_C.PER_CALL_OPTIONS)
    orig = _C.rasterize_gaussians_backward

    def with_override(*a, options=None, **kw):
        return orig(*a, options=dict(_C.current_options() if options is None else options, **override), **kw)
    _C.rasterize_gaussians_backward = with_override
    try:
        yield
    finally:
        _C.rasterize_gaussians_backward = orig


def _worst(got, want, tol):
    return float((np.abs(got - want) / np.maximum(tol, 1e-300)).max())


def _check_grads(got, want, r64, r32, what, names=None):
    """got against want (fp64 reference, or another device run) at grad_tol(r64, r32) per tensor; prints the worst err / bar."""
    worst = ("", 0.0)
    for n in (names or r64):
        assert n in got, (what, n, "the device side produced no gradient of this name")
        tol = grad_tol(r64[n].reshape(got[n].shape), r32[n].reshape(got[n].shape) if r32 is not None and n in r32 else None)
        ratio = _worst(got[n], np.asarray(want[n], np.float64).reshape(got[n].shape), tol)
        worst = max(worst, (n, ratio), key=lambda x: x[1])
        assert np.abs(got[n]).max() > 0 or n in ("shs", "features_dc", "features_rest"), (what, n)
        assert ratio <= 1.0, (what, n, ratio, float(np.abs(r64[n]).max()))
    print(f"{what}: worst gradient err / bar {worst[1]:.3f} ({worst[0]})")
    return worst[1]


def _check_map(got, ref, amb, what):
    a, r = MAP_BAR
    ok = ~amb
    err = np.abs(got - ref)[:, ok]
    tol = 4.0 * (a * np.abs(ref[:, ok]).max() + r * np.abs(ref[:, ok]))
    print(f"{what}: map max|err| {err.max():.3e} max|ref| {np.abs(ref[:, ok]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
    assert not np.isnan(got).any(), "a pixel of the map was not written"
    assert (err <= tol).all(), (what, float(err.max()), float((err / tol).max()))


# ---- (a) feature chunks ------------------------------------------------------------------------------------------------------------------------
def _features(rast, gpu, r, F=None, **kw):
    import test_gpu_features as tgf
    return tgf._render(rast, gpu, r["sc"], r["cam"], r["F"] if F is None else F, **kw)


@pytest.mark.parametrize("C", vt.FEATURE_WIDTHS)
@pytest.mark.parametrize("name", list(cm.CASES))
def test_feature_chunks_against_fp64(name, C, rast, gpu):
    r = fm.reference(name, C)
    r64, r32 = r["r64"], r["r32"]
    assert r64["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    with _launches(rast) as n:
        h = _features(rast, gpu, r, g1=r64["g1"], g0=r64["g0"])
    assert n["features_fwd"] == 1 and n["features_bwd"] == 1 and n["blend_fwd"] >= 1 and n["blend_bwd"] == 1 and n["preprocess_bwd"] == 1, n
    assert np.array_equal(h["out"][1].cpu().numpy() > 0, r64["vis"]), "radius decision differs: pick another seed"
    assert tuple(h["map"].shape) == (C,) + r64["amb"].shape and len(h["out"]) == 4
    what = f"features_fwd / features_bwd <0, {vt.feature_passes(C)}>: case {name}, C {C}"
    _check_map(_np(h["map"]), r64["map"], r64["amb"], what)
    _check_grads(h["grads"], r64["grads"], r64["grads"], r32["grads"], what)
    gF = h["grads"]["features"]      # culled and never-blended Gaussians: exactly zero rows
    assert not gF[~r64["vis"]].any() and np.array_equal(gF.any(1), r64["grads"]["features"].any(1))


@pytest.mark.parametrize("C,k", vt.FEATURE_SPLITS)
@pytest.mark.parametrize("name", list(cm.CASES))
@pytest.mark.parametrize("exp_mode", [0, 1, 2])
def test_feature_columns_do_not_depend_on_their_chunk(exp_mode, name, C, k, rast, gpu):
    """Device against device in every exp_mode (the fp64 reference belongs to mode 0 and only scales the gradient bar here): the map of
    F[:, perm] is the permuted map and the maps of F[:, :k] / F[:, k:] are the two parts of the map, bit for bit; dL/dfeatures and the
    geometry leaves of the permuted call at grad_tol of the fp64 gradient (module docstring).  The two parts run their backward as well, on
    their slice of the upstream gradient alone: dL/dF[i][c] = sum_p w_ip g1[c][p] depends on no other channel, so each part's dL/dfeatures
    is the full call's columns, at the same bar.  C = 12, k = 4 is the split whose head is one pass of four channels."""
    r = fm.reference(name, C)
    r64, r32, F = r["r64"], r["r32"], r["F"]
    perm = np.random.default_rng(100 * C + k).permutation(C)
    assert (perm != np.arange(C)).sum() > C // 2 and {p // 8 for p in perm[:8]} != {0}      # columns change their slot and their group of eight
    with vt.switched(rast, dict(exp_mode=exp_mode)), _launches(rast) as n:
        full = _features(rast, gpu, r, g1=r64["g1"], g0=r64["g0"])
        moved = _features(rast, gpu, r, F=np.ascontiguousarray(F[:, perm]), g1=np.ascontiguousarray(r64["g1"][perm]), g0=r64["g0"])
        head = _features(rast, gpu, r, F=np.ascontiguousarray(F[:, :k]), g1=np.ascontiguousarray(r64["g1"][:k]))
        tail = _features(rast, gpu, r, F=np.ascontiguousarray(F[:, k:]), g1=np.ascontiguousarray(r64["g1"][k:]))
    assert n["features_fwd"] == 4 and n["features_bwd"] == 4 and n["blend_bwd"] == 4, n
    what = f"features <{exp_mode}, {vt.feature_passes(C)} / {vt.feature_passes(k)} + {vt.feature_passes(C - k)}>: case {name}, C {C}"
    m = full["map"].detach()
    assert not torch.isnan(m).any() and float(m.abs().max()) > 0
    idx = torch.as_tensor(perm, device=gpu)
    assert torch.equal(moved["map"].detach(), m[idx]), (what, int((moved["map"].detach() != m[idx]).sum()), "entries of the permuted map differ")
    assert torch.equal(head["map"].detach(), m[:k]) and torch.equal(tail["map"].detach(), m[k:]), (what, "a column's bits depend on the chunk it lands in")
    for part, cols in ((head, slice(0, k)), (tail, slice(k, C))):
        sub = lambda g: dict(features=g["features"][:, cols])      # noqa: E731
        assert np.array_equal(part["grads"]["features"].any(1), full["grads"]["features"].any(1))
        _check_grads(part["grads"], sub(full["grads"]), sub(r64["grads"]), sub(r32["grads"]), what + f", dL/dfeatures of F[:, {cols.start}:{cols.stop}] against the full call's columns")
    want = dict(full["grads"], features=full["grads"]["features"][:, perm])
    ref64 = dict(r64["grads"], features=r64["grads"]["features"][:, perm])
    ref32 = dict(r32["grads"], features=r32["grads"]["features"][:, perm])
    print(f"{what}: {int((moved['grads']['features'] != want['features']).sum())} of {want['features'].size} entries of dL/dfeatures differ in their bits")
    assert np.array_equal(moved["grads"]["features"].any(1), want["features"].any(1))
    _check_grads(moved["grads"], want, ref64, ref32, what + ", permuted against unpermuted")
    if exp_mode == 0:
        _check_grads(moved["grads"], ref64, ref64, ref32, what + ", permuted against fp64")


# ---- (b) the blend grid ------------------------------------------------------------------------------------------------------------------------
_blend_cases, _blend_defaults = {}, {}


def _blend_case(name, orc, scenes):
    if name not in _blend_cases:
        r = cm.reference(name)
        sc, cam, amb = r["sc"], r["cam"], r["amb"]
        H, W = amb.shape
        g = (scenes.upstream_grad(H, W, 31) * (H * W)).astype(np.float32)
        g[:, amb] = 0.0
        orc.set_exp_mode(0)
        _blend_cases[name] = dict(sc=sc, cam=cam, amb=amb, g=g, o32=orc.render(sc, cam, g), o64=orc.render(sc, cam, g, f64=True))
    return _blend_cases[name]


def _grid_switches(fwd, bwd):
    """(the thread's switches of one forward x backward pair, the backward's own per-call options where the two disagree on options.cull)."""
    f, b = vt.fwd_switches(fwd), vt.bwd_switches(bwd)
    if fwd == "culled" and b["cull"] == 0:
        return dict(f, **{k: v for k, v in b.items() if k != "cull"}), dict(cull=0)
    return dict(f, **b), None


def _run_blend(rast, gpu, c, mode, fwd, bwd):
    thread, override = _grid_switches(fwd, bwd)
    with vt.switched(rast, dict(exp_mode=mode, **thread)), _backward_options(rast, override), _launches(rast) as n:
        h = run_hip(rast, c["sc"], c["cam"], gpu, dL_dcolor=c["g"], exp_mode=mode)
    assert n["blend_fwd"] >= 2 and n["blend_bwd"] == 1 and n["preprocess_bwd"] == 1, (fwd, bwd, n)
    return h


def _blend_default(rast, gpu, name, mode, c):
    """The default kernels of a mode (culled forward, transposed backward) on a case, once per process, and their worst err / bar against fp64."""
    if (name, mode) not in _blend_defaults:
        h = _run_blend(rast, gpu, c, mode, "culled", "transposed")
        ratios = {k: _worst(h[k].astype(np.float64).reshape(c["o64"][k].shape), c["o64"][k], grad_tol(c["o64"][k], c["o32"][k])) for k in GRADS}
        print(f"case {name}, exp_mode {mode}: default kernels against the fp64 oracle, worst err / bar {max(ratios.values()):.3f} "
              + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        _blend_defaults[name, mode] = h
    return _blend_defaults[name, mode]


def _tile_max_of(rast, gpu, sc, cam):
    """(tile_max u32[T] read from the image buffer, n_contrib [H,W]) of one low-level forward under the calling thread's options.  The offsets
    restate gsrast_common.h: img_layout (final_T f32[N] | n_contrib u32[N] | ranges uint2[T] | tile_max u32[T], each rounded up to 256 bytes);
    final_T and n_contrib read at those offsets must be gsrast_debug_export's."""
    _C = rast._C
    rs = settings_from(rast, cam, sc, gpu)
    H, W, P = rs.image_height, rs.image_width, sc["means3D"].shape[0]
    e = torch.empty(0)
    ten = {k: _t(sc[k], gpu) for k in fm.DENSE}
    R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix,
                                                                rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, ten["shs"], rs.sh_degree, rs.campos, False)
    st = _C.debug_export(P, R, W, H, gb, bb, ib)
    torch.cuda.synchronize()
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    up = lambda b: (b + 255) & ~255      # noqa: E731
    o_nc = up(N * 4)
    o_tm = o_nc + up(N * 4) + up(T * 8)
    raw = ib.cpu().numpy()
    nc = st["n_contrib"].cpu().numpy().view(np.uint32).reshape(H, W)
    assert np.array_equal(raw[:N * 4].view(np.uint32), bits(st["final_T"].cpu().numpy()).reshape(-1)) and np.array_equal(raw[o_nc:o_nc + N * 4].view(np.uint32), nc.reshape(-1))
    return raw[o_tm:o_tm + T * 4].view(np.uint32).copy(), nc


@pytest.mark.parametrize("name", list(cm.CASES))
@pytest.mark.parametrize("fwd", FORWARDS, ids=[f"fwd_{f}" for f in FORWARDS])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_blend_grid(mode, fwd, name, orc, scenes, rast, gpu):
    """One (mode, forward) pair with its seven backwards.  Forward: out_color, out_depth, radii, final_T, n_contrib (and the lists) are the
    default forward's of the same mode bit for bit -- in mode 0 also the oracle's --, tile_max is the per-tile maximum of n_contrib.
    Gradients: GRADIENT_REFERENCE[mode] at grad_tol(o64, o32)."""
    from test_gpu_parity import _check_forward_exact
    c = _blend_case(name, orc, scenes)
    assert c["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    o64, o32 = c["o64"], c["o32"]
    base = _blend_default(rast, gpu, name, mode, c)
    target = o64 if GRADIENT_REFERENCE[mode] == "fp64" else base
    for bwd in vt.BACKWARDS:
        h = _run_blend(rast, gpu, c, mode, fwd, bwd)
        what = f"blend <{mode}> forward {fwd} backward {bwd}, case {name}"
        assert h["R"] == base["R"]
        for k in ("out_color", "out_depth", "radii", "final_T", "n_contrib", "point_list", "ranges"):
            assert np.array_equal(bits(h[k]), bits(base[k])), (what, k, "differs from the default forward of the mode")
        if mode == 0:
            _check_forward_exact(o32, h)
        worst = ("", 0.0)
        for k in GRADS:
            ratio = _worst(h[k].astype(np.float64).reshape(o64[k].shape), np.asarray(target[k], np.float64).reshape(o64[k].shape), grad_tol(o64[k], o32[k]))
            worst = max(worst, (k, ratio), key=lambda x: x[1])
            assert np.abs(h[k]).max() > 0, (what, k)
            assert not h[k].reshape(o64[k].shape[0], -1)[o32["radii"] == 0].any(), (what, k, "a culled Gaussian's row is not zero")
        print(f"{what}: worst gradient err / bar {worst[1]:.3f} ({worst[0]}, against {GRADIENT_REFERENCE[mode]})")
        assert worst[1] <= 1.0, (what, worst)
    with vt.switched(rast, dict(exp_mode=mode, **vt.fwd_switches(fwd))):
        tm, nc = _tile_max_of(rast, gpu, c["sc"], c["cam"])
    H, W = nc.shape
    pad = np.zeros((3 * 16, 5 * 16), np.uint32)
    pad[:H, :W] = nc
    assert np.array_equal(tm, pad.reshape(3, 16, 5, 16).max(axis=(1, 3)).reshape(-1)), (mode, fwd, name, "tile_max is not the per-tile maximum of n_contrib")
    assert tm.max() > 512 or name != "a"      # (case a: pixels that walk more than two 256-entry batches)


# ---- (c) the replays on the state an un-culled forward left -----------------------------------------------------------------------------------
REPLAY_FORWARDS = dict(cull_0=dict(cull=0), ppl_1=dict(cull=1, fwd_pixels_per_lane=1), ppl_2=dict(cull=1, fwd_pixels_per_lane=2), ppl_4=dict(cull=1, fwd_pixels_per_lane=4))
_replay_defaults = {}


def _replays(rast, gpu, name, aa, mode, with_distortion_grad=True):
    """Under the calling thread's switches: the contrib sink, the feature maps (C = 19, 40) with their gradients, the distortion map with its."""
    import test_gpu_contrib as tgc
    import test_gpu_distort as tgd
    rc = cm.reference(name, aa)
    out = dict(sink=tgc._render(rast, gpu, rc["sc"], rc["cam"], weights=rc["weights"], aa=aa)["sink"])
    for C in (19, 40):
        r = fm.reference(name, C, aa=aa)
        out[C] = _features(rast, gpu, r, aa=aa, g1=r["r64"]["g1"], g0=r["r64"]["g0"])
    rd = dm.reference(name, "antialias" if aa else "plain")
    if with_distortion_grad:
        out["distort"] = tgd._render(rast, gpu, rd["sc"], rd["cam"], aa=aa, g=rd["r64"]["g"])
    else:
        with torch.no_grad():
            out["distort"] = tgd._render(rast, gpu, rd["sc"], rd["cam"], aa=aa)
    return out


@pytest.mark.parametrize("name,aa", [("a", False), ("b", True)], ids=["a_plain", "b_antialias"])
@pytest.mark.parametrize("fwd", list(REPLAY_FORWARDS))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_replays_on_unculled_states(mode, fwd, name, aa, rast, gpu):
    """contrib_blend_kernel<MODE>, features_*_kernel<MODE, 32 | 32 + 8>, distort_*_kernel<MODE> on a forward with cull = 0 or a forced
    fwd_pixels_per_lane: sink and maps are the default forward's bit for bit; the gradients of the feature loss (all forwards) and of the
    distortion loss (cull = 1) meet fp64 in every mode, as the default forward's do (asserted first); with cull = 0 the
    distortion gradient raises and the next plain render succeeds."""
    import test_gpu_distort as tgd
    sw = REPLAY_FORWARDS[fwd]
    culled_bwd = sw["cull"] == 1
    if (name, aa, mode) not in _replay_defaults:
        with vt.switched(rast, dict(exp_mode=mode)):
            _replay_defaults[name, aa, mode] = d = _replays(rast, gpu, name, aa, mode)
        for C in (19, 40):      # the default forward of the mode against fp64: what decides the reference of its variants (GRADIENT_REFERENCE)
            r = fm.reference(name, C, aa=aa)
            _check_grads(d[C]["grads"], r["r64"]["grads"], r["r64"]["grads"], r["r32"]["grads"], f"replays <{mode}> on the default forward, case {name}, features C {C} against fp64")
        rd = dm.reference(name, "antialias" if aa else "plain")
        _check_grads(d["distort"]["grads"], rd["r64"]["grads"], rd["r64"]["grads"], rd["r32"]["grads"], f"replays <{mode}> on the default forward, case {name}, distortion against fp64")
    base = _replay_defaults[name, aa, mode]
    with vt.switched(rast, dict(exp_mode=mode, **sw)), _launches(rast) as n:
        got = _replays(rast, gpu, name, aa, mode, with_distortion_grad=culled_bwd)
    assert n["contrib_blend"] == 1 and n["features_fwd"] == 2 and n["features_bwd"] == 2 and n["distort_fwd"] == 1 and n["distort_bwd"] == int(culled_bwd), n
    assert n["blend_fwd"] >= 4 and n["blend_bwd"] == 2 + int(culled_bwd), n
    what = f"replays <{mode}> on forward {fwd}, case {name}{' antialias' if aa else ''}"
    assert not torch.isnan(got["sink"]).any() and torch.equal(got["sink"], base["sink"]), (what, "contrib sink")
    for C in (19, 40):
        assert torch.equal(got[C]["out"][0], base[C]["out"][0]) and torch.equal(got[C]["map"], base[C]["map"]), (what, f"feature_map, C {C}")
        r = fm.reference(name, C, aa=aa)
        _check_grads(got[C]["grads"], r["r64"]["grads"], r["r64"]["grads"], r["r32"]["grads"], f"{what}, features C {C} against fp64")
    assert torch.equal(got["distort"]["map"], base["distort"]["map"]) and float(got["distort"]["map"].detach().max()) > 0, (what, "distort_map")
    rd = dm.reference(name, "antialias" if aa else "plain")
    if culled_bwd:
        _check_grads(got["distort"]["grads"], rd["r64"]["grads"], rd["r64"]["grads"], rd["r32"]["grads"], f"{what}, distortion against fp64")
    else:
        with vt.switched(rast, dict(exp_mode=mode, **sw)):
            with pytest.raises(RuntimeError, match=r"distortion=True: the gradient of the distortion map needs the culled blend kernels \(options.cull != 0\)"):
                tgd._render(rast, gpu, rd["sc"], rd["cam"], aa=aa, g=rd["r64"]["g"])
            torch.cuda.synchronize()
            after = tgd._render(rast, gpu, rd["sc"], rd["cam"], aa=aa, distortion=False, g=dict(g0=rd["r64"]["g"]["g0"]))      # the process lives on
            assert torch.equal(after["out"][0], base["distort"]["out"][0]) and np.abs(after["grads"]["means3D"]).max() > 0


# ---- (d) preprocess_bwd_kernel<RAW, SPARSE, GROUPED, AA, POSE> in its 24 shapes ----------------------------------------------------------------
POSE_CASES = dict(dense=("a", None), dense_aa=("e", None), raw=("b", None), raw_aa=("b", dict(raw=True, aa=True)))      # posegrad_math letter; a variant beside pm.VARIANTS


def _raw_chain(raw, dense_grads):
    """The gradients of GaussianRasterizerRaw's leaves (posegrad_math.raw_leaves' activations, fp64) from those of the dense inputs."""
    l = {n: torch.as_tensor(np.asarray(v, np.float64)).requires_grad_(True) for n, v in raw.items()}
    q = l["rotation"] + l["rot_res"][:, :4]
    acts = dict(means3D=l["xyz"] + l["motion_res"], rotations=q / torch.linalg.norm(q, dim=1, keepdim=True), scales=torch.exp(l["scaling"] + l["rot_res"][:, 4:]),
                opacities=l["trbf"] * torch.sigmoid(l["opacity_logit"]), shs=torch.cat([l["features_dc"], l["features_rest"]], 1) + l["shs_res"])
    names = list(acts)
    torch.autograd.backward([acts[n] for n in names], [torch.as_tensor(np.asarray(dense_grads[n], np.float64)).reshape(acts[n].shape) for n in names])
    return {n: x.grad.numpy() for n, x in l.items()}


@functools.lru_cache(maxsize=None)
def _pose_reference(key):
    """posegrad_math.reference for the three variants it has; raw + aa built beside it the way posegrad_math._reference builds them.  Raw: the
    leaves' fp64 / fp32 gradients by the activations' chain rule in fp64 (leaf64 / leaf32)."""
    import scenes
    import test_gpu_independent as tgi
    letter, v = POSE_CASES[key]
    if v is None:
        r = dict(pm.reference(letter))
    else:
        c = next(k for k in tgi.CASES if k["name"].startswith(letter + "_"))
        sc, cam, names = tgi._case_inputs(scenes, c)
        raw = pm.raw_leaves(sc, c["seed"])
        cfg = pm.cfg_of(cam, sc, c, aa=True)
        r64, r32 = pm.reference_pair(sc, cam, names, cfg, c)
        r = dict(v, c=c, sc=sc, cam=cam, names=names, cfg=cfg, raw=raw, r64=r64, r32=r32)
    if r.get("raw"):
        assert float(r["cam"].get("scale_modifier", 1.0)) == 1.0
        r["leaf64"], r["leaf32"] = _raw_chain(r["raw"], r["r64"]["want"]), _raw_chain(r["raw"], r["r32"]["want"])
    else:
        r["leaf64"], r["leaf32"] = ({n: w["want"][n] for n in r["names"]} for w in (r["r64"], r["r32"]))
    # means2D.grad as features_math.restate32 derives it: every Gaussian has its own copy of projmatrix, hom = [mean, 1] @ copy, so the copy's
    # gradient row 3 is dL/dhom, and dL/dndc.xy = dL/dhom.xy / p_w with 1 / p_w = hom.w + C_WEPS
    m = np.asarray(r["sc"]["means3D"], np.float64)
    hw = (np.concatenate([m, np.ones_like(m[:, :1])], 1) @ np.asarray(r["cam"]["projmatrix"], np.float64))[:, 3] + mr.C_WEPS
    for leaf, w in ((r["leaf64"], r["r64"]), (r["leaf32"], r["r32"])):
        leaf["means2D"] = w["terms"]["projmatrix"][:, 3, :2] * hw[:, None]
    return r


@pytest.mark.parametrize("shape", list(vt.PREPROCESS_BWD_SHAPES))
@pytest.mark.parametrize("pose", [False, True], ids=["no_pose", "pose"])
@pytest.mark.parametrize("key", list(POSE_CASES))
def test_preprocess_bwd_in_every_shape(key, pose, shape, rast, gpu):
    import test_gpu_posegrad as tgp
    r = _pose_reference(key)
    raw, aa = bool(r.get("raw")), bool(r.get("aa"))
    row = next(x for x in vt.rows_of("preprocess_bwd") if x.args == (raw,) + vt.PREPROCESS_BWD_SHAPES[shape] + (aa, pose))
    r64 = r["r64"]
    assert r64["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    with vt.switched(rast, row.switches), _launches(rast) as n:
        rs = tgp._settings(rast, r["cam"], r["sc"], gpu, grad=pose)
        run = tgp._render(rast, r, rs, gpu, True if pose else None)
    assert n["preprocess_bwd"] == 1 and n["preprocess_fwd"] == 1 and n["blend_bwd"] == 1, n
    # grouped = late fill wanted AND the side stream had: late_rows_zero_kernel runs beside the blend backward with that shape and no other
    assert n["late_rows_zero"] == int(shape == "grouped"), (shape, n["late_rows_zero"], "the row's shape is not the one that ran")
    assert np.array_equal(run["res"][1].cpu().numpy() > 0, r64["out"]["vis"]), "radius decision differs: pick another seed"
    what = f"preprocess_bwd <{', '.join(str(int(a)) for a in row.args)}> ({key}, {shape}{', pose' if pose else ''})"
    got = {k: _np(x.grad) for k, x in run["leaves"].items()}
    got["means2D"] = _np(run["m2"].grad)[:, :2]
    assert set(got) == set(r["leaf64"])
    _check_grads(got, r["leaf64"], r["leaf64"], r["leaf32"], what + ", leaves")
    if pose:
        cam_got = tgp._camera_grads(rs)
        worst = 0.0
        for k in pm.CAMERA:
            ratio = _worst(cam_got[k], r64["want"][k], grad_tol(r64["want"][k], r["r32"]["want"][k]))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, k, ratio)
        assert np.abs(cam_got["viewmatrix"]).max() > 0
        tgp._assert_structural_zeros(cam_got)
        print(f"{what}: camera worst err / bar {worst:.3f}")
    else:
        assert all(getattr(rs, k).grad is None for k in pm.CAMERA)


# ---- (e) blend_bwd_cull_t_kernel<MODE, AUX, ABS> (and blend_fwd_cull_kernel<MODE, AUX>) ----------------------------------------------------------
@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_transposed_backward_with_aux_and_absgrad(mode, aux, rast, gpu):
    """absgrad_math case a (d with the aux outputs' gradients): the sink against the fp64 reference at tests/test_gpu_absgrad.py's bar,
    grad_tol(ref) without a floor; sink >= |means2D.grad| (1 - 1e-4); without a sink (ABS = 0) the same forward bits and the signed
    gradient at the same bar."""
    import test_gpu_absgrad as tga
    name = "d" if aux else "a"
    with vt.switched(rast, dict(exp_mode=mode)), _launches(rast) as n:
        h = tga._run(rast, gpu, name)
        wo = tga._run(rast, gpu, name, sink=False)
    assert n["blend_fwd"] >= 2 and n["blend_bwd"] == 2 and n["preprocess_bwd"] == 2, n
    r = h["r"]
    assert r["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    assert len(h["out"]) == (5 if aux else 3) and all(torch.equal(a, b) for a, b in zip(h["out"], wo["out"]))
    if aux:      # blend_fwd_cull_kernel<MODE, 1>: the colour is blend_fwd_cull_kernel<MODE, 0>'s, alpha is 1 - final_T of a render on black
        with vt.switched(rast, dict(exp_mode=mode)):
            plain = tga._run(rast, gpu, "a", sink=False)
        assert torch.equal(h["out"][0], plain["out"][0]) and torch.equal(h["out"][2], plain["out"][2])
        alpha = _np(h["out"][4])
        assert alpha.min() >= 0.0 and alpha.max() <= 1.0 and alpha.max() > 0.0 and np.isfinite(_np(h["out"][3])).all()
    got, signed = _np(h["sink"]), _np(h["grads"]["means2D"])[:, :2]
    what = f"blend_bwd_cull_t <{mode}, {int(aux)}, 1>: absgrad case {name}"
    assert not np.isnan(got).any(), "a row of the sink was not written"
    assert not got[h["out"][1].cpu().numpy() == 0].any() and (got >= 0.0).all() and float(r["abs"].max()) > 0.0
    tol = grad_tol(r["abs"])
    print(f"{what}: sink max|err| {np.abs(got - r['abs']).max():.3e} max|ref| {r['abs'].max():.3e} worst err / bar {_worst(got, r['abs'], tol):.3f}")
    assert (np.abs(got - r["abs"]) <= tol).all(), (what, _worst(got, r["abs"], tol))
    assert (got >= np.abs(signed) * (1.0 - 1e-4)).all(), what
    # ABS = 0: every gradient of the backward without a sink against the one with, the same zero rows (tests/test_gpu_absgrad.py:
    # test_nothing_else_moves, here in every mode); the signed screen-space gradient against fp64 is printed (absgrad_math has no fp32 floor for it)
    worst = ("", 0.0)
    for k in h["grads"]:
        a, b = _np(wo["grads"][k]), _np(h["grads"][k])
        assert np.array_equal((a.reshape(a.shape[0], -1) != 0).any(1), (b.reshape(b.shape[0], -1) != 0).any(1)), (what, k)
        worst = max(worst, (k, _worst(a, b, grad_tol(b))), key=lambda x: x[1])
    s_wo = _np(wo["grads"]["means2D"])[:, :2]
    print(f"blend_bwd_cull_t <{mode}, {int(aux)}, 0>: without a sink against with, worst err / bar {worst[1]:.3f} ({worst[0]}); signed means2D.grad against fp64 "
          f"at grad_tol without a floor: {_worst(s_wo, r['signed'], grad_tol(r['signed'])):.3f}")
    assert worst[1] <= 1.0, (what, worst)
