"""No GPU: the facts tests/test_gpu_sparse_states.py relies on, and the helpers both files share.

That file runs every gradient source of the backward (colour, aux, features, distortion, camera) over gradient records of which only the
consumed Gaussians' were zeroed (grec_zero_touched_kernel; every other record keeps the 0xFF bytes the poisoned state buffer was handed out
with), and asserts that the rows of the Gaussians that contribute to nothing come out as exact zeros.  It bites only if the cases HAVE such
rows, and enough of them; which rows they are is decided here, in fp64, by nothing the device computes:

    nothing(case, antialiasing) = visible (radius > 0), and no pair of the Gaussian is blended at a pixel that is not fp32-ambiguous
                                  (math_renderer.render's `live` table and `ambiguous` mask, through contrib_math.reference)

Measured on the CPU: case a 12 (plain) / 32 (antialiasing) of 672 visible Gaussians, 28 culled; case b 57 / 58 of 274 visible, 1726 culled;
0.06 % - 0.67 % of the pixels ambiguous.  posegrad_math's cases a (dense, 64 x 48) and b (raw, 50 x 37), which the camera source runs on:
counted the same way from posegrad_math.render's own tables, printed and asserted to be at least ten as well.

`reference_zero_rows` reads the same off a source's fp64 GRADIENTS (a row that is exactly zero in every tensor of the reference); it is
asserted here to contain the pair table's rows for every source, and to equal them for every source but the distortion-only loss of case
b (one Gaussian that is alone at each of its pixels).  The GPU file asserts exact zeros on the pair table's rows."""
import re

import numpy as np
import pytest

import contrib_math as cm
import distort_math as dm
import features_math as fm
import posegrad_math as pm
import variant_table as vt

NOTHING = {("a", False): 12, ("a", True): 32, ("b", False): 57, ("b", True): 58}      # visible, contributes to no unambiguous pixel
CULLED = dict(a=28, b=1726)
POSE_LETTERS = dict(dense="a", raw="b")                                                # posegrad_math's cases of the camera source
# process-wide switches the GPU file sets through rast._C.set_option beside variant_table.switched's (variant_table.DEFAULTS does not list them)
SWITCH_DEFAULTS = dict(sparse_grec=1, touch_bits=1, list_cut_always=0, no_list_cut=0)
LAUNCH_NAMES = ("late_rows_zero", "grec_zero_touched", "features_bwd", "distort_bwd", "features_fwd", "distort_fwd", "blend_bwd", "preprocess_bwd")


def rows_of_case(name, aa=False):
    """dict(vis, culled, contributing, nothing: bool [P]; amb [H,W]) of contrib_math.CASES[name] from the fp64 render's pair table."""
    r = cm.reference(name, aa)
    out = r["out"]
    vis = np.asarray(out["proj"]["disc"]["vis"], bool)
    live = np.asarray(out["live"], bool)                       # [N, K]: pixel x visible Gaussian in depth order
    amb = np.asarray(out["ambiguous"], bool)
    used = (live & ~amb.reshape(-1)[:, None]).any(axis=0)
    contributing = np.zeros(vis.shape[0], bool)
    contributing[np.asarray(out["order"])[used]] = True
    assert not (contributing & ~vis).any()
    return dict(vis=vis, culled=~vis, contributing=contributing, nothing=vis & ~contributing, amb=amb)


def rows_of_pose_case(letter):
    """The same of posegrad_math.reference(letter), from posegrad_math.render's decisions."""
    r64 = pm.reference(letter)["r64"]
    out = r64["out"]
    D = out["decisions"]
    vis = np.asarray(out["vis"], bool)
    live = np.asarray(out["live"], bool)
    amb = np.asarray(r64["amb"], bool)
    used = (live & ~amb.reshape(-1)[:, None]).any(axis=0)
    contributing = np.zeros(vis.shape[0], bool)
    contributing[np.asarray(D["idx"])[used]] = True
    assert not (contributing & ~vis).any()
    return dict(vis=vis, culled=~vis, contributing=contributing, nothing=vis & ~contributing, amb=amb)


def reference_zero_rows(grads):
    """bool [P]: the rows that are exactly zero in every tensor of an fp64 reference's gradients (each [P, ...])."""
    zero = None
    for g in grads.values():
        g = np.asarray(g)
        z = ~(g.reshape(g.shape[0], -1) != 0).any(axis=1)
        zero = z if zero is None else zero & z
    return zero


def aux_only(name):
    """The fp64 / fp32 references of sum acc_depth gD + sum alpha gA on a case: distort_math's return_aux evaluation without the colour
    and with a zero upstream gradient of the map.  dict(sc, cam, g, r64, r32)."""
    if name not in _aux_only:
        r = dm.reference(name, "return_aux")
        g = dict(r["r64"]["g"], gd=np.zeros_like(r["r64"]["g"]["gd"]))
        r64 = dm.evaluate64(r["sc"], r["cam"], aux=True, colour_loss=False, g=g)
        r32 = dm.restate32(r["sc"], r["cam"], g, aux=True, colour_loss=False)
        _aux_only[name] = dict(sc=r["sc"], cam=r["cam"], g=g, r64=r64, r32=r32)
    return _aux_only[name]


def everything(name):
    """The all-at-once source (features C = 19, distortion, aux, antialiasing, raw family): its two parts, features_math's feature + colour
    loss and distort_math's distortion + aux loss without the colour, each fp64 / fp32.  dict(rf, g, d64, d32)."""
    if name not in _everything:
        rf = fm.reference(name, 19, aa=True, raw=True)
        d64 = dm.evaluate64(rf["sc"], rf["cam"], aa=True, raw=True, aux=True, colour_loss=False)
        d32 = dm.restate32(rf["sc"], rf["cam"], d64["g"], aa=True, raw=True, aux=True, colour_loss=False)
        _everything[name] = dict(rf=rf, g=d64["g"], d64=d64, d32=d32)
    return _everything[name]


def retained(name="a"):
    """Section 4's source (features C = 19 + distortion + aux + colour, plain, dense family): features_math's feature + colour loss and
    distort_math's distortion + aux loss without the colour."""
    if name not in _retained:
        rf = fm.reference(name, 19)
        d64 = dm.evaluate64(rf["sc"], rf["cam"], aux=True, colour_loss=False)
        d32 = dm.restate32(rf["sc"], rf["cam"], d64["g"], aux=True, colour_loss=False)
        _retained[name] = dict(rf=rf, g=d64["g"], d64=d64, d32=d32)
    return _retained[name]


def summed(a, b):
    """{name: a[name] + b[name]} over a's names (b's where it has them): the gradients of the sum of two losses."""
    return {n: np.asarray(a[n]) + (np.asarray(b[n]).reshape(np.asarray(a[n]).shape) if n in b else 0.0) for n in a}


_aux_only, _everything, _retained = {}, {}, {}


# ---- the conditions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_cases_have_rows_that_keep_stale_records(name, aa):
    rows = rows_of_case(name, aa)
    n = int(rows["nothing"].sum())
    print(f"case {name}{' antialias' if aa else ''}: {int(rows['vis'].sum())} visible, {int(rows['culled'].sum())} culled, {n} visible that contribute to nothing, "
          f"{100.0 * rows['amb'].mean():.2f} % of the pixels ambiguous")
    assert n >= 10 and n == NOTHING[name, aa]
    assert int(rows["culled"].sum()) == CULLED[name]
    assert rows["amb"].mean() < 0.05 and rows["amb"].mean() <= 0.007
    # contrib_math's own table (pixel_weights = ~ambiguous, its mask a superset of the render's) counts the same rows
    r = cm.reference(name, aa)
    assert np.array_equal(rows["vis"] & (r["table"][:, 2] == 0), rows["nothing"])


@pytest.mark.parametrize("kind", list(POSE_LETTERS))
def test_pose_cases_have_them_too(kind):
    rows = rows_of_pose_case(POSE_LETTERS[kind])
    r = pm.reference(POSE_LETTERS[kind])
    print(f"posegrad case {POSE_LETTERS[kind]} ({kind}): {int(rows['vis'].sum())} visible, {int(rows['culled'].sum())} culled, {int(rows['nothing'].sum())} visible that "
          f"contribute to nothing, {100.0 * rows['amb'].mean():.2f} % of the pixels ambiguous")
    assert int(rows["nothing"].sum()) >= 10 and int(rows["culled"].sum()) >= 1 and rows["amb"].mean() < 0.05
    assert bool(r.get("raw")) == (kind == "raw")
    want = {n: r["r64"]["want"][n] for n in r["names"]}
    assert np.array_equal(reference_zero_rows(want), rows["culled"] | rows["nothing"])


def _zero_on(amb, *arrays):
    return all(not np.asarray(a)[..., amb].any() for a in arrays if a is not None)


@pytest.mark.parametrize("name", list(cm.CASES))
def test_upstream_gradients_are_zero_on_the_ambiguous_pixels(name):
    for C in (5, 40):
        r = fm.reference(name, C, colour_loss=False)["r64"]
        assert _zero_on(r["amb"], r["g1"], r["g0"]) and np.abs(r["g1"]).max() > 0
    for variant, colour in (("plain", False), ("return_aux", True)):
        r = dm.reference(name, variant, colour_loss=colour)["r64"]
        assert _zero_on(r["amb"], *r["g"].values()) and all(np.abs(v).max() > 0 for v in r["g"].values())
    a = aux_only(name)
    assert _zero_on(a["r64"]["amb"], *a["g"].values()) and not a["g"]["gd"].any()
    e = everything(name)
    assert np.array_equal(e["rf"]["r64"]["amb"], e["d64"]["amb"]), "the two parts of the all-at-once source mask different pixels"
    assert _zero_on(e["d64"]["amb"], e["rf"]["r64"]["g1"], e["rf"]["r64"]["g0"], *e["g"].values())
    assert e["d64"]["amb"].mean() < 0.05


def test_upstream_gradients_of_the_other_sources():
    for letter in POSE_LETTERS.values():
        r64 = pm.reference(letter)["r64"]
        assert _zero_on(r64["amb"], r64["g"], r64["gD"], r64["gA"]) and r64["amb"].mean() < 0.05
    t = retained("a")
    assert np.array_equal(t["rf"]["r64"]["amb"], t["d64"]["amb"])
    assert _zero_on(t["d64"]["amb"], t["rf"]["r64"]["g1"], t["rf"]["r64"]["g0"], *t["g"].values())


@pytest.mark.parametrize("name", list(cm.CASES))
def test_rows_that_contribute_to_nothing_are_zero_rows_of_every_fp64_gradient(name):
    """The pair table's rows against the references' own gradients (the raw family's and the anti-aliased ones included, whose references
    render for themselves): a Gaussian that contributes to nothing has an fp64 gradient of exactly zero in every tensor of every source.
    The converse holds for every source but one -- a Gaussian that is the ONLY contributor of each of its pixels has no distortion
    gradient (case b: one such row) --, which is why the GPU file takes its zero rows from the pair table and not from the gradients."""
    for aa, refs in ((False, dict(features5=fm.reference(name, 5, colour_loss=False)["r64"]["grads"], features40=fm.reference(name, 40, colour_loss=False)["r64"]["grads"],
                                  distortion=dm.reference(name, "plain", colour_loss=False)["r64"]["grads"], distortion_aux=dm.reference(name, "return_aux")["r64"]["grads"],
                                  aux=aux_only(name)["r64"]["grads"])),
                     (True, dict(everything=summed(everything(name)["rf"]["r64"]["grads"], everything(name)["d64"]["grads"])))):
        rows = rows_of_case(name, aa)
        for src, grads in refs.items():
            zero, want = reference_zero_rows(grads), rows["culled"] | rows["nothing"]
            assert not (want & ~zero).any(), (name, src, int((want & ~zero).sum()), "rows that contribute to nothing have an fp64 gradient")
            extra = int((zero & ~want).sum())
            print(f"case {name}, {src}: {int(want.sum())} rows contribute to nothing (culled included), {extra} more have a zero fp64 gradient")
            assert extra == (1 if (name, src) == ("b", "distortion") else 0), (name, src, extra)
            assert np.isfinite(np.concatenate([np.asarray(g).reshape(-1) for g in grads.values()])).all()


# ---- the switches and the launch names ----------------------------------------------------------------------------------------------------
def test_switches_and_launch_names_exist():
    """variant_table.switched sets the three backward forms and the exp mode; the other four switches are process-wide words of the library's
    option table with the defaults restored by the GPU file; the launch counts it reads are rows of the profile table."""
    import os
    from conftest import PKG
    assert {"late_fill_min_p", "dense_backward", "exp_mode"} <= set(vt.DEFAULTS)
    assert vt.DEFAULTS["late_fill_min_p"] == 750000 and vt.DEFAULTS["dense_backward"] == 0
    text = open(os.path.join(PKG, "csrc", "gsrast_capi.hip")).read()
    for name, default in SWITCH_DEFAULTS.items():
        if name == "no_list_cut":      # a per-call option (include/gsrast.h: gsrast_options), not a word of the table
            continue
        m = re.search(r'\{\s*"%s",\s*&g_opt\.%s,\s*(-?\d+),' % (name, name), text)
        assert m is not None and int(m.group(1)) == default, name
    import diff_gaussian_rasterization_ch3 as rast
    assert "no_list_cut" in rast._C.PER_CALL_OPTIONS and rast._C._OPTION_DEFAULTS["no_list_cut"] == 0 and "dense_backward" in rast._C.PER_CALL_OPTIONS
    for name in LAUNCH_NAMES:
        assert re.search(r'"%s"' % name, text), name
