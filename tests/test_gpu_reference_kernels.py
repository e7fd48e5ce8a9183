"""-m gpu: the REFERENCE's own kernels -- cuda_rasterizer/forward.cu, backward.cu, rasterizer_impl.cu, compiled for gfx950 by
oracle/ref_build.py into oracle/_ref/libref_rasterizer.so -- beside the fp64 math renderer, the fp32 oracle and the HIP renderer, on the
project's eight smallest hard scenes (the six edge cases of test_gpu_independent.py and contrib_math's two).  The library is run ONCE, in
a child process of its own (tests/ref_kernels.py), so a fault in foreign code cannot take this process's GPU context with it; if the
library is not there (no reference tree where build() ran) the module skips.

  a. reference binary vs fp64 truth (tests/math_renderer.py): the statements of test_gpu_independent._compare, the binary standing where
     the device stands -- pins that the reference computes this mathematics.  Gradient bar grad_tol(truth, oracle32): if the reference
     needed more than 8 x the fp32 oracle's own error, the oracle would not be the fp32 floor conftest.grad_tol says it is.
  b. fp32 oracle vs reference binary, intermediates and lists (ref_compare.check_intermediates / check_lists): where a transcription
     error shared by oracle/gsrast_oracle.c and csrc/gsrast_preprocess.h would show.  The lists also against run_hip(tile_clip=0)'s.
  c. HIP vs reference binary, exp modes 0 and 1 of the product:
        forward    |hip - truth| <= max(4 x max|refbin - truth| over the case's unambiguous pixels, 2e-6 * max(1, max|ref|))
                   with the floor taken from the child's output at test time; (a) must pass first and the floor may not exceed 2 x the
                   value recorded below, so a broken reference run cannot inflate the bar
        gradients  |hip - truth| <= grad_tol(truth, refbin): the reference's binary stands where the fp32 oracle stands elsewhere
        n_contrib equal on the unambiguous pixels, markVisible equal on every Gaussian.

Measured on the MI355X (the first run of this module; -s prints every figure again).  max |reference binary - fp64 truth| over the
unambiguous pixels -- RECORDED below -- and, per intermediate array, the number of entries on visible Gaussians whose BITS differ between
the reference binary and the fp32 oracle:

    case   colour      1 - final_T   median depth   depths means2D cov3D conic rgb clamped tiles_touched | keys, point_list, ranges
    a      7.164e-07   1.695e-07     1.945e-07      0      0       0     0     0   0       0             | equal entry by entry
    b      6.113e-07   6.043e-08     1.943e-07      0      0       0     0     0   0       0             | equal entry by entry
    c      1.600e-06   2.856e-07     3.445e-07      0      0       0     0     0   0       0             | equal entry by entry
    d      5.252e-07   1.823e-07     2.321e-07      0      0       -     0     -   -       0             | equal entry by entry
    e      1.592e-06   5.753e-07     2.638e-07      0      0       0     0     0   0       0             | equal entry by entry
    f      1.691e-06   2.282e-08     1.978e-07      0      0       0     0     0   0       0             | equal entry by entry
    g      3.770e-07   3.133e-07     2.331e-07      0      0       0     0     0   0       0             | equal entry by entry
    h      1.610e-06   2.350e-06     3.659e-07      0      0       0     0     0   0       0             | equal entry by entry

(d: colours and covariances are inputs there.)  The reference's preprocess, compiled without contraction, and the fp32 oracle agree in
every bit of every per-Gaussian array on all eight scenes, so the lists -- the oracle's and run_hip(tile_clip=0)'s -- are the reference's
entry by entry, and the worst relative difference between the two sides is 0: ref_compare.REL_BAR, 4 x that, leaves a differing entry
only the 4 ulp around the correctly rounded fp64 value.  The forward columns differ from test_gpu_independent.py's oracle table only
through exp (the device's against the oracle's fixed sequence) and are of the same size.

Gradients, worst over the eight cases: |refbin - truth| / grad_tol(truth, oracle32) is 0.12 means3D, 0.10 opacities, 0.13 shs, 0.14 scales,
0.09 rotations, 0.12 means2D, 0.02 rgb, 0.06 cov3D, 0.09 clamped rows of means3D (dL_dconic 0.05, dL_dcov3D 0.13 against the fp64 oracle);
|hip - truth| / grad_tol(truth, refbin) is 0.13 means3D, 0.08 opacities, 0.14 shs, 0.15 scales, 0.22 rotations, 0.14 means2D, 0.02 rgb, 0.08
cov3D, 0.13 clamped rows -- the same in both exp modes.  The reference needs nowhere near 8 x the fp32 oracle's error: the oracle IS its
fp32 floor.  Exp modes: max |hip - refbin| of the colour is 1.2e-07 ... 2.7e-07 in both modes (mode 1 closer on a, mode 0 on f, equal on
the other six): neither mode sits measurably closer to the reference's hardware exp at these sizes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_compare as rc
import ref_kernels
from conftest import grad_tol, settings_from
from gpu_harness import bits, run_hip

pytestmark = pytest.mark.gpu

# case: (colour, 1 - final_T, median depth), the table above
RECORDED = {
    "a_deg3_long_lists": (7.164e-07, 1.695e-07, 1.945e-07),
    "b_deg1_white_50x37": (6.113e-07, 6.043e-08, 1.943e-07),
    "c_deg2_colour_clamp": (1.600e-06, 2.856e-07, 3.445e-07),
    "d_precomp_colour_cov3D": (5.252e-07, 1.823e-07, 2.321e-07),
    "e_scale_modifier_0.7": (1.592e-06, 5.753e-07, 2.638e-07),
    "f_saturated_early_stop": (1.691e-06, 2.282e-08, 1.978e-07),
    "g_contrib_cluster": (3.770e-07, 3.133e-07, 2.331e-07),
    "h_contrib_sparse": (1.610e-06, 2.350e-06, 3.659e-07),
}
NAMES = [c["name"] for c in rc.ALL_CASES]
_closeness = {}      # (case, exp mode) -> (max |hip - reference binary| of the colour, number of colour entries whose bits differ)


@pytest.fixture(scope="session")
def refbin(gpu, tmp_path_factory):
    """{case: every array the reference binary wrote}: one child process for all cases; no retry."""
    if not os.path.exists(ref_kernels.LIB_PATH):
        pytest.skip("oracle/_ref/libref_rasterizer.so is not there: build() found no reference tree to compile it from")
    d = tmp_path_factory.mktemp("refbin")
    inputs = {"names": np.array(NAMES)}
    for n in NAMES:
        t = rc.truth(n)
        inputs.update(ref_kernels.pack_case(n, t["r"]["sc"], t["r"]["cam"], t["c"]["deg"], t["r"]["g"]))
    np.savez(d / "in.npz", **inputs)
    try:
        p = subprocess.run([sys.executable, ref_kernels.__file__, str(d / "in.npz"), str(d / "out.npz")], capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the reference binary's child process did not finish in 180 s: {e.stderr}")
    if p.returncode != 0:
        pytest.fail(f"the reference binary's child process exited with {p.returncode}:\n{p.stdout}\n{p.stderr}")
    print(p.stdout)
    return ref_kernels.unpack(np.load(d / "out.npz"), NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_a_reference_binary_against_the_fp64_math_renderer(name, refbin):
    rb, t = refbin[name], rc.truth(name)
    rc.check_truth(name, rb)
    # the two gradients that are no leaf: against the fp64 build of the oracle, same bar
    for k in ("dL_dconic", "dL_dcov3D"):
        want = np.asarray(t["o64"][k], np.float64)
        err = np.abs(np.asarray(rb[k], np.float64).reshape(want.shape) - want)
        tol = grad_tol(want, t["o32"][k])
        print(f"{name}: {k} vs the fp64 oracle: worst err / bar {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
        assert (err <= tol).all(), (k, float(err.max()))


@pytest.mark.parametrize("name", NAMES)
def test_b_oracle_intermediates_against_the_reference_binary(name, refbin):
    rc.check_intermediates(name, refbin[name])
    rc.check_lists(name, refbin[name], rc.truth(name)["o32"], "fp32 oracle")


@pytest.mark.parametrize("name", NAMES)
def test_b_hip_lists_against_the_reference_binary(name, refbin, rast, gpu):
    r = rc.truth(name)["r"]
    sc = r["sc"]
    h = run_hip(rast, sc, r["cam"], gpu, colors_precomp=sc.get("rgb"), cov3D_precomp=sc.get("cov3D"), exp_mode=0, tile_clip=0)
    rc.check_lists(name, refbin[name], h, "run_hip(tile_clip=0)")


@pytest.mark.parametrize("exp_mode", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_c_hip_against_the_reference_binary(name, exp_mode, refbin, rast, gpu):
    rb, t = refbin[name], rc.truth(name)
    c, r = t["c"], t["r"]
    sc, cam, out, keep = r["sc"], r["cam"], r["out"], r["keep"]
    floors, _ = rc.check_truth(name, rb)                                   # (a) first
    for q, f, rec in zip(("colour", "alpha", "depth"), floors, RECORDED[name]):
        assert f <= 2.0 * rec, f"{q}: the reference binary is {f:.3e} from the truth, recorded {rec:.3e}: its run is not the one the bars were sized on"
    try:
        h = run_hip(rast, sc, cam, gpu, dL_dcolor=r["g"], colors_precomp=sc.get("rgb"), cov3D_precomp=sc.get("cov3D"), exp_mode=exp_mode, tile_clip=0)
    finally:
        rast._C.set_option("exp_mode", 0)
    H, W = c["H"], c["W"]
    colour, depth = h["out_color"].astype(np.float64), h["out_depth"].astype(np.float64).reshape(H, W)
    alpha = 1.0 - h["final_T"].astype(np.float64)
    refs = (out["color"].detach().numpy(), 1.0 - out["final_T"].detach().numpy(), out["depth"].numpy())
    errs = rc.forward_errors(r, colour, alpha, depth)
    bars = [max(4.0 * f, 2e-6 * max(1.0, float(np.abs(ref).max()))) for f, ref in zip(floors, refs)]
    ref_colour = np.asarray(rb["out_color"], np.float32)
    _closeness[(name, exp_mode)] = (float(np.abs(h["out_color"].astype(np.float64) - ref_colour.astype(np.float64))[:, keep].max()),
                                    int((bits(h["out_color"]) != bits(ref_colour))[:, keep].sum()))
    got = rc.grads_by_leaf(r, h)
    ratios = rc.grad_ratios(r, got, rc.grads_by_leaf(r, rb))
    print(f"{name} exp_mode {exp_mode}: hip vs fp64 truth, err / bar: " + "  ".join(f"{q} {e:.3e} / {b:.3e}" for q, e, b in zip(("colour", "alpha", "depth"), errs, bars))
          + "   gradients, worst err / grad_tol(truth, refbin): " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + "   max |hip - refbin| colour %.3e, %d entries differ in bits" % _closeness[(name, exp_mode)], flush=True)
    if (name, 0) in _closeness and (name, 1) in _closeness:
        a, b = _closeness[(name, 0)], _closeness[(name, 1)]
        print(f"{name}: closer to the reference binary: exp_mode {0 if a < b else 1 if b < a else '0 = 1'} ((max, entries) {a} vs {b})", flush=True)
    for q, e, b in zip(("colour", "alpha", "depth"), errs, bars):
        assert e <= b, (q, e, b)
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    np.testing.assert_array_equal(h["n_contrib"].reshape(H, W)[keep], np.asarray(rb["n_contrib"]).reshape(H, W)[keep])
    rs = settings_from(rast, cam, sc, gpu)
    present = rast.GaussianRasterizer(rs).markVisible(torch.as_tensor(sc["means3D"], device=gpu)).cpu().numpy()
    np.testing.assert_array_equal(present.astype(bool), np.asarray(rb["present"]) != 0)
