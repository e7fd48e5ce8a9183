"""The comparisons of tests/test_gpu_reference_kernels.py (-m gpu, the reference's kernels run in a child process) and of
tests/test_oracle_ref_kernels.py (CPU, the same kernels' recorded outputs, tests/golden/ref_kernel_vectors.npz) -- a helper, not a test.

`rb` is always one case's output of tests/ref_kernels.py: what the REFERENCE's own forward.cu / backward.cu / rasterizer_impl.cu, compiled
for gfx950 by oracle/ref_build.py, wrote.  The truth is tests/math_renderer.py in fp64 (edge_scenes.reference), the fp32 oracle
(oracle/gsrast_oracle.c) is the side a shared transcription error would show on.

  a. check_truth:          rb against the fp64 truth -- test_gpu_independent._compare's statements, rb standing where the device stands.
  b. check_intermediates:  the fp32 oracle's per-Gaussian arrays against rb's, bits first, then a margin around the fp64 oracle's value.
     check_lists:          num_rendered, sorted keys, point list, tile ranges of rb against another side's literal lists.

The margin of (b), per array: a differing entry must lie within max(4 ulp of the fp64 value's fp32 rounding, REL_BAR x the largest |fp64
value| of the entry's ROW) -- the row, because the entries of one row (a conic, a covariance, a pixel position) come out of the same sums
of products and inherit the rounding of the row's largest term; a near-zero off-diagonal entry has no relative accuracy of its own.
REL_BAR started at 1e-6 (the forward's measured floors, test_gpu_independent.py: worst 7e-7) and is now 4 x the worst relative difference
MEASURED between the two sides on the MI355X over the eight cases (table in test_gpu_reference_kernels.py).  That difference is 0: the
reference binary and the fp32 oracle agree in every bit of every array.  So a differing entry passes only within 4 ulp of the correctly
rounded fp64 value -- on the well-conditioned arrays; an ill-conditioned conic that differs at all is a finding to look at."""
import functools

import numpy as np

import test_gpu_independent as tgi
from conftest import grad_tol
from edge_scenes import CASES, reference
from gpu_harness import bits

CONTRIB = [
    dict(name="g_contrib_cluster", contrib="a", seed=2, W=70, H=45, deg=3),
    dict(name="h_contrib_sparse", contrib="b", seed=4, W=70, H=45, deg=3),
]
ALL_CASES = CASES + CONTRIB
BY_NAME = {c["name"]: c for c in ALL_CASES}
GOLDEN_CASES = ("b_deg1_white_50x37", "d_precomp_colour_cov3D", "e_scale_modifier_0.7")

FLOAT_ARRAYS = ("depths", "means2D", "cov3D", "conic_opacity", "rgb")
REL_BAR = dict(depths=0.0, means2D=0.0, cov3D=0.0, conic_opacity=0.0, rgb=0.0)      # 4 x 0, see above
GRAD_OUT = dict(tgi.ORACLE_KEYS)      # leaf name -> name of the reference's gradient array
# (colour, 1 - final_T) floors of the two contrib_math scenes: max |oracle32 - fp64 truth| over their unambiguous pixels, measured on the
# CPU exactly as test_gpu_independent.py's table was (forward_errors with the fp32 oracle standing where the device stands);
# median depth there 2.33e-07 / 3.66e-07 (max|ref| 15), relative form as in that module
FLOORS = {"g_contrib_cluster": (3.17e-07, 3.13e-07), "h_contrib_sparse": (1.61e-06, 2.35e-06)}
MIN_DEPTH_GAP = 2e-6                  # edge_scenes / _assert_non_vacuous: no two visible Gaussians closer in depth than this


@functools.lru_cache(maxsize=None)
def _truth(name):
    import scenes
    from oracle import oracle as orc
    orc.build()
    orc.set_exp_mode(0)
    c = BY_NAME[name]
    r = reference(scenes, c)
    sc = r["sc"]
    o32, f32 = tgi._oracle32(orc, r)
    o64 = orc.render(sc, r["cam"], r["g"], f64=True, colors_precomp=sc.get("rgb"), cov3D_precomp=sc.get("cov3D"))
    return dict(c=c, r=r, o32=o32, f32=f32, o64=o64)


def truth(name):
    """dict(c, r = edge_scenes.reference, o32 / o64 = the oracle's fp32 / fp64 build on the case, f32 = o32's gradients by leaf name):
    computed once per process and shared -- do not modify it."""
    return _truth(name)


def grads_by_leaf(r, side):
    """The gradient arrays of one side (reference binary, oracle, run_hip: all use the reference's names) as float64, by leaf name."""
    got = {n: np.asarray(side[GRAD_OUT[n]], np.float64).reshape(r["want"][n].shape) for n in r["names"]}
    got["means2D"] = np.asarray(side["dL_dmeans2D"], np.float64)[:, :2]
    return got


def grad_ratios(r, got, floor32):
    """{tensor: worst |got - truth| / grad_tol(truth, floor32)}, the clamped rows of means3D as a tensor of their own."""
    out = {}
    for n in r["names"] + ["means2D"]:
        out[n] = float((np.abs(got[n] - r["want"][n]) / np.maximum(grad_tol(r["want"][n], floor32[n]), 1e-300)).max(initial=0.0))
    cl = r["clamped"]
    w = r["want"]["means3D"][cl]
    out["means3D[clamped]"] = float((np.abs(got["means3D"][cl] - w) / np.maximum(grad_tol(w, floor32["means3D"][cl]), 1e-300)).max(initial=0.0))
    return out


def forward_errors(r, colour, alpha, depth):
    """max |side - truth| over the unambiguous pixels: (colour, 1 - final_T, median depth)."""
    out, keep = r["out"], r["keep"]
    return (float(np.abs(colour[:, keep] - out["color"].detach().numpy()[:, keep]).max()),
            float(np.abs(alpha[keep] - (1.0 - out["final_T"].detach().numpy()[keep])).max()),
            float(np.abs(depth[keep] - out["depth"].numpy()[keep]).max()))


def check_truth(name, rb, label="reference binary"):
    """(a).  Returns (forward errors, gradient ratios) after asserting them."""
    t = truth(name)
    c, r = t["c"], t["r"]
    colour = np.asarray(rb["out_color"], np.float64)
    depth = np.asarray(rb["out_depth"], np.float64).reshape(c["H"], c["W"])
    alpha = 1.0 - np.asarray(rb["accum_alpha"], np.float64)
    got = grads_by_leaf(r, rb)
    fwd = forward_errors(r, colour, alpha, depth)
    ratios = grad_ratios(r, got, t["f32"])
    print(f"{name}: {label} vs fp64 truth: colour {fwd[0]:.3e}  alpha {fwd[1]:.3e}  depth {fwd[2]:.3e}   "
          f"gradients, worst err / grad_tol(truth, oracle32): " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)
    _compare(c, r, got, t["f32"], np.asarray(rb["radii"]), colour, depth, alpha)
    return fwd, ratios


def _compare(c, r, got, f32, radii, colour, depth, alpha):
    """test_gpu_independent._compare, statement by statement; the one difference is where the colour / alpha floors come from: that
    module's constants are the maximum over ITS six cases, the two contrib_math scenes bring their own (FLOORS)."""
    colour_floor, alpha_floor = FLOORS.get(c["name"], (tgi.COLOUR_FLOOR, tgi.ALPHA_FLOOR))
    out, keep, want = r["out"], r["keep"], r["want"]
    d = out["proj"]["disc"]
    assert np.array_equal(radii > 0, d["vis"]), "radius decision differs: pick another seed"
    firm = (d["radius_margin"] > 1e-4) & (d["rect_margin"] > 1e-5)
    assert firm.mean() > 0.98
    np.testing.assert_array_equal(radii[firm], d["radius"][firm])
    ref = out["color"].detach().numpy()
    np.testing.assert_allclose(colour[:, keep], ref[:, keep], rtol=0, atol=tgi._bar(colour_floor, ref))
    np.testing.assert_allclose(alpha[keep], 1.0 - out["final_T"].detach().numpy()[keep], rtol=0, atol=tgi._bar(alpha_floor, 1.0))
    dref = out["depth"].numpy()
    np.testing.assert_allclose(depth[keep], dref[keep], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(dref).max())))
    for n in r["names"] + ["means2D"]:
        err = np.abs(got[n] - want[n])
        assert (err <= grad_tol(want[n], f32[n])).all(), (n, float(err.max()), float(np.abs(want[n]).max()))
    cl = r["clamped"]
    err = np.abs(got["means3D"][cl] - want["means3D"][cl])
    assert (err <= grad_tol(want["means3D"][cl], f32["means3D"][cl])).all(), ("means3D, clamped rows", float(err.max()), float(np.abs(want["means3D"][cl]).max()))


def _row_scale(v64):
    v = np.abs(v64)
    return v if v.ndim == 1 else np.broadcast_to(v.max(axis=1, keepdims=True), v.shape)


def check_intermediates(name, rb, oracle32=None):
    """(b), the per-Gaussian arrays.  oracle32: the fp32 oracle's forward state (default: the shared one).  Returns {array: (number of
    entries whose bits differ, worst relative difference of rb from the fp64 oracle, worst of the fp32 oracle)}."""
    t = truth(name)
    c, r, o64 = t["c"], t["r"], t["o64"]
    o32 = t["o32"] if oracle32 is None else oracle32
    out = r["out"]
    d = out["proj"]["disc"]
    vis = d["vis"]
    assert np.array_equal(np.asarray(rb["radii"]) > 0, vis) and np.array_equal(o32["radii"] > 0, vis)
    pre = bool(c.get("precomp"))
    table = {}
    for k in FLOAT_ARRAYS:
        if pre and k in ("cov3D", "rgb"):      # given as inputs: the forward neither computes nor stores them
            continue
        a, b, v = np.asarray(rb[k], np.float32)[vis], np.asarray(o32[k], np.float32)[vis], np.asarray(o64[k], np.float64)[vis]
        if k == "conic_opacity":                # the opacity is a copy of the input: bits, always
            np.testing.assert_array_equal(bits(a[:, 3]), bits(b[:, 3]))
            a, b, v = a[:, :3], b[:, :3], v[:, :3]
        differ = bits(a) != bits(b)
        scale = _row_scale(v)
        rel_a = np.abs(a.astype(np.float64) - v) / np.maximum(scale, 1e-300)
        rel_b = np.abs(b.astype(np.float64) - v) / np.maximum(scale, 1e-300)
        table[k] = (int(differ.sum()), float(rel_a.max(initial=0.0)), float(rel_b.max(initial=0.0)))
        print(f"{name}: {k}: {int(differ.sum())} of {differ.size} entries differ in bits (reference binary vs fp32 oracle); worst |x - fp64| / row scale: "
              f"reference binary {table[k][1]:.3e}, oracle {table[k][2]:.3e}, where the bits differ: reference binary "
              f"{float(rel_a[differ].max(initial=0.0)):.3e}, oracle {float(rel_b[differ].max(initial=0.0)):.3e}", flush=True)
        bar = np.maximum(4.0 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64), REL_BAR[k] * scale)
        for side, x in (("reference binary", a), ("fp32 oracle", b)):
            err = np.abs(x.astype(np.float64) - v)
            bad = differ & (err > bar)
            assert not bad.any(), (f"{k}: {int(bad.sum())} entries of the {side} differ from the other side AND lie outside the margin around the fp64 value; "
                                   f"worst err / bar {float((err / bar)[differ].max()):.2f}")
    firm = vis & (d["radius_margin"] > 1e-4) & (d["rect_margin"] > 1e-5)
    assert firm.sum() >= 0.98 * vis.sum()
    diff_tt = np.asarray(rb["tiles_touched"]).astype(np.int64) != np.asarray(o32["tiles_touched"]).astype(np.int64)
    print(f"{name}: tiles_touched: {int(diff_tt.sum())} differ ({int((diff_tt & firm).sum())} on firm Gaussians)", flush=True)
    assert not (diff_tt & firm).any()
    np.testing.assert_array_equal(np.asarray(rb["tiles_touched"])[firm], d["tiles"][firm])
    table["tiles_touched"] = (int(diff_tt.sum()), 0.0, 0.0)
    if not pre:
        firm_c = firm & (out["colour_clamp_margin"] > 1e-5)
        diff_c = (np.asarray(rb["clamped"]) != 0) != (np.asarray(o32["clamped"]) != 0)
        print(f"{name}: clamped: {int(diff_c.sum())} differ ({int(diff_c[firm_c].sum())} on firm Gaussians)", flush=True)
        assert not diff_c[firm_c].any()
        table["clamped"] = (int(diff_c.sum()), 0.0, 0.0)
    return table


def _lists_of(side):
    R = int(np.asarray(side["num_rendered"]).reshape(-1)[0]) if "num_rendered" in side else int(side["R"])
    return (R, np.asarray(side["keys_sorted"]).view(np.uint64).reshape(-1), np.asarray(side["point_list"]).view(np.uint32).reshape(-1),
            np.asarray(side["ranges"]).view(np.uint32).reshape(-1, 2))


def check_lists(name, rb, other, label):
    """(b), the lists: rb's num_rendered, sorted keys, point list and tile ranges against another side's LITERAL lists (the fp32 oracle's,
    or run_hip(..., tile_clip=0)'s).  Entry by entry where the two sides' depth bits are equal; otherwise the tile ids and every tile's id
    set entry by entry, and the order only between neighbours whose fp64 depths differ by more than MIN_DEPTH_GAP."""
    t = truth(name)
    vis = t["r"]["out"]["proj"]["disc"]["vis"]
    Ra, ka, pa, ra = _lists_of(rb)
    Rb, kb, pb, rg = _lists_of(other)
    same_depth_bits = np.array_equal(bits(np.asarray(rb["depths"], np.float32)[vis]), bits(np.asarray(other["depths"], np.float32)[vis]))
    print(f"{name}: lists, reference binary vs {label}: num_rendered {Ra} / {Rb}, depth bits {'equal' if same_depth_bits else 'DIFFER'}", flush=True)
    assert Ra == Rb and Ra > 0
    np.testing.assert_array_equal(ra, rg)
    assert len(ka) == Ra and len(pa) == Ra
    np.testing.assert_array_equal(ka >> np.uint64(32), kb >> np.uint64(32))
    if same_depth_bits:
        np.testing.assert_array_equal(ka, kb)
        np.testing.assert_array_equal(pa, pb)
        return
    z = np.asarray(t["o64"]["depths"], np.float64)
    for lo, hi in ra.astype(np.int64):
        la, lb = pa[lo:hi], pb[lo:hi]
        np.testing.assert_array_equal(np.sort(la), np.sort(lb))
        pos = np.empty(int(max(la.max(initial=0), 0)) + 1, np.int64)
        pos[lb] = np.arange(len(lb))
        apart = np.abs(z[la[1:]] - z[la[:-1]]) > MIN_DEPTH_GAP
        assert (pos[la[1:]][apart] > pos[la[:-1]][apart]).all(), "two Gaussians further apart in depth than fp32 resolves are ordered differently"
