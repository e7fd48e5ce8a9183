"""-m gpu: randomised parity sweep.  Sixty seeded configurations drawn over everything the API accepts -- Gaussian count,
image size (multiples of 16 or not, tiny, tall, wide), SH degree and row count, SH vs precomputed colours, scale / rotation vs
precomputed covariance, background, scale_modifier, camera, opacity range, anisotropy -- each checked like the hand-written
cases: forward bit-exact against the oracle (literal and clipped lists), gradients within the bar of the fp64 truth."""
import numpy as np
import pytest

from gpu_harness import bits, run_hip
from test_gpu_parity import _check_forward_exact, _check_grads

pytestmark = pytest.mark.gpu


def _config(seed, large=False):
    rng = np.random.default_rng(1000 + seed)
    P = int(rng.choice([33000, 40001, 65536, 90000])) if large else int(rng.choice([1, 2, 5, 17, 64, 300, 1000, 3000]))
    W = int(rng.choice([16, 17, 31, 48, 64, 97, 160, 203, 320]))
    H = int(rng.choice([5, 16, 33, 48, 83, 112, 240]))
    deg = int(rng.integers(0, 4))
    return dict(P=P, W=W, H=H, deg=deg, use_rgb=bool(rng.random() < 0.25), use_cov=bool(rng.random() < 0.25),
                scale_mul=float(rng.choice([0.3, 1.0, 2.5, 8.0])), aniso=float(rng.choice([1.0, 1.0, 10.0, 40.0])),
                opac_mul=float(rng.choice([1.0, 1.0, 0.3, 0.02])), scale_modifier=float(rng.choice([1.0, 1.0, 0.5, 1.7])),
                bg=rng.uniform(0, 1, 3).astype(np.float32) if rng.random() < 0.5 else np.zeros(3, np.float32),
                cam=(int(rng.integers(0, 7)), 7), big_grad=bool(rng.random() < 0.5), rng=rng)


@pytest.mark.parametrize("seed", range(100, 112))
def test_random_configuration_at_bucket_sort_sizes(seed, orc, scenes, rast, gpu, scatter_form):
    """The same sweep at Gaussian counts that take the bucket depth sort (P >= 32768) -- the context carries its capacity hints from
    one random configuration to the next, so undersized speculative launches and their repeats are part of it.

    The compared render (gpu_harness.run_hip's module call) runs the product plan, debug_state = 0: the repeated clip = 1 pass comes back to a
    pose whose cut depths the pass before left, so it runs `cut_colors` -- the compacting colour kernel on the early Gaussians only, with
    colors_precomp, cov3D_precomp, SH degrees 0-2 and odd image sizes as the seed draws them."""
    # ... and so are the list cut's depths (include/gsrast.h: options.no_list_cut), forced on here: the seven camera poses come back with
    # another scene each time, so cut lists that hold, cut lists that are too short (the forward falls back inside the call) and stale
    # entries of another image size all occur; every render after a pose's first one is checked exactly like the first
    rast._C.set_option("list_cut_always", 1)
    try:
        _run_configuration(seed, _config(seed, large=True), orc, scenes, rast, gpu, clips=(0, 1, 1))
    finally:
        rast._C.set_option("list_cut_always", 0)


@pytest.mark.parametrize("seed", range(60))
def test_random_configuration(seed, orc, scenes, rast, gpu):
    _run_configuration(seed, _config(seed), orc, scenes, rast, gpu)


def _run_configuration(seed, c, orc, scenes, rast, gpu, clips=(0, 1)):
    rng = c["rng"]
    P, W, H = c["P"], c["W"], c["H"]
    sc = scenes.synth(P, 2000 + seed, sh_degree=c["deg"], scale_mul=c["scale_mul"])
    if c["aniso"] != 1.0:
        sc["scales"][:, 0] *= (c["aniso"] ** rng.uniform(0, 1, P)).astype(np.float32)
    sc["opacities"] = (sc["opacities"] * c["opac_mul"]).astype(np.float32)
    sc["bg"] = c["bg"]
    if P <= 5:
        sc["means3D"] *= 0.2                              # keep the handful of Gaussians in view
    cam = scenes.camera(c["cam"][0], c["cam"][1], W, H)
    cam["scale_modifier"] = c["scale_modifier"]
    g = scenes.upstream_grad(H, W, 3000 + seed) * ((H * W) if c["big_grad"] else 1.0)
    kw = {}
    names = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity"]
    if c["use_rgb"]:
        kw["colors_precomp"] = rng.uniform(0, 1, size=(P, 3)).astype(np.float32)
        names.append("dL_dcolors")
    else:
        names.append("dL_dsh")
    if c["use_cov"]:
        base = orc.forward(sc, cam)
        kw["cov3D_precomp"] = np.ascontiguousarray(base["cov3D"]).astype(np.float32)
        names.append("dL_dcov3D")
    else:
        names += ["dL_dscales", "dL_drotations"]
    o32 = orc.render(sc, cam, g, **kw)
    o64 = orc.render(sc, cam, g, f64=True, **kw)
    for clip in clips:
        h = run_hip(rast, sc, cam, gpu, dL_dcolor=g, tile_clip=clip, **kw)
        if c["use_cov"]:
            # with a precomputed covariance the oracle's per-Gaussian cov3D is the input itself
            np.testing.assert_array_equal(h["radii"], o32["radii"])
            np.testing.assert_array_equal(bits(h["out_color"]), bits(o32["out_color"]))
            np.testing.assert_array_equal(bits(h["out_depth"]), bits(o32["out_depth"]))
        else:
            _check_forward_exact(o32, h, clipped=bool(clip))
        # dL/dcov3D amplifies the rounding of the conic gradient by (focal / depth)^2 ~ 1e4: with tens of thousands of sub-pixel
        # Gaussians the fp32 oracle itself misses the absolute bar there, so the large cases hold it to the fp32 oracle's own error
        # (likewise tens of thousands of image-sized or 10:1 Gaussians: thousands of contributors per pixel; tools/fuzz_one.py prints
        # the HIP and the fp32-oracle errors side by side -- the HIP path is the more accurate of the two on every tensor there)
        hard = P > 30000 and (c["use_cov"] or c["aniso"] >= 10.0 or c["scale_mul"] >= 8.0)
        _check_grads(o64, o32, h, names, strict=not c["big_grad"], conditioning=c["aniso"] > 10.0 or hard)
