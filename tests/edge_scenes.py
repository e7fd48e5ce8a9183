"""Small scenes with the Gaussians a training view has at its borders -- a helper of the tests, not a test.

edge_scene(scenes, c) is scenes.synth + needles + Gaussians at the near plane + Gaussians whose centre lies OUTSIDE 1.3 x the field
of view while their footprint reaches into the image.  For the last group the projection clamps t.x / t.z, t.y / t.z before the Jacobian
(forward.cu:82-87) and the reference's backward treats the clamped value as a constant (backward.cu:172-176, :262-264);
tests/math_renderer.py reproduces that convention (clamp_grad="reference"), so these rows are compared like every other row, and once
more as a tensor of their own (clamped_mask), at their own scale: their gradients are 2-3 orders of magnitude below the tensor's largest.

c: dict(P, seed, W, H, k, V, deg, smul, bg[, omul]) -- the same keys as the CASES / SMALL lists of the tests.

CASES, case_inputs and reference (below) are the six edge cases of tests/test_gpu_independent.py with their fp64 side; the
reference-kernel tests share them."""
import numpy as np
import torch

import math_renderer as mr

# (ratio of |t.x / t.z| to tanfovx resp. |t.y / t.z| to tanfovy; the clamp sets in at 1.3): from just outside to far outside
RATIOS = (1.31, 1.45, 1.7, 2.0, 2.5)
N_CLAMPED = 4 * len(RATIOS) + 8
N_NEAR = 4
NEAR_SCALE = 0.012      # at z = 0.2 ... 0.3 a footprint of some ten pixels: larger ones would own every pixel's median depth
N_NEEDLES = 6


def _clamped_centres(cam, rng):
    """View-space centres + isotropic scales of N_CLAMPED Gaussians outside the clamp: x only, y only and both axes, both signs."""
    tx, ty = cam["tanfovx"], cam["tanfovy"]
    spec = []                                   # (x / (tanfovx z), y / (tanfovy z))
    for r in RATIOS:
        for s in (-1.0, 1.0):
            spec.append((s * r, rng.uniform(-0.8, 0.8)))           # x only
            spec.append((rng.uniform(-0.8, 0.8), s * r))           # y only
    for r, q in ((1.31, 1.6), (1.9, 1.4)):                          # both axes, the four corners
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                spec.append((sx * r, sy * q))
    pts, scl = [], []
    for ax, ay in spec:
        z = rng.uniform(2.0, 5.0)
        pts.append([ax * tx * z, ay * ty * z, z])
        # the image's edge is at ratio 1: sigma = 2/3 of the centre's distance from it, so the footprint reaches well inside
        out = np.hypot(max(abs(ax) - 1.0, 0.0) * tx, max(abs(ay) - 1.0, 0.0) * ty) * z
        scl.append(max(0.15, out / 1.5))
    return np.array(pts), np.array(scl)


def edge_scene(scenes, c):
    """(scene, camera).  The added rows are the LAST N_NEAR + N_CLAMPED ones; the needles are rows 0 .. N_NEEDLES - 1."""
    sc = scenes.synth(c["P"], c["seed"], sh_degree=c["deg"], scale_mul=c["smul"])
    sc["bg"] = np.array(c["bg"], np.float32)
    sc["opacities"] = (sc["opacities"] * c.get("omul", 1.0)).astype(np.float32)
    cam = scenes.camera(c["k"], c["V"], c["W"], c["H"])
    V = cam["viewmatrix"].astype(np.float64)
    Vi = np.linalg.inv(V)
    rng = np.random.default_rng(c["seed"] + 7)
    pts = []
    for _ in range(N_NEAR):      # just in front of / behind the near plane (z = 0.2) near the optical axis
        pts.append([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.2 + rng.choice([-1, 1]) * rng.uniform(0.02, 0.1)])
    cpts, cscl = _clamped_centres(cam, rng)
    pts = np.concatenate([np.array(pts), cpts])
    world = (np.concatenate([pts, np.ones((len(pts), 1))], 1) @ Vi)[:, :3]
    n = len(pts)
    for i in range(N_NEEDLES):      # needles among the visible ones
        sc["scales"][i] = np.array([0.3, 0.004, 0.004], np.float32) * c["smul"]
    scl = np.concatenate([np.full(N_NEAR, NEAR_SCALE), cscl])
    opa = np.concatenate([np.full(N_NEAR, 0.6), rng.uniform(0.15, 0.5, len(cscl))])
    sc["means3D"] = np.concatenate([sc["means3D"], world.astype(np.float32)])
    sc["scales"] = np.concatenate([sc["scales"], np.repeat(scl[:, None], 3, 1).astype(np.float32)])
    sc["rotations"] = np.concatenate([sc["rotations"], np.tile(np.array([[1, 0, 0, 0]], np.float32), (n, 1))])
    sc["opacities"] = np.concatenate([sc["opacities"], opa[:, None].astype(np.float32)])
    sc["shs"] = np.concatenate([sc["shs"], sc["shs"][:n]])
    return sc, cam


def clamped_mask(sc, cam, cov3D=None):
    """bool [P]: the visible Gaussians whose t.x / t.z or t.y / t.z the projection clamps (math_renderer.project's own decisions, fp64).
    None of them may sit within fp32 rounding of the clamp's threshold -- the builder's start at 1.31 / 1.3 of it."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))      # noqa: E731
    d = mr.project(t(sc["means3D"]), t(sc["scales"]), t(sc["rotations"]), cam, cam.get("scale_modifier", 1.0),
                   None if cov3D is None else t(cov3D))["disc"]
    V = cam["viewmatrix"].astype(np.float64)
    tv = sc["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    rx, ry = np.abs(tv[:, 0] / tv[:, 2]) / (mr.C_LIM * mr.F32(cam["tanfovx"])), np.abs(tv[:, 1] / tv[:, 2]) / (mr.C_LIM * mr.F32(cam["tanfovy"]))
    firm = (np.abs(rx - 1.0) > 1e-5) & (np.abs(ry - 1.0) > 1e-5)
    assert firm[d["vis"]].all(), "a visible Gaussian sits on the frustum clamp's threshold: pick another seed"
    return d["clamped"] & d["vis"]


# ---- the cases built on edge_scene, shared by tests/test_gpu_independent.py, tests/test_gpu_reference_kernels.py, tests/test_oracle_ref_kernels.py ----

CASES = [
    # SH degree 3, non-zero background, long lists: > 256 per tile (the forward blend's second staging round), > 128 contributors per pixel
    dict(name="a_deg3_long_lists", P=1500, seed=49, W=64, H=48, k=2, V=7, deg=3, smul=1.0, bg=(0.3, 0.1, 0.2), omul=0.35, aux=True, long=True),
    # SH degree 1, white background, an image that is no multiple of the 16 x 16 tile
    dict(name="b_deg1_white_50x37", P=600, seed=61, W=50, H=37, k=0, V=3, deg=1, smul=1.2, bg=(1.0, 1.0, 1.0), omul=1.0),
    # SH degree 2, a third of the DC coefficients at -2: colour channels clamped at zero
    dict(name="c_deg2_colour_clamp", P=800, seed=67, W=96, H=64, k=1, V=5, deg=2, smul=0.8, bg=(0.0, 0.0, 0.0), omul=0.8, dark=True),
    # precomputed colours and 3-D covariances
    dict(name="d_precomp_colour_cov3D", P=500, seed=63, W=80, H=64, k=3, V=7, deg=0, smul=0.9, bg=(0.1, 0.2, 0.3), omul=0.7, aux=True, precomp=True),
    # scale_modifier
    dict(name="e_scale_modifier_0.7", P=500, seed=64, W=80, H=64, k=2, V=6, deg=0, smul=1.0, bg=(0.0, 0.5, 0.0), omul=0.6, scale_modifier=0.7),
    # saturating opacities on big Gaussians: alpha clamped at 0.99, pixels ended by the T < 1e-4 stop
    dict(name="f_saturated_early_stop", P=300, seed=65, W=64, H=64, k=1, V=4, deg=0, smul=1.5, bg=(0.0, 0.0, 0.0), omul=1.0, aux=True, saturate=True),
]


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def case_inputs(scenes, c):
    """(scene, camera, names of the case's leaves): float32 arrays, the inputs of both sides."""
    if c.get("contrib"):      # tests/contrib_math.py's scenes: Gaussians behind the camera and off screen, empty tiles
        import contrib_math
        sc, cam = contrib_math.case_scene(scenes, contrib_math.CASES[c["contrib"]])
    else:
        sc, cam = edge_scene(scenes, c)
    P = sc["means3D"].shape[0]
    cam["scale_modifier"] = float(c.get("scale_modifier", 1.0))
    if c.get("dark"):
        sc["shs"][::3, 0, :] = -2.0
    if c.get("saturate"):
        big = np.argsort(-sc["scales"].max(axis=1))[:P // 3]
        sc["opacities"][big] = 0.999
    names = ["means3D", "opacities"]
    if c.get("precomp"):
        S = mr.project(t64(sc["means3D"]), t64(sc["scales"]), t64(sc["rotations"]), cam)["Sigma"].numpy()
        sc["cov3D"] = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
        sc["rgb"] = np.random.default_rng(c["seed"] + 5).uniform(0.0, 1.0, size=(P, 3)).astype(np.float32)
        names += ["rgb", "cov3D"]
    else:
        names += ["shs", "scales", "rotations"]
    return sc, cam, names


def reference(scenes, c):
    """The fp64 side: forward, upstream gradient (zero on the ambiguous pixels), autograd's gradients of every leaf of the case."""
    sc, cam, names = case_inputs(scenes, c)
    P, W, H = sc["means3D"].shape[0], c["W"], c["H"]
    t = {n: t64(sc[n]).requires_grad_(True) for n in names}
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    pre = bool(c.get("precomp"))
    out = mr.render(t["means3D"], None if pre else t["scales"], None if pre else t["rotations"], t["opacities"], None if pre else t["shs"],
                    c["deg"], cam, sc["bg"], colors_precomp=t["rgb"] if pre else None, cov3D=t["cov3D"] if pre else None,
                    scale_modifier=cam["scale_modifier"], ndc_offset=off, clamp_grad="reference")
    amb = out["ambiguous"]
    g = (scenes.upstream_grad(H, W, c["seed"] + 1) * (H * W)).astype(np.float32)
    g[:, amb] = 0.0
    (out["color"] * t64(g)).sum().backward()
    want = {n: t[n].grad.numpy() for n in names}
    want["means2D"] = off.grad.numpy()
    return dict(sc=sc, cam=cam, names=names, out=out, g=g, g_seed=c["seed"] + 1, want=want, keep=~amb,
                clamped=clamped_mask(sc, cam, sc["cov3D"] if pre else None))
