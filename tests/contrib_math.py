"""The per-Gaussian blend-weight statistics (include/gsrast.h: gsrast_contrib_stats; `contrib=sink` of the Python package) in torch --
a helper of the tests, not a test.

Built on tests/math_renderer.py: render() gives the discrete decisions of the projection (visibility, tile rectangles, depth order), final_T
and its fp32-ambiguity mask; project_gaussians and blend_pairs run again in `dtype` on those lists (`pairs`), and the weights and the
contribution decisions they return are turned into the [P, 4] table

    col 0 weight_sum = sum_p m_p w_ip   col 1 weight_max = max over m_p > 0 of w_ip   col 2 pixel_count   col 3 top_count

with w_ip = alpha_ip T_ip for the pairs the forward blends (listed, power <= 0, alpha = min(0.99, o G) >= 1/255, T (1 - alpha) >= 1e-4) and
m_p = pixel_weights[p] clamped to [0, 1] (1 without weights).  `ambiguous` [H, W] is render()'s own mask OR'd with the pixels whose best
and second-best w differ by less than 1e-5 relative (a top_count coin flip).

`dtype`: the per-pair part -- and the continuous screen-space quantities it starts from (project_cont: math_renderer.project_gaussians
deciding its frustum clamp in `dtype`) -- run in this dtype; float32 is the fp32 evaluation the GPU test's tolerance is measured with.
Visibility, rectangles and the depth order always come from the float64 projection, so both dtypes walk the same lists.

CASES are the shapes of tests/test_gpu_contrib.py; the seeds were picked on the CPU so that the ambiguous pixels stay under 5 %."""
import functools

import numpy as np
import torch

import aa_math
import math_renderer as mr
from math_renderer import t64

W_IMG, H_IMG = 70, 45      # 5 x 3 tiles, ragged in both axes: 8 x 8 wave blocks lie half outside
CASES = dict(a=dict(kind="cluster", P=700, seed=2, k=1, V=6), b=dict(kind="sparse", P=2000, seed=4, k=2, V=6))
TOP_GAP = 1e-5


def _world(cam, px, py, z):
    """World positions of view-space points given by pixel coordinates and view depth z (any sign)."""
    W, H = cam["image_width"], cam["image_height"]
    x = ((2.0 * px + 1.0) / W - 1.0) * cam["tanfovx"] * z
    y = ((2.0 * py + 1.0) / H - 1.0) * cam["tanfovy"] * z
    view = np.stack([x, y, z, np.ones_like(z)], 1)
    return (view @ np.linalg.inv(cam["viewmatrix"].astype(np.float64)))[:, :3]


def _finish(rng, cam, px, py, z, scale, opac):
    P = len(px)
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    scales = scale[:, None] * np.exp(rng.uniform(-0.25, 0.25, size=(P, 3)))      # roughly isotropic: well-conditioned conics
    shs = np.zeros((P, 16, 3))
    shs[:, 0] = rng.uniform(-1.77, 1.77, size=(P, 3))
    shs[:, 1:] = rng.normal(0.0, 0.1, size=(P, 15, 3))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    return dict(means3D=f32(_world(cam, px, py, z)), scales=f32(scales), rotations=f32(q), opacities=f32(opac[:, None]), shs=f32(shs),
                sh_degree=3, bg=np.array([0.1, 0.2, 0.3], np.float32))


def case_scene(scenes, c):
    """(scene, camera) of a case, float32 arrays.
    cluster (A): 610 small translucent Gaussians whose 3-sigma squares all reach tile (2, 1) -- a list of more than two 256-entry batches,
    walked to its end --, 12 large ones spanning four or more tiles in front of and behind it, an opaque stack of 30 that terminates its
    pixels long before the list ends with 20 more hidden behind it, 14 behind the camera (or the near plane) and 14 off screen.
    sparse (B): 2000 small Gaussians over a region 13 x the image, none near tiles (0, 0) and (4, 2): most tiles hold under 64 entries, two are
    empty, most Gaussians get a zero row."""
    rng = np.random.default_rng(c["seed"])
    cam = scenes.camera(c["k"], c["V"], W_IMG, H_IMG)
    u = rng.uniform
    if c["kind"] == "cluster":
        parts = [  # px, py, z, scale, opacity
            (u(37, 43, 610), u(21, 27, 610), u(3.5, 4.5, 610), u(0.02, 0.05, 610), u(0.01, 0.06, 610)),
            (u(5, 65, 12), u(5, 40, 12), np.concatenate([u(2.6, 3.0, 4), u(5.0, 6.0, 8)]), u(0.5, 1.2, 12), u(0.05, 0.3, 12)),
            (u(11, 13, 30), u(9, 11, 30), u(2.0, 3.0, 30), u(0.10, 0.16, 30), u(0.9, 0.99, 30)),
            (u(10, 14, 20), u(8, 12, 20), u(4.0, 5.0, 20), u(0.05, 0.1, 20), u(0.3, 0.9, 20)),
            (u(10, 60, 14), u(5, 40, 14), np.concatenate([-u(1.0, 3.0, 10), u(0.05, 0.15, 4)]), u(0.05, 0.1, 14), u(0.3, 0.9, 14)),
            (np.concatenate([u(-300, -150, 7), u(220, 400, 7)]), u(-200, 250, 14), u(3.0, 5.0, 14), u(0.03, 0.06, 14), u(0.3, 0.9, 14)),
        ]
        cols = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    else:
        P = c["P"]
        px, py = np.empty(0), np.empty(0)
        while len(px) < P:      # rejection: nothing within 10 px of the two tiles that stay empty
            x, y = u(-90, 160, P), u(-60, 105, P)
            near = ((x < 26) & (y < 26)) | ((x > 54) & (y > 22))
            px, py = np.concatenate([px, x[~near]])[:P], np.concatenate([py, y[~near]])[:P]
        cols = [px, py, u(2.5, 6.0, P), u(0.02, 0.07, P), 1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.0, P)))]
    perm = rng.permutation(len(cols[0]))      # index order is not depth or kind order
    sc = _finish(rng, cam, *[col[perm] for col in cols])
    assert sc["means3D"].shape[0] == c["P"]
    return sc, cam


def _project(means3D, scales, rotations, cam, dtype):
    t = dict(means3D=means3D.to(dtype), scales=scales.to(dtype), rotations=rotations.to(dtype))
    return mr.project_gaussians(t, t64(cam["viewmatrix"]).to(dtype), t64(cam["projmatrix"]).to(dtype), None, mr.camera_cfg(cam))


def project_cont(means3D, scales, rotations, cam, dtype):
    """(pix [P,2], conic [P,3] = (A, B, C), cov2 = (a, b, c) dilated) in `dtype`: math_renderer.project_gaussians deciding in `dtype`
    (EWA projection, frustum clamp, + 0.3 dilation), every operand and operation in `dtype`."""
    pr = _project(means3D, scales, rotations, cam, dtype)
    return pr["pix"], pr["conic"], pr["cov2"]


def pairs(sc, cam, dtype=torch.float64, antialiasing=False, render_out=None):
    """(math_renderer.blend_pairs' result in `dtype` on the float64 render's lists, out = math_renderer.render's result) of one scene."""
    m, s, q, sh, o = t64(sc["means3D"]), t64(sc["scales"]), t64(sc["rotations"]), t64(sc["shs"]), t64(sc["opacities"])
    with torch.no_grad():
        pr = _project(m, s, q, cam, dtype)
        o_d = o[:, 0].to(dtype)
        if antialiasing:
            vidx = torch.as_tensor(mr.project(m, s, q, cam)["disc"]["vis"]).nonzero()[:, 0]
            comp64, _ = aa_math.comp(m[vidx], s[vidx], q[vidx], cam)
            o = o[:, 0].index_put((vidx,), o[vidx, 0] * comp64)[:, None]
            o_d = o_d * aa_math.comp_of_cov2(*pr["cov2"])[0]
        out = render_out if render_out is not None else mr.render(m, s, q, o, sh, int(sc.get("sh_degree", 3)), cam, sc["bg"])
        idx = torch.as_tensor(out["order"])                        # visible Gaussians in depth order
        g = dict(pix=pr["pix"][idx], conic=pr["conic"][idx], o=o_d[idx], z=pr["depth"][idx], col=None, rect=out["proj"]["sorted"]["rect"])
        return mr.blend_pairs(g, None, pr["W"], pr["H"]), out


def contrib(sc, cam, pixel_weights=None, dtype=torch.float64, antialiasing=False, render_out=None):
    """(table [P,4] float64 numpy, ambiguous [H,W] bool numpy, out = math_renderer.render's result) of one scene.
    pixel_weights: [H,W] array or None.  antialiasing: the opacity is o * comp (tests/aa_math.py).  render_out: a previous call's `out`
    for the same scene and antialiasing (the float64 render is the expensive part and does not depend on dtype or weights)."""
    P = sc["means3D"].shape[0]
    bl, out = pairs(sc, cam, dtype, antialiasing, render_out)
    with torch.no_grad():
        H, W = out["ambiguous"].shape
        idx, live, w = torch.as_tensor(out["order"]), bl["live"], bl["w"].to(torch.float64)      # [N, K]
        N, K = w.shape
        mp = torch.ones((N,), dtype=torch.float64) if pixel_weights is None else torch.clamp(t64(pixel_weights).reshape(-1), 0.0, 1.0)
        active = mp > 0.0
        table = torch.zeros((P, 4), dtype=torch.float64)
        amb = torch.as_tensor(out["ambiguous"].reshape(-1).copy())
        if K > 0:
            wa = w * active[:, None]
            table[idx, 0] = (w * mp[:, None]).sum(dim=0)
            table[idx, 1] = wa.max(dim=0).values
            table[idx, 2] = (live & active[:, None]).sum(dim=0).to(torch.float64)
            best = torch.argmax(w, dim=1)                          # the FIRST maximal entry: list order breaks a tie
            has = live.any(dim=1) & active
            table[idx, 3] = torch.bincount(best[has], minlength=K).to(torch.float64)
            if K > 1:
                top2 = torch.topk(w, 2, dim=1).values
                amb = amb | ((top2[:, 1] > 0.0) & ((top2[:, 0] - top2[:, 1]) < TOP_GAP * top2[:, 0]))
    return table.numpy(), amb.reshape(H, W).numpy(), out


@functools.lru_cache(maxsize=None)
def _reference(name, antialiasing):
    import scenes
    c = CASES[name]
    sc, cam = case_scene(scenes, c)
    _, amb, out = contrib(sc, cam, antialiasing=antialiasing)      # the mask first, then the table with the ambiguous pixels weighted out
    weights = (~amb).astype(np.float32)
    table, _, _ = contrib(sc, cam, pixel_weights=weights, antialiasing=antialiasing, render_out=out)
    return dict(sc=sc, cam=cam, c=c, amb=amb, weights=weights, table=table, out=out)


def reference(name, antialiasing=False):
    """The float64 reference of CASES[name] with pixel_weights = ~ambiguous, computed once per process and shared: do not modify it."""
    return _reference(name, bool(antialiasing))
