"""The per-Gaussian blend-weight statistics (include/gsrast.h: gsrast_contrib_stats; `contrib=sink` of the Python package) in torch --
a helper of the tests, not a test.

Built on tests/math_renderer.py as it stands: project() gives the screen-space quantities and the discrete decisions (visibility, tile
rectangles), render() the depth order, final_T and its fp32-ambiguity mask.  Here the per-pair alpha, T and contribution decisions are
recomputed in render()'s depth order and turned into the [P, 4] table

    col 0 weight_sum = sum_p m_p w_ip   col 1 weight_max = max over m_p > 0 of w_ip   col 2 pixel_count   col 3 top_count

with w_ip = alpha_ip T_ip for the pairs the forward blends (listed, power <= 0, alpha = min(0.99, o G) >= 1/255, T (1 - alpha) >= 1e-4) and
m_p = pixel_weights[p] clamped to [0, 1] (1 without weights).  `ambiguous` [H, W] is render()'s own mask OR'd with the pixels whose best
and second-best w differ by less than 1e-5 relative (a top_count coin flip).

`dtype`: the per-pair part -- and the continuous screen-space quantities it starts from (project_cont: the same formulas as
math_renderer.project, checked against it in float64) -- run in this dtype; float32 is the fp32 restatement the GPU test's tolerance is
measured with.  The discrete decisions and the depth order always come from the float64 projection, so both dtypes walk the same lists.

CASES are the shapes of tests/test_gpu_contrib.py; the seeds were picked on the CPU so that the ambiguous pixels stay under 5 %."""
import functools

import numpy as np
import torch

import aa_math
import math_renderer as mr

W_IMG, H_IMG = 70, 45      # 5 x 3 tiles, ragged in both axes: 8 x 8 wave blocks lie half outside
CASES = dict(a=dict(kind="cluster", P=700, seed=2, k=1, V=6), b=dict(kind="sparse", P=2000, seed=4, k=2, V=6))
TOP_GAP = 1e-5


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


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


def project_cont(means3D, scales, rotations, cam, dtype):
    """(pix [P,2], conic [P,3] = (A, B, C), cov2 = (a, b, c) dilated) in `dtype`: the formulas of math_renderer.project (EWA projection,
    frustum clamp, + 0.3 dilation), every operand and operation in `dtype`."""
    W, H = int(cam["image_width"]), int(cam["image_height"])
    V = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float64)).to(dtype)
    Pm = torch.as_tensor(np.asarray(cam["projmatrix"], np.float64)).to(dtype)
    tanx, tany = mr.F32(cam["tanfovx"]), mr.F32(cam["tanfovy"])
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    m, s, q = means3D.to(dtype), scales.to(dtype), rotations.to(dtype)
    ph = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    t = (ph @ V)[:, :3]
    hom = ph @ Pm
    pw = 1.0 / (hom[:, 3] + mr.C_WEPS)
    ndc = hom[:, :2] * pw[:, None]
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    Mx = mr.rotation_matrix(q) * s[:, None, :]
    Sigma = Mx @ Mx.transpose(1, 2)
    tz = t[:, 2]
    txc = torch.clamp(t[:, 0] / tz, -mr.C_LIM * tanx, mr.C_LIM * tanx) * tz
    tyc = torch.clamp(t[:, 1] / tz, -mr.C_LIM * tany, mr.C_LIM * tany) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], dim=1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    cov2 = A @ Sigma @ A.transpose(1, 2)
    a, b, c2 = cov2[:, 0, 0] + mr.C_DILATE, cov2[:, 0, 1], cov2[:, 1, 1] + mr.C_DILATE
    det = a * c2 - b * b
    return pix, torch.stack([c2 / det, -b / det, a / det], dim=1), (a, b, c2)


def contrib(sc, cam, pixel_weights=None, dtype=torch.float64, antialiasing=False, render_out=None):
    """(table [P,4] float64 numpy, ambiguous [H,W] bool numpy, out = math_renderer.render's result) of one scene.
    pixel_weights: [H,W] array or None.  antialiasing: the opacity is o * comp (tests/aa_math.py).  render_out: a previous call's `out`
    for the same scene and antialiasing (the float64 render is the expensive part and does not depend on dtype or weights)."""
    P = sc["means3D"].shape[0]
    m, s, q, sh, o = t64(sc["means3D"]), t64(sc["scales"]), t64(sc["rotations"]), t64(sc["shs"]), t64(sc["opacities"])
    with torch.no_grad():
        pr64 = mr.project(m, s, q, cam)
        vis = torch.as_tensor(pr64["disc"]["vis"])
        vidx = vis.nonzero()[:, 0]
        pix_d, conic_d, cov2_d = project_cont(m[vidx], s[vidx], q[vidx], cam, dtype)
        if dtype == torch.float64:      # the restatement IS math_renderer's projection
            assert float((pix_d - pr64["pix"][vidx]).abs().max()) < 1e-9 and float((conic_d / pr64["conic"][vidx] - 1.0).abs().max()) < 1e-6
        if antialiasing:
            comp64, _ = aa_math.comp(m[vidx], s[vidx], q[vidx], cam)
            o = o[:, 0].index_put((vidx,), o[vidx, 0] * comp64)[:, None]
            comp_d, _ = aa_math.comp_of_cov2(*cov2_d)
            o_d = (t64(sc["opacities"])[vidx, 0].to(dtype) * comp_d)
        else:
            o_d = o[vidx, 0].to(dtype)
        out = render_out if render_out is not None else mr.render(m, s, q, o, sh, int(sc.get("sh_degree", 3)), cam, sc["bg"])
        W, H = pr64["W"], pr64["H"]
        idx = torch.as_tensor(out["order"])                        # visible Gaussians in depth order
        where = torch.full((P,), -1, dtype=torch.int64)
        where[vidx] = torch.arange(len(vidx))
        sel = where[idx]
        pix, conic, od = pix_d[sel], conic_d[sel], o_d[sel]
        rect = torch.as_tensor(pr64["disc"]["rect"])[idx]
        ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
        px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)
        tx, ty = torch.div(px, 16, rounding_mode="floor"), torch.div(py, 16, rounding_mode="floor")
        listed = (tx >= rect[None, :, 0]) & (tx < rect[None, :, 2]) & (ty >= rect[None, :, 1]) & (ty < rect[None, :, 3])
        dx, dy = pix[None, :, 0] - px, pix[None, :, 1] - py
        power = -0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) - conic[None, :, 1] * dx * dy
        alpha = torch.clamp(od[None, :] * torch.exp(power), max=mr.C_AMAX)
        ok = listed & (power <= 0.0) & (alpha >= mr.C_AMIN)
        one_minus = torch.where(ok, 1.0 - alpha, torch.ones_like(alpha))
        T_incl = torch.cumprod(one_minus, dim=1)
        T_excl = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)      # the transmittance in front of the pair
        live = ok & (T_incl >= mr.C_TMIN)                          # the pair that would push T below 1e-4 ends the pixel
        w = torch.where(live, alpha * T_excl, torch.zeros_like(alpha)).to(torch.float64)      # [N, K]
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
