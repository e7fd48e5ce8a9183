"""The depth-distortion map (`distortion=True`; include/gsrast.h: gsrast_distortion_forward / _backward) in torch -- a helper of the
tests, not a test.

    distort[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_{i-1} - D_{i-1})      over the pairs the forward blends at p

float64 (`evaluate64`): math_renderer.render returns no weights, so the pair loop is restated here on math_renderer.project -- the same
depth order (view-space z, ties by index), the same `ok` / `live` logic --, the colour with it (pinned against mr.render by
tests/test_distort_host.py), the distortion by cumulative sums along the depth order, the gradients of
    sum distort gd + sum color g0 [+ sum acc_depth gD + sum alpha gA]
by autograd (the screen-space mean's through project()'s ndc_offset).  Anti-aliasing: the opacity is o * comp (tests/aa_math.py).  Raw
path: features_math.activate in front of it, gradients with respect to the raw leaves (features_math.raw_arrays).

float32 (`restate32`): the same function in float32 on the discrete decisions of its own float64 pass (visibility, rectangles, order,
thresholds, clamps, lists) with the KERNEL'S association: depths relative to z0, the depth of the first Gaussian listed for the pixel's
tile.  What fp32 rounding alone does: the measure of the map's bar and the floor of conftest.grad_tol.  Its projection restates
posegrad_math.render's (camera tensors as leaves), so `camera_reference` gives the camera's gradients of a distortion-only loss as well.

Cases: contrib_math.CASES / case_scene (70 x 45, 5 x 3 ragged tiles).  Upstream gradients are zero on the fp64 render's fp32-ambiguous
pixels."""
import functools

import numpy as np
import torch

import aa_math
import contrib_math as cm
import features_math as fm
import math_renderer as mr
import posegrad_math as pm

VARIANTS = dict(plain=dict(), antialias=dict(aa=True), return_aux=dict(aux=True), raw=dict(raw=True))


def upstream(H, W, amb, seed=29):
    """dict(gd [H,W] for the map, g0 [3,H,W] colour, gD [H,W] acc_depth, gA [H,W] alpha), float32, zero on the ambiguous pixels."""
    rng = np.random.default_rng(seed)
    g = dict(gd=rng.normal(size=(H, W)), g0=rng.normal(size=(3, H, W)), gD=rng.normal(size=(H, W)) * 0.25, gA=rng.normal(size=(H, W)))
    g = {k: v.astype(np.float32) for k, v in g.items()}
    for v in g.values():
        v[..., amb] = 0.0
    return g


def blend(pix, conic, o, z, col, bg, rect, W, H, D=None, z0_relative=False):
    """The pair loop in the dtype of its inputs: Gaussians in depth order (pix [K,2], conic [K,3], o [K], z [K], col [K,3], rect [K,4] tile
    rectangles), pixels row-major.  D: the discrete decisions of an earlier pass (listed, ok, live) or None = decide here.  z0_relative: the
    kernel's association.  dict(color [3,H,W], acc_depth, alpha, distort [H,W], w [N,K], live, decisions)."""
    dt = pix.dtype
    first = D is None
    D = {} if first else D
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)
    dx, dy = pix[None, :, 0] - px, pix[None, :, 1] - py
    power = -0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) - conic[None, :, 1] * dx * dy
    alpha = mr.clamp_passthrough(o[None, :] * torch.exp(power), mr.C_AMAX)
    if first:
        with torch.no_grad():
            tx, ty = torch.div(px, 16, rounding_mode="floor"), torch.div(py, 16, rounding_mode="floor")
            D["listed"] = (tx >= rect[None, :, 0]) & (tx < rect[None, :, 2]) & (ty >= rect[None, :, 1]) & (ty < rect[None, :, 3])
            D["ok"] = D["listed"] & (power <= 0.0) & (alpha >= mr.C_AMIN)
    ok = D["ok"]
    one_minus = torch.where(ok, 1.0 - alpha, torch.ones_like(alpha))
    T_incl = torch.cumprod(one_minus, dim=1)
    T_excl = T_incl / one_minus
    if first:
        with torch.no_grad():
            D["live"] = ok & (T_incl >= mr.C_TMIN)          # the pair that would push T below 1e-4 ends the pixel
    live = D["live"]
    w = torch.where(live, alpha * T_excl, torch.zeros_like(alpha))
    T_final = torch.where(live, one_minus, torch.ones_like(alpha)).prod(dim=1)
    colour = w @ col + T_final[:, None] * torch.as_tensor(np.asarray(bg, np.float64)).to(dt)[None, :]
    zr = z[None, :]
    if z0_relative:
        with torch.no_grad():
            has = D["listed"].any(dim=1)
            z0 = torch.where(has, z.detach()[torch.argmax(D["listed"].to(torch.int8), dim=1)], torch.zeros((), dtype=dt))
        zr = zr - z0[:, None]
    zero = torch.zeros_like(w[:, :1])
    A_prev = torch.cat([zero, torch.cumsum(w, dim=1)[:, :-1]], dim=1)
    D_prev = torch.cat([zero, torch.cumsum(w * zr, dim=1)[:, :-1]], dim=1)
    distort = 2.0 * (w * (zr * A_prev - D_prev)).sum(dim=1)
    return dict(color=colour.T.reshape(3, H, W), acc_depth=(w @ z).reshape(H, W), alpha=(1.0 - T_final).reshape(H, W), distort=distort.reshape(H, W),
                w=w, live=live, decisions=D)


def _loss(out, g, dt, colour_loss, aux, distort_loss=True):
    L = torch.zeros((), dtype=dt)
    tt = lambda a: torch.as_tensor(a).to(dt)      # noqa: E731
    if distort_loss:
        L = L + (out["distort"] * tt(g["gd"])).sum()
    if colour_loss:
        L = L + (out["color"] * tt(g["g0"])).sum()
    if aux:
        L = L + (out["acc_depth"] * tt(g["gD"])).sum() + (out["alpha"] * tt(g["gA"])).sum()
    return L


def pairs64(sc, cam, aa=False, raw=False):
    """The float64 pair loop on math_renderer.project: (leaves, the means2D sink, math_renderer.render's result, blend()'s result)."""
    leaves, d = fm._leaves(sc, raw, torch.float64)
    P = d["means3D"].shape[0]
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    o = d["opacities"]
    if aa:
        comp, _ = aa_math.comp(d["means3D"], d["scales"], d["rotations"], cam)
        o = o * comp[:, None]
    deg = int(sc.get("sh_degree", 3))
    with torch.no_grad():
        ref = mr.render(d["means3D"], d["scales"], d["rotations"], o, d["shs"], deg, cam, sc["bg"])
    pr = mr.project(d["means3D"], d["scales"], d["rotations"], cam, ndc_offset=off)
    idx = torch.as_tensor(ref["order"])                     # visible Gaussians by view-space z, ties by index
    dirs = d["means3D"] - torch.as_tensor(np.asarray(cam["campos"], np.float64))
    col = torch.clamp(mr.sh_colour(deg, d["shs"], dirs / torch.linalg.norm(dirs, dim=1, keepdim=True)) + 0.5, min=0.0)
    out = blend(pr["pix"][idx], pr["conic"][idx], o.reshape(-1)[idx], pr["depth"][idx], col[idx], sc["bg"], torch.as_tensor(pr["disc"]["rect"])[idx],
                pr["W"], pr["H"])
    return leaves, off, ref, out


def evaluate64(sc, cam, aa=False, raw=False, aux=False, colour_loss=True, g=None):
    """One float64 forward + backward.  dict(map [H,W], color, acc_depth, alpha, amb [H,W], g, grads {leaf, "means2D"}, vis, n_live, w, z)."""
    leaves, off, ref, out = pairs64(sc, cam, aa, raw)
    H, W = out["distort"].shape
    amb = ref["ambiguous"]
    g = g if g is not None else upstream(H, W, amb)
    _loss(out, g, torch.float64, colour_loss, aux).backward()
    np_ = lambda x: x.detach().numpy()      # noqa: E731
    return dict(map=np_(out["distort"]), color=np_(out["color"]), ref_color=np_(ref["color"]), acc_depth=np_(out["acc_depth"]), alpha=np_(out["alpha"]), amb=amb, g=g,
                grads=fm._grads(leaves, dict(means2D=off)), vis=ref["proj"]["disc"]["vis"], n_live=np_(out["live"].sum(dim=1)).reshape(H, W),
                w=np_(out["w"]), z=np_(ref["proj"]["depth"])[ref["order"]], final_T=np_(ref["final_T"]))


def project(t, V, Pm, Cp, cfg, D, off=None):
    """posegrad_math.render's projection, restated (camera tensors as given; `off`: the means2D sink added to ndc.xy): the per-Gaussian
    quantities of the visible Gaussians in depth order, in the dtype of the inputs, on the decisions D (filled on the first pass)."""
    m = t["means3D"]
    dt, W, H = m.dtype, cfg["W"], cfg["H"]
    first = "idx" not in D
    fx, fy = W / (2.0 * cfg["tanx"]), H / (2.0 * cfg["tany"])
    ph = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    tv = (ph @ V)[:, :3]
    hom = ph @ Pm
    pw = 1.0 / (hom[:, 3] + mr.C_WEPS)
    ndc = hom[:, :2] * pw[:, None]
    if off is not None:
        ndc = ndc + off
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    Mx = mr.rotation_matrix(t["rotations"]) * t["scales"][:, None, :]
    Sigma = Mx @ Mx.transpose(1, 2)
    limx, limy = mr.C_LIM * cfg["tanx"], mr.C_LIM * cfg["tany"]
    tz = tv[:, 2]
    rx, ry = tv[:, 0] / tz, tv[:, 1] / tz
    if first:
        with torch.no_grad():
            D["clx"], D["cly"] = rx.abs() > limx, ry.abs() > limy
            D["sx"], D["sy"] = torch.sign(rx), torch.sign(ry)
    cx, cy = (D["sx"].to(dt) * limx * tz).detach(), (D["sy"].to(dt) * limy * tz).detach()
    txc, tyc = torch.where(D["clx"], cx, rx * tz), torch.where(D["cly"], cy, ry * tz)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], dim=1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    cov2 = A @ Sigma @ A.transpose(1, 2)
    c00, c11 = cov2[:, 0, 0], cov2[:, 1, 1]
    a, b, c2 = c00 + mr.C_DILATE, cov2[:, 0, 1], c11 + mr.C_DILATE
    with torch.no_grad():
        det0 = a * c2 - b * b
        reg = det0 * det0 / (det0 * det0 + mr.C_WEPS)
    ar, br, cr = mr._scale_grad(a, reg), mr._scale_grad(b, reg), mr._scale_grad(c2, reg)
    det = ar * cr - br * br
    conic = torch.stack([cr / det, -br / det, ar / det], dim=1)
    if first:
        with torch.no_grad():
            mid = 0.5 * (a + c2)
            radius = torch.ceil(3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))))
            gx, gy = (W + 15) // 16, (H + 15) // 16
            x0 = torch.clamp(torch.trunc((pix[:, 0] - radius) / 16.0), 0, gx); x1 = torch.clamp(torch.trunc((pix[:, 0] + radius + 15.0) / 16.0), 0, gx)
            y0 = torch.clamp(torch.trunc((pix[:, 1] - radius) / 16.0), 0, gy); y1 = torch.clamp(torch.trunc((pix[:, 1] + radius + 15.0) / 16.0), 0, gy)
            vis = (tz > mr.C_NEAR) & (det != 0.0) & ((x1 - x0) * (y1 - y0) > 0)
            idx = torch.nonzero(vis)[:, 0]
            idx = idx[torch.as_tensor(np.lexsort((idx.numpy(), tz[idx].numpy())))]
            D.update(vis=vis, idx=idx, rect=torch.stack([x0, y0, x1, y1], 1)[idx])
    idx = D["idx"]
    o = t["opacities"].reshape(-1)
    if cfg["aa"]:
        rho = (c00 * c11 - b * b) / (a * c2 - b * b)
        if first:
            D["floor"] = (rho <= aa_math.FLOOR).detach()
        o = o * torch.where(D["floor"], torch.full_like(rho, aa_math.FLOOR ** 0.5), torch.sqrt(torch.where(D["floor"], torch.ones_like(rho), rho)))
    d = m - Cp
    raw = mr.sh_colour(cfg["deg"], t["shs"], d / torch.linalg.norm(d, dim=1, keepdim=True)) + 0.5
    if first:
        D["colpos"] = (raw > 0.0).detach()
    col = torch.where(D["colpos"], raw, torch.zeros_like(raw))
    return dict(pix=pix[idx], conic=conic[idx], o=o[idx], z=tz[idx], col=col[idx], rect=D["rect"])


def _run(sc, cam, dtype, D, g, aa, raw, aux, colour_loss, camera=False, z0_relative=True):
    """One pass of the restated renderer in `dtype` on the decisions D (None: decide).  (decisions, map, grads, camera grads)."""
    leaves, d = fm._leaves(sc, raw, dtype)
    V, Pm, Cp = pm.camera_leaves(cam, dtype)
    cfg = pm.cfg_of(cam, sc, aa=aa)
    off = torch.zeros((d["means3D"].shape[0], 2), dtype=dtype, requires_grad=True)
    D = {} if D is None else D
    pr = project(d, V, Pm, Cp, cfg, D, off)
    out = blend(pr["pix"], pr["conic"], pr["o"], pr["z"], pr["col"], cfg["bg"], pr["rect"], cfg["W"], cfg["H"], D.get("blend"), z0_relative=z0_relative)
    D["blend"] = out["decisions"]
    if g is None:
        return D, out, None, None
    _loss(out, g, dtype, colour_loss, aux).backward()
    z = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.double().numpy()      # noqa: E731
    return D, out, fm._grads(leaves, dict(means2D=off)), (dict(viewmatrix=z(V), projmatrix=z(Pm), campos=z(Cp)) if camera else None)


def restate32(sc, cam, g, aa=False, raw=False, aux=False, colour_loss=True):
    """The float32 restatement on its own float64 pass's decisions, z0-relative.  dict(map [H,W] float64 numpy, grads {leaf, "means2D"})."""
    with torch.no_grad():
        D, _, _, _ = _run(sc, cam, torch.float64, None, None, aa, raw, aux, colour_loss)
    _, out, grads, _ = _run(sc, cam, torch.float32, D, g, aa, raw, aux, colour_loss)
    return dict(map=out["distort"].detach().double().numpy(), grads=grads)


def camera_reference(sc, cam, g):
    """{float64 / float32: dict(viewmatrix, projmatrix, campos)}: the camera's gradients of the distortion-only loss sum distort gd."""
    D, _, _, c64 = _run(sc, cam, torch.float64, None, g, False, False, False, False, camera=True, z0_relative=False)
    _, _, _, c32 = _run(sc, cam, torch.float32, D, g, False, False, False, False, camera=True)
    return {torch.float64: c64, torch.float32: c32}


def pairwise(w, z):
    """sum_i sum_j w_i w_j |z_i - z_j| of one pixel's weights and depths, the O(K^2) way."""
    w, z = np.asarray(w, np.float64), np.asarray(z, np.float64)
    return float((w[:, None] * w[None, :] * np.abs(z[:, None] - z[None, :])).sum())


@functools.lru_cache(maxsize=None)
def _reference(name, variant, colour_loss):
    import scenes
    v = VARIANTS[variant]
    sc, cam = cm.case_scene(scenes, cm.CASES[name])
    aa, raw, aux = v.get("aa", False), v.get("raw", False), v.get("aux", False)
    r64 = evaluate64(sc, cam, aa=aa, raw=raw, aux=aux, colour_loss=colour_loss)
    r32 = restate32(sc, cam, r64["g"], aa=aa, raw=raw, aux=aux, colour_loss=colour_loss)
    return dict(sc=sc, cam=cam, r64=r64, r32=r32, aa=aa, raw=raw, aux=aux)


def reference(name, variant="plain", colour_loss=True):
    """The float64 / float32 references of one case and variant, computed once per process and shared: do not modify them."""
    return _reference(name, variant, bool(colour_loss))


def map_bar_terms(ref, got, ok):
    """(a, r) of one comparison on the pixels `ok`: r = the largest relative error among entries above a tenth of the map's maximum, a = what
    that leaves of the others, relative to the maximum (the bar is a max|ref| + r |ref|)."""
    ref, err = np.abs(ref[ok]), np.abs(got[ok] - ref[ok])
    big = ref > 0.1 * ref.max()
    r = float((err[big] / ref[big]).max())
    a = float(np.maximum(err - r * ref, 0.0).max() / ref.max())
    return a, r
