"""The renderer with the CAMERA as differentiable input, in torch -- a helper of the tests, not a test.

tests/math_renderer.py turns viewmatrix / projmatrix / campos into constants through numpy; here they are three leaf tensors
(include/gsrast.h: GSRAST_RENDER_POSEGRAD treats them as three independent inputs) and autograd of the forward below gives their
gradients.  The conventions are math_renderer's (its docstring): row-vector matrices stored transposed, t = [mean, 1] @ viewmatrix,
hom = [mean, 1] @ projmatrix; the 0.99 alpha clamp straight-through; no gradient through the median depth (not rendered here); a
frustum-clamped t.x / t.y a constant inside J (clamp_grad="reference"; "true" differentiates the clamp as written);
det^2 / (det^2 + 1e-7) in the conic chain; dL/dscales with respect to scale_modifier * scales.  tanfovx / tanfovy are constants.
No tile lists, no hand-written gradient, nothing shared with csrc/ or oracle/.

Per-Gaussian contributions: every Gaussian gets its OWN copy of the three camera tensors ([P,4,4], [P,4,4], [P,3], `per` in the result);
after a backward their .grad rows are the Gaussians' terms of the three sums -- what the tests need to assert non-vacuity and to form
sum_i |term_i|.

fp32: render(..., decisions=<the fp64 pass's>) evaluates the same expressions in the dtype of its inputs on the discrete decisions
(visibility, rectangles, order, the alpha / transmittance thresholds, clamps, the anti-aliasing floor) of the fp64 pass -- the `ref32` of
conftest.grad_tol: what fp32 rounding alone does to these sums.

halve: "JW" multiplies the gradient that reaches viewmatrix through the rotation inside T = J W by 0.5 -- a wrong reference on purpose,
for the test that shows the bar biting."""
import functools

import numpy as np
import torch

import aa_math
import math_renderer as mr


def cfg_of(cam, sc, c=None, aa=False):
    """The constants of a render: sizes, focal tangents, background, SH degree, scale_modifier, anti-aliasing."""
    return dict(W=int(cam["image_width"]), H=int(cam["image_height"]), tanx=mr.F32(cam["tanfovx"]), tany=mr.F32(cam["tanfovy"]),
                bg=np.asarray(sc["bg"], np.float64), deg=int(c["deg"]) if c is not None else int(sc.get("sh_degree", 0)),
                scale_modifier=float(cam.get("scale_modifier", 1.0)), aa=bool(aa))


def camera_leaves(cam, dtype=torch.float64):
    """(viewmatrix [4,4], projmatrix [4,4], campos [3]) as leaves that require grad."""
    return tuple(torch.as_tensor(np.asarray(cam[k], np.float64)).to(dtype).requires_grad_(True) for k in ("viewmatrix", "projmatrix", "campos"))


def _own_copies(x, P):
    e = x.unsqueeze(0).expand((P,) + tuple(x.shape)) * 1.0      # one row per Gaussian, each with its own gradient
    if e.requires_grad:
        e.retain_grad()
    return e


def render(t, V, Pm, C, cfg, decisions=None, clamp_grad="reference", halve=None, fp32_eps=4e-6):
    """t: dict of tensors -- means3D [P,3], opacities [P,1] and (shs [P,M,3], scales, rotations) or (rgb [P,3], cov3D [P,6]).
    Returns dict(color [3,H,W], acc_depth [H,W], alpha [H,W], per=(Ve, Pe, Ce), decisions, ambiguous [H,W], n_live, clamped [P], vis [P])."""
    assert clamp_grad in ("reference", "true") and halve in (None, "JW")
    m = t["means3D"]
    dt, P, W, H = m.dtype, m.shape[0], cfg["W"], cfg["H"]
    first = decisions is None
    D = {} if first else decisions
    Ve, Pe, Ce = _own_copies(V, P), _own_copies(Pm, P), _own_copies(C, P)
    fx, fy = W / (2.0 * cfg["tanx"]), H / (2.0 * cfg["tany"])
    ph = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    tv = torch.einsum("pr,prc->pc", ph, Ve)[:, :3]
    hom = torch.einsum("pr,prc->pc", ph, Pe)
    pw = 1.0 / (hom[:, 3] + mr.C_WEPS)
    ndc = hom[:, :2] * pw[:, None]
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    if "cov3D" in t:
        c6 = t["cov3D"]
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], dim=1).reshape(-1, 3, 3)
    else:
        s_mod = cfg["scale_modifier"] * t["scales"]
        if cfg["scale_modifier"] != 1.0:
            s_mod = mr._scale_grad(s_mod, 1.0 / cfg["scale_modifier"])
        Mx = mr.rotation_matrix(t["rotations"]) * s_mod[:, None, :]
        Sigma = Mx @ Mx.transpose(1, 2)
    limx, limy = mr.C_LIM * cfg["tanx"], mr.C_LIM * cfg["tany"]
    tz = tv[:, 2]
    rx, ry = tv[:, 0] / tz, tv[:, 1] / tz
    if first:
        with torch.no_grad():
            D["clx"], D["cly"] = rx.abs() > limx, ry.abs() > limy
            D["sx"], D["sy"] = torch.sign(rx), torch.sign(ry)
    cx, cy = D["sx"].to(dt) * limx * tz, D["sy"].to(dt) * limy * tz
    if clamp_grad == "reference":
        cx, cy = cx.detach(), cy.detach()
    txc, tyc = torch.where(D["clx"], cx, rx * tz), torch.where(D["cly"], cy, ry * tz)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], dim=1).reshape(-1, 2, 3)
    Wr = Ve[:, :3, :3].transpose(1, 2)
    if halve == "JW":
        Wr = mr._scale_grad(Wr, 0.5)
    A = J @ Wr
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
            z = tz[idx]
            idx = idx[torch.as_tensor(np.lexsort((idx.numpy(), z.numpy())))]
            D.update(vis=vis, idx=idx, rect=torch.stack([x0, y0, x1, y1], 1)[idx])
    idx, rect = D["idx"], D["rect"]
    o = t["opacities"].reshape(-1)
    if cfg["aa"]:
        rho = (c00 * c11 - b * b) / (a * c2 - b * b)
        if first:
            D["floor"] = (rho <= aa_math.FLOOR).detach()
        o = o * torch.where(D["floor"], torch.full_like(rho, aa_math.FLOOR ** 0.5), torch.sqrt(torch.where(D["floor"], torch.ones_like(rho), rho)))
    if "rgb" in t:
        col = t["rgb"]
    else:
        d = m - Ce
        raw = mr.sh_colour(cfg["deg"], t["shs"], d / torch.linalg.norm(d, dim=1, keepdim=True)) + 0.5
        if first:
            D["colpos"] = (raw > 0.0).detach()
        col = torch.where(D["colpos"], raw, torch.zeros_like(raw))
    pixk, conk, ok_o, colk, depk = pix[idx], conic[idx], o[idx], col[idx], tz[idx]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)
    dx, dy = pixk[None, :, 0] - px, pixk[None, :, 1] - py
    power = -0.5 * (conk[None, :, 0] * dx * dx + conk[None, :, 2] * dy * dy) - conk[None, :, 1] * dx * dy
    alpha_raw = ok_o[None, :] * torch.exp(power)
    alpha = mr.clamp_passthrough(alpha_raw, mr.C_AMAX)
    amb_pix = None
    if first:
        with torch.no_grad():
            tx, ty = torch.div(px, 16, rounding_mode="floor"), torch.div(py, 16, rounding_mode="floor")
            listed = (tx >= rect[None, :, 0]) & (tx < rect[None, :, 2]) & (ty >= rect[None, :, 1]) & (ty < rect[None, :, 3])
            D["ok"] = listed & (power <= 0.0) & (alpha >= mr.C_AMIN)
    ok = D["ok"]
    one_minus = torch.where(ok, 1.0 - alpha, torch.ones_like(alpha))
    T_incl = torch.cumprod(one_minus, dim=1)
    T_excl = T_incl / one_minus
    if first:
        with torch.no_grad():
            D["live"] = ok & (T_incl >= mr.C_TMIN)
            # the pixels in which a decision sits within fp32 rounding of its threshold (math_renderer.render's rules; the median
            # depth's crossing is not rendered here and decides nothing)
            sq = conk[None, :, 0].abs() * dx * dx + conk[None, :, 2].abs() * dy * dy + 2 * conk[None, :, 1].abs() * (dx * dy).abs()
            amb = listed & ((power.abs() <= fp32_eps * (1.0 + sq)) | ((power <= 0.0) & ((alpha_raw / mr.C_AMIN - 1.0).abs() <= 8 * fp32_eps * (1.0 + sq))))
            amb = amb | (ok & ((T_incl / mr.C_TMIN - 1.0).abs() <= 64 * fp32_eps))
            amb_pix = amb.any(dim=1).reshape(H, W).numpy()
    live = D["live"]
    w = torch.where(live, alpha * T_excl, torch.zeros_like(alpha))
    T_final = torch.where(live, one_minus, torch.ones_like(alpha)).prod(dim=1)
    colour = w @ colk + T_final[:, None] * torch.as_tensor(cfg["bg"]).to(dt)[None, :]
    return dict(color=colour.T.reshape(3, H, W), acc_depth=(w @ depk).reshape(H, W), alpha=(1.0 - T_final).reshape(H, W),
                per=(Ve, Pe, Ce), decisions=D, ambiguous=amb_pix, n_live=live.sum(dim=1).reshape(H, W).numpy(),
                clamped=((D["clx"] | D["cly"]) & D["vis"]).numpy(), vis=D["vis"].numpy())


def tensors(sc, names, dtype=torch.float64, grad=True):
    return {n: torch.as_tensor(np.asarray(sc[n], np.float64)).to(dtype).requires_grad_(grad) for n in names}


def upstream(c, cfg, amb, aux):
    """(g [3,H,W], gD [H,W] or None, gA [H,W] or None), float32, zero on the ambiguous pixels: the colour gradient is the one
    tests/test_gpu_independent.py uses, the aux ones are of the same size."""
    import scenes
    H, W = cfg["H"], cfg["W"]
    g = (scenes.upstream_grad(H, W, c["seed"] + 1) * (H * W)).astype(np.float32)
    g[:, amb] = 0.0
    gD = gA = None
    if aux:
        rng = np.random.default_rng(c["seed"] + 2)
        gD, gA = (rng.normal(size=(H, W)) * 0.25).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32)
        gD[amb] = 0.0; gA[amb] = 0.0
    return g, gD, gA


def loss_of(out, g, gD, gA):
    dt = out["color"].dtype
    L = (out["color"] * torch.as_tensor(g).to(dt)).sum()
    if gD is not None:
        L = L + (out["acc_depth"] * torch.as_tensor(gD).to(dt)).sum() + (out["alpha"] * torch.as_tensor(gA).to(dt)).sum()
    return L


CAMERA = ("viewmatrix", "projmatrix", "campos")


def evaluate(sc, cam, names, cfg, c, aux=False, dtype=torch.float64, decisions=None, upstream_grads=None, clamp_grad="reference", halve=None):
    """One forward + backward.  dict(out, want {viewmatrix, projmatrix, campos, + the leaves}: gradients as float64 numpy,
    terms {...}: the per-Gaussian contributions [P, ...], g / gD / gA, amb)."""
    t = tensors(sc, names, dtype)
    V, Pm, C = camera_leaves(cam, dtype)
    out = render(t, V, Pm, C, cfg, decisions=decisions, clamp_grad=clamp_grad, halve=halve)
    g, gD, gA = upstream_grads if upstream_grads is not None else upstream(c, cfg, out["ambiguous"], aux)
    loss_of(out, g, gD, gA).backward()
    z = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.double().numpy()      # noqa: E731
    want = dict(zip(CAMERA, (z(V), z(Pm), z(C))))
    want.update({n: z(t[n]) for n in names})
    terms = dict(zip(CAMERA, (z(e) for e in out["per"])))
    return dict(out=out, want=want, terms=terms, g=g, gD=gD, gA=gA, amb=out["ambiguous"])


def reference_pair(sc, cam, names, cfg, c, aux=False, halve=None):
    """(the fp64 evaluation, the float32 evaluation on the fp64 pass's decisions and upstream gradients)."""
    r64 = evaluate(sc, cam, names, cfg, c, aux=aux, halve=halve)
    sc32 = {n: np.asarray(sc[n], np.float32) for n in names}
    r32 = evaluate(sc32, cam, names, cfg, c, aux=aux, dtype=torch.float32, decisions=r64["out"]["decisions"],
                   upstream_grads=(r64["g"], r64["gD"], r64["gA"]), halve=halve)
    return r64, r32


# ---- the cases of tests/test_gpu_posegrad.py: case dicts of tests/test_gpu_independent.py by their first letter -------------------------
def raw_leaves(sc, seed):
    """Raw leaves + residuals of GaussianRasterizerRaw whose activations (scene/saro_gaussian.py:807-847, in fp64) replace the dense
    arrays of `sc` in place; returns the float32 raw dict."""
    rng = np.random.default_rng(seed + 11)
    P = sc["means3D"].shape[0]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    trbf = f32(rng.uniform(0.6, 1.0, size=(P, 1)))
    sig = np.clip(sc["opacities"].astype(np.float64) / trbf, 1e-4, 1 - 1e-4)
    raw = dict(xyz=f32(sc["means3D"]), motion_res=f32(rng.normal(0, 0.002, size=(P, 3))), rotation=f32(sc["rotations"]),
               rot_res=f32(rng.normal(0, 0.02, size=(P, 7))), scaling=f32(np.log(sc["scales"])), opacity_logit=f32(np.log(sig / (1 - sig))),
               trbf=trbf, features_dc=f32(sc["shs"][:, :1]), features_rest=f32(sc["shs"][:, 1:]), shs_res=f32(rng.normal(0, 0.02, size=sc["shs"].shape)))
    r = {n: v.astype(np.float64) for n, v in raw.items()}
    q = r["rotation"] + r["rot_res"][:, :4]
    sc["means3D"] = r["xyz"] + r["motion_res"]
    sc["rotations"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    sc["scales"] = np.exp(r["scaling"] + r["rot_res"][:, 4:])
    sc["opacities"] = trbf / (1.0 + np.exp(-r["opacity_logit"]))
    sc["shs"] = np.concatenate([r["features_dc"], r["features_rest"]], 1) + r["shs_res"]
    return raw


VARIANTS = dict(a=dict(aux=True), d=dict(), e=dict(aa=True), b=dict(raw=True))


@functools.lru_cache(maxsize=None)
def _reference(letter, halve):
    import scenes
    import test_gpu_independent as tgi
    c = next(k for k in tgi.CASES if k["name"].startswith(letter + "_"))
    v = VARIANTS[letter]
    sc, cam, names = tgi._case_inputs(scenes, c)
    raw = raw_leaves(sc, c["seed"]) if v.get("raw") else None
    cfg = cfg_of(cam, sc, c, aa=v.get("aa", False))
    r64, r32 = reference_pair(sc, cam, names, cfg, c, aux=v.get("aux", False), halve=halve)
    return dict(v, c=c, sc=sc, cam=cam, names=names, cfg=cfg, raw=raw, r64=r64, r32=r32)      # (raw: the raw leaves, or None)


def reference(letter, halve=None):
    """The fp64 / fp32 references of one case, computed once per process and shared: do not modify them."""
    return _reference(letter, halve)


# ---- a camera from a 6-vector, as scene/cameras.py composes it ----------------------------------------------------------------------------
def compose(xi, V0, proj):
    """xi [6] = (axis-angle, translation): viewmatrix = V0 @ [[R(xi[:3]), 0], [xi[3:], 1]] (row-vector storage: a rigid motion applied in
    view space), projmatrix = viewmatrix @ proj, campos = inverse(viewmatrix)[3, :3] -- scene/cameras.py's full_proj_transform and
    camera_center.  Any dtype / device (those of xi)."""
    w = xi[:3]
    th = torch.sqrt((w * w).sum() + 1e-24)
    k = w / th
    zero = torch.zeros_like(th)
    K = torch.stack([zero, -k[2], k[1], k[2], zero, -k[0], -k[1], k[0], zero]).reshape(3, 3)
    R = torch.eye(3, dtype=xi.dtype, device=xi.device) + torch.sin(th) * K + (1.0 - torch.cos(th)) * (K @ K)
    top = torch.cat([R, torch.zeros((3, 1), dtype=xi.dtype, device=xi.device)], dim=1)
    bot = torch.cat([xi[3:], torch.ones(1, dtype=xi.dtype, device=xi.device)])[None, :]
    V = V0 @ torch.cat([top, bot], dim=0)
    return V, V @ proj, torch.linalg.inv(V)[3, :3]
