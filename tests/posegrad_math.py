"""The renderer with the CAMERA as differentiable input, in torch -- a helper of the tests, not a test.

tests/math_renderer.py's render() turns viewmatrix / projmatrix / campos into constants through numpy; here they are three leaf tensors
(include/gsrast.h: GSRAST_RENDER_POSEGRAD treats them as three independent inputs) given to the same two functions
(math_renderer.project_gaussians, blend_pairs), and autograd gives their gradients.  The conventions are math_renderer's (its docstring): row-vector matrices stored transposed, t = [mean, 1] @ viewmatrix,
hom = [mean, 1] @ projmatrix; the 0.99 alpha clamp straight-through; no gradient through the median depth (not rendered here); a
frustum-clamped t.x / t.y a constant inside J (clamp_grad="reference"; "true" differentiates the clamp as written);
det^2 / (det^2 + 1e-7) in the conic chain; dL/dscales with respect to scale_modifier * scales.  tanfovx / tanfovy are constants.
No tile lists, no hand-written gradient, nothing shared with csrc/ or oracle/.

Per-Gaussian contributions: every Gaussian gets its OWN copy of the three camera tensors ([P,4,4], [P,4,4], [P,3], `per` in the result);
after a backward their .grad rows are the Gaussians' terms of the three sums -- what the tests need to assert non-vacuity and to form
sum_i |term_i|.

fp32: render(..., decisions=<the fp64 pass's>) evaluates the same expressions in the dtype of its inputs on the discrete decisions of the
fp64 pass (math_renderer's decisions contract) -- the `ref32` of conftest.grad_tol: what fp32 rounding alone does to these sums.

halve: "JW" multiplies the gradient that reaches viewmatrix through the rotation inside T = J W by 0.5 -- a wrong reference on purpose,
for the test that shows the bar biting."""
import functools

import numpy as np
import torch

import math_renderer as mr


def cfg_of(cam, sc, c=None, aa=False):
    """The constants of a render: sizes, focal tangents, background, SH degree, scale_modifier, anti-aliasing."""
    return mr.camera_cfg(cam, bg=np.asarray(sc["bg"], np.float64), deg=int(c["deg"]) if c is not None else int(sc.get("sh_degree", 0)),
                         scale_modifier=float(cam.get("scale_modifier", 1.0)), aa=bool(aa))


def camera_leaves(cam, dtype=torch.float64):
    """(viewmatrix [4,4], projmatrix [4,4], campos [3]) as leaves that require grad."""
    return tuple(torch.as_tensor(np.asarray(cam[k], np.float64)).to(dtype).requires_grad_(True) for k in ("viewmatrix", "projmatrix", "campos"))


def render(t, V, Pm, C, cfg, decisions=None, clamp_grad="reference", halve=None, fp32_eps=4e-6, per=True):
    """t: dict of tensors -- means3D [P,3], opacities [P,1] and (shs [P,M,3], scales, rotations) or (rgb [P,3], cov3D [P,6]).
    Returns dict(color [3,H,W], acc_depth [H,W], alpha [H,W], per=(Ve, Pe, Ce) or None, decisions, ambiguous [H,W], n_live, clamped [P], vis [P])."""
    W, H = cfg["W"], cfg["H"]
    pr = mr.project_gaussians(t, V, Pm, C, cfg, clamp_grad=clamp_grad, per=per, halve=halve, decisions=decisions)
    bl = mr.blend_pairs(pr["sorted"], cfg["bg"], W, H, decisions=decisions, fp32_eps=fp32_eps)
    D = {**pr["decisions"], **bl["decisions"]} if decisions is None else decisions
    return dict(color=bl["color"], acc_depth=bl["acc_depth"], alpha=bl["alpha"], per=pr["per"], decisions=D,
                ambiguous=None if decisions is not None else bl["ambiguous"].reshape(H, W).numpy(), w=bl["w"], live=bl["live"],
                n_live=bl["live"].sum(dim=1).reshape(H, W).numpy(), clamped=((D["clx"] | D["cly"]) & D["vis"]).numpy(), vis=D["vis"].numpy())


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
    want = dict(zip(CAMERA, (mr.grad64(V), mr.grad64(Pm), mr.grad64(C))))
    want.update({n: mr.grad64(t[n]) for n in names})
    terms = dict(zip(CAMERA, (mr.grad64(e) for e in out["per"])))
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
