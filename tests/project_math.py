"""The stand-alone projection (fused_project.project_gaussians; include/gsrast.h: gsrast_project_forward / _backward) in torch -- a helper
of the tests, not a test.

float64: math_renderer.project_gaussians at its defaults (clamp_grad="reference", the conic's det^2 / (det^2 + 1e-7), dL/dscales as of
scale_modifier * scales), deciding.  The compensation is the helper's `o` with opacities = 1 and aa = True.  Rows the projection culls
(`vis` of its decisions: view z <= 0.2, det == 0, no tile touched) read zero in every output, so they receive no gradient.
float32 (`ref32`): the same function in float32 on the float64 pass's decisions -- what fp32 rounding alone does; the floor of
conftest.grad_tol.  Gradients: of  sum_k <output_k, upstream_k>  over the four float outputs with one seeded upstream each (`upstream`).

Scenes (SCENES): the six edge_scenes.CASES (needles, near-plane rows, 30-34 frustum-clamped rows, a cov3D case, scale_modifier 0.7) and
contrib_math.CASES a and b (b: 1726 of 2000 rows culled)."""
import functools

import numpy as np
import torch

import contrib_math
import edge_scenes
import math_renderer as mr
from math_renderer import t64

OUTPUTS = ("means2D", "depths", "conics", "compensation")
SCENES = tuple(c["name"] for c in edge_scenes.CASES) + ("contrib_a", "contrib_b")


def scene(name):
    """(sc, cam, leaves): float32 arrays, cam["scale_modifier"] set, leaves = the names of the differentiable inputs."""
    import scenes
    if name.startswith("contrib_"):
        sc, cam = contrib_math.case_scene(scenes, contrib_math.CASES[name[len("contrib_"):]])
        cam["scale_modifier"] = 1.0
        return sc, cam, ("means3D", "scales", "rotations")
    c = next(c for c in edge_scenes.CASES if c["name"] == name)
    sc, cam, _ = edge_scenes.case_inputs(scenes, c)
    return sc, cam, ("means3D", "cov3D") if c.get("precomp") else ("means3D", "scales", "rotations")


UP_FLOOR = dict(means2D=1.0, depths=0.2, conics=1e-6, compensation=0.005)


def upstream(values, seed=31):
    """One float32 upstream gradient per float output: N(0, 1) over the size of the row's own value (its largest component; at least
    UP_FLOOR: a pixel, the near plane, the compensation's floor), i.e. the gradient of  sum n log|output|.  Every output of every row then
    weighs alike in the gradients, whatever its unit: with a plain N(0, 1) the pixel centres' term (tens of pixels per unit of depth) buries
    the conic's and the compensation's (1e-3 for the large footprints at the image's border), and with them what the conventions decide."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in OUTPUTS:
        v = np.abs(values[k])
        size = np.maximum(v if v.ndim == 1 else v.max(axis=1, keepdims=True), UP_FLOOR[k])
        out[k] = (rng.normal(size=v.shape) / size).astype(np.float32)
    return out


def evaluate(sc, cam, leaves, up, dtype=torch.float64, decisions=None, clamp_grad="reference"):
    """One forward + backward in `dtype`.  dict(values {output: float64 numpy, culled rows zero}, grads {leaf: float64 numpy}, disc (deciding
    pass only), decisions, vis bool numpy)."""
    P = sc["means3D"].shape[0]
    x = {n: t64(sc[n]).to(dtype).requires_grad_(True) for n in leaves}
    t = dict(x, opacities=torch.ones((P, 1), dtype=dtype))
    cfg = mr.camera_cfg(cam, scale_modifier=float(cam.get("scale_modifier", 1.0)), aa=True)
    pr = mr.project_gaussians(t, t64(cam["viewmatrix"]).to(dtype), t64(cam["projmatrix"]).to(dtype), None, cfg, clamp_grad=clamp_grad,
                              decisions=decisions)
    vis = pr["decisions"]["vis"]
    raw = dict(means2D=pr["pix"], depths=pr["depth"], conics=pr["conic"], compensation=pr["o"])
    vals = {k: torch.where(vis.reshape((P,) + (1,) * (v.dim() - 1)), v, torch.zeros_like(v)) for k, v in raw.items()}
    loss = sum((vals[k] * torch.as_tensor(up[k]).to(dtype)).sum() for k in OUTPUTS)
    loss.backward()
    grads = {n: mr.grad64(v) for n, v in x.items()}
    assert all(np.isfinite(g).all() for g in grads.values())
    return dict(values={k: v.detach().double().numpy() for k, v in vals.items()}, grads=grads, disc=pr["disc"], decisions=pr["decisions"],
                vis=vis.numpy())


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(sc, cam, leaves, up, r64, r32, true64, true32) of one scene, computed once per process and shared: do not modify it.  r64 / r32: evaluate()
    in float64 (deciding) and float32 (on its decisions); true64 / true32: the same pair with clamp_grad="true" (the forward expression
    differentiated as written: another convention on the frustum-clamped rows, the same values)."""
    sc, cam, leaves = scene(name)
    zero = {k: np.zeros(s, np.float32) for k, s in zip(OUTPUTS, ((len(sc["means3D"]), 2), (len(sc["means3D"]),), (len(sc["means3D"]), 3), (len(sc["means3D"]),)))}
    up = upstream(evaluate(sc, cam, leaves, zero)["values"])
    r64 = evaluate(sc, cam, leaves, up)
    r32 = evaluate(sc, cam, leaves, up, torch.float32, r64["decisions"])
    true64 = evaluate(sc, cam, leaves, up, clamp_grad="true")
    true32 = evaluate(sc, cam, leaves, up, torch.float32, true64["decisions"], clamp_grad="true")
    return dict(sc=sc, cam=cam, leaves=leaves, up=up, r64=r64, r32=r32, true64=true64, true32=true32)


def radius_firm(disc):
    """bool [P]: rows whose integer radius and tile rectangle do not sit within fp32 rounding of flipping."""
    return ~((disc["radius_margin"] < 1e-4 * np.maximum(disc["radius"], 1)) | (disc["rect_margin"] < 1e-5))


# ---- end to end: two projections -> screen flow -> rendered as features -> L1 against a target map --------------------------------------
FLOW_SHIFT = (0.03, -0.02, 0.04)      # the rigid shift between the two sets of means3D


def _flow_chain(sc, cam, target, keep, dtype, decisions=None):
    """means3D (set 0, also what is rendered) and means3D + FLOW_SHIFT (set 1) -> flow = pix1 - pix0 where both are visible, 0 elsewhere ->
    feature map (math_renderer's colour of [flow, 0], black background) -> sum keep |map - target|.  target None: forward only."""
    import posegrad_math as pm
    f = lambda a, g=False: t64(a).to(dtype).requires_grad_(g)      # noqa: E731
    m0, m1 = f(sc["means3D"], True), f(sc["means3D"].astype(np.float64) + np.asarray(FLOW_SHIFT), True)
    s, q, o = f(sc["scales"]), f(sc["rotations"]), f(sc["opacities"])
    V, Pm = f(cam["viewmatrix"]), f(cam["projmatrix"])
    cfg = dict(pm.cfg_of(cam, sc), bg=np.zeros(3))
    D = decisions or {}
    pr = [mr.project_gaussians(dict(means3D=m, scales=s, rotations=q), V, Pm, None, cfg, decisions=D.get(k)) for k, m in (("p0", m0), ("p1", m1))]
    valid = pr[0]["decisions"]["vis"] & pr[1]["decisions"]["vis"]
    d = pr[1]["pix"] - pr[0]["pix"]
    flow = torch.where(valid[:, None], d, torch.zeros_like(d))
    out = pm.render(dict(means3D=m0, opacities=o, scales=s, rotations=q, rgb=torch.cat([flow, torch.zeros_like(flow[:, :1])], dim=1)), V, Pm, None, cfg,
                    decisions=D.get("r"), per=False)
    fmap = out["color"][:2]
    if target is not None:
        ((fmap - t64(target).to(dtype)).abs() * torch.as_tensor(keep).to(dtype)).sum().backward()
    return dict(map=fmap.detach().double().numpy(), flow=flow.detach().double().numpy(), valid=valid.numpy(), ambiguous=out["ambiguous"],
                grads=dict(m0=mr.grad64(m0), m1=mr.grad64(m1)), decisions=dict(p0=pr[0]["decisions"], p1=pr[1]["decisions"], r=out["decisions"]))


@functools.lru_cache(maxsize=None)
def flow_reference(name="contrib_a"):
    """dict(sc, cam, target [2,H,W], keep [H,W] float32, r64, r32) of the end-to-end chain.  target: a seeded N(0, 2 px) map; keep: 1 on the
    pixels that are fp32-unambiguous in the render AND more than 1e-3 px from the L1 kink in both channels, 0 elsewhere."""
    sc, cam, _ = scene(name)
    fwd = _flow_chain(sc, cam, None, None, torch.float64)
    target = (2.0 * np.random.default_rng(41).normal(size=fwd["map"].shape)).astype(np.float32)
    keep = (~fwd["ambiguous"] & (np.abs(fwd["map"] - target).min(axis=0) > 1e-3)).astype(np.float32)
    r64 = _flow_chain(sc, cam, target, keep, torch.float64)
    r32 = _flow_chain(sc, cam, target, keep, torch.float32, r64["decisions"])
    return dict(sc=sc, cam=cam, target=target, keep=keep, r64=r64, r32=r32)
