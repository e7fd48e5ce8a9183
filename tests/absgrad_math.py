"""The absolute screen-space gradient (include/gsrast.h: GSRAST_RENDER_ABSGRAD) in torch fp64 -- a helper of the tests, not a test.

AbsGS's statistic for Gaussian i is  sum over pixels p of |d L_p / d mean2D_i|, where L_p is the part of the loss pixel p carries:
L_p = sum_c g[c, p] colour[c, p]  (+ gD[p] acc_depth[p] + gA[p] alpha[p] with the aux outputs).  It is built here on
tests/math_renderer.py as it stands: `ndc_offset`, the sink math_renderer.render has for the projected centre, is differentiated once per
pixel (a loop over the pixels: per_pixel_grads says why not batched grad_outputs), and the absolute values are summed.  The units
are those of means2D.grad (the reference's normalised device coordinates).  acc_depth is the colour of a (z, 0, 0) render on black and
alpha = 1 - final_T, as the reference of tests/test_gpu_render_aux.py builds them.

Self-check, on every call: the SIGNED sum over the pixels is the ordinary gradient of the whole loss, to 1e-12 of its largest entry
(plus the fp64 rounding of the sum itself, which is all that is left where the signed sum cancels).

CASES are the shapes of tests/test_gpu_absgrad.py (the smallest at which blend_bwd_cull_t_kernel<.., ABS> can still go wrong); the seeds
were picked on the CPU so that the share of fp32-ambiguous pixels stays under the 5 % cap of tests/test_gpu_independent.py."""
import functools

import numpy as np
import torch

import aa_math
import math_renderer as mr
from math_renderer import t64

CASES = dict(
    # four tiles, all four 8 x 8 blocks of each
    a=dict(P=96, seed=3, W=32, H=32, k=1, V=5, smul=1.0, omul=0.8, bg=(0.1, 0.2, 0.3)),
    # ragged right and bottom tiles: lanes outside the image
    b=dict(P=96, seed=5, W=40, H=24, k=2, V=5, smul=1.0, omul=0.8, bg=(1.0, 1.0, 1.0)),
    # one tile, 200 Gaussians in it at moderate opacity: every pixel walks a list of more than 128 entries -- the 64-instance batch
    # boundary twice, partly-alive groups of eight
    c=dict(P=200, seed=7, W=16, H=16, k=0, V=3, smul=0.5, omul=0.12, bg=(0.0, 0.0, 0.0), spread=0.45, long=True),
)
CASES["d"] = dict(CASES["a"], aux=True)
CASES["e"] = dict(CASES["a"], aa=True)
CASES["f"] = dict(CASES["a"], raw=True)


def case_scene(scenes, c):
    """(scene, camera) of a case: float32 arrays, the inputs of both sides.  raw: sc["raw"] holds the raw leaves and residuals of
    GaussianRasterizerRaw, and the dense arrays are their activations (scene/saro_gaussian.py:807-847) in fp64."""
    sc = scenes.synth(c["P"], c["seed"], scale_mul=c["smul"])
    if "spread" in c:      # every centre near the optical axis: one tile holds them all
        sc["means3D"] = (sc["means3D"] * c["spread"]).astype(np.float32)
    sc["bg"] = np.array(c["bg"], np.float32)
    sc["opacities"] = (sc["opacities"] * c["omul"]).astype(np.float32)
    cam = scenes.camera(c["k"], c["V"], c["W"], c["H"])
    if c.get("raw"):
        rng = np.random.default_rng(c["seed"] + 11)
        P = c["P"]
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
        trbf = f32(rng.uniform(0.6, 1.0, size=(P, 1)))
        sig = np.clip(sc["opacities"].astype(np.float64) / trbf, 1e-4, 1 - 1e-4)
        raw = dict(xyz=f32(sc["means3D"]), motion_res=f32(rng.normal(0, 0.02, size=(P, 3))), rotation=f32(sc["rotations"]),
                   rot_res=f32(rng.normal(0, 0.05, size=(P, 7))), scaling=f32(np.log(sc["scales"])), opacity_logit=f32(np.log(sig / (1 - sig))),
                   trbf=trbf, features_dc=f32(sc["shs"][:, :1]), features_rest=f32(sc["shs"][:, 1:]), shs_res=f32(rng.normal(0, 0.05, size=sc["shs"].shape)))
        r = {n: v.astype(np.float64) for n, v in raw.items()}
        q = r["rotation"] + r["rot_res"][:, :4]
        sc["means3D"] = r["xyz"] + r["motion_res"]
        sc["rotations"] = q / np.linalg.norm(q, axis=1, keepdims=True)
        sc["scales"] = np.exp(r["scaling"] + r["rot_res"][:, 4:])
        sc["opacities"] = trbf / (1.0 + np.exp(-r["opacity_logit"]))
        sc["shs"] = np.concatenate([r["features_dc"], r["features_rest"]], 1) + r["shs_res"]
        sc["raw"] = raw
    return sc, cam


def upstream(c, amb):
    """The case's upstream gradients (g [3,H,W], gD [H,W] or None, gA [H,W] or None), float32, zero on the ambiguous pixels."""
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(c["seed"] + 1)
    g = rng.normal(size=(3, H, W)).astype(np.float32)
    g[:, amb] = 0.0
    gD = gA = None
    if c.get("aux"):
        gD = rng.normal(size=(H, W)).astype(np.float32); gA = rng.normal(size=(H, W)).astype(np.float32)
        gD[amb] = 0.0; gA[amb] = 0.0
    return g, gD, gA


def per_pixel_grads(Lp, off):
    """d Lp[p] / d off for every pixel p: [N, P, 2], one backward per pixel.  (autograd's batched grad_outputs give the same numbers --
    vmap has a rule for every op of math_renderer.render's graph -- but take twice as long on these shapes: 5.2 s against 2.9 s for the
    1024 pixels of case a, the batched intermediates being [chunk, N, K].)"""
    return torch.stack([torch.autograd.grad(Lp[p], off, retain_graph=True)[0] for p in range(Lp.numel())])


def absgrad_of(sc, cam, c, upstream_fn=upstream):
    """dict(abs [P,2], signed [P,2], out = math_renderer.render's result, amb [H,W], g, gD, gA): the statistic of one case.
    upstream_fn(c, amb) -> (g, gD, gA)."""
    P, W, H = sc["means3D"].shape[0], c["W"], c["H"]
    m, s, q, sh = t64(sc["means3D"]), t64(sc["scales"]), t64(sc["rotations"]), t64(sc["shs"])
    o = t64(sc["opacities"])
    deg = int(sc.get("sh_degree", 3))
    if c.get("aa"):      # the anti-aliased render is the plain one at o * comp (tests/aa_math.py)
        vis = mr.project(m, s, q, cam)["disc"]["vis"]
        idx = torch.as_tensor(vis).nonzero()[:, 0]
        comp, _ = aa_math.comp(m[idx], s[idx], q[idx], cam, clamp_grad="reference")
        o = o[:, 0].index_put((idx,), o[idx, 0] * comp.detach())[:, None]
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    out = mr.render(m, s, q, o, sh, deg, cam, sc["bg"], ndc_offset=off, clamp_grad="reference")
    amb = out["ambiguous"].copy()
    outd = None
    if c.get("aux"):
        V = t64(cam["viewmatrix"])
        z = m @ V[:3, 2] + V[3, 2]
        outd = mr.render(m, s, q, o, sh, deg, cam, np.zeros(3), colors_precomp=torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1),
                         ndc_offset=off, clamp_grad="reference")
        amb |= outd["ambiguous"]
    g, gD, gA = upstream_fn(c, amb)
    Lp = (out["color"] * t64(g)).sum(dim=0)
    if c.get("aux"):
        Lp = Lp + outd["color"][0] * t64(gD) + (1.0 - out["final_T"]) * t64(gA)
    Lp = Lp.reshape(-1)
    per = per_pixel_grads(Lp, off)
    signed = per.sum(dim=0)
    whole = torch.autograd.grad(Lp.sum(), off)[0]
    absg = per.abs().sum(dim=0)
    # 1e-12 of the gradient's largest entry, and never below what summing N terms in fp64 leaves of their absolute sum (sqrt(N) eps: all
    # there is to compare with where the signed sum cancels to nothing)
    bar = 1e-12 * float(whole.abs().max()) + np.sqrt(Lp.numel()) * np.finfo(np.float64).eps * float(absg.max())
    assert float(absg.max()) > 0.0 and float((signed - whole).abs().max()) <= bar, "the per-pixel gradients do not add up to the loss's"
    return dict(abs=absg.numpy(), signed=whole.numpy(), out=out, amb=amb, g=g, gD=gD, gA=gA)


@functools.lru_cache(maxsize=None)
def _reference(name):
    import scenes
    c = CASES[name]
    sc, cam = case_scene(scenes, c)
    r = absgrad_of(sc, cam, c)
    r.update(sc=sc, cam=cam, c=c)
    return r


def reference(name):
    """The fp64 reference of CASES[name], computed once per process and shared: do not modify it."""
    return _reference(name)
