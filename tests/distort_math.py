"""The depth-distortion map (`distortion=True`; include/gsrast.h: gsrast_distortion_forward / _backward) in torch -- a helper of the
tests, not a test.

    distort[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_i w_i (z_i A_{i-1} - D_{i-1})      over the pairs the forward blends at p

float64 (`evaluate64`): math_renderer.project + math_renderer.blend_pairs (the projection and the pair loop of mr.render, whose colour
tests/test_distort_host.py compares), on their weights the distortion by cumulative sums along the depth order, the gradients of
    sum distort gd + sum color g0 [+ sum acc_depth gD + sum alpha gA]
by autograd (the screen-space mean's through project()'s ndc_offset).  Anti-aliasing: the opacity is o * comp (tests/aa_math.py).  Raw
path: features_math.activate in front of it, gradients with respect to the raw leaves (features_math.raw_arrays).

float32 (`restate32`): the same two functions in float32 on the discrete decisions of their own float64 pass (math_renderer's decisions
contract) with the KERNEL'S association: depths relative to z0, the depth of the first Gaussian listed for the pixel's tile.  What fp32
rounding alone does: the measure of the map's bar and the floor of conftest.grad_tol.  The camera tensors are leaves there, so
`camera_reference` gives the camera's gradients of a distortion-only loss as well.

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
    """math_renderer.blend_pairs + the distortion by cumulative sums along the depth order (z0_relative: in the kernel's association).
    dict(color [3,H,W], acc_depth, alpha, distort [H,W], w [N,K], live, decisions)."""
    bl = mr.blend_pairs(dict(pix=pix, conic=conic, o=o, z=z, col=col, rect=rect), bg, W, H, decisions=D, z0_relative=z0_relative)
    w, zr = bl["w"], bl["z_rel"]
    zero = torch.zeros_like(w[:, :1])
    A_prev = torch.cat([zero, torch.cumsum(w, dim=1)[:, :-1]], dim=1)
    D_prev = torch.cat([zero, torch.cumsum(w * zr, dim=1)[:, :-1]], dim=1)
    distort = 2.0 * (w * (zr * A_prev - D_prev)).sum(dim=1)
    # acc_depth is formed again here, after the sums: autograd adds w's gradient terms in reverse order of creation, and so in the same order as ever
    return dict(color=bl["color"], acc_depth=(w @ z).reshape(H, W), alpha=bl["alpha"], distort=distort.reshape(H, W), w=w, live=bl["live"],
                decisions=bl["decisions"])


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
    """The float64 pass: (leaves, the means2D sink, math_renderer.render's result, blend()'s result)."""
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
    g = mr.project(d["means3D"], d["scales"], d["rotations"], cam, ndc_offset=off, deg=deg, opacities=o, shs=d["shs"])["sorted"]
    out = blend(g["pix"], g["conic"], g["o"], g["z"], g["col"], sc["bg"], g["rect"], ref["proj"]["W"], ref["proj"]["H"])
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
    """math_renderer.project_gaussians' visible Gaussians in depth order (camera tensors as given; `off`: the means2D sink), on the decisions D
    (empty: filled here)."""
    pr = mr.project_gaussians(t, V, Pm, Cp, cfg, ndc_offset=off, decisions=D if "idx" in D else None)
    D.update(pr["decisions"])
    return pr["sorted"]


def _run(sc, cam, dtype, D, g, aa, raw, aux, colour_loss, camera=False, z0_relative=True):
    """One pass with the camera as leaves in `dtype` on the decisions D (None: decide).  (decisions, map, grads, camera grads)."""
    leaves, d = fm._leaves(sc, raw, dtype)
    V, Pm, Cp = pm.camera_leaves(cam, dtype)
    cfg = pm.cfg_of(cam, sc, aa=aa)
    off = torch.zeros((d["means3D"].shape[0], 2), dtype=dtype, requires_grad=True)
    D = {} if D is None else D
    pr = project(d, V, Pm, Cp, cfg, D, off)
    out = blend(pr["pix"], pr["conic"], pr["o"], pr["z"], pr["col"], cfg["bg"], pr["rect"], cfg["W"], cfg["H"], D if "live" in D else None, z0_relative=z0_relative)
    D.update(out["decisions"])
    if g is None:
        return D, out, None, None
    _loss(out, g, dtype, colour_loss, aux).backward()
    return D, out, fm._grads(leaves, dict(means2D=off)), (dict(viewmatrix=mr.grad64(V), projmatrix=mr.grad64(Pm), campos=mr.grad64(Cp)) if camera else None)


def restate32(sc, cam, g, aa=False, raw=False, aux=False, colour_loss=True):
    """The float32 evaluation on its own float64 pass's decisions, z0-relative.  dict(map [H,W] float64 numpy, grads {leaf, "means2D"})."""
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
