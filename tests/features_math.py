"""Per-Gaussian feature vectors through the blend (`features=F`; include/gsrast.h: gsrast_features_forward / _backward) in torch -- a helper
of the tests, not a test.

float64: tests/math_renderer.py as it stands.  render() is linear in colors_precomp, so C channels are ceil(C / 3) calls
mr.render(..., colors_precomp=F[:, 3k:3k+3] zero-padded, bg=0); gradients of  sum feature_map g1 + sum color g0  come from autograd (the
screen-space mean's through render()'s ndc_offset).  Anti-aliasing: the opacity is o * comp (tests/aa_math.py, differentiable).  Raw path:
the activations of GaussianRasterizerRaw (means3D = xyz, rotations = normalize(rotation), scales = exp(scaling), opacities =
sigmoid(opacity), shs = cat(features_dc, features_rest)) in front of it, gradients with respect to the raw leaves.

float32 (`restate32`): the same function -- math_renderer.project_gaussians / blend_pairs, through tests/posegrad_math.render -- in float32
on the discrete decisions of its own float64 pass (math_renderer's decisions contract) -- what fp32 rounding alone does; the floor of conftest.grad_tol and the measure of
the map's bar.  Its gradient of the screen-space mean: posegrad_math gives every Gaussian its own copy of projmatrix, hom = [mean, 1] @
copy, so the copy's gradient row 3 is dL/dhom, and dL/dndc.xy = dL/dhom.xy / p_w -- what an offset added to ndc.xy (means2D) receives.

Cases: contrib_math.CASES / case_scene (70 x 45, 5 x 3 ragged tiles).  The upstream gradients are zero on the fp64 render's
fp32-ambiguous pixels."""
import functools

import numpy as np
import torch

import aa_math
import contrib_math as cm
import math_renderer as mr
import posegrad_math as pm

DENSE = ("means3D", "opacities", "scales", "rotations", "shs")
RAW = ("xyz", "opacity", "scaling", "rotation", "features_dc", "features_rest")
CHANNELS = (1, 3, 19, 64)


def features_of(P, C, seed=17):
    """[P, C] float32: per-Gaussian vectors of order one, both signs."""
    return np.random.default_rng(seed + 100 * C).normal(size=(P, C)).astype(np.float32)


def upstream(C, H, W, amb, seed=23):
    """(g1 [C,H,W] for the map, g0 [3,H,W] for the colour), float32, zero on the ambiguous pixels."""
    rng = np.random.default_rng(seed + C)
    g1, g0 = rng.normal(size=(C, H, W)).astype(np.float32), rng.normal(size=(3, H, W)).astype(np.float32)
    g1[:, amb] = 0.0
    g0[:, amb] = 0.0
    return g1, g0


def raw_arrays(sc):
    """float32 raw leaves whose activations are (up to their own rounding) the scene's dense arrays."""
    sig = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1 - 1e-6)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    return dict(xyz=f32(sc["means3D"]), rotation=f32(sc["rotations"]), scaling=f32(np.log(sc["scales"].astype(np.float64))), opacity=f32(np.log(sig / (1 - sig))),
                features_dc=f32(sc["shs"][:, :1]), features_rest=f32(sc["shs"][:, 1:]))


def activate(l):
    """The dense inputs of raw leaves (scene/saro_gaussian.py:807-847 without residuals), any dtype."""
    q = l["rotation"]
    return dict(means3D=l["xyz"], rotations=q / torch.linalg.norm(q, dim=1, keepdim=True), scales=torch.exp(l["scaling"]),
                opacities=torch.sigmoid(l["opacity"]), shs=torch.cat([l["features_dc"], l["features_rest"]], dim=1))


def _leaves(sc, raw, dtype):
    src = raw_arrays(sc) if raw else {n: sc[n] for n in DENSE}
    leaves = {n: torch.as_tensor(np.asarray(v, np.float64)).to(dtype).requires_grad_(True) for n, v in src.items()}
    return leaves, (activate(leaves) if raw else leaves)


def _triples(F):
    """F [P, C] -> the ceil(C / 3) zero-padded [P, 3] slices and the number of real channels of each."""
    P, C = F.shape
    out = []
    for k in range(0, C, 3):
        n = min(3, C - k)
        out.append((k, n, torch.cat([F[:, k:k + n], torch.zeros((P, 3 - n), dtype=F.dtype)], dim=1) if n < 3 else F[:, k:k + 3]))
    return out


def _grads(leaves, extra):
    return {n: mr.grad64(x) for n, x in {**leaves, **extra}.items()}


def evaluate64(sc, cam, F, aa=False, raw=False, colour_loss=True, feature_loss=True, g=None):
    """One float64 forward + backward.  dict(map [C,H,W], color [3,H,W], amb [H,W], g1, g0, grads {leaf, "features", "means2D"}, vis)."""
    leaves, d = _leaves(sc, raw, torch.float64)
    P, C = F.shape
    Ft = torch.as_tensor(np.asarray(F, np.float64)).requires_grad_(True)
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    o = d["opacities"]
    if aa:
        comp, _ = aa_math.comp(d["means3D"], d["scales"], d["rotations"], cam)
        o = o * comp[:, None]
    H, W = int(cam["image_height"]), int(cam["image_width"])
    col = mr.render(d["means3D"], d["scales"], d["rotations"], o, d["shs"], int(sc.get("sh_degree", 3)), cam, sc["bg"], ndc_offset=off)
    amb = col["ambiguous"]
    g1, g0 = g if g is not None else upstream(C, H, W, amb)
    loss = (col["color"] * torch.as_tensor(g0, dtype=torch.float64)).sum() if colour_loss else torch.zeros((), dtype=torch.float64)
    fmap = torch.zeros((C, H, W), dtype=torch.float64)
    g1t = torch.as_tensor(g1, dtype=torch.float64)
    for k, n, Fk in _triples(Ft):
        outk = mr.render(d["means3D"], d["scales"], d["rotations"], o, None, 0, cam, np.zeros(3), colors_precomp=Fk, ndc_offset=off)
        fmap[k:k + n] = outk["color"][:n].detach()
        if feature_loss:
            loss = loss + (outk["color"][:n] * g1t[k:k + n]).sum()
    if loss.requires_grad:
        loss.backward()
    return dict(map=fmap.numpy(), color=col["color"].detach().numpy(), amb=amb, g1=g1, g0=g0, grads=_grads(leaves, dict(features=Ft, means2D=off)),
                vis=col["proj"]["disc"]["vis"], final_T=col["final_T"].detach().numpy(), n_live=col["n_live"])


def restate32(sc, cam, F, g1, g0, aa=False, raw=False, colour_loss=True, feature_loss=True):
    """The float32 evaluation on its own float64 pass's decisions.  dict(map [C,H,W] float64 numpy, grads {leaf, "features"})."""
    def run(dtype, decisions, grad):
        leaves, d = _leaves(sc, raw, dtype)
        Ft = torch.as_tensor(np.asarray(F, np.float64)).to(dtype).requires_grad_(True)
        V, Pm, Cp = pm.camera_leaves(cam, dtype)
        pers = []
        cfg = pm.cfg_of(cam, sc, aa=aa)
        cfg0 = dict(cfg, bg=np.zeros(3))
        base = dict(means3D=d["means3D"], opacities=d["opacities"], scales=d["scales"], rotations=d["rotations"])
        col = pm.render(dict(base, shs=d["shs"]), V, Pm, Cp, cfg, decisions=decisions)
        D = col["decisions"]
        if not grad:
            return D, None, None
        pers.append(col["per"][1])
        C, (H, W) = F.shape[1], (cfg["H"], cfg["W"])
        loss = (col["color"] * torch.as_tensor(g0).to(dtype)).sum() if colour_loss else torch.zeros((), dtype=dtype)
        fmap = np.zeros((C, H, W))
        for k, n, Fk in _triples(Ft):
            outk = pm.render(dict(base, rgb=Fk), V, Pm, Cp, cfg0, decisions=D)
            fmap[k:k + n] = outk["color"][:n].detach().double().numpy()
            pers.append(outk["per"][1])
            if feature_loss:
                loss = loss + (outk["color"][:n] * torch.as_tensor(g1[k:k + n]).to(dtype)).sum()
        if loss.requires_grad:
            loss.backward()
        grads = _grads(leaves, dict(features=Ft))
        with torch.no_grad():
            m = d["means3D"].detach().double()
            hw = (torch.cat([m, torch.ones_like(m[:, :1])], dim=1) @ Pm.detach().double())[:, 3] + mr.C_WEPS      # 1 / p_w
            dhom = sum(e.grad[:, 3, :2].double() for e in pers if e.grad is not None)
            grads["means2D"] = (dhom * hw[:, None]).numpy()
        return D, fmap, grads
    with torch.no_grad():
        D, _, _ = run(torch.float64, None, False)
    _, fmap, grads = run(torch.float32, D, True)
    return dict(map=fmap, grads=grads)


@functools.lru_cache(maxsize=None)
def _reference(name, C, aa, raw, colour_loss, feature_loss):
    import scenes
    sc, cam = cm.case_scene(scenes, cm.CASES[name])
    F = features_of(sc["means3D"].shape[0], C)
    r64 = evaluate64(sc, cam, F, aa=aa, raw=raw, colour_loss=colour_loss, feature_loss=feature_loss)
    r32 = restate32(sc, cam, F, r64["g1"], r64["g0"], aa=aa, raw=raw, colour_loss=colour_loss, feature_loss=feature_loss)
    return dict(sc=sc, cam=cam, F=F, r64=r64, r32=r32)


def reference(name, C, aa=False, raw=False, colour_loss=True, feature_loss=True):
    """The float64 / float32 references of one case, computed once per process and shared: do not modify them."""
    return _reference(name, int(C), bool(aa), bool(raw), bool(colour_loss), bool(feature_loss))
