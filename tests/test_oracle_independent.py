"""CPU: the oracle against an INDEPENDENT derivation (tests/math_renderer.py: torch float64, autograd, no tile lists, no
hand-written gradients -- written from the mathematics, sharing no code with oracle/gsrast_oracle.c or the HIP kernels).

What this pins that the reference-derived golden vectors cannot (no CUDA here): computeCov2D / conic / radius / getRect
(forward.cu:74-113, :218-236, auxiliary.h:46-56), the compositing recurrence (forward.cu:311-381) and EVERY backward formula
(backward.cu:144-341, :399-557) -- the latter as "the oracle's hand-derived gradients equal autograd's".  A misreading of the
reference shared by the oracle and the kernels would have to be shared by the textbook formulas too to stay green."""
import numpy as np
import pytest
import torch

import math_renderer as mr
from edge_scenes import clamped_mask, edge_scene


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _scene(scenes, P, seed, W, H, k, V, deg=3, scale_mul=1.0, bg=(0.0, 0.0, 0.0), opac_mul=1.0):
    sc = scenes.synth(P, seed, sh_degree=deg, scale_mul=scale_mul)
    sc["bg"] = np.array(bg, np.float32)
    sc["opacities"] = (sc["opacities"] * opac_mul).astype(np.float32)
    return sc, scenes.camera(k, V, W, H)


@pytest.mark.parametrize("P,seed,W,H,k,V,smul", [(400, 11, 96, 64, 1, 5, 1.0), (900, 12, 80, 112, 2, 7, 0.6), (120, 13, 64, 48, 0, 3, 2.5)])
def test_projection_conic_radius_rect_against_the_math(orc, scenes, P, seed, W, H, k, V, smul):
    sc, cam = _scene(scenes, P, seed, W, H, k, V, scale_mul=smul)
    o32 = orc.forward(sc, cam)
    o64 = orc.forward(sc, cam, st32=o32)
    pr = mr.project(_t(sc["means3D"]), _t(sc["scales"]), _t(sc["rotations"]), cam)
    d = pr["disc"]
    # discrete quantities: equal unless the real-valued radius / rectangle edge sits within fp32 rounding of an integer
    firm = (d["radius_margin"] > 1e-4) & (d["rect_margin"] > 1e-5)
    assert firm.mean() > 0.98
    np.testing.assert_array_equal(o32["radii"][firm], d["radius"][firm])
    np.testing.assert_array_equal(o32["tiles_touched"][firm].astype(np.int64), d["tiles"][firm])
    vis = (o32["radii"] > 0) & firm
    assert vis.sum() > P // 4
    # continuous quantities, fp64 oracle build vs fp64 math: rounding only
    np.testing.assert_allclose(o64["means2D"][vis], pr["pix"].numpy()[vis], rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(o64["depths"][vis], pr["depth"].numpy()[vis], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(o64["conic_opacity"][vis, :3], pr["conic"].numpy()[vis], rtol=1e-9, atol=1e-12)
    S = pr["Sigma"].numpy()
    cov6 = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
    np.testing.assert_allclose(o64["cov3D"][vis], cov6[vis], rtol=1e-12, atol=1e-15)
    # ... and the fp32 build (what the HIP kernel is bit-compared with) within fp32 rounding of the math
    np.testing.assert_allclose(o32["conic_opacity"][vis, :3], pr["conic"].numpy()[vis], rtol=3e-4, atol=1e-6)
    assert (np.abs(o32["cov3D"][vis] - cov6[vis]) <= 1e-6 * np.abs(cov6[vis]).max(axis=1, keepdims=True)).all()   # off-diagonals cancel


CASES = [
    dict(P=300, seed=21, W=64, H=48, k=1, V=5, deg=3, smul=0.8, bg=(0.1, 0.2, 0.3), omul=1.0),
    dict(P=700, seed=22, W=96, H=80, k=3, V=7, deg=2, smul=0.5, bg=(0.0, 0.0, 0.0), omul=0.7),
    dict(P=150, seed=23, W=48, H=64, k=0, V=4, deg=1, smul=1.6, bg=(1.0, 1.0, 1.0), omul=1.0),
    dict(P=500, seed=24, W=80, H=64, k=2, V=6, deg=0, smul=0.7, bg=(0.0, 0.5, 0.0), omul=0.5),
]


# the same, with edge_scenes' Gaussians added: at the near plane, needles, and outside the frustum clamp (x, y, both; 1.31 ... 2.5)
EDGE = [
    dict(name="edge_P300_deg3", P=300, seed=21, W=64, H=48, k=1, V=5, deg=3, smul=0.8, bg=(0.1, 0.2, 0.3), omul=1.0),
    dict(name="edge_P150_deg1", P=150, seed=23, W=48, H=64, k=0, V=4, deg=1, smul=1.6, bg=(1.0, 1.0, 1.0), omul=1.0),
    dict(name="edge_P500_deg0", P=500, seed=24, W=80, H=64, k=2, V=6, deg=0, smul=0.7, bg=(0.0, 0.5, 0.0), omul=0.5),
]
# long lists: the forward blend stages 256 / PPL instances per round, the backward 64 (csrc/gsrast_blend.h) -- a tile with more than
# 256 listed, a pixel with more than 128 contributors and pixels that end by the T < 1e-4 stop reach the later rounds of both
LONG = [
    dict(name="long_P1500_deg2", P=1500, seed=49, W=64, H=48, k=2, V=7, deg=2, smul=1.0, bg=(0.3, 0.1, 0.2), omul=0.35),
    dict(name="long_P800_deg1", P=800, seed=53, W=50, H=37, k=0, V=3, deg=1, smul=1.3, bg=(0.0, 0.0, 0.0), omul=0.4),
]
_ID = lambda c: c.get("name") or f"P{c['P']}_deg{c['deg']}"      # noqa: E731


def _build(scenes, c):
    if "name" in c:
        return edge_scene(scenes, c)
    return _scene(scenes, c["P"], c["seed"], c["W"], c["H"], c["k"], c["V"], c["deg"], c["smul"], c["bg"], c["omul"])


def _autograd(sc, cam, deg, clamp_grad="reference"):
    P = sc["means3D"].shape[0]
    leaves = {n: _t(sc[n]).clone().requires_grad_(True) for n in LEAF_KEYS}
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    out = mr.render(leaves["means3D"], leaves["scales"], leaves["rotations"], leaves["opacities"], leaves["shs"], deg, cam,
                    sc["bg"], ndc_offset=off, clamp_grad=clamp_grad)
    return leaves, off, out


LEAF_KEYS = {"means3D": "dL_dmeans3D", "scales": "dL_dscales", "rotations": "dL_drotations", "opacities": "dL_dopacity", "shs": "dL_dsh"}


def _assert_rows(got, want, name):
    np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9 * max(1.0, float(np.abs(want).max())), err_msg=name)


@pytest.mark.parametrize("c", CASES + EDGE + LONG, ids=_ID)
def test_forward_and_all_gradients_against_autograd_of_the_math(orc, scenes, c):
    sc, cam = _build(scenes, c)
    W, H, P = c["W"], c["H"], sc["means3D"].shape[0]
    leaves, off, out = _autograd(sc, cam, c["deg"])
    amb = out["ambiguous"]
    assert amb.mean() < (0.05 if "name" in c else 0.02), "too many pixels with an fp32-ambiguous decision for a meaningful comparison"
    assert out["min_depth_gap"] > 2e-6, "two Gaussians closer in depth than fp32 resolves: pick another seed"
    g = (scenes.upstream_grad(H, W, c["seed"] + 1) * (H * W)).astype(np.float32)
    g[:, amb] = 0.0                                     # ambiguous pixels take no part in the gradient, on either side
    o64 = orc.render(sc, cam, g, f64=True)
    # same Gaussians drawn, same order inside every tile
    o32 = orc.forward(sc, cam)
    d = out["proj"]["disc"]
    assert np.array_equal(o32["radii"] > 0, d["vis"]) and np.array_equal(o32["radii"], d["radius"]), "radius decision differs: pick another seed"
    keep = ~amb
    np.testing.assert_allclose(o64["out_color"][:, keep], out["color"].detach().numpy()[:, keep], rtol=0, atol=1e-10)
    np.testing.assert_allclose(o64["final_T"][keep], out["final_T"].detach().numpy()[keep], rtol=0, atol=1e-10)
    np.testing.assert_allclose(o64["out_depth"][0][keep], out["depth"].numpy()[keep], rtol=0, atol=1e-9)
    # backward: autograd of the math vs the oracle's hand-derived formulas, every row of every leaf
    (out["color"] * _t(g)).sum().backward()
    for name, key in LEAF_KEYS.items():
        _assert_rows(o64[key].reshape(leaves[name].shape), leaves[name].grad.numpy(), name)
    _assert_rows(o64["dL_dmeans2D"][:, :2], off.grad.numpy(), "means2D")
    want = leaves["means3D"].grad.numpy()
    assert np.abs(want).max() > 1e-3      # the comparison is not vacuous
    assert out["n_live"].max() >= 5
    if "name" in c:
        # the frustum-clamped rows once more, as a tensor of their own: their gradients are far below the tensor's largest entry
        cl = clamped_mask(sc, cam)
        assert (np.abs(want[cl]).max(axis=1) > 0).sum() >= 16, "too few clamped Gaussians with a gradient"
        _assert_rows(o64["dL_dmeans3D"][cl], want[cl], "means3D, clamped rows")
    if c in LONG:
        assert out["tile_list_max"] > 256
        assert int((o32["ranges"][:, 1].astype(np.int64) - o32["ranges"][:, 0]).max()) == out["tile_list_max"]
        assert out["n_live"].max() > 128
        assert (out["stopped"] & keep).sum() > 0, "no pixel ends by the T < 1e-4 stop"


def test_clamp_convention_matters_only_on_clamped_rows(orc, scenes):
    """backward.cu:172-176, :262-264: the clamped t.x, t.y are constants of the reference's backward.  Differentiating the clamp as
    written ("true") changes dL/dmeans3D of the clamped rows -- nothing else -- by far more than the comparison's bar, and the
    oracle sides with the reference's convention."""
    for c in EDGE:
        sc, cam = edge_scene(scenes, c)
        ref_l, ref_off, ref = _autograd(sc, cam, c["deg"], "reference")
        tru_l, tru_off, tru = _autograd(sc, cam, c["deg"], "true")
        for k in ("color", "final_T", "depth"):
            assert np.array_equal(ref[k].detach().numpy(), tru[k].detach().numpy()), k      # the forward is the same function
        g = (scenes.upstream_grad(c["H"], c["W"], c["seed"] + 1) * (c["H"] * c["W"])).astype(np.float32)
        g[:, ref["ambiguous"]] = 0.0
        (ref["color"] * _t(g)).sum().backward()
        (tru["color"] * _t(g)).sum().backward()
        cl = clamped_mask(sc, cam)
        clamped = ref["proj"]["disc"]["clamped"]
        assert cl.sum() >= 16
        for n in LEAF_KEYS:
            a, b = ref_l[n].grad.numpy(), tru_l[n].grad.numpy()
            rows = ~clamped if n == "means3D" else np.ones(len(a), bool)
            assert np.array_equal(a[rows], b[rows]), n
        assert np.array_equal(ref_off.grad.numpy(), tru_off.grad.numpy())
        a, b = ref_l["means3D"].grad.numpy()[cl], tru_l["means3D"].grad.numpy()[cl]
        own = float(np.abs(a).max())
        assert float(np.abs(a - b).max()) > 1e-3 * own, (float(np.abs(a - b).max()), own)
        o64 = orc.render(sc, cam, g, f64=True)["dL_dmeans3D"][cl]
        _assert_rows(o64, a, "the oracle follows the reference's convention")
        with pytest.raises(AssertionError):
            _assert_rows(o64, b, "... and not the true derivative")


def test_clamp_passthrough_matters_only_where_alpha_saturates(orc, scenes):
    """backward.cu:538 / :554 apply no mask for alpha clamped at 0.99: with saturating Gaussians the oracle follows the reference
    (straight-through), and the two conventions differ exactly when such pairs exist."""
    sc, cam = _scene(scenes, 60, 31, 48, 48, 1, 4, deg=0, scale_mul=3.0)
    sc["opacities"][:] = 0.999
    t = {n: _t(sc[n]).clone().requires_grad_(True) for n in ("means3D", "scales", "rotations", "opacities", "shs")}
    out = mr.render(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], 0, cam, sc["bg"])
    assert out["clamped_pairs"] > 0
    g = (scenes.upstream_grad(48, 48, 32) * (48 * 48)).astype(np.float32)
    g[:, out["ambiguous"]] = 0.0
    (out["color"] * _t(g)).sum().backward()
    o64 = orc.render(sc, cam, g, f64=True)
    want = t["opacities"].grad.numpy()
    np.testing.assert_allclose(o64["dL_dopacity"], want, rtol=1e-7, atol=1e-9 * max(1.0, float(np.abs(want).max())))
