"""-m gpu: per-Gaussian feature vectors through the blend (`features=F`; include/gsrast.h: gsrast_features_forward / _backward,
csrc/gsrast_features.h) against tests/features_math.py -- torch fp64 on tests/math_renderer.py.

Cases (contrib_math.CASES), image 70 x 45 = 5 x 3 tiles, ragged in both axes.  a: 700 Gaussians, one tile list of more than two 256-entry
batches, an opaque stack that ends its pixels early, Gaussians behind the camera and off screen.  b: 2000 sparse Gaussians, two empty tiles.
C in {1, 3, 19, 64}: one channel, the colour's width, a ragged tail behind a full chunk, the maximum (two passes of 32).  Maps are compared
on the fp32-unambiguous pixels (more than 95 % of each case, asserted), the upstream gradients are zero on the others.

Map bar: 4 x the fp32 restatement's own error against fp64 (features_math.restate32), as a max|ref| + r |ref| (r: the largest relative
error among entries above a tenth of the map's maximum, a: what that leaves of the others).  Measured on the CPU over cases a and b, the
variants plain / antialiasing / raw and the four widths:   a = 1.42e-6   r = 1.85e-5   (worst: case b, C = 64 plain for a; case b, C = 3 raw for r -- small Gaussians whose
few pixels sit on the steep flank of exp).
Gradient bar: conftest.grad_tol(ref64, ref32) per tensor, loss = sum feature_map g1 + sum color g0.  Every test prints its worst err / bar."""
import numpy as np
import pytest
import torch

import contrib_math as cm
import features_math as fm
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu

MAP_BAR = (1.42e-6, 1.85e-5)      # (a, r): the test bar is 4 x (a max|ref| + r |ref|)


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _np(x):
    return x.detach().double().cpu().numpy()


def _render(rast, gpu, sc, cam, F=None, *, aa=False, aux=False, raw=False, g1=None, g0=None, precomp=None, bg=None, camera=False, contrib=False,
            retain=False, rs=None, **more):
    """One forward (+ one backward when g1 or g0 is given: loss = sum map g1 + sum color g0).  F: [P,C] array, None = no features.
    precomp: [P,3] array rendered as colors_precomp instead of the SH colour.  Returns dict(out, map, grads, leaves, sink, rs, loss)."""
    P = sc["means3D"].shape[0]
    grad = g1 is not None or g0 is not None
    rs = rs if rs is not None else settings_from(rast, cam, sc, gpu, bg=bg)
    kw = dict(return_aux=aux, antialiasing=aa, **more)
    Ft = None
    if F is not None:
        Ft = F if isinstance(F, torch.Tensor) else _t(F, gpu).requires_grad_(grad)
        kw["features"] = Ft
    if camera:
        kw["camera_grads"] = True
    sink = torch.full((P, 4), float("nan"), device=gpu) if contrib else None
    if contrib:
        kw["contrib"] = sink
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=grad)
    if raw:
        leaves = {n: _t(v, gpu).requires_grad_(grad) for n, v in fm.raw_arrays(sc).items()}
        out = rast.GaussianRasterizerRaw(rs)(means2D=m2, **leaves, **kw)
    else:
        leaves = {n: _t(sc[n], gpu).requires_grad_(grad) for n in fm.DENSE}
        col = dict(shs=leaves["shs"])
        if precomp is not None:
            leaves["shs"] = _t(precomp, gpu).requires_grad_(grad)
            col = dict(colors_precomp=leaves["shs"])
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], scales=leaves["scales"],
                                          rotations=leaves["rotations"], **col, **kw)
    fmap = out[-1] if F is not None else None
    grads, loss = None, None
    if grad:
        loss = 0.0
        if g1 is not None:
            loss = loss + (fmap * _t(g1, gpu)).sum()
        if g0 is not None:
            loss = loss + (out[0] * _t(g0, gpu)).sum()
        loss.backward(retain_graph=retain)
        grads = _grads_of(leaves, m2, Ft)
    torch.cuda.synchronize()
    return dict(out=out, map=fmap, grads=grads, leaves=leaves, m2=m2, F=Ft, sink=sink, rs=rs, loss=loss)


def _grads_of(leaves, m2, Ft):
    z = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else _np(x.grad)      # noqa: E731
    g = {n: z(x) for n, x in leaves.items()}
    g["means2D"] = z(m2)[:, :2]
    if Ft is not None:
        g["features"] = z(Ft)
    return g


def _check_map(got, ref, amb, what):
    a, r = MAP_BAR
    ok = ~amb
    err = np.abs(got - ref)[:, ok]
    tol = 4.0 * (a * np.abs(ref[:, ok]).max() + r * np.abs(ref[:, ok]))
    print(f"{what}: map max|err| {err.max():.3e} max|ref| {np.abs(ref[:, ok]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
    assert not np.isnan(got).any(), "a pixel of the map was not written"
    assert (err <= tol).all(), (what, float(err.max()), float((err / tol).max()))


def _check_grads(got, r64, r32, what, names=None):
    worst = ("", 0.0)
    for n in (names or r64):
        assert n in got, (what, n, "the device side produced no gradient of this name")
        want = r64[n].reshape(got[n].shape)
        tol = grad_tol(want, r32[n].reshape(got[n].shape) if r32 is not None and n in r32 else None)
        err = np.abs(got[n] - want)
        ratio = float((err / np.maximum(tol, 1e-300)).max())
        worst = max(worst, (n, ratio), key=lambda x: x[1])
        assert np.abs(want).max() > 0 or n == "shs", (what, n)
        assert (err <= tol).all(), (what, n, float(err.max()), float(np.abs(want).max()), ratio)
    print(f"{what}: worst gradient err / bar {worst[1]:.3f} ({worst[0]})")


# ---- 1. against the fp64 reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "antialias", "return_aux", "raw"])
@pytest.mark.parametrize("C", fm.CHANNELS)
@pytest.mark.parametrize("name", list(cm.CASES))
def test_against_the_fp64_reference(name, C, variant, rast, gpu):
    aa, raw, aux = variant == "antialias", variant == "raw", variant == "return_aux"
    r = fm.reference(name, C, aa=aa, raw=raw)
    r64, r32 = r["r64"], r["r32"]
    assert r64["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    h = _render(rast, gpu, r["sc"], r["cam"], r["F"], aa=aa, raw=raw, aux=aux, g1=r64["g1"], g0=r64["g0"])
    assert np.array_equal(h["out"][1].cpu().numpy() > 0, r64["vis"]), "radius decision differs: pick another seed"
    assert tuple(h["map"].shape) == (C,) + r64["amb"].shape and len(h["out"]) == (6 if aux else 4)
    what = f"case {name}, C {C}, {variant}"
    _check_map(_np(h["map"]), r64["map"], r64["amb"], what)
    _check_grads(h["grads"], r64["grads"], r32["grads"], what)
    # culled and never-blended Gaussians: exactly zero rows
    gF = h["grads"]["features"]
    assert not gF[~r64["vis"]].any() and np.array_equal(gF.any(1), r64["grads"]["features"].any(1))


# ---- 2. against the existing HIP path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cm.CASES))
def test_three_channels_are_the_colour_path(name, rast, gpu):
    r = fm.reference(name, 3, colour_loss=False)
    r64, r32 = r["r64"], r["r32"]
    h = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r64["g1"])
    c = _render(rast, gpu, r["sc"], r["cam"], None, precomp=r["F"], bg=np.zeros(3, np.float32), g0=r64["g1"])
    a, rr = MAP_BAR
    ok = ~r64["amb"]
    m, col = _np(h["map"])[:, ok], _np(c["out"][0])[:, ok]
    assert (np.abs(m - col) <= 4.0 * (a * np.abs(col).max() + rr * np.abs(col))).all()
    # the two HIP paths against each other, within grad_tol of the fp64 gradients (and each against those, within the same bar)
    worst = ("", 0.0)
    for n, m in (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("scales", "scales"), ("rotations", "rotations"), ("features", "shs")):
        want = r64["grads"][n]
        tol = grad_tol(want, r32["grads"][n])
        assert np.abs(want).max() > 0, n
        assert (np.abs(h["grads"][n] - want) <= tol).all() and (np.abs(c["grads"][m] - want) <= tol).all(), n
        ratio = float((np.abs(h["grads"][n] - c["grads"][m]) / tol).max())
        worst = max(worst, (n, ratio), key=lambda x: x[1])
        assert (np.abs(h["grads"][n] - c["grads"][m]) <= tol).all(), (n, ratio)
    print(f"case {name}: features vs colors_precomp, worst gradient |h - c| / bar {worst[1]:.3f} ({worst[0]})")


@pytest.mark.parametrize("exp_mode", [1, 2])
def test_three_channels_are_the_colour_path_in_the_other_exp_modes(exp_mode, rast, gpu):
    """The device-against-device half of the test above with both renders under exp_mode 1 / 2: the replay's alpha and T are the forward's
    own in every mode, so the bars stand as they are and every pixel is compared (the fp64 reference and its ambiguity mask belong to mode 0
    and serve as the gradient bar's scale only)."""
    r = fm.reference("a", 3, colour_loss=False)
    r64, r32 = r["r64"], r["r32"]
    rast._C.set_option("exp_mode", exp_mode)
    try:
        h = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r64["g1"])
        c = _render(rast, gpu, r["sc"], r["cam"], None, precomp=r["F"], bg=np.zeros(3, np.float32), g0=r64["g1"])
    finally:
        rast._C.set_option("exp_mode", 0)
    a, rr = MAP_BAR
    m, col = _np(h["map"]), _np(c["out"][0])
    tol = 4.0 * (a * np.abs(col).max() + rr * np.abs(col))
    print(f"exp_mode {exp_mode}: features vs colors_precomp, map worst |h - c| / bar {float((np.abs(m - col) / tol).max()):.3f}")
    assert not np.isnan(m).any() and np.abs(col).max() > 0 and (np.abs(m - col) <= tol).all()
    worst = ("", 0.0)
    for n, k in (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("scales", "scales"), ("rotations", "rotations"), ("features", "shs")):
        tol = grad_tol(r64["grads"][n], r32["grads"][n])
        ratio = float((np.abs(h["grads"][n] - c["grads"][k]) / tol).max())
        worst = max(worst, (n, ratio), key=lambda x: x[1])
        assert np.abs(h["grads"][n]).max() > 0, n
        assert (np.abs(h["grads"][n] - c["grads"][k]) <= tol).all(), (n, ratio)
    print(f"exp_mode {exp_mode}: features vs colors_precomp, worst gradient |h - c| / bar {worst[1]:.3f} ({worst[0]})")


# ---- 3. additivity: the records are added to, not overwritten --------------------------------------------------------------------------------
def test_colour_and_feature_gradients_add(rast, gpu):
    r = fm.reference("a", 19)
    r64, r32 = r["r64"], r["r32"]
    both = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r64["g1"], g0=r64["g0"])
    feat = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r64["g1"])
    colr = _render(rast, gpu, r["sc"], r["cam"], r["F"], g0=r64["g0"])
    assert not colr["grads"]["features"].any()
    for n in both["grads"]:
        s = feat["grads"][n] + colr["grads"][n]
        tol = grad_tol(r64["grads"][n].reshape(s.shape), r32["grads"][n].reshape(s.shape))
        assert np.abs(feat["grads"][n]).max() > 0 or n == "shs", n
        assert (np.abs(both["grads"][n] - s) <= tol).all(), (n, float(np.abs(both["grads"][n] - s).max()))
    for n in ("means2D", "opacities", "means3D"):      # neither part is negligible: overwriting would show
        tol = grad_tol(r64["grads"][n].reshape(both["grads"][n].shape))
        assert (np.abs(both["grads"][n] - feat["grads"][n]) > 100 * tol).any() and (np.abs(both["grads"][n] - colr["grads"][n]) > 100 * tol).any(), n


# ---- 4. nothing else moves ------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves_and_no_launch_without_features(rast, gpu):
    _C = rast._C
    r = fm.reference("a", 19)
    _C.set_option("profile", -1)
    try:
        _C.profile_reset()
        wo = _render(rast, gpu, r["sc"], r["cam"], None, aux=True, contrib=True, g0=r["r64"]["g0"])
        prof = _C.profile_read()
        assert prof["features_fwd"][1] == 0 and prof["features_bwd"][1] == 0 and prof["blend_fwd"][1] >= 1 and prof["blend_bwd"][1] == 1
        w = _render(rast, gpu, r["sc"], r["cam"], r["F"], aux=True, contrib=True, g1=r["r64"]["g1"], g0=r["r64"]["g0"])
        prof = _C.profile_read()
        assert prof["features_fwd"][1] == 1 and prof["features_bwd"][1] == 1 and prof["blend_bwd"][1] == 2
        _C.profile_reset()
        _render(rast, gpu, r["sc"], r["cam"], r["F"], g0=r["r64"]["g0"])      # a map nobody differentiates: today's backward
        prof = _C.profile_read()
        assert prof["features_fwd"][1] == 1 and prof["features_bwd"][1] == 0 and prof["blend_bwd"][1] == 1
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()
    assert len(w["out"]) == len(wo["out"]) + 1
    for a, b in zip(w["out"][:-1], wo["out"]):      # colour, radii, depth, acc_depth, alpha
        assert torch.equal(a, b)
    assert torch.equal(w["sink"], wo["sink"]) and not torch.isnan(w["sink"]).any()


@pytest.mark.parametrize("raw", [False, True], ids=["dense", "raw"])
def test_every_keyword_at_once(raw, rast, gpu):
    """One render with return_aux, antialiasing, absgrad, camera_grads, contrib and features together, loss = sum map g1 + sum color g0: every
    forward output is bit for bit that of the render that gives its keyword alone, the gradients meet the fp64 reference at the file's bar, and
    the launches are those of the parts.  The launch counts are read the way test_nothing_else_moves_and_no_launch_without_features reads them:
    the profile runs over two backwards -- the return_aux-only render, then the all-at-once one -- so blend_bwd ends at 2 (1 after the first).
    A window of the all-at-once render alone counts blend_bwd 1, features_fwd 1, features_bwd 1, contrib_blend 1, contrib_finish 1, in both families."""
    _C = rast._C
    r = fm.reference("a", 19, aa=True, raw=raw)
    r64, r32 = r["r64"], r["r32"]
    sc, cam, F = r["sc"], r["cam"], r["F"]
    P, H, W = sc["means3D"].shape[0], cam["image_height"], cam["image_width"]
    rs = settings_from(rast, cam, sc, gpu)
    rq = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    single = lambda F=None, **kw: _render(rast, gpu, sc, cam, F, aa=True, raw=raw, rs=rs, g0=r64["g0"], **kw)      # noqa: E731
    plain, con, feat = single(), single(contrib=True), single(F)
    sink2 = torch.full((P, 2), float("nan"), device=gpu)
    _C.set_option("profile", -1)
    try:
        _C.profile_reset()
        aux = single(aux=True)
        prof = _C.profile_read()
        assert prof["blend_bwd"][1] == 1 and not any(prof[k][1] for k in ("features_fwd", "features_bwd", "contrib_blend", "contrib_finish"))
        h = _render(rast, gpu, sc, cam, F, aa=True, aux=True, raw=raw, g1=r64["g1"], g0=r64["g0"], camera=True, contrib=True, rs=rq, absgrad=sink2)
        prof = _C.profile_read()
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()
    print(f"{'raw' if raw else 'dense'}: launches " + ", ".join(f"{k} {prof[k][1]}" for k in ("features_fwd", "features_bwd", "blend_bwd", "contrib_blend", "contrib_finish")))
    assert prof["features_fwd"][1] == 1 and prof["features_bwd"][1] == 1 and prof["blend_bwd"][1] == 2
    assert prof["contrib_blend"][1] == 1 and prof["contrib_finish"][1] == 1
    # (color, radii, depth, acc_depth, alpha, feature_map), each what its own keyword gives
    color, radii, depth, acc_depth, alpha, fmap = h["out"]
    assert tuple(color.shape) == (3, H, W) and tuple(radii.shape) == (P,) and radii.dtype is torch.int32 and tuple(fmap.shape) == (19, H, W)
    assert tuple(depth.shape) == tuple(acc_depth.shape) == tuple(alpha.shape) == (1, H, W)
    for a, b in zip((color, radii, depth), plain["out"]):
        assert torch.equal(a, b)
    assert len(aux["out"]) == 5 and torch.equal(acc_depth, aux["out"][3]) and torch.equal(alpha, aux["out"][4])
    assert torch.equal(h["sink"], con["sink"]) and not torch.isnan(h["sink"]).any()
    assert torch.equal(fmap, feat["map"]) and not torch.isnan(fmap).any()
    what = f"every keyword at once, {'raw' if raw else 'dense'}"
    _check_grads(h["grads"], r64["grads"], r32["grads"], what)
    gv = rq.viewmatrix.grad
    assert gv is not None and gv.shape == rq.viewmatrix.shape and gv.dtype is rq.viewmatrix.dtype
    assert bool(torch.isfinite(gv).all()) and bool(gv.any())
    # the sink against the signed gradient: the expression and the slack of tests/test_gpu_absgrad.py.  The sink is a statistic of the colour
    # (and aux) loss alone (module docstring of the package: "absgrad stays a statistic of the colour and the aux outputs only"), so the signed
    # gradient it bounds is that of sum color g0 -- the single-keyword render's --, not this backward's means2D.grad, which includes the map's
    # loss: against that one the relation fails in 1016 of the 1400 entries, by up to 1.07e+02, in both families, before and after the refactor
    got, signed, both = _np(sink2), plain["grads"]["means2D"], h["grads"]["means2D"]
    assert not np.isnan(got).any(), "a row of the sink was not written"
    print(f"{what}: sink - |means2D.grad| (1 - 1e-4), smallest entry: colour loss alone {float((got - np.abs(signed) * (1.0 - 1e-4)).min()):.3e}, "
          f"colour + map loss {float((got - np.abs(both) * (1.0 - 1e-4)).min()):.3e} ({int((got < np.abs(both) * (1.0 - 1e-4)).sum())} of {got.size} entries below)")
    assert np.abs(signed).max() > 0 and (got >= np.abs(signed) * (1.0 - 1e-4)).all()


# ---- 5. retained graph ----------------------------------------------------------------------------------------------------------------------
def test_second_backward_on_a_retained_graph(rast, gpu):
    r = fm.reference("b", 19)
    r64, r32 = r["r64"], r["r32"]
    h = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r64["g1"], g0=r64["g0"], retain=True)
    first = h["grads"]
    for x in list(h["leaves"].values()) + [h["m2"], h["F"]]:
        x.grad = None
    h["loss"].backward()
    torch.cuda.synchronize()
    second = _grads_of(h["leaves"], h["m2"], h["F"])
    for n in first:
        tol = grad_tol(r64["grads"][n].reshape(first[n].shape), r32["grads"][n].reshape(first[n].shape))
        assert (np.abs(second[n] - first[n]) <= tol).all() and np.abs(second[n]).max() > 0, n
    _check_grads(second, r64["grads"], r32["grads"], "second backward")


# ---- 6. camera gradients -----------------------------------------------------------------------------------------------------------------------
def test_camera_gradients_of_a_feature_only_loss(rast, gpu):
    """The camera's gradient of sum feature_map g1 against posegrad_math in fp64 (the three-channel map is its colour render of rgb = F over a
    zero background), bar grad_tol(want, its float32 evaluation) -- the bar of tests/test_gpu_posegrad.py."""
    pm = fm.pm
    r = fm.reference("a", 3, colour_loss=False)
    sc, cam, F, g1 = r["sc"], r["cam"], r["F"], r["r64"]["g1"]
    cfg = dict(pm.cfg_of(cam, sc), bg=np.zeros(3))
    want = {}
    D = None
    for dtype in (torch.float64, torch.float32):
        t = pm.tensors(dict(sc, rgb=F), ("means3D", "opacities", "scales", "rotations", "rgb"), dtype, grad=False)
        V, Pm, Cp = pm.camera_leaves(cam, dtype)
        out = pm.render(t, V, Pm, Cp, cfg, decisions=D)
        D = out["decisions"]
        (out["color"] * torch.as_tensor(g1).to(dtype)).sum().backward()
        want[dtype] = dict(viewmatrix=_np(V.grad), projmatrix=_np(Pm.grad))
    rs = settings_from(rast, cam, sc, gpu)
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True))
    _render(rast, gpu, sc, cam, F, g1=g1, camera=True, rs=rs)
    for n, x in (("viewmatrix", rs.viewmatrix), ("projmatrix", rs.projmatrix)):
        w64 = want[torch.float64][n]
        err = np.abs(_np(x.grad) - w64)
        tol = grad_tol(w64, want[torch.float32][n])
        print(f"camera {n}: max|want| {np.abs(w64).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
        assert np.abs(w64).max() > 0 and (err <= tol).all(), (n, float(err.max()))


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------------------------
def test_empty_scene_one_pixel_and_no_grad(rast, gpu, scenes):
    r = fm.reference("b", 19)
    sc0 = {k: (v[:0] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in r["sc"].items()}
    h = _render(rast, gpu, sc0, r["cam"], np.zeros((0, 5), np.float32), g1=np.ones((5, 45, 70), np.float32), g0=np.ones((3, 45, 70), np.float32))
    assert tuple(h["map"].shape) == (5, 45, 70) and not h["map"].any() and h["grads"]["features"].shape == (0, 5)
    cam1 = scenes.camera(1, 6, 1, 1)
    sc = scenes.synth(50, 3, scale_mul=3.0)
    F = fm.features_of(50, 7)
    a = _render(rast, gpu, sc, cam1, F, aux=True, g1=np.ones((7, 1, 1), np.float32))
    w = a["grads"]["features"]
    # dL/dF[i][c] = w_i for every channel; sum_i w_i = alpha; the map is sum_i w_i F[i]
    assert (np.abs(w - w[:, :1]) <= 1e-7).all() and abs(w[:, 0].sum() - float(a["out"][4].detach().sum())) <= 1e-5 and w[:, 0].max() > 0
    assert (np.abs(_np(a["map"]).reshape(-1) - (w[:, :1] * F).sum(0)) <= 1e-5 * np.abs(F).max()).all()
    with torch.no_grad():
        ng = _render(rast, gpu, r["sc"], r["cam"], r["F"])
    ref = _render(rast, gpu, r["sc"], r["cam"], r["F"], g1=r["r64"]["g1"])
    assert torch.equal(ng["map"], ref["map"]) and not ng["map"].requires_grad


def test_low_level_backward_writes_no_row_past_P(rast, gpu, monkeypatch):
    """gsrast_features_backward in the window its contract names -- behind a render backward with backward_phase = 1, in front of one with
    backward_phase = 2 --, on the binding's own entries: dL_dfeatures is rows [0, P) of a NaN-poisoned [P + 1, C] buffer; row P keeps its NaN,
    every row below is written, non-zero only where gsrast_touched_rows allows; the second phase's gradients include the map's loss."""
    _C = rast._C
    r = fm.reference("a", 19)
    sc, cam, F = r["sc"], r["cam"], r["F"]
    P, H, W, Cn = sc["means3D"].shape[0], cam["image_height"], cam["image_width"], F.shape[1]
    rs = settings_from(rast, cam, sc, gpu)
    e = torch.empty(0)
    ten = {n: _t(sc[n], gpu) for n in fm.DENSE}
    Ft = _t(F, gpu)
    R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix,
                                                                rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
    fmap = _C.features_forward(Ft, R, W, H, gb, bb, ib)
    mod = _render(rast, gpu, sc, cam, F, g1=r["r64"]["g1"], g0=r["r64"]["g0"])
    assert torch.equal(fmap, mod["map"])
    big = torch.full((P + 1, Cn), float("nan"), device=gpu)
    gmap = _t(r["r64"]["g1"], gpu)
    o = _C._options_struct()
    import ctypes

    def backward(phase):      # (one phase of the render backward on this state: the handle tests/test_gpu_posegrad.py uses)
        monkeypatch.setattr(_C, "_run_backward", lambda ar, call, P_, geom_, dev_: call(phase))
        return _C.rasterize_gaussians_backward(rs.bg, ten["means3D"], radii, e, ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                               rs.tanfovy, _t(r["r64"]["g0"], gpu), ten["shs"], 3, rs.campos, gb, R, bb, ib, first_backward=(phase == 1))

    backward(1)
    rc = _C.lib().gsrast_features_backward(ctypes.byref(o), P, R, Cn, W, H, gb.data_ptr(), bb.data_ptr(), ib.data_ptr(), Ft.data_ptr(), gmap.data_ptr(),
                                           big.data_ptr(), _C._stream_of(gpu))
    second = backward(2)
    monkeypatch.undo()
    flags = torch.zeros(P, dtype=torch.uint8, device=gpu)
    assert rc == 0 and _C.lib().gsrast_touched_rows(P, gb.data_ptr(), flags.data_ptr(), _C._stream_of(gpu)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(big[P]).all() and not torch.isnan(big[:P]).any()
    nonzero = (big[:P] != 0).any(dim=1)
    assert not (nonzero & (flags == 0)).any() and int(nonzero.sum()) > 600
    tol = grad_tol(r["r64"]["grads"]["features"], r["r32"]["grads"]["features"])
    assert (np.abs(_np(big[:P]) - r["r64"]["grads"]["features"]) <= tol).all()
    for got, n in ((second[0][:, :2], "means2D"), (second[2], "opacities"), (second[3], "means3D")):
        want = r["r64"]["grads"][n]
        assert (np.abs(_np(got) - want) <= grad_tol(want, r["r32"]["grads"][n])).all(), n


# ---- 8. list cut ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.remembered_cut_only
def test_list_cut_is_bit_identical_to_no_list_cut(rast, gpu, scenes):
    """The shape of tests/test_gpu_contrib.py's list-cut test: 50 000 Gaussians at 256 x 192 with raised opacities.  The first render, without
    the cut, leaves the pose's cut depths; the next ones leave the late Gaussians out of the lists and must give the same map bit for bit."""
    _C = rast._C
    P, W, H = 50_000, 256, 192
    sc = scenes.synth(P, 451)
    sc["opacities"] = (1.0 / (1.0 + np.exp(-(np.log(sc["opacities"] / (1.0 - sc["opacities"])) + 2.0)))).astype(np.float32)
    cam = scenes.camera(2, 5, W, H)
    F = fm.features_of(P, 19)
    _C.set_option("list_cut_always", 1)
    try:
        _C.set_option("no_list_cut", 1)
        try:
            full = _render(rast, gpu, sc, cam, F)
            assert _C.context_query("last_late") == 0
        finally:
            _C.set_option("no_list_cut", 0)
        for visit in range(2):
            cut = _render(rast, gpu, sc, cam, F)
            assert _C.context_query("last_late") > 0, "the repeated pose was expected to run under the list cut"
            assert torch.equal(cut["out"][0], full["out"][0])
            assert torch.equal(cut["map"], full["map"]), f"visit {visit}: {int((cut['map'] != full['map']).sum())} entries differ"
    finally:
        _C.set_option("list_cut_always", 0)
    assert not torch.isnan(full["map"]).any() and float(full["map"].abs().max()) > 0.5
