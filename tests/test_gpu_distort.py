"""-m gpu: the depth-distortion map (`distortion=True`; include/gsrast.h: gsrast_distortion_forward / _backward, csrc/gsrast_distort.h)
against tests/distort_math.py -- torch fp64 on tests/math_renderer.py's projection.

Cases (contrib_math.CASES), image 70 x 45 = 5 x 3 tiles, ragged in both axes.  a: 700 Gaussians, one tile list of more than two 256-entry
batches, an opaque stack that ends its pixels early, Gaussians behind the camera and off screen; every pixel has two contributors or more.
b: 2000 sparse Gaussians, two empty tiles, 53 % of the pixels with fewer than two contributors.  Maps are compared on the fp32-unambiguous
pixels (more than 95 % of each case and variant, asserted), the upstream gradients are zero on the others.

Map bar: 4 x the fp32 restatement's own error against fp64 (distort_math.restate32: float32 on the fp64 pass's decisions, depths relative
to the tile's first listed Gaussian like the kernel), as a max|ref| + r |ref| (r: the largest relative error among entries above a tenth of
the map's maximum, a: what that leaves of the others; distort_math.map_bar_terms).  Measured on the CPU over cases a and b and the variants
plain / antialias / return_aux / raw:   a = 3.75e-7   r = 1.44e-5   (worst: case b antialias for a, 3.74e-7; case b plain for r, 1.430e-5 --
pixels whose two or three contributors lie a few hundredths apart in depth, so that |z_i - z_j| itself carries the fp32 rounding of z).
Gradient bar: conftest.grad_tol(ref64, ref32) per tensor, for all leaves and means2D.  Every test prints its worst err / bar.

Gradients and bit-identity: two backwards of the same call do not give bit-equal gradients (float atomics; tests/test_gpu_absgrad.py,
tests/test_gpu_contrib.py), so "nothing else moved" holds the forward's outputs bit for bit, the launches by the profile table's counts, and
the gradients at the suite's run-to-run bar, conftest.grad_tol of the fp64 gradient."""
import numpy as np
import pytest
import torch

import contrib_math as cm
import distort_math as dm
import features_math as fm
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu

MAP_BAR = (3.75e-7, 1.44e-5)      # (a, r): the test bar is 4 x (a max|ref| + r |ref|)


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _np(x):
    return x.detach().double().cpu().numpy()


def _render(rast, gpu, sc, cam, *, distortion=True, aa=False, aux=False, raw=False, g=None, colour_loss=True, F=None, g1=None, camera=False, contrib=False,
            rs=None, absent=False):
    """One forward (+ one backward when g is given: loss = sum map gd [+ sum color g0] [+ sum acc_depth gD + sum alpha gA] [+ sum feature_map g1]).
    absent: the keyword is not passed at all.  Returns dict(out, map, fmap, grads, leaves, m2, sink, rs)."""
    P = sc["means3D"].shape[0]
    grad = g is not None
    rs = rs if rs is not None else settings_from(rast, cam, sc, gpu)
    kw = dict(return_aux=aux, antialiasing=aa)
    if not absent:
        kw["distortion"] = distortion
    Ft = None
    if F is not None:
        Ft = _t(F, gpu).requires_grad_(grad)
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
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], scales=leaves["scales"],
                                          rotations=leaves["rotations"], shs=leaves["shs"], **kw)
    has = distortion and not absent
    dmap = out[-1] if has else None
    fmap = None if F is None else out[-2] if has else out[-1]
    grads = None
    if grad:
        loss = 0.0
        if has and "gd" in g:
            loss = loss + (dmap * _t(g["gd"], gpu)).sum()
        if colour_loss:
            loss = loss + (out[0] * _t(g["g0"], gpu)).sum()
        if aux:
            loss = loss + (out[3][0] * _t(g["gD"], gpu)).sum() + (out[4][0] * _t(g["gA"], gpu)).sum()
        if g1 is not None:
            loss = loss + (fmap * _t(g1, gpu)).sum()
        loss.backward()
        z = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else _np(x.grad)      # noqa: E731
        grads = {n: z(x) for n, x in leaves.items()}
        grads["means2D"] = z(m2)[:, :2]
        if Ft is not None:
            grads["features"] = z(Ft)
    torch.cuda.synchronize()
    return dict(out=out, map=dmap, fmap=fmap, grads=grads, leaves=leaves, m2=m2, sink=sink, rs=rs)


def _check_map(got, ref, amb, what):
    a, r = MAP_BAR
    ok = ~amb
    err = np.abs(got - ref)[ok]
    tol = 4.0 * (a * np.abs(ref[ok]).max() + r * np.abs(ref[ok]))
    print(f"{what}: map max|err| {err.max():.3e} max|ref| {np.abs(ref[ok]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
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
        assert np.abs(want).max() > 0 or n in ("shs", "features_dc", "features_rest"), (what, n)
        assert (err <= tol).all(), (what, n, float(err.max()), float(np.abs(want).max()), ratio)
    print(f"{what}: worst gradient err / bar {worst[1]:.3f} ({worst[0]})")


# ---- 1. against the fp64 reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(dm.VARIANTS))
@pytest.mark.parametrize("name", list(cm.CASES))
def test_against_the_fp64_reference(name, variant, rast, gpu):
    """return_aux: the loss is on the map, the colour, acc_depth and alpha together, so float 9 of the records receives both its parts."""
    r = dm.reference(name, variant)
    r64, r32 = r["r64"], r["r32"]
    assert r64["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    h = _render(rast, gpu, r["sc"], r["cam"], aa=r["aa"], raw=r["raw"], aux=r["aux"], g=r64["g"])
    assert np.array_equal(h["out"][1].cpu().numpy() > 0, r64["vis"]), "radius decision differs: pick another seed"
    assert tuple(h["map"].shape) == r64["amb"].shape and len(h["out"]) == (6 if r["aux"] else 4)
    what = f"case {name}, {variant}"
    got = _np(h["map"])
    _check_map(got, r64["map"], r64["amb"], what)
    _check_grads(h["grads"], r64["grads"], r32["grads"], what)
    # fewer than two contributors: exactly 0; nowhere negative beyond rounding, nowhere NaN (ragged border pixels included)
    lone = (r64["n_live"] < 2) & ~r64["amb"]
    assert (got[lone] == 0.0).all() and (name == "a" or lone.mean() > 0.4)
    assert got.min() >= -4.0 * MAP_BAR[0] * r64["map"].max()


# ---- 2. composition -------------------------------------------------------------------------------------------------------------------------
def test_with_features_the_gradients_are_the_sum_of_both_losses(rast, gpu):
    """loss = sum feature_map g1 + sum color g0 (features_math's reference) + sum distort gd (distort_math's, without the colour): the
    gradients are the fp64 sum; both between-phase calls ran."""
    _C = rast._C
    rf, rd = fm.reference("a", 19), dm.reference("a", "plain", colour_loss=False)
    assert np.array_equal(rf["r64"]["amb"], rd["r64"]["amb"])
    g = dict(rd["r64"]["g"], g0=rf["r64"]["g0"])
    _C.set_option("profile", -1)
    try:
        _C.profile_reset()
        h = _render(rast, gpu, rd["sc"], rd["cam"], F=rf["F"], g=g, g1=rf["r64"]["g1"])
        prof = _C.profile_read()
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()
    assert all(prof[k][1] == 1 for k in ("features_fwd", "features_bwd", "distort_fwd", "distort_bwd", "blend_bwd"))
    assert len(h["out"]) == 5 and tuple(h["fmap"].shape) == (19, 45, 70) and tuple(h["map"].shape) == (45, 70)
    _check_map(_np(h["map"]), rd["r64"]["map"], rd["r64"]["amb"], "with features")
    alone = _render(rast, gpu, rd["sc"], rd["cam"])
    assert torch.equal(h["map"], alone["map"])
    want64 = {n: rf["r64"]["grads"][n] + rd["r64"]["grads"][n] for n in rd["r64"]["grads"]}
    want32 = {n: rf["r32"]["grads"][n] + rd["r32"]["grads"][n] for n in rd["r32"]["grads"]}
    want64["features"], want32["features"] = rf["r64"]["grads"]["features"], rf["r32"]["grads"]["features"]
    _check_grads(h["grads"], want64, want32, "features + distortion")
    for n in ("means2D", "opacities", "means3D"):      # neither part is negligible: overwriting instead of adding would show
        tol = grad_tol(want64[n].reshape(h["grads"][n].shape))
        assert (np.abs(rd["r64"]["grads"][n]).reshape(tol.shape) > 100 * tol).any() and (np.abs(rf["r64"]["grads"][n]).reshape(tol.shape) > 100 * tol).any(), n


@pytest.mark.parametrize("exp_mode", [1, 2])
def test_with_features_in_the_other_exp_modes(exp_mode, rast, gpu):
    """Device against device under exp_mode 1 / 2 (the fp64 references belong to mode 0 and only scale the gradient bar): the map beside 19
    feature channels is the map alone, bit for bit and from run to run; the gradients of the three-part loss of the test above are the sum
    of the feature-and-colour loss's and the distortion loss's; one launch of each of the four kernels."""
    _C = rast._C
    rf, rd = fm.reference("a", 19), dm.reference("a", "plain", colour_loss=False)
    g = dict(rd["r64"]["g"], g0=rf["r64"]["g0"])
    sc, cam = rd["sc"], rd["cam"]
    _C.set_option("exp_mode", exp_mode)
    try:
        _C.set_option("profile", -1)
        try:
            _C.profile_reset()
            both = _render(rast, gpu, sc, cam, F=rf["F"], g=g, g1=rf["r64"]["g1"])
            prof = _C.profile_read()
        finally:
            _C.set_option("profile", 0)
            _C.profile_reset()
        again = _render(rast, gpu, sc, cam, F=rf["F"])
        alone = _render(rast, gpu, sc, cam)
        feat = _render(rast, gpu, sc, cam, F=rf["F"], g=dict(g0=g["g0"]), g1=rf["r64"]["g1"])
        dist = _render(rast, gpu, sc, cam, F=rf["F"], g=dict(gd=g["gd"]), colour_loss=False)
    finally:
        _C.set_option("exp_mode", 0)
    assert all(prof[k][1] == 1 for k in ("features_fwd", "features_bwd", "distort_fwd", "distort_bwd"))
    assert not torch.isnan(both["map"]).any() and float(both["map"].detach().max()) > 0
    assert torch.equal(both["map"], alone["map"]) and torch.equal(both["map"], again["map"]) and torch.equal(both["fmap"], again["fmap"])
    assert not dist["grads"]["features"].any()
    worst = ("", 0.0)
    for n in both["grads"]:
        s = feat["grads"][n] + dist["grads"][n]
        w64 = rf["r64"]["grads"][n] + (rd["r64"]["grads"][n] if n in rd["r64"]["grads"] else 0.0)
        w32 = rf["r32"]["grads"][n] + (rd["r32"]["grads"][n] if n in rd["r32"]["grads"] else 0.0)
        tol = grad_tol(w64.reshape(s.shape), w32.reshape(s.shape))
        ratio = float((np.abs(both["grads"][n] - s) / np.maximum(tol, 1e-300)).max())
        worst = max(worst, (n, ratio), key=lambda x: x[1])
        assert np.abs(feat["grads"][n]).max() > 0 or n == "shs", n
        assert (np.abs(both["grads"][n] - s) <= tol).all(), (n, ratio)
    print(f"exp_mode {exp_mode}: features + distortion, worst gradient |both - (feat + dist)| / bar {worst[1]:.3f} ({worst[0]})")
    for n in ("means2D", "opacities", "means3D"):      # neither part is negligible: overwriting instead of adding would show
        tol = grad_tol(rd["r64"]["grads"][n].reshape(both["grads"][n].shape))
        assert (np.abs(both["grads"][n] - feat["grads"][n]) > 100 * tol).any() and (np.abs(both["grads"][n] - dist["grads"][n]) > 100 * tol).any(), n


def test_camera_gradients_of_a_distortion_only_loss(rast, gpu):
    """viewmatrix.grad / projmatrix.grad of sum distort gd against the restated renderer with the camera as leaves, fp64; bar grad_tol(want, its
    float32 evaluation).  The path through z (float 9 of the records -> the per-Gaussian backward's dV) is the new part."""
    r = dm.reference("a", "plain", colour_loss=False)
    sc, cam, g = r["sc"], r["cam"], r["r64"]["g"]
    want = dm.camera_reference(sc, cam, g)
    rs = settings_from(rast, cam, sc, gpu)
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True))
    _render(rast, gpu, sc, cam, g=g, colour_loss=False, camera=True, rs=rs)
    for n, x in (("viewmatrix", rs.viewmatrix), ("projmatrix", rs.projmatrix)):
        w64 = want[torch.float64][n]
        err = np.abs(_np(x.grad) - w64)
        tol = grad_tol(w64, want[torch.float32][n])
        print(f"camera {n}: max|want| {np.abs(w64).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
        assert np.abs(w64).max() > 0 and (err <= tol).all(), (n, float(err.max()))
    assert np.abs(want[torch.float64]["viewmatrix"][:, 2]).max() > 0      # (the z column: what only dL/dz reaches)


def test_contrib_sink_and_no_grad(rast, gpu):
    r = dm.reference("b")
    sc, cam = r["sc"], r["cam"]
    w = _render(rast, gpu, sc, cam, contrib=True)
    wo = _render(rast, gpu, sc, cam, contrib=True, distortion=False)
    assert torch.equal(w["sink"], wo["sink"]) and not torch.isnan(w["sink"]).any() and bool(w["sink"].any())
    with torch.no_grad():
        ng = _render(rast, gpu, sc, cam)
    ref = _render(rast, gpu, sc, cam, g=r["r64"]["g"])
    assert torch.equal(ng["map"], ref["map"]) and not ng["map"].requires_grad and ref["map"].requires_grad
    again = _render(rast, gpu, sc, cam)
    assert torch.equal(again["map"], ref["map"])          # bit-identical between two runs of the same state


def test_empty_scene_and_one_pixel(rast, gpu, scenes):
    r = dm.reference("b")
    sc0 = {k: (v[:0] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in r["sc"].items()}
    g = dict(gd=np.ones((45, 70), np.float32), g0=np.ones((3, 45, 70), np.float32))
    h = _render(rast, gpu, sc0, r["cam"], g=g)
    assert tuple(h["map"].shape) == (45, 70) and not h["map"].any()
    cam1 = scenes.camera(1, 6, 1, 1)
    sc = scenes.synth(50, 3, scale_mul=3.0)
    a = _render(rast, gpu, sc, cam1, g=dict(gd=np.ones((1, 1), np.float32)), colour_loss=False)
    assert tuple(a["map"].shape) == (1, 1) and bool(torch.isfinite(a["map"]).all()) and float(a["map"].detach()) > 0
    assert all(np.isfinite(v).all() for v in a["grads"].values()) and np.abs(a["grads"]["means3D"]).max() > 0


# ---- 3. invariance under a shift along the view axis ------------------------------------------------------------------------------------------
def test_shift_along_the_view_axis(rast, gpu):
    """Scene and camera translated together by s = 4 along the camera's view axis (the scene lies at view depths 2.5 ... 6, so its world
    coordinates roughly double): the map stays what it was, within the file's bar.  The device's map of the MOVED scene is held to the fp64
    reference of the UNMOVED one at MAP_BAR, on the pixels unambiguous in both; so is the moved scene's own fp64 reference (what the float32
    rounding of the moved inputs alone does: 1.3e-7 of the map's maximum on the CPU, worst err / bar 0.014), and so is the device's map of
    the moved scene against the device's map of the unmoved one."""
    r = dm.reference("a")
    sc, cam, r64 = r["sc"], r["cam"], r["r64"]
    s = 4.0
    V = np.asarray(cam["viewmatrix"], np.float64)
    axis = V[:3, 2] / np.linalg.norm(V[:3, 2])                  # the world direction whose view-space image is +z
    proj = np.linalg.inv(V) @ np.asarray(cam["projmatrix"], np.float64)
    V2 = V.copy()
    V2[3, :] = V[3, :] - (s * axis) @ V[:3, :]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    cam2 = dict(cam, viewmatrix=f32(V2), projmatrix=f32(V2 @ proj), campos=f32(np.asarray(cam["campos"], np.float64) + s * axis))
    sc2 = dict(sc, means3D=f32(sc["means3D"].astype(np.float64) + s * axis))
    moved = dm.evaluate64(sc2, cam2, colour_loss=False)
    amb = moved["amb"] | r64["amb"]                             # compared where neither scene has an fp32-ambiguous decision
    assert amb.mean() < 0.05
    _check_map(moved["map"], r64["map"], amb, "moved fp64 reference against the unmoved one")
    h = _render(rast, gpu, sc2, cam2)
    h0 = _render(rast, gpu, sc, cam)
    assert np.array_equal(h["out"][1].cpu().numpy() > 0, r64["vis"])
    _check_map(_np(h["map"]), r64["map"], amb, "device, moved by 4 along the view axis, against the unmoved fp64 reference")
    _check_map(_np(h["map"]), _np(h0["map"]), amb, "device, moved against unmoved")


# ---- 4. nothing else moved ------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moved(rast, gpu):
    """distortion=False and the keyword absent: the same tuple, the same launches, outputs bit for bit.  A backward after a distortion=True
    forward whose map got no gradient is the plain backward: no distort_bwd, no GSRAST_RENDER_AUX (the plain blend backward's launch count).
    Gradients: at grad_tol of the fp64 gradient (module docstring: float atomics)."""
    _C = rast._C
    r = dm.reference("a")
    sc, cam, r64 = r["sc"], r["cam"], r["r64"]
    g = {k: v for k, v in r64["g"].items() if k != "gd"}          # a loss on the colour alone
    counts = []
    _C.set_option("profile", -1)
    try:
        runs = []
        for kw in (dict(absent=True), dict(distortion=False), dict(distortion=True)):
            _C.profile_reset()
            runs.append(_render(rast, gpu, sc, cam, g=g, **kw))
            prof = _C.profile_read()
            counts.append({k: prof[k][1] for k in prof})
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()
    absent, off, on = runs
    assert counts[0] == counts[1] and counts[0]["distort_fwd"] == 0 and counts[0]["distort_bwd"] == 0
    assert counts[2] == dict(counts[0], distort_fwd=1), {k: (counts[0][k], counts[2][k]) for k in counts[0] if counts[0][k] != counts[2][k]}
    assert len(absent["out"]) == len(off["out"]) == 3 and len(on["out"]) == 4
    for a, b, c in zip(absent["out"], off["out"], on["out"]):
        assert torch.equal(a, b) and torch.equal(a, c)
    want = dm.evaluate64(sc, cam, g=dict(r64["g"], gd=np.zeros_like(r64["g"]["gd"])))["grads"]
    exact = True
    for n in absent["grads"]:
        tol = grad_tol(want[n].reshape(absent["grads"][n].shape))
        for other in (off, on):
            exact = exact and np.array_equal(other["grads"][n], absent["grads"][n])
            assert (np.abs(other["grads"][n] - absent["grads"][n]) <= tol).all(), n
        assert np.abs(absent["grads"][n]).max() > 0, n
    print(f"nothing else moved: the three backwards' gradients are {'bit-equal' if exact else 'equal at the bar, not bit for bit (float atomics)'}")
