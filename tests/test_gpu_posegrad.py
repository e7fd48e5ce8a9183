"""-m gpu: camera-pose gradients (camera_grads=True; include/gsrast.h: GSRAST_RENDER_POSEGRAD) of the HIP renderer against
tests/posegrad_math.py, the torch fp64 renderer whose camera is three leaf tensors (pinned to tests/math_renderer.py, to finite
differences and to the function's own identities by tests/test_posegrad_host.py).

Scenes: edge_scenes.edge_scene with the case dicts of tests/test_gpu_independent.py (needles, near-plane Gaussians, Gaussians outside the
frustum clamp); upstream gradients are zero on the fp32-ambiguous pixels.  Bar per camera tensor: conftest.grad_tol(want, ref32) with
ref32 = the helper evaluated in float32 on the fp64 pass's decisions -- what fp32 rounding alone does to a sum of P terms that partly
cancel.  Measured on the CPU (posegrad_math.reference; max|want|, the share max|want| / max sum_i |term_i| that survives the
cancellation, max|ref32 - want| and that as a share of max|want|; grad_tol's own first term is 1e-5 of max|want|):

    case (variant)             tensor       max|want|   max|want| / sum|term|   max|ref32 - want|   / max|want|
    a deg 3, aux gradients     viewmatrix   1.07e+01    0.104                   6.96e-05            6.5e-06
                               projmatrix   3.62e+02    0.420                   1.39e-03            3.8e-06
                               campos       4.04e+00    0.287                   7.59e-06            1.9e-06
    d precomputed, aux off     viewmatrix   8.54e+00    0.270                   5.83e-06            6.8e-07
                               projmatrix   9.92e+00    0.182                   1.01e-05            1.0e-06
    e scale_modifier 0.7, AA   viewmatrix   2.10e+01    0.460                   2.67e-05            1.3e-06
                               projmatrix   9.84e+01    0.571                   9.66e-04            9.8e-06
    b deg 1, raw + residuals   viewmatrix   8.49e+00    0.481                   8.68e-06            1.0e-06
                               projmatrix   7.65e+01    0.791                   4.98e-05            6.5e-07
                               campos       3.98e-01    0.361                   2.52e-07            6.3e-07

(d and e: campos is exactly zero on both sides.)  So 8 x max|ref32 - want| is 0.5 ... 8 x grad_tol's own 1e-5 max|want|: the floor is what
binds for projmatrix of cases a and e (sums of 1500 / 500 terms of either sign), the 1e-5 term elsewhere.  Fewer than 3.4 % of the pixels
are ambiguous in every case, and 29-32 frustum-clamped Gaussians contribute to dL/dviewmatrix.

The sizes of the reduction test are the smallest at which preprocess_bwd_kernel<.., POSE> takes another path: one Gaussian, one workgroup
with an idle lane / full / one lane of a second workgroup (PP_THREADS = 128), several workgroups; each also in the GROUPED form
(option late_fill_min_p = 0), and a camera that sees nothing."""
import numpy as np
import pytest
import torch

import posegrad_math as pm
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu

_device_runs = {}


def _t(a, gpu, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu).requires_grad_(grad)


def _settings(rast, cam, sc, gpu, camera=None, grad=True):
    """The case's settings with the three camera tensors as float32 device leaves (requiring grad unless grad=False)."""
    rs = settings_from(rast, cam, sc, gpu)
    V, Pm, C = camera if camera is not None else (_t(cam["viewmatrix"], gpu, grad), _t(cam["projmatrix"], gpu, grad), _t(cam["campos"], gpu, grad))
    return rs._replace(viewmatrix=V, projmatrix=Pm, campos=C)


def _render(rast, r, rs, gpu, camera_grads, upstream=None):
    """One forward + backward of a reference case on the device.  dict(res = the outputs, leaves, m2)."""
    sc, names = r["sc"], r["names"]
    P = sc["means3D"].shape[0]
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    kw = dict(return_aux=bool(r.get("aux")), antialiasing=bool(r.get("aa")))
    if camera_grads is not None:
        kw["camera_grads"] = camera_grads
    if r.get("raw"):
        t = {n: _t(v, gpu, True) for n, v in r["raw"].items()}
        res = rast.GaussianRasterizerRaw(rs)(t["xyz"], m2, t["rotation"], t["scaling"], t["opacity_logit"], t["features_dc"], t["features_rest"],
                                              motion_residual=t["motion_res"], rot_residual=t["rot_res"], trbfoutput=t["trbf"],
                                              shs_residual=t["shs_res"], **kw)
    else:
        t = {n: _t(sc[n], gpu, True) for n in names}
        a = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"])
        a.update(colors_precomp=t["rgb"], cov3D_precomp=t["cov3D"]) if "rgb" in names else a.update(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
        res = rast.GaussianRasterizer(rs)(**a, **kw)
    g, gD, gA = upstream if upstream is not None else (r["r64"]["g"], r["r64"]["gD"], r["r64"]["gA"])
    loss = (res[0] * torch.from_numpy(g).to(gpu)).sum()
    if gD is not None:
        loss = loss + (res[3][0] * torch.from_numpy(gD).to(gpu)).sum() + (res[4][0] * torch.from_numpy(gA).to(gpu)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return dict(res=res, leaves=t, m2=m2)


def _camera_grads(rs):
    return {k: getattr(rs, k).grad.double().cpu().numpy() for k in pm.CAMERA}


def _device(letter, rast, gpu):
    """The device's camera gradients (+ everything else of the run) for a reference case, once per process."""
    if letter not in _device_runs:
        r = pm.reference(letter)
        rs = _settings(rast, r["cam"], r["sc"], gpu)
        run = _render(rast, r, rs, gpu, True)
        run.update(rs=rs, got=_camera_grads(rs))
        _device_runs[letter] = run
    return _device_runs[letter]


def _assert_structural_zeros(got):
    assert not got["viewmatrix"][:, 3].any() and not got["projmatrix"][:, 2].any()


# ---- 1. parity with the fp64 helper ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ["a", "d", "e", "b"])
def test_camera_gradients_against_the_fp64_helper(letter, rast, gpu):
    r = pm.reference(letter)
    r64, r32 = r["r64"], r["r32"]
    want, terms = r64["want"], r64["terms"]
    # non-vacuity
    assert r64["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    cl = r64["out"]["clamped"]
    assert int((np.abs(terms["viewmatrix"][cl]).max(axis=(1, 2)) > 0).sum()) >= 16, "too few frustum-clamped Gaussians contribute to dL/dviewmatrix"
    live = [k for k in pm.CAMERA if k != "campos" or r["c"]["deg"] > 0]
    for k in live:
        mass = float(np.abs(terms[k]).sum(axis=0).max())
        print(f"{letter} {k}: max|want| {np.abs(want[k]).max():.3e}  sum|term| {mass:.3e}  max|ref32 - want| {np.abs(r32['want'][k] - want[k]).max():.3e}")
        assert float(np.abs(want[k]).max()) >= 1e-3 * mass, (k, "the sum has cancelled to noise")
    run = _device(letter, rast, gpu)
    assert np.array_equal(run["res"][1].cpu().numpy() > 0, r64["out"]["vis"]), "radius decision differs: pick another seed"
    got = run["got"]
    for k in pm.CAMERA:
        err = np.abs(got[k] - want[k])
        tol = grad_tol(want[k], r32["want"][k])
        print(f"{letter} {k}: max err {err.max():.3e}  max tol {np.max(tol):.3e}  worst err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all(), (k, float(err.max()), float(np.abs(want[k]).max()))
    _assert_structural_zeros(got)
    if r["c"]["deg"] == 0:
        assert not got["campos"].any()      # exactly zero with colors_precomp or SH degree 0


# ---- 2. the translation identity on the device's own outputs -----------------------------------------------------------------------------
def _translation_sides(w, cam):
    V, Pm_ = np.asarray(cam["viewmatrix"], np.float64), np.asarray(cam["projmatrix"], np.float64)
    return w["means3D"].sum(axis=0), V[:3, :] @ w["viewmatrix"][3, :] + Pm_[:3, :] @ w["projmatrix"][3, :] - w["campos"]


def test_translation_identity_on_the_device(rast, gpu):
    """sum_i dL/dmeans3D_i against the three camera gradients, both from ONE backward (case a: SH, aux gradients).  Each side is judged
    against the fp64 value with the helper's fp32 evaluation of that side as grad_tol's floor."""
    r = pm.reference("a")
    run = _device("a", rast, gpu)
    dev = dict(run["got"], means3D=run["leaves"]["means3D"].grad.double().cpu().numpy())
    truth, truth_rhs = _translation_sides(r["r64"]["want"], r["cam"])
    assert float(np.abs(truth - truth_rhs).max()) <= 1e-9 * float(np.abs(r["r64"]["terms"]["viewmatrix"][:, 3, :]).sum())
    lhs32, rhs32 = _translation_sides(r["r32"]["want"], r["cam"])
    lhs, rhs = _translation_sides(dev, r["cam"])
    print("truth", truth, "device lhs", lhs, "device rhs", rhs, "fp32 lhs", lhs32, "fp32 rhs", rhs32)
    assert (np.abs(lhs - truth) <= grad_tol(truth, lhs32)).all(), (lhs, truth)
    assert (np.abs(rhs - truth) <= grad_tol(truth, rhs32)).all(), (rhs, truth)


# ---- 3. the reduction ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_refs(scenes):
    """The last N rows of case b's edge scene (the frustum-clamped and near-plane Gaussians are its last rows): N -> reference."""
    import test_gpu_independent as tgi
    c = next(k for k in tgi.CASES if k["name"].startswith("b_"))
    sc, cam, names = tgi._case_inputs(scenes, c)
    out = {}
    for n in (1, 127, 128, 129):
        sub = {k: (v[-n:] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == sc["means3D"].shape[0] else v) for k, v in sc.items()}
        cfg = pm.cfg_of(cam, sub, c)
        r64, r32 = pm.reference_pair(sub, cam, names, cfg, c)
        out[n] = dict(c=c, sc=sub, cam=cam, names=names, cfg=cfg, r64=r64, r32=r32)
    return out


@pytest.mark.parametrize("grouped", [False, True], ids=["plain_launch", "grouped_launch"])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 1500])
def test_the_reduction_at_every_size(n, grouped, small_refs, rast, gpu):
    r = pm.reference("a") if n == 1500 else small_refs[n]
    assert r["sc"]["means3D"].shape[0] == (1532 if n == 1500 else n)      # (case a: P = 1500 + the edge rows)
    assert r["r64"]["out"]["vis"].any() and float(np.abs(r["r64"]["want"]["viewmatrix"]).max()) > 0.0
    keep = rast._C.get_option("late_fill_min_p")
    if grouped:
        rast._C.set_option("late_fill_min_p", 0)
    try:
        rs = _settings(rast, r["cam"], r["sc"], gpu)
        _render(rast, r, rs, gpu, True)
    finally:
        rast._C.set_option("late_fill_min_p", keep)
    got = _camera_grads(rs)
    for k in pm.CAMERA:
        err = np.abs(got[k] - r["r64"]["want"][k])
        assert (err <= grad_tol(r["r64"]["want"][k], r["r32"]["want"][k])).all(), (k, n, float(err.max()), float(np.abs(r["r64"]["want"][k]).max()))
    _assert_structural_zeros(got)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain_launch", "grouped_launch"])
def test_a_camera_that_sees_nothing_gets_exact_zeros(grouped, rast, gpu):
    """Every Gaussian behind the camera: the 35 floats, NaN before the backward, come back exactly zero."""
    r = pm.reference("a")
    cam = dict(r["cam"])
    flip = np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    proj = np.linalg.inv(cam["viewmatrix"].astype(np.float64)) @ cam["projmatrix"].astype(np.float64)
    cam["viewmatrix"] = cam["viewmatrix"] @ flip
    cam["projmatrix"] = (cam["viewmatrix"].astype(np.float64) @ proj).astype(np.float32)
    P = r["sc"]["means3D"].shape[0]
    keep = rast._C.get_option("late_fill_min_p")
    if grouped:
        rast._C.set_option("late_fill_min_p", 0)
    try:
        rs = _settings(rast, cam, r["sc"], gpu)
        rast._C._pose_buffers(P, gpu)[0].fill_(float("nan"))
        run = _render(rast, r, rs, gpu, True)
    finally:
        rast._C.set_option("late_fill_min_p", keep)
    assert not (run["res"][1] > 0).any()
    for k in pm.CAMERA:
        g = getattr(rs, k).grad
        assert g is not None and g.shape == getattr(rs, k).shape and not g.isnan().any() and not g.any(), k


# ---- 4. determinism, no side effects ------------------------------------------------------------------------------------------------------
def test_phase_two_is_deterministic_and_changes_no_other_output(rast, gpu, monkeypatch):
    """Phase 1 (the blend backward) once; then phase 2 (the per-Gaussian backward) twice with the flag and once without, on the same
    gradient records: no atomics anywhere in it, so the camera outputs are bit-equal and so is every other output of the three runs."""
    _C = rast._C
    r = pm.reference("a")
    sc, cam = r["sc"], r["cam"]
    rs = settings_from(rast, cam, sc, gpu)
    t = {n: _t(sc[n], gpu) for n in r["names"]}
    e = torch.empty(0, device=gpu)
    num_rendered, color, radii, geom, binb, img, depth, acc, alpha = _C.rasterize_gaussians(
        rs.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
        rs.image_height, rs.image_width, t["shs"], rs.sh_degree, rs.campos, False, aux=True)
    g, gD, gA = (torch.from_numpy(x).to(gpu) for x in (r["r64"]["g"], r["r64"]["gD"][None], r["r64"]["gA"][None]))

    def backward(phase, **kw):
        monkeypatch.setattr(_C, "_run_backward", lambda ar, call, P, geomBuffer, dev: call(phase))
        out = _C.rasterize_gaussians_backward(rs.bg, t["means3D"], radii, e, t["scales"], t["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix,
                                              rs.tanfovx, rs.tanfovy, g, t["shs"], rs.sh_degree, rs.campos, geom, num_rendered, binb, img,
                                              first_backward=(phase == 1), dL_dacc_depth=gD, dL_dalpha=gA, **kw)
        torch.cuda.synchronize()
        return out

    backward(1, camera_grads=True)
    one, two, plain = backward(2, camera_grads=True), backward(2, camera_grads=True), backward(2)
    assert len(one) == 9 and len(plain) == 8
    for a, b in zip(one[8], two[8]):
        assert a.any() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = r["r64"]["want"]
    for k, a in zip(pm.CAMERA, one[8]):      # (and they are the gradients test 1 judges)
        assert (np.abs(a.double().cpu().numpy() - want[k]) <= grad_tol(want[k], r["r32"]["want"][k])).all(), k
    for i in range(8):
        assert one[i].numel() == plain[i].numel() and (one[i].numel() == 0 or one[i].any())
        assert torch.equal(one[i].view(torch.int32), two[i].view(torch.int32)) and torch.equal(one[i].view(torch.int32), plain[i].view(torch.int32)), i


# ---- 5. autograd --------------------------------------------------------------------------------------------------------------------------
XI = (0.010, -0.020, 0.015, 0.020, -0.010, 0.030)


@pytest.fixture(scope="module")
def pose_ref(scenes):
    """Case b seen from a camera composed from a 6-vector (posegrad_math.compose): the helper's gradient of the 6-vector, fp64 and fp32."""
    import test_gpu_independent as tgi
    c = next(k for k in tgi.CASES if k["name"].startswith("b_"))
    sc, cam, names = tgi._case_inputs(scenes, c)
    cfg = pm.cfg_of(cam, sc, c)
    V0 = np.asarray(cam["viewmatrix"], np.float64)
    proj = np.linalg.inv(V0) @ np.asarray(cam["projmatrix"], np.float64)
    res = {}
    up, dec = None, None
    for dt in (torch.float64, torch.float32):
        xi = torch.tensor(XI, dtype=dt, requires_grad=True)
        V, Pm, C = pm.compose(xi, torch.as_tensor(V0).to(dt), torch.as_tensor(proj).to(dt))
        out = pm.render(pm.tensors(sc, names, dt, grad=False), V, Pm, C, cfg, decisions=dec)
        if up is None:
            up, dec = pm.upstream(c, cfg, out["ambiguous"], False), out["decisions"]
            res["amb"], res["vis"] = out["ambiguous"], out["vis"]
        pm.loss_of(out, *up).backward()
        res[dt] = xi.grad.double().numpy()
    res.update(c=c, sc=sc, cam=cam, names=names, V0=V0, proj=proj, g=up[0])
    return res


def _pose_render(rast, p, gpu, camera_grads, leaf=True):
    xi = torch.tensor(XI, dtype=torch.float32, device=gpu, requires_grad=leaf)
    V, Pm, C = pm.compose(xi, _t(p["V0"], gpu), _t(p["proj"], gpu))
    if not leaf:
        V, Pm, C = V.detach(), Pm.detach(), C.detach()
    rs = _settings(rast, p["cam"], p["sc"], gpu, camera=(V, Pm, C))
    r = dict(sc=p["sc"], names=p["names"])
    run = _render(rast, r, rs, gpu, camera_grads, upstream=(p["g"], None, None))
    run.update(xi=xi)
    return run


def test_autograd_reaches_a_pose_parameter(pose_ref, rast, gpu):
    p = pose_ref
    assert p["amb"].mean() < 0.05
    want, f32 = p[torch.float64], p[torch.float32]
    run = _pose_render(rast, p, gpu, True)
    assert np.array_equal(run["res"][1].cpu().numpy() > 0, p["vis"]), "radius decision differs: pick another seed"
    got = run["xi"].grad.double().cpu().numpy()
    err = np.abs(got - want)
    print("xi.grad", got, "want", want, "fp32", f32)
    assert float(np.abs(want).min()) > 0.0 and (err <= grad_tol(want, f32)).all(), (got, want)
    # camera_grads=False (and the default): the pose gets no gradient, the colour is bit-equal
    for flag in (False, None):
        off = _pose_render(rast, p, gpu, flag)
        assert off["xi"].grad is None
        assert torch.equal(off["res"][0].detach().view(torch.int32), run["res"][0].detach().view(torch.int32))
    # camera_grads=True without a camera tensor that requires grad: the plain call -- the plain node with the plain node's inputs, the
    # same outputs bit for bit, the same per-Gaussian gradients (at the suite's bar: the blend backward's float atomics arrive in
    # another order every run, so no two backwards are bit-equal, with or without the flag)
    plain, same = _pose_render(rast, p, gpu, None, leaf=False), _pose_render(rast, p, gpu, True, leaf=False)
    assert len(same["res"][0].grad_fn.next_functions) == len(plain["res"][0].grad_fn.next_functions) == len(run["res"][0].grad_fn.next_functions) - 3
    for a, b in zip(plain["res"], same["res"]):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    for n in list(p["names"]) + ["m2"]:
        a, b = (x["m2"] if n == "m2" else x["leaves"][n] for x in (plain, same))
        a, b = a.grad.double().cpu().numpy(), b.grad.double().cpu().numpy()
        assert np.array_equal(a == 0, b == 0) and (np.abs(a - b) <= grad_tol(a)).all(), n


# ---- 6. the bar bites ---------------------------------------------------------------------------------------------------------------------
def test_the_bar_bites(rast, gpu):
    """The helper with HALF of the term that reaches viewmatrix through the rotation inside T = J W (posegrad_math: halve="JW"): the
    comparison of test 1 fails against it, for the device's gradient as for the true one."""
    good, bad = pm.reference("a"), pm.reference("a", halve="JW")
    want, wrong = good["r64"]["want"]["viewmatrix"], bad["r64"]["want"]["viewmatrix"]
    tol = grad_tol(wrong, bad["r32"]["want"]["viewmatrix"])
    got = _device("a", rast, gpu)["got"]["viewmatrix"]
    print("worst |true - halved| / tol", float(np.max(np.abs(want - wrong) / tol)), " worst |device - halved| / tol", float(np.max(np.abs(got - wrong) / tol)))
    assert not (np.abs(want - wrong) <= tol).all() and not (np.abs(got - wrong) <= tol).all()
    for k in ("projmatrix", "campos"):      # (the other two tensors do not depend on that term)
        assert np.array_equal(good["r64"]["want"][k], bad["r64"]["want"][k])
