"""CPU: camera-pose gradients (include/gsrast.h: GSRAST_RENDER_POSEGRAD, dL_dcamera / pose_scratch of gsrast_backward_call;
`camera_grads=` of the Python package).  tests/posegrad_math.py -- the fp64 renderer with the camera as leaf tensors that
tests/test_gpu_posegrad.py compares the kernels with -- is pinned to tests/math_renderer.py, satisfies the identities the function
itself implies and agrees with finite differences; the scratch size is declared, exported and bound, the backward's plan reports the
decision and every refusal is produced before any device work; the package knows the keyword."""
import ctypes as C

import numpy as np
import pytest
import torch

import math_renderer as mr
import capi_records as cr
import posegrad_math as pm
import test_gpu_independent as tgi


def _case(letter):
    return next(c for c in tgi.CASES if c["name"].startswith(letter + "_"))


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / max(float(np.abs(np.asarray(want)).max()), 1e-300)


# ---- 1. the helper is pinned to the independent renderer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", tgi.CASES, ids=lambda c: c["name"])
def test_helper_equals_the_math_renderer_with_constant_cameras(c, scenes):
    """Colour and every leaf gradient of the six cases, 1e-10 relative (both are fp64 evaluations of one function, written twice)."""
    r = tgi._reference(scenes, c)
    sc, cam, names = r["sc"], r["cam"], r["names"]
    e = pm.evaluate(sc, cam, names, pm.cfg_of(cam, sc, c), c, upstream_grads=(r["g"], None, None))
    assert np.array_equal(e["out"]["vis"], r["out"]["proj"]["disc"]["vis"])
    assert _rel(e["out"]["color"].detach().numpy(), r["out"]["color"].detach().numpy()) <= 1e-10
    assert _rel(e["out"]["alpha"].detach().numpy(), 1.0 - r["out"]["final_T"].detach().numpy()) <= 1e-10
    for n in names:
        assert float(np.abs(r["want"][n]).max()) > 0.0
        assert _rel(e["want"][n], r["want"][n]) <= 1e-10, n
    # the Gaussians' own terms add up to the camera's gradient
    for k in pm.CAMERA:
        assert _rel(e["terms"][k].sum(axis=0), e["want"][k]) <= 1e-10 or not e["want"][k].any()


def test_one_projection_and_one_pair_loop_under_every_helper(scenes):
    """contrib_math's case a (700 Gaussians, 70 x 45, ragged tiles, frustum-clamped and colour-clamped rows).  (a) project_gaussians +
    blend_pairs deciding, then replaying their own decisions: bit-equal outputs and leaf gradients; (b) a float32 replay rewrites no decision;
    (c) the adapters -- mr.render, pm.render without per-Gaussian camera copies, dm.blend, contrib_math's weights -- agree on `live` and on
    the weights EXACTLY: they are one function now, which the tolerances of the pins above could not say of four copies."""
    import contrib_math as cm
    import distort_math as dm
    sc, cam = cm.case_scene(scenes, cm.CASES["a"])
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    cfg = pm.cfg_of(cam, sc)
    W, H = cfg["W"], cfg["H"]
    rng = np.random.default_rng(41)
    maps = ("color", "acc_depth", "alpha")
    up = [torch.as_tensor(rng.normal(size=s)) for s in ((3, H, W), (H, W), (H, W))]
    same = lambda a, b: np.array_equal(a.detach().numpy(), b.detach().numpy(), equal_nan=True)      # noqa: E731  (rows behind the camera hold NaN)

    def run(dtype, D):
        t, cams = pm.tensors(sc, names, dtype), pm.camera_leaves(cam, dtype)
        pr = mr.project_gaussians(t, *cams, cfg, decisions=D)
        bl = mr.blend_pairs(pr["sorted"], cfg["bg"], W, H, decisions=D)
        sum((bl[k] * g.to(dtype)).sum() for k, g in zip(maps, up)).backward()
        return pr, bl, {n: x.grad for n, x in (*t.items(), *zip(pm.CAMERA, cams))}

    pr0, bl0, g0 = run(torch.float64, None)
    D = {**pr0["decisions"], **bl0["decisions"]}
    assert pr0["disc"]["clamped"].any() and not D["colpos"][D["idx"]].all()      # frustum-clamped rows, colour channels clamped at zero
    assert (D["ok"] & ~D["live"]).any() and (D["listed"] & ~D["ok"]).any()      # pixels ended by the T stop, listed pairs that are skipped
    held = {k: (v, v.clone()) for k, v in D.items()}
    pr1, bl1, g1 = run(torch.float64, D)
    for k in ("pix", "conic", "depth", "o", "col"):
        assert same(pr0[k], pr1[k]), k
    for k in maps + ("w", "T_incl", "T_excl", "T_final", "power", "alpha_raw", "live", "ok", "listed"):
        assert same(bl0[k], bl1[k]), k
    for n in g0:
        assert g0[n] is not None and g0[n].any() and same(g0[n], g1[n]), n
    run(torch.float32, D)
    assert D.keys() == held.keys()
    for k, (v, copy) in held.items():
        assert D[k] is v and torch.equal(v, copy), k
    with torch.no_grad():
        t = pm.tensors(sc, names, grad=False)
        cams = pm.camera_leaves(cam)
        ref = mr.render(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], cfg["deg"], cam, sc["bg"])
        g = dm.project(t, *cams, cfg, {})
        others = dict(posegrad=pm.render(t, *cams, cfg, per=False), contrib=cm.pairs(sc, cam)[0],
                      distort=dm.blend(g["pix"], g["conic"], g["o"], g["z"], g["col"], cfg["bg"], g["rect"], W, H))
    assert ref["live"].any(dim=1).sum() > 0.5 * W * H
    for n, o in others.items():
        assert torch.equal(o["live"], ref["live"]) and torch.equal(o["w"], ref["w"]), n
    assert torch.equal(bl0["w"], ref["w"])


# ---- 2. identities of the function itself ------------------------------------------------------------------------------------------------
def _translation_sides(want, cam):
    V, Pm_ = np.asarray(cam["viewmatrix"], np.float64), np.asarray(cam["projmatrix"], np.float64)
    lhs = want["means3D"].sum(axis=0)
    rhs = V[:3, :] @ want["viewmatrix"][3, :] + Pm_[:3, :] @ want["projmatrix"][3, :] - want["campos"]
    return lhs, rhs


@pytest.mark.parametrize("aux,aa", [(False, False), (True, True)], ids=["plain", "aux_antialiased"])
def test_translation_identity(scenes, aux, aa):
    """Moving every Gaussian by d is moving the camera by -d: sum_i dL/dmeans3D_i[k] = sum_c V[k,c] dV[3,c] + sum_c Pm[k,c] dPm[3,c] - dcampos[k],
    with SH colours (the campos term), the aux outputs and the anti-aliasing factor."""
    c = _case("b")
    sc, cam, names = tgi._case_inputs(scenes, c)
    e = pm.evaluate(sc, cam, names, pm.cfg_of(cam, sc, c, aa=aa), c, aux=aux)
    lhs, rhs = _translation_sides(e["want"], cam)
    assert float(np.abs(e["want"]["campos"]).max()) > 0.0 and float(np.abs(lhs).max()) > 0.0
    scale = float(np.abs(e["terms"]["viewmatrix"][:, 3, :]).sum())      # (what the sums are made of: they may cancel)
    assert float(np.abs(lhs - rhs).max()) <= 1e-9 * scale, (lhs, rhs)


def test_rotation_identity(scenes):
    """colors_precomp + cov3D_precomp: rotating the world by I + eps G (G antisymmetric) -- means m @ (I + eps G), covariances
    (I + eps G)^T S (I + eps G) -- is replacing rows 0-2 of viewmatrix and projmatrix by (I + eps G) @ rows: the two first-order changes
    of the loss agree for the three generators."""
    c = _case("d")
    sc, cam, names = tgi._case_inputs(scenes, c)
    e = pm.evaluate(sc, cam, names, pm.cfg_of(cam, sc, c), c, aux=True)
    w = e["want"]
    V, Pm_ = np.asarray(cam["viewmatrix"], np.float64), np.asarray(cam["projmatrix"], np.float64)
    m, c6 = np.asarray(sc["means3D"], np.float64), np.asarray(sc["cov3D"], np.float64)
    S = np.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(-1, 3, 3)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        G = np.zeros((3, 3)); G[i, j], G[j, i] = 1.0, -1.0
        dS = G.T @ S + S @ G
        d6 = np.stack([dS[:, 0, 0], dS[:, 0, 1], dS[:, 0, 2], dS[:, 1, 1], dS[:, 1, 2], dS[:, 2, 2]], 1)
        scene = float((w["means3D"] * (m @ G)).sum() + (w["cov3D"] * d6).sum())
        camera = float((w["viewmatrix"][:3] * (G @ V[:3])).sum() + (w["projmatrix"][:3] * (G @ Pm_[:3])).sum())
        scale = float(np.abs(w["means3D"] * (m @ G)).sum() + np.abs(w["cov3D"] * d6).sum())
        assert abs(scene) > 1e-6 * scale and abs(scene - camera) <= 1e-9 * scale, (scene, camera)


def test_structural_zeros(scenes):
    """The forward never reads column 3 of viewmatrix or column 2 of projmatrix, and with degree 0 / precomputed colours not campos."""
    for letter in ("b", "d", "e"):
        c = _case(letter)
        sc, cam, names = tgi._case_inputs(scenes, c)
        e = pm.evaluate(sc, cam, names, pm.cfg_of(cam, sc, c), c)
        assert not e["want"]["viewmatrix"][:, 3].any() and not e["want"]["projmatrix"][:, 2].any()
        assert e["want"]["viewmatrix"][:, :3].all() and e["want"]["projmatrix"][:, [0, 1, 3]].all()
        assert e["want"]["campos"].any() == (c["deg"] > 0)


# ---- 3. finite differences ---------------------------------------------------------------------------------------------------------------
def test_helper_agrees_with_central_finite_differences(scenes):
    """20 Gaussians, none frustum-clamped, no ambiguous pixel, clamp_grad="true" (the forward differentiated as written): all 35 entries
    against (L(x + h) - L(x - h)) / 2h in fp64 on the discrete decisions of the unperturbed pass (the function is smooth inside one
    cell of its decisions; h = 1e-5 would flip some alpha >= 1/255 test otherwise, a jump no derivative describes).  Bar: 1e-6 of the
    tensor's largest entry -- truncation h^2 f''' / 6 ~ 1e-10 relative and rounding eps |L| / h ~ 1e-11 |L| are both far below it, a
    missing or halved term far above."""
    c = dict(P=20, seed=5, W=32, H=32, k=1, V=5, deg=3, smul=1.0, bg=(0.2, 0.1, 0.3))
    sc = scenes.synth(c["P"], c["seed"], sh_degree=3)
    sc["bg"] = np.array(c["bg"], np.float32)
    cam = scenes.camera(c["k"], c["V"], c["W"], c["H"])
    names = ["means3D", "opacities", "shs", "scales", "rotations"]
    cfg = pm.cfg_of(cam, sc, c, aa=True)
    e = pm.evaluate(sc, cam, names, cfg, c, aux=True, clamp_grad="true")
    assert not e["amb"].any() and not e["out"]["clamped"].any() and e["out"]["vis"].sum() >= 10 and e["out"]["n_live"].max() >= 3
    t = pm.tensors(sc, names, grad=False)
    base = [np.asarray(cam[k], np.float64) for k in pm.CAMERA]

    def L(k, idx, h):
        arrs = [b.copy() for b in base]
        arrs[k][idx] += h
        with torch.no_grad():
            out = pm.render(t, *[torch.as_tensor(a) for a in arrs], cfg, decisions=e["out"]["decisions"], clamp_grad="true")
            return float(pm.loss_of(out, e["g"], e["gD"], e["gA"]))

    h = 1e-5
    for k, name in enumerate(pm.CAMERA):
        want = e["want"][name]
        fd = np.zeros_like(want)
        for idx in np.ndindex(want.shape):
            fd[idx] = (L(k, idx, h) - L(k, idx, -h)) / (2 * h)
        assert float(np.abs(want).max()) > 0.0
        assert float(np.abs(fd - want).max()) <= 1e-6 * float(np.abs(want).max()), (name, fd, want)


# ---- 4. without a device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_symbols_are_declared_exported_and_bound(rast, L):
    """(The record's pose fields and the flag's value: tests/test_capi_abi.py.)"""
    assert rast._C.CAMERA_FLOATS == 35
    # one 128-byte row per workgroup of the larger grid (128 Gaussians each); the state buffers do not grow with the feature
    assert [L.gsrast_pose_scratch_bytes(p) for p in (1, 128, 129, 1500)] == [128, 128, 256, 12 * 128]
    assert L.gsrast_pose_scratch_bytes(0) > 0


def _plan_fn(rast):
    fn = C.CDLL(rast._C.LIB_PATH).gsrast_debug_backward_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(rast._C.OptionsStruct), C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return fn


def test_backward_plan_reports_the_pose_sums(L, rast):
    _C = rast._C
    POSE, AUX, AA = _C.RENDER_POSEGRAD, _C.RENDER_AUX, _C.RENDER_ANTIALIAS
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    fn, err = _plan_fn(rast), L.gsrast_last_error
    SYM, OUT, SCR = 32, 64, 128
    for kind in (2, 2 | 1, 4 | 8):      # SH dense, SH raw, precomputed colour + covariance
        for extra in (0, AA, AUX):
            for phase in (0, 1, 2):
                opts.backward_phase = phase
                base = (C.c_int * 7)(1000, 3, 5000, 64, 64, kind | (16 if extra == AUX else 0), 1)
                full = (C.c_int * 7)(1000, 3, 5000, 64, 64, kind | (16 if extra == AUX else 0) | SYM | OUT | SCR, 1)
                plain, sym, pose = fn(C.byref(opts), extra, base, None), fn(C.byref(opts), extra, (C.c_int * 7)(*base[:5], base[5] | SYM, 1), None), fn(C.byref(opts), extra | POSE, full, None)
                assert plain >= 0 and not plain & (1 << 28)
                assert sym == plain                           # the longer record without the bit and with NULL pointers IS the shorter one's call
                assert pose == plain | (1 << 28)              # bit 28, and no other decision moves
    opts.backward_phase = 0
    # the refusals, one text each, before any device work
    w = lambda bits: (C.c_int * 7)(1000, 3, 5000, 64, 64, 2 | bits, 1)      # noqa: E731
    assert fn(C.byref(opts), POSE, w(0), None) == -1 and err() == b"flags: unknown bits"
    assert fn(C.byref(opts), POSE, w(SYM | SCR), None) == -1 and b"GSRAST_RENDER_POSEGRAD with a NULL dL_dcamera" in err()
    assert fn(C.byref(opts), POSE, w(SYM | OUT), None) == -1 and b"GSRAST_RENDER_POSEGRAD with a NULL pose_scratch" in err()
    for bits in (SYM | OUT, SYM | SCR, SYM | OUT | SCR):
        assert fn(C.byref(opts), 0, w(bits), None) == -1 and b"without GSRAST_RENDER_POSEGRAD" in err()
    assert fn(C.byref(opts), POSE | 0x10, w(SYM | OUT | SCR), None) == -1 and b"unknown bits" in err()


def test_bad_arguments_fail_before_any_device_work(L, rast):
    """The same refusals through the exported entry point (pointers that would fault if anything touched them)."""
    _C = rast._C
    one = cr.ONE
    AA, ABS, POSE = _C.RENDER_ANTIALIAS, _C.RENDER_ABSGRAD, _C.RENDER_POSEGRAD
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))

    def call(family, size, P, flags, sink=None, camera=None, scratch=None):
        return cr.call(cr.backward(P, flags, family, size=size, dL_dmean2D_abs=sink, dL_dcamera=camera, pose_scratch=scratch), opts)

    for family in ("dense", "raw"):
        for fl in (POSE, POSE | AA):
            rc, err = call(family, "full", 10, fl, None, None, one)
            assert rc == -1 and b"NULL dL_dcamera" in err
            rc, err = call(family, "full", 10, fl, None, one, None)
            assert rc == -1 and b"NULL pose_scratch" in err
            # every shorter record refuses the bit as an unknown one
            for size in ("min", "abs"):
                rc, err = call(family, size, 10, fl)
                assert rc == -1 and b"unknown bits" in err
        for fl in (0, AA):
            for scratch in (one, None):
                rc, err = call(family, "full", 10, fl, None, one, scratch)
                assert rc == -1 and b"without GSRAST_RENDER_POSEGRAD" in err
        # the absgrad rules hold on the full record
        rc, err = call(family, "full", 10, POSE | ABS, None, one, one)
        assert rc == -1 and b"NULL dL_dmean2D_abs" in err
        rc, err = call(family, "full", 10, POSE, one, one, one)
        assert rc == -1 and b"without GSRAST_RENDER_ABSGRAD" in err
        rc, err = call(family, "full", 10, POSE | 0x10, None, one, one)
        assert rc == -1 and b"unknown bits" in err
        # a good combination reaches the ordinary checks (here: the negative P), with and without the bit
        rc, err = call(family, "full", -1, POSE, None, one, one)
        assert rc == -1 and b"POSEGRAD" not in err and b"unknown bits" not in err
        rc, err = call(family, "full", -1, 0)
        assert rc == -1 and b"POSEGRAD" not in err
        assert call(family, "full", 0, 0)[0] == 0      # nothing to do, no device touched
    # no forward knows the bit
    rc, err = cr.call(cr.forward(10, POSE), opts)
    assert rc == -1 and b"unknown bits" in err


def test_the_package_knows_the_keyword(rast):
    """camera_grads is keyword-only, defaults to False, is rejected nowhere, and without a camera tensor that requires grad adds nothing
    to the autograd node's inputs.  The settings tuple keeps the reference's 11 fields."""
    import inspect
    assert len(rast.GaussianRasterizationSettings._fields) == 11
    p = inspect.signature(rast.rasterize_gaussians).parameters["camera_grads"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for fn in (rast._C.rasterize_gaussians_backward, rast._C.rasterize_gaussians_raw_backward):
        q = inspect.signature(fn).parameters["camera_grads"]
        assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default is False
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):
        assert fn.__kwdefaults__ == {"return_aux": False}
    P, cpu = 5, torch.device("cpu")
    mk = lambda V: rast.GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, V, torch.eye(4), 0, torch.zeros(3), False)      # noqa: E731
    rs, rq = mk(torch.eye(4)), mk(torch.eye(4, requires_grad=True))
    request = lambda settings, **kw: rast._parse_request(settings, P, cpu, **kw)      # noqa: E731  ((the record, the node's four trailing inputs))
    assert request(rq)[0].camera is False and request(rq, camera_grads=1)[0].camera is True
    assert request(rq, camera_grads=True)[0].antialiasing is False      # (the check of unknown keywords lets it through)
    with pytest.raises(TypeError):
        request(rq, camera_grad=True)
    # no settings tensor requires grad: no camera request, whatever camera_grads says -- the plain call
    for settings, flag in ((rs, True), (rs, False), (rq, False)):
        req, slots = request(settings, camera_grads=flag)
        assert req.camera is False and slots == (None, None, None, None)
    req, got = request(rq, camera_grads=True)
    assert req.camera is True and len(got) == 4 and got[0] is None and got[1] is rq.viewmatrix and got[2] is rq.projmatrix and got[3] is rq.campos
    # through the public entry points the keyword gets as far as the device check (no GPU in this test), in all three places
    m3, m2, op = torch.zeros((P, 3)), torch.zeros((P, 3)), torch.zeros((P, 1))
    e = torch.empty(0)
    for rset in (rs, rq):
        for kw in (dict(), dict(camera_grads=False), dict(camera_grads=True)):
            with pytest.raises(RuntimeError, match="GPU"):
                rast.rasterize_gaussians(m3, m2, e, torch.zeros((P, 3)), op, torch.ones((P, 3)), torch.ones((P, 4)), e, rset, **kw)
            with pytest.raises(RuntimeError, match="GPU"):
                rast.GaussianRasterizer(rset)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), **kw)
            with pytest.raises(RuntimeError, match="GPU"):
                rast.GaussianRasterizerRaw(rset)(m3, m2, torch.ones((P, 4)), torch.zeros((P, 3)), op, torch.zeros((P, 1, 3)), torch.zeros((P, 15, 3)), **kw)
