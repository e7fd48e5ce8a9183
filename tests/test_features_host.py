"""CPU: per-Gaussian feature vectors through the blend (include/gsrast.h: gsrast_features_forward / gsrast_features_backward; `features=` of
the Python package) -- the two symbols are declared, exported and bound, the ABI version and the profile table are what they should be,
both calls refuse bad arguments before any device work, the package refuses a bad tensor (ValueError) or an installed GradArena
(RuntimeError) at call time, and the reference of tests/features_math.py is math_renderer.render for three channels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import features_math as fm
from capi_records import ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsrast.h")


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_symbols_are_declared_exported_and_bound(rast, L):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+GSRAST_FEATURES_MAX_C\s+64\b", text) and rast._C.FEATURES_MAX_C == 64
    assert L.gsrast_abi_version() == 6 and re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)      # additive: the version does not move
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert "features_fwd" in names and "features_bwd" in names
    assert len(set(names)) == len(names)


def test_bad_arguments_fail_before_any_device_work(L, rast):
    opts = rast._C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    one = C.c_void_p(ONE)
    err = L.gsrast_last_error

    def fwd(P=10, R=5, Cn=4, W=64, H=48, geom=one, binning=one, img=one, feats=one, out=one, o=C.byref(opts)):
        return L.gsrast_features_forward(o, P, R, Cn, W, H, geom, binning, img, feats, out, None)

    def bwd(P=10, R=5, Cn=4, W=64, H=48, geom=one, binning=one, img=one, feats=one, gmap=one, out=one, o=C.byref(opts)):
        return L.gsrast_features_backward(o, P, R, Cn, W, H, geom, binning, img, feats, gmap, out, None)

    for call, who in ((fwd, b"features_forward"), (bwd, b"features_backward")):
        for Cn in (0, -3, 65, 1 << 20):
            assert call(Cn=Cn) == -1 and who in err() and b"1..64" in err()
        assert call(P=-1) == -1 and who in err() and b"negative" in err()
        assert call(R=-1) == -1 and who in err() and b"negative" in err()
        assert call(W=0) == -1 and who in err() and b"zero-size" in err()
        assert call(H=0) == -1 and who in err() and b"zero-size" in err()
        for kw in (dict(geom=None), dict(img=None), dict(binning=None)):
            assert call(**kw) == -1 and who in err() and b"NULL state buffer" in err()
        assert call(feats=None) == -1 and who in err() and b"NULL features" in err()
        opts.exp_mode = 9
        assert call() == -1 and b"exp_mode" in err()
        opts.exp_mode = 0
        assert call(P=0, Cn=0) == -1 and call(P=0, W=0) == -1      # (C and the sizes are checked first)
    assert fwd(out=None) == -1 and b"NULL feature_map" in err()
    assert bwd(gmap=None) == -1 and b"NULL dL_dfeature_map" in err()
    assert bwd(out=None) == -1 and b"NULL dL_dfeatures" in err()
    # P = 0, backward: nothing to write, no launch, whatever state is NULL; with or without an options struct
    assert bwd(P=0, geom=None, binning=None, img=None, feats=None, out=None) == 0
    assert bwd(P=0, o=None, geom=None, binning=None, img=None, feats=None, out=None) == 0
    assert fwd(P=0, out=None) == -1 and b"NULL feature_map" in err()      # (the forward still owes a zero map)


def test_python_refuses_bad_features_at_call_time(rast):
    _C = rast._C
    P, H, W, cpu = 7, 16, 16, torch.device("cpu")
    good = torch.zeros((P, 5))
    _C.check_features(None, P, cpu)
    _C.check_features(good, P, cpu)
    _C.check_features(torch.zeros((P, 64), requires_grad=True), P, cpu)      # (a differentiable input: requires_grad is welcome)
    bad = dict(rows=torch.zeros((P + 1, 5)), flat=torch.zeros(P * 5), three=torch.zeros((P, 5, 1)), none=torch.zeros((P, 0)), wide=torch.zeros((P, 65)),
               dtype=torch.zeros((P, 5), dtype=torch.float64), layout=torch.zeros((5, P)).T, device=torch.zeros((P, 5), device="meta"), kind=[[0.0] * 5] * P)
    for what, t in bad.items():
        with pytest.raises(ValueError, match="features"):
            _C.check_features(t, P, cpu)
    # through the public entry points: ValueError before anything is rendered (no GPU here)
    rs = rast.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    m3, m2, op = torch.zeros((P, 3)), torch.zeros((P, 3)), torch.zeros((P, 1))
    e = torch.empty(0)

    def entries(**kw):
        yield lambda: rast.rasterize_gaussians(m3, m2, e, torch.zeros((P, 3)), op, torch.ones((P, 3)), torch.ones((P, 4)), e, rs, **kw)
        yield lambda: rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), **kw)
        yield lambda: rast.GaussianRasterizerRaw(rs)(m3, m2, torch.ones((P, 4)), torch.zeros((P, 3)), op, torch.zeros((P, 1, 3)), torch.zeros((P, 15, 3)), **kw)

    for k in ("rows", "wide", "none", "dtype", "layout", "device", "kind"):
        for call in entries(features=bad[k]):
            with pytest.raises(ValueError, match="features"):
                call()
    # an installed GradArena: RuntimeError, like return_aux, before anything is rendered
    arena = _C.GradArena(P, 16, cpu)
    _C.set_grad_arena(arena)
    try:
        for call in entries(features=good):
            with pytest.raises(RuntimeError, match="GradArena"):
                call()
    finally:
        _C.set_grad_arena(None)
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):      # the published keyword defaults do not move
        assert fn.__kwdefaults__ == {"return_aux": False}
    with pytest.raises(TypeError):
        rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), feature=good)
    with pytest.raises(TypeError, match="unexpected keyword argument 'feature'"):
        rast._parse_request(rs, P, cpu, feature=good)
    # what the node finds in its four fixed trailing slots (features, viewmatrix, projmatrix, campos): None where unused
    rq = rs._replace(viewmatrix=torch.eye(4, requires_grad=True))
    cam = (rq.viewmatrix, rq.projmatrix, rq.campos)
    for feats in (None, good):
        kw = {} if feats is None else dict(features=feats)
        for settings, camera_grads in ((rs, False), (rs, True), (rq, False)):
            req, slots = rast._parse_request(settings, P, cpu, camera_grads=camera_grads, **kw)
            assert req.camera is False and len(slots) == 4 and slots[0] is feats and slots[1:] == (None, None, None)
        req, slots = rast._parse_request(rq, P, cpu, camera_grads=True, **kw)
        assert req.camera is True and len(slots) == 4 and slots[0] is feats and all(a is b for a, b in zip(slots[1:], cam))


def test_reference_with_three_channels_is_the_colour_render(scenes):
    """features_math in fp64, C = 3: the map equals mr.render(colors_precomp=F, bg=0)["color"], and a feature-only loss has the gradients of
    that colour's loss."""
    import contrib_math as cm
    mr = fm.mr
    sc, cam = cm.case_scene(scenes, cm.CASES["b"])
    P = sc["means3D"].shape[0]
    F = fm.features_of(P, 3)
    r = fm.evaluate64(sc, cam, F, colour_loss=False)
    t = {n: cm.t64(sc[n]).requires_grad_(True) for n in ("means3D", "scales", "rotations", "opacities")}
    Ft = cm.t64(F).requires_grad_(True)
    out = mr.render(t["means3D"], t["scales"], t["rotations"], t["opacities"], None, 0, cam, np.zeros(3), colors_precomp=Ft)
    assert np.array_equal(r["map"], out["color"].detach().numpy()) and np.abs(r["map"]).max() > 0.1
    assert r["amb"].mean() < 0.05
    (out["color"] * torch.as_tensor(r["g1"], dtype=torch.float64)).sum().backward()
    for n, x in list(t.items()) + [("features", Ft)]:
        np.testing.assert_allclose(r["grads"][n], x.grad.numpy(), rtol=1e-12, atol=1e-15 * np.abs(x.grad.numpy()).max())
    assert not r["grads"]["shs"].any()      # (no colour loss: nothing reaches the SH coefficients)
    gF = r["grads"]["features"]
    assert not gF[~r["vis"]].any() and (~gF[r["vis"]].any(1)).any() and np.abs(gF).max() > 1.0      # culled rows; listed but never blended
    # the map is additive over channels: one channel of a wider F is the same channel
    F19 = fm.features_of(P, 19)
    r19 = fm.evaluate64(sc, cam, F19, feature_loss=False, colour_loss=False)
    one = mr.render(t["means3D"].detach(), t["scales"].detach(), t["rotations"].detach(), t["opacities"].detach(), None, 0, cam, np.zeros(3),
                    colors_precomp=cm.t64(np.stack([F19[:, 18], F19[:, 3], F19[:, 7]], 1)))["color"].numpy()
    np.testing.assert_allclose(r19["map"][[18, 3, 7]], one, rtol=1e-13, atol=1e-15)
