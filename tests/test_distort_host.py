"""CPU: the depth-distortion map (include/gsrast.h: gsrast_distortion_forward / gsrast_distortion_backward; `distortion=True` of the Python
package) -- the helper tests/distort_math.py pins itself (its colour is math_renderer.render's, its cumulative-sum distortion the brute-force
pairwise sum, the closed forms of one and two Gaussians, the bounds of the map), the two symbols are declared, exported and bound, the ABI
version and the profile table are what they should be, both calls refuse bad arguments before any device work, and the package refuses a
`distortion` that is no bool (ValueError) or an installed GradArena (RuntimeError) at call time."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import contrib_math as cm
import distort_math as dm
from capi_records import ONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsrast.h")
NAMES = ("gsrast_distortion_forward", "gsrast_distortion_backward")


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


# ---- the helper pins itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cm.CASES))
def test_the_helper_is_the_math_renderer_and_the_pairwise_sum(name):
    r64 = dm.reference(name)["r64"]
    assert np.abs(r64["color"] - r64["ref_color"]).max() <= 1e-12 and np.abs(r64["ref_color"]).max() > 0.1
    assert np.abs((1.0 - r64["alpha"]) - r64["final_T"]).max() <= 1e-12
    assert r64["amb"].mean() < 0.05
    H, W = r64["map"].shape
    # a sample of pixels: the busiest one, the first with exactly two contributors, one with none or one, and a spread over the image
    flat = r64["n_live"].reshape(-1)
    sample = {int(np.argmax(flat)), int(np.argmin(flat))} | set(np.flatnonzero(flat == 2)[:2].tolist()) | set(range(0, H * W, 97))
    worst = 0.0
    for p in sorted(sample):
        want = dm.pairwise(r64["w"][p], r64["z"])
        got = float(r64["map"].reshape(-1)[p])
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (p, got, want)
        if flat[p] < 2:
            assert got == 0.0
    assert max(flat[p] for p in sample) > (100 if name == "a" else 4)      # (a: 163 of the 610 clustered Gaussians reach 1 / 255 at the busiest pixel)
    # the bounds: 0 <= distort <= (1 - T_final)^2 (z_max - z_min) over the pixel's contributors
    w, z = r64["w"], r64["z"]
    zhi = np.where(w > 0, z[None, :], -np.inf).max(axis=1)
    zlo = np.where(w > 0, z[None, :], np.inf).min(axis=1)
    span = np.where(flat > 0, zhi - zlo, 0.0)
    m = r64["map"].reshape(-1)
    assert (m >= -1e-15).all() and (m <= r64["alpha"].reshape(-1) ** 2 * span + 1e-12).all() and m.max() > 0.1
    assert (m[flat < 2] == 0.0).all()


def _tiny(scenes, centres, opac, scale=0.15):
    """(scene, camera): Gaussians at the given (px, py, z), 70 x 45."""
    cam = scenes.camera(1, 6, cm.W_IMG, cm.H_IMG)
    c = np.asarray(centres, np.float64)
    rng = np.random.default_rng(5)
    sc = cm._finish(rng, cam, c[:, 0], c[:, 1], c[:, 2], np.full(len(c), scale), np.asarray(opac, np.float64))
    return sc, cam


def test_one_gaussian_is_zero_and_two_are_the_closed_form(scenes):
    sc, cam = _tiny(scenes, [(35.0, 22.0, 3.0)], [0.7])
    r = dm.evaluate64(sc, cam)
    assert r["n_live"].max() == 1 and not r["map"].any()
    assert not any(np.abs(g).max() > 0 for n, g in dm.evaluate64(sc, cam, colour_loss=False)["grads"].items())
    sc, cam = _tiny(scenes, [(35.0, 22.0, 3.0), (35.0, 22.0, 4.5)], [0.6, 0.8])
    r = dm.evaluate64(sc, cam, colour_loss=False)
    w, z = r["w"][22 * cm.W_IMG + 35], r["z"]
    assert (w > 0.3).all() and z[1] - z[0] > 1.4
    want = 2.0 * w[0] * w[1] * abs(z[1] - z[0])
    assert abs(r["map"][22, 35] - want) <= 1e-14 and want > 0.3
    # pushing the two apart raises the distortion: dL/dz (through means3D along the view axis) has opposite signs on the two
    view_z = np.asarray(cam["viewmatrix"], np.float64)[:3, 2]
    order = np.argsort(sc["means3D"].astype(np.float64) @ view_z)
    g = dict(r["g"], gd=np.ones_like(r["g"]["gd"]))
    gz = dm.evaluate64(sc, cam, colour_loss=False, g=g)["grads"]["means3D"] @ view_z
    assert gz[order[0]] < 0 < gz[order[1]]
    # the restatement in float32 with the kernel's z0-relative association is the same function
    r32 = dm.restate32(sc, cam, r["g"], colour_loss=False)
    assert np.abs(r32["map"] - r["map"]).max() <= 1e-5 * r["map"].max()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(rast, L):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert not re.fullmatch(r"gsrast_(render_)?(forward|backward)\w*", n)
    assert L.gsrast_abi_version() == 6 and re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)      # additive: the version does not move
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert "distort_fwd" in names and "distort_bwd" in names and len(set(names)) == len(names)
    assert not re.search(r"#define\s+GSRAST_RENDER_\w+\s+0x10u", text)      # no render flag bit was added
    assert os.path.exists(os.path.join(ROOT, "saro-gs_amd", "csrc", "gsrast_distort.h"))


def test_bad_arguments_fail_before_any_device_work(L, rast):
    opts = rast._C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    one = C.c_void_p(ONE)
    err = L.gsrast_last_error

    def fwd(P=10, R=5, W=64, H=48, geom=one, binning=one, img=one, out=one, mom=one, o=C.byref(opts)):
        return L.gsrast_distortion_forward(o, P, R, W, H, geom, binning, img, out, mom, None)

    def bwd(P=10, R=5, W=64, H=48, geom=one, binning=one, img=one, mom=one, gmap=one, o=C.byref(opts)):
        return L.gsrast_distortion_backward(o, P, R, W, H, geom, binning, img, mom, gmap, None)

    for call, who in ((fwd, b"distortion_forward"), (bwd, b"distortion_backward")):
        assert call(P=-1) == -1 and who in err() and b"negative" in err()
        assert call(R=-1) == -1 and who in err() and b"negative" in err()
        assert call(W=0) == -1 and who in err() and b"zero-size" in err()
        assert call(H=0) == -1 and who in err() and b"zero-size" in err()
        for kw in (dict(geom=None), dict(img=None), dict(binning=None)):
            assert call(**kw) == -1 and who in err() and b"NULL state buffer" in err()
        assert call(mom=None) == -1 and who in err() and b"NULL moments" in err()
        assert call(geom=None, mom=None) == -1 and b"NULL state buffer" in err()      # (the ladder's order: state first)
        opts.exp_mode = 9
        assert call() == -1 and who in err() and b"exp_mode" in err()
        assert call(mom=None) == -1 and b"NULL moments" in err()                       # (pointers before the options)
        opts.exp_mode = 0
        assert call(P=0, W=0) == -1 and b"zero-size" in err()                          # (the sizes are checked first)
    assert fwd(out=None) == -1 and b"NULL distort_map" in err()
    assert bwd(gmap=None) == -1 and b"NULL dL_ddistort" in err()
    # P = 0, backward: nothing to write, no launch, whatever is NULL; with or without an options struct
    assert bwd(P=0, geom=None, binning=None, img=None, mom=None, gmap=None) == 0
    assert bwd(P=0, o=None, geom=None, binning=None, img=None, mom=None, gmap=None) == 0
    assert fwd(P=0, out=None) == -1 and b"NULL distort_map" in err()      # (the forward still owes a zero map)
    assert fwd(P=0, mom=None) == -1 and b"NULL moments" in err()


# ---- the package's own checks ---------------------------------------------------------------------------------------------------------------
def test_python_argument_checks(rast):
    _C = rast._C
    P, H, W, cpu = 7, 16, 16, torch.device("cpu")
    rs = rast.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    m3, m2, op = torch.zeros((P, 3)), torch.zeros((P, 3)), torch.zeros((P, 1))
    e = torch.empty(0)

    def entries(**kw):
        yield lambda: rast.rasterize_gaussians(m3, m2, e, torch.zeros((P, 3)), op, torch.ones((P, 3)), torch.ones((P, 4)), e, rs, **kw)
        yield lambda: rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), **kw)
        yield lambda: rast.GaussianRasterizerRaw(rs)(m3, m2, torch.ones((P, 4)), torch.zeros((P, 3)), op, torch.zeros((P, 1, 3)), torch.zeros((P, 15, 3)), **kw)

    for bad in (1, "yes", None, torch.ones(())):
        for call in entries(distortion=bad):
            with pytest.raises(ValueError, match="distortion"):
                call()
    arena = _C.GradArena(P, 16, cpu)
    _C.set_grad_arena(arena)
    try:
        for call in entries(distortion=True):
            with pytest.raises(RuntimeError, match="GradArena"):
                call()
        req, _ = rast._parse_request(rs, P, cpu, distortion=False)      # (asked for nothing: no refusal)
        assert req.distortion is False
    finally:
        _C.set_grad_arena(None)
    # keyword-only, default False; the published keyword defaults do not move
    import inspect
    p = inspect.signature(rast.rasterize_gaussians).parameters["distortion"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):
        assert fn.__kwdefaults__ == {"return_aux": False}
    with pytest.raises(TypeError, match="unexpected keyword argument 'distort'"):
        rast._parse_request(rs, P, cpu, distort=True)
    # the request: the bit travels in the record's TYPE (its six fields are pinned elsewhere), the four fixed trailing slots are what they were
    for kw, want in ((dict(), False), (dict(distortion=False), False), (dict(distortion=True), True)):
        req, slots = rast._parse_request(rs, P, cpu, **kw)
        assert req.distortion is want and slots == (None, None, None, None)
        assert (type(req) is rast._DistortionRequest) is want and req._fields == rast._Request._fields and len(req) == 6
        assert type(req._replace(return_aux=True)) is type(req)
    # a backward whose plan cannot consume dL/dz (options.cull == 0) names the keyword
    with pytest.raises(RuntimeError, match="distortion"):
        _C._distortion_aux((torch.zeros((2, H, W)), torch.zeros((H, W))), None, None, H, W, cpu, dict(_C.current_options(), cull=0))
    assert _C._distortion_aux(None, None, None, H, W, cpu, dict(_C.current_options(), cull=0)) is None
    z = _C._distortion_aux((torch.zeros((2, H, W)), torch.zeros((H, W))), None, None, H, W, cpu, None)
    assert tuple(z.shape) == (1, H, W) and not z.any()
    given = torch.ones((1, H, W))
    assert _C._distortion_aux((torch.zeros((2, H, W)), torch.zeros((H, W))), given, None, H, W, cpu, None) is given
    assert _C._distortion_aux((torch.zeros((2, H, W)), torch.zeros((H, W))), None, given, H, W, cpu, None) is None
    for text in (rast.__doc__, rast.rasterize_gaussians.__doc__):
        assert "distortion" in text and "absgrad" in text
