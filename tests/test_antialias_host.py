"""CPU: the anti-aliased rendering (include/gsrast.h: GSRAST_RENDER_ANTIALIAS and the gsrast_*_flags entry points) -- declared,
exported and bound; argument errors refused before any device work; `antialiasing` keyword-only and False by default on every Python
surface; the fp64 helper the GPU tests measure against (tests/aa_math.py)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsrast.h")
FLAGS = ("gsrast_forward_flags", "gsrast_backward_flags", "gsrast_forward_raw_flags", "gsrast_backward_raw_flags")
SIBLINGS = ("gsrast_forward_aux", "gsrast_backward_aux", "gsrast_forward_raw_aux", "gsrast_backward_raw_aux")


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_flags_symbols_are_declared_exported_and_bound(rast, L):
    src = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(rast._C.LIB_PATH)
    for n, sib in zip(FLAGS, SIBLINGS):
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in gsrast.h"
        assert hasattr(raw, n), f"{n} not exported"
        assert n in rast._C.EXPORTS
        # the aux sibling's arguments with an unsigned flags word behind the options
        at = 2 if "forward" in n else 1
        want = list(getattr(L, sib).argtypes)
        assert getattr(L, n).argtypes == want[:at] + [C.c_uint] + want[at:], n
        assert getattr(L, n).restype is C.c_int
    assert re.search(r"#define\s+GSRAST_RENDER_AUX\s+0x1u\b", src)
    assert re.search(r"#define\s+GSRAST_RENDER_ANTIALIAS\s+0x2u\b", src)
    assert (rast._C.RENDER_AUX, rast._C.RENDER_ANTIALIAS) == (1, 2)
    assert L.gsrast_abi_version() == 5


def _fwd(L, cb, P, one, opts, flags, acc, alpha):
    return L.gsrast_forward_flags(None, opts, flags, cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, one, one, None, one, one, 1.0, one,
                                  None, one, one, one, 0.5, 0.5, 0, one, one, one, None, acc, alpha)


def _bwd(L, P, one, opts, flags, dacc=None, dal=None):
    return L.gsrast_backward_flags(opts, flags, P, 3, 16, 5, one, 64, 64, one, one, None, one, 1.0, one, None, one, one, one, 0.5, 0.5, one,
                                   one, one, one, one, one, None, one, None, one, None, one, one, one, None, dacc, dal)


def test_flags_entry_points_refuse_bad_arguments_before_any_device_work(L, rast):
    _C = rast._C
    ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
    cb = ALLOC(lambda ctx, n: None)      # an allocation would fail: a refusal that got that far would say "allocation"
    one = C.c_void_p(16)
    AUX, AA = _C.RENDER_AUX, _C.RENDER_ANTIALIAS
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    o = C.byref(opts)
    # unknown bits, alone and next to known ones
    for bad in (0x4, 0x80000000, AA | 0x8, AUX | AA | 0x10):
        assert _fwd(L, cb, 10, one, o, bad, one, one) == -1 and b"unknown bits" in L.gsrast_last_error(), bad
        assert _bwd(L, 10, one, o, bad) == -1 and b"unknown bits" in L.gsrast_last_error(), bad
    # AUX with a NULL aux output (AA or not)
    for fl in (AUX, AUX | AA):
        for a, b in ((None, one), (one, None), (None, None)):
            assert _fwd(L, cb, 10, one, o, fl, a, b) == -1 and b"NULL acc_depth / alpha" in L.gsrast_last_error()
    # AUX with cull = 0, forward and backward
    opts.cull = 0
    for fl in (AUX, AUX | AA):
        assert _fwd(L, cb, 10, one, o, fl, one, one) == -1 and b"cull" in L.gsrast_last_error()
        assert _bwd(L, 10, one, o, fl, one, None) == -1 and b"cull" in L.gsrast_last_error()
        assert _bwd(L, 10, one, o, fl) == -1 and b"cull" in L.gsrast_last_error()
    # (AA alone does not need the culled kernels: it reaches the ordinary argument checks -- here the negative P)
    assert _fwd(L, cb, -1, one, o, AA, None, None) == -1 and b"bad P" in L.gsrast_last_error()
    L.gsrast_options_init(C.byref(opts))
    assert _fwd(L, cb, -1, one, o, AA, None, None) == -1
    assert _bwd(L, -1, one, o, AA) == -1
    # the raw pair
    ins = _C.RawInputsStruct(xyz=16, rotation=16, scaling=16, opacity_logit=16, features_dc=16, features_rest=16)
    fr = lambda P, fl, a, b: L.gsrast_forward_raw_flags(None, o, fl, cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, C.byref(ins),   # noqa: E731
                                                        1.0, one, one, one, 1.0, 1.0, one, one, one, None, a, b)
    gr = _C.RawGradsStruct(dL_dmean2D=16, d_xyz=16, d_rotation=16, d_scaling=16, d_opacity_logit=16, d_features_dc=16, d_features_rest=16)
    br = lambda P, fl, a=None, b=None: L.gsrast_backward_raw_flags(o, fl, P, 3, 16, 5, one, 64, 64, C.byref(ins), 1.0, one, one, one,   # noqa: E731
                                                                   1.0, 1.0, one, one, one, one, one, C.byref(gr), None, a, b)
    assert fr(10, 0x4, one, one) == -1 and b"unknown bits" in L.gsrast_last_error()
    assert br(10, 0x4) == -1 and b"unknown bits" in L.gsrast_last_error()
    assert fr(10, AUX | AA, None, one) == -1 and b"NULL acc_depth / alpha" in L.gsrast_last_error()
    assert fr(-1, AA, None, None) == -1
    assert br(-1, AA) == -1
    opts.cull = 0
    assert fr(10, AUX, one, one) == -1 and b"cull" in L.gsrast_last_error()
    assert br(10, AUX | AA, one, None) == -1 and b"cull" in L.gsrast_last_error()
    L.gsrast_options_init(C.byref(opts))


def test_every_render_symbol_is_an_adapter_over_one_path(L, rast):
    """The same bad argument through every symbol of a family that can express it: the same return code and the same
    gsrast_last_error() text, forward and backward, dense (_ex, _aux, _flags) and raw (_raw, _raw_aux, _raw_flags).  All of these return
    before any device work (the allocators would fail: a refusal that got that far would say "allocation")."""
    _C = rast._C
    cb = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)(lambda ctx, n: None)
    one = C.c_void_p(16)
    AUX = _C.RENDER_AUX
    opts = _C.OptionsStruct()
    o = C.byref(opts)
    ins = _C.RawInputsStruct(xyz=16, rotation=16, scaling=16, opacity_logit=16, features_dc=16, features_rest=16)
    gr = _C.RawGradsStruct(dL_dmean2D=16, d_xyz=16, d_rotation=16, d_scaling=16, d_opacity_logit=16, d_features_dc=16, d_features_rest=16)
    body = {      # the arguments between the options (+ flags) and the aux pair, as a function of P
        "forward": lambda P: (cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, one, one, None, one, one, 1.0, one, None, one, one, one,
                              0.5, 0.5, 0, one, one, one, None),
        "backward": lambda P: (P, 3, 16, 5, one, 64, 64, one, one, None, one, 1.0, one, None, one, one, one, 0.5, 0.5, one, one, one, one,
                               one, one, None, one, None, one, None, one, one, one, None),
        "forward_raw": lambda P: (cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, C.byref(ins), 1.0, one, one, one, 1.0, 1.0,
                                  one, one, one, None),
        "backward_raw": lambda P: (P, 3, 16, 5, one, 64, 64, C.byref(ins), 1.0, one, one, one, 1.0, 1.0, one, one, one, one, one,
                                   C.byref(gr), None),
    }

    def outcomes(family, P, flags, a, b):
        """(symbol, return code, error text) of every symbol of the family that can express (flags, aux pair)."""
        head = (None, o) if family.startswith("forward") else (o,)
        plain = "gsrast_" + family + ("" if family.endswith("raw") else "_ex")
        calls = [("gsrast_" + family + "_flags", head + (flags,) + body[family](P) + (a, b))]
        if flags == AUX:
            calls.append(("gsrast_" + family + "_aux", head + body[family](P) + (a, b)))
        if flags == 0:
            calls.append((plain, head + body[family](P)))
        out = []
        for name, args in calls:
            rc = getattr(L, name)(*args)
            out.append((name, rc, L.gsrast_last_error()))
        return out

    def same(results, n_symbols, needle):
        assert len(results) == n_symbols, results
        assert {r[1] for r in results} == {-1}, results
        assert len({r[2] for r in results}) == 1, results
        assert needle in results[0][2], results

    for family in ("forward", "backward", "forward_raw", "backward_raw"):
        L.gsrast_options_init(o)
        # P = -1: through all three (plain and _flags with flags = 0, _aux and _flags with AUX)
        sizes = b"bad P" if family.startswith("forward") else b"bad sizes"
        plain = outcomes(family, -1, 0, None, None)
        auxed = outcomes(family, -1, AUX, one, one)
        same(plain + auxed, 4, sizes)
        # an unknown flag bit: _flags alone can express it
        same(outcomes(family, 10, 0x4, one, one), 1, b"unknown bits")
        # forward, AUX with a NULL aux output: _aux and _flags
        if family.startswith("forward"):
            for a, b in ((None, one), (one, None), (None, None)):
                same(outcomes(family, 10, AUX, a, b), 2, b"NULL acc_depth / alpha")
        # AUX with cull = 0: _aux and _flags
        opts.cull = 0
        same(outcomes(family, 10, AUX, one, one), 2, b"cull")
    L.gsrast_options_init(o)


def test_antialiasing_is_keyword_only_and_false_by_default_on_every_surface(rast):
    # functional form: a plain keyword-only parameter
    p = inspect.signature(rast.rasterize_gaussians).parameters["antialiasing"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    # the two modules: keyword-only through **render_options (their published keyword defaults stay {"return_aux": False}) ...
    for cls in (rast.GaussianRasterizer, rast.GaussianRasterizerRaw):
        ps = inspect.signature(cls.forward, follow_wrapped=False).parameters
        assert "antialiasing" not in ps
    assert rast._antialiasing_of({}) is False
    assert rast._antialiasing_of({"antialiasing": True}) is True
    with pytest.raises(TypeError, match="unexpected keyword argument 'antialias'"):
        rast._antialiasing_of({"antialias": True})
    # ... reached before anything touches a tensor: a typo fails on a CPU machine too, and a positional value has no slot to land in
    rs = rast.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    with pytest.raises(TypeError, match="antialias"):
        rast.GaussianRasterizer(rs)(torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 1), colors_precomp=torch.zeros(1, 3),
                                    cov3D_precomp=torch.zeros(1, 6), antialias=True)
    with pytest.raises(TypeError):
        rast.GaussianRasterizer(rs)(torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 1), None, torch.zeros(1, 3), None, None,
                                    torch.zeros(1, 6), True)
    # the binding layer
    for fn in (rast._C.rasterize_gaussians, rast._C.rasterize_gaussians_raw, rast._C.rasterize_gaussians_backward,
               rast._C.rasterize_gaussians_raw_backward):
        p = inspect.signature(fn).parameters["antialiasing"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, fn


def _cam(W=64, H=48, tan=0.5):
    V = np.eye(4, dtype=np.float32)
    return dict(image_width=W, image_height=H, tanfovx=tan, tanfovy=tan * H / W, viewmatrix=V, projmatrix=V)


def test_aa_math_spot_checks():
    import aa_math
    # an isotropic screen-space covariance sigma^2 I: rho = (sigma^2 / (sigma^2 + 0.3))^2, comp = sigma^2 / (sigma^2 + 0.3)
    d = float(np.float32(0.3))
    for s2 in (1e-3, 0.05, 0.3, 1.0, 7.5, 250.0):
        a = torch.tensor([s2 + d], dtype=torch.float64)
        c, rho = aa_math.comp_of_cov2(a, torch.zeros(1, dtype=torch.float64), a.clone())
        assert math.isclose(float(c), max(s2 / (s2 + d), math.sqrt(aa_math.FLOOR)), rel_tol=1e-12), s2
    # rho <= 0 (and rho under the floor) lands on the floor: sqrt(0.000025) = 0.005
    for a, b, c in ((0.3, 0.0, 0.3), (0.31, 0.2, 0.31), (0.3 + 1e-9, 0.0, 0.3 + 1e-9)):
        cc, rho = aa_math.comp_of_cov2(*(torch.tensor([v], dtype=torch.float64) for v in (a, b, c)))
        assert float(rho) < aa_math.FLOOR
        assert math.isclose(float(cc), 0.005, rel_tol=1e-6)
    # through the projection: an isotropic Gaussian on the optical axis at depth z has cov2 = (f s / z)^2 I
    cam = _cam()
    z, s = 4.0, 0.02
    m = torch.tensor([[0.0, 0.0, z]], dtype=torch.float64)
    c, _ = aa_math.comp(m, torch.full((1, 3), s, dtype=torch.float64), torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64), cam)
    f = 64 / (2 * float(np.float32(0.5)))
    s2 = (f * s / z) ** 2
    assert math.isclose(float(c), s2 / (s2 + d), rel_tol=1e-9)
    # the cov3D_precomp form agrees with the scales / rotations form, and the fp32 chain with the fp64 one
    rng = np.random.default_rng(0)
    P = 64
    means = torch.as_tensor(np.c_[rng.uniform(-0.5, 0.5, (P, 2)), rng.uniform(2.0, 6.0, P)])
    scales = torch.as_tensor(np.exp(rng.uniform(np.log(0.002), np.log(0.1), (P, 3))))
    q = rng.normal(size=(P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    rots = torch.as_tensor(q)
    c1, _ = aa_math.comp(means, scales, rots, cam)
    R = aa_math.mr.rotation_matrix(rots); Mx = R * scales[:, None, :]; S = Mx @ Mx.transpose(1, 2)
    cov6 = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    c2, _ = aa_math.comp(means, None, None, cam, cov3D=cov6)
    assert torch.allclose(c1, c2, rtol=1e-12, atol=0)
    c32, _ = aa_math.comp32(means.float(), scales.float(), rots.float(), cam)
    assert float((c1 < 0.9).float().mean()) > 0.2 and float((c1 > 0.1).float().mean()) > 0.2      # (the sample spans the filter's range)
    assert torch.allclose(c32.double(), c1, rtol=1e-4, atol=1e-5)
    # differentiable: d comp / d scale > 0 above the floor
    sc = scales.clone().requires_grad_(True)
    cc, rho = aa_math.comp(means, sc, rots, cam)
    cc.sum().backward()
    assert bool((sc.grad.sum(1)[rho > aa_math.FLOOR] > 0).all())
