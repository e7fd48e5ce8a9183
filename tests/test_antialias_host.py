"""CPU: the anti-aliased rendering (include/gsrast.h: GSRAST_RENDER_ANTIALIAS, the `flags` word of the call records) -- argument
errors refused before any device work; `antialiasing` keyword-only and False by default on every Python surface; the fp64 helper the
GPU tests measure against (tests/aa_math.py).  (The records' layout and the flag values: tests/test_capi_abi.py.)"""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import capi_records as cr

ONE = cr.ONE


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def _fwd(P, opts, flags, acc, alpha, family="dense"):
    return cr.call(cr.forward(P, flags, family, out_acc_depth=acc, out_alpha=alpha), opts)


def _bwd(P, opts, flags, dacc=None, dal=None, family="dense"):      # (the record of a caller that knows the flags word and nothing later)
    return cr.call(cr.backward(P, flags, family, size="min", dL_dacc_depth=dacc, dL_dalpha=dal), opts)


def test_flags_entry_points_refuse_bad_arguments_before_any_device_work(L, rast):
    _C = rast._C
    AUX, AA = _C.RENDER_AUX, _C.RENDER_ANTIALIAS
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    # unknown bits, alone and next to known ones
    for bad in (0x4, 0x80000000, AA | 0x8, AUX | AA | 0x10):
        rc, err = _fwd(10, opts, bad, ONE, ONE)
        assert rc == -1 and b"unknown bits" in err, bad
        rc, err = _bwd(10, opts, bad)
        assert rc == -1 and b"unknown bits" in err, bad
    # AUX with a NULL aux output (AA or not)
    for fl in (AUX, AUX | AA):
        for a, b in ((None, ONE), (ONE, None), (None, None)):
            rc, err = _fwd(10, opts, fl, a, b)
            assert rc == -1 and b"NULL acc_depth / alpha" in err
    # AUX with cull = 0, forward and backward
    opts.cull = 0
    for fl in (AUX, AUX | AA):
        for rc, err in (_fwd(10, opts, fl, ONE, ONE), _bwd(10, opts, fl, ONE, None), _bwd(10, opts, fl)):
            assert rc == -1 and b"cull" in err
    # (AA alone does not need the culled kernels: it reaches the ordinary argument checks -- here the negative P)
    rc, err = _fwd(-1, opts, AA, None, None)
    assert rc == -1 and b"bad P" in err
    L.gsrast_options_init(C.byref(opts))
    assert _fwd(-1, opts, AA, None, None)[0] == -1
    assert _bwd(-1, opts, AA)[0] == -1
    # the raw family
    fr = lambda P, fl, a, b: _fwd(P, opts, fl, a, b, "raw")                  # noqa: E731
    br = lambda P, fl, a=None, b=None: _bwd(P, opts, fl, a, b, "raw")        # noqa: E731
    for rc, err in (fr(10, 0x4, ONE, ONE), br(10, 0x4)):
        assert rc == -1 and b"unknown bits" in err
    rc, err = fr(10, AUX | AA, None, ONE)
    assert rc == -1 and b"NULL acc_depth / alpha" in err
    assert fr(-1, AA, None, None)[0] == -1
    assert br(-1, AA)[0] == -1
    opts.cull = 0
    for rc, err in (fr(10, AUX, ONE, ONE), br(10, AUX | AA, ONE, None)):
        assert rc == -1 and b"cull" in err
    L.gsrast_options_init(C.byref(opts))


def test_every_render_symbol_is_an_adapter_over_one_path(L, rast):
    """The same bad argument through every way of a family that can express it: the same return code and the same gsrast_last_error()
    text, forward and backward, dense and raw -- the backward record at each of its three sizes ("min": what a caller compiled before the
    absgrad sink passes, "abs": before the pose fields, "full"), and for the dense family with flags = 0 the positional gsrast_forward /
    gsrast_backward (which take no options: the process defaults).  All of these return before any device work (the allocators would
    fail: a refusal that got that far would say "allocation")."""
    _C = rast._C
    one = C.c_void_p(ONE)
    AUX = _C.RENDER_AUX
    opts = _C.OptionsStruct()

    def positional(family, P):
        if family == "forward":
            rc = L.gsrast_forward(cr.NO_ALLOC, None, cr.NO_ALLOC, None, cr.NO_ALLOC, None, P, 3, 16, one, 64, 64, one, one, None, one, one, 1.0, one, None,
                                  one, one, one, 0.5, 0.5, 0, one, one, one, None)
        else:
            rc = L.gsrast_backward(P, 3, 16, 5, one, 64, 64, one, one, None, one, 1.0, one, None, one, one, one, 0.5, 0.5, one, one, one, one,
                                   one, one, None, one, None, one, None, one, one, one, None)
        return ("gsrast_" + family, rc, L.gsrast_last_error())

    def outcomes(family, P, flags, a, b, with_positional=False):
        """(way, return code, error text) of every way of the family that can express (flags, aux pair)."""
        direction, _, raw = family.partition("_")
        kind = "raw" if raw else "dense"
        if direction == "forward":
            recs = [("record", cr.forward(P, flags, kind, out_acc_depth=a, out_alpha=b))]
        else:
            recs = [(size, cr.backward(P, flags, kind, size=size, dL_dacc_depth=a, dL_dalpha=b)) for size in ("min", "abs", "full")]
        out = [(way,) + cr.call(rec, opts) for way, rec in recs]
        if with_positional and not raw:
            out.append(positional(direction, P))
        return out

    def same(results, n_ways, needle):
        assert len(results) == n_ways, results
        assert {r[1] for r in results} == {-1}, results
        assert len({r[2] for r in results}) == 1, results
        assert needle in results[0][2], results

    for family in ("forward", "backward", "forward_raw", "backward_raw"):
        L.gsrast_options_init(C.byref(opts))
        n = 1 if family.startswith("forward") else 3      # the records of the family
        # P = -1: flags = 0 (the positional call too) and AUX
        sizes = b"bad P" if family.startswith("forward") else b"bad sizes"
        plain = outcomes(family, -1, 0, None, None, with_positional=True)
        auxed = outcomes(family, -1, AUX, ONE, ONE)
        same(plain + auxed, 2 * n + (0 if family.endswith("raw") else 1), sizes)
        # an unknown flag bit
        same(outcomes(family, 10, 0x10, ONE, ONE), n, b"unknown bits")
        # forward, AUX with a NULL aux output
        if family.startswith("forward"):
            for a, b in ((None, ONE), (ONE, None), (None, None)):
                same(outcomes(family, 10, AUX, a, b), n, b"NULL acc_depth / alpha")
        # AUX with cull = 0
        opts.cull = 0
        same(outcomes(family, 10, AUX, ONE, ONE), n, b"cull")
    L.gsrast_options_init(C.byref(opts))


def test_antialiasing_is_keyword_only_and_false_by_default_on_every_surface(rast):
    # functional form: a plain keyword-only parameter
    p = inspect.signature(rast.rasterize_gaussians).parameters["antialiasing"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    # the two modules: keyword-only through **render_options (their published keyword defaults stay {"return_aux": False}) ...
    for cls in (rast.GaussianRasterizer, rast.GaussianRasterizerRaw):
        ps = inspect.signature(cls.forward, follow_wrapped=False).parameters
        assert "antialiasing" not in ps
    rs = rast.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    cpu = torch.device("cpu")
    assert rast._parse_request(rs, 1, cpu)[0].antialiasing is False
    assert rast._parse_request(rs, 1, cpu, antialiasing=True)[0].antialiasing is True
    with pytest.raises(TypeError, match="unexpected keyword argument 'antialias'"):
        rast._parse_request(rs, 1, cpu, antialias=True)
    # ... reached before anything touches a tensor: a typo fails on a CPU machine too, and a positional value has no slot to land in
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
