"""CPU: the differentiable alpha / accumulated-depth outputs (include/gsrast.h: GSRAST_RENDER_AUX; out_acc_depth / out_alpha of
gsrast_forward_call, dL_dacc_depth / dL_dalpha of gsrast_backward_call, either family) -- argument errors refused before any device
work; the Python surfaces default to the plain path.  (The records' layout: tests/test_capi_abi.py.)"""
import ctypes as C
import inspect

import pytest

import capi_records as cr

ONE = cr.ONE


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_aux_entry_points_refuse_bad_arguments_before_any_device_work(L, rast):
    _C = rast._C
    AUX = _C.RENDER_AUX
    # negative P
    assert cr.call(cr.forward(-1, AUX, out_acc_depth=ONE, out_alpha=ONE))[0] == -1
    assert cr.call(cr.backward(-1, AUX, dL_dacc_depth=ONE, dL_dalpha=ONE))[0] == -1
    # NULL aux outputs
    for a, b in ((None, ONE), (ONE, None), (None, None)):
        rc, err = cr.call(cr.forward(10, AUX, out_acc_depth=a, out_alpha=b))
        assert rc == -1 and b"NULL acc_depth / alpha" in err
    # cull = 0
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    opts.cull = 0
    fwd = cr.forward(10, AUX, out_acc_depth=ONE, out_alpha=ONE)
    rc, err = cr.call(fwd, opts)
    assert rc == -1 and b"cull" in err
    for a, b in ((ONE, None), (None, ONE)):
        rc, err = cr.call(cr.backward(10, AUX, dL_dacc_depth=a, dL_dalpha=b), opts)
        assert rc == -1 and b"cull" in err
    # a forced pixels-per-lane forward selects the un-culled kernel, which has no aux outputs
    L.gsrast_options_init(C.byref(opts))
    opts.fwd_pixels_per_lane = 2
    rc, err = cr.call(fwd, opts)
    assert rc == -1 and b"cull" in err
    # the raw family
    L.gsrast_options_init(C.byref(opts))
    fr = lambda P, a, b: cr.call(cr.forward(P, AUX, "raw", out_acc_depth=a, out_alpha=b), opts)      # noqa: E731
    br = lambda P, a, b: cr.call(cr.backward(P, AUX, "raw", dL_dacc_depth=a, dL_dalpha=b), opts)     # noqa: E731
    assert fr(-1, ONE, ONE)[0] == -1
    rc, err = fr(10, None, ONE)
    assert rc == -1 and b"NULL acc_depth / alpha" in err
    opts.cull = 0
    rc, err = fr(10, ONE, ONE)
    assert rc == -1 and b"cull" in err
    rc, err = br(10, ONE, None)
    assert rc == -1 and b"cull" in err
    L.gsrast_options_init(C.byref(opts))
    assert br(-1, ONE, ONE)[0] == -1


def test_return_aux_defaults_to_false_on_every_surface(rast):
    # (GaussianRasterizer.forward shows the reference's signature to introspection: the keyword-only default is read from the function)
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):
        assert fn.__kwdefaults__ == {"return_aux": False}, fn
    assert inspect.signature(rast.rasterize_gaussians).parameters["return_aux"].default is False
    assert "return_aux" not in inspect.signature(rast.GaussianRasterizer.forward).parameters
    for fn in (rast._C.rasterize_gaussians, rast._C.rasterize_gaussians_raw):
        assert inspect.signature(fn).parameters["aux"].default is False
    for fn in (rast._C.rasterize_gaussians_backward, rast._C.rasterize_gaussians_raw_backward):
        ps = inspect.signature(fn).parameters
        assert ps["dL_dacc_depth"].default is None and ps["dL_dalpha"].default is None
