"""CPU: the differentiable alpha / accumulated-depth outputs (include/gsrast.h: gsrast_forward_aux, gsrast_backward_aux and the raw
pair) -- declared, exported and bound; argument errors refused before any device work; the Python surfaces default to the plain path."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsrast.h")
AUX = ("gsrast_forward_aux", "gsrast_backward_aux", "gsrast_forward_raw_aux", "gsrast_backward_raw_aux")


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_aux_symbols_are_declared_exported_and_listed(rast, L):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = C.CDLL(rast._C.LIB_PATH)
    for n in AUX:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in gsrast.h"
        assert hasattr(raw, n), f"{n} not exported"
        assert n in rast._C.EXPORTS
    # each takes its sibling's arguments + the two [1,H,W] arrays
    for n, sib in zip(AUX, ("gsrast_forward_ex", "gsrast_backward_ex", "gsrast_forward_raw", "gsrast_backward_raw")):
        assert getattr(L, n).argtypes == getattr(L, sib).argtypes + [C.c_void_p, C.c_void_p]
    assert L.gsrast_abi_version() == 5


def _fwd_args(L, cb, P, one):
    return (None, None, cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, one, one, None, one, one, 1.0, one, None,
            one, one, one, 0.5, 0.5, 0, one, one, one, None)


def _bwd_args(P, one, opts=None):
    return (opts, P, 3, 16, 5, one, 64, 64, one, one, None, one, 1.0, one, None, one, one, one, 0.5, 0.5, one, one, one, one, one,
            one, None, one, None, one, None, one, one, one, None)


def test_aux_entry_points_refuse_bad_arguments_before_any_device_work(L, rast):
    _C = rast._C
    ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
    cb = ALLOC(lambda ctx, n: None)      # an allocation would fail: a refusal that got that far would say "allocation"
    one = C.c_void_p(16)
    # negative P
    assert L.gsrast_forward_aux(*_fwd_args(L, cb, -1, one), one, one) == -1
    assert L.gsrast_backward_aux(*_bwd_args(-1, one), one, one) == -1
    # NULL aux outputs
    for a, b in ((None, one), (one, None), (None, None)):
        assert L.gsrast_forward_aux(*_fwd_args(L, cb, 10, one), a, b) == -1
        assert b"NULL acc_depth / alpha" in L.gsrast_last_error()
    # cull = 0
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    opts.cull = 0
    args = list(_fwd_args(L, cb, 10, one)); args[1] = C.byref(opts)
    assert L.gsrast_forward_aux(*args, one, one) == -1 and b"cull" in L.gsrast_last_error()
    assert L.gsrast_backward_aux(*_bwd_args(10, one, C.byref(opts)), one, None) == -1 and b"cull" in L.gsrast_last_error()
    assert L.gsrast_backward_aux(*_bwd_args(10, one, C.byref(opts)), None, one) == -1 and b"cull" in L.gsrast_last_error()
    # a forced pixels-per-lane forward selects the un-culled kernel, which has no aux outputs
    L.gsrast_options_init(C.byref(opts))
    opts.fwd_pixels_per_lane = 2
    args[1] = C.byref(opts)
    assert L.gsrast_forward_aux(*args, one, one) == -1 and b"cull" in L.gsrast_last_error()
    # the raw pair
    L.gsrast_options_init(C.byref(opts))
    ins = _C.RawInputsStruct(xyz=16, rotation=16, scaling=16, opacity_logit=16, features_dc=16, features_rest=16)
    fr = lambda P, o: (None, o, cb, None, cb, None, cb, None, P, 3, 16, one, 64, 64, C.byref(ins), 1.0, one, one, one, 1.0, 1.0,   # noqa: E731
                       one, one, one, None)
    assert L.gsrast_forward_raw_aux(*fr(-1, C.byref(opts)), one, one) == -1
    assert L.gsrast_forward_raw_aux(*fr(10, C.byref(opts)), None, one) == -1 and b"NULL acc_depth / alpha" in L.gsrast_last_error()
    opts.cull = 0
    assert L.gsrast_forward_raw_aux(*fr(10, C.byref(opts)), one, one) == -1 and b"cull" in L.gsrast_last_error()
    gr = _C.RawGradsStruct(dL_dmean2D=16, d_xyz=16, d_rotation=16, d_scaling=16, d_opacity_logit=16, d_features_dc=16, d_features_rest=16)
    br = lambda P, o: (o, P, 3, 16, 5, one, 64, 64, C.byref(ins), 1.0, one, one, one, 1.0, 1.0, one, one, one, one, one, C.byref(gr), None)  # noqa: E731
    assert L.gsrast_backward_raw_aux(*br(10, C.byref(opts)), one, None) == -1 and b"cull" in L.gsrast_last_error()
    L.gsrast_options_init(C.byref(opts))
    assert L.gsrast_backward_raw_aux(*br(-1, C.byref(opts)), one, one) == -1


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
