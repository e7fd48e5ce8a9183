"""Call records (include/gsrast.h: gsrast_forward_call / gsrast_backward_call) for the host tests of the C ABI: a forward or backward
record of either family from keyword overrides over a default set in which every required pointer is 16 -- non-NULL, 16-byte aligned
and never dereferenced, because every call these tests make is refused (or has P = 0) before any device work -- and, optionally, a
truncated struct_size: what a caller compiled against an earlier header passes."""
import ctypes as C

from diff_gaussian_rasterization_ch3 import _C

ONE = 16
NO_ALLOC = _C._ALLOC_FN(lambda ctx, n: None)      # an allocation would fail: a refusal that got that far would say "allocation"
RAW_INPUTS = dict(xyz=ONE, rotation=ONE, scaling=ONE, opacity_logit=ONE, features_dc=ONE, features_rest=ONE)
RAW_GRADS = dict(dL_dmean2D=ONE, d_xyz=ONE, d_rotation=ONE, d_scaling=ONE, d_opacity_logit=ONE, d_features_dc=ONE, d_features_rest=ONE)
_CAMERA = dict(D=3, M=16, background=ONE, width=64, height=64, scale_modifier=1.0, viewmatrix=ONE, projmatrix=ONE, tan_fovx=0.5, tan_fovy=0.5)
_FORWARD = dict(_CAMERA, geometry_alloc=NO_ALLOC, binning_alloc=NO_ALLOC, image_alloc=NO_ALLOC, cam_pos=ONE, out_color=ONE, out_depth=ONE, radii=ONE)
_BACKWARD = dict(_CAMERA, R=5, campos=ONE, radii=ONE, geom_buffer=ONE, binning_buffer=ONE, image_buffer=ONE, dL_dpix=ONE)
_DENSE_IN = dict(means3D=ONE, shs=ONE, scales=ONE, rotations=ONE)
_DENSE_OUT = dict(dL_dmean2D=ONE, dL_dopacity=ONE, dL_dmean3D=ONE, dL_dsh=ONE, dL_dscale=ONE, dL_drot=ONE)
# the struct_size of a backward record by the last feature its header knew
SIZES = dict(min=_C.BackwardCallStruct.dL_dmean2D_abs.offset, abs=_C.BackwardCallStruct.dL_dcamera.offset, full=C.sizeof(_C.BackwardCallStruct))


def _record(cls, defaults, P, flags, family, size, over):
    raw = family == "raw"
    v = dict(defaults, P=P, flags=flags, family=_C.FAMILY_RAW if raw else _C.FAMILY_DENSE, **over)
    for k in ("raw", "raw_grads"):      # a dict of fields, a struct, or None
        if isinstance(v.get(k), dict):
            v[k] = (_C.RawInputsStruct if k == "raw" else _C.RawGradsStruct)(**v[k])
        if isinstance(v.get(k), C.Structure):
            v[k] = C.pointer(v[k])
    rec = cls(**{k: x for k, x in v.items() if x is not None})      # (None: the field stays NULL)
    rec.struct_size = C.sizeof(cls) if size is None else SIZES.get(size, size)
    return rec


def forward(P=10, flags=0, family="dense", size=None, **over):
    """A gsrast_forward_call.  family "dense" / "raw"; size: struct_size (default: the whole record); over: fields by name (`raw`: a dict of
    gsrast_raw_inputs fields or a RawInputsStruct)."""
    family_in = dict(raw=RAW_INPUTS) if family == "raw" else dict(_DENSE_IN, opacities=ONE)
    return _record(_C.ForwardCallStruct, dict(_FORWARD, **family_in), P, flags, family, size, over)


def backward(P=10, flags=0, family="dense", size=None, **over):
    """A gsrast_backward_call.  size: "min" / "abs" / "full" (SIZES) or a number of bytes (default: the whole record); `raw` / `raw_grads`
    as in forward()."""
    family_io = dict(raw=RAW_INPUTS, raw_grads=RAW_GRADS) if family == "raw" else dict(_DENSE_IN, **_DENSE_OUT)
    return _record(_C.BackwardCallStruct, dict(_BACKWARD, **family_io), P, flags, family, size, over)


def call(rec, options=None, ctx=None):
    """The record through its entry point: (return code, gsrast_last_error())."""
    L = _C.lib()
    if isinstance(rec, _C.ForwardCallStruct):
        rc = L.gsrast_render_forward(ctx, options, C.byref(rec))
    else:
        rc = L.gsrast_render_backward(options, C.byref(rec))
    return rc, L.gsrast_last_error()
