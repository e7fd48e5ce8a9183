"""`_C` -- the native binding layer of the drop-in package.

In the reference this module is a pybind11 torch extension (ext.cpp:15-19) exposing
``rasterize_gaussians``, ``rasterize_gaussians_backward`` and ``mark_visible``
(rasterize_points.cu:35-215).  Here the same three callables, with the same positional argument
lists and the same return tuples, marshal torch tensors onto the C ABI of ``include/gsrast.h``
(``libgsrast_hip.so``, hand-written HIP for gfx950) through ctypes: raw device pointers, sizes and
the current HIP stream -- no torch types cross the boundary.

There is NO fallback: if the shared library is missing or a tensor is not on a GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import threading
from typing import List, Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsrast_hip.so")

NUM_CHANNELS = 3  # reference config.h:15
ABI_VERSION = 6   # include/gsrast.h: GSRAST_ABI_VERSION this binding was written against

_ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_lib: Optional[C.CDLL] = None

# include/gsrast.h: the flags word of a call record
RENDER_AUX = 0x1
RENDER_ANTIALIAS = 0x2
RENDER_ABSGRAD = 0x4      # backward records whose struct_size covers dL_dmean2D_abs
RENDER_POSEGRAD = 0x8     # backward records whose struct_size covers dL_dcamera / pose_scratch
FAMILY_DENSE, FAMILY_RAW = 0, 1
FEATURES_MAX_C = 64       # include/gsrast.h: GSRAST_FEATURES_MAX_C
CAMERA_FLOATS = 35        # dL_dcamera: dL_dviewmatrix[16] | dL_dprojmatrix[16] | dL_dcampos[3]


class OptionsStruct(C.Structure):
    """gsrast_options (include/gsrast.h): everything that changes what ONE call computes / how it is scheduled."""
    _fields_ = [("exp_mode", C.c_int), ("binning", C.c_int), ("tile_clip", C.c_int), ("cull", C.c_int), ("lpt", C.c_int),
                ("speculative", C.c_int), ("fwd_pixels_per_lane", C.c_int), ("bwd_pixels_per_lane", C.c_int),
                ("sh_grad_factors", C.c_int), ("side_stream", C.c_int), ("grads_zeroed", C.c_int), ("backward_phase", C.c_int), ("depth_sort", C.c_int),
                ("forward_only", C.c_int), ("no_order_hint", C.c_int), ("dense_backward", C.c_int), ("no_list_cut", C.c_int)]


# Per-call options are kept PER HOST THREAD on the Python side and travel with every call (gsrast_render_forward /
# gsrast_render_backward): two threads rendering on two streams with different options never see each other's settings.
PER_CALL_OPTIONS = ("exp_mode", "binning", "tile_clip", "cull", "lpt", "speculative", "fwd_pixels_per_lane", "bwd_pixels_per_lane", "side_stream", "depth_sort", "forward_only", "no_order_hint", "dense_backward", "no_list_cut")
_OPTION_DEFAULTS = dict(exp_mode=0, binning=0, tile_clip=1, cull=1, lpt=1, speculative=1, fwd_pixels_per_lane=0, bwd_pixels_per_lane=0, side_stream=1, depth_sort=0, forward_only=0, no_order_hint=0, dense_backward=0, no_list_cut=0)
_OPTION_RANGE = dict(exp_mode=(0, 1, 2), binning=(0, 1), depth_sort=(0, 1), fwd_pixels_per_lane=(0, 1, 2, 4), bwd_pixels_per_lane=(0, 1, 2, 4))
_tls = threading.local()


def _thread_options() -> dict:
    o = getattr(_tls, "options", None)
    if o is None:
        o = _tls.options = dict(_OPTION_DEFAULTS)
    return o


def current_options() -> dict:
    """A copy of the calling thread's per-call options.  The autograd node stores it at forward time: autograd runs the
    backward on ITS OWN worker thread, which must use the options of the thread that issued the forward."""
    return dict(_thread_options())


_options_cache: dict = {}
_options_epoch = itertools.count(1)


def _options_struct(sh_grad_factors: bool = False, options: Optional[dict] = None, grads_zeroed: bool = False,
                    backward_phase: int = 0, forward_only: bool = False) -> OptionsStruct:
    """The gsrast_options value of one call.  The library copies it at entry, so one struct per distinct combination is built once and
    reused (round 6: fourteen setattr on a fresh ctypes Structure were ~8 us of every call's host time in front of the first launch)."""
    src = _thread_options() if options is None else options
    # (the calling thread's own dict is identified by its version -- bumped by set_option -- instead of by its fourteen items)
    ident = ("tls", getattr(_tls, "options_version", 0)) if options is None else tuple(src.items())      # (0 = the defaults; every set_option draws a process-wide unique number)
    key = (ident, bool(sh_grad_factors), bool(grads_zeroed), int(backward_phase), bool(forward_only))
    o = _options_cache.get(key)
    if o is None:
        o = OptionsStruct()
        for k, v in src.items():
            setattr(o, k, int(v))
        o.forward_only = int(bool(forward_only) or bool(o.forward_only))
        o.sh_grad_factors = int(bool(sh_grad_factors))
        o.grads_zeroed = int(bool(grads_zeroed))
        o.backward_phase = int(backward_phase)
        if len(_options_cache) > 256:
            _options_cache.clear()
        _options_cache[key] = o
    return o


class RawInputsStruct(C.Structure):
    """gsrast_raw_inputs (include/gsrast.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("xyz", "motion_res", "rotation", "rot_res", "scaling", "opacity_logit", "trbf",
                                          "features_dc", "features_rest", "shs_res")]


class RawGradsStruct(C.Structure):
    """gsrast_raw_grads (include/gsrast.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dL_dmean2D", "d_xyz", "d_rotation", "d_scaling", "d_rot_res", "d_opacity_logit", "d_trbf",
                                          "d_features_dc", "d_features_rest", "d_shs_res", "d_sh_factor")]


_fields = lambda *groups: [(n, t) for t, names in groups for n in names.split()]  # noqa: E731  ([(name, ctype), ...] from (ctype, "name name ...") groups)


class ForwardCallStruct(C.Structure):
    """gsrast_forward_call (include/gsrast.h)."""
    _fields_ = _fields((C.c_size_t, "struct_size"), (C.c_uint, "flags"), (C.c_int, "family"), (_ALLOC_FN, "geometry_alloc"), (C.c_void_p, "geometry_ctx"), (_ALLOC_FN, "binning_alloc"),
                       (C.c_void_p, "binning_ctx"), (_ALLOC_FN, "image_alloc"), (C.c_void_p, "image_ctx"), (C.c_int, "P D M"), (C.c_void_p, "background"), (C.c_int, "width height"),
                       (C.c_void_p, "means3D shs colors_precomp opacities scales rotations cov3D_precomp"), (C.POINTER(RawInputsStruct), "raw"), (C.c_float, "scale_modifier"),
                       (C.c_void_p, "viewmatrix projmatrix cam_pos"), (C.c_float, "tan_fovx tan_fovy"), (C.c_int, "prefiltered"), (C.c_void_p, "out_color out_depth radii stream out_acc_depth out_alpha"))


class BackwardCallStruct(C.Structure):
    """gsrast_backward_call (include/gsrast.h); GSRAST_BACKWARD_CALL_MIN ends in front of dL_dmean2D_abs, GSRAST_BACKWARD_CALL_ABS in front of dL_dcamera."""
    _fields_ = _fields((C.c_size_t, "struct_size"), (C.c_uint, "flags"), (C.c_int, "family"), (C.c_int, "P D M R"), (C.c_void_p, "background"), (C.c_int, "width height"),
                       (C.c_void_p, "means3D shs colors_precomp scales rotations cov3D_precomp"), (C.POINTER(RawInputsStruct), "raw"), (C.c_float, "scale_modifier"),
                       (C.c_void_p, "viewmatrix projmatrix campos"), (C.c_float, "tan_fovx tan_fovy"), (C.c_void_p, "radii geom_buffer binning_buffer image_buffer dL_dpix"),
                       (C.c_void_p, "dL_dmean2D dL_dconic dL_dopacity dL_dcolor dL_dmean3D dL_dcov3D dL_dsh dL_dscale dL_drot"), (C.POINTER(RawGradsStruct), "raw_grads"),
                       (C.c_void_p, "stream dL_dacc_depth dL_dalpha dL_dmean2D_abs dL_dcamera pose_scratch"))


class AdamGroupStruct(C.Structure):
    """gsrast_adam_group (include/gsrast.h)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("lr_rows", C.c_void_p), ("lr", C.c_float), ("rows", C.c_int), ("width", C.c_int)]


class DensifyGroupStruct(C.Structure):
    """gsrast_densify_group (include/gsrast.h)."""
    _fields_ = [("src", C.c_void_p), ("src_m", C.c_void_p), ("src_v", C.c_void_p), ("dst", C.c_void_p), ("dst_m", C.c_void_p), ("dst_v", C.c_void_p),
                ("width", C.c_int), ("role", C.c_int)]


DENSIFY_COPY, DENSIFY_XYZ, DENSIFY_SCALING = 0, 1, 2      # include/gsrast.h: GSRAST_DENSIFY_*
MCMC_COPY, MCMC_OPACITY, MCMC_SCALING = 0, 1, 2           # include/gsrast.h: GSRAST_MCMC_* (the role of a gsrast_densify_group in the mcmc calls)


MLP_FP32, MLP_BF16 = 0, 1                                  # include/gsrast.h: GSRAST_MLP_* (the precision of the gsrast_mlp3_*_p calls)


class Mlp3Struct(C.Structure):
    """gsrast_mlp3 (include/gsrast.h): the dims, the sigmoid flag and the pointers of one fused 3-layer head."""
    _fields_ = ([(k, C.c_int) for k in ("n", "d_x", "d_tail", "h1", "h2", "d_out", "sigmoid")]
                + [(k, C.c_void_p) for k in ("x", "x_tail", "w1", "b1", "w2", "b2", "w3", "b3", "y", "dy", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")])


class BilagridStruct(C.Structure):
    """gsrast_bilagrid (include/gsrast.h): the grid, the image (crop), where it lies in its frame, and the backward's slab count."""
    _fields_ = [(k, C.c_int) for k in ("GW", "GH", "L", "W", "H", "x0", "y0", "full_W", "full_H", "splits")]


PROJECT_ANTIALIAS = 1                                      # include/gsrast.h: GSRAST_PROJECT_ANTIALIAS


class ProjectStruct(C.Structure):
    """gsrast_project (include/gsrast.h): one projection's sizes, camera, inputs, flags, the five outputs, the four upstream gradients and the
    four gradient outputs.  The two calls take its address (C.addressof)."""
    _fields_ = ([(k, C.c_int) for k in ("P", "width", "height")] + [(k, C.c_float) for k in ("tanfovx", "tanfovy", "scale_modifier")]
                + [(k, C.c_void_p) for k in ("viewmatrix", "projmatrix", "means3D", "scales", "rotations", "cov3D_precomp")] + [("flags", C.c_uint)]
                + [(k, C.c_void_p) for k in ("means2D", "depths", "conics", "radii", "compensation", "dL_dmeans2D", "dL_ddepths", "dL_dconics",
                                             "dL_dcompensation", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dcov3D")])


class PlaneStruct(C.Structure):
    """gsrast_plane (include/gsrast.h)."""
    _fields_ = [("tex", C.c_void_p), ("grad_tex", C.c_void_p), ("W", C.c_int), ("H", C.c_int), ("cu", C.c_int), ("cv", C.c_int),
                ("max_mip_level", C.c_int), ("out_offset", C.c_int)]


_vp, _ci, _cf, _cd, _sz, _ll, _u32, _str = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_longlong, C.c_uint32, C.c_char_p
_opt, _adam, _dens, _mlp, _bila, _plane = (C.POINTER(S) for S in (OptionsStruct, AdamGroupStruct, DensifyGroupStruct, Mlp3Struct, BilagridStruct, PlaneStruct))
_vpp, _uints = C.POINTER(_vp), C.POINTER(C.c_uint)      # a host array of device pointers; a host array of counts

# name -> (restype, argtypes) of every function include/gsrast.h declares: the one place a signature is written (lib() binds each row;
# tests/test_capi_abi.py compares every row with its prototype).  A new C entry point is a new row here.
SIGNATURES = {
    # the render calls: the reference-shaped positional pair, and the pair over one call record each (the one this binding calls: _render_call)
    "gsrast_forward": (_ci, (_ALLOC_FN, _vp, _ALLOC_FN, _vp, _ALLOC_FN, _vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _ci, _vp, _vp, _vp, _vp)),
    "gsrast_backward": (_ci, (_ci, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _vp, _vp, _cf, _cf) + (_vp,) * 15),
    "gsrast_render_forward": (_ci, (_vp, _opt, C.POINTER(ForwardCallStruct))),
    "gsrast_render_backward": (_ci, (_opt, C.POINTER(BackwardCallStruct))),
    "gsrast_mark_visible": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_geometry_bytes": (_sz, (_ci,)),
    "gsrast_binning_bytes": (_sz, (_ci, _ci, _ci)),
    "gsrast_image_bytes": (_sz, (_ci, _ci)),
    "gsrast_pose_scratch_bytes": (_sz, (_ci,)),
    "gsrast_alloc_prealloc": (_vp, (_vp, _sz)),
    "gsrast_debug_export": (_ci, (_ci, _ci, _ci, _ci) + (_vp,) * 16),
    # options, contexts, the host-side plans, profiling
    "gsrast_options_init": (None, (_opt,)),
    "gsrast_context_create": (_vp, ()),
    "gsrast_context_destroy": (None, (_vp,)),
    "gsrast_context_query": (_ci, (_vp, _str)),
    "gsrast_policy_event": (_ci, (_vp, _str, _ci, _ci, _ci)),
    "gsrast_debug_forward_plan": (_ci, (_vp, _opt, C.c_uint, _ci, _ci, _ci, C.POINTER(_ci))),
    "gsrast_debug_backward_plan": (_ci, (_opt, C.c_uint, C.POINTER(_ci), C.POINTER(_ci))),
    "gsrast_set_option": (_ci, (_str, _ci)),
    "gsrast_get_option": (_ci, (_str,)),
    "gsrast_profile_kernel_count": (_ci, ()),
    "gsrast_profile_kernel_name": (_str, (_ci,)),
    "gsrast_profile_collect": (_ci, ()),
    "gsrast_profile_read": (_ci, (_ci, C.POINTER(_cd), C.POINTER(_ll))),
    "gsrast_profile_reset": (None, ()),
    "gsrast_last_error": (_str, ()),
    "gsrast_abi_version": (_ci, ()),
    # what runs on a forward's state: blend-weight statistics, feature maps, distortion maps
    "gsrast_contrib_scratch_bytes": (_sz, (_ci,)),
    "gsrast_contrib_stats": (_ci, (_opt, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_features_forward": (_ci, (_opt, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_features_backward": (_ci, (_opt, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_distortion_forward": (_ci, (_opt, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_distortion_backward": (_ci, (_opt, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_pixel_contributors": (_ci, (_opt, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _vp)),
    # the projection as a call of its own (the descriptor: ProjectStruct, passed by address)
    "gsrast_project_forward": (_ci, (_vp, _vp)),
    "gsrast_project_backward": (_ci, (_vp, _vp)),
    # normal consistency: Gaussian normals, depth-map normals, the fused loss
    "gsrast_gaussian_normals_forward": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_gaussian_normals_backward": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_depth_normal_forward": (_ci, (_ci, _ci, _cd, _cd, _vp, _vp, _vp)),
    "gsrast_depth_normal_backward": (_ci, (_ci, _ci, _cd, _cd, _vp, _vp, _vp, _vp)),
    "gsrast_normal_loss_scratch_bytes": (_sz, (_ci, _ci)),
    "gsrast_normal_loss_forward": (_ci, (_ci, _ci, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_normal_loss_backward": (_ci, (_ci, _ci, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    # Mip-Splatting's 3-D smoothing filter: the camera sweep, the fused activation
    "gsrast_filter3d_scratch_bytes": (_sz, (_ci, _ci)),
    "gsrast_filter3d_compute": (_ci, (_ci, _ci, _vp, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp)),
    "gsrast_filter3d_apply_forward": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_filter3d_apply_backward": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    # the multi-GPU gradient exchange
    "gsrast_sh_grad_combine": (_ci, (_ci, _ci, _ci, _ci, _vp, _vp, _sz, _cf, _vp, _vp)),
    "gsrast_sh_grad_combine_rows": (_ci, (_ci, _ci, _ci, _ci, _vp, _vp, _sz, _ci, _vp, _cf, _vp, _vp, _vp, _vp)),
    "gsrast_sh_grad_combine_union": (_ci, (_ci, _ci, _ci, _ci, _vp, _vp, _sz, _ci, _vp, _cf, _vp, _vp, _vp, _vp)),
    "gsrast_touched_rows": (_ci, (_ci, _vp, _vp, _vp)),
    "gsrast_rows_pack": (_ci, (_ll, _vp, _ci, _vpp, C.POINTER(_ci), _vp, _vp)),
    "gsrast_rows_unpack": (_ci, (_ll, _vp, _ci, _vpp, C.POINTER(_ci), _vp, _vp)),
    "gsrast_grad_rows_pack": (_ci, (_ci, _vp, _vpp, _vp, _vp, _u32, _vp)),
    "gsrast_grad_rows_clear": (_ci, (_ci, _vp, _ci, _sz, _u32, _vpp, _ci, _vp, _vp, _vp, _vp)),
    "gsrast_grad_rows_add": (_ci, (_ci, _vp, _u32, _vpp, _ci, _ci, _vp, _cf, _vp, _vp, _vp, _vp)),
    # loss, epilogue, Adam, k-NN
    "gsrast_loss_scratch_bytes": (_sz, (_ci, _ci, _ci)),
    "gsrast_loss_forward": (_ci, (_ci, _ci, _ci, _vp, _vp, _cf, _vp, _vp, _vp)),
    "gsrast_loss_backward": (_ci, (_ci, _ci, _ci, _vp, _vp, _cf, _vp, _vp, _vp, _vp)),
    "gsrast_activate_forward": (_ci, (_ci, _ci) + (_vp,) * 16),
    "gsrast_activate_backward": (_ci, (_ci,) + (_vp,) * 14),
    "gsrast_adam_step": (_ci, (_ci, _adam, _cd, _cd, _cd, _ci, _vp)),
    "gsrast_adam_step_visible": (_ci, (_ci, _adam, _vp, _ci, _ll, _cd, _cd, _cd, _ci, _vp)),
    "gsrast_knn_scratch_bytes": (_sz, (_ci,)),
    "gsrast_knn3_mean_dist2": (_ci, (_ci, _vp, _vp, _vp, _vp)),
    "gsrast_knn_query_scratch_bytes": (_sz, (_ci, _ci)),
    "gsrast_knn_query": (_ci, (_ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp)),
    # densification: clone / split / prune, and MCMC
    "gsrast_densify_scratch_bytes": (_sz, (_ci,)),
    "gsrast_densify_plan": (_ci, (_ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _cf, _vp, _vp, _vp)),
    "gsrast_densify_apply": (_ci, (_ci, _ci, _vp, _uints, _ci, _dens, _vp, _vp, _vp, _vp)),
    "gsrast_densify_scatter": (_ci, (_ci, _vp, _uints, _ci, _dens, _vp)),
    "gsrast_densify_stats_update": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp)),
    "gsrast_mcmc_scratch_bytes": (_sz, (_ci, _ci)),
    "gsrast_mcmc_plan": (_ci, (_ci, _vp, _vp, _cf, _vp, _vp, _vp, _vp)),
    "gsrast_mcmc_sample": (_ci, (_ci, _ci, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_mcmc_relocate": (_ci, (_ci, _ci, _vp, _vp, _uints, _cf, _ci, _dens, _vp)),
    "gsrast_mcmc_grow": (_ci, (_ci, _ci, _vp, _vp, _uints, _cf, _ci, _dens, _vp)),
    "gsrast_mcmc_noise": (_ci, (_ci, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _cf, _cf, _vp)),
    # the fused MLP heads, the temporal gate, the bilateral grid, the hexplane lookup
    "gsrast_mlp3_scratch_bytes": (_sz, (_mlp, _ci)),
    "gsrast_mlp3_forward": (_ci, (_mlp, _ci, _vp)),
    "gsrast_mlp3_backward": (_ci, (_mlp, _ci, _vp, _vp)),
    "gsrast_mlp3_scratch_bytes_p": (_sz, (_mlp, _ci, _ci)),
    "gsrast_mlp3_forward_p": (_ci, (_mlp, _ci, _ci, _vp)),
    "gsrast_mlp3_backward_p": (_ci, (_mlp, _ci, _ci, _vp, _vp)),
    "gsrast_temporal_gate_forward": (_ci, (_ci, _ci, _ci, _cf, _cf, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_temporal_gate_backward": (_ci, (_ci, _ci, _cf, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_temporal_integral": (_ci, (_ci, _ci, _cf, _cf, _cf, _cf, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_bilagrid_scratch_bytes": (_sz, (_bila,)),
    "gsrast_bilagrid_forward": (_ci, (_bila, _vp, _vp, _vp, _vp)),
    "gsrast_bilagrid_backward": (_ci, (_bila, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_bilagrid_tv": (_ci, (_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_hexplane_scratch_bytes": (_sz, (_ci, _plane, _ci, _ci)),
    "gsrast_hexplane_forward": (_ci, (_ci, _ci, _ci, _ci, _ci, _plane, _vp, _vp, _vp, _vp, _vp)),
    "gsrast_hexplane_backward": (_ci, (_ci, _ci, _ci, _ci, _ci, _plane, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp)),
}
EXPORTS = tuple(SIGNATURES)


def lib() -> C.CDLL:
    """Load libgsrast_hip.so (built by saro-gs_amd/build.py / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python saro-gs_amd/build.py` "
            "(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for the rasterizer.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    global _PREALLOC_CB
    _PREALLOC_CB = _ALLOC_FN(C.cast(L.gsrast_alloc_prealloc, C.c_void_p).value)      # the library's own C callback over pre-allocated memory (no trip into Python)
    if L.gsrast_abi_version() != ABI_VERSION:
        raise ImportError("libgsrast_hip.so: ABI version mismatch")
    _lib = L
    return L


def _err(code: int, where: str) -> RuntimeError:
    msg = lib().gsrast_last_error()
    return RuntimeError(f"{where} failed ({code}): {msg.decode() if msg else ''}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer, or NULL for an absent optional input (the reference passes CPU
    ``torch.Tensor([])`` and tests for a null data pointer, __init__.py:173-183)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _dev_f32(t: torch.Tensor, name: str, device: torch.device) -> torch.Tensor:
    if t.dtype is torch.float32 and t.device == device and t.is_contiguous():      # (the usual case: nothing to do)
        return t
    if t.numel() == 0:
        return t
    if t.device != device:
        raise RuntimeError(f"{name} must live on {device} (got {t.device})")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _require_gpu(t: torch.Tensor) -> torch.device:
    if not t.is_cuda:
        raise RuntimeError("gsrast: tensors must be on a GPU (HIP) device; there is no CPU fallback")
    return t.device


class GradArena:
    """Optional zero-copy gradient bucket for the multi-GPU path (view_parallel.py).

    When installed with ``set_grad_arena``, ``rasterize_gaussians_backward`` carves the leaf
    gradients it returns (means3D, sh, opacities, scales, rotations) out of ONE flat fp32 buffer, in
    that order, so the cross-rank exchange is a single in-place all-reduce of ``flat`` with no pack /
    unpack copies (the same idea as DDP's gradient-as-bucket-view).  The screen-space gradient
    (means2D) is deliberately NOT in the bucket: the reference only ever uses its per-view norm
    (train.py:212), which is reduced separately as a [P] statistic.  Not part of the reference's _C:
    without an arena the outputs are ordinary tensors, exactly as before.

    Contract: the arena holds the gradients of ONE step.  The first backward after ``zero_grad()`` writes its leaf gradients
    into the arena (autograd adopts the views as ``.grad``); a further backward before the next ``zero_grad()`` -- the
    reference's batch loop, or ``views_of_rank`` yielding several views per rank -- gets ordinary tensors, which autograd
    ADDS into those ``.grad`` views (the sum of the views' gradients, as ``cache_gradient`` keeps it,
    scene/saro_gaussian.py:242-247).  With ``sh_factors=True`` a second backward raises: the factor buffer holds exactly one
    view's factor.  Call ``zero_grad()`` (after ``optimizer.zero_grad(set_to_none=True)``) at the start of every step."""

    ORDER = (("means3D", 3), ("sh", None), ("opacity", 1), ("scales", 3), ("rotations", 4))
    # sh_factors=True: the dense part first (one contiguous all-reduce), dL/dsh last -- it is not exchanged at all: the
    # backward writes the per-view FACTOR g[P,3] of dL/dsh (include/gsrast.h, gsrast_sh_grad_combine) into `factor`,
    # ranks all-gather the factors (+ their camera positions) and every rank recombines dL/dsh locally.
    ORDER_FACTORS = (("means3D", 3), ("opacity", 1), ("scales", 3), ("rotations", 4), ("sh", None))
    # raw=True (round 4): the bucket of GaussianRasterizerRaw's six LEAVES -- SaRO-GS's own call pattern, where the rasterizer's
    # `shs` is cat(features_dc, features_rest) [+ residual], never a leaf (scene/saro_gaussian.py:836-845): dense part first, the
    # two SH leaves last (with sh_factors they are completed by gsrast_sh_grad_combine_rows after the exchange)
    ORDER_RAW = (("xyz", 3), ("opacity_logit", 1), ("scaling", 3), ("rotation", 4), ("features_dc", 3), ("features_rest", -1))

    def __init__(self, P: int, M: int, device: torch.device, sh_factors: bool = False, world: int = 1, raw: bool = False):
        self.P, self.M, self.sh_factors, self.world, self.raw = P, M, bool(sh_factors), int(world), bool(raw)
        order = self.ORDER_RAW if raw else (self.ORDER_FACTORS if sh_factors else self.ORDER)
        self.widths = {name: (M * 3 if w is None else ((M - 1) * 3 if w == -1 else w)) for name, w in order}
        self.offsets, o = {}, 0
        for name, _ in order:
            self.offsets[name] = o
            o += ((P * self.widths[name] + 3) // 4) * 4        # every segment starts on a 16-byte boundary (float4 stores of dL/drot)
        self.flat = torch.zeros(o, dtype=torch.float32, device=device)
        self.dirty = False                                     # a backward has written this step's gradients
        self.dense_names = tuple(n for n, _ in order if n not in ("sh", "features_dc", "features_rest"))
        if sh_factors:
            self.dense = self.flat[: self.offsets["features_dc" if raw else "sh"]]   # 11 floats / Gaussian: the all-reduced part
            self.chunk = ((3 * P + 3 + 3) // 4) * 4                            # [3P g | 3 campos | pad], 16-byte multiple
            self.factor = torch.zeros(self.chunk, dtype=torch.float32, device=device)
            self.gathered = torch.zeros(self.world * self.chunk, dtype=torch.float32, device=device)
        self.last_degree = 0

    def zero_grad(self) -> None:
        """Start of a step: the next backward writes into the arena again.  (Does not touch memory: the backward overwrites
        every element; set the leaves' .grad to None first, or autograd would add the arena to itself.)"""
        self.dirty = False

    def dense_segments(self):
        """The dense (non-SH) gradient arrays as [P, w] views of the bucket, in bucket order."""
        return [self.flat[self.offsets[n]: self.offsets[n] + self.P * self.widths[n]].view(self.P, self.widths[n]) for n in self.dense_names]

    def take(self, name: str, shape, zero: bool) -> torch.Tensor:
        n = self.P * self.widths[name]
        v = self.flat[self.offsets[name]: self.offsets[name] + n].view(shape)   # a fresh view every call
        if zero:
            v.zero_()
        return v


def _export_touched(ar: "GradArena", P: int, geomBuffer: torch.Tensor, dev: torch.device) -> None:
    """gsrast_touched_rows into the arena (round 5): one byte per Gaussian, 1 = some pixel of THIS view consumed it -- what the sparse
    exchange (view_parallel.exchange_gradients(sparse=True)) takes the union over ranks of, instead of scanning the gradient arrays."""
    pending = getattr(ar, "touched_reader_event", None)      # somebody still reads the previous step's flags on another stream
    if pending is not None:
        pending.synchronize()
        ar.touched_reader_event = None
    t = getattr(ar, "touched", None)
    if t is None or t.numel() != P or t.device != dev:
        t = ar.touched = torch.empty(P, dtype=torch.uint8, device=dev)
    launch("gsrast_touched_rows", dev, P, _ptr(geomBuffer), t.data_ptr())
    ar.touched_fresh = True
    ar.touched_seq = getattr(ar, "touched_seq", 0) + 1       # which backward these flags belong to (view_parallel._touched_hook tags its capacity event with it)


_grad_arena: Optional[GradArena] = None
_factor_ready_hook = None
_touched_ready_hook = None


def set_grad_arena(arena: Optional[GradArena]) -> None:
    global _grad_arena
    _grad_arena = arena


def set_factor_ready_hook(fn) -> None:
    """fn(arena) is called INSIDE the backward of a factor-mode arena, between the blend backward (after which arena.factor --
    the view's factor of dL/dsh and its camera position -- is final on the current stream) and the per-Gaussian backward:
    view_parallel starts the asynchronous all-gather of the factors there, so that it runs beside the second phase."""
    global _factor_ready_hook
    _factor_ready_hook = fn


def set_touched_ready_hook(fn) -> None:
    """fn(arena) is called INSIDE the backward of a factor-mode arena BEFORE any of its kernels is enqueued, right after arena.touched
    (one byte per Gaussian: some pixel of this view consumed it) has been written on the current stream."""
    global _touched_ready_hook
    _touched_ready_hook = fn


POISON_STATE_BUFFERS = bool(int(os.environ.get("GSRAST_POISON_STATE", "0")))      # tests: every state buffer is handed out filled with 0xFF bytes (NaN as floats, all-ones as bits / indices)


_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_of(dev: torch.device) -> int:
    """The raw handle of torch's current stream on `dev` (what every launch of a call goes to).  torch.cuda.current_stream(dev).cuda_stream builds a
    Stream object per call (~3 us); torch's own raw accessor -- the one its compiled-code launchers use -- returns the handle directly."""
    if _get_raw_stream is not None and dev.index is not None:
        return _get_raw_stream(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


class PreallocStruct(C.Structure):
    """gsrast_prealloc (include/gsrast.h)."""
    _fields_ = [("ptr", C.c_void_p), ("capacity", C.c_size_t), ("requested", C.c_size_t)]


_PREALLOC_CB = None
PREALLOC_STATE = True       # geometry / image state buffers are allocated BEFORE the forward's C call and handed over through gsrast_alloc_prealloc
                            # (round 6: two Python callbacks fewer in front of the first launch); False: all three through Python callbacks, as rounds 1-5
_size_cache: dict = {}


def _state_bytes(P: int, W: int, H: int):
    k = (P, W, H)
    v = _size_cache.get(k)
    if v is None:
        L = lib()
        if len(_size_cache) > 64:
            _size_cache.clear()
        v = _size_cache[k] = (int(L.gsrast_geometry_bytes(P)), int(L.gsrast_image_bytes(W, H)))
    return v


class _on_device:
    """`with torch.cuda.device(dev)` without its cost when `dev` already is the current device (the usual case: two runtime calls and a
    Python context manager's bookkeeping per entry point, in front of the first launch)."""
    __slots__ = ("dev", "inner")

    def __init__(self, dev: torch.device):
        self.dev, self.inner = dev, None

    def __enter__(self):
        idx = self.dev.index
        if idx is not None and idx != torch.cuda.current_device():
            self.inner = torch.cuda.device(self.dev)
            self.inner.__enter__()
        return self

    def __exit__(self, *exc):
        if self.inner is not None:
            return self.inner.__exit__(*exc)
        return False


def launch(name: str, dev: torch.device, *args) -> None:
    """The library's `name`(*args, stream) -- how every training kernel is launched: `dev` made current if it is not, the stream torch's
    current one on `dev`; raises _err on a non-zero result.  (Not the render calls: _render_call.)"""
    with _on_device(dev):
        rc = getattr(lib(), name)(*args, _stream_of(dev))
    if rc != 0:
        raise _err(rc, name)


def scratch_bytes(name: str, *args) -> int:
    """The library's `name`(*args) of the *_scratch_bytes calls whose 0 is a refusal: raises with the reason the call left in gsrast_last_error."""
    n = getattr(lib(), name)(*args)
    if n == 0:
        raise _err(-1, name)
    return n


class _Arena:
    """The three resizable state buffers of the reference (rasterize_points.cu:27-33, :71-78):
    each allocation callback creates one uint8 tensor that is later saved for backward."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buffers: List[Optional[torch.Tensor]] = [None, None, None]
        self.callbacks = [_ALLOC_FN(self._make(i)) for i in range(3)]  # keep references alive
        self.pre = (PreallocStruct * 2)()                              # geometry, image (gsrast_alloc_prealloc)

    def forward_allocators(self, P: int, W: int, H: int):
        """(geometry_alloc, geometry_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx) of one forward.  With PREALLOC_STATE the geometry
        and image buffers are allocated here, their sizes being known (gsrast_geometry_bytes / gsrast_image_bytes), and the library's own C
        callback hands them out; the binning buffer, whose size the library decides, keeps the Python callback."""
        if not PREALLOC_STATE or P <= 0:
            return (self.callbacks[0], None, self.callbacks[1], None, self.callbacks[2], None)
        gb, ib = _state_bytes(P, W, H)
        geom = torch.empty(gb, dtype=torch.uint8, device=self.device)
        img = torch.empty(ib, dtype=torch.uint8, device=self.device)
        if POISON_STATE_BUFFERS:
            geom.fill_(255); img.fill_(255)
        self.buffers[0], self.buffers[2] = geom, img
        pre = self.pre
        pre[0].ptr, pre[0].capacity = geom.data_ptr(), gb
        pre[1].ptr, pre[1].capacity = img.data_ptr(), ib
        return (_PREALLOC_CB, C.addressof(pre[0]), self.callbacks[1], None, _PREALLOC_CB, C.addressof(pre[1]))

    @staticmethod
    def acquire(device: torch.device) -> "_Arena":
        """An arena of the calling thread's pool (round 6): building three ctypes callbacks per forward cost ~20 us of host time in front of
        the first launch; a pooled arena keeps its callbacks and only ever holds buffers between acquire() and close()."""
        pool = getattr(_tls, "arena_pool", None)
        if pool is None:
            pool = _tls.arena_pool = []
        if pool:
            a = pool.pop()
            a.device = device
            return a
        return _Arena(device)

    def _make(self, slot: int):
        def alloc(_ctx, nbytes):
            try:
                buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
                if POISON_STATE_BUFFERS:
                    buf.fill_(255)
            except Exception:  # out of memory -> NULL -> GSRAST_E_ALLOC
                return None
            self.buffers[slot] = buf
            return buf.data_ptr()
        return alloc

    def tensor(self, slot: int) -> torch.Tensor:
        b = self.buffers[slot]
        return b if b is not None else torch.empty(0, dtype=torch.uint8, device=self.device)

    def close(self) -> None:
        """Drop the callbacks and the buffer references.  The callbacks are closures over `self`, so the arena sits in
        a reference cycle: without this the three state buffers (hundreds of MB) stay alive until Python's CYCLIC
        collector happens to run, the caching allocator sees them freed at irregular times and occasionally has to
        hipMalloc fresh blocks in the middle of a training loop (a ~250 ms stall)."""
        self.buffers = [None, None, None]       # (the callbacks stay: the arena goes back to its thread's pool, holding nothing)
        pool = getattr(_tls, "arena_pool", None)
        if pool is not None and len(pool) < 8:
            pool.append(self)
        else:
            self.callbacks = None


def _render_call(entry: str, head: tuple, rec, flags: int, absgrad: Optional[torch.Tensor] = None,
                 camera: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> int:
    """The one native render call: gsrast_render_forward / gsrast_render_backward (`entry`) on the call record `rec`, whose inputs the caller has filled
    by name (include/gsrast.h).  Returns its result (forward: the number of rendered instances), raises on an error code.  Backward: `absgrad`, the [P,2] sink
    of GSRAST_RENDER_ABSGRAD; `camera`, (the [35] output, the scratch) of GSRAST_RENDER_POSEGRAD (_pose_buffers); either sets its bit and its fields."""
    if absgrad is not None:
        flags, rec.dL_dmean2D_abs = flags | RENDER_ABSGRAD, absgrad.data_ptr()
    if camera is not None:
        flags, rec.dL_dcamera, rec.pose_scratch = flags | RENDER_POSEGRAD, camera[0].data_ptr(), camera[1].data_ptr()
    rec.struct_size, rec.flags = C.sizeof(rec), flags
    rc = getattr(lib(), entry)(*head, rec)
    if rc < 0:
        raise _err(rc, entry)
    return rc


def _per_stream(cache: dict, P: int, dev: torch.device, make):
    """cache's entry for (device, current stream, P), made by make() on its first use: scratch that one call at a time owns on its stream."""
    k = (dev.index, int(_stream_of(dev) or 0), P)
    v = cache.get(k)
    if v is None:
        if len(cache) > 16:
            cache.clear()
        v = cache[k] = make()
    return v


_pose_cache: dict = {}
_contrib_cache: dict = {}


def _pose_buffers(P: int, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(the [35] float32 output, the scratch) of a backward with GSRAST_RENDER_POSEGRAD, kept per device, stream and P: both are fully
    overwritten by every such backward (zeroed here for P = 0, which makes no call), and the backward hands autograd a copy of the output."""
    v = _per_stream(_pose_cache, P, dev, lambda: (torch.empty((CAMERA_FLOATS,), dtype=torch.float32, device=dev),
                                                  torch.empty((int(lib().gsrast_pose_scratch_bytes(P)),), dtype=torch.uint8, device=dev)))
    if P == 0:
        v[0].zero_()
    return v


def _camera_result(camera: Optional[Tuple[torch.Tensor, torch.Tensor]]):
    """(dL_dviewmatrix [4,4], dL_dprojmatrix [4,4], dL_dcampos [3]): views of one fresh copy of the cached output."""
    g = camera[0].clone()
    return g[:16].view(4, 4), g[16:32].view(4, 4), g[32:]


def _forward(rec: ForwardCallStruct, dev: torch.device, forward_only: bool, aux: bool, antialiasing: bool):
    """What the dense and the raw forward share: the outputs, the state arena, the call (`rec`: the record with the family's inputs
    filled in) and the return tuple."""
    P, H, W = rec.P, rec.height, rec.width
    o = dict(dtype=torch.float32, device=dev)
    out_color, out_depth = torch.empty((NUM_CHANNELS, H, W), **o), torch.empty((1, H, W), **o)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    aux_out = (torch.empty((1, H, W), **o), torch.empty((1, H, W), **o)) if aux else ()
    arena = _Arena.acquire(dev)
    try:
        with _on_device(dev):
            (rec.geometry_alloc, rec.geometry_ctx, rec.binning_alloc, rec.binning_ctx, rec.image_alloc, rec.image_ctx) = arena.forward_allocators(P, W, H)
            rec.out_color, rec.out_depth, rec.radii, rec.stream = out_color.data_ptr(), out_depth.data_ptr(), _ptr(radii), _stream_of(dev)
            rec.out_acc_depth, rec.out_alpha = (aux_out[0].data_ptr(), aux_out[1].data_ptr()) if aux else (None, None)
            rendered = _render_call("gsrast_render_forward", (_current_context(), _options_struct(forward_only=forward_only)),       # context: the innermost `with Context()` of the calling thread, else the thread's own
                                    rec, (RENDER_AUX if aux else 0) | (RENDER_ANTIALIAS if antialiasing else 0))
        return (rendered, out_color, radii, arena.tensor(0), arena.tensor(1), arena.tensor(2), out_depth) + aux_out
    finally:
        arena.close()       # break the arena <-> callback cycle now, not whenever the cyclic GC runs


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height,
                        image_width, sh, degree, campos, prefiltered, *, forward_only: bool = False, aux: bool = False,
                        antialiasing: bool = False) -> Tuple[torch.Tensor, ...]:
    """Forward.  Mirrors RasterizeGaussiansCUDA (rasterize_points.cu:35-115): returns
    ``(num_rendered, out_color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer,
    out_depth[1,H,W])``.  `forward_only` (not in the reference): no backward will follow on the returned state (the autograd
    node passes it when no input requires a gradient): the library skips what it only prepares for the backward.
    `aux` (not in the reference): GSRAST_RENDER_AUX, the tuple continues with ``acc_depth[1,H,W], alpha[1,H,W]``
    (include/gsrast.h); without it nothing more is allocated.
    `antialiasing` (not in the reference): GSRAST_RENDER_ANTIALIAS -- the opacity-compensated 2-D filter; the
    backward on the returned state must be given antialiasing=True as well."""
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:56-58
    dev = _require_gpu(means3D)
    P, H, W = int(means3D.shape[0]), int(image_height), int(image_width)
    f = lambda t, n: _dev_f32(t, n, dev)  # noqa: E731
    background, means3D, colors, opacity = f(background, "bg"), f(means3D, "means3D"), f(colors, "colors_precomp"), f(opacity, "opacities")
    scales, rotations, cov3D_precomp = f(scales, "scales"), f(rotations, "rotations"), f(cov3D_precomp, "cov3D_precomp")
    viewmatrix, projmatrix, sh, campos = f(viewmatrix, "viewmatrix"), f(projmatrix, "projmatrix"), f(sh, "shs"), f(campos, "campos")
    M = int(sh.shape[1]) if sh.numel() != 0 else 0  # rasterize_points.cu:83-87
    rec = ForwardCallStruct(family=FAMILY_DENSE, P=P, D=int(degree), M=M, background=background.data_ptr(), width=W, height=H, means3D=means3D.data_ptr(), shs=_ptr(sh),
                            colors_precomp=_ptr(colors), opacities=opacity.data_ptr(), scales=_ptr(scales), rotations=_ptr(rotations), cov3D_precomp=_ptr(cov3D_precomp),
                            scale_modifier=float(scale_modifier), viewmatrix=viewmatrix.data_ptr(), projmatrix=projmatrix.data_ptr(), cam_pos=_ptr(campos),
                            tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy), prefiltered=int(bool(prefiltered)))
    return _forward(rec, dev, forward_only, aux, antialiasing)


def _claim_grad_arena(fits, P: int, campos: torch.Tensor, degree: int, no_factors: Optional[str] = None) -> Optional["GradArena"]:
    """The installed GradArena if this backward writes into it, else None: it must fit the call (`fits(arena)`) and be clean -- a second
    backward of the same step gets ordinary tensors (GradArena docstring), which factor mode cannot allow.  `no_factors`: why this call
    cannot be served in factor mode.  A claimed arena is marked dirty; in factor mode the camera position goes behind the factor."""
    ar = _grad_arena
    if ar is None or not fits(ar):
        return None
    if ar.dirty:
        if ar.sh_factors:
            raise RuntimeError("GradArena(sh_factors=True): a second backward before zero_grad() would overwrite the first view's "
                               "factor; use one view per rank and exchange, or the plain arena (which accumulates)")
        return None                     # ordinary tensors: autograd adds them into the arena views it adopted as .grad
    if ar.sh_factors and no_factors:
        raise RuntimeError(no_factors)
    ar.dirty = True
    if ar.sh_factors:
        # the SH gradient (views of the arena) is returned to autograd as usual but only becomes valid after
        # sh_grad_combine(); the kernel writes this view's factor g[P,3] (+ the camera position behind it)
        ar.factor[3 * P: 3 * P + 3].copy_(campos.reshape(-1)[:3])
        ar.last_degree = int(degree)
    return ar


def _run_backward(ar: Optional["GradArena"], call, P: int, geomBuffer: torch.Tensor, dev: torch.device) -> None:
    """call(phase) enqueues the native backward (0: all of it).  In factor mode the touched rows are exported first and, with a
    factor-ready hook, the backward runs in two phases around it: on one call record, only the options differ."""
    factors = ar is not None and ar.sh_factors
    if factors:
        # which rows this view can touch is known since the forward's blend (its untouched bits): exported BEFORE the backward
        # is enqueued, so that a caller's hook can start on it -- the all-gather exchange agrees on its row capacity beside
        # the backward instead of waiting for it (view_parallel._touched_hook)
        _export_touched(ar, P, geomBuffer, dev)
        if _touched_ready_hook is not None:
            _touched_ready_hook(ar)
    if factors and _factor_ready_hook is not None:
        call(1)                      # blend backward + the factors
        _factor_ready_hook(ar)       # e.g. the asynchronous all-gather of the factors
        call(2)                      # the per-Gaussian backward, beside it
    else:
        call(0)


def _backward(rec: BackwardCallStruct, flags: int, ar: Optional["GradArena"], sh_grad_factors: bool, dev: torch.device, radii: torch.Tensor,
              geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imageBuffer: torch.Tensor, options: Optional[dict], first_backward: bool,
              absgrad: Optional[torch.Tensor], camera_grads: bool, features: Optional[tuple], distortion: Optional[tuple] = None):
    """What the dense and the raw backward share behind their outputs (`rec`: the record with the family's inputs and outputs filled in; the
    forward's state, the stream and the keyword-driven fields are filled here): the pose buffers, the feature map's and the distortion map's
    steps between the phases, the call -- through _run_backward, or around that step -- and the results the keywords add: ((dL_dviewmatrix, dL_dprojmatrix,
    dL_dcampos) or None, dL_dfeatures or None)."""
    P = rec.P
    camera = _pose_buffers(P, dev) if camera_grads else None
    between, dL_dfeatures = _features_between(features, ar, P, rec.R, rec.width, rec.height, geomBuffer, binningBuffer, imageBuffer, options, dev)
    between = _distortion_between(distortion, between, ar, P, rec.R, rec.width, rec.height, geomBuffer, binningBuffer, imageBuffer, options, dev)
    if P != 0:
        with _on_device(dev):
            radii = radii.contiguous()
            rec.radii, rec.geom_buffer, rec.binning_buffer, rec.image_buffer = _ptr(radii), _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer)
            rec.stream = _stream_of(dev)
            call = lambda phase: _render_call(      # noqa: E731  (options travel per call: no process-wide switch is flipped)
                "gsrast_render_backward", (_options_struct(sh_grad_factors=sh_grad_factors, options=options, grads_zeroed=first_backward, backward_phase=phase),), rec, flags, absgrad, camera)
            if between is None:
                _run_backward(ar, call, P, geomBuffer, dev)
            else:
                _run_backward_around(call, between)
    return (None if camera is None else _camera_result(camera)), dL_dfeatures


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, *, options: Optional[dict] = None,
                                 first_backward: bool = False, dL_dacc_depth: Optional[torch.Tensor] = None,
                                 dL_dalpha: Optional[torch.Tensor] = None, antialiasing: bool = False,
                                 absgrad: Optional[torch.Tensor] = None, camera_grads: bool = False, features: Optional[tuple] = None,
                                 distortion: Optional[tuple] = None):
    """Backward.  Mirrors RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-194): returns
    ``(dL_dmeans2D[P,3], dL_dcolors[P,3], dL_dopacity[P,1], dL_dmeans3D[P,3], dL_dcov3D[P,6],
    dL_dsh[P,M,3], dL_dscales[P,3], dL_drotations[P,4])``.  `options` (not in the reference): the per-call options to use
    instead of the calling thread's (current_options() captured at forward time); `first_backward`: no backward has touched
    geomBuffer since its forward, whose gradient records are therefore still zero (the library skips its zero-fill).
    `dL_dacc_depth` / `dL_dalpha` ([1,H,W] or None = zero): the upstream gradients of the aux outputs -- GSRAST_RENDER_AUX when
    either is given.  `antialiasing`: the state comes from an antialiasing=True forward (GSRAST_RENDER_ANTIALIAS; the same flags for
    both phases of a two-phase backward).  `absgrad`: a [P,2] sink (check_absgrad) that the call overwrites with the absolute
    screen-space gradient (include/gsrast.h: GSRAST_RENDER_ABSGRAD); it is no gradient of anything and never lives in a GradArena.
    `camera_grads`: the tuple continues with ``(dL_dviewmatrix[4,4], dL_dprojmatrix[4,4], dL_dcampos[3])`` (include/gsrast.h:
    GSRAST_RENDER_POSEGRAD); without it the call and its result are what they were before the flag existed.
    `features`: (features [P,C], dL_dfeature_map [C,H,W]) of a feature map rendered from this state (features_forward) whose gradient is
    not zero -- the backward then runs in two phases around gsrast_features_backward, every returned gradient includes the map's loss
    (`absgrad` does not) and the tuple ends with ``dL_dfeatures[P,C]`` (behind the camera's); without it the call is what it was.
    `distortion`: (moments [2,H,W], dL_ddistort [H,W]) of a distortion map rendered from this state (distortion_forward) whose gradient is
    not zero -- the backward runs in two phases around gsrast_distortion_backward (beside the feature map's step, if any), with
    GSRAST_RENDER_AUX and a zero dL_dacc_depth of its own when no aux gradient is given (the per-Gaussian phase then consumes dL/dz); every
    returned gradient includes the map's loss (`absgrad` does not), the tuple is unchanged."""
    dev = _require_gpu(means3D)
    P = int(means3D.shape[0])
    check_absgrad(absgrad, P, dev)
    H, W = int(dL_dout_color.shape[1]), int(dL_dout_color.shape[2])  # rasterize_points.cu:141-142
    dL_dacc_depth = _distortion_aux(distortion, dL_dacc_depth, dL_dalpha, H, W, dev, options)
    flags, aux, _keep = _backward_flags(dL_dacc_depth, dL_dalpha, H, W, dev, antialiasing)
    f = lambda t, n: _dev_f32(t, n, dev)  # noqa: E731
    background, means3D, colors = f(background, "bg"), f(means3D, "means3D"), f(colors, "colors_precomp")
    scales, rotations, cov3D_precomp = f(scales, "scales"), f(rotations, "rotations"), f(cov3D_precomp, "cov3D_precomp")
    viewmatrix, projmatrix, sh, campos = f(viewmatrix, "viewmatrix"), f(projmatrix, "projmatrix"), f(sh, "shs"), f(campos, "campos")
    dL_dout_color = f(dL_dout_color, "dL_dout_color")
    M = int(sh.shape[1]) if sh.numel() != 0 else 0
    opts = dict(dtype=torch.float32, device=dev)
    use_sh = sh.numel() != 0 and colors.numel() == 0
    use_sr = cov3D_precomp.numel() == 0
    # (the arena only serves the SH + scale/rotation training path)
    ar = _claim_grad_arena(lambda a: a.P == P and a.M == M and use_sh and use_sr and a.flat.device == dev, P, campos, degree)

    def out(name, shape, zero):
        if ar is not None and name in ar.offsets:
            return ar.take(name, shape, zero)
        return torch.zeros(shape, **opts) if zero else torch.empty(shape, **opts)

    # Nothing is zero-filled here: the library accumulates into its own 64-byte-per-Gaussian records inside geomBuffer and
    # writes every returned array exactly once (include/gsrast.h).  dL_dconic (an intermediate of the reference) is not
    # requested at all.
    dL_dmeans2D = torch.empty((P, 3), **opts)
    dL_dopacity = out("opacity", (P, 1), False)
    # with SH colours dL_dcolors is an intermediate nobody reads (the node returns None for the absent colors_precomp input):
    # not written -- an empty tensor in its place, like dL_dcov3D below (12 B / Gaussian of the bandwidth-bound per-Gaussian backward)
    dL_dcolors = torch.empty((0, NUM_CHANNELS) if use_sh else (P, NUM_CHANNELS), **opts)
    dL_dmeans3D = out("means3D", (P, 3), False)
    # with scales / rotations dL_dcov3D is an intermediate nobody reads (the autograd node returns None for the absent
    # cov3D_precomp input): not computed, not written -- the binding returns an empty tensor in its place
    dL_dcov3D = torch.empty((0, 6) if use_sr else (P, 6), **opts)
    dL_dsh = out("sh", (P, M, 3), not use_sh)
    factors = ar is not None and ar.sh_factors      # dL_dsh is then only valid after sh_grad_combine(): the kernel writes this view's factor
    dL_dscales = out("scales", (P, 3), not use_sr)
    dL_drotations = out("rotations", (P, 4), not use_sr)
    rec = BackwardCallStruct(
        family=FAMILY_DENSE, P=P, D=int(degree), M=M, R=int(R), background=_ptr(background), width=W, height=H, means3D=_ptr(means3D), shs=_ptr(sh),
        colors_precomp=_ptr(colors), scales=_ptr(scales), rotations=_ptr(rotations), cov3D_precomp=_ptr(cov3D_precomp), scale_modifier=float(scale_modifier),
        viewmatrix=_ptr(viewmatrix), projmatrix=_ptr(projmatrix), campos=_ptr(campos), tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy),
        dL_dpix=_ptr(dL_dout_color), dL_dmean2D=_ptr(dL_dmeans2D), dL_dopacity=_ptr(dL_dopacity), dL_dcolor=_ptr(dL_dcolors), dL_dmean3D=_ptr(dL_dmeans3D), dL_dcov3D=_ptr(dL_dcov3D),
        dL_dsh=ar.factor.data_ptr() if factors else _ptr(dL_dsh), dL_dscale=_ptr(dL_dscales), dL_drot=_ptr(dL_drotations), dL_dacc_depth=aux[0], dL_dalpha=aux[1])
    grad_camera, dL_dfeatures = _backward(rec, flags, ar, factors, dev, radii, geomBuffer, binningBuffer, imageBuffer, options, first_backward, absgrad, camera_grads, features,
                                          distortion)
    grads = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    grads = grads if grad_camera is None else grads + (grad_camera,)
    return grads if features is None else grads + (dL_dfeatures,)


def _check_tensor(name: str, t, shapes: tuple, dev: torch.device, no_grad: Optional[str] = None, channels: Optional[tuple] = None) -> None:
    """The one ladder of check_absgrad / check_contrib / check_features: `t` is a contiguous float32 tensor on `dev` in one of `shapes`
    (an extent of None, printed as C: any -- then within `channels` = (lowest, highest)); `no_grad`: it must not require grad, and why.
    ValueError otherwise."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor or None (got {type(t).__name__})")
    if not any(len(s) == t.ndim and all(w is None or w == int(n) for w, n in zip(s, t.shape)) for s in shapes):
        want = " or ".join("[" + ", ".join("C" if w is None else str(w) for w in s) + "]" for s in shapes)
        raise ValueError(f"{name} must be {want} (got {list(t.shape)})")
    if channels is not None and not channels[0] <= int(t.shape[-1]) <= channels[1]:
        raise ValueError(f"{name} must have {channels[0]}..{channels[1]} channels (got {int(t.shape[-1])})")
    if t.dtype is not torch.float32:
        raise ValueError(f"{name} must be float32 (got {t.dtype})")
    if t.device != dev:
        raise ValueError(f"{name} must live on {dev} (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if no_grad is not None and t.requires_grad:
        raise ValueError(f"{name} {no_grad} (requires_grad must be False)")


def check_absgrad(absgrad: Optional[torch.Tensor], P: int, dev: torch.device) -> None:
    """The caller-owned sink of the absolute screen-space gradient: a contiguous float32 [P,2] tensor on the render's device (None: not
    wanted).  ValueError otherwise -- the library gets a pointer and would write P * 2 floats through it."""
    if absgrad is not None:
        _check_tensor("absgrad", absgrad, ((P, 2),), dev, no_grad="is a statistic the backward writes, not a differentiable tensor")


def check_contrib(contrib: Optional[torch.Tensor], pixel_weights: Optional[torch.Tensor], P: int, H: int, W: int, dev: torch.device) -> None:
    """The caller-owned sink of the blend-weight statistics (`contrib=`): a contiguous float32 [P,4] tensor on the render's device (None: not
    wanted), and its optional per-pixel weights (`pixel_weights=`): a contiguous float32 [H,W] or [1,H,W] tensor on the same device, only legal
    together with a sink.  ValueError otherwise -- the library gets pointers and would write P * 4 floats / read H * W floats through them."""
    if contrib is None:
        if pixel_weights is not None:
            raise ValueError("pixel_weights is only legal together with contrib")
        return
    for name, t, shapes in (("contrib", contrib, ((P, 4),)), ("pixel_weights", pixel_weights, ((H, W), (1, H, W)))):
        if t is not None:
            _check_tensor(name, t, shapes, dev, no_grad="is not a differentiable tensor")
    if contrib.numel() != 0 and contrib.device.type != "meta" and contrib.data_ptr() % 16 != 0:
        raise ValueError("contrib must be 16-byte aligned (rows of a fresh or row-sliced [*, 4] float32 tensor are)")


def _contrib_scratch(P: int, dev: torch.device) -> torch.Tensor:
    """The accumulators of gsrast_contrib_stats, kept per device, stream and P (the call zeroes them itself and leaves them zeroed)."""
    return _per_stream(_contrib_cache, P, dev, lambda: torch.empty((int(lib().gsrast_contrib_scratch_bytes(P)),), dtype=torch.uint8, device=dev))


def contrib_stats(contrib: torch.Tensor, pixel_weights: Optional[torch.Tensor], R: int, W: int, H: int, geomBuffer: torch.Tensor,
                  binningBuffer: torch.Tensor, imageBuffer: torch.Tensor, *, options: Optional[dict] = None) -> torch.Tensor:
    """gsrast_contrib_stats (include/gsrast.h) on the state a forward returned: OVERWRITES `contrib` [P,4] with the per-Gaussian rows
    [weight_sum, weight_max, pixel_count, top_count] on the current stream, behind everything the forward enqueued there.  Valid until a
    backward runs on the state.  `options`: the per-call options of that forward (default: the calling thread's)."""
    P = int(contrib.shape[0])
    dev = _require_gpu(contrib)
    check_contrib(contrib, pixel_weights, P, int(H), int(W), dev)
    if P == 0:
        return contrib
    launch("gsrast_contrib_stats", dev, C.byref(_options_struct(options=options)), P, int(R), int(W), int(H), _ptr(geomBuffer), _ptr(binningBuffer),
         _ptr(imageBuffer), _ptr(pixel_weights), contrib.data_ptr(), _contrib_scratch(P, dev).data_ptr())
    return contrib


def check_features(features: Optional[torch.Tensor], P: int, dev: torch.device) -> None:
    """The per-Gaussian feature vectors of `features=`: a contiguous float32 [P, C] tensor on the render's device, 1 <= C <= FEATURES_MAX_C
    (None: not wanted).  It may require grad.  ValueError otherwise -- the library gets a pointer and would read P * C floats through it."""
    if features is not None:
        _check_tensor("features", features, ((P, None),), dev, channels=(1, FEATURES_MAX_C))


def no_arena_for_features() -> None:
    if _grad_arena is not None:
        raise RuntimeError("features= is not supported with a GradArena installed (multi-GPU / view_parallel training): the arena drives the "
                           "backward's two phases itself; uninstall it with _C.set_grad_arena(None) for renders that need a feature map")


def features_forward(features: torch.Tensor, R: int, W: int, H: int, geomBuffer: torch.Tensor, binningBuffer: torch.Tensor,
                     imageBuffer: torch.Tensor, *, options: Optional[dict] = None) -> torch.Tensor:
    """gsrast_features_forward (include/gsrast.h) on the state a forward returned: feature_map [C,H,W] = sum_i alpha_i T_i features[i], over
    the forward's own contributors, on the current stream behind everything the forward enqueued there.  `options`: the per-call options
    of that forward (default: the calling thread's)."""
    P = int(features.shape[0])
    dev = _require_gpu(features)
    check_features(features, P, dev)
    Cn = int(features.shape[1])
    out = torch.empty((Cn, int(H), int(W)), dtype=torch.float32, device=dev)
    launch("gsrast_features_forward", dev, C.byref(_options_struct(options=options)), P, int(R), Cn, int(W), int(H), _ptr(geomBuffer), _ptr(binningBuffer),
         _ptr(imageBuffer), _ptr(features), out.data_ptr())
    return out


def _run_backward_around(call, between) -> None:
    """The backward of a render whose feature map has a gradient (never with an arena: _features_between): the two phases of call(phase)
    around between(), on one call record -- only the options differ."""
    call(1)                      # blend backward: the gradient records exist
    between()                    # gsrast_features_backward adds the feature map's part to them
    call(2)                      # the per-Gaussian backward consumes them


def _features_between(features: Optional[tuple], ar, P: int, R: int, W: int, H: int, geomBuffer, binningBuffer, imageBuffer, options, dev):
    """(what a backward with `features` = (features, dL_dfeature_map) runs between its two phases, the dL_dfeatures [P,C] it fills); (None,
    None) without.  The call (gsrast_features_backward) adds the map's part to the gradient records phase 1 left and phase 2 consumes."""
    if features is None:
        return None, None
    if ar is not None:
        raise RuntimeError("a feature map's gradient cannot be served with a GradArena claimed by this backward")
    feats, dL_dmap = features
    check_features(feats, P, dev)
    Cn = int(feats.shape[1])
    if tuple(dL_dmap.shape) != (Cn, H, W):
        raise RuntimeError(f"dL_dfeature_map must be [{Cn},{H},{W}] (got {list(dL_dmap.shape)})")
    dL_dmap = _dev_f32(dL_dmap, "dL_dfeature_map", dev)
    dL_dfeatures = torch.empty((P, Cn), dtype=torch.float32, device=dev)

    def between():
        launch("gsrast_features_backward", dev, C.byref(_options_struct(options=options)), P, R, Cn, W, H, _ptr(geomBuffer), _ptr(binningBuffer),
             _ptr(imageBuffer), _ptr(feats), dL_dmap.data_ptr(), _ptr(dL_dfeatures))
    return between, dL_dfeatures


def no_arena_for_distortion() -> None:
    if _grad_arena is not None:
        raise RuntimeError("distortion= is not supported with a GradArena installed (multi-GPU / view_parallel training): the arena drives the "
                           "backward's two phases itself; uninstall it with _C.set_grad_arena(None) for renders that need a distortion map")


def distortion_forward(P: int, R: int, W: int, H: int, geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imageBuffer: torch.Tensor,
                       dev: torch.device, *, options: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gsrast_distortion_forward (include/gsrast.h) on the state a forward of P Gaussians returned: (distort_map [H,W] = sum_ij w_i w_j
    |z_i - z_j| over the forward's own contributors, moments [2,H,W] for distortion's backward), on the current stream behind everything the
    forward enqueued there.  `options`: the per-call options of that forward (default: the calling thread's)."""
    out = torch.empty((int(H), int(W)), dtype=torch.float32, device=dev)
    moments = torch.empty((2, int(H), int(W)), dtype=torch.float32, device=dev)
    launch("gsrast_distortion_forward", dev, C.byref(_options_struct(options=options)), int(P), int(R), int(W), int(H), _ptr(geomBuffer), _ptr(binningBuffer),
         _ptr(imageBuffer), out.data_ptr(), moments.data_ptr())
    return out, moments


TOPK_MAX = 16                                              # include/gsrast.h: gsrast_pixel_contributors takes 1 <= K <= 16
TOPK_ORDERS = {"weight": 0, "depth": 1}


def _gaussians_of_state(geomBuffer: torch.Tensor) -> int:
    """A number of Gaussians whose geometry buffer has this one's size (0 for an empty one).  Every array of that buffer grows with P and is
    rounded up on its own, so two P of one total size have one layout: whichever is found addresses the state like the forward's own P."""
    nbytes = int(geomBuffer.numel())
    if nbytes == 0:
        return 0
    size = lib().gsrast_geometry_bytes
    lo, hi = 1, 1
    while int(size(hi)) < nbytes:
        lo, hi = hi, hi * 2
        if hi > 1 << 30:
            raise ValueError("pixel_contributors: geomBuffer is no forward's geometry buffer (too large)")
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if int(size(mid)) >= nbytes else (mid + 1, hi)
    if int(size(lo)) != nbytes:
        raise ValueError(f"pixel_contributors: geomBuffer is no forward's geometry buffer ({nbytes} bytes)")
    return lo


def check_pixel_contributors(K, order) -> int:
    """The C call's `order` (0 weight, 1 depth) of a query for K slots per pixel; ValueError for a K outside 1..TOPK_MAX or no int, and for
    an order that is neither "weight" nor "depth" (nor the C call's 0 / 1)."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= TOPK_MAX:
        raise ValueError(f"pixel_contributors: K must be an int in 1..{TOPK_MAX} (got {K!r})")
    if isinstance(order, str) and order in TOPK_ORDERS:
        return TOPK_ORDERS[order]
    if not isinstance(order, bool) and isinstance(order, int) and order in (0, 1):
        return order
    raise ValueError(f"pixel_contributors: order must be 'weight' or 'depth' (got {order!r})")


def pixel_contributors(K: int, order, R: int, W: int, H: int, geomBuffer: torch.Tensor, binningBuffer: torch.Tensor, imageBuffer: torch.Tensor, *,
                       options: Optional[dict] = None, with_count: bool = True, P: Optional[int] = None):
    """gsrast_pixel_contributors (include/gsrast.h) on the state any forward returned, dense or raw family: (ids [K,H,W] int32, weights
    [K,H,W] float32, count [H,W] int32 or None without `with_count`) -- each pixel's heaviest (order "weight" / 0: descending, slot 0 the
    `top` Gaussian of contrib_stats) or first (order "depth" / 1: blend order) K contributors, -1 / +0.0 in unused slots, and how many
    contributors it has in all.  On the current stream, behind everything the forward enqueued there; valid until a backward runs on the
    state.  Nothing is differentiable.  `options`: the per-call options of that forward (default: the calling thread's); `P`: that
    forward's number of Gaussians (default: recovered from the geometry buffer's size)."""
    order = check_pixel_contributors(K, order)
    dev = _require_gpu(imageBuffer)
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError(f"pixel_contributors: the image must not be empty (got {W} x {H})")
    P = _gaussians_of_state(geomBuffer) if P is None else int(P)
    ids = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    weights = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev) if with_count else None
    launch("gsrast_pixel_contributors", dev, C.byref(_options_struct(options=options)), P, int(R), W, H, _ptr(geomBuffer), _ptr(binningBuffer),
           _ptr(imageBuffer), K, order, ids.data_ptr(), weights.data_ptr(), None if count is None else count.data_ptr())
    return ids, weights, count


def _distortion_aux(distortion: Optional[tuple], dL_dacc_depth, dL_dalpha, H: int, W: int, dev: torch.device, options: Optional[dict]):
    """The dL_dacc_depth of a backward: the caller's -- or, with `distortion` and no aux gradient at all, a zero one of the call's own, so that
    the record carries GSRAST_RENDER_AUX and the per-Gaussian phase reads float 9 of the gradient records (dL/dz).  That plan needs the
    culled blend kernels, and options.cull is the only switch the backward's plan reads for that (gsrast_policy.h: culled_blend(o, true) is
    cull != 0), so its refusal is raised here, under the keyword's name, before the library would refuse "acc_depth / alpha gradients"."""
    if distortion is None:
        return dL_dacc_depth
    if int((_thread_options() if options is None else options).get("cull", 1)) == 0:
        raise RuntimeError("distortion=True: the gradient of the distortion map needs the culled blend kernels (options.cull != 0)")
    if dL_dacc_depth is None and dL_dalpha is None:
        return torch.zeros((1, H, W), dtype=torch.float32, device=dev)
    return dL_dacc_depth


def _distortion_between(distortion: Optional[tuple], between, ar, P: int, R: int, W: int, H: int, geomBuffer, binningBuffer, imageBuffer, options, dev):
    """What a backward runs between its two phases: `between` (the feature map's step, or None) and, with `distortion` = (moments,
    dL_ddistort), gsrast_distortion_backward -- it adds the map's part to the gradient records phase 1 left and phase 2 consumes (floats
    0-5, and dL/dz in float 9).  The two only add: their order does not matter."""
    if distortion is None:
        return between
    if ar is not None:
        raise RuntimeError("a distortion map's gradient cannot be served with a GradArena claimed by this backward")
    moments, dL_dmap = distortion
    if tuple(moments.shape) != (2, H, W) or dL_dmap.numel() != H * W:
        raise RuntimeError(f"distortion: moments must be [2,{H},{W}] and dL_ddistort [{H},{W}] (got {list(moments.shape)}, {list(dL_dmap.shape)})")
    moments, dL_dmap = _dev_f32(moments, "moments", dev), _dev_f32(dL_dmap, "dL_ddistort", dev)

    def both():
        if between is not None:
            between()
        launch("gsrast_distortion_backward", dev, C.byref(_options_struct(options=options)), P, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer),
             _ptr(imageBuffer), moments.data_ptr(), dL_dmap.data_ptr())
    return both


def _backward_flags(dL_dacc_depth, dL_dalpha, H: int, W: int, dev: torch.device, antialiasing: bool):
    """A backward's (flags, (dL/dacc_depth, dL/dalpha) pointers, the tensors they point into): each gradient a contiguous fp32 [1,H,W]
    device tensor or None = zero; GSRAST_RENDER_AUX when either is given."""
    flags = RENDER_ANTIALIAS if antialiasing else 0
    if dL_dacc_depth is None and dL_dalpha is None:
        return flags, (None, None), ()
    keep = []
    for t, n in ((dL_dacc_depth, "dL_dacc_depth"), (dL_dalpha, "dL_dalpha")):
        if t is not None:
            if t.numel() != H * W:
                raise RuntimeError(f"{n} must hold one value per pixel ([1,{H},{W}])")
            t = _dev_f32(t, n, dev)
        keep.append(t)
    return flags | RENDER_AUX, (_ptr(keep[0]), _ptr(keep[1])), keep


# ---- raw-parameter entry points (include/gsrast.h: GSRAST_FAMILY_RAW records; no counterpart in the reference's _C) ----
RAW_NAMES = ("xyz", "motion_res", "rotation", "rot_res", "scaling", "opacity_logit", "trbf", "features_dc", "features_rest", "shs_res")


def _raw_struct(raw: dict, dev: torch.device, P: int):
    """raw: name -> tensor or None (RAW_NAMES).  Returns (struct, the contiguous tensors it points into, M)."""
    keep = {}
    for n in RAW_NAMES:
        t = raw.get(n)
        if t is not None and t.numel() == 0 and P != 0:
            t = None
        keep[n] = None if t is None else _dev_f32(t, n, dev)
    for n in ("xyz", "rotation", "scaling", "opacity_logit", "features_dc", "features_rest"):
        if keep[n] is None:
            raise RuntimeError(f"rasterize_gaussians_raw: {n} is required")
    if keep["xyz"].ndim != 2 or keep["xyz"].shape[1] != 3:
        raise RuntimeError("xyz must have dimensions (num_points, 3)")
    M = 1 + int(keep["features_rest"].shape[1])
    shapes = dict(motion_res=(P, 3), rotation=(P, 4), rot_res=(P, 7), scaling=(P, 3), features_dc=(P, 1, 3), features_rest=(P, M - 1, 3),
                  shs_res=(P, M, 3))
    for n, shp in shapes.items():
        if keep[n] is not None and tuple(keep[n].shape) != shp:
            raise RuntimeError(f"rasterize_gaussians_raw: {n} must be {list(shp)} (got {list(keep[n].shape)})")
    for n in ("opacity_logit", "trbf"):
        if keep[n] is not None and keep[n].numel() != P:
            raise RuntimeError(f"rasterize_gaussians_raw: {n} must hold one value per Gaussian")
    st = RawInputsStruct(**{n: _ptr(keep[n]) for n in RAW_NAMES})
    return st, keep, M


def rasterize_gaussians_raw(background, raw: dict, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width,
                            degree, campos, *, forward_only: bool = False, aux: bool = False, antialiasing: bool = False):
    """rasterize_gaussians taking the model's raw leaves + optional residuals (`raw`: RAW_NAMES -> tensor / None); the activations
    of scene/saro_gaussian.py:39-47, :807-847 run inside the per-Gaussian kernels.  Same return tuple (`aux`: + acc_depth, alpha;
    `antialiasing`: as rasterize_gaussians)."""
    dev = _require_gpu(raw["xyz"])
    P, H, W = int(raw["xyz"].shape[0]), int(image_height), int(image_width)
    st, keep, M = _raw_struct(raw, dev, P)
    f = lambda t, n: _dev_f32(t, n, dev)  # noqa: E731
    background, viewmatrix, projmatrix, campos = f(background, "bg"), f(viewmatrix, "viewmatrix"), f(projmatrix, "projmatrix"), f(campos, "campos")
    rec = ForwardCallStruct(family=FAMILY_RAW, P=P, D=int(degree), M=M, background=_ptr(background), width=W, height=H, raw=C.pointer(st), scale_modifier=float(scale_modifier),
                            viewmatrix=_ptr(viewmatrix), projmatrix=_ptr(projmatrix), cam_pos=_ptr(campos), tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy))
    return _forward(rec, dev, forward_only, aux, antialiasing)


def rasterize_gaussians_raw_backward(background, raw: dict, radii, scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                     degree, campos, geomBuffer, R, binningBuffer, imageBuffer, *, options: Optional[dict] = None,
                                     first_backward: bool = False, dL_dacc_depth: Optional[torch.Tensor] = None,
                                     dL_dalpha: Optional[torch.Tensor] = None, antialiasing: bool = False,
                                     absgrad: Optional[torch.Tensor] = None, camera_grads: bool = False, features: Optional[tuple] = None,
                                     distortion: Optional[tuple] = None) -> dict:
    """Gradients of the raw leaves: dict with dL_dmeans2D [P,3], xyz (= motion_res), rotation, scaling, opacity_logit [P,1], features_dc,
    features_rest, and -- when the residual was given -- rot_res [P,7], trbf [P,1], shs_res [P,M,3].  `dL_dacc_depth` / `dL_dalpha`: as
    rasterize_gaussians_backward; `antialiasing`, `absgrad`: as rasterize_gaussians_backward; `camera_grads`: also "camera", the
    (dL_dviewmatrix, dL_dprojmatrix, dL_dcampos) of rasterize_gaussians_backward; `features`: as rasterize_gaussians_backward, the result
    then has "features" (dL_dfeatures [P,C]); `distortion`: as rasterize_gaussians_backward."""
    dev = _require_gpu(raw["xyz"])
    P = int(raw["xyz"].shape[0])
    check_absgrad(absgrad, P, dev)
    H, W = int(dL_dout_color.shape[1]), int(dL_dout_color.shape[2])
    st, keep, M = _raw_struct(raw, dev, P)
    f = lambda t, n: _dev_f32(t, n, dev)  # noqa: E731
    background, viewmatrix, projmatrix, campos = f(background, "bg"), f(viewmatrix, "viewmatrix"), f(projmatrix, "projmatrix"), f(campos, "campos")
    dL_dout_color = f(dL_dout_color, "dL_dout_color")
    dL_dacc_depth = _distortion_aux(distortion, dL_dacc_depth, dL_dalpha, H, W, dev, options)
    flags, aux, _keep = _backward_flags(dL_dacc_depth, dL_dalpha, H, W, dev, antialiasing)
    o = dict(dtype=torch.float32, device=dev)
    ar = _claim_grad_arena(      # (else: the bucket of another call shape)
        lambda a: getattr(a, "raw", False) and a.P == P and a.M == M and a.flat.device == dev, P, campos, degree,
        no_factors=None if keep["shs_res"] is None else
        "GradArena(raw=True, sh_factors=True) cannot serve a call with shs_residual: every rank needs the whole "
        "gradient of its own residual; use GradArena(raw=True) + view_parallel.allreduce_mean_inplace")
    factors = ar is not None and ar.sh_factors

    def out(name, shape):
        return ar.take(name, shape, False) if ar is not None else torch.empty(shape, **o)

    g = dict(dL_dmeans2D=torch.empty((P, 3), **o), xyz=out("xyz", (P, 3)), rotation=out("rotation", (P, 4)), scaling=out("scaling", (P, 3)),
             opacity_logit=out("opacity_logit", (P, 1)))
    if keep["rot_res"] is not None:
        g["rot_res"] = torch.empty((P, 7), **o)
    if keep["trbf"] is not None:
        g["trbf"] = torch.empty((P, 1), **o)
    if keep["shs_res"] is not None:
        g["shs_res"] = torch.empty((P, M, 3), **o)
    # the two SH leaves get their own contiguous gradients also when the residual's gradient holds the same rows: autograd would copy
    # strided slices of it into the leaves' .grad (two elementwise kernels, 96 us at 1 M), the kernel writes them for a third of that
    g["features_dc"], g["features_rest"] = out("features_dc", (P, 1, 3)), out("features_rest", (P, M - 1, 3))
    p_dc, p_rest = g["features_dc"].data_ptr(), _ptr(g["features_rest"])
    p_fac = None
    if factors:     # the two SH leaves' gradients are then only valid after sh_grad_combine(): the kernel writes this view's factor
        p_dc, p_rest, p_fac = None, None, ar.factor.data_ptr()
    gs = RawGradsStruct(dL_dmean2D=g["dL_dmeans2D"].data_ptr(), d_xyz=g["xyz"].data_ptr(), d_rotation=g["rotation"].data_ptr(),
                        d_scaling=g["scaling"].data_ptr(), d_rot_res=_ptr(g.get("rot_res")), d_opacity_logit=g["opacity_logit"].data_ptr(),
                        d_trbf=_ptr(g.get("trbf")), d_features_dc=p_dc, d_features_rest=p_rest, d_shs_res=_ptr(g.get("shs_res")),
                        d_sh_factor=p_fac)
    rec = BackwardCallStruct(
        family=FAMILY_RAW, P=P, D=int(degree), M=M, R=int(R), background=_ptr(background), width=W, height=H, raw=C.pointer(st), scale_modifier=float(scale_modifier),
        viewmatrix=_ptr(viewmatrix), projmatrix=_ptr(projmatrix), campos=_ptr(campos), tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy),
        dL_dpix=_ptr(dL_dout_color), raw_grads=C.pointer(gs), dL_dacc_depth=aux[0], dL_dalpha=aux[1])
    # (sh_grad_factors stays off: a raw factor call is told by d_sh_factor in its gradient record)
    grad_camera, dL_dfeatures = _backward(rec, flags, ar, False, dev, radii, geomBuffer, binningBuffer, imageBuffer, options, first_backward, absgrad, camera_grads, features,
                                          distortion)
    if features is not None:
        g["features"] = dL_dfeatures
    if grad_camera is not None:
        g["camera"] = grad_camera
    if keep["motion_res"] is not None:
        g["motion_res"] = g["xyz"]
    return g


def sh_grad_combine(arena: "GradArena", means3D: torch.Tensor, chunks: torch.Tensor, n_views: int, scale: float,
                    rows: Optional[int] = None, row_of: Optional[torch.Tensor] = None, chunk_stride: Optional[int] = None,
                    idx: Optional[torch.Tensor] = None):
    """dL/dsh of `n_views` views from their factors (include/gsrast.h: gsrast_sh_grad_combine / _rows / _union), written into the
    arena's SH region(s) -- the tensor(s) autograd already handed out as shs.grad, or as features_dc.grad / features_rest.grad for a
    raw arena.  rows / row_of: the records hold only `rows` factors, Gaussian i's is row row_of[i] (int32 [P], -1 = not sent).

    idx (int64 [rows], ascending, distinct; round 5) instead of row_of: record row j is Gaussian idx[j]'s, and ONLY those rows of the
    SH region are written.  The region is kept zero elsewhere from one step to the next: the rows of the previous union are cleared
    first (the whole region once after a dense combine or a fresh arena).  Whoever writes into those .grad tensors in a way that makes
    a zero row non-zero must set arena.sh_rows_known = False."""
    P, M = arena.P, arena.M
    if getattr(arena, "raw", False):
        whole, dc, rest = None, arena.take("features_dc", (P, 1, 3), False), arena.take("features_rest", (P, M - 1, 3), False)
    else:
        whole, dc, rest = arena.take("sh", (P, M, 3), False), None, None
    if P == 0:
        return whole if whole is not None else (dc, rest)
    dev = means3D.device
    union = idx is not None and (M * 3) % 4 == 0 and M * 3 <= 48
    if union:
        views = [v.view(P, -1) for v in (whole, dc, rest) if v is not None and v.numel()]
        prev = getattr(arena, "_sh_union", None)
        arena._rows_prev = None                      # (the all-gather exchange keeps its own record of the rows it wrote)
        if not getattr(arena, "sh_rows_known", False) or prev is None:
            for v in views:
                v.zero_()
        else:
            for v in views:
                v.index_fill_(0, prev, 0.0)
        arena._sh_union, arena.sh_rows_known = idx, True
        launch("gsrast_sh_grad_combine_union", dev, P, int(arena.last_degree), M, int(n_views), means3D.data_ptr(), chunks.data_ptr(),
             int(chunk_stride if chunk_stride is not None else arena.chunk), int(idx.numel()), idx.data_ptr(), float(scale), _ptr(whole), _ptr(dc), _ptr(rest))
        return whole if whole is not None else (dc, rest)
    if idx is not None:                  # (an M the union kernel does not take: the row map form)
        row_of = torch.full((P,), -1, dtype=torch.int32, device=dev)
        row_of[idx] = torch.arange(idx.numel(), dtype=torch.int32, device=dev)
        rows = int(idx.numel())
    arena.sh_rows_known = False
    launch("gsrast_sh_grad_combine_rows", dev, P, int(arena.last_degree), M, int(n_views), means3D.data_ptr(), chunks.data_ptr(),
         int(chunk_stride if chunk_stride is not None else arena.chunk), int(P if rows is None else rows),
         None if row_of is None else row_of.data_ptr(), float(scale), _ptr(whole), _ptr(dc), _ptr(rest))
    return whole if whole is not None else (dc, rest)


def rows_pack(idx: torch.Tensor, arrays, packed: torch.Tensor, unpack: bool = False) -> torch.Tensor:
    """Rows `idx` (int64) of the [P, w_k] float32 arrays side by side in packed [n, sum w_k] (include/gsrast.h: gsrast_rows_pack), or --
    unpack=True -- back into those rows.  One launch either way."""
    n, k = int(idx.numel()), len(arrays)
    widths = [int(a.shape[1]) for a in arrays]
    if packed.shape != (n, sum(widths)) or not packed.is_contiguous() or any(not a.is_contiguous() for a in arrays):
        raise ValueError("rows_pack: packed must be a contiguous [n, sum of widths] array, the arrays contiguous")
    ptrs = (C.c_void_p * k)(*[a.data_ptr() for a in arrays])
    wid = (C.c_int * k)(*widths)
    launch("gsrast_rows_unpack" if unpack else "gsrast_rows_pack", packed.device, n, idx.data_ptr(), k, ptrs, wid, packed.data_ptr())
    return packed


# ---- the all-gather gradient exchange (include/gsrast.h: gsrast_grad_rows_*; csrc/gsrast_exchange.h) -----------------------------------
GRAD_ROW_WORDS = 16


def _arena_sh_arrays(arena: "GradArena"):
    P, M = arena.P, arena.M
    if getattr(arena, "raw", False):
        return None, arena.take("features_dc", (P, 1, 3), False), (arena.take("features_rest", (P, M - 1, 3), False) if M > 1 else None)
    return arena.take("sh", (P, M, 3), False), None, None


def _dense_ptrs(arena: "GradArena"):
    segs = arena.dense_segments()
    if [int(sg.shape[1]) for sg in segs] != [3, 1, 3, 4]:
        raise ValueError("the gradient rows hold mean 3 | opacity 1 | scale 3 | rotation 4: the arena's dense segments differ")
    return (C.c_void_p * 4)(*[sg.data_ptr() for sg in segs])


def grad_rows_pack(arena: "GradArena", touched: torch.Tensor, rows: torch.Tensor) -> None:
    """This rank's touched gradient rows into rows[1:] (int32 [1 + cap, 16]; rows[0, 0], zeroed by the caller, counts them)."""
    launch("gsrast_grad_rows_pack", rows.device, arena.P, touched.data_ptr(), _dense_ptrs(arena), arena.factor.data_ptr(), rows.data_ptr(), int(rows.shape[0]) - 1)


def grad_rows_clear(arena: "GradArena", chunks: torch.Tensor, dense: bool, sh: bool) -> None:
    """Zero the rows the chunks (int32 [n, 1 + cap, 16]) name: of the dense arrays and / or of the SH region(s)."""
    n, cap = int(chunks.shape[0]), int(chunks.shape[1]) - 1
    whole, dc, rest = _arena_sh_arrays(arena) if sh else (None, None, None)
    launch("gsrast_grad_rows_clear", chunks.device, arena.P, chunks.data_ptr(), n, (1 + cap) * GRAD_ROW_WORDS, cap, _dense_ptrs(arena) if dense else None, arena.M,
         _ptr(whole), _ptr(dc), _ptr(rest))


def grad_rows_add(arena: "GradArena", chunk: torch.Tensor, means3D: torch.Tensor, scale: float) -> None:
    """One rank's chunk (int32 [1 + cap, 16]) added into the arena: the dense rows and, recombined from the factor, dL/dsh."""
    whole, dc, rest = _arena_sh_arrays(arena)
    launch("gsrast_grad_rows_add", chunk.device, arena.P, chunk.data_ptr(), int(chunk.shape[0]) - 1, _dense_ptrs(arena), int(arena.last_degree), arena.M,
         means3D.data_ptr(), float(scale), _ptr(whole), _ptr(dc), _ptr(rest))


def mark_visible(means3D, viewmatrix, projmatrix) -> torch.Tensor:
    """Mirrors markVisible (rasterize_points.cu:196-215): bool[P], view-space z > 0.2."""
    dev = _require_gpu(means3D)
    P = int(means3D.shape[0])
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P != 0:
        means3D, viewmatrix, projmatrix = (_dev_f32(t, n, dev) for t, n in
                                           ((means3D, "means3D"), (viewmatrix, "viewmatrix"), (projmatrix, "projmatrix")))
        launch("gsrast_mark_visible", dev, P, means3D.data_ptr(), viewmatrix.data_ptr(), projmatrix.data_ptr(), present.data_ptr())
    return present


# ---- not part of the reference's _C: options, profiling and the parity-test state export --------
def set_option(name: str, value: int) -> None:
    """Per-call options (PER_CALL_OPTIONS; "pixels_per_lane" sets both directions) are set for the CALLING THREAD and passed
    with each of its calls; the process-wide diagnostics ("profile", "debug_sync", "hexplane_scatter", ...) go to the library."""
    value = int(value)
    names = ("fwd_pixels_per_lane", "bwd_pixels_per_lane") if name == "pixels_per_lane" else (name,)
    if all(n in _OPTION_DEFAULTS for n in names):
        for n in names:
            if n in _OPTION_RANGE:
                if value not in _OPTION_RANGE[n]:
                    raise ValueError(f"gsrast: unknown option or bad value: {name}={value}")
                _thread_options()[n] = value
            else:
                _thread_options()[n] = 1 if value else 0
        _tls.options_version = next(_options_epoch)          # (a new, process-wide unique identity for the cached option structs)
        return
    if lib().gsrast_set_option(name.encode(), value) != 0:
        raise ValueError(f"gsrast: unknown option or bad value: {name}={value}")


def get_option(name: str) -> int:
    if name == "pixels_per_lane":
        name = "fwd_pixels_per_lane"
    if name in _OPTION_DEFAULTS:
        return int(_thread_options()[name])
    return int(lib().gsrast_get_option(name.encode()))


class Context:
    """A caller-owned gsrast_context (include/gsrast.h: gsrast_context_create / _destroy): the state a sequence of similar views shares --
    capacity hints of the speculative launch, the depth sort's history, the pose table with its launch-order hints and cut depths, the
    side streams.  By default every host thread has one of its own; a caller that keeps SEVERAL views in flight on several streams of one
    thread (view_parallel.distributed_step(views_in_flight=n)) gives each lane its own, so that the lanes' forwards do not share side
    streams, gate words and adaptive state:

        ctx = _C.Context()
        with ctx:                      # forwards issued by this thread inside the block use ctx
            color, radii, depth = GaussianRasterizer(settings)(...)
        ctx.close()                    # frees its device memory (or let the object die)

    Results never depend on which context a call runs in."""

    def __init__(self):
        self._h = lib().gsrast_context_create()
        if not self._h:
            raise MemoryError("gsrast_context_create failed")

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("gsrast: the context has been closed")
        return self._h

    def query(self, name: str) -> int:
        v = int(lib().gsrast_context_query(self.handle, name.encode()))
        if v < 0:
            raise ValueError(f"gsrast: unknown context query: {name}")
        return v

    def policy_event(self, what: str, a: int = 0, b: int = 0, c: int = 0) -> int:
        """gsrast_policy_event (include/gsrast.h): one host-side decision of the context, no device involved."""
        v = int(lib().gsrast_policy_event(self.handle, what.encode(), int(a), int(b), int(c)))
        if v < 0:
            raise ValueError(f"gsrast: unknown policy event: {what}")
        return v

    def close(self) -> None:
        h, self._h = self._h, None
        if h:
            lib().gsrast_context_destroy(h)     # (waits for the context's own streams)

    def __enter__(self):
        stack = getattr(_tls, "contexts", None)
        if stack is None:
            stack = _tls.contexts = []
        stack.append(self)
        return self

    def __exit__(self, *exc):
        _tls.contexts.pop()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass


def policy_event(what: str, a: int = 0, b: int = 0, c: int = 0) -> int:
    """gsrast_policy_event on the calling thread's current context."""
    v = int(lib().gsrast_policy_event(_current_context(), what.encode(), int(a), int(b), int(c)))
    if v < 0:
        raise ValueError(f"gsrast: unknown policy event: {what}")
    return v


def _current_context():
    """The handle of the innermost `with Context():` block of the calling thread, or None = the thread's own default context."""
    stack = getattr(_tls, "contexts", None)
    return stack[-1].handle if stack else None


def context_query(name: str) -> int:
    """gsrast_context_query on the calling thread's current context (include/gsrast.h): "last_instances", "last_runs", "redo_count",
    "bucket_skip", "last_late", "last_early_runs", "cut_pause", "cut_fallbacks", "completion_passes", "cut_margin_x4", "tau_req", ..."""
    v = int(lib().gsrast_context_query(_current_context(), name.encode()))
    if v < 0:
        raise ValueError(f"gsrast: unknown context query: {name}")
    return v


def profile_read() -> dict:
    """{kernel name: (total_ms, launches)} gathered while option 'profile' is 1."""
    L = lib()
    L.gsrast_profile_collect()
    out = {}
    for k in range(L.gsrast_profile_kernel_count()):
        ms, n = C.c_double(0), C.c_longlong(0)
        L.gsrast_profile_read(k, C.byref(ms), C.byref(n))
        out[L.gsrast_profile_kernel_name(k).decode()] = (ms.value, n.value)
    return out


def profile_reset() -> None:
    lib().gsrast_profile_reset()


def debug_export(P: int, R: int, W: int, H: int, geomBuffer, binningBuffer, imageBuffer) -> dict:
    """Copy the opaque state out in the reference's array layout (parity tests only)."""
    dev = geomBuffer.device
    T = ((W + 15) // 16) * ((H + 15) // 16)
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(
        depths=torch.zeros(P, **f32), means2D=torch.zeros((P, 2), **f32), cov3D=torch.zeros((P, 6), **f32),
        conic_opacity=torch.zeros((P, 4), **f32), rgb=torch.zeros((P, 3), **f32),
        clamped=torch.zeros((P, 3), dtype=torch.uint8, device=dev),
        tiles_touched=torch.zeros(P, dtype=torch.int32, device=dev),
        keys_sorted=torch.zeros(max(R, 1), dtype=torch.int64, device=dev)[:R],
        point_list=torch.zeros(max(R, 1), dtype=torch.int32, device=dev)[:R],
        ranges=torch.zeros((T, 2), dtype=torch.int32, device=dev),
        final_T=torch.zeros((H, W), **f32), n_contrib=torch.zeros((H, W), dtype=torch.int32, device=dev))
    # cov3D is kept by the forward only under the process-wide option "debug_state" (24 B / Gaussian nothing else reads)
    keep_cov = int(lib().gsrast_get_option(b"debug_state")) != 0
    if not keep_cov:
        del out["cov3D"]
    launch("gsrast_debug_export", dev, P, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer), out["depths"].data_ptr(),
         out["means2D"].data_ptr(), out["cov3D"].data_ptr() if keep_cov else None, out["conic_opacity"].data_ptr(),
         out["rgb"].data_ptr(), out["clamped"].data_ptr(), out["tiles_touched"].data_ptr(),
         _ptr(out["keys_sorted"]), _ptr(out["point_list"]), out["ranges"].data_ptr(),
         out["final_T"].data_ptr(), out["n_contrib"].data_ptr())
    return out
