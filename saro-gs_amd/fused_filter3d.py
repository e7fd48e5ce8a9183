"""Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024; include/gsrast.h: gsrast_filter3d_*; csrc/gsrast_filter3d.h) -- the
companion of ``antialiasing=True`` (the 2-D screen-space filter): every Gaussian's size is bounded below by the highest sampling rate at
which any training camera sees it, so zooming in or rendering above the training resolution does not erode thin structures.

    table = camera_table(train_cameras, device)                    # once: [C, 16]
    flt = compute_filter_3d(xyz, table)                            # every 100 iterations and after every densification / prune (P changed)
    scales, opacities = apply_filter_3d(scales, opacities, flt.filter_3D)      # every view, behind activate_gaussians / exp, sigmoid
    rasterizer(..., scales=scales, opacities=opacities)            # GaussianRasterizer with antialiasing=True

``compute_filter_3d`` restates upstream's ``compute_3D_filter`` (a Python loop over the cameras with about twenty [P] temporaries each) as
one sweep with the cameras in the inner loop; ``apply_filter_3d`` restates ``get_scaling_with_3D_filter`` / ``get_opacity_with_3D_filter``
with their autograd as one launch each way, in a form that does not underflow for thin Gaussians; ``bake_filter_3d`` is upstream's
``save_fused_ply`` step.  The filter is computed on the means the caller passes: for the dynamic model these are the canonical ``_xyz``;
the per-time motion residual is NOT swept.

Not supported: the raw family (``GaussianRasterizerRaw`` activates inside the rasterizer, so the filter cannot be applied behind it); the
paper's per-camera rate max f_n / d_n (upstream's code takes min d and max f separately, and so does this); per-time sweeps.
GPU tensors only; there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import math
from typing import Iterable, NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C

__all__ = ["camera_table", "camera_table_from_arrays", "compute_filter_3d", "apply_filter_3d", "bake_filter_3d", "Filter3D", "CameraTable"]

CAMERA_FLOATS = 16      # include/gsrast.h: R (9, row-major) | T (3) | focal_x | focal_y | W | H


class Filter3D(NamedTuple):
    filter_3D: torch.Tensor      # [P, 1] float32
    valid: torch.Tensor          # [P] bool: some camera sees the row


class CameraTable(torch.Tensor):
    """The [C, 16] float32 table of ``camera_table``: a tensor that remembers ``focal_max`` (the largest focal_x, as the Python float it
    was computed in), so that ``compute_filter_3d`` needs no read-back for it."""
    focal_max: Optional[float] = None


def _check(name: str, t, shape: Tuple, dev: Optional[torch.device], first: str = "") -> None:
    """`t` is a contiguous fp32 GPU tensor of `shape` (None: any extent) on `dev` (None: any GPU), or the refusal."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"fused_filter3d: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"fused_filter3d: {name} must be on a GPU (HIP) device; there is no CPU fallback")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"fused_filter3d: {name} is on {t.device}, {first} on {dev}")
    if t.dtype != torch.float32:
        raise ValueError(f"fused_filter3d: {name} must be float32 (got {t.dtype})")
    if t.dim() != len(shape) or any(s is not None and int(v) != s for v, s in zip(t.shape, shape)):
        want = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"fused_filter3d: {name} must be [{want}] (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"fused_filter3d: {name} must be contiguous")


def _field(cam, name: str):
    return cam[name] if isinstance(cam, dict) else getattr(cam, name)


def _table(R: torch.Tensor, T: torch.Tensor, fx, fy, W, H, device: torch.device) -> CameraTable:
    """R [C, 3, 3] and T [C, 3] on `device`; the four per-camera numbers as Python floats, written to the device in one copy."""
    C = int(R.shape[0])
    for name, v in (("focal_x", fx), ("focal_y", fy), ("width", W), ("height", H)):
        if len(v) != C:
            raise ValueError(f"fused_filter3d: {name} has {len(v)} entries for {C} cameras")
        if not all(math.isfinite(x) and x > 0.0 for x in v):
            raise ValueError(f"fused_filter3d: {name} must be finite and > 0 for every camera")
    if C < 1:
        raise ValueError("fused_filter3d: a camera table needs at least one camera")
    intr = torch.tensor(np.stack([np.asarray(v, np.float64) for v in (fx, fy, W, H)], axis=1), dtype=torch.float32).to(device)      # (rounded once)
    table = torch.cat([R.reshape(C, 9), T.reshape(C, 3), intr], dim=1).contiguous().as_subclass(CameraTable)
    table.focal_max = max(fx)
    return table


def _on(a, device: torch.device) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    return t.detach().to(device=device, dtype=torch.float32)


def camera_table(cameras: Iterable, device) -> CameraTable:
    """[C, 16] float32 on `device`, one row per camera: R = viewmatrix[:3, :3] row-major, T = viewmatrix[3, :3], focal_x, focal_y, W, H.
    ``viewmatrix`` is the transposed world -> view matrix a ``GaussianRasterizationSettings`` carries (p_cam = p @ R + T): exactly
    Mip-Splatting's ``camera.R`` and ``camera.T``.  `cameras`: objects or dicts (``scenes.camera``) with ``image_width``,
    ``image_height``, ``tanfovx``, ``tanfovy`` and ``viewmatrix``.  focal_x = W / (2 tanfovx) and focal_y = H / (2 tanfovy) are computed
    in Python floats and rounded once; R and T are stacked on the device with no read-back.  The result remembers ``focal_max``."""
    device = torch.device(device)
    cams = list(cameras)
    if not cams:
        raise ValueError("fused_filter3d: a camera table needs at least one camera")
    W = [float(int(_field(c, "image_width"))) for c in cams]
    H = [float(int(_field(c, "image_height"))) for c in cams]
    fx = [w / (2.0 * float(_field(c, "tanfovx"))) for c, w in zip(cams, W)]
    fy = [h / (2.0 * float(_field(c, "tanfovy"))) for c, h in zip(cams, H)]
    views = []
    for c in cams:
        v = _on(_field(c, "viewmatrix"), device)
        if v.numel() != 16:
            raise ValueError("fused_filter3d: a camera's viewmatrix must hold 16 floats")
        views.append(v.reshape(4, 4))
    V = torch.stack(views)
    return _table(V[:, :3, :3], V[:, 3, :3], fx, fy, W, H, device)


def _floats(v, C: int) -> list:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    a = np.asarray(v, np.float64).reshape(-1)
    return [float(x) for x in (np.repeat(a, C) if a.size == 1 and C != 1 else a)]


def camera_table_from_arrays(R, T, focal_x, focal_y, width, height, device=None) -> CameraTable:
    """The same table from Mip-Splatting-style cameras: R [C, 3, 3] (``camera.R``), T [C, 3] (``camera.T``), and per camera (a sequence,
    or one number for all) ``focal_x``, ``focal_y``, ``image_width``, ``image_height``.  `device`: where the table lives (default: R's,
    if R is a tensor)."""
    if device is None:
        if not isinstance(R, torch.Tensor):
            raise ValueError("fused_filter3d: camera_table_from_arrays needs device= when R is not a tensor")
        device = R.device
    device = torch.device(device)
    R, T = _on(R, device), _on(T, device)
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3):
        raise ValueError(f"fused_filter3d: R must be [C, 3, 3] (got {tuple(R.shape)})")
    C = int(R.shape[0])
    if tuple(T.shape) != (C, 3):
        raise ValueError(f"fused_filter3d: T must be [{C}, 3] (got {tuple(T.shape)})")
    return _table(R, T, _floats(focal_x, C), _floats(focal_y, C), _floats(width, C), _floats(height, C), device)


def compute_filter_3d(means3D: torch.Tensor, table: torch.Tensor, *, near: float = 0.2, margin: float = 0.15, variance: float = 0.2,
                      focal_max: Optional[float] = None) -> Filter3D:
    """``Filter3D(filter_3D [P, 1] float32, valid [P] bool)`` of the means under the cameras of `table` (``camera_table``).  Per row and
    camera, in fp32 with every operation rounded:
        xc = ((x R00 + y R10) + z R20) + T0, yc, zc likewise;  zz = max(zc, 0.001);  px = (xc / zz) focal_x + W / 2,  py likewise
        seen = zc > near and zz < inf and -(margin W) <= px <= W + margin W and -(margin H) <= py <= H + margin H
    ``dist`` = the smallest zz over the cameras that see the row, ``valid`` = some camera does, ``dmax`` = the largest dist of a valid
    row, and  filter_3D = (dist if valid else dmax) * k,  k = float32(sqrt(variance) / focal_max)  formed in fp64.  `focal_max`: the
    largest focal_x; taken from a table ``camera_table`` built, to be given for any other tensor.  A NaN or Inf row is never valid and
    gets dmax.  Upstream's ``compute_3D_filter`` at the defaults, with three stated deviations: one multiplication by k where it divides
    and multiplies (<= 1 ulp); the screen bounds W + margin W where it writes the literal W * 1.15; when NO row is valid every filter_3D
    is +0.0 (upstream raises on the max() of an empty tensor).
    The filter is computed on the means passed: for the dynamic model the canonical ``_xyz``; the per-time motion residual is not swept.
    Nothing is differentiable (inputs that require grad are fine); no host synchronisation, no read-back.  Two launches; the maximum is
    an integer max on the bits of positive floats, one writer per element: bit-identical from run to run and on every rank.
    Raises before any launch: a CPU, non-float32, non-contiguous, wrong-shape or other-device tensor, a missing ``focal_max``, a
    non-finite or non-positive ``near`` / ``variance`` / ``focal_max``, a non-finite or negative ``margin``."""
    _check("means3D", means3D, (None, 3), None)
    P, dev = int(means3D.shape[0]), means3D.device
    _check("table", table, (None, CAMERA_FLOATS), dev, "means3D")
    C = int(table.shape[0])
    if C < 1:
        raise ValueError("fused_filter3d: table must hold at least one camera")
    if focal_max is None:
        focal_max = getattr(table, "focal_max", None)
        if focal_max is None:
            raise ValueError("fused_filter3d: focal_max= is needed for a table that camera_table did not build (there is no read-back)")
    near, margin, variance, focal_max = float(near), float(margin), float(variance), float(focal_max)
    for name, v, low in (("near", near, False), ("variance", variance, False), ("focal_max", focal_max, False), ("margin", margin, True)):
        if not math.isfinite(v) or v < 0.0 or (v == 0.0 and not low):
            raise ValueError(f"fused_filter3d: {name} must be finite and {'>= 0' if low else '> 0'} (got {v})")
    with torch.no_grad():
        filt = torch.empty((P, 1), dtype=torch.float32, device=dev)
        valid = torch.empty((P,), dtype=torch.bool, device=dev)
        if P > 0:      # (an empty tensor has no pointer to give; no row, no launch)
            scratch = torch.empty((_C.scratch_bytes("gsrast_filter3d_scratch_bytes", P, C),), dtype=torch.uint8, device=dev)
            _C.launch("gsrast_filter3d_compute", dev, P, C, means3D.detach().data_ptr(), table.detach().data_ptr(), near, margin, variance, focal_max,
                      filt.data_ptr(), valid.data_ptr(), scratch.data_ptr())
    return Filter3D(filt, valid)


def _upstream(g: torch.Tensor, dev: torch.device) -> torch.Tensor:
    if g.device != dev:
        raise RuntimeError(f"fused_filter3d: the upstream gradient is on {g.device}, the inputs on {dev}")
    return g.contiguous().float()


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacities, filter_3D):
        s, o, f = scales.detach(), opacities.detach(), filter_3D.detach()
        P, dev = int(s.shape[0]), s.device
        s_f, o_f = torch.empty_like(s), torch.empty_like(o)
        if P > 0:
            _C.launch("gsrast_filter3d_apply_forward", dev, P, s.data_ptr(), o.data_ptr(), f.data_ptr(), s_f.data_ptr(), o_f.data_ptr())
        ctx.save_for_backward(s, o, f)      # (the inputs alone: the backward recomputes s_f, r and coef)
        ctx.set_materialize_grads(False)
        return s_f, o_f

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, g_s, g_o):
        s, o, f = ctx.saved_tensors
        need_s, need_o = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_s is None and g_o is None) or not (need_s or need_o):
            return None, None, None
        P, dev = int(s.shape[0]), s.device
        g_s = None if g_s is None else _upstream(g_s, dev)
        g_o = None if g_o is None else _upstream(g_o, dev)
        d_s = torch.empty_like(s) if need_s else None
        d_o = torch.empty_like(o) if need_o else None
        if P > 0:
            _C.launch("gsrast_filter3d_apply_backward", dev, P, s.data_ptr(), o.data_ptr(), f.data_ptr(), _C._ptr(g_s), _C._ptr(g_o),
                      None if d_s is None else d_s.data_ptr(), None if d_o is None else d_o.data_ptr())
        return d_s, d_o, None


def apply_filter_3d(scales: torch.Tensor, opacities: torch.Tensor, filter_3D: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(scales_f [P, 3], opacities_f [P, 1])`` from ACTIVATED scales and opacities -- behind ``activate_gaussians(...)`` for the dynamic
    stage, behind plain ``exp`` / ``sigmoid`` for the static one -- to hand to ``GaussianRasterizer`` as ``scales=`` / ``opacities=``:
        s_f,k = sqrt(s_k^2 + f^2);  r_k = s_k / s_f,k (1 where s_f,k == 0);  o_f = o (r_0 r_1) r_2
    which equals upstream's  o sqrt(prod s^2 / prod (s^2 + f^2))  without the products of squares that underflow in fp32 for thin
    Gaussians.  Gradients go to ``scales`` and ``opacities``, each only when it requires one; ``filter_3D`` [P, 1] (or [P]) gets none
    (upstream keeps it as a buffer); an unused output counts as zero upstream.  One launch each way, one lane per row; the backward
    recomputes everything from the three inputs.  Works under ``torch.no_grad()``; a double backward raises.  Contiguous fp32 tensors on
    one GPU; anything else raises before a launch.
    Not for the raw family: ``GaussianRasterizerRaw`` activates inside the rasterizer, so the filter cannot be applied behind it."""
    _check("scales", scales, (None, 3), None)
    P, dev = int(scales.shape[0]), scales.device
    _check("opacities", opacities, (P, 1), dev, "scales")
    if isinstance(filter_3D, torch.Tensor) and filter_3D.dim() == 1:
        _check("filter_3D", filter_3D, (P,), dev, "scales")
    else:
        _check("filter_3D", filter_3D, (P, 1), dev, "scales")
    return _ApplyFilter3D.apply(scales, opacities, filter_3D)


@torch.no_grad()
def bake_filter_3d(scaling_raw: torch.Tensor, opacity_raw: torch.Tensor, filter_3D: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Raw ``(log s_f, logit o_f)`` of the raw leaves ``scaling_raw`` [P, 3] (log scale) and ``opacity_raw`` [P, 1] (logit): upstream's
    ``save_fused_ply`` step, so that an exported model renders the filtered Gaussians in a viewer that knows no filter (plain ``exp`` /
    ``sigmoid``).  No kernel of its own: the fused forward between torch's activations and their inverses."""
    s_f, o_f = apply_filter_3d(torch.exp(scaling_raw.detach()), torch.sigmoid(opacity_raw.detach()), filter_3D)
    return torch.log(s_f), torch.log(o_f / (1.0 - o_f))
