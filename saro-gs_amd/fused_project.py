"""The renderer's per-Gaussian projection as a differentiable call of its own (include/gsrast.h: gsrast_project_forward / _backward,
csrc/gsrast_project.h; gsplat's ``fully_fused_projection``).

A render computes, for every Gaussian, the pixel centre, the view-space depth, the dilated conic, the integer radius and (with
``antialiasing``) the opacity compensation, and keeps them inside its geometry state.  ``project_gaussians`` returns them:

    p = project_gaussians(means3D, scales, rotations, raster_settings=settings)      # the settings a render takes
    p.means2D [P,2] pixels   p.depths [P]   p.conics [P,3] = (c, -b, a) / det   p.radii [P] int32   p.compensation [P] or None

with the renderer's own expressions and its own culling: on a row with ``radii > 0`` the values are bit-equal to what a render of the same
inputs holds, ``radii`` equals the render's on every row, and a culled row (behind the near plane, a degenerate covariance, no tile
touched, a NaN mean) reads +0.0 / radius 0.  Gradients follow the render backward's conventions (frustum clamp, the conic's
det^2 / (det^2 + 1e-7), dL/dscales as of scale_modifier * scales, no compensation gradient on its floor), so the gradients of a render and
of a projection of the same leaves add consistently.  One launch forward, one backward that recomputes the forward from the inputs.

What it is for: 2-D supervision on projected centres (point tracks; optical flow -- ``screen_flow`` of two projections handed to
``GaussianRasterizer.forward(..., features=flow)``; depth-ordering terms), screen-size rules for pruning and LOD, statistics on projected
quantities.  Callers that hold raw leaves activate them first (fused_epilogue.activate_gaussians).  GPU fp32 tensors only; there is no
CPU / PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C

__all__ = ["Projection", "project_gaussians", "screen_flow"]


class Projection(NamedTuple):
    means2D: torch.Tensor                   # [P,2] pixel centres
    depths: torch.Tensor                    # [P] view-space z
    conics: torch.Tensor                    # [P,3] (c, -b, a) / det of the dilated 2-D covariance
    radii: torch.Tensor                     # [P] int32, 0 = culled; not differentiable
    compensation: Optional[torch.Tensor]    # [P] with antialiasing, else None


def _check_layout(name: str, t, width: int, P: Optional[int]) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"fused_project: {name} must be a tensor (got {type(t).__name__})")
    if t.dtype != torch.float32:
        raise ValueError(f"fused_project: {name} must be float32 (got {t.dtype})")
    if t.dim() != 2 or int(t.shape[1]) != width or (P is not None and int(t.shape[0]) != P):
        raise ValueError(f"fused_project: {name} must be [{'P' if P is None else P}, {width}] (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"fused_project: {name} must be contiguous")


def _check_device(name: str, t: torch.Tensor, dev: Optional[torch.device]) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"fused_project: {name} must be on a GPU (HIP) device; there is no CPU fallback")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"fused_project: {name} is on {t.device}, means3D on {dev}")


def _camera(name: str, t, dev: torch.device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.numel() != 16:
        raise ValueError(f"fused_project: raster_settings.{name} must be a tensor of 16 floats")
    if t.device != dev:
        raise RuntimeError(f"fused_project: raster_settings.{name} is on {t.device}, means3D on {dev}")
    if t.dtype != torch.float32:
        raise ValueError(f"fused_project: raster_settings.{name} must be float32 (got {t.dtype})")
    return t.detach().contiguous()


def _descriptor(P: int, rs, view, proj, means3D, scales, rotations, cov3D, antialiasing: bool) -> _C.ProjectStruct:
    d = _C.ProjectStruct()
    d.P, d.width, d.height = P, int(rs.image_width), int(rs.image_height)
    d.tanfovx, d.tanfovy, d.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier)
    d.viewmatrix, d.projmatrix = view.data_ptr(), proj.data_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    d.means3D, d.scales, d.rotations, d.cov3D_precomp = ptr(means3D), ptr(scales), ptr(rotations), ptr(cov3D)
    d.flags = _C.PROJECT_ANTIALIAS if antialiasing else 0
    return d


class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, cov3D, raster_settings, antialiasing):
        rs, dev, P = raster_settings, means3D.device, int(means3D.shape[0])
        view, proj = _camera("viewmatrix", rs.viewmatrix, dev), _camera("projmatrix", rs.projmatrix, dev)
        inputs = [None if t is None else t.detach() for t in (means3D, scales, rotations, cov3D)]
        f32 = dict(dtype=torch.float32, device=dev)
        means2D, depths, conics = torch.empty((P, 2), **f32), torch.empty((P,), **f32), torch.empty((P, 3), **f32)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        comp = torch.empty((P,), **f32) if antialiasing else None
        d = _descriptor(P, rs, view, proj, *inputs, antialiasing)
        d.means2D, d.depths, d.conics, d.radii, d.compensation = [None if t is None else t.data_ptr() for t in (means2D, depths, conics, radii, comp)]
        if P > 0:      # (an empty tensor has no pointer to give; no row, no launch)
            _C.launch("gsrast_project_forward", dev, C.addressof(d))
        ctx.save_for_backward(view, proj, *[t for t in inputs if t is not None])
        ctx.args = (rs, bool(antialiasing), cov3D is not None)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)      # an output nothing flows through counts as zero upstream: a NULL pointer, no zero tensor
        return means2D, depths, conics, radii, comp

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, g_means2D, g_depths, g_conics, _g_radii, g_comp):
        rs, antialiasing, have_cov = ctx.args
        view, proj, means3D, *rest = ctx.saved_tensors
        scales, rotations, cov3D = (None, None, rest[0]) if have_cov else (rest[0], rest[1], None)
        P, dev = int(means3D.shape[0]), means3D.device
        ups = []
        for g in (g_means2D, g_depths, g_conics, g_comp):
            if g is not None:
                if g.device != dev:
                    raise RuntimeError(f"fused_project: an upstream gradient is on {g.device}, the inputs on {dev}")
                g = g.contiguous().float()
            ups.append(g)
        need = ctx.needs_input_grad[:4]
        out = [torch.empty_like(t) if n and t is not None else None for n, t in zip(need, (means3D, scales, rotations, cov3D))]
        if P > 0 and any(o is not None for o in out):
            d = _descriptor(P, rs, view, proj, means3D, scales, rotations, cov3D, antialiasing)
            d.dL_dmeans2D, d.dL_ddepths, d.dL_dconics, d.dL_dcompensation = [None if g is None else g.data_ptr() for g in ups]
            d.dL_dmeans3D, d.dL_dscales, d.dL_drotations, d.dL_dcov3D = [None if o is None else o.data_ptr() for o in out]
            _C.launch("gsrast_project_backward", dev, C.addressof(d))
        return (*out, None, None)


def project_gaussians(means3D: torch.Tensor, scales: Optional[torch.Tensor] = None, rotations: Optional[torch.Tensor] = None,
                      cov3D_precomp: Optional[torch.Tensor] = None, *, raster_settings, antialiasing: bool = False) -> Projection:
    """The projection stage of ``GaussianRasterizer(raster_settings)`` for means3D [P,3] and (scales [P,3], rotations [P,4]) or cov3D_precomp
    [P,6] (xx xy xz yy yz zz): ``Projection(means2D, depths, conics, radii, compensation)``, ``compensation`` None without ``antialiasing``.
    Of ``raster_settings`` (a GaussianRasterizationSettings) the image size, tanfovx / tanfovy, scale_modifier, viewmatrix and projmatrix
    are read.  Gradients go to means3D, scales, rotations and cov3D_precomp, each only when it requires one; an output that takes no part in
    the backward pass counts as zero upstream; ``radii`` is non-differentiable; a double backward raises.  Works under ``torch.no_grad()``.
    The camera is NOT differentiated: viewmatrix / projmatrix may require grad, the call works and they get none from here.
    Raises before any launch: a CPU, non-float32, non-contiguous, wrong-shape or other-device tensor (RuntimeError for the device, ValueError
    else), and ``Exception`` unless exactly one of (scales, rotations) / cov3D_precomp is given, as GaussianRasterizer.forward."""
    have_sr = scales is not None or rotations is not None
    full_sr = scales is not None and rotations is not None
    have_cov = cov3D_precomp is not None
    if (not full_sr and not have_cov) or (have_sr and have_cov):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    _check_layout("means3D", means3D, 3, None)
    P = int(means3D.shape[0])
    given = (("cov3D_precomp", cov3D_precomp, 6),) if have_cov else (("scales", scales, 3), ("rotations", rotations, 4))
    for name, t, width in given:
        _check_layout(name, t, width, P)
    _check_device("means3D", means3D, None)
    for name, t, _ in given:
        _check_device(name, t, means3D.device)
    rs = raster_settings
    if int(rs.image_width) <= 0 or int(rs.image_height) <= 0 or not float(rs.tanfovx) > 0.0 or not float(rs.tanfovy) > 0.0:
        raise ValueError("fused_project: raster_settings needs a positive image size and positive tanfovx / tanfovy")
    return Projection(*_ProjectGaussians.apply(means3D, scales, rotations, cov3D_precomp, rs, bool(antialiasing)))


def screen_flow(p0: Projection, p1: Projection) -> Tuple[torch.Tensor, torch.Tensor]:
    """(flow [P,2], valid [P] bool) of two projections of the same Gaussians (two timestamps, two cameras): flow = p1.means2D - p0.means2D in
    pixels where both radii > 0, +0.0 elsewhere.  Differentiable through both projections.  ``flow`` is what a caller hands to
    ``GaussianRasterizer.forward(..., features=flow)`` to render an optical-flow map with the colour's own blend weights."""
    if p0.means2D.shape != p1.means2D.shape:
        raise ValueError(f"fused_project: the projections have {int(p0.means2D.shape[0])} and {int(p1.means2D.shape[0])} rows")
    valid = (p0.radii > 0) & (p1.radii > 0)
    d = p1.means2D - p0.means2D
    return torch.where(valid[:, None], d, torch.zeros_like(d)), valid
