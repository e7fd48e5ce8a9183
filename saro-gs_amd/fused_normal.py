"""Normal consistency between the render and the loss (include/gsrast.h: gsrast_gaussian_normals_*, gsrast_depth_normal_*,
gsrast_normal_loss_*; csrc/gsrast_normal.h): the geometry regulariser of 2DGS, gsplat's 2DGS trainer, GOF, RaDe-GS and PGSR -- the
alpha-blended Gaussian normals should agree with the normals of the rendered depth surface.

    n_g = gaussian_normals(means3D, scales, rotations, raster_settings=rs)                       # [P, 3], view space, facing the camera
    color, radii, depth, acc_depth, alpha, normal_map = rasterizer(..., return_aux=True, features=n_g)
    loss = loss + lam * normal_consistency_loss(normal_map, acc_depth / alpha.clamp_min(1e-6), raster_settings=rs, weight=alpha.detach())

``depth_to_normal`` is the middle piece on its own: the [3, H, W] normals of a depth map (gsplat's / 2DGS's central-difference
``depth_to_normal`` in view space).  The fused loss never writes those normals to memory: one launch and a small reduction forward, one
launch backward, where the torch composition is about twenty full-image passes and autograd's copies.  Every backward recomputes the forward
from its inputs; one writer per element, no atomics: values and gradients are bit-identical from run to run.  fp32 tensors in and out (the
kernels evaluate in fp64 and round once).  GPU tensors only; there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C

__all__ = ["gaussian_normals", "depth_to_normal", "normal_consistency_loss"]

MAX_SIDE = 32768      # include/gsrast.h: the limit of W and H


def _check(name: str, t, shape: Tuple, dev: Optional[torch.device], first: str = "") -> None:
    """`t` is a contiguous fp32 GPU tensor of `shape` (None: any extent) on `dev` (None: any GPU), or the refusal."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"fused_normal: {name} must be a tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"fused_normal: {name} must be on a GPU (HIP) device; there is no CPU fallback")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"fused_normal: {name} is on {t.device}, {first} on {dev}")
    if t.dtype != torch.float32:
        raise ValueError(f"fused_normal: {name} must be float32 (got {t.dtype})")
    if t.dim() != len(shape) or any(s is not None and int(v) != s for v, s in zip(t.shape, shape)):
        want = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"fused_normal: {name} must be [{want}] (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"fused_normal: {name} must be contiguous")


def _image(rs) -> Tuple[int, int, float, float]:
    """(W, H, tanfovx, tanfovy) of the settings, or the refusal."""
    W, H, tx, ty = int(rs.image_width), int(rs.image_height), float(rs.tanfovx), float(rs.tanfovy)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"fused_normal: raster_settings needs an image of 1 to {MAX_SIDE} pixels on a side (got {W} x {H})")
    if not (0.0 < tx < float("inf") and 0.0 < ty < float("inf")):
        raise ValueError(f"fused_normal: raster_settings needs finite tanfovx, tanfovy > 0 (got {tx}, {ty})")
    return W, H, tx, ty


def _upstream(g: torch.Tensor, dev: torch.device) -> torch.Tensor:
    if g.device != dev:
        raise RuntimeError(f"fused_normal: the upstream gradient is on {g.device}, the inputs on {dev}")
    return g.contiguous().float()


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, view):
        m, s, q = means3D.detach(), scales.detach(), rotations.detach()
        P, dev = int(m.shape[0]), m.device
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
        if P > 0:      # (an empty tensor has no pointer to give; no row, no launch)
            _C.launch("gsrast_gaussian_normals_forward", dev, P, m.data_ptr(), s.data_ptr(), q.data_ptr(), view.data_ptr(), out.data_ptr())
        ctx.save_for_backward(m, s, q, view)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, g):
        m, s, q, view = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[2]:
            return None, None, None, None
        P, dev = int(m.shape[0]), m.device
        g = _upstream(g, dev)
        d_q = torch.empty_like(q)
        if P > 0:
            _C.launch("gsrast_gaussian_normals_backward", dev, P, m.data_ptr(), s.data_ptr(), q.data_ptr(), view.data_ptr(), g.data_ptr(), d_q.data_ptr())
        return None, None, d_q, None


def gaussian_normals(means3D: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, raster_settings) -> torch.Tensor:
    """[P, 3]: the unit normal of each Gaussian in VIEW space, facing the camera -- what to hand to a render as ``features=``.
    k = argmin(scales[i]) (a tie: the lowest index); the normal is column k of the rotation matrix of rotations[i] / |rotations[i]|
    (q = (w, x, y, z): the axis whose variance in the render's covariance is the smallest), rotated by ``raster_settings.viewmatrix`` and
    negated where it points away from the camera (n . p_view > 0; an exact 0 is left).  |q| = 0 or a non-finite q gives a zero normal and a
    zero gradient.  Gradients go to ``rotations`` only: the argmin (scales) and the sign (means3D) are piecewise constant.
    The camera is NOT differentiated: viewmatrix may require grad, the call works and it gets none from here.
    One launch each way; P = 0 launches nothing; works under ``torch.no_grad()``; a double backward raises.
    Raises before any launch: a CPU, non-float32, non-contiguous, wrong-shape or other-device tensor (RuntimeError for the device, ValueError
    else)."""
    _check("means3D", means3D, (None, 3), None)
    P, dev = int(means3D.shape[0]), means3D.device
    _check("scales", scales, (P, 3), dev, "means3D")
    _check("rotations", rotations, (P, 4), dev, "means3D")
    view = raster_settings.viewmatrix
    if not isinstance(view, torch.Tensor) or view.numel() != 16:
        raise ValueError("fused_normal: raster_settings.viewmatrix must be a tensor of 16 floats")
    if view.device != dev:
        raise RuntimeError(f"fused_normal: raster_settings.viewmatrix is on {view.device}, means3D on {dev}")
    if view.dtype != torch.float32:
        raise ValueError(f"fused_normal: raster_settings.viewmatrix must be float32 (got {view.dtype})")
    return _GaussianNormals.apply(means3D, scales, rotations, view.detach().contiguous())


def _depth_plane(depth, W: int, H: int, dev: Optional[torch.device], first: str = "") -> None:
    if isinstance(depth, torch.Tensor) and depth.dim() == 3:
        _check("depth", depth, (1, H, W), dev, first)
    else:
        _check("depth", depth, (H, W), dev, first)


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, W, H, tx, ty):
        d = depth.detach()
        out = torch.empty((3, H, W), dtype=torch.float32, device=d.device)
        _C.launch("gsrast_depth_normal_forward", d.device, W, H, tx, ty, d.data_ptr(), out.data_ptr())
        ctx.save_for_backward(d)
        ctx.args = (W, H, tx, ty)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = _upstream(g, d.device)
        d_depth = torch.empty_like(d)      # (the shape that was given: [H, W] or [1, H, W])
        _C.launch("gsrast_depth_normal_backward", d.device, *ctx.args, d.data_ptr(), g.data_ptr(), d_depth.data_ptr())
        return d_depth, None, None, None, None


def depth_to_normal(depth: torch.Tensor, raster_settings) -> torch.Tensor:
    """[3, H, W]: the view-space normals of the surface ``depth`` ([H, W] or [1, H, W]; view-space z: the render's ``depth``, or
    ``acc_depth / alpha``), by central differences as gsplat's and 2DGS's ``depth_to_normal``:
        u_x = ((2x + 1) / W - 1) tanfovx,  v_y = ((2y + 1) / H - 1) tanfovy,  P(x, y) = d(x, y) (u_x, v_y, 1)
        a = P(x, y+1) - P(x, y-1),  b = P(x+1, y) - P(x-1, y),  n = (a x b) / |a x b|
    A fronto-parallel plane gives (0, 0, -1): towards the camera.  The normal is 0, with a zero gradient, on the one-pixel border (gsplat's
    zero padding), where any of the four neighbours' depths is not > 0 (an uncovered pixel, a NaN), and where |a x b|^2 < 1e-24.  The last
    two are deviations from gsplat, which divides by max(|a x b|, 1e-12) and has no coverage rule.
    Of ``raster_settings`` the image size and tanfovx / tanfovy are read.  The gradient comes back in the shape ``depth`` was given in.
    One launch each way; works under ``torch.no_grad()``; a double backward raises.  Contiguous fp32 tensors on one GPU; anything else
    raises before a launch."""
    W, H, tx, ty = _image(raster_settings)
    _depth_plane(depth, W, H, None)
    return _DepthToNormal.apply(depth, W, H, tx, ty)


class _NormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal_map, depth, weight, W, H, tx, ty):
        N, d = normal_map.detach(), depth.detach()
        dev = N.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty((_C.scratch_bytes("gsrast_normal_loss_scratch_bytes", W, H),), dtype=torch.uint8, device=dev)
        _C.launch("gsrast_normal_loss_forward", dev, W, H, tx, ty, N.data_ptr(), d.data_ptr(), _C._ptr(weight), loss.data_ptr(), scratch.data_ptr())
        ctx.save_for_backward(N, d, weight)
        ctx.args = (W, H, tx, ty)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        N, d, weight = ctx.saved_tensors
        need_N, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_N or need_d):
            return (None,) * 7
        dev = N.device
        g = _upstream(g, dev).reshape(1)
        d_N = torch.empty_like(N) if need_N else None
        d_d = torch.empty_like(d) if need_d else None
        _C.launch("gsrast_normal_loss_backward", dev, *ctx.args, N.data_ptr(), d.data_ptr(), _C._ptr(weight), g.data_ptr(), _C._ptr(d_N), _C._ptr(d_d))
        return d_N, d_d, None, None, None, None, None


def normal_consistency_loss(normal_map: torch.Tensor, depth: torch.Tensor, raster_settings, *, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scalar  L = (1 / (H W)) sum_p (1 - w_p <N_p, n_p>)  with n = ``depth_to_normal(depth)`` (never written to memory), N =
    ``normal_map`` [3, H, W] used as given (not normalised: 2DGS's ``rend_normal``, e.g. the ``features=gaussian_normals(...)`` map of a
    render) and w = ``weight`` [H, W] or [1, H, W] (default 1; e.g. ``alpha.detach()``), which gets no gradient even if it requires one.
    ``depth`` is [H, W] or [1, H, W].  A pixel without a normal (``depth_to_normal``'s rules) counts 1 and has zero gradients.
    Gradients go to ``normal_map`` and to ``depth``, each only when it requires one.  Forward: one launch and a fixed-order fp64 sum of its
    per-workgroup partials; backward: one launch that recomputes everything from the inputs.  The value and both gradients are
    bit-identical from run to run.  Works under ``torch.no_grad()``; a double backward raises.  Contiguous fp32 tensors on one GPU; anything
    else raises before a launch."""
    W, H, tx, ty = _image(raster_settings)
    _check("normal_map", normal_map, (3, H, W), None)
    dev = normal_map.device
    _depth_plane(depth, W, H, dev, "normal_map")
    if weight is not None:
        if isinstance(weight, torch.Tensor) and weight.dim() == 3:
            _check("weight", weight, (1, H, W), dev, "normal_map")
        else:
            _check("weight", weight, (H, W), dev, "normal_map")
        weight = weight.detach()
    return _NormalLoss.apply(normal_map, depth, weight, W, H, tx, ty)
