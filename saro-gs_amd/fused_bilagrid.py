"""Bilateral-grid colour correction between the render and the loss (include/gsrast.h: gsrast_bilagrid_*, csrc/gsrast_bilagrid.h).

Per-camera appearance compensation as gsplat ships it (lib_bilagrid's `slice` and `total_variation_loss`; upstream 3DGS's "exposure" is
the 1 x 1 x 1 grid): a low-resolution grid [12, L, GH, GW] of 3 x 4 colour matrices per camera, indexed by pixel position and luminance.
Per pixel of `image` [3, H, W], the crop at (x0, y0) of a full_W x full_H frame:
    x = (x0 + px + 0.5) / full_W,  y = (y0 + py + 0.5) / full_H,  gray = 0.299 r + 0.587 g + 0.114 b
    A = F.grid_sample(grid[None], 2 (x, y, gray) - 1, mode="bilinear", padding_mode="border", align_corners=True)   [12]
    out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3]
One launch forward; the backward recomputes everything from its inputs: one launch for dL/dimage, a gather of one or two launches for
dL/dgrid (no floating-point atomics: bit-identical from run to run).  Which camera owns which grid, the TV weight (gsplat: 10) and the
learning rate stay the caller's.  GPU fp32 tensors only; there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C

MAX_GRID, MAX_GUIDANCE, MAX_FRAME = 64, 16, 32768      # include/gsrast.h: the limits of GW / GH, of L and of a frame side


def _check(name: str, x: torch.Tensor, dev: Optional[torch.device] = None) -> None:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"fused_bilagrid: {name} must be a tensor (got {type(x).__name__})")
    if not x.is_cuda:
        raise RuntimeError(f"fused_bilagrid: {name} must be on a GPU (HIP) device; there is no CPU fallback")
    if dev is not None and x.device != dev:
        raise RuntimeError(f"fused_bilagrid: {name} is on {x.device}, the grid on {dev}")
    if x.dtype != torch.float32:
        raise ValueError(f"fused_bilagrid: {name} must be float32 (got {x.dtype})")
    if not x.is_contiguous():
        raise ValueError(f"fused_bilagrid: {name} must be contiguous")


def _grid_dims(shape: Sequence[int], lead: int) -> Tuple[int, int, int]:
    """(GW, GH, L) of a [..., 12, L, GH, GW] shape with `lead` leading axes, or the refusal."""
    if len(shape) != lead + 4 or int(shape[lead]) != 12:
        raise ValueError(f"fused_bilagrid: the grid must be {'[N, ' if lead else '['}12, L, GH, GW] (got {tuple(shape)})")
    L, GH, GW = (int(v) for v in shape[lead + 1:])
    if not (1 <= GW <= MAX_GRID and 1 <= GH <= MAX_GRID):
        raise ValueError(f"fused_bilagrid: GW and GH must be in [1, {MAX_GRID}] (got {GW}, {GH})")
    if not 1 <= L <= MAX_GUIDANCE:
        raise ValueError(f"fused_bilagrid: L must be in [1, {MAX_GUIDANCE}] (got {L})")
    return GW, GH, L


def _descriptor(grid: torch.Tensor, image: torch.Tensor, window, splits: int = 0) -> "_C.BilagridStruct":
    """The checks of bilagrid_apply, before any launch; -> the call's descriptor."""
    _check("grid", grid)
    _check("image", image, grid.device)
    GW, GH, L = _grid_dims(grid.shape, 0)
    if image.dim() != 3 or int(image.shape[0]) != 3 or image.numel() == 0:
        raise ValueError(f"fused_bilagrid: image must be [3, H, W] with H, W >= 1 (got {tuple(image.shape)})")
    H, W = int(image.shape[1]), int(image.shape[2])
    x0, y0, full_W, full_H = (0, 0, W, H) if window is None else (int(v) for v in window)
    if not (1 <= full_W <= MAX_FRAME and 1 <= full_H <= MAX_FRAME):
        raise ValueError(f"fused_bilagrid: the frame must be at most {MAX_FRAME} on a side (got {full_W} x {full_H})")
    if x0 < 0 or y0 < 0 or x0 + W > full_W or y0 + H > full_H:
        raise ValueError(f"fused_bilagrid: the window ({x0}, {y0}) + {W} x {H} must lie inside the {full_W} x {full_H} frame")
    if splits < 0:
        raise ValueError(f"fused_bilagrid: splits must be >= 0 (got {splits})")
    return _C.BilagridStruct(GW, GH, L, W, H, x0, y0, full_W, full_H, int(splits))


def _forward(desc, grid: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(image)
    _C.launch("gsrast_bilagrid_forward", image.device, desc, grid.data_ptr(), image.data_ptr(), out.data_ptr())
    return out


def _backward(desc, grid: torch.Tensor, image: torch.Tensor, d_out: torch.Tensor, need_grid: bool, need_image: bool):
    """(dL/dgrid or None, dL/dimage or None); at least one is wanted."""
    dev = image.device
    d_grid = torch.empty_like(grid) if need_grid else None
    d_image = torch.empty_like(image) if need_image else None
    scratch = None
    if need_grid:
        scratch = torch.empty((_C.scratch_bytes("gsrast_bilagrid_scratch_bytes", desc),), dtype=torch.uint8, device=dev)
    _C.launch("gsrast_bilagrid_backward", dev, desc, grid.data_ptr(), image.data_ptr(), d_out.data_ptr(), _C._ptr(d_image), _C._ptr(d_grid), _C._ptr(scratch))
    return d_grid, d_image


class _BilagridApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, image, desc):
        g, im = grid.detach(), image.detach()
        ctx.save_for_backward(g, im)
        ctx.desc = desc
        return _forward(desc, g, im)

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, d_out):
        g, im = ctx.saved_tensors
        need_grid, need_image = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_grid or need_image):
            return None, None, None
        if d_out.device != im.device:
            raise RuntimeError(f"fused_bilagrid: the upstream gradient is on {d_out.device}, the image on {im.device}")
        d_grid, d_image = _backward(ctx.desc, g, im, d_out.contiguous().float(), need_grid, need_image)
        return d_grid, d_image, None


def bilagrid_apply(grid: torch.Tensor, image: torch.Tensor, *, window: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
    """out [3, H, W]: `image` [3, H, W] mapped through `grid` [12, L, GH, GW] (one camera's grid).  window = (x0, y0, full_W, full_H): the
    image is the crop at (x0, y0) of a full_W x full_H frame; default the whole frame.  Gradients go to `grid` and `image`, each only when
    it requires one (to the image also through the luminance that indexes the grid).  Works under torch.no_grad().  Contiguous fp32
    tensors on one GPU; anything else raises before a launch."""
    return _BilagridApply.apply(grid, image, _descriptor(grid, image, window))


def _tv_call(grids: torch.Tensor, want_value: bool, upstream: Optional[torch.Tensor]):
    N, (GW, GH, L) = int(grids.shape[0]), _grid_dims(grids.shape, 1)
    dev = grids.device
    value = torch.empty((), dtype=torch.float32, device=dev) if want_value else None
    d_grids = None if want_value else torch.empty_like(grids)
    _C.launch("gsrast_bilagrid_tv", dev, N, GW, GH, L, grids.data_ptr(), value.data_ptr() if want_value else None,
            upstream.data_ptr() if upstream is not None else None, _C._ptr(d_grids))
    return value if want_value else d_grids


class _BilagridTV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        g = grids.detach()
        ctx.save_for_backward(g)
        return _tv_call(g, True, None)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_value):
        (g,) = ctx.saved_tensors
        if d_value.device != g.device:
            raise RuntimeError(f"fused_bilagrid: the upstream gradient is on {d_value.device}, the grids on {g.device}")
        return _tv_call(g, False, d_value.contiguous().float())


def tv(grids: torch.Tensor) -> torch.Tensor:
    """The total variation of grids [N, 12, L, GH, GW] as a differentiable scalar on the device: the sum over the three grid axes of the
    mean, over every element pair along that axis, of the squared forward difference (an axis of size 1 contributes 0)."""
    _check("grids", grids)
    _grid_dims(grids.shape, 1)
    if int(grids.shape[0]) < 1:
        raise ValueError("fused_bilagrid: tv needs at least one grid")
    return _BilagridTV.apply(grids)


def identity_grids(num: int, grid_x: int = 16, grid_y: int = 16, grid_w: int = 8) -> torch.Tensor:
    """[num, 12, grid_w, grid_y, grid_x] with A = [I | 0] at every vertex: channels 0, 5 and 10 are 1."""
    g = torch.zeros((num, 12, grid_w, grid_y, grid_x), dtype=torch.float32)
    g[:, (0, 5, 10)] = 1.0
    return g


class BilateralGrids(nn.Module):
    """`num` cameras' grids as one parameter `grids` [num, 12, L = grid_w, GH = grid_y, GW = grid_x], initialised to the identity."""

    def __init__(self, num: int, grid_x: int = 16, grid_y: int = 16, grid_w: int = 8):
        super().__init__()
        if int(num) < 1:
            raise ValueError(f"fused_bilagrid: num must be >= 1 (got {num})")
        _grid_dims((int(num), 12, int(grid_w), int(grid_y), int(grid_x)), 1)
        self.grids = nn.Parameter(identity_grids(int(num), int(grid_x), int(grid_y), int(grid_w)))

    def forward(self, image: torch.Tensor, idx: int, window: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
        """`image` through camera `idx`'s grid (autograd's select routes the gradient into that slice of `grids`)."""
        idx = int(idx)
        if not 0 <= idx < int(self.grids.shape[0]):
            raise IndexError(f"fused_bilagrid: camera index {idx} outside [0, {int(self.grids.shape[0])})")
        return bilagrid_apply(self.grids[idx], image, window=window)

    def tv_loss(self) -> torch.Tensor:
        return tv(self.grids)
