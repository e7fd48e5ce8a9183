"""Adam for the per-Gaussian parameter groups with a per-Gaussian learning rate, one HIP launch per step
(third item).

Mirror of how the reference drives its optimizer (/root/reference/scene/saro_gaussian.py):
  :306-323  groups xyz / f_dc / f_rest / opacity / scaling / rotation / temporal_pos, torch.optim.Adam(l, lr=0.0, eps=1e-15)
  :345-398  update_learning_rate assigns  param_group['lr'] = lr * self.inv_intergral  -- a [P,1] tensor: one rate per row

`GaussianAdam` keeps torch.optim.Adam's surface for those groups (`param_groups` with 'params' / 'lr' / 'name',
`step()`, `zero_grad()`, `state`), accepts a float or a [P] / [P,1] tensor as a group's 'lr', and updates every group in ONE
kernel (`gsrast_adam_step`).  amsgrad / maximize / weight_decay are not supported (the reference does not use them for
these groups).  GPU tensors only; no fallback.

`step(visibility=mask)` steps only the rows a view saw (`gsrast_adam_step_visible`): what upstream 3DGS ships as
`SparseGaussianAdam`, gsplat as `SelectiveAdam`, PyTorch as `torch.optim.SparseAdam`.  The mask is a render's `radii` (int32,
> 0 = visible) as it is, or a bool / uint8 tensor such as `view_parallel.distributed_step`'s `"visibility_filter"`.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch

from diff_gaussian_rasterization_ch3 import _C


class GaussianAdam:
    def __init__(self, param_groups: Iterable[Dict], betas=(0.9, 0.999), eps: float = 1e-15):
        self.param_groups: List[Dict] = []
        for g in param_groups:
            g = dict(g)
            ps = g["params"]
            g["params"] = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            if len(g["params"]) != 1:
                raise ValueError("GaussianAdam: one tensor per group (the per-Gaussian groups of saro_gaussian.py:306-318)")
            g.setdefault("lr", 0.0)
            self.param_groups.append(g)
        if len(self.param_groups) > 8:
            raise ValueError("GaussianAdam: at most 8 groups per launch")
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.state: Dict[torch.Tensor, Dict[str, torch.Tensor]] = {}
        self._step = 0

    def zero_grad(self, set_to_none: bool = True) -> None:
        for g in self.param_groups:
            p = g["params"][0]
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, *, visibility: Optional[torch.Tensor] = None) -> None:
        """One Adam step of every group that has a gradient.

        visibility=None: the dense step.  Otherwise a [P] or [P, 1] tensor on the parameters' device that selects rows: torch.bool /
        torch.uint8 (non-zero = visible) or torch.int32 (> 0 = visible: a render's `radii`).  A visible row gets exactly the dense
        update; a row that is not visible keeps its parameter and both moments bit for bit, and neither its gradient nor its
        per-row learning rate is read (NaN / Inf there reach nothing).  Every group's row count must equal the mask's length.

        The step count t of the bias corrections is the optimizer's one global count: it increases by one on every call, masked or
        not, an all-false mask included (torch.optim.SparseAdam's and gsplat's choice).  A row first seen late is therefore NOT
        bias-corrected as if that were its step 1."""
        mask = None
        if visibility is not None:
            if not isinstance(visibility, torch.Tensor) or visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
                raise RuntimeError("GaussianAdam: visibility must be a torch.bool, torch.uint8 or torch.int32 tensor "
                                   f"(got {getattr(visibility, 'dtype', type(visibility))})")
            if visibility.dim() not in (1, 2) or (visibility.dim() == 2 and visibility.shape[1] != 1):
                raise RuntimeError(f"GaussianAdam: visibility must have shape [P] or [P, 1] (got {tuple(visibility.shape)})")
            mask = visibility.detach().reshape(-1).contiguous()
        arr = (_C.AdamGroupStruct * len(self.param_groups))()
        n, keep, dev = 0, [], None
        for g in self.param_groups:
            p = g["params"][0]
            if p.grad is None:
                continue
            if mask is not None and (int(p.shape[0]) if p.dim() > 0 else 1) != mask.numel():
                raise RuntimeError(f"GaussianAdam: group {g.get('name')} has {int(p.shape[0]) if p.dim() > 0 else 1} rows, the visibility mask {mask.numel()} entries")
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("GaussianAdam: parameters must be contiguous float32 GPU tensors (no CPU fallback)")
            dev = p.device
            if mask is not None and mask.device != dev:
                raise RuntimeError(f"GaussianAdam: the visibility mask lives on {mask.device}, the parameters on {dev}")
            st = self.state.get(p)
            if st is None:
                st = self.state[p] = {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
            grad = p.grad.contiguous()
            rows = int(p.shape[0]) if p.dim() > 0 else 1
            width = p.numel() // max(rows, 1) if rows else 1
            lr = g["lr"]
            lr_rows = None
            if isinstance(lr, torch.Tensor) and lr.numel() > 1:
                if lr.numel() != rows:
                    raise RuntimeError(f"GaussianAdam: per-row lr of group {g.get('name')} has {lr.numel()} entries, the parameter {rows} rows")
                lr_rows = lr.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
                lr_scalar = 1.0
            else:
                lr_scalar = float(lr)
            a = arr[n]
            a.param, a.grad, a.exp_avg, a.exp_avg_sq = p.data_ptr(), grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            a.lr_rows = lr_rows.data_ptr() if lr_rows is not None else None
            a.lr, a.rows, a.width = lr_scalar, rows, max(width, 1)
            keep.extend((grad, lr_rows))
            n += 1
        self._step += 1
        if n == 0:
            return
        if mask is None:
            _C.launch("gsrast_adam_step", dev, n, arr, self.betas[0], self.betas[1], self.eps, self._step)
        else:
            _C.launch("gsrast_adam_step_visible", dev, n, arr, mask.data_ptr(), 4 if mask.dtype == torch.int32 else 1, mask.numel(),
                    self.betas[0], self.betas[1], self.eps, self._step)
