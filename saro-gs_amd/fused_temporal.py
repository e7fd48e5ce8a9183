"""The temporal lifespan on the device: what turns the deformation step into a 4-D model (include/gsrast.h: gsrast_temporal_*,
csrc/gsrast_temporal.h).

Mirror of the reference (paths relative to its root):
  scene/saro_gaussian.py:782-795  get_deformation: lifespan from the opacity head, distance, survival state, time_emb  -> temporal_gate
  scene/saro_gaussian.py:871-881  get_deformation_eval: state > 0.001 and the boolean index of ten tensors             -> temporal_select
  (not in the reference)          the same selection in a TRAINING step, differentiable (fused_densify.RowSelection)       -> temporal_rows
  scene/saro_gaussian.py:761-777  get_intergral (Eq. 22)                                                              -> temporal_integral
  scene/saro_gaussian.py:345-356  update_learning_rate's integral prune and inv_intergral                              -> temporal_prune

With head = the opacity head's output AFTER its Sigmoid ([P,1] or [P]), c = temporal_pos (sigmoid(temporal_pos) under sigmoid_tcenter)
and min_scale = min_interval / duration:
    lifespan = (1 - min_scale) (1 - head) + min_scale;   distance = t - c;   state = exp(-4 (distance / lifespan)^2)
    time_emb = [distance, sin, cos, sin 2., cos 2., ...]  (2 multires + 1 columns, the reference's Embedder)
`state` is activate_gaussians' `trbfoutput`, `time_emb` is fused_mlp3's `x_tail` (no gradient: the reference detaches it at the cat; the
second embedding the reference computes, time_emb(0), is the constant row [0, 0, 1, 0, 1, ...]).  One launch forward, one backward that
recomputes everything from the two inputs.  GPU fp32 tensors only; there is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

import fused_densify
from diff_gaussian_rasterization_ch3 import _C

MAX_MULTIRES = 8
MAX_SELECT_TENSORS = 14      # + state and time_emb: the 16 arrays one gsrast_densify_apply moves


def _timestamp(t) -> float:
    """A Python float.  A one-element tensor is read with float(): that SYNCHRONISES with the device when the tensor lives on the GPU."""
    t = float(t)
    if not math.isfinite(t):
        raise ValueError(f"fused_temporal: the timestamp must be finite (got {t})")
    return t


def _rows(head: torch.Tensor, temporal_pos: torch.Tensor) -> Tuple[int, torch.device, torch.Tensor, torch.Tensor]:
    """(P, device, head [P], temporal_pos [P]) as contiguous fp32, or the refusal."""
    for name, x in (("head", head), ("temporal_pos", temporal_pos)):
        if not x.is_cuda:
            raise RuntimeError(f"fused_temporal: {name} must be on a GPU (HIP) device; there is no CPU fallback")
        if x.dtype != torch.float32:
            raise ValueError(f"fused_temporal: {name} must be float32 (got {x.dtype})")
        if x.dim() not in (1, 2) or (x.dim() == 2 and int(x.shape[1]) != 1):
            raise ValueError(f"fused_temporal: {name} must be [P] or [P, 1] (got {tuple(x.shape)})")
    P = int(head.shape[0])
    if int(temporal_pos.shape[0]) != P:
        raise ValueError(f"fused_temporal: head has {P} rows, temporal_pos {int(temporal_pos.shape[0])}")
    if temporal_pos.device != head.device:
        raise RuntimeError(f"fused_temporal: temporal_pos is on {temporal_pos.device}, head on {head.device}")
    return P, head.device, head.detach().reshape(-1).contiguous(), temporal_pos.detach().reshape(-1).contiguous()


def _check_scalars(min_scale: float, multires: int = 0) -> Tuple[float, int]:
    if not 0.0 < float(min_scale) <= 1.0:
        raise ValueError(f"fused_temporal: min_scale = min_interval / duration must be in (0, 1] (got {min_scale})")
    if not 0 <= int(multires) <= MAX_MULTIRES:
        raise ValueError(f"fused_temporal: multires must be in [0, {MAX_MULTIRES}] (got {multires})")
    return float(min_scale), int(multires)


def _gate_forward(P, dev, h, c, t, min_scale, multires, sig, with_embedding, threshold: Optional[float]):
    """One launch: (lifespan [P,1], state [P,1], time_emb [P, 2 multires + 1] or None, dead uint8 [P] or None)."""
    o = dict(dtype=torch.float32, device=dev)
    lifespan, state = torch.empty((P, 1), **o), torch.empty((P, 1), **o)
    emb = torch.empty((P, 2 * multires + 1), **o) if with_embedding else None
    dead = torch.empty((P,), dtype=torch.uint8, device=dev) if threshold is not None else None
    _C.launch("gsrast_temporal_gate_forward", dev, P, multires, int(sig), t, min_scale, 0.0 if threshold is None else float(threshold), _C._ptr(h), _C._ptr(c),
            _C._ptr(lifespan), _C._ptr(state), _C._ptr(emb), _C._ptr(dead))
    return lifespan, state, emb, dead


class _TemporalGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, temporal_pos, t, min_scale, multires, sig, with_embedding, threshold=None):
        P, dev, h, c = _rows(head, temporal_pos)
        lifespan, state, emb, dead = _gate_forward(P, dev, h, c, t, min_scale, multires, sig, with_embedding, threshold)
        ctx.save_for_backward(h, c)
        ctx.args = (t, min_scale, sig, tuple(head.shape), tuple(temporal_pos.shape))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[x for x in (emb, dead) if x is not None])
        return lifespan, state, emb, dead      # (dead: the uint8 [P] of `threshold`, written by the same launch; None without one)

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, d_lifespan, d_state, _d_emb, _d_dead):
        h, c = ctx.saved_tensors
        t, min_scale, sig, head_shape, pos_shape = ctx.args
        P, dev = int(h.shape[0]), h.device
        need_head, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grads = []
        for g in (d_lifespan, d_state):
            if g is not None:
                if g.device != dev:
                    raise RuntimeError(f"fused_temporal: an upstream gradient is on {g.device}, the inputs on {dev}")
                g = g.contiguous().float()
            grads.append(g)
        d_head = torch.empty(head_shape, dtype=torch.float32, device=dev) if need_head else None
        d_pos = torch.empty(pos_shape, dtype=torch.float32, device=dev) if need_pos else None
        _C.launch("gsrast_temporal_gate_backward", dev, P, int(sig), t, min_scale, _C._ptr(h), _C._ptr(c), _C._ptr(grads[0]), _C._ptr(grads[1]),
                _C._ptr(d_head), _C._ptr(d_pos))
        return d_head, d_pos, None, None, None, None, None, None


def temporal_gate(head: torch.Tensor, temporal_pos: torch.Tensor, timestamp, *, min_scale: float, multires: int = 4,
                  sigmoid_tcenter: bool = False, with_embedding: bool = True):
    """Returns (lifespan [P,1], state [P,1], time_emb [P, 2 multires + 1] or None).  Gradients go to `head` and `temporal_pos`, each only
    when it requires one; an output that takes no part in the backward pass counts as zero upstream; time_emb is non-differentiable.
    Works under torch.no_grad().  `timestamp`: a Python float; a one-element tensor is converted with float(), which synchronises when it
    lives on the GPU."""
    min_scale, multires = _check_scalars(min_scale, multires)
    return _TemporalGate.apply(head, temporal_pos, _timestamp(timestamp), min_scale, multires, bool(sigmoid_tcenter), bool(with_embedding))[:3]


def temporal_rows(head: torch.Tensor, temporal_pos: torch.Tensor, timestamp, *, min_scale: float, multires: int = 4,
                  sigmoid_tcenter: bool = False, threshold: float = 0.001, also_dead: Optional[torch.Tensor] = None):
    """get_deformation_eval's selection for a TRAINING step: the gate with `temporal_gate`'s full-size outputs and autograd, and the
    `fused_densify.RowSelection` of the rows with state > threshold, taken from the `dead` byte the gate launch itself writes (no second pass
    over `state`).  Returns (sel, lifespan [P,1], state [P,1], time_emb [P, 2 multires + 1]); one read-back, the count.
    `sel.gather` / `sel.scatter` then run the heads, and optionally the rasterizer, on the alive rows only, with full-size gradients on the leaves.
    Exactness: a dropped row has opacity * state <= threshold, and the blend rejects every pair with alpha < 1/255, with or without
    antialiasing (that factor is <= 1).  So while threshold < 1/255 a dropped row adds nothing to the image and every gradient the render
    sends back to it is exactly zero: selecting changes no result.  A threshold >= 1/255 makes it an approximation.
    also_dead: a bool / uint8 [P] or [P, 1] tensor OR-ed into the mask -- the caller's own cull, e.g. the negation of mark_visible on the base
    positions.  Unlike the lifespan rule that one IS an approximation wherever a head's residual would have moved a culled row into view."""
    min_scale, multires = _check_scalars(min_scale, multires)
    t = _timestamp(timestamp)
    if also_dead is not None:
        fused_densify._check_mask(also_dead, int(head.shape[0]) if head.dim() else None, "also_dead")
    lifespan, state, emb, dead = _TemporalGate.apply(head, temporal_pos, t, min_scale, multires, bool(sigmoid_tcenter), True, float(threshold))
    P, dev = int(dead.shape[0]), dead.device
    if also_dead is not None:
        if also_dead.device != dev:
            raise RuntimeError(f"fused_temporal: also_dead is on {also_dead.device}, head on {dev}")
        dead = dead | (also_dead.detach().reshape(-1) != 0).to(torch.uint8)
    return fused_densify._select_dead_u8(dead, P, dev), lifespan, state, emb


@torch.no_grad()
def temporal_select(head: torch.Tensor, temporal_pos: torch.Tensor, timestamp, tensors: Sequence[torch.Tensor], *, min_scale: float,
                    multires: int = 4, sigmoid_tcenter: bool = False, threshold: float = 0.001):
    """get_deformation_eval's selection: the gate, then every row with !(state > threshold) leaves `state`, `time_emb` and each tensor of
    `tensors` (at most 14, [P, ...] contiguous fp32 of 1 ... 64 floats per row) in ONE row-moving launch instead of one boolean index per
    tensor.  Survivors keep index order, as tensor[mask] leaves them.  One read-back: the count.
    Returns (count, state [count,1], time_emb [count, 2 multires + 1], [t[alive] for t in tensors]); count = 0 gives empty tensors."""
    min_scale, multires = _check_scalars(min_scale, multires)
    t = _timestamp(timestamp)
    P, dev, h, c = _rows(head, temporal_pos)
    tensors = list(tensors)
    if len(tensors) > MAX_SELECT_TENSORS:
        raise RuntimeError(f"fused_temporal: {len(tensors)} tensors to select, at most {MAX_SELECT_TENSORS} per call")
    for k, x in enumerate(tensors):
        fused_densify._check_param(x, f"tensor {k}", P)
        if not 1 <= fused_densify._rows_width(x) <= 64 or x.numel() != P * fused_densify._rows_width(x):
            raise RuntimeError(f"fused_temporal: tensor {k} has {tuple(x.shape)}: 1 ... 64 floats per row")
    if P == 0:
        o = dict(dtype=torch.float32, device=dev)
        return 0, torch.empty((0, 1), **o), torch.empty((0, 2 * multires + 1), **o), [x.clone() for x in tensors]
    _, state, emb, dead = _gate_forward(P, dev, h, c, t, min_scale, multires, sigmoid_tcenter, True, float(threshold))
    moved = [(x, None, None, _C.DENSIFY_COPY) for x in [state, emb] + tensors]
    counts, results = fused_densify._run(P, dev, 1, dict(thr=math.inf, prune_src=_C._ptr(dead)), moved, None, None, None, None)
    out = [r[0] for r in results]
    return counts["P"], out[0], out[1], out[2:]


@torch.no_grad()
def temporal_integral(head: torch.Tensor, temporal_pos: torch.Tensor, *, min_scale: float, min_integral: float, start: float = 0.0,
                      end: float = 1.0, sigmoid_tcenter: bool = False):
    """get_intergral and the first lines of update_learning_rate.  Returns (integral [P,1], dead_mask uint8 [P] = !(integral >
    min_integral), inv [P,1] = integral_max / integral on a valid row and 0 on a dead one -- the reference's (1/I) / min(1/I) --, stats:
    int32 [2] on the device = (the float bits of the largest valid integral, the number of valid rows)).  No synchronisation."""
    min_scale, _ = _check_scalars(min_scale)
    P, dev, h, c = _rows(head, temporal_pos)
    integral, inv = torch.empty((P, 1), dtype=torch.float32, device=dev), torch.empty((P, 1), dtype=torch.float32, device=dev)
    dead = torch.empty((P,), dtype=torch.uint8, device=dev)
    stats = torch.zeros((2,), dtype=torch.int32, device=dev) if P == 0 else torch.empty((2,), dtype=torch.int32, device=dev)
    _C.launch("gsrast_temporal_integral", dev, P, int(bool(sigmoid_tcenter)), float(start), float(end), min_scale, float(min_integral), _C._ptr(h), _C._ptr(c),
            _C._ptr(integral), _C._ptr(dead), _C._ptr(inv), stats.data_ptr())
    return integral, dead, inv, stats


@torch.no_grad()
def temporal_prune(opt, head: torch.Tensor, temporal_pos: torch.Tensor, *, min_scale: float, min_integral: float, start: float = 0.0, end: float = 1.0,
                   sigmoid_tcenter: bool = False, stats: Optional[fused_densify.DensifyStats] = None, extras: Iterable[torch.Tensor] = (),
                   contrib: Optional[fused_densify.ContribStats] = None):
    """update_learning_rate's every-50-iterations block (scene/saro_gaussian.py:349-356): the integral, then fused_densify.prune of the rows
    with integral <= min_integral from `opt`'s per-Gaussian groups, their moments, `stats`, `contrib` and `extras`, with inv_intergral
    carried along.  Returns (counts, {group name: new parameter}, inv [P',1], [the extras at P']); `inv` is what the caller multiplies
    into the six groups' `lr` (GaussianAdam takes [P',1] rates).  `head` is the opacity head evaluated on the model as it stands."""
    _, dead, inv, _ = temporal_integral(head, temporal_pos, min_scale=min_scale, min_integral=min_integral, start=start, end=end,
                                        sigmoid_tcenter=sigmoid_tcenter)
    counts, new, rest = fused_densify.prune(opt, dead, stats, extras=[inv, *extras], contrib=contrib)
    return counts, new, rest[0], rest[1:]
