"""Densification on the device: clone / split / prune of the per-Gaussian parameter groups TOGETHER with their Adam moments, and
the per-iteration statistics the criterion reads (include/gsrast.h: gsrast_densify_plan / _apply / _stats_update,
csrc/gsrast_densify.h).

Mirror of the reference (paths relative to its root):
  scene/saro_gaussian.py:705-736  densify_pruneclone  (clone :685-701, split :646-682, prune :577-593)            -> densify_and_prune
  scene/saro_gaussian.py:555-640  _prune_optimizer / cat_tensors_to_optimizer / densification_postfix             -> inside both calls
  scene/saro_gaussian.py:577-593  prune_points; :347-356 the every-50-iterations integral prune                    -> prune
  train.py:282-292 + scene/saro_gaussian.py:745-750 add_densification_stats_grad                                   -> DensifyStats.update
Not in the reference: ContribStats accumulates the rasterizer's per-Gaussian blend-weight statistics (`contrib=sink`) over views and ranks
them into a keep mask, whose negation is a `prune_mask` for the two calls below (importance pruning: LightGaussian, RadSplat, Mini-Splatting).

One classification pass, one scan and ONE row-moving launch for all groups replace the reference's chain of boolean-mask indexing
and torch.cat over seven groups and fourteen moment tensors; the only host read-back is the five counts (for the new P).  The result
is the reference's layout row for row:
  [ originals !split && !pruned | clones | split copy 0 | copy 1 | ... ]      (every part in index order)
and is bit-identical from run to run and from rank to rank (no atomics), so replicated models stay replicated.

Not in the reference either: `select_rows` / `RowSelection` keep a prune-only plan beyond its apply and make the row move differentiable --
`gather` ([P, ...] -> [n, ...], gsrast_densify_apply) and `scatter` ([n, ...] -> [P, ...] with zeros elsewhere, gsrast_densify_scatter), each the
other's backward -- so that a training step runs the deformation heads, and optionally the rasterizer, on the rows alive at the view's time.

The second policy, 3DGS-MCMC as gsplat's MCMCStrategy runs it (include/gsrast.h: gsrast_mcmc_*, csrc/gsrast_mcmc.h), sits beside it:
  gsplat/strategy/ops.py relocate + gsplat/relocation.py compute_relocation                                        -> mcmc_relocate
  gsplat/strategy/ops.py sample_add                                                                                -> mcmc_grow
  gsplat/strategy/ops.py inject_noise_to_position                                                                  -> mcmc_inject_noise
  MCMCStrategy.step_post_backward's refine branch (relocate, then add)                                             -> mcmc_refine
A fixed budget (`cap_max`), no gradient thresholds, dead Gaussians re-used instead of pruned.  The multinomial is integer arithmetic on
fixed-point weights, so the same draws select the same rows on every rank.  Two stated deviations from gsplat: compute_relocation's
alternating sum runs in fp64, and a model with no alive row is a no-op where torch.multinomial would raise.

What stays the caller's: `reset_opacity` and the colmap `z < 4.5` rule, which arrives here as `prune_mask`.  The integral prune
`get_intergral() <= min_intergral` is `fused_temporal.temporal_prune` (the integral and its mask on the device from the opacity head's
output, then `prune` below with `inv_intergral` carried along); per-row `lr` tensors of the old P (GaussianAdam.step raises on a mismatch) and the
`view_parallel.StepBucket`, which is rebuilt after P changed.  GPU tensors only; no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization_ch3 import _C

MAX_GROUPS = 16
COUNT_NAMES = ("n_kept", "n_clone", "n_split", "n_split_all", "P")
DEFAULT_NAMES = dict(xyz="xyz", scaling="scaling", rotation="rotation", opacity="opacity")


class DensifyStats:
    """xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P] (scene/saro_gaussian.py:638-640), updated by one launch per iteration."""

    def __init__(self, P: int, device):
        self.device = torch.device(device)
        self.reset(P)

    def reset(self, P: int) -> None:
        """Zeros at P rows, as densification_postfix leaves them (scene/saro_gaussian.py:638-641)."""
        o = dict(dtype=torch.float32, device=self.device)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = torch.zeros((P, 1), **o), torch.zeros((P, 1), **o), torch.zeros((P,), **o)

    @property
    def P(self) -> int:
        return int(self.denom.shape[0])

    @torch.no_grad()
    def update(self, step_out: Dict[str, torch.Tensor], use_absgrad: bool = False) -> None:
        """step_out: what `view_parallel.distributed_step` returns.  Its "viewspace_point_grad" [P,1] is ALREADY the per-visible mean
        (sum of the per-view norms / visibility count, train.py:286-287) and is added as it is.  A dict with "viewspace_point_grad_sum"
        [P] or [P,1] instead -- the plain sum over the batch -- is divided by "visibility_count" here.  "visibility_count" [P] (rows
        with count > 0 are updated, the others untouched) and "radii" [P] (max over the batch) are read in both forms.
        use_absgrad=True: "viewspace_point_absgrad" [P,1] (distributed_step's per-visible mean of the absolute screen-space gradient,
        there when the views rendered with ``absgrad=``) is accumulated in place of "viewspace_point_grad"; KeyError if it is absent.
        The densification threshold for it is the caller's: higher than for the signed gradient (AbsGS: about 2x)."""
        if use_absgrad:
            is_mean, grad = True, step_out["viewspace_point_absgrad"]
        else:
            is_mean = "viewspace_point_grad_sum" not in step_out
            grad = step_out["viewspace_point_grad" if is_mean else "viewspace_point_grad_sum"]
        P = self.P
        dev = _C._require_gpu(self.denom)
        f = lambda t, n: _flat_f32(t, n, P, dev)  # noqa: E731
        grad, count, radii = f(grad, "viewspace_point_grad"), f(step_out["visibility_count"], "visibility_count"), f(step_out["radii"], "radii")
        _C.launch("gsrast_densify_stats_update", dev, P, _C._ptr(grad), _C._ptr(count), _C._ptr(radii), _C._ptr(self.xyz_gradient_accum),
                _C._ptr(self.denom), _C._ptr(self.max_radii2D), int(is_mean))


class ContribStats:
    """The rasterizer's blend-weight statistics (`forward(..., contrib=sink)`, include/gsrast.h: gsrast_contrib_stats) accumulated over views:
    weight_sum, pixel_count, top_count (summed over the views), weight_max (the maximum over them) and views (in how many views the
    Gaussian had pixel_count > 0), [P] float32 each.  Plain torch ops on whatever device the sinks live on: this is not a hot path.
    Storage: `sums` [P,4] = (weight_sum, pixel_count, top_count, views) and `weight_max` [P] -- what view_parallel.reduce_contrib_stats
    all-reduces with SUM and MAX."""
    SUM_COLUMNS = ("weight_sum", "pixel_count", "top_count", "views")
    COLUMNS = SUM_COLUMNS + ("weight_max",)

    def __init__(self, P: int, device):
        self.device = torch.device(device)
        self.reset(P)

    def reset(self, P: Optional[int] = None) -> None:
        """Zeros (at P rows; default: the current P)."""
        P = self.P if P is None else int(P)
        self.sums = torch.zeros((P, 4), dtype=torch.float32, device=self.device)
        self.weight_max = torch.zeros((P,), dtype=torch.float32, device=self.device)

    @property
    def P(self) -> int:
        return int(self.weight_max.shape[0])

    weight_sum = property(lambda self: self.sums[:, 0])
    pixel_count = property(lambda self: self.sums[:, 1])
    top_count = property(lambda self: self.sums[:, 2])
    views = property(lambda self: self.sums[:, 3])

    @torch.no_grad()
    def update(self, sink: torch.Tensor) -> None:
        """One view's sink [P,4] = [weight_sum, weight_max, pixel_count, top_count] (the rasterizer's columns)."""
        if tuple(sink.shape) != (self.P, 4) or sink.device != self.device:
            raise RuntimeError(f"ContribStats.update: the sink must be [{self.P}, 4] on {self.device} (got {list(sink.shape)} on {sink.device})")
        sink = sink.detach().to(torch.float32)
        self.sums[:, 0] += sink[:, 0]
        self.sums[:, 1] += sink[:, 2]
        self.sums[:, 2] += sink[:, 3]
        self.sums[:, 3] += (sink[:, 2] > 0).to(torch.float32)
        torch.maximum(self.weight_max, sink[:, 1], out=self.weight_max)

    def column(self, name: str) -> torch.Tensor:
        if name not in self.COLUMNS:
            raise KeyError(f"ContribStats: no column {name!r} (one of {', '.join(self.COLUMNS)})")
        return getattr(self, name)

    @torch.no_grad()
    def keep_mask_by_rank(self, column: str, keep_fraction: float) -> torch.Tensor:
        """bool [P]: True for the ceil(keep_fraction * P) Gaussians with the largest `column`; among equal values the lower index ranks
        first (a stable sort), so replicated ranks agree.  Its negation is the `prune_mask` of prune() / densify_and_prune()."""
        if not 0.0 <= float(keep_fraction) <= 1.0:
            raise ValueError(f"keep_fraction must be in [0, 1] (got {keep_fraction})")
        P = self.P
        k = min(P, int(math.ceil(float(keep_fraction) * P)))
        order = torch.sort(self.column(column), descending=True, stable=True).indices
        mask = torch.zeros((P,), dtype=torch.bool, device=self.device)
        mask[order[:k]] = True
        return mask


def _flat_f32(t: torch.Tensor, name: str, P: int, dev: torch.device) -> torch.Tensor:
    if t.numel() != P:
        raise RuntimeError(f"fused_densify: {name} has {t.numel()} entries, the model {P} Gaussians")
    if t.device != dev:
        raise RuntimeError(f"fused_densify: {name} must live on {dev} (got {t.device}); there is no CPU fallback")
    return t.detach().to(torch.float32).reshape(-1).contiguous()


def _rows_width(t: torch.Tensor) -> int:
    return max(int(math.prod(t.shape[1:])), 1)


def _check_param(p: torch.Tensor, name: str, P: int) -> None:
    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError(f"fused_densify: {name} must be a contiguous float32 GPU tensor (no CPU fallback)")
    if p.dim() < 1 or int(p.shape[0]) != P:
        raise RuntimeError(f"fused_densify: {name} has {tuple(p.shape)}, expected {P} rows")


def _plan(P: int, dev: torch.device, N: int, plan_args: dict) -> Tuple[torch.Tensor, List[int]]:
    """gsrast_densify_plan and the read-back of its five counts (the one synchronisation).  Returns (scratch, the counts as host words):
    together they are the plan, which any number of gsrast_densify_apply / gsrast_densify_scatter calls with the same P and N may use."""
    L = _C.lib()
    scratch = torch.empty(int(L.gsrast_densify_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    counts_dev = torch.empty(5, dtype=torch.int32, device=dev)
    with _C._on_device(dev):
        rc = L.gsrast_densify_plan(P, N, plan_args.get("accum"), plan_args.get("denom"), plan_args.get("grad_scale"), plan_args.get("scaling"),
                                   plan_args.get("opacity"), plan_args.get("prune_src"), float(plan_args["thr"]), float(plan_args.get("tau", 0.0)),
                                   float(plan_args.get("min_opacity", 0.0)), scratch.data_ptr(), counts_dev.data_ptr(), _C._stream_of(dev))
        if rc != 0:
            raise _C._err(rc, "gsrast_densify_plan")
        host = [int(v) & 0xFFFFFFFF for v in counts_dev.cpu().tolist()]
    return scratch, host


def _run(P: int, dev: torch.device, N: int, plan_args: dict, moved: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], int]],
         rotation: Optional[torch.Tensor], scaling: Optional[torch.Tensor], generator, noise: Optional[torch.Tensor]):
    """plan -> read the counts back (the one synchronisation) -> noise -> allocate -> apply.  `moved`: (src, exp_avg, exp_avg_sq, role) per
    group.  Returns (counts dict, [(dst, dst_m, dst_v)])."""
    if len(moved) > MAX_GROUPS:
        raise RuntimeError(f"fused_densify: {len(moved)} arrays to move, at most {MAX_GROUPS} per launch")
    L = _C.lib()
    scratch, host = _plan(P, dev, N, plan_args)
    with _C._on_device(dev):
        stream = _C._stream_of(dev)
        counts = dict(zip(COUNT_NAMES, host))
        n_all, P_new = counts["n_split_all"], counts["P"]
        if noise is None:
            noise = torch.randn((N * n_all, 3), generator=generator, device=dev, dtype=torch.float32) if n_all else None
        elif n_all:
            if tuple(noise.shape) != (N * n_all, 3) or noise.device != dev:
                raise RuntimeError(f"fused_densify: noise must be [{N * n_all}, 3] on {dev} (N * n_split_all rows), got {tuple(noise.shape)} on {noise.device}")
            noise = noise.to(torch.float32).contiguous()
        arr = (_C.DensifyGroupStruct * max(len(moved), 1))()
        out = []
        for a, (src, m, v, role) in zip(arr, moved):
            shape = (P_new,) + tuple(src.shape[1:])
            dst = torch.empty(shape, dtype=torch.float32, device=dev)
            dm = torch.empty(shape, dtype=torch.float32, device=dev) if m is not None else None
            dv = torch.empty(shape, dtype=torch.float32, device=dev) if v is not None else None
            a.src, a.src_m, a.src_v = _C._ptr(src), _C._ptr(m), _C._ptr(v)
            a.dst, a.dst_m, a.dst_v = _C._ptr(dst), _C._ptr(dm), _C._ptr(dv)
            a.width, a.role = _rows_width(src), role
            out.append((dst, dm, dv))
        if P_new == 0:          # nothing survives: the new tensors are empty, there is no row to move
            return counts, out
        ch = (C.c_uint * 5)(*host)
        rc = L.gsrast_densify_apply(P, N, scratch.data_ptr(), ch, len(moved), arr, _C._ptr(rotation), _C._ptr(scaling),
                                    _C._ptr(noise) if n_all else None, stream)
        if rc != 0:
            raise _C._err(rc, "gsrast_densify_apply")
    return counts, out


def _optimizer_groups(opt, P: Optional[int] = None):
    """[(group, parameter, state or None)] of the optimizer's per-Gaussian groups (one tensor each, saro_gaussian.py:306-318)."""
    rows = []
    for g in opt.param_groups:
        if len(g["params"]) != 1:
            raise RuntimeError("fused_densify: one tensor per group (the per-Gaussian groups of saro_gaussian.py:306-318)")
        p = g["params"][0]
        if P is None:
            P = int(p.shape[0])
        _check_param(p, f"group {g.get('name')}", P)
        st = opt.state.get(p)
        if st is not None and ("exp_avg" not in st or "exp_avg_sq" not in st):
            st = None
        if st is not None:
            for k in ("exp_avg", "exp_avg_sq"):
                if st[k].shape != p.shape or not st[k].is_contiguous() or st[k].dtype != torch.float32 or st[k].device != p.device:
                    raise RuntimeError(f"fused_densify: {k} of group {g.get('name')} does not match its parameter")
        rows.append((g, p, st))
    return rows, (P or 0)


def _install(opt, rows, results) -> Dict[str, nn.Parameter]:
    """Every group's params[0] becomes a fresh leaf; opt.state is re-keyed with the new moments (other entries, e.g. torch.optim's
    "step", are kept -- as is GaussianAdam's own step count)."""
    new = {}
    for (g, p, st), (dst, dm, dv) in zip(rows, results):
        q = nn.Parameter(dst.requires_grad_(True))
        old = opt.state.pop(p, None)
        if st is not None:
            ns = dict(old)
            ns["exp_avg"], ns["exp_avg_sq"] = dm, dv
            opt.state[q] = ns
        g["params"][0] = q
        new[g.get("name")] = q
    return new


@torch.no_grad()
def densify_and_prune(opt, stats: DensifyStats, *, grad_threshold: float, percent_dense: float, extent: float, min_opacity: Optional[float] = None,
                      prune_mask: Optional[torch.Tensor] = None, grad_scale: Optional[torch.Tensor] = None, n_split: int = 2,
                      generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None, names: Dict[str, str] = DEFAULT_NAMES):
    """densify_pruneclone (scene/saro_gaussian.py:705-736) on `opt`'s per-Gaussian groups (GaussianAdam, or any optimizer with
    torch.optim's `param_groups` / `state` surface) with the statistics in `stats`:
      g = accum / denom (NaN -> 0) * grad_scale;  clone where g >= grad_threshold and max exp(scaling) <= percent_dense * extent,
      split into n_split copies where g >= grad_threshold and max exp(scaling) > percent_dense * extent,
      prune where prune_mask (bool / uint8 [P]) or sigmoid(opacity) < min_opacity -- a pruned source leaves neither clone nor copies.
    grad_scale: the reference's inv_intergral_fordensify [P] / [P,1].  names: which group is xyz / scaling / rotation / opacity.
    noise [n_split * n_split_all, 3] (row k * n_split_all + rank among ALL split-selected sources) is drawn with torch.randn(...,
    generator=generator) on the device unless given.  Every group's params[0] is replaced by a fresh nn.Parameter leaf, opt.state is
    re-keyed with the new moments (kept rows gathered, new rows zero), `stats` is reset to zeros at the new P.
    Returns (counts, {group name: new parameter}); counts = dict(n_kept, n_clone, n_split, n_split_all, P)."""
    rows, P = _optimizer_groups(opt, stats.P)
    by_name = {g.get("name"): p for g, p, _ in rows}
    for role in ("xyz", "scaling", "rotation", "opacity"):
        if names.get(role) not in by_name:
            raise RuntimeError(f"fused_densify: no group named {names.get(role)!r} (names[{role!r}])")
    xyz, scaling, rotation, opacity = (by_name[names[r]] for r in ("xyz", "scaling", "rotation", "opacity"))
    if _rows_width(xyz) != 3 or _rows_width(scaling) != 3 or _rows_width(rotation) != 4 or _rows_width(opacity) != 1:
        raise RuntimeError("fused_densify: xyz / scaling / rotation / opacity must be [P,3] / [P,3] / [P,4] / [P,1]")
    dev = _C._require_gpu(xyz)
    keep = [_flat_f32(stats.xyz_gradient_accum, "xyz_gradient_accum", P, dev), _flat_f32(stats.denom, "denom", P, dev)]
    plan = dict(accum=_C._ptr(keep[0]), denom=_C._ptr(keep[1]), scaling=_C._ptr(scaling), opacity=_C._ptr(opacity),
                thr=grad_threshold, tau=float(percent_dense) * float(extent), min_opacity=0.0 if min_opacity is None else min_opacity)
    if grad_scale is not None:
        keep.append(_flat_f32(grad_scale, "grad_scale", P, dev))
        plan["grad_scale"] = _C._ptr(keep[-1])
    if prune_mask is not None:
        keep.append(_mask_u8(prune_mask, P, dev))
        plan["prune_src"] = _C._ptr(keep[-1])
    role_of = {id(xyz): _C.DENSIFY_XYZ, id(scaling): _C.DENSIFY_SCALING}
    moved = [(p, st["exp_avg"] if st else None, st["exp_avg_sq"] if st else None, role_of.get(id(p), _C.DENSIFY_COPY)) for _, p, st in rows]
    counts, results = _run(P, dev, int(n_split), plan, moved, rotation, scaling, generator, noise)
    new = _install(opt, rows, results)
    stats.reset(counts["P"])
    return counts, new


def _mask_u8(mask: torch.Tensor, P: int, dev: torch.device) -> torch.Tensor:
    if mask.numel() != P:
        raise RuntimeError(f"fused_densify: the prune mask has {mask.numel()} entries, the model {P} Gaussians")
    if mask.device != dev:
        raise RuntimeError(f"fused_densify: the prune mask must live on {dev}; there is no CPU fallback")
    return mask.reshape(-1).to(torch.uint8).contiguous()


@torch.no_grad()
def prune(opt, mask: torch.Tensor, stats: Optional[DensifyStats] = None, extras: Iterable[torch.Tensor] = (), contrib: Optional[ContribStats] = None):
    """prune_points (scene/saro_gaussian.py:577-593) and the integral prune of update_learning_rate (:347-356): rows with mask != 0
    leave every group, its moments, `stats` (gathered, NOT reset), `contrib` (a ContribStats: gathered like `stats`, NOT reset -- the
    survivors keep what the views so far saw of them) and every tensor of `extras` ([P, ...] float32 each, e.g. t_gradient_accum).
    The same plan / apply pair with an infinite threshold.  Returns (counts, {group name: new parameter}, [new extras])."""
    rows, P = _optimizer_groups(opt, stats.P if stats is not None else None)
    dev = _C._require_gpu(rows[0][1]) if rows else _C._require_gpu(mask)
    m8 = _mask_u8(mask, P, dev)
    moved = [(p, st["exp_avg"] if st else None, st["exp_avg_sq"] if st else None, _C.DENSIFY_COPY) for _, p, st in rows]
    carried: List[torch.Tensor] = (([stats.xyz_gradient_accum, stats.denom, stats.max_radii2D] if stats is not None else [])
                                   + ([contrib.sums, contrib.weight_max] if contrib is not None else []) + list(extras))
    for k, t in enumerate(carried):
        _check_param(t, f"carried tensor {k}", P)
        moved.append((t, None, None, _C.DENSIFY_COPY))
    counts, results = _run(P, dev, 1, dict(thr=math.inf, prune_src=_C._ptr(m8)), moved, None, None, None, None)
    new = _install(opt, rows, results[: len(rows)])
    rest = [r[0] for r in results[len(rows):]]
    if stats is not None:
        stats.xyz_gradient_accum, stats.denom, stats.max_radii2D = rest[:3]
        rest = rest[3:]
    if contrib is not None:
        contrib.sums, contrib.weight_max = rest[:2]
        rest = rest[2:]
    return counts, new, rest


# ---- differentiable row selection -------------------------------------------------------------------------------------------------
_MOVABLE = (torch.float32, torch.int32)


def _check_mask(mask, P: Optional[int], name: str) -> int:
    """The refusals of a row mask that need no device: a bool / uint8 [P] or [P, 1] tensor (P: the expected length, None: any).  Returns P."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"fused_densify: {name} must be a bool or uint8 tensor (got {getattr(mask, 'dtype', type(mask).__name__)})")
    if mask.dim() not in (1, 2) or (mask.dim() == 2 and int(mask.shape[1]) != 1):
        raise RuntimeError(f"fused_densify: {name} must be [P] or [P, 1] (got {tuple(mask.shape)})")
    if P is not None and int(mask.shape[0]) != P:
        raise RuntimeError(f"fused_densify: {name} has {int(mask.shape[0])} entries, expected {P} rows")
    return int(mask.shape[0])


def _check_movable(tensors: Sequence[torch.Tensor], rows: int, dev: torch.device, what: str) -> None:
    """What one gsrast_densify_apply / gsrast_densify_scatter launch can move, refused before it: at most 16 contiguous float32 / int32 tensors of
    `rows` rows and 1 ... 64 four-byte elements per row, on `dev`."""
    if len(tensors) > MAX_GROUPS:
        raise RuntimeError(f"fused_densify: {len(tensors)} tensors to {what}, at most {MAX_GROUPS} per call")
    for k, x in enumerate(tensors):
        if not isinstance(x, torch.Tensor) or x.dtype not in _MOVABLE:
            raise RuntimeError(f"fused_densify: {what}: tensor {k} must be float32 or int32 (got {getattr(x, 'dtype', type(x).__name__)})")
        if x.dim() < 1 or int(x.shape[0]) != rows:
            raise RuntimeError(f"fused_densify: {what}: tensor {k} has {tuple(x.shape)}, expected {rows} rows")
        if not 1 <= int(math.prod(x.shape[1:])) <= 64:
            raise RuntimeError(f"fused_densify: {what}: tensor {k} has {tuple(x.shape)}: 1 ... 64 four-byte elements per row")
        if not x.is_contiguous():
            raise RuntimeError(f"fused_densify: {what}: tensor {k} must be contiguous")
        if x.device != dev:
            raise RuntimeError(f"fused_densify: {what}: tensor {k} must live on {dev} (got {x.device}); there is no CPU fallback")


class RowSelection:
    """A prune-only plan that outlives its apply: which `count` of `P` rows are kept, as the scratch and the host counts of one
    gsrast_densify_plan.  Immutable; `gather` and `scatter` may be called any number of times, in any order, each ONE launch for all its tensors:
        a_n, b_n = sel.gather(a, b)      # [P, ...] -> [count, ...], the kept rows in index order (x[mask]);            backward = scatter
        r_P, = sel.scatter(r_n)          # [count, ...] -> [P, ...], +0.0 on every other row (zeros.index_copy(0, rows)); backward = gather
    At most 16 tensors per call, each contiguous with 1 ... 64 four-byte elements per row on the selection's device.  float32 tensors are
    differentiable (once: a double backward raises); int32 tensors (radii, row numbers) are moved as bits and are non-differentiable; anything
    else raises before a launch.  The backward launches only for the tensors that need a gradient and received one.  Both work under
    torch.no_grad(), and with count = 0 or P = 0.  With a `GradArena` installed, gathering a leaf that requires a gradient raises (a render of
    the gathered rows does not fit the arena: the leaf's gradient would miss the exchanged bucket), as `features=` does there.
    Made by `select_rows` or `fused_temporal.temporal_rows`."""
    __slots__ = ("P", "count", "device", "_scratch", "_counts", "_rows")

    def __init__(self, P: int, device: torch.device, scratch: Optional[torch.Tensor], counts: Sequence[int]):
        set_ = lambda k, v: object.__setattr__(self, k, v)  # noqa: E731
        set_("P", int(P)); set_("count", int(counts[0])); set_("device", torch.device(device))
        set_("_scratch", scratch); set_("_counts", (C.c_uint * 5)(*counts)); set_("_rows", None)

    def __setattr__(self, name, value):
        raise AttributeError("RowSelection is immutable")

    @property
    def rows(self) -> torch.Tensor:
        """int32 [count], ascending: the kept row numbers (an arange moved through the plan, built on first use)."""
        if self._rows is None:
            with torch.no_grad():
                object.__setattr__(self, "_rows", _move_rows(self, [torch.arange(self.P, dtype=torch.int32, device=self.device)], True)[0])
        return self._rows

    @property
    def mask(self) -> torch.Tensor:
        """bool [P]: True on the kept rows."""
        m = torch.zeros(self.P, dtype=torch.bool, device=self.device)
        m[self.rows.long()] = True
        return m

    def gather(self, *tensors: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        if _C._grad_arena is not None and torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.is_leaf and x.requires_grad for x in tensors):
            raise RuntimeError("RowSelection.gather of a leaf that requires a gradient is not supported with a GradArena installed (multi-GPU / "
                               "view_parallel training): a render of the gathered rows does not fit the arena, so the leaf's gradient would arrive "
                               "outside the bucket the exchange reduces; gather only the heads' inputs there, or uninstall it with _C.set_grad_arena(None)")
        _check_movable(tensors, self.P, self.device, "gather")
        return _GatherRows.apply(self, *tensors) if tensors else ()

    def scatter(self, *tensors: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        _check_movable(tensors, self.count, self.device, "scatter")
        return _ScatterRows.apply(self, *tensors) if tensors else ()


def _move_rows(sel: RowSelection, tensors: Sequence[torch.Tensor], compact: bool) -> List[torch.Tensor]:
    """One launch over `sel`'s plan for all of `tensors` (checked by the caller): gsrast_densify_apply ([P, ...] -> [count, ...]) when `compact`,
    else gsrast_densify_scatter ([count, ...] -> [P, ...]).  Nothing to write: no launch."""
    P, n, dev = sel.P, sel.count, sel.device
    rows_out = n if compact else P
    out = [torch.empty((rows_out,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev) for x in tensors]
    if rows_out == 0 or not tensors:
        return out
    arr = (_C.DensifyGroupStruct * len(tensors))()
    for a, src, dst in zip(arr, tensors, out):
        a.src, a.dst, a.width, a.role = _C._ptr(src), _C._ptr(dst), _rows_width(src), _C.DENSIFY_COPY
    if compact:
        _C.launch("gsrast_densify_apply", dev, P, 1, sel._scratch.data_ptr(), sel._counts, len(tensors), arr, None, None, None)
    else:
        _C.launch("gsrast_densify_scatter", dev, P, sel._scratch.data_ptr(), sel._counts, len(tensors), arr)
    return out


def _move_rows_backward(ctx, grads, compact: bool):
    """The transposed move of the upstream gradients that exist and are needed, in one launch; None for the others."""
    sel = ctx.sel
    todo = [k for k, g in enumerate(grads) if g is not None and ctx.needs_input_grad[k + 1]]
    gs = []
    for k in todo:
        g = grads[k]
        if g.device != sel.device or g.dtype != torch.float32:
            raise RuntimeError(f"fused_densify: an upstream gradient is {g.dtype} on {g.device}, expected float32 on {sel.device}")
        gs.append(g.contiguous())
    res: List[Optional[torch.Tensor]] = [None] * (1 + len(grads))
    for k, r in zip(todo, _move_rows(sel, gs, compact)):
        res[k + 1] = r
    return tuple(res)


def _move_rows_forward(ctx, sel, tensors, compact: bool):
    out = _move_rows(sel, [x.detach() for x in tensors], compact)
    ctx.sel = sel
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(*[o for o in out if o.dtype != torch.float32])
    return tuple(out)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sel, *tensors):
        return _move_rows_forward(ctx, sel, tensors, True)

    @staticmethod
    @once_differentiable      # (the kernels are not differentiable themselves: a double backward raises)
    def backward(ctx, *grads):
        return _move_rows_backward(ctx, grads, False)


class _ScatterRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sel, *tensors):
        return _move_rows_forward(ctx, sel, tensors, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _move_rows_backward(ctx, grads, True)


def _select_dead_u8(dead_u8: torch.Tensor, P: int, dev: torch.device) -> RowSelection:
    """The prune-only plan over `dead_u8` (uint8 [P] on `dev`, != 0: the row is dropped).  The count is the one read-back."""
    scratch, host = _plan(P, dev, 1, dict(thr=math.inf, prune_src=_C._ptr(dead_u8)))
    return RowSelection(P, dev, scratch, host)


def select_rows(*, keep: Optional[torch.Tensor] = None, dead: Optional[torch.Tensor] = None) -> RowSelection:
    """The selection of the rows with keep != 0, or with dead == 0: exactly one of the two, a bool / uint8 [P] or [P, 1] tensor on the GPU.
    Two launches (classify, scan) and one read-back, the count; the mask is not needed afterwards."""
    if (keep is None) == (dead is None):
        raise ValueError("fused_densify.select_rows: give exactly one of keep= and dead=")
    mask, name = (keep, "keep") if dead is None else (dead, "dead")
    P = _check_mask(mask, None, name)
    dev = _C._require_gpu(mask)
    flat = mask.detach().reshape(-1)
    return _select_dead_u8((flat == 0).to(torch.uint8) if dead is None else flat.to(torch.uint8).contiguous(), P, dev)


# ---- 3DGS-MCMC ------------------------------------------------------------------------------------------------------------------
DRAW_RANGE = 1 << 62      # draws are int64 in [0, DRAW_RANGE): draw d targets floor(d * W / 2^62) of the total weight W


def _mcmc_moved(opt, names: Dict[str, str], extras: Iterable[torch.Tensor]):
    """(rows, P, device, the opacity parameter, [(tensor, exp_avg, exp_avg_sq, role)] of every group and extra)."""
    rows, P = _optimizer_groups(opt)
    by_name = {g.get("name"): p for g, p, _ in rows}
    for role in ("scaling", "opacity"):
        if names.get(role) not in by_name:
            raise RuntimeError(f"fused_densify: no group named {names.get(role)!r} (names[{role!r}])")
    scaling, opacity = by_name[names["scaling"]], by_name[names["opacity"]]
    if _rows_width(scaling) != 3 or _rows_width(opacity) != 1:
        raise RuntimeError("fused_densify: scaling / opacity must be [P,3] / [P,1]")
    dev = _C._require_gpu(opacity)
    role_of = {id(scaling): _C.MCMC_SCALING, id(opacity): _C.MCMC_OPACITY}
    moved = [(p, st["exp_avg"] if st else None, st["exp_avg_sq"] if st else None, role_of.get(id(p), _C.MCMC_COPY)) for _, p, st in rows]
    for k, t in enumerate(extras):
        _check_param(t, f"extra tensor {k}", P)
        moved.append((t, None, None, _C.MCMC_COPY))
    if len(moved) > MAX_GROUPS:
        raise RuntimeError(f"fused_densify: {len(moved)} arrays to move, at most {MAX_GROUPS} per launch")
    return rows, P, dev, opacity, moved


def _mcmc_plan(P: int, dev: torch.device, opacity: torch.Tensor, dead_u8: Optional[torch.Tensor], min_opacity: float, n: int = 0):
    """gsrast_mcmc_plan and the read-back of its counts (the one synchronisation).  Returns (scratch, weights [P] int32, the four words,
    n_dead, n_alive, W)."""
    scratch = torch.empty(int(_C.lib().gsrast_mcmc_scratch_bytes(P, n)), dtype=torch.uint8, device=dev)
    weights = torch.empty(P, dtype=torch.int32, device=dev)
    counts_dev = torch.empty(4, dtype=torch.int32, device=dev)
    _C.launch("gsrast_mcmc_plan", dev, P, _C._ptr(opacity), _C._ptr(dead_u8), float(min_opacity), _C._ptr(weights), scratch.data_ptr(), counts_dev.data_ptr())
    host = [int(v) & 0xFFFFFFFF for v in counts_dev.cpu().tolist()]
    return scratch, weights, host, host[0], host[1], host[2] | (host[3] << 32)


def _mcmc_sample(P: int, n: int, dev: torch.device, scratch: torch.Tensor, generator, draws: Optional[torch.Tensor]) -> torch.Tensor:
    """n draws (torch.randint on the device unless given) -> src [n] int32."""
    if draws is None:
        draws = torch.randint(0, DRAW_RANGE, (n,), generator=generator, device=dev, dtype=torch.int64)
    else:
        if tuple(draws.shape) != (n,) or draws.dtype != torch.int64 or draws.device != dev:
            raise RuntimeError(f"fused_densify: draws must be int64 [{n}] on {dev} (got {draws.dtype} {tuple(draws.shape)} on {draws.device})")
        draws = draws.contiguous()
    src = torch.empty(n, dtype=torch.int32, device=dev)
    _C.launch("gsrast_mcmc_sample", dev, P, n, _C._ptr(draws), scratch.data_ptr(), _C._ptr(src), None)
    return src


def _check_min_opacity(min_opacity: float) -> float:
    if not 0.0 <= float(min_opacity) < 1.0:
        raise ValueError(f"min_opacity must be in [0, 1) (got {min_opacity})")
    return float(min_opacity)


@torch.no_grad()
def mcmc_relocate(opt, *, min_opacity: float = 0.005, dead_mask: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                  draws: Optional[torch.Tensor] = None, extras: Iterable[torch.Tensor] = (), names: Dict[str, str] = DEFAULT_NAMES) -> Dict[str, int]:
    """gsplat's relocate (strategy/ops.py) on `opt`'s per-Gaussian groups, in place: a row is dead where sigmoid(opacity) <= min_opacity or
    dead_mask (bool / uint8 [P]) is set; the j-th dead row in index order becomes a copy of an alive row sampled with probability
    proportional to its opacity, both get compute_relocation's opacity and scale for the number of copies, the sampled sources' Adam
    moments become zero and the dead rows keep theirs.  draws: int64 [n_dead] in [0, 2^62), drawn with torch.randint(..., generator=) on
    the device unless given.  extras: [P, ...] float32 tensors without moments, copied like any other group.  The parameters stay the
    same leaf objects and opt.state keeps its keys.  No dead row, or no alive row (where torch.multinomial would raise): nothing changes.
    Returns dict(n_dead, n_alive, n_relocated)."""
    min_opacity = _check_min_opacity(min_opacity)
    rows, P, dev, opacity, moved = _mcmc_moved(opt, names, extras)
    dead_u8 = _mask_u8(dead_mask, P, dev) if dead_mask is not None else None
    with _C._on_device(dev):
        scratch, _, host, n_dead, n_alive, _W = _mcmc_plan(P, dev, opacity, dead_u8, min_opacity)
        counts = dict(n_dead=n_dead, n_alive=n_alive, n_relocated=0)
        if n_dead == 0 or n_alive == 0:
            return counts
        src = _mcmc_sample(P, n_dead, dev, scratch, generator, draws)
        arr = (_C.DensifyGroupStruct * len(moved))()
        for a, (t, m, v, role) in zip(arr, moved):
            a.dst, a.dst_m, a.dst_v, a.width, a.role = _C._ptr(t), _C._ptr(m), _C._ptr(v), _rows_width(t), role
        _C.launch("gsrast_mcmc_relocate", dev, P, n_dead, _C._ptr(src), scratch.data_ptr(), (C.c_uint * 4)(*host), min_opacity, len(moved), arr)
    counts["n_relocated"] = n_dead
    return counts


@torch.no_grad()
def mcmc_grow(opt, *, cap_max: int, growth: float = 1.05, min_opacity: float = 0.005, generator: Optional[torch.Generator] = None,
              draws: Optional[torch.Tensor] = None, extras: Iterable[torch.Tensor] = (), names: Dict[str, str] = DEFAULT_NAMES):
    """gsplat's sample_add (strategy/ops.py): n = max(0, min(cap_max, int(growth * P)) - P) rows are appended, copies of rows sampled with
    probability proportional to opacity (every row: sample_add samples from opacities.flatten()); a sampled row and its copies get
    compute_relocation's opacity (clamped to [min_opacity, 1 - eps]) and scale.  The first P rows keep their moments, the new rows start
    from zero.  Every group's params[0] becomes a fresh leaf (as densify_and_prune installs them; GaussianAdam's step count goes on);
    n = 0 returns without installing anything.  draws: int64 [n] in [0, 2^62).  Returns (dict(n_added, P), {group name: parameter},
    [extras at the new P])."""
    min_opacity = _check_min_opacity(min_opacity)
    extras = list(extras)
    rows, P, dev, opacity, moved = _mcmc_moved(opt, names, extras)
    n = max(0, min(int(cap_max), int(float(growth) * P)) - P)
    if n == 0:
        return dict(n_added=0, P=P), {g.get("name"): p for g, p, _ in rows}, extras
    with _C._on_device(dev):
        scratch, _, host, _, _, W = _mcmc_plan(P, dev, opacity, None, 0.0, n)
        if W == 0:
            raise RuntimeError("fused_densify: mcmc_grow on a model whose every opacity is 0: nothing to sample from")
        src = _mcmc_sample(P, n, dev, scratch, generator, draws)
        arr = (_C.DensifyGroupStruct * len(moved))()
        out = []
        for a, (t, m, v, role) in zip(arr, moved):
            shape = (P + n,) + tuple(t.shape[1:])
            dst = torch.empty(shape, dtype=torch.float32, device=dev)
            dm = torch.empty(shape, dtype=torch.float32, device=dev) if m is not None else None
            dv = torch.empty(shape, dtype=torch.float32, device=dev) if v is not None else None
            a.src, a.src_m, a.src_v, a.dst, a.dst_m, a.dst_v = _C._ptr(t), _C._ptr(m), _C._ptr(v), _C._ptr(dst), _C._ptr(dm), _C._ptr(dv)
            a.width, a.role = _rows_width(t), role
            out.append((dst, dm, dv))
        _C.launch("gsrast_mcmc_grow", dev, P, n, _C._ptr(src), scratch.data_ptr(), (C.c_uint * 4)(*host), min_opacity, len(moved), arr)
    new = _install(opt, rows, out[: len(rows)])
    return dict(n_added=n, P=P + n), new, [r[0] for r in out[len(rows):]]


@torch.no_grad()
def mcmc_inject_noise(xyz: torch.Tensor, rotation: torch.Tensor, scaling: torch.Tensor, opacity: torch.Tensor, *, scale: float,
                      row_scale: Optional[torch.Tensor] = None, k: float = 100.0, x0: float = 0.995,
                      generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> None:
    """gsplat's inject_noise_to_position (strategy/ops.py), one launch, `xyz` updated in place:
      xyz += Sigma (noise * gate * scale [* row_scale]),  Sigma = R(q / |q|) diag(exp(scaling))^2 R^T,  gate = 1 / (1 + exp(-k ((1 - sigmoid(opacity)) - x0)))
    over the raw parameters xyz [P,3], rotation [P,4] (r, x, y, z), scaling [P,3], opacity [P,1].  scale: the caller's xyz_lr * noise_lr;
    row_scale [P]: a per-Gaussian factor on it (per-row learning rates).  noise [P,3]: torch.randn(..., generator=) on the device unless given."""
    P = int(xyz.shape[0])
    for t, name, w in ((xyz, "xyz", 3), (rotation, "rotation", 4), (scaling, "scaling", 3), (opacity, "opacity", 1)):
        _check_param(t, name, P)
        if _rows_width(t) != w:
            raise RuntimeError(f"fused_densify: {name} must have {w} floats per Gaussian (got {tuple(t.shape)})")
    dev = _C._require_gpu(xyz)
    if noise is None:
        noise = torch.randn((P, 3), generator=generator, device=dev, dtype=torch.float32)
    else:
        if tuple(noise.shape) != (P, 3) or noise.device != dev:
            raise RuntimeError(f"fused_densify: noise must be [{P}, 3] on {dev}, got {tuple(noise.shape)} on {noise.device}")
        noise = noise.to(torch.float32).contiguous()
    rs = _flat_f32(row_scale, "row_scale", P, dev) if row_scale is not None else None
    _C.launch("gsrast_mcmc_noise", dev, P, _C._ptr(xyz), _C._ptr(rotation), _C._ptr(scaling), _C._ptr(opacity), _C._ptr(noise), _C._ptr(rs),
            float(scale), float(k), float(x0))


def mcmc_refine(opt, *, cap_max: int, min_opacity: float = 0.005, growth: float = 1.05, generator: Optional[torch.Generator] = None,
                names: Dict[str, str] = DEFAULT_NAMES):
    """MCMCStrategy's refine step in gsplat's order: mcmc_relocate, then mcmc_grow (whose weights see the relocated opacities).
    Returns (dict(n_dead, n_alive, n_relocated, n_added, P), {group name: parameter})."""
    counts = mcmc_relocate(opt, min_opacity=min_opacity, generator=generator, names=names)
    grown, new, _ = mcmc_grow(opt, cap_max=cap_max, growth=growth, min_opacity=min_opacity, generator=generator, names=names)
    counts.update(grown)
    return counts, new
