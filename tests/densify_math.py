"""TEST INFRASTRUCTURE ONLY: torch-CPU restatement of the reference's densification (densify_pruneclone: clone, split, prune, with the
optimizer surgery that goes with each), written twice from the behaviour the project documents (include/gsrast.h):

  sequential()   the reference's ORDER of operations on a real torch.optim.Adam: append the clones (cat, moments get zeros), append N
                 copies of every split source, remove the sources, then prune by a flag the copies inherit -- index and cat operations.
  closed_form()  the layout rule: [ originals !split && !pruned | clones | split copy 0 | ... | copy N-1 ], noise rows ranked over ALL
                 split-selected sources.

Both work in the dtype (sequential(): and on the device) of their inputs (fp32 for the exact host comparison, fp64 as the GPU tests' truth) and share the elementwise
helpers below, so that equal inputs give equal bits.  tests/test_densify_host.py holds them against each other.
"""
import math

import torch

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "temporal_pos")


def shapes(M=16):
    """The seven per-Gaussian groups (tests/test_adam.py::SHAPES is M = 16)."""
    return {"xyz": (3,), "f_dc": (1, 3), "f_rest": (M - 1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "temporal_pos": (1,)}


def rotation_matrix(q):
    """Rows (r, x, y, z), normalised here; [n, 3, 3]."""
    q = q / torch.sqrt((q * q).sum(1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.shape[0], 3, 3), dtype=q.dtype, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def rotate(R, s):
    """R s per row, spelled elementwise (a batched matmul may sum in another order for another batch size)."""
    return torch.stack([R[:, c, 0] * s[:, 0] + R[:, c, 1] * s[:, 1] + R[:, c, 2] * s[:, 2] for c in range(3)], 1)


def split_xyz(xyz, rotation, scaling, noise):
    return xyz + rotate(rotation_matrix(rotation), noise * torch.exp(scaling))


def split_scaling(scaling, N):
    return torch.log(torch.exp(scaling) / (0.8 * N))


def criterion(accum, denom, grad_scale, thr):
    g = accum.reshape(-1) / denom.reshape(-1)
    g[g.isnan()] = 0.0
    if grad_scale is not None:
        g = g * grad_scale.reshape(-1)
    return g, ((g >= thr) if math.isfinite(thr) else torch.zeros_like(g, dtype=torch.bool))


def classify(params, accum, denom, *, thr, tau, min_opacity=None, prune_mask=None, grad_scale=None):
    """(clone, split_all, pruned) bool [P]; clone / split_all BEFORE the prune is applied."""
    P = params["xyz"].shape[0]
    _, sel = criterion(accum, denom, grad_scale, thr)
    dev = params["xyz"].device
    smax = torch.exp(params["scaling"]).max(1).values if P else torch.zeros(0, dtype=params["scaling"].dtype, device=dev)
    pruned = torch.zeros(P, dtype=torch.bool, device=dev) if prune_mask is None else prune_mask.reshape(-1).bool().clone()
    if min_opacity is not None and min_opacity > 0:
        pruned |= torch.sigmoid(params["opacity"]).reshape(-1) < min_opacity
    return sel & (smax <= tau), sel & (smax > tau), pruned


# ---- (a) sequential, on a real optimizer -------------------------------------------------------------------------------------
def make_adam(params, moments):
    """torch.optim.Adam over copies of `params` (name -> [P, ...]) with its state set to `moments` (name -> (exp_avg, exp_avg_sq))."""
    leaves = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
    opt = torch.optim.Adam([{"params": [leaves[k]], "lr": 0.0, "name": k} for k in params], lr=0.0, eps=1e-15)
    for k, p in leaves.items():
        if moments is not None:
            opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    return opt


def _cat(opt, new):
    for g in opt.param_groups:
        p, ext = g["params"][0], new[g["name"]]
        st = opt.state.pop(p, None)
        q = torch.nn.Parameter(torch.cat((p.detach(), ext), 0))
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), 0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), 0)
            opt.state[q] = st
        g["params"][0] = q


def _keep(opt, valid):
    for g in opt.param_groups:
        p = g["params"][0]
        st = opt.state.pop(p, None)
        q = torch.nn.Parameter(p.detach()[valid])
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][valid], st["exp_avg_sq"][valid]
            opt.state[q] = st
        g["params"][0] = q


def _cur(opt):
    return {g["name"]: g["params"][0].detach() for g in opt.param_groups}


def sequential(opt, accum, denom, noise, *, thr, tau, N=2, min_opacity=None, prune_mask=None, grad_scale=None):
    """Clone, split, remove the sources, prune -- in that order, in place on `opt`.  noise: [N * (number of split-selected), 3].
    Returns the number of rows left."""
    P = _cur(opt)["xyz"].shape[0]
    dt = _cur(opt)["xyz"].dtype
    g, sel = criterion(accum, denom, grad_scale, thr)
    dev = _cur(opt)["xyz"].device
    flag = torch.zeros(P, dtype=torch.bool, device=dev) if prune_mask is None else prune_mask.reshape(-1).bool().clone()      # travels with its row
    # clone
    cur = _cur(opt)
    mask = sel & (torch.exp(cur["scaling"]).max(1).values <= tau) if P else sel
    _cat(opt, {k: v[mask] for k, v in cur.items()})
    flag = torch.cat((flag, flag[mask]))
    # split: the appended clones carry a zero gradient
    cur = _cur(opt)
    n_init = cur["xyz"].shape[0]
    padded = torch.zeros(n_init, dtype=dt, device=dev)
    padded[:P] = g
    mask = ((padded >= thr) if math.isfinite(thr) else torch.zeros(n_init, dtype=torch.bool, device=dev))
    if n_init:
        mask = mask & (torch.exp(cur["scaling"]).max(1).values > tau)
    n_sel = int(mask.sum())
    assert noise.shape[0] == N * n_sel, (noise.shape, N, n_sel)
    new = {k: v[mask].repeat((N,) + (1,) * (v.dim() - 1)) for k, v in cur.items()}
    new["xyz"] = split_xyz(new["xyz"], new["rotation"], new["scaling"], noise.to(dt).reshape(N * n_sel, 3))
    new["scaling"] = split_scaling(new["scaling"], N)
    _cat(opt, new)
    flag = torch.cat((flag, flag[mask].repeat(N)))
    gone = torch.cat((mask, torch.zeros(N * n_sel, dtype=torch.bool, device=dev)))
    _keep(opt, ~gone)
    flag = flag[~gone]
    # prune
    if min_opacity is not None and min_opacity > 0:
        flag = flag | (torch.sigmoid(_cur(opt)["opacity"]).reshape(-1) < min_opacity)
    _keep(opt, ~flag)
    return _cur(opt)["xyz"].shape[0]


def optimizer_rows(opt):
    """name -> (param, exp_avg or None, exp_avg_sq or None)."""
    out = {}
    for g in opt.param_groups:
        p = g["params"][0]
        st = opt.state.get(p)
        out[g["name"]] = (p.detach(), st["exp_avg"] if st else None, st["exp_avg_sq"] if st else None)
    return out


# ---- (b) closed form ---------------------------------------------------------------------------------------------------------
def closed_form(params, moments, accum, denom, noise, *, thr, tau, N=2, min_opacity=None, prune_mask=None, grad_scale=None):
    """Returns (counts, name -> (param, exp_avg, exp_avg_sq), parts): counts = dict(n_kept, n_clone, n_split, n_split_all, P);
    parts = dict(kept, clone, split: source indices; n_new: rows that are not kept originals)."""
    clone, split_all, pruned = classify(params, accum, denom, thr=thr, tau=tau, min_opacity=min_opacity, prune_mask=prune_mask, grad_scale=grad_scale)
    kept_i = torch.nonzero(~split_all & ~pruned).reshape(-1)
    clone_i = torch.nonzero(clone & ~pruned).reshape(-1)
    split_i = torch.nonzero(split_all & ~pruned).reshape(-1)
    n_all = int(split_all.sum())
    rank_all = torch.cumsum(split_all.long(), 0) - 1
    assert noise.shape[0] == N * n_all, (noise.shape, N, n_all)
    out = {}
    for k, v in params.items():
        parts = [v[kept_i], v[clone_i]]
        for c in range(N):
            rows = v[split_i]
            if k == "xyz":
                rows = split_xyz(rows, params["rotation"][split_i], params["scaling"][split_i], noise.to(v.dtype)[c * n_all + rank_all[split_i]])
            elif k == "scaling":
                rows = split_scaling(rows, N)
            parts.append(rows)
        p = torch.cat(parts, 0)
        mv = (None, None)
        if moments is not None:
            n_new = p.shape[0] - kept_i.numel()
            mv = tuple(torch.cat((m[kept_i], torch.zeros((n_new,) + tuple(m.shape[1:]), dtype=m.dtype)), 0) for m in moments[k])
        out[k] = (p,) + mv
    counts = dict(n_kept=kept_i.numel(), n_clone=clone_i.numel(), n_split=split_i.numel(), n_split_all=n_all,
                  P=kept_i.numel() + clone_i.numel() + N * split_i.numel())
    return counts, out, dict(kept=kept_i, clone=clone_i, split=split_i)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
MIXES = ("mixed", "none", "all_clone", "all_split", "all_pruned", "overlap")
THR, TAU, MIN_OPACITY = 2e-4, 0.05, 0.005


def draw(P, M, mix, seed, with_moments=True):
    """Inputs whose g, max exp(scaling) and sigmoid(opacity) all lie well clear (>= 5 %) of their thresholds, so that fp32 and fp64
    classify alike -- by construction, nothing is redrawn or left out.  mix: which classes occur.  Returns a dict of fp32 tensors."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    sh = shapes(M)
    params = {k: n(P, *s) for k, s in sh.items()}
    sel_p, big_p, prune_p = dict(mixed=(0.3, 0.4, 0.2), none=(0.0, 0.5, 0.0), all_clone=(1.0, 0.0, 0.0), all_split=(1.0, 1.0, 0.0),
                                 all_pruned=(0.3, 0.4, 1.0), overlap=(0.7, 0.6, 0.6))[mix]
    sel, big, low = u(P) < sel_p, u(P) < big_p, u(P) < prune_p * 0.5
    mask = u(P) < prune_p * 0.5 if prune_p < 1.0 else torch.ones(P, dtype=torch.bool)
    # g = accum / denom: selected 1.05 ... 3 x thr, others 0 ... 0.95 x thr; a tenth of the rows never seen (0 / 0 = NaN -> 0)
    denom = torch.floor(1 + 6 * u(P))
    g = torch.where(sel, THR * (1.05 + 1.95 * u(P)), THR * 0.95 * u(P))
    unseen = (u(P) < 0.1) & ~sel
    denom[unseen] = 0.0
    accum = g * denom
    # scaling: the largest component's exp is 1.05 ... 4 x tau (big) or 0.2 ... 0.95 x tau; the other two are smaller
    top = torch.where(big, TAU * (1.05 + 2.95 * u(P)), TAU * (0.2 + 0.75 * u(P)))
    s = top[:, None] * (0.1 + 0.9 * u(P, 3))
    if P:
        s[torch.arange(P), torch.randint(0, 3, (P,), generator=gen)] = top
    params["scaling"] = torch.log(s)
    # opacity: sigmoid 0.05 ... 0.5 x min_opacity (pruned by opacity) or 2 x min_opacity ... 0.99
    o = torch.where(low, MIN_OPACITY * (0.05 + 0.45 * u(P)), 2 * MIN_OPACITY + (0.99 - 2 * MIN_OPACITY) * u(P))
    params["opacity"] = torch.log(o / (1 - o)).reshape(P, 1)
    moments = {k: (n(P, *sh[k]) * 1e-3, u(P, *sh[k]) * 1e-5) for k in sh} if with_moments else None
    grad_scale = 1.0 + 0.02 * u(P) if mix != "mixed" else None     # (inv_intergral_fordensify; at most 2 %: the margins above hold with it)
    return dict(params=params, moments=moments, accum=accum.reshape(P, 1), denom=denom.reshape(P, 1), prune_mask=mask, grad_scale=grad_scale,
                kw=dict(thr=THR, tau=TAU, min_opacity=MIN_OPACITY))


def margins_ok(d, rel=1e-3):
    """No g, max exp(scaling), sigmoid(opacity) within `rel` relative of its threshold (fp64)."""
    g, _ = criterion(d["accum"].double(), d["denom"].double(), None if d["grad_scale"] is None else d["grad_scale"].double(), THR)
    smax = torch.exp(d["params"]["scaling"].double()).max(1).values if g.numel() else g
    o = torch.sigmoid(d["params"]["opacity"].double()).reshape(-1)
    far = lambda x, t: bool(((x - t).abs() > rel * t).all())  # noqa: E731
    return far(g, THR) and far(smax, TAU) and far(o, MIN_OPACITY)
