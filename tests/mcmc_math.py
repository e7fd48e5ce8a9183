"""TEST INFRASTRUCTURE ONLY: fp64 restatement of the MCMC densification calls (include/gsrast.h: gsrast_mcmc_*), written from the
formulas the header states, not from the kernels:

  weights()      q_i = 0 for a dead row (sigmoid(opacity) <= min_opacity, or the mask), else max(1, floor(sigmoid(opacity) * 2^24))
  sample()       draw d in [0, 2^62) targets t = floor(d * W / 2^62) and selects the smallest i whose inclusive prefix of q exceeds t --
                 Python integers and bisect; sample_brute() is the same rule as a linear walk
  relocation()   gsplat's compute_relocation (N_MAX = 51): r = min(count + 1, 51), o' = 1 - (1 - o)^(1/r),
                 denom = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1), scale factor o / denom -- the double loop as
                 written, vectorised over the sources; relocation_literal() is the scalar transcription
  relocate()     the j-th dead row in index order becomes row src[j]; sources and copies take the new opacity / scaling; the sources'
                 moments become zero, the dead rows keep theirs
  grow()         rows [0, P) with the sources updated, then one copy of the updated row src[j] per draw with zero moments
  noise()        xyz + R diag(exp(s))^2 R^T (noise * gate * scale [* row_scale]); noise_gsplat() is gsplat's inject_noise_to_position
                 spelled with explicit covariances and einsum
"""
import bisect
import math

import numpy as np
import torch

import densify_math as dm

N_MAX = 51
Q_ONE = 1 << 24
DRAW_RANGE = 1 << 62
EPS32 = float(np.finfo(np.float32).eps)


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x.double()))


def weights(opacity_logit, min_opacity, dead_mask=None):
    """(q int64 [P], dead bool [P]) from the fp64 sigmoid."""
    o = sigmoid(opacity_logit).reshape(-1)
    dead = o <= min_opacity
    if dead_mask is not None:
        dead = dead | dead_mask.reshape(-1).bool()
    q = torch.clamp(torch.floor(o * Q_ONE).long(), min=1)
    q[dead] = 0
    return q, dead


def target(d, W):
    return (int(d) * int(W)) >> 62


def sample(q, draws):
    """(src list, count list) with Python integers.  q: any sequence of non-negative ints with a positive sum."""
    q = [int(v) for v in q]
    cum, run = [], 0
    for v in q:
        run += v
        cum.append(run)
    W = run
    src, count = [], [0] * len(q)
    for d in draws:
        i = bisect.bisect_right(cum, target(d, W))      # the first index whose inclusive prefix is > t
        src.append(i)
        count[i] += 1
    return src, count


def sample_brute(q, t):
    run = 0
    for i, v in enumerate(q):
        run += int(v)
        if run > t:
            return i
    raise ValueError("t is not below the total weight")


def relocation_literal(o, count):
    """One source, plain Python floats: (o', o / denom)."""
    r = min(int(count) + 1, N_MAX)
    on = 1.0 - (1.0 - o) ** (1.0 / r)
    denom = 0.0
    for i in range(1, r + 1):
        for k in range(i):
            denom += math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * on ** (k + 1)
    return on, o / denom


def relocation(o, count):
    """fp64 arrays over the sources: (o' unclamped, o / denom)."""
    o = np.asarray(o, dtype=np.float64)
    r = np.minimum(np.asarray(count, dtype=np.int64) + 1, N_MAX)
    on = 1.0 - (1.0 - o) ** (1.0 / r)
    denom = np.zeros_like(o)
    power = [on ** (k + 1) for k in range(int(r.max(initial=1)))]
    for i in range(1, N_MAX + 1):
        live = i <= r
        if not live.any():
            break
        for k in range(i):
            denom += np.where(live, math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * power[k], 0.0)
    return on, o / denom


def new_values(opacity_logit, scaling, count, min_opacity):
    """(sources idx, new opacity logit [n_src], new log-scale [n_src, 3]) in fp64, from the pre-call values."""
    count = torch.as_tensor(count, dtype=torch.long)
    idx = torch.nonzero(count > 0).reshape(-1)
    o = sigmoid(opacity_logit).reshape(-1)[idx]
    on, coeff = relocation(o.numpy(), count[idx].numpy())
    on = torch.from_numpy(np.clip(on, min_opacity, 1.0 - EPS32))
    new_logit = torch.log(on / (1.0 - on))
    new_scale = torch.log(torch.from_numpy(coeff)[:, None] * torch.exp(scaling.double()[idx]))
    return idx, new_logit, new_scale


def _updated(params, count, min_opacity):
    out = {k: v.double().clone() for k, v in params.items()}
    idx, lo, ls = new_values(params["opacity"], params["scaling"], count, min_opacity)
    out["opacity"][idx] = lo.reshape(-1, 1)
    out["scaling"][idx] = ls
    return out, idx


def relocate(params, moments, dead, src, count, min_opacity):
    """name -> (param, exp_avg, exp_avg_sq) in fp64 (moments None: (param, None, None)); src: one source per dead row, in index order."""
    out, idx = _updated(params, count, min_opacity)
    dead_idx = torch.nonzero(dead).reshape(-1)
    src = torch.as_tensor(src, dtype=torch.long)
    assert src.numel() == dead_idx.numel()
    res = {}
    for k, v in out.items():
        v[dead_idx] = v[src]
        mv = (None, None)
        if moments is not None:
            mv = tuple(m.double().clone() for m in moments[k])
            for m in mv:
                m[idx] = 0.0
        res[k] = (v,) + mv
    return res


def grow(params, moments, src, count, min_opacity):
    out, _ = _updated(params, count, min_opacity)
    src = torch.as_tensor(src, dtype=torch.long)
    res = {}
    for k, v in out.items():
        mv = (None, None)
        if moments is not None:
            mv = tuple(torch.cat((m.double(), torch.zeros((src.numel(),) + tuple(m.shape[1:]), dtype=torch.float64)), 0) for m in moments[k])
        res[k] = (torch.cat((v, v[src]), 0),) + mv
    return res


def gate(opacity_logit, k=100.0, x0=0.995):
    return 1.0 / (1.0 + torch.exp(-k * ((1.0 - sigmoid(opacity_logit).reshape(-1)) - x0)))


def noise(xyz, rotation, scaling, opacity_logit, eps, scale, row_scale=None, k=100.0, x0=0.995):
    R = dm.rotation_matrix(rotation.double())
    v = eps.double() * (gate(opacity_logit, k, x0) * scale)[:, None]
    if row_scale is not None:
        v = v * row_scale.double().reshape(-1, 1)
    Rt = R.transpose(1, 2)
    t = dm.rotate(Rt, v) * torch.exp(scaling.double()) ** 2
    return xyz.double() + dm.rotate(R, t)


def noise_gsplat(xyz, rotation, scaling, opacity_logit, eps, scale, k=100.0, x0=0.995):
    """inject_noise_to_position: covars = R S S^T R^T (quat_scale_to_covar_preci), noise = einsum("bij,bj->bi", covars, noise * op_sigmoid * scaler)."""
    q = rotation.double()
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * torch.exp(scaling.double())[:, None, :]
    covars = torch.bmm(M, M.transpose(1, 2))
    opacities = torch.sigmoid(opacity_logit.double().reshape(-1))
    op_sigmoid = 1.0 / (1.0 + torch.exp(-k * ((1.0 - opacities) - x0)))
    n = eps.double() * op_sigmoid[:, None] * scale
    return xyz.double() + torch.einsum("bij,bj->bi", covars, n)
