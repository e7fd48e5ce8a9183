"""TEST INFRASTRUCTURE ONLY: the temporal lifespan (include/gsrast.h: gsrast_temporal_*) restated in numpy fp64 from its formulas -- the gate
forward with its analytic backward, the time embedding, Eq. 22's integral with its mask, `inv` and statistics, and the eval-time select --
and the same ops as a torch composition (`torch_gate`, `torch_integral`; any dtype and device) for torch.autograd to differentiate.

    L = (1 - ms) (1 - head) + ms;   c = center or sigmoid(center);   d = t - c;   u = d / L;   state = exp(-4 u^2)
    time_emb = [d, sin d, cos d, sin 2d, cos 2d, ..., sin 2^(m-1) d, cos 2^(m-1) d]
    Q(x) = 1 / (1 + exp(-(a1 x^3 + a2 x)));   I = L sqrt(pi)/2 (Q(2 sqrt2 (end - c) / L) - Q(2 sqrt2 (start - c) / L))
"""
import numpy as np

A1, A2 = 0.070565902, 1.5976
FIXED_ROWS = ("head0", "head1", "center_t", "center_m5", "center_40")


def make_case(P, t, seed):
    """head ~ U(0,1), center ~ U(-0.2, 1.2), upstream gradients ~ N(0,1), fp32 [P]; the LAST rows (as many as fit) are fixed: head 0, head 1,
    center = t (state 1, embedding [0, 0, 1, 0, 1, ...] exactly), center = -5 and center = 40 (the state underflows).  Returns (dict, {name: row})."""
    rng = np.random.default_rng(seed)
    c = dict(head=rng.uniform(0, 1, P), center=rng.uniform(-0.2, 1.2, P), d_lifespan=rng.standard_normal(P), d_state=rng.standard_normal(P))
    rows = {}
    for k, name in enumerate(FIXED_ROWS):
        i = P - 1 - k
        if i < 0:
            break
        rows[name] = i
        if name == "head0":
            c["head"][i] = 0.0
        elif name == "head1":
            c["head"][i] = 1.0
        else:
            c["center"][i] = {"center_t": t, "center_m5": -5.0, "center_40": 40.0}[name]
    return {k: v.astype(np.float32) for k, v in c.items()}, rows


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def embed(d, multires):
    """[P, 2 multires + 1]: the input, then sin and cos of it at the exact powers of two 1 ... 2^(multires-1), sin before cos."""
    d = np.asarray(d, np.float64).reshape(-1)
    cols = [d]
    for k in range(multires):
        cols += [np.sin(d * 2.0 ** k), np.cos(d * 2.0 ** k)]
    return np.stack(cols, 1)


def gate(head, center, t, min_scale, multires=4, sigmoid_center=False, d_lifespan=None, d_state=None, threshold=0.001):
    """dict(lifespan, state, time_emb, dead, d_head, d_center) in fp64 ([P] each, time_emb [P, 2 multires + 1]); a missing upstream is 0."""
    head, center = np.asarray(head, np.float64).reshape(-1), np.asarray(center, np.float64).reshape(-1)
    ms = float(min_scale)
    c = _sigmoid(center) if sigmoid_center else center
    L = (1.0 - ms) * (1.0 - head) + ms
    d = float(t) - c
    u = d / L
    with np.errstate(under="ignore"):
        state = np.exp(-4.0 * u * u)
    dl = np.zeros_like(L) if d_lifespan is None else np.asarray(d_lifespan, np.float64).reshape(-1)
    ds = np.zeros_like(L) if d_state is None else np.asarray(d_state, np.float64).reshape(-1)
    g_d = ds * (-8.0 * u * state / L)
    g_L = dl + ds * (8.0 * u * u * state / L)
    d_center = -g_d * (c * (1.0 - c) if sigmoid_center else 1.0)
    return dict(lifespan=L, state=state, time_emb=embed(d, multires), dead=~(state > threshold), d_head=-(1.0 - ms) * g_L, d_center=d_center)


def Q(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-(A1 * x ** 3 + A2 * x)))


def Q_reference_form(x):
    """1 - 1 / (1 + e^z): the same number, cancelled to 0 where e^z < 2^-53."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 - 1.0 / (1.0 + np.exp(A1 * x ** 3 + A2 * x))


def integral(head, center, min_scale, sigmoid_center=False, start=0.0, end=1.0):
    head, center = np.asarray(head, np.float64).reshape(-1), np.asarray(center, np.float64).reshape(-1)
    ms = float(min_scale)
    c = _sigmoid(center) if sigmoid_center else center
    L = (1.0 - ms) * (1.0 - head) + ms
    k = 2.0 * np.sqrt(2.0)
    return L * (np.sqrt(np.pi) / 2.0) * (Q(k * (end - c) / L) - Q(k * (start - c) / L))


def integral_outputs(I, min_integral):
    """(dead bool [P], inv [P], (I_max, n_valid)) from integrals I: inv = I_max / I on a valid row, 0 on a dead one; no valid row: I_max = 0."""
    I = np.asarray(I, np.float64).reshape(-1)
    dead = ~(I > min_integral)
    imax = float(I[~dead].max()) if (~dead).any() else 0.0
    inv = np.zeros_like(I)
    inv[~dead] = imax / I[~dead]
    return dead, inv, (imax, int((~dead).sum()))


def select(state, tensors, threshold=0.001):
    """(count, [t[alive] for t in tensors]) with alive = state > threshold, in index order."""
    alive = np.asarray(state).reshape(-1) > threshold
    return int(alive.sum()), [np.asarray(x)[alive] for x in tensors]


# ---- the same ops as torch compositions (the reference's own op order: scene/saro_gaussian.py get_deformation / get_intergral) ----
def torch_embed(d, multires):
    import torch
    cols = [d]
    for k in range(multires):
        cols += [torch.sin(d * 2.0 ** k), torch.cos(d * 2.0 ** k)]
    return torch.cat(cols, -1)


def torch_gate(head, center, t, min_scale, multires=4, sigmoid_center=False):
    """(lifespan, state, time_emb) of [P,1] tensors `head`, `center`."""
    import torch
    lifespan = 1 - head
    lifespan = (1 - min_scale) * lifespan + min_scale
    distance = t - (torch.sigmoid(center) if sigmoid_center else center)
    state = torch.exp(-4 * (distance / lifespan) ** 2)
    return lifespan, state, torch_embed(distance, multires).detach()


def torch_integral(head, center, min_scale, sigmoid_center=False, start=0.0, end=1.0):
    import torch
    lifespan = (1 - min_scale) * (1 - head) + min_scale
    c = torch.sigmoid(center) if sigmoid_center else center
    q = lambda x: 1 / (1 + torch.exp(-(A1 * x ** 3 + A2 * x)))  # noqa: E731
    p1, p2 = q(2 * np.sqrt(2) * (end - c) / lifespan), q(2 * np.sqrt(2) * (start - c) / lifespan)
    return lifespan * np.sqrt(np.pi) / 2 * (p1 - p2)
