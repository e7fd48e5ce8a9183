"""The bf16 path of the fused 3-layer head (csrc/gsrast_mlp_bf16.h) restated in numpy: the rounding model of that header, with the
accumulation of every sum selectable.  The yardstick of tests/test_mlp_bf16_host.py (held against torch.autograd there) and
tests/test_gpu_mlp_bf16.py.

    x~ = bf([x | x_tail])    W~k = bf(Wk)    biases fp32
    a1 = W~1 x~ + b1     h~1 = bf(relu(a1))
    a2 = W~2 h~1 + b2    h~2 = bf(relu(a2))
    y  = W~3 h~2 + b3, or its sigmoid

    g3 = dy, or dy y (1 - y)         g~3 = bf(g3)    dW3 = sum_rows g~3 (x) h~2    db3 = sum_rows g3
    g2 = (W~3^T g~3) [a2 > 0]        g~2 = bf(g2)    dW2 = sum_rows g~2 (x) h~1    db2 = sum_rows g2
    g1 = (W~2^T g~2) [a1 > 0]        g~1 = bf(g1)    dW1 = sum_rows g~1 (x) x~     db1 = sum_rows g1      dx = (W~1^T g~1)[:, :D_x]

bf(.) rounds to bfloat16, to nearest, ties to even; products are bf16 x bf16 (exact in fp32); a1, a2, y and g1, g2, g3 are fp32 values.
`acc` chooses how the sums over k run:
    "fp64"   every dot product in fp64, rounded to fp32 once (with its bias); weight gradients left in fp64
    "fp32"   an fp32 chain per dot product in the k order `order` gives (None: natural, "reversed", or a numpy Generator: a random
             permutation per product); weight gradients as fp32 chains over at most 512 rows in that order, the chains' sums added in fp64
Bias gradients are fp64 sums of the unrounded g either way."""
import numpy as np

NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")
CHAIN = 512      # rows: the longest fp32 chain of a weight gradient


def bf(a):
    """fp32 -> bfloat16, round to nearest even, as fp32 values.  +-0, +-Inf stay; a NaN stays a NaN (quiet)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(a), (u.astype(np.uint32) | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r)
    return r.view(np.float32).reshape(a.shape)


def truncate(a):
    """fp32 -> bfloat16 by dropping the low 16 bits: a WRONG rounding, for showing that a test tells it from bf."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(a.shape)


def _perm(order, k):
    if order is None:
        return np.arange(k)
    if isinstance(order, str):
        assert order == "reversed", order
        return np.arange(k)[::-1]
    return order.permutation(k)


def _dot(A, B, acc, order):
    """A [n, k] . B [k, m], both fp32 holding bf16 values -> fp64 (acc "fp64") or the fp32 chain's result."""
    if acc == "fp64":
        return A.astype(np.float64) @ B.astype(np.float64)
    assert acc == "fp32", acc
    out = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in _perm(order, A.shape[1]):
        out += A[:, k:k + 1] * B[k:k + 1, :]      # (the product of two bf16 values is exact in fp32: one rounding per step, as an fmaf)
    return out


def _wgrad(G, H, acc, order):
    """sum over rows of G[row] (x) H[row] -> [G's width, H's width] fp64."""
    if acc == "fp64":
        return G.astype(np.float64).T @ H.astype(np.float64)
    n = G.shape[0]
    total = np.zeros((G.shape[1], H.shape[1]), np.float64)
    if n == 0:
        return total
    rows = _perm(order, n)
    n_chains = -(-n // CHAIN)
    pad = n_chains * CHAIN - n
    Gc = np.concatenate((G[rows], np.zeros((pad, G.shape[1]), np.float32))).reshape(n_chains, CHAIN, -1)
    Hc = np.concatenate((H[rows], np.zeros((pad, H.shape[1]), np.float32))).reshape(n_chains, CHAIN, -1)
    part = np.zeros((n_chains, G.shape[1], H.shape[1]), np.float32)
    for k in range(CHAIN):
        part += Gc[:, k, :, None] * Hc[:, k, None, :]
    for c in range(n_chains):
        total += part[c].astype(np.float64)
    return total


def forward_backward(x, w1, b1, w2, b2, w3, b3, dy, x_tail=None, sigmoid=False, acc="fp64", order=None, rounding=bf, keep=False):
    """dict of y and the seven gradients (fp64 arrays holding the model's values); keep: the intermediates too."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    x, w1, b1, w2, b2, w3, b3, dy = (f32(a) for a in (x, w1, b1, w2, b2, w3, b3, dy))
    xin = x if x_tail is None else np.concatenate((x, f32(x_tail)), axis=1)
    d_x = x.shape[1]
    xt, w1t, w2t, w3t = rounding(xin), rounding(w1), rounding(w2), rounding(w3)

    def affine(A, Wt, b):      # fp32 (A Wt^T + b)
        s = _dot(A, Wt.T, acc, order)
        return (s + b.astype(np.float64)).astype(np.float32) if acc == "fp64" else s + b

    a1 = affine(xt, w1t, b1)
    h1t = rounding(np.where(a1 < 0, np.float32(0), a1))      # (a NaN stays a NaN through the ReLU)
    a2 = affine(h1t, w2t, b2)
    h2t = rounding(np.where(a2 < 0, np.float32(0), a2))
    z = affine(h2t, w3t, b3)
    with np.errstate(over="ignore"):
        y = 1.0 / (1.0 + np.exp(-z.astype(np.float64))) if sigmoid else z.astype(np.float64)
    g3 = (dy.astype(np.float64) * y * (1.0 - y)).astype(np.float32) if sigmoid else dy
    g3t = rounding(g3)
    g2 = (_dot(g3t, w3t, acc, order) * (a2 > 0)).astype(np.float32)
    g2t = rounding(g2)
    g1 = (_dot(g2t, w2t, acc, order) * (a1 > 0)).astype(np.float32)
    g1t = rounding(g1)
    out = dict(y=y, dx=_dot(g1t, w1t, acc, order)[:, :d_x].astype(np.float64),
               dw1=_wgrad(g1t, xt, acc, order), db1=g1.astype(np.float64).sum(axis=0),
               dw2=_wgrad(g2t, h1t, acc, order), db2=g2.astype(np.float64).sum(axis=0),
               dw3=_wgrad(g3t, h2t, acc, order), db3=g3.astype(np.float64).sum(axis=0))
    if keep:
        out.update(xin=xin, xt=xt, a1=a1, h1t=h1t, a2=a2, h2t=h2t, g3=g3, g2=g2, g1=g1)
    return out


# ---- the exact cases: every product and partial sum representable in fp32, so no summation order and no accumulator width can show ----
_GRID = dict(xin=9, xt=9, a1=10, h1t=10, a2=11, h2t=11, y=12, g3=1, g2=2, g1=3, dx=4, dw1=12, dw2=12, dw3=12, db1=3, db2=2, db3=1)
_dyadic_cache = {}


def make_dyadic_case(d_x, d_tail, h1, h2, d_out, n, seed=0):
    """x = integers in [-2^9, 2^9] / 2^9, weights in {+-1, +-1/2} with one in four non-zero, biases and dy in {+-1, +-1/2}; no Sigmoid.
    Returns (inputs, model outputs); asserts what makes the case exact: the fp64 model, the fp32 model and the fp32 model in reversed k
    order agree bit for bit, every tensor T on its grid 2^-g has max|T| 2^g < 2^24, and (D_in >= 8) rounding changes at least 10 % of
    h~1 and of h~2 -- a case that rounds nothing would not tell bf16 from fp32."""
    key = (d_x, d_tail, h1, h2, d_out, n, seed)
    if key in _dyadic_cache:
        return _dyadic_cache[key]
    rng = np.random.default_rng(seed)
    d_in = d_x + d_tail
    half = lambda shape: (rng.choice([-1.0, -0.5, 0.5, 1.0], size=shape)).astype(np.float32)  # noqa: E731
    sparse = lambda shape: (half(shape) * (rng.integers(0, 4, size=shape) == 0)).astype(np.float32)  # noqa: E731
    xin = (rng.integers(-512, 513, size=(n, d_in)) / 512.0).astype(np.float32)
    c = dict(x=np.ascontiguousarray(xin[:, :d_x]), x_tail=np.ascontiguousarray(xin[:, d_x:]) if d_tail else None,
             w1=sparse((h1, d_in)), b1=half((h1,)), w2=sparse((h2, h1)), b2=half((h2,)), w3=sparse((d_out, h2)), b3=half((d_out,)),
             dy=half((n, d_out)))
    args = (c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], False)
    m64 = forward_backward(*args, acc="fp64", keep=True)
    m32 = forward_backward(*args, acc="fp32", keep=True)
    m32r = forward_backward(*args, acc="fp32", order="reversed", keep=True)
    for k, g in _GRID.items():
        v = np.asarray(m64[k], np.float64)
        assert np.array_equal(v, np.asarray(m32[k], np.float64)) and np.array_equal(v, np.asarray(m32r[k], np.float64)), (key, k)
        scaled = v * 2.0 ** g
        assert np.array_equal(scaled, np.round(scaled)) and float(np.abs(scaled).max(initial=0.0)) < 2.0 ** 24, (key, k)
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), (key, k)
    if d_in >= 8 and n > 0:
        for k, pre in (("h1t", "a1"), ("h2t", "a2")):
            changed = float(np.mean(m64[k] != np.maximum(m64[pre], 0)))
            assert changed >= 0.10, (key, k, changed)
    for d in (c, m64):
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
    _dyadic_cache[key] = (c, m64)
    return _dyadic_cache[key]
