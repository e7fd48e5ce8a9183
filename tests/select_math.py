"""TEST INFRASTRUCTURE ONLY: the differentiable row selection (fused_densify.RowSelection; include/gsrast.h: gsrast_densify_apply over COPY
groups and gsrast_densify_scatter) restated in numpy.  With keep a bool [P] of n True entries, in index order:

    gather(x)  = x[keep]                         [P, ...] -> [n, ...]
    scatter(y) = z, z[keep] = y, z = +0 else     [n, ...] -> [P, ...]

Both are linear and each is the other's transpose, so the vector-Jacobian product of one is the other applied to the upstream gradient.
"""
import numpy as np

PATTERNS = ("all", "none", "alternating", "runs300", "random", "first", "last")


def pattern(name, P, seed=0):
    """bool [P]: which rows are kept."""
    i = np.arange(P)
    if name == "random":
        return np.random.default_rng(seed).random(P) < 0.5
    return dict(all=i >= 0, none=i < 0, alternating=i % 2 == 0, runs300=(i // 300) % 2 == 0, first=i == 0, last=i == P - 1)[name]


def rows(keep):
    """int32 [n], ascending: the kept row numbers."""
    return np.flatnonzero(np.asarray(keep, bool).reshape(-1)).astype(np.int32)


def gather(x, keep):
    return np.asarray(x)[np.asarray(keep, bool).reshape(-1)]


def scatter(y, keep):
    keep, y = np.asarray(keep, bool).reshape(-1), np.asarray(y)
    z = np.zeros((keep.shape[0],) + y.shape[1:], y.dtype)
    z[keep] = y
    return z


def gather_vjp(g, keep):
    """d/dx of sum(g * gather(x))."""
    return scatter(g, keep)


def scatter_vjp(g, keep):
    """d/dy of sum(g * scatter(y))."""
    return gather(g, keep)
