"""The masked Adam step (GaussianAdam.step(visibility=...)) restated in numpy fp64 -- a helper of the tests, not a test.

A visible row gets oracle/adam_oracle.step's update with the optimizer's ONE global step count t; a row that is not visible keeps
p, m, v, and neither its gradient nor its learning rate enters any arithmetic (NaN / Inf there reach nothing).
tests/test_sparse_adam_host.py pins it against torch.optim.SparseAdam and against the dense oracle."""
import numpy as np


def visible_rows(mask):
    """bool [P] from a mask as GaussianAdam takes it: bool / uint8 non-zero, int32 > 0; [P] or [P, 1]."""
    mask = np.asarray(mask).reshape(-1)
    return mask.copy() if mask.dtype == np.bool_ else mask > 0


def step(p, g, m, v, lr, t, visible, b1=0.9, b2=0.999, eps=1e-15):
    """One step t (1-based, counted over ALL steps, masked or not).  lr: scalar or [rows]; arrays [rows, ...].  Returns (p, m, v) as fp64."""
    p, m, v = (np.array(a, np.float64) for a in (p, m, v))
    vis = visible_rows(visible)
    lr = np.asarray(lr, np.float64)
    lr = lr.reshape(-1)[vis].reshape((-1,) + (1,) * (p.ndim - 1)) if lr.ndim else lr
    gv = np.asarray(g)[vis].astype(np.float64)
    mv = b1 * m[vis] + (1 - b1) * gv
    vv = b2 * v[vis] + (1 - b2) * gv * gv
    denom = np.sqrt(vv) / np.sqrt(1 - b2 ** t) + eps
    p[vis] = p[vis] - (lr / (1 - b1 ** t)) * (mv / denom)
    m[vis], v[vis] = mv, vv
    return p, m, v
