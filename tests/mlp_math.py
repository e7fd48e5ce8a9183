"""The fused 3-layer head in fp64 numpy: forward and backward written out from the chain rule (no autograd), the yardstick of
tests/test_mlp_host.py (held against torch.autograd there) and tests/test_gpu_mlp.py.

    a1 = [x | x_tail] W1^T + b1      h1 = max(a1, 0)
    a2 = h1 W2^T + b2                h2 = max(a2, 0)
    z  = h2 W3^T + b3                y  = z, or 1 / (1 + exp(-z))

    dz  = dy, or dy y (1 - y)
    dW3 = dz^T h2     db3 = sum_rows dz     dh2 = dz W3       da2 = dh2 [a2 > 0]
    dW2 = da2^T h1    db2 = sum_rows da2    dh1 = da2 W2      da1 = dh1 [a1 > 0]
    dW1 = da1^T [x | x_tail]    db1 = sum_rows da1    dx = (da1 W1)[:, :D_x]

A pre-activation of exactly 0 passes no gradient (the derivative of max(a, 0) taken as 0 at 0, as torch does)."""
import numpy as np

NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def forward(x, w1, b1, w2, b2, w3, b3, x_tail=None, sigmoid=False, keep=False):
    x, w1, b1, w2, b2, w3, b3, x_tail = (_f64(a) for a in (x, w1, b1, w2, b2, w3, b3, x_tail))
    xin = x if x_tail is None else np.concatenate((x, x_tail), axis=1)
    a1 = xin @ w1.T + b1
    h1 = np.maximum(a1, 0.0)
    a2 = h1 @ w2.T + b2
    h2 = np.maximum(a2, 0.0)
    z = h2 @ w3.T + b3
    y = 1.0 / (1.0 + np.exp(-z)) if sigmoid else z
    return (y, xin, a1, h1, a2, h2) if keep else y


def forward_backward(x, w1, b1, w2, b2, w3, b3, dy, x_tail=None, sigmoid=False):
    """dict of y and the seven gradients, fp64."""
    y, xin, a1, h1, a2, h2 = forward(x, w1, b1, w2, b2, w3, b3, x_tail, sigmoid, keep=True)
    w1, w2, w3, dy = _f64(w1), _f64(w2), _f64(w3), _f64(dy)
    dz = dy * y * (1.0 - y) if sigmoid else dy
    da2 = (dz @ w3) * (a2 > 0.0)
    da1 = (da2 @ w2) * (a1 > 0.0)
    d_x = np.asarray(x).shape[1]
    return dict(y=y, dx=(da1 @ w1)[:, :d_x], dw1=da1.T @ xin, db1=da1.sum(axis=0), dw2=da2.T @ h1, db2=da2.sum(axis=0),
                dw3=dz.T @ h2, db3=dz.sum(axis=0))


def make_case(d_x, d_tail, h1, h2, d_out, n, seed=0):
    """Inputs of one test case as fp32 numpy: nn.Linear-sized weights (uniform in +-1/sqrt(fan_in)), N(0,1) rows and upstream gradient."""
    rng = np.random.default_rng(seed)
    d_in = d_x + d_tail

    def lin(o, i):
        k = 1.0 / np.sqrt(i)
        return rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, (o,)).astype(np.float32)

    w1, b1 = lin(h1, d_in)
    w2, b2 = lin(h2, h1)
    w3, b3 = lin(d_out, h2)
    return dict(x=rng.standard_normal((n, d_x)).astype(np.float32),
                x_tail=rng.standard_normal((n, d_tail)).astype(np.float32) if d_tail else None,
                w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, dy=rng.standard_normal((n, d_out)).astype(np.float32))
