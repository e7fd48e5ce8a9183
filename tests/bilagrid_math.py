"""fp64 numpy restatement of the bilateral-grid colour correction (include/gsrast.h: gsrast_bilagrid_*): forward, both gradients, the
total variation and its gradient; the torch composition the host test pins it to (F.grid_sample + a 3 x 4 matrix product, and its
autograd); and the generator of the test inputs.

Per pixel (px, py) of image [3, H, W], the crop at (x0, y0) of a full_W x full_H frame, with grid [12, L, GH, GW]:
    x = (x0 + px + 0.5) / full_W,  y = (y0 + py + 0.5) / full_H,  gray = 0.299 r + 0.587 g + 0.114 b
    u = x (GW - 1),  v = y (GH - 1),  t = clamp(gray, 0, 1) (L - 1);   A = trilinear(grid; u, v, t);   out_c = A[c, :3] . rgb + A[c, 3]
The guidance slope (d out / d gray through t) is 0 where gray is outside (0, 1) and jumps where t is an integer: the generator keeps every
pixel away from both, so the gradient to the image is well defined at every pixel of a test."""
import numpy as np

GRAY = np.array([0.299, 0.587, 0.114])
GRIDS = [(1, 1, 1), (2, 2, 2), (5, 3, 4), (16, 16, 8), (3, 7, 1)]      # (GW, GH, L)
BAND = 0.02


def window_of(W, H, window=None):
    return (0, 0, W, H) if window is None else tuple(int(v) for v in window)


def _axis(c, n):
    """lower vertex, upper vertex, fraction for index coordinates c on an axis of n vertices (the top end belongs to the last cell)"""
    i0 = np.clip(np.floor(c).astype(np.int64), 0, max(n - 2, 0))
    return i0, np.minimum(i0 + 1, n - 1), c - i0


def _setup(grid, image, window):
    C, L, GH, GW = grid.shape
    assert C == 12 and image.shape[0] == 3
    H, W = image.shape[1:]
    x0, y0, full_W, full_H = window_of(W, H, window)
    img = image.astype(np.float64)
    u = (x0 + np.arange(W) + 0.5) / full_W * (GW - 1)
    v = (y0 + np.arange(H) + 0.5) / full_H * (GH - 1)
    gray = np.tensordot(GRAY, img, 1)                                   # [H, W]
    t = np.clip(gray, 0.0, 1.0) * (L - 1)
    gx0, gx1, fx = _axis(np.broadcast_to(u[None, :], (H, W)), GW)
    gy0, gy1, fy = _axis(np.broadcast_to(v[:, None], (H, W)), GH)
    l0, l1, ft = _axis(t, L)
    corners = []                                                        # (l, gy, gx, weight, d weight / d t) of the 8 corners
    for li, wl, dl in ((l0, 1 - ft, -1.0), (l1, ft, 1.0)):
        for yi, wy in ((gy0, 1 - fy), (gy1, fy)):
            for xi, wx in ((gx0, 1 - fx), (gx1, fx)):
                corners.append((li, yi, xi, wl * wy * wx, dl * wy * wx))
    inside = (gray > 0.0) & (gray < 1.0) & (L > 1)
    return img, gray, inside, corners


def forward(grid, image, window=None):
    """out [3, H, W] (fp64)"""
    g = grid.astype(np.float64)
    img, _, _, corners = _setup(grid, image, window)
    A = sum(g[:, li, yi, xi] * w for li, yi, xi, w, _ in corners)      # [12, H, W]
    A = A.reshape(3, 4, *img.shape[1:])
    return (A[:, :3] * img[None]).sum(1) + A[:, 3]


def backward(grid, image, d_out, window=None):
    """(dL/dgrid [12, L, GH, GW], dL/dimage [3, H, W]) (fp64)"""
    g = grid.astype(np.float64)
    go = d_out.astype(np.float64)
    L = grid.shape[1]
    img, _, inside, corners = _setup(grid, image, window)
    H, W = img.shape[1:]
    rgb1 = np.concatenate([img, np.ones((1, H, W))], 0)                 # [4, H, W]
    val = (go[:, None] * rgb1[None]).reshape(12, H, W)                  # dL/dA
    d_grid = np.zeros_like(g)
    A = np.zeros((12, H, W))
    dA_dt = np.zeros((12, H, W))
    for li, yi, xi, w, dw in corners:
        for ch in range(12):
            np.add.at(d_grid[ch], (li, yi, xi), val[ch] * w)
        A += g[:, li, yi, xi] * w
        dA_dt += g[:, li, yi, xi] * dw
    d_image = (go[:, None] * A.reshape(3, 4, H, W)[:, :3]).sum(0)
    d_gray = np.where(inside, (val * dA_dt).sum(0) * (L - 1), 0.0)
    return d_grid, d_image + GRAY[:, None, None] * d_gray[None]


def tv(grids):
    """sum over the three grid axes of the mean of the squared forward differences of grids [N, 12, L, GH, GW] (fp64)"""
    g = grids.astype(np.float64)
    total = 0.0
    for axis in (2, 3, 4):
        d = np.diff(g, axis=axis)
        if d.size:
            total += float((d * d).mean())
    return total


def tv_grad(grids):
    g = grids.astype(np.float64)
    out = np.zeros_like(g)
    for axis in (2, 3, 4):
        d = np.diff(g, axis=axis)
        if not d.size:
            continue
        d = d * (2.0 / d.size)
        lo, hi = [slice(None)] * 5, [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        out[tuple(hi)] += d
        out[tuple(lo)] -= d
    return out


# ---- the torch composition (any dtype, CPU): what the restatement is pinned to and what sets the fp32 bar of the GPU tests ----
def torch_apply(grid, image, window=None):
    import torch
    import torch.nn.functional as F
    H, W = image.shape[1:]
    x0, y0, full_W, full_H = window_of(W, H, window)
    x = (x0 + torch.arange(W, dtype=image.dtype) + 0.5) / full_W
    y = (y0 + torch.arange(H, dtype=image.dtype) + 0.5) / full_H
    gray = 0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]
    coords = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), gray], -1)          # [H, W, 3]: (x, y, z) -> (GW, GH, L)
    A = F.grid_sample(grid[None], (2.0 * coords - 1.0)[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A.reshape(3, 4, H, W)
    return torch.einsum("ckhw,khw->chw", A[:, :3], image) + A[:, 3]


def torch_tv(grids):
    total = 0.0
    for axis in (2, 3, 4):
        if grids.shape[axis] > 1:
            d = grids.narrow(axis, 1, grids.shape[axis] - 1) - grids.narrow(axis, 0, grids.shape[axis] - 1)
            total = total + (d * d).mean()
    return total if not isinstance(total, float) else grids.sum() * 0.0


def torch_run(grid, image, d_out, window=None, dtype=None):
    """torch's CPU run of the composition and its autograd in `dtype` -> dict(out, d_grid, d_image) as numpy"""
    import torch
    g = torch.tensor(np.asarray(grid), dtype=dtype).requires_grad_(True)
    im = torch.tensor(np.asarray(image), dtype=dtype).requires_grad_(True)
    out = torch_apply(g, im, window)
    out.backward(torch.tensor(np.asarray(d_out), dtype=dtype))
    return dict(out=out.detach().numpy(), d_grid=g.grad.numpy(), d_image=im.grad.numpy())


def torch_tv_run(grids, dtype=None):
    import torch
    g = torch.tensor(np.asarray(grids), dtype=dtype).requires_grad_(True)
    value = torch_tv(g)
    value.backward()
    return dict(tv=value.detach().numpy(), d_tv=g.grad.numpy())


# ---- inputs ----
def identity_grid(GW, GH, L):
    g = np.zeros((12, L, GH, GW), np.float32)
    g[[0, 5, 10]] = 1.0
    return g


def make_case(GW, GH, L, W, H, seed):
    """dict(grid [12, L, GH, GW], image [3, H, W], d_out [3, H, W]) as float32.  rgb is drawn in [-0.2, 1.2]; then every pixel whose gray
    (fp64, from the float32 channels) has frac(t) outside [BAND, 1 - BAND] (L > 1) or lies within BAND of 0 or 1 gets ONE shift added to
    its three channels -- gray moves by that shift, the weights sum to 1 -- that lands frac(t) on 0.5 (L = 1: gray on 0.5).
    Asserted afterwards, on the float32 values: no pixel is left in a band (so none is excluded from a comparison) and, on an image of at least 64 pixels, at least 5 % of them are clamped."""
    rng = np.random.default_rng(seed)
    grid = (identity_grid(GW, GH, L) + 0.3 * rng.standard_normal((12, L, GH, GW))).astype(np.float32)
    # rgb in [-0.2, 1.2], the three channels of a pixel around a common brightness: independent channels would leave under 5 % of the grays outside [0, 1]
    image = np.clip(rng.uniform(-0.2, 1.2, (1, H, W)) + 0.15 * rng.standard_normal((3, H, W)), -0.2, 1.2).astype(np.float32)
    d_out = rng.standard_normal((3, H, W)).astype(np.float32)

    def bands(img):
        gray = np.tensordot(GRAY, img.astype(np.float64), 1)
        near = (np.abs(gray) < BAND) | (np.abs(gray - 1.0) < BAND)
        if L > 1:
            fr = np.clip(gray, 0.0, 1.0) * (L - 1)
            fr = fr - np.floor(fr)
            near |= ((fr < BAND) | (fr > 1 - BAND)) & (gray > 0.0) & (gray < 1.0)
        return gray, near

    gray, near = bands(image)
    if L > 1:      # the middle of the pixel's cell (of the first / last cell for a gray at or beyond the ends)
        target = (np.clip(np.floor(np.clip(gray, 0.0, 1.0) * (L - 1)), 0, L - 2) + 0.5) / (L - 1)
    else:
        target = np.full_like(gray, 0.5)
    image = np.where(near[None], image.astype(np.float64) + (target - gray)[None], image).astype(np.float32)
    gray, near = bands(image)
    assert not near.any(), (GW, GH, L, W, H, seed, int(near.sum()))
    if W * H >= 64:
        assert ((gray < 0.0) | (gray > 1.0)).mean() >= 0.05, (GW, GH, L, W, H, seed)
    return dict(grid=grid, image=image, d_out=d_out)


def make_grids(N, GW, GH, L, seed):
    rng = np.random.default_rng(seed)
    return (identity_grid(GW, GH, L)[None] + 0.3 * rng.standard_normal((N, 12, L, GH, GW))).astype(np.float32)
