"""Normal consistency (include/gsrast.h: gsrast_gaussian_normals_*, gsrast_depth_normal_*, gsrast_normal_loss_*) restated in fp64 numpy,
each op with its analytic backward; the torch composition that serves as the fp32 yardstick (and, in fp64 under torch.autograd, as the
check of the analytic backwards: tests/test_normal_host.py); and the case generators of tests/test_gpu_normal.py.

    per Gaussian   k = argmin(scales) (a tie: the lowest index), n = +-column k of R(q / |q|) rotated by V[:3, :3], facing the camera
                   (negated where n . p_view > 0); |q| = 0 or a non-finite q: n = 0
    per pixel      u_x = ((2x + 1) / W - 1) tanfovx, v_y likewise, P = d (u, v, 1); a = P(x, y+1) - P(x, y-1), b = P(x+1, y) - P(x-1, y),
                   c = a x b, n = c / |c|; n = 0 on the border, where one of the four depths is not > 0, where c . c < 1e-24
    the loss       mean_p (1 - w_p <N_p, n_p>)

The generators keep every case away from the rules' edges and assert it, so that no element has to be left out of a comparison: scales of a
row differ by >= 5 % of the smallest, |n . p| >= 1e-3 |p|, a stencil depth is >= 0.2 or invalid on purpose (0, negative, NaN), and
c . c >= 1e-16 wherever a normal exists."""
import numpy as np
import torch
import torch.nn.functional as F

import math_renderer as mr

MIN_CC = 1e-24
TANFOV = (0.6, 0.45)      # of every image case
TILE_W, TILE_H = 64, 16   # csrc/gsrast_normal.h: NM_TW, NM_TH
WIDTHS = (1, 2, 3, 5, 63, 64, 65, 66, 67, 130)
HEIGHTS = (1, 2, 3, 4, 5, 9, 33, 70) + (TILE_H - 1, TILE_H, TILE_H + 1, TILE_H + 2, 2 * TILE_H + 3)
FIELDS = ("plane", "wavy", "step", "hole", "nan", "negative")
PLANE = (2.5, 0.3, -0.2)  # z = z0 + alpha x + beta y in view space


# ---- the image ops --------------------------------------------------------------------------------------------------------------------------
def rays(W, H, tx, ty):
    return ((2.0 * np.arange(W) + 1.0) / W - 1.0) * tx, ((2.0 * np.arange(H) + 1.0) / H - 1.0) * ty


def _stencils(depth, tx, ty):
    """a, b, c [3, H, W], c . c and valid [H, W] of every pixel (zeros where the pixel has no normal)"""
    d = np.asarray(depth, np.float64)
    d = d.reshape(d.shape[-2:])
    H, W = d.shape
    u, v = rays(W, H, tx, ty)
    a, b = np.zeros((3, H, W)), np.zeros((3, H, W))
    valid = np.zeros((H, W), bool)
    if H >= 3 and W >= 3:
        up, dn, lf, rt = d[:-2, 1:-1], d[2:, 1:-1], d[1:-1, :-2], d[1:-1, 2:]
        with np.errstate(invalid="ignore"):
            valid[1:-1, 1:-1] = (up > 0) & (dn > 0) & (lf > 0) & (rt > 0)
            ui, vi = u[None, 1:-1], v[1:-1, None]
            a[:, 1:-1, 1:-1] = np.stack([dn * ui - up * ui, dn * v[2:, None] - up * v[:-2, None], dn - up])
            b[:, 1:-1, 1:-1] = np.stack([rt * u[None, 2:] - lf * u[None, :-2], rt * vi - lf * vi, rt - lf])
    a, b = np.where(valid, a, 0.0), np.where(valid, b, 0.0)
    c = np.cross(a, b, axis=0)
    cc = (c * c).sum(0)
    valid &= ~(cc < MIN_CC)
    return np.where(valid, a, 0.0), np.where(valid, b, 0.0), np.where(valid, c, 0.0), np.where(valid, cc, 1.0), valid


def depth_to_normal(depth, tx, ty):
    _, _, c, cc, _ = _stencils(depth, tx, ty)
    return c / np.sqrt(cc)


def _depth_grad(depth, tx, ty, g):
    """dL/dd [H, W] from g = dL/dn [3, H, W]"""
    a, b, c, cc, valid = _stencils(depth, tx, ty)
    H, W = valid.shape
    u, v = rays(W, H, tx, ty)
    inv = 1.0 / np.sqrt(cc)
    n = c * inv
    dc = np.where(valid, (g - n * (n * g).sum(0)) * inv, 0.0)
    da, db = np.cross(b, dc, axis=0), np.cross(dc, a, axis=0)
    dd = np.zeros((H, W))
    ray = lambda t: u[None, :] * t[0] + v[:, None] * t[1] + t[2]  # noqa: E731  (the dot product with every pixel's own ray)
    shift = lambda t, dy, dx: np.roll(t, (dy, dx), axis=(1, 2))  # noqa: E731  (da, db vanish on the border: nothing wraps around)
    dd += ray(shift(da, 1, 0))       # the pixel above has q as its lower tap
    dd -= ray(shift(da, -1, 0))
    dd += ray(shift(db, 0, 1))       # the pixel to the left has q as its right tap
    dd -= ray(shift(db, 0, -1))
    return dd


def depth_to_normal_backward(depth, tx, ty, d_normals):
    return _depth_grad(depth, tx, ty, np.asarray(d_normals, np.float64))


def _weight(weight, shape):
    return np.ones(shape) if weight is None else np.asarray(weight, np.float64).reshape(shape)


def normal_loss(normal_map, depth, tx, ty, weight=None):
    N, n = np.asarray(normal_map, np.float64), depth_to_normal(depth, tx, ty)
    return float(np.mean(1.0 - _weight(weight, n.shape[1:]) * (N * n).sum(0)))


def normal_loss_backward(normal_map, depth, tx, ty, weight=None, upstream=1.0):
    """(dL/dnormal_map [3, H, W], dL/ddepth [H, W])"""
    N, n = np.asarray(normal_map, np.float64), depth_to_normal(depth, tx, ty)
    s = -float(upstream) / (n.shape[1] * n.shape[2]) * _weight(weight, n.shape[1:])
    return s * n, _depth_grad(depth, tx, ty, s * N)


# ---- the per-Gaussian op --------------------------------------------------------------------------------------------------------------------
def _columns(qh, k):
    """column k[i] of the rotation matrix of the unit quaternion qh[i] = (r, x, y, z)"""
    r, x, y, z = qh.T
    cols = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
                     np.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
                     np.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1)], 1)      # [P, k, 3]
    return cols[np.arange(len(k)), k]


def _gauss(means3D, scales, rotations, V):
    m, s, q, V = (np.asarray(t, np.float64) for t in (means3D, scales, rotations, V))
    k = np.argmin(s, axis=1) if len(s) else np.zeros(0, int)      # (numpy: the first of equal minima)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((q * q).sum(1))
        ok = np.isfinite(q).all(1) & (length > 0)
        qh = np.where(ok[:, None], q / np.where(ok, length, 1.0)[:, None], [1.0, 0.0, 0.0, 0.0])
    n = _columns(qh, k) @ V[:3, :3]
    p = m @ V[:3, :3] + V[3, :3]
    with np.errstate(invalid="ignore"):
        dot = (n * p).sum(1)
        sign = np.where(dot > 0, -1.0, 1.0)
    return k, qh, np.where(ok, length, 1.0), ok, sign, n, p, dot


def gaussian_normals(means3D, scales, rotations, V):
    _, _, _, ok, sign, n, _, _ = _gauss(means3D, scales, rotations, V)
    return np.where(ok[:, None], sign[:, None] * n, 0.0)


def gaussian_normals_backward(means3D, scales, rotations, V, d_normals):
    """dL/drotations [P, 4]"""
    k, qh, length, ok, sign, _, _, _ = _gauss(means3D, scales, rotations, V)
    G = sign[:, None] * (np.asarray(d_normals, np.float64) @ np.asarray(V, np.float64)[:3, :3].T)      # dL / d (column k), world space
    r, x, y, z = qh.T
    G0, G1, G2 = G.T
    per_k = [np.stack([2 * (z * G1 - y * G2), 2 * (y * G1 + z * G2), 2 * (x * G1 - r * G2) - 4 * y * G0, 2 * (r * G1 + x * G2) - 4 * z * G0], 1),
             np.stack([2 * (x * G2 - z * G0), 2 * (y * G0 + r * G2) - 4 * x * G1, 2 * (x * G0 + z * G2), 2 * (y * G2 - r * G0) - 4 * z * G1], 1),
             np.stack([2 * (y * G0 - x * G1), 2 * (z * G0 - r * G1) - 4 * x * G2, 2 * (r * G0 + z * G1) - 4 * y * G2, 2 * (x * G0 + y * G1)], 1)]
    dqh = np.stack(per_k, 1)[np.arange(len(k)), k]
    dq = (dqh - qh * (qh * dqh).sum(1, keepdims=True)) / length[:, None]
    return np.where(ok[:, None], dq, 0.0)


# ---- the torch composition: gsplat's slicing form of depth_to_normal (points, two slice differences, cross, F.normalize, zero padding) in
# view space, with the two stated deviations (the coverage rule, no normal below c . c = 1e-24) as masks; the reference's rotation matrix ----
def torch_depth_to_normal(depth, tx, ty):
    d = depth.reshape(depth.shape[-2:])
    H, W = d.shape
    if H < 3 or W < 3:
        return torch.zeros((3, H, W), dtype=d.dtype, device=d.device) + 0.0 * d.sum().nan_to_num()
    x, y = torch.arange(W, dtype=d.dtype, device=d.device), torch.arange(H, dtype=d.dtype, device=d.device)
    u, v = ((2.0 * x + 1.0) / W - 1.0) * tx, ((2.0 * y + 1.0) / H - 1.0) * ty
    dirs = torch.stack([u[None, :].expand(H, W), v[:, None].expand(H, W), torch.ones_like(d)], dim=-1)
    points = torch.where(d > 0, d, torch.ones_like(d))[..., None] * dirs      # (a depth that is not > 0 only feeds stencils the mask drops: any finite stand-in keeps 0 x NaN out of the backward)
    dx = points[2:, 1:-1, :] - points[:-2, 1:-1, :]
    dy = points[1:-1, 2:, :] - points[1:-1, :-2, :]
    c = torch.cross(dx, dy, dim=-1)
    ok = (d[2:, 1:-1] > 0) & (d[:-2, 1:-1] > 0) & (d[1:-1, 2:] > 0) & (d[1:-1, :-2] > 0) & ((c * c).sum(-1) >= MIN_CC)
    away = torch.tensor([0.0, 0.0, -1.0], dtype=d.dtype, device=d.device)
    n = F.normalize(torch.where(ok[..., None], c, away), dim=-1)      # (a masked stencil never reaches the division)
    n = torch.where(ok[..., None], n, torch.zeros_like(n))
    return F.pad(n, (0, 0, 1, 1, 1, 1), value=0.0).permute(2, 0, 1)


def torch_normal_loss(normal_map, depth, tx, ty, weight=None):
    dot = (normal_map * torch_depth_to_normal(depth, tx, ty)).sum(0)
    return (1.0 - (dot if weight is None else weight.reshape(dot.shape) * dot)).mean()


def torch_gaussian_normals(means3D, scales, rotations, V):
    P = means3D.shape[0]
    length = torch.sqrt((rotations * rotations).sum(1))
    ok = torch.isfinite(rotations).all(1) & (length > 0)
    unit = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=rotations.dtype, device=rotations.device)
    q = torch.where(ok[:, None], rotations, unit)
    R = mr.rotation_matrix(q / torch.sqrt((q * q).sum(1))[:, None])      # utils/general_utils.build_rotation: normalise, then this matrix
    k = torch.argmin(scales, dim=1) if P else torch.zeros(0, dtype=torch.long, device=scales.device)      # (torch: the first of equal minima)
    n = R[torch.arange(P, device=R.device), :, k] @ V[:3, :3]
    p = (torch.cat([means3D, torch.ones_like(means3D[:, :1])], 1) @ V)[:, :3]
    n = torch.where(((n * p).sum(1) > 0)[:, None], -n, n)
    return torch.where(ok[:, None], n, torch.zeros_like(n))


def torch_image_run(case, dtype, weight=True, device="cpu"):
    """dict(n, d_depth, loss, dN, dd) of one image case by autograd of the composition in `dtype`"""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    tx, ty = case["tanfov"]
    d = t(case["depth"]).requires_grad_(True)
    n = torch_depth_to_normal(d, tx, ty)
    n.backward(t(case["d_normals"]))
    out = dict(n=n.detach().cpu().numpy(), d_depth=d.grad.cpu().numpy())
    d2, N = t(case["depth"]).requires_grad_(True), t(case["normal_map"]).requires_grad_(True)
    loss = torch_normal_loss(N, d2, tx, ty, t(case["weight"]) if weight else None)
    (loss * case["upstream"]).backward()
    out.update(loss=loss.detach().cpu().numpy(), dN=N.grad.cpu().numpy(), dd=d2.grad.cpu().numpy())
    return out


def numpy_image_run(case, weight=True):
    tx, ty = case["tanfov"]
    w = case["weight"] if weight else None
    dN, dd = normal_loss_backward(case["normal_map"], case["depth"], tx, ty, w, case["upstream"])
    return dict(n=depth_to_normal(case["depth"], tx, ty), d_depth=depth_to_normal_backward(case["depth"], tx, ty, case["d_normals"]),
                loss=np.float64(normal_loss(case["normal_map"], case["depth"], tx, ty, w)), dN=dN, dd=dd)


def torch_gaussian_run(case, dtype, device="cpu"):
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    q = t(case["rotations"]).requires_grad_(True)
    n = torch_gaussian_normals(t(case["means3D"]), t(case["scales"]), q, t(case["viewmatrix"]))
    n.backward(t(case["d_normals"]))
    return dict(n=n.detach().cpu().numpy(), d_rotations=q.grad.cpu().numpy())


def numpy_gaussian_run(case):
    args = (case["means3D"], case["scales"], case["rotations"], case["viewmatrix"])
    return dict(n=gaussian_normals(*args), d_rotations=gaussian_normals_backward(*args, case["d_normals"]))


# ---- generators -------------------------------------------------------------------------------------------------------------------------------
def plane_depth(W, H, z0, alpha, beta, tanfov=TANFOV):
    """[H, W] fp64: the view-space z of the plane z = z0 + alpha x + beta y along every pixel's ray (x = z u, y = z v)"""
    u, v = rays(W, H, *tanfov)
    return z0 / (1.0 - alpha * u[None, :] - beta * v[:, None])


def make_depth(kind, W, H, seed=0, tanfov=TANFOV):
    """[H, W] float32.  plane: z = z0 + alpha x + beta y in view space; wavy: smooth; step: an edge of 2 units down the middle; hole: a
    rectangle of zeros across the corner of the first pixel tile; nan / negative: one such pixel, the first of the tile behind that corner."""
    assert kind in FIELDS, kind
    tx, ty = tanfov
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if kind == "plane":
        d = plane_depth(W, H, *PLANE, tanfov)
    else:
        rng = np.random.default_rng(seed)
        ph = rng.uniform(0, 2 * np.pi, 3)
        d = 3.0 + 0.4 * np.sin(0.31 * xx + ph[0]) * np.cos(0.23 * yy + ph[1]) + 0.1 * np.sin(0.7 * xx + 0.9 * yy + ph[2])
    if kind == "step":
        d = d + 2.0 * (xx >= W // 2)
    d = d.astype(np.float32)
    x0, y0 = min(TILE_W - 4, max(W // 2 - 1, 0)), min(TILE_H - 3, max(H // 2 - 1, 0))
    if kind == "hole":
        d[y0:y0 + 7, x0:x0 + 10] = 0.0
    if kind in ("nan", "negative"):
        d[min(TILE_H, H // 2), min(TILE_W, W // 2)] = np.nan if kind == "nan" else -1.0
    with np.errstate(invalid="ignore"):
        assert ((d >= 0.2) | (d <= 0.0) | np.isnan(d)).all(), "a stencil depth is >= 0.2 or invalid on purpose"
    _, _, _, cc, valid = _stencils(d, tx, ty)
    assert (cc[valid] >= 1e-16).all(), ("c . c >= 1e-16 wherever a normal exists", float(cc[valid].min()))
    return d


def make_image_case(kind, W, H, seed=0):
    """depth, a render-like normal map (0.8 x the surface's own normal + noise, not normalised), an upstream for depth_to_normal, a weight
    in [0, 1] and the loss's upstream scalar; float32 arrays"""
    rng = np.random.default_rng(1000 * seed + 7 * W + H)
    d = make_depth(kind, W, H, seed)
    N = 0.8 * depth_to_normal(d, *TANFOV) + 0.2 * rng.normal(size=(3, H, W))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(kind=kind, W=W, H=H, tanfov=TANFOV, depth=d, normal_map=f32(N), d_normals=f32(rng.normal(size=(3, H, W))),
                weight=f32(rng.uniform(0, 1, (H, W))), upstream=0.75)


SPECIAL_ROWS = ("tie", "zero quaternion", "nan quaternion", "un-normalised quaternion")      # rows 0 .. 3 of a case with special=True and P >= 4


def make_gaussian_case(P, cam, seed=0, special=True):
    """means3D, scales, rotations (un-normalised: lengths in [0.5, 2]), the camera's viewmatrix and an upstream [P, 3]; float32.
    special (P >= 4): row 0 has its two smallest scales equal, row 1 a zero quaternion, row 2 a NaN in its quaternion, row 3 a quaternion of length 37.5."""
    rng = np.random.default_rng(seed + 31 * P)
    V = np.asarray(cam["viewmatrix"], np.float32)
    smin = np.exp(rng.uniform(np.log(0.01), np.log(0.2), P))
    smid = smin * (1.07 + rng.uniform(0, 1, P))
    smax = smid * (1.07 + rng.uniform(0, 1, P))
    scales = np.stack([smin, smid, smax], 1)
    scales = np.take_along_axis(scales, np.argsort(rng.uniform(size=(P, 3)), axis=1), 1).astype(np.float32)
    q = rng.normal(size=(P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32)
    means = rng.uniform(-1.3, 1.3, (P, 3)).astype(np.float32)
    distinct, has_normal = np.ones(P, bool), np.ones(P, bool)      # rows whose three scales differ; rows that have a normal
    if special and P >= 4:
        scales[0] = (0.05, 0.05, 0.3)
        q[1] = 0.0
        q[2, 2] = np.nan
        q[3] *= np.float32(37.5) / np.linalg.norm(q[3].astype(np.float64))
        distinct[0], has_normal[1:3] = False, False
    for _ in range(20):      # a mean whose normal is nearly tangent to its view ray is drawn again
        *_, p, dot = _gauss(means, scales, q, V)
        near = has_normal & ~(np.abs(dot) >= 2e-3 * np.linalg.norm(p, axis=1))
        if not near.any():
            break
        means[near] = rng.uniform(-1.3, 1.3, (int(near.sum()), 3)).astype(np.float32)
    *_, p, dot = _gauss(means, scales, q, V)
    srt = np.sort(scales.astype(np.float64), axis=1)
    assert (np.abs(dot[has_normal]) >= 1e-3 * np.linalg.norm(p[has_normal], axis=1)).all(), "|n . p| >= 1e-3 |p|"
    assert ((srt[distinct, 1] - srt[distinct, 0]) >= 0.05 * srt[distinct, 0]).all() and ((srt[:, 2] - srt[:, 1]) >= 0.05 * srt[:, 0]).all(), "scales differ by >= 5 % of the smallest"
    return dict(P=P, means3D=means, scales=scales, rotations=q, viewmatrix=V, d_normals=rng.normal(size=(P, 3)).astype(np.float32))
