"""Mip-Splatting's 3-D smoothing filter restated for the tests (include/gsrast.h: gsrast_filter3d_*):

* ``sweep``: the camera sweep in the header's order of operations, in np.float32 (the BIT MODEL of filter3d_sweep_kernel +
  filter3d_finish_kernel: every operation rounded, no FMA) or np.float64, with the rows whose validity hangs on a rounding marked;
* ``apply_fwd`` / ``apply_bwd``: the fused activation and its analytic backward in fp64, in the ratio form of the header;
* ``upstream_compute_3D_filter`` / ``upstream_scaling`` / ``upstream_opacity``: a literal torch transcription of Mip-Splatting's
  ``compute_3D_filter`` loop and its two getters (scene/gaussian_model.py there), which pin the restatements.
"""
import math

import numpy as np
import torch

NEAR, MARGIN, VARIANCE = 0.2, 0.15, 0.2
AMBIGUOUS = 1e-4      # |zc - near| < 1e-4, or a projection within 1e-4 W (1e-4 H) of a screen bound


def table_of(cameras, dtype=np.float64):
    """([C, 16] table in `dtype` from the fp32 viewmatrices and the fp64 focal lengths rounded as the library's table is, focal_max)."""
    rows, fmax = [], 0.0
    for c in cameras:
        V = np.asarray(c["viewmatrix"], np.float32).reshape(4, 4)
        W, H = float(c["image_width"]), float(c["image_height"])
        fx, fy = W / (2.0 * float(c["tanfovx"])), H / (2.0 * float(c["tanfovy"]))
        fmax = max(fmax, fx)
        rows.append(np.concatenate([V[:3, :3].reshape(9), V[3, :3], np.array([fx, fy, W, H], np.float64).astype(np.float32)]))
    return np.stack(rows).astype(np.float32).astype(dtype), fmax


def sweep(xyz, table, dtype, focal_max, near=NEAR, margin=MARGIN, variance=VARIANCE):
    """dict(filter [P, 1], valid [P] bool, dist [P] (inf where not valid), cam [P] (the camera attaining dist, -1), dmax, k, ambiguous [P]
    bool) of the sweep evaluated in `dtype`; near, margin, variance are rounded to `dtype` once, k is formed in fp64 and rounded once."""
    dt = np.dtype(dtype).type
    xyz, table = np.asarray(xyz).astype(dt), np.asarray(table).astype(dt)
    P = xyz.shape[0]
    near_t, margin_t, var_t = dt(near), dt(margin), dt(variance)
    k = dt(math.sqrt(float(var_t)) / float(focal_max))
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    dist, cam = np.full(P, np.inf, dt), np.full(P, -1, np.int64)
    ambiguous = np.zeros(P, bool)
    half, tiny = dt(0.5), dt(0.001)
    with np.errstate(all="ignore"):
        for c, r in enumerate(table):
            xc = ((x * r[0] + y * r[3]) + z * r[6]) + r[9]
            yc = ((x * r[1] + y * r[4]) + z * r[7]) + r[10]
            zc = ((x * r[2] + y * r[5]) + z * r[8]) + r[11]
            zz = np.fmax(zc, tiny)
            fx, fy, W, H = r[12], r[13], r[14], r[15]
            mw, mh = margin_t * W, margin_t * H
            px = (xc / zz) * fx + W * half
            py = (yc / zz) * fy + H * half
            front = zc > near_t
            seen = front & (zz < np.inf) & (px >= -mw) & (px <= W + mw) & (py >= -mh) & (py <= H + mh)
            closer = seen & (zz < dist)
            dist = np.where(closer, zz, dist)
            cam = np.where(closer, c, cam)
            edge = np.zeros(P, bool)
            for p, lo, hi, size in ((px, -mw, W + mw, W), (py, -mh, H + mh, H)):
                edge |= (np.abs(p - lo) < AMBIGUOUS * size) | (np.abs(p - hi) < AMBIGUOUS * size)
            ambiguous |= (np.abs(zc - near_t) < AMBIGUOUS) | (front & edge)
    valid = dist < np.inf
    dmax = dist[valid].max() if valid.any() else dt(0.0)
    filt = (np.where(valid, dist, dmax) * k).astype(dt)
    return dict(filter=filt[:, None], valid=valid, dist=dist, cam=cam, dmax=dmax, k=k, ambiguous=ambiguous)


def _axes(s, f):
    s, f = np.asarray(s, np.float64), np.asarray(f, np.float64).reshape(-1, 1)
    sf = np.sqrt(s * s + f * f)
    zero = sf == 0.0
    safe = np.where(zero, 1.0, sf)
    return sf, np.where(zero, 1.0, s / safe), np.where(zero, 0.0, f / safe), zero, safe


def apply_fwd(s, o, f):
    """(scales_f [P, 3], opacities_f [P, 1], coef [P, 1]) in fp64:  s_f = sqrt(s^2 + f^2), r = s / s_f (1 where s_f == 0), o_f = o (r0 r1) r2."""
    sf, r, _, _, _ = _axes(s, f)
    coef = ((r[:, 0] * r[:, 1]) * r[:, 2])[:, None]
    return sf, np.asarray(o, np.float64).reshape(-1, 1) * coef, coef


def apply_bwd(s, o, f, g_s, g_o):
    """(d scales, d opacities, term_a, term_b) in fp64: d s_k = g_s,k r_k + (G prod_{j != k} r_j) (q_k^2 / s_f,k), G = g_o o; d o = g_o coef.
    term_a = |g_s r| and term_b = |G prod r q^2 / s_f|: what the d scales bar of the GPU test is made of.  None upstream = zero."""
    sf, r, q, zero, safe = _axes(s, f)
    o = np.asarray(o, np.float64).reshape(-1, 1)
    g_s = np.zeros_like(sf) if g_s is None else np.asarray(g_s, np.float64)
    g_o = np.zeros_like(o) if g_o is None else np.asarray(g_o, np.float64).reshape(-1, 1)
    G = g_o * o
    others = np.stack([r[:, 1] * r[:, 2], r[:, 0] * r[:, 2], r[:, 0] * r[:, 1]], axis=1)
    t = np.where(zero, 0.0, (q * q) / safe)
    a, b = g_s * r, (G * others) * t
    return a + b, g_o * ((r[:, 0] * r[:, 1]) * r[:, 2])[:, None], np.abs(a), np.abs(b)


# ---- the literal transcription of upstream (Mip-Splatting, scene/gaussian_model.py) -------------------------------------------------
class UpstreamCamera:
    """What upstream's loop reads of a camera: R, T (numpy), focal_x, focal_y, image_width, image_height."""

    def __init__(self, cam):
        V = np.asarray(cam["viewmatrix"], np.float32).reshape(4, 4)
        self.R, self.T = V[:3, :3].copy(), V[3, :3].copy()
        self.image_width, self.image_height = int(cam["image_width"]), int(cam["image_height"])
        self.focal_x = self.image_width / (2.0 * float(cam["tanfovx"]))
        self.focal_y = self.image_height / (2.0 * float(cam["tanfovy"]))


@torch.no_grad()
def upstream_compute_3D_filter(xyz, cameras, dtype=torch.float32):
    """compute_3D_filter, line for line (its float32 tensors in `dtype`); returns (filter_3D [P, 1], valid_points [P])."""
    distance = torch.ones((xyz.shape[0]), device=xyz.device, dtype=dtype) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.
    for camera in cameras:
        R = torch.tensor(camera.R, device=xyz.device, dtype=dtype)
        T = torch.tensor(camera.T, device=xyz.device, dtype=dtype)
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * camera.focal_x + camera.image_width / 2.0
        y = y / z * camera.focal_y + camera.image_height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * camera.image_width, x <= camera.image_width * 1.15),
                                      torch.logical_and(y >= -0.15 * camera.image_height, y <= 1.15 * camera.image_height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < camera.focal_x:
            focal_length = camera.focal_x
    distance[~valid_points] = distance[valid_points].max()
    filter_3D = distance / focal_length * (0.2 ** 0.5)
    return filter_3D[..., None], valid_points


def upstream_scaling(scales, filter_3D):
    """get_scaling_with_3D_filter on activated scales"""
    scales = torch.square(scales) + torch.square(filter_3D)
    return torch.sqrt(scales)


def upstream_opacity(opacity, scales, filter_3D):
    """get_opacity_with_3D_filter on activated values"""
    scales_square = torch.square(scales)
    det1 = scales_square.prod(dim=1)
    scales_after_square = scales_square + torch.square(filter_3D)
    det2 = scales_after_square.prod(dim=1)
    coef = torch.sqrt(det1 / det2)
    return opacity * coef[..., None]


# ---- the cases the host and the GPU tests share -------------------------------------------------------------------------------------
SWEEP_CASES = [(4099, 7, 2.0), (70001, 33, 2.0), (4099, 3, 1.0)]      # (P, V, radius)


def ring(scenes, V, radius=2.0):
    """V cameras on a ring, three image sizes in one table"""
    return [scenes.camera(k, V, 130 + 16 * (k % 3), 70, radius=radius) for k in range(V)]


EDGE_ROWS = dict(s=[[0.0, 0.0, 0.0], [1e-20, 1.0, 1e-3], [1e-15, 1e-15, 1e-15], [0.0, 0.5, 0.25]], f=[0.0, 1e-3, 1e-3, 0.0], o=[0.7, 0.9, 0.6, 0.8])


def apply_case(P, seed=0, edges=True):
    """fp32 (scales [P, 3] log-uniform in [1e-4, 1], opacities [P, 1], filter [P, 1] in [1e-3, 3e-2] with every 7th 0, g_s, g_o); with
    `edges` the first rows (as far as P reaches) are EDGE_ROWS."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(math.log(1e-4), 0.0, size=(P, 3))).astype(np.float32)
    o = rng.uniform(0.01, 0.99, size=(P, 1)).astype(np.float32)
    f = rng.uniform(1e-3, 3e-2, size=(P, 1)).astype(np.float32)
    f[::7] = 0.0
    if edges:
        n = min(P, len(EDGE_ROWS["f"]))
        s[:n] = np.float32(EDGE_ROWS["s"][:n]).reshape(n, 3)
        f[:n, 0], o[:n, 0] = np.float32(EDGE_ROWS["f"][:n]), np.float32(EDGE_ROWS["o"][:n])
    g_s = rng.normal(size=(P, 3)).astype(np.float32)
    g_o = rng.normal(size=(P, 1)).astype(np.float32)
    return s, o, f, g_s, g_o
