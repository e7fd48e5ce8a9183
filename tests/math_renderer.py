"""An INDEPENDENT differentiable splatting renderer, written from the mathematics of the method (EWA projection of 3-D
Gaussians, front-to-back alpha compositing) in torch float64 with autograd -- test infrastructure, used by
tests/test_oracle_independent.py to check the oracle's forward AND its hand-derived backward formulas against something that
shares no code and no derivation with oracle/gsrast_oracle.c or the HIP kernels: there is no tile list, no per-tile loop, no
hand-written gradient here; gradients come from autograd of the forward below.

What is taken from the reference (cited) is only what DEFINES the function being differentiated:
  * conventions: row-vector matrices stored transposed (scene/cameras.py:90-100), quaternion (r, x, y, z) used as given
    (forward.cu:127-131), p_w = 1 / (w + 1e-7) (forward.cu:195-197), pixel = ((ndc + 1) * S - 1) / 2 (auxiliary.h:41-44);
  * constants: near-plane cull z <= 0.2 (auxiliary.h:154), frustum clamp 1.3 * tanfov (forward.cu:82-87), + 0.3 on the 2-D
    covariance diagonal (forward.cu:110-111), radius = ceil(3 sqrt(lambda_max)), lambda from max(0.1, mid^2 - det)
    (forward.cu:229-232), 16 x 16 tiles with (int) truncation (auxiliary.h:46-56), alpha = min(0.99, o G), skip alpha < 1/255,
    stop before T (1 - alpha) < 1e-4 (forward.cu:343-357), colour = max(SH + 0.5, 0) (forward.cu:60-70);
  * two deliberate deviations of the reference's backward from the true derivative, reproduced so that the comparison is
    meaningful: the 0.99 clamp of alpha passes gradients through (backward.cu:538, :554 apply no mask) -> straight-through
    here (`clamp_passthrough`); the depth output carries no gradient;
  * a third one, on by default (`clamp_grad="reference"`): outside 1.3 x the field of view the backward recomputes the
    clamped t.x, t.y and treats them as constants in J (backward.cu:172-176), and zeroes only the direct dL/dt.x, dL/dt.y
    (x_grad_mul / y_grad_mul, :262-264) -- it drops d(clamp(t.x / t.z) * t.z)/dt.z = +-lim, which autograd of the forward
    expression keeps.  Here: the value entering J on a clamped axis is (+-lim * t.z).detach().  `clamp_grad="true"` is the
    forward expression differentiated as written; the forward VALUES of the two modes are identical;
  * a fourth: the gradient of the conic (the inverse of the 2-D covariance) with respect to that covariance is computed with
    1 / (det^2 + 1e-7) in place of 1 / det^2 (backward.cu:203-212), i.e. scaled by det^2 / (det^2 + 1e-7) -- 1.2e-5 relative
    for the smallest footprints (det -> 0.09), which the fp64 comparison with the oracle resolves (`_scale_grad`);
  * a fifth: dL/dscales is the gradient with respect to scale_modifier * scales -- computeCov3D's backward forms s = mod * scale
    and returns dL/ds (backward.cu:295, :323-325), dropping the chain rule's factor mod.  Invisible at scale_modifier = 1.

One projection (`project_gaussians`) and one pair loop (`blend_pairs`) serve every torch helper of the rasterizer's tests: project() /
render() here (the camera a dict of constant arrays, float64), posegrad_math.render (the camera as leaf tensors, per-Gaussian terms),
distort_math, features_math, contrib_math, absgrad_math and aa_math.comp are adapters that add what is theirs -- the median depth and
the statistics here, the distortion sums, the contribution table.  Both compute in the dtype of their inputs.

The decisions contract.  Everything discrete lives in one flat dict of tensors: of the projection `clx`, `cly`, `sx`, `sy` (frustum
clamp and its sign), `vis`, `idx` (the visible Gaussians in depth order: view-space z, ties by index), `rect` (their tile rectangles),
`floor` (anti-aliasing, only with cfg["aa"]) and `colpos` (the colour clamp, only with shs); of the pair loop `listed`, `ok`, `live`.
decisions=None: the function decides on detached values in its own dtype and returns its part of the dict.  decisions given: it
replays them, reads only its own keys and writes nothing -- float32 on a float64 pass's decisions is what fp32 rounding alone does to
the function (the `ref32` of conftest.grad_tol), and a second float64 pass on them is bit-equal to the first.  `ambiguous` flags every
pixel in which a decision sits within fp32 rounding of its threshold -- the caller zeroes the upstream gradient there and skips those
pixels, so an fp32 implementation is never asked to reproduce a coin flip."""
from __future__ import annotations

import math

import numpy as np
import torch

PI = math.pi
# the function's constants are the reference's fp32 literals (0.3f, 0.99f, 1.0f / 255.0f, 0.0001f, 0.0000001f, 0.2f, 1.3f)
F32 = lambda v: float(np.float32(v))      # noqa: E731
C_DILATE, C_AMAX, C_AMIN, C_TMIN, C_WEPS, C_NEAR, C_LIM = F32(0.3), F32(0.99), float(np.float32(1.0) / np.float32(255.0)), F32(0.0001), F32(0.0000001), F32(0.2), F32(1.3)
AA_FLOOR = F32(0.000025)                  # the anti-aliasing factor's floor (tests/aa_math.py)
# real spherical-harmonics normalisation constants from their closed forms, rounded to fp32 like the kernel's literals
# (auxiliary.h:22-39 holds them as float)
SH_C0 = F32(0.5 * math.sqrt(1.0 / PI))
SH_C1 = F32(math.sqrt(3.0 / (4.0 * PI)))
SH_C2 = tuple(F32(v) for v in (0.5 * math.sqrt(15.0 / PI), -0.5 * math.sqrt(15.0 / PI), 0.25 * math.sqrt(5.0 / PI), -0.5 * math.sqrt(15.0 / PI),
                               0.25 * math.sqrt(15.0 / PI)))
SH_C3 = tuple(F32(v) for v in (-0.25 * math.sqrt(35.0 / (2.0 * PI)), 0.5 * math.sqrt(105.0 / PI), -0.25 * math.sqrt(21.0 / (2.0 * PI)),
                               0.25 * math.sqrt(7.0 / PI), -0.25 * math.sqrt(21.0 / (2.0 * PI)), 0.25 * math.sqrt(105.0 / PI),
                               -0.25 * math.sqrt(35.0 / (2.0 * PI))))


def sh_colour(deg: int, sh: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """Real spherical harmonics up to degree 3, sh [P, M, 3], unit directions d [P, 3] -> [P, 3]."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    c = SH_C0 * sh[:, 0]
    if deg > 0:
        c = c - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        c = (c + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2.0 * zz - xx - yy) * sh[:, 6]
             + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
        if deg > 2:
            c = (c + SH_C3[0] * y * (3.0 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
                 + SH_C3[2] * y * (4.0 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[:, 12]
                 + SH_C3[4] * x * (4.0 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
                 + SH_C3[6] * x * (xx - 3.0 * yy) * sh[:, 15])
    return c


def rotation_matrix(q: torch.Tensor) -> torch.Tensor:
    """Rotation matrix of the quaternion (r, x, y, z) AS GIVEN (no normalisation)."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def grad64(x: torch.Tensor) -> np.ndarray:
    """x.grad as float64 numpy; zeros where autograd never reached x."""
    return np.zeros(tuple(x.shape)) if x.grad is None else x.grad.double().numpy()


def camera_cfg(cam, **more):
    """The constants of a camera as project_gaussians takes them: sizes, and the focal tangents as floats like the entry points' arguments."""
    return dict(W=int(cam["image_width"]), H=int(cam["image_height"]), tanx=F32(cam["tanfovx"]), tany=F32(cam["tanfovy"]), **more)


def _scale_grad(x: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """x itself, with the gradient arriving through this copy multiplied by the constant f."""
    y = x.clone()
    if y.requires_grad:
        y.register_hook(lambda g: g * f)
    return y


def _own_copies(x, P):
    e = x.unsqueeze(0).expand((P,) + tuple(x.shape)) * 1.0      # one row per Gaussian, each with its own gradient
    if e.requires_grad:
        e.retain_grad()
    return e


def _frustum_clamped(u, tz, lim, D, axis, decide, clamp_grad):
    """t.x (or t.y) as it enters J: itself, in the form (u / t.z) * t.z, or +-lim * t.z outside 1.3 x the field of view."""
    r = u / tz
    if decide:
        D["cl" + axis], D["s" + axis] = r.detach().abs() > lim, torch.sign(r.detach())
    c = D["s" + axis].to(u.dtype) * lim * tz
    return torch.where(D["cl" + axis], c.detach() if clamp_grad == "reference" else c, r * tz)


def project_gaussians(t, V, Pm, campos, cfg, *, ndc_offset=None, clamp_grad="reference", per=False, halve=None, decisions=None):
    """THE projection, in the dtype of its inputs.  t: dict of tensors -- means3D [P,3], (scales, rotations) or cov3D [P,6], and optionally
    opacities [P,1] and (shs [P,M,3] or rgb [P,3]).  V, Pm [4,4], campos [3] (None without shs): the camera as tensors, leaves or not.
    cfg: camera_cfg's constants + scale_modifier, deg, aa (each optional).  ndc_offset: the means2D sink added to ndc.xy.  clamp_grad:
    "reference" (a frustum-clamped t.x / t.y enters J as a constant, backward.cu:172-176, :262-264) or "true".  per: every Gaussian gets its
    own copy of the three camera tensors ([P,4,4], [P,4,4], [P,3], `per` in the result), whose .grad rows are the Gaussians' terms of the
    camera's gradient.  halve="JW": the gradient reaching viewmatrix through the rotation inside J W times 0.5 (a wrong reference on purpose).
    decisions: None = decide here (the module docstring's contract), or an earlier pass's dict.
    Returns dict(pix [P,2], conic [P,3], depth [P], cov2 = (a, b, c) dilated, Sigma [P,3,3], o [P], col [P,3], col_margin, per, W, H,
    sorted = the visible Gaussians' (pix, conic, o, col, z, rect) in depth order, decisions, disc = the discrete quantities as numpy (deciding
    pass only): vis, radius, rect, tiles, radius_margin, rect_margin, clamped)."""
    assert clamp_grad in ("reference", "true") and halve in (None, "JW"), (clamp_grad, halve)
    m = t["means3D"]
    dt, P, W, H = m.dtype, m.shape[0], cfg["W"], cfg["H"]
    decide = decisions is None
    D = {} if decide else decisions
    fx, fy = W / (2.0 * cfg["tanx"]), H / (2.0 * cfg["tany"])                # rasterizer_impl.cu:222-223
    ph = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
    if per:
        Ve, Pe, Ce = _own_copies(V, P), _own_copies(Pm, P), _own_copies(campos, P)
        tv = torch.einsum("pr,prc->pc", ph, Ve)[:, :3]
        hom = torch.einsum("pr,prc->pc", ph, Pe)
        Wr = Ve[:, :3, :3].transpose(1, 2)
    else:
        Ve, Pe, Ce = None, None, campos
        tv = (ph @ V)[:, :3]                                                  # transposed storage: row vector @ V; view space
        hom = ph @ Pm
        Wr = V[:3, :3].T                                                      # world -> view rotation (math layout)
    pw = 1.0 / (hom[:, 3] + C_WEPS)
    ndc = hom[:, :2] * pw[:, None]
    if ndc_offset is not None:
        ndc = ndc + ndc_offset                                               # gradient sink for the screen-space mean
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)
    if "cov3D" in t:
        c = t["cov3D"]
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], dim=1).reshape(-1, 3, 3)
    else:
        mod = cfg.get("scale_modifier", 1.0)
        s_mod = mod * t["scales"]
        if mod != 1.0:
            s_mod = _scale_grad(s_mod, 1.0 / mod)                             # dL/dscales as the reference's: of mod * scale
        Mx = rotation_matrix(t["rotations"]) * s_mod[:, None, :]              # R @ diag(s)
        Sigma = Mx @ Mx.transpose(1, 2)
    tz = tv[:, 2]
    # (x entirely before y: t.z's gradient is a sum of nearly cancelling terms that autograd adds in reverse order of creation)
    txc = _frustum_clamped(tv[:, 0], tz, C_LIM * cfg["tanx"], D, "x", decide, clamp_grad)
    tyc = _frustum_clamped(tv[:, 1], tz, C_LIM * cfg["tany"], D, "y", decide, clamp_grad)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * txc / (tz * tz), zero, fy / tz, -fy * tyc / (tz * tz)], dim=1).reshape(-1, 2, 3)
    if halve == "JW":
        Wr = _scale_grad(Wr, 0.5)
    A = J @ Wr
    cov2 = A @ Sigma @ A.transpose(1, 2)
    c00, c11 = cov2[:, 0, 0], cov2[:, 1, 1]
    a, b, c2 = c00 + C_DILATE, cov2[:, 0, 1], c11 + C_DILATE
    with torch.no_grad():
        det0 = a * c2 - b * b
        reg = det0 * det0 / (det0 * det0 + C_WEPS)
    ar, br, cr = _scale_grad(a, reg), _scale_grad(b, reg), _scale_grad(c2, reg)
    det = ar * cr - br * br
    conic = torch.stack([cr / det, -br / det, ar / det], dim=1)
    disc = None
    if decide:
        with torch.no_grad():
            mid = 0.5 * (a + c2)
            r_real = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1)))
            radius = torch.ceil(r_real)
            gx, gy = (W + 15) // 16, (H + 15) // 16
            trunc = torch.trunc                                               # (int) cast
            x0 = torch.clamp(trunc((pix[:, 0] - radius) / 16.0), 0, gx); x1 = torch.clamp(trunc((pix[:, 0] + radius + 15.0) / 16.0), 0, gx)
            y0 = torch.clamp(trunc((pix[:, 1] - radius) / 16.0), 0, gy); y1 = torch.clamp(trunc((pix[:, 1] + radius + 15.0) / 16.0), 0, gy)
            tiles = (x1 - x0) * (y1 - y0)
            vis = (tz > C_NEAR) & (det != 0.0) & (tiles > 0)
            # depth order as the 64-bit key sort gives it inside any tile: by view-space z, ties by index (stable)
            idx = torch.nonzero(vis)[:, 0]
            idx = idx[torch.as_tensor(np.lexsort((idx.numpy(), tz[idx].numpy())))]
            rect = torch.stack([x0, y0, x1, y1], 1)
            D.update(vis=vis, idx=idx, rect=rect[idx])
            # how close the discrete decisions are to flipping under fp32 rounding of their inputs
            edge = lambda v: torch.abs(v - torch.round(v))      # noqa: E731
            rect_margin = torch.minimum(torch.minimum(edge((pix[:, 0] - radius) / 16.0), edge((pix[:, 0] + radius + 15.0) / 16.0)),
                                        torch.minimum(edge((pix[:, 1] - radius) / 16.0), edge((pix[:, 1] + radius + 15.0) / 16.0)))
            disc = dict(vis=vis.numpy(), radius=(radius * vis).numpy().astype(np.int64), rect=rect.numpy().astype(np.int64),
                        tiles=(tiles * vis).numpy().astype(np.int64), radius_margin=edge(r_real).numpy(), rect_margin=rect_margin.numpy(),
                        clamped=(D["clx"] | D["cly"]).numpy())
    o = col = col_margin = None
    if "opacities" in t:
        o = t["opacities"].reshape(-1)
        if cfg.get("aa"):                                                     # o * sqrt(max(AA_FLOOR, det(cov2D) / det(cov2D + 0.3 I)))
            rho = (c00 * c11 - b * b) / (a * c2 - b * b)
            if decide:
                D["floor"] = (rho <= AA_FLOOR).detach()
            o = o * torch.where(D["floor"], torch.full_like(rho, AA_FLOOR ** 0.5), torch.sqrt(torch.where(D["floor"], torch.ones_like(rho), rho)))
    if "rgb" in t:
        col, col_margin = t["rgb"], torch.ones((P,), dtype=dt)
    elif "shs" in t:
        d = m - Ce
        raw = sh_colour(int(cfg.get("deg", 0)), t["shs"], d / torch.linalg.norm(d, dim=1, keepdim=True)) + 0.5
        if decide:
            D["colpos"] = (raw > 0.0).detach()
        col = torch.where(D["colpos"], raw, torch.zeros_like(raw))           # max(SH + 0.5, 0)
        col_margin = raw.detach().abs().min(dim=1).values
    idx = D["idx"]
    take = lambda x: None if x is None else x[idx]      # noqa: E731
    return dict(pix=pix, conic=conic, depth=tz, cov2=(a, b, c2), Sigma=Sigma, o=o, col=col, col_margin=col_margin, per=(Ve, Pe, Ce) if per else None,
                sorted=dict(pix=pix[idx], conic=conic[idx], o=take(o), col=take(col), z=tz[idx], rect=D["rect"]), decisions=D, disc=disc, W=W, H=H)


def clamp_passthrough(alpha: torch.Tensor, hi: float) -> torch.Tensor:
    return alpha + (torch.clamp(alpha, max=hi) - alpha).detach()


def blend_pairs(g, bg, W, H, *, decisions=None, z0_relative=False, fp32_eps=4e-6):
    """THE pair loop, in the dtype of its inputs.  g: project_gaussians' `sorted` -- Gaussians in depth order (pix [K,2], conic [K,3], o [K],
    z [K], rect [K,4] tile rectangles, col [K,3] or None); pixels row-major, N = H W.  decisions: None = decide here (listed, ok, live; the
    module docstring's contract) or an earlier pass's.  z0_relative: `z_rel` is the depth relative to z0, the depth of the first Gaussian
    listed for the pixel's tile (the kernels' association); otherwise z itself.
    Returns dict(w [N,K] = alpha T the blending weights, live, ok, listed, T_incl, T_excl, power, alpha_raw [N,K], T_final [N], z_rel,
    color [3,H,W] (col given), acc_depth [H,W], alpha [H,W], decisions, ambiguous [N] bool (deciding pass: a decision within fp32 rounding
    of its threshold))."""
    pix, conic, o, z, col = g["pix"], g["conic"], g["o"], g["z"], g["col"]
    dt = pix.dtype
    decide = decisions is None
    D = {} if decide else decisions
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    px, py = xs.reshape(-1, 1), ys.reshape(-1, 1)                            # [N, 1]
    dx, dy = pix[None, :, 0] - px, pix[None, :, 1] - py
    power = -0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) - conic[None, :, 1] * dx * dy
    alpha_raw = o[None, :] * torch.exp(power)
    alpha = clamp_passthrough(alpha_raw, C_AMAX)
    if decide:
        with torch.no_grad():
            rect = g["rect"]
            tx, ty = torch.div(px, 16, rounding_mode="floor"), torch.div(py, 16, rounding_mode="floor")
            D["listed"] = (tx >= rect[None, :, 0]) & (tx < rect[None, :, 2]) & (ty >= rect[None, :, 1]) & (ty < rect[None, :, 3])   # [N, K]
            D["ok"] = D["listed"] & (power <= 0.0) & (alpha >= C_AMIN)
    listed, ok = D["listed"], D["ok"]
    one_minus = torch.where(ok, 1.0 - alpha, torch.ones_like(alpha))
    T_incl = torch.cumprod(one_minus, dim=1)
    T_excl = T_incl / one_minus                                              # the transmittance in front of the pair
    amb_pix = None
    if decide:
        with torch.no_grad():
            # the pair that would push T below 1e-4 ends the pixel: it is finished at the FIRST such pair (T_incl is monotone)
            D["live"] = ok & (T_incl >= C_TMIN)
            # ambiguity of the decisions under fp32 rounding (relative eps on alpha and T, absolute on power)
            scale_q = conic[None, :, 0].abs() * dx * dx + conic[None, :, 2].abs() * dy * dy + 2 * conic[None, :, 1].abs() * (dx * dy).abs()
            amb = listed & ((power.abs() <= fp32_eps * (1.0 + scale_q)) |
                            ((power <= 0.0) & ((alpha_raw / C_AMIN - 1.0).abs() <= 8 * fp32_eps * (1.0 + scale_q))))
            amb = amb | (ok & ((T_incl / C_TMIN - 1.0).abs() <= 64 * fp32_eps))
            amb_pix = amb.any(dim=1)
    live = D["live"]
    w = torch.where(live, alpha * T_excl, torch.zeros_like(alpha))
    colour = None if col is None else w @ col                                # [N, 3]
    T_final = torch.where(live, one_minus, torch.ones_like(alpha)).prod(dim=1)
    if col is not None:
        colour = (colour + T_final[:, None] * t64(bg).to(dt)[None, :]).T.reshape(3, H, W)
    z_rel = z[None, :]
    if z0_relative:
        with torch.no_grad():
            z0 = torch.where(listed.any(dim=1), z.detach()[torch.argmax(listed.to(torch.int8), dim=1)], torch.zeros((), dtype=dt))
        z_rel = z_rel - z0[:, None]
    return dict(w=w, live=live, ok=ok, listed=listed, T_incl=T_incl, T_excl=T_excl, power=power, alpha_raw=alpha_raw, T_final=T_final, z_rel=z_rel,
                color=colour, acc_depth=(w @ z).reshape(H, W), alpha=(1.0 - T_final).reshape(H, W), decisions=D, ambiguous=amb_pix)


def project(means3D, scales, rotations, cam, scale_modifier=1.0, cov3D=None, ndc_offset=None, clamp_grad="reference", deg=0, **blended):
    """project_gaussians in float64 for a camera given as a dict of arrays (constants), deciding here.  `blended`: opacities, shs or rgb."""
    t = dict(means3D=means3D, **blended)
    t.update(dict(scales=scales, rotations=rotations) if cov3D is None else dict(cov3D=cov3D))
    return project_gaussians(t, t64(cam["viewmatrix"]), t64(cam["projmatrix"]), t64(cam["campos"]) if "shs" in t else None,
                             camera_cfg(cam, scale_modifier=scale_modifier, deg=deg), ndc_offset=ndc_offset, clamp_grad=clamp_grad)


def _tile_list_max(rect, W, H):
    """The longest per-tile list: how many visible Gaussians' rectangles cover the fullest 16 x 16 tile."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    n = np.zeros((gy, gx), np.int64)
    for x0, y0, x1, y1 in rect:
        n[y0:y1, x0:x1] += 1
    return int(n.max())


def render(means3D, scales, rotations, opacities, shs, sh_degree, cam, bg, *, colors_precomp=None, cov3D=None,
           scale_modifier=1.0, ndc_offset=None, fp32_eps=4e-6, clamp_grad="reference"):
    """Returns dict(color [3,H,W], depth [H,W], final_T [H,W], ambiguous [H,W] bool, proj=...).  clamp_grad: see project_gaussians()."""
    pr = project(means3D, scales, rotations, cam, scale_modifier, cov3D, ndc_offset, clamp_grad, int(sh_degree), opacities=opacities,
                 **(dict(shs=shs) if colors_precomp is None else dict(rgb=colors_precomp)))
    W, H, g, idx = pr["W"], pr["H"], pr["sorted"], pr["decisions"]["idx"]
    bl = blend_pairs(g, bg, W, H, fp32_eps=fp32_eps)
    live, T_incl, T_excl = bl["live"], bl["T_incl"], bl["T_excl"]
    with torch.no_grad():
        zs = g["z"]
        gap = (zs[1:] - zs[:-1]).min().item() if len(zs) > 1 else 1.0
        # median depth: the contributing pair at which T crosses 0.5 (forward.cu:368-372); default 15
        T_after = torch.where(live, T_incl, torch.full_like(T_incl, 2.0))
        T_prev = torch.where(live, T_excl, torch.full_like(T_incl, -1.0))
        cross = live & (T_prev > 0.5) & (T_after < 0.5)
        has = cross.any(dim=1)
        first = torch.argmax(cross.to(torch.int8), dim=1)
        depth = torch.where(has, zs[first], torch.full((H * W,), 15.0, dtype=torch.float64))
        amb_pix = bl["ambiguous"] | ((live & (((T_prev - 0.5).abs() <= 64 * fp32_eps) | ((T_after - 0.5).abs() <= 64 * fp32_eps))).any(dim=1))
    return dict(color=bl["color"], depth=depth.reshape(H, W), final_T=bl["T_final"].reshape(H, W),
                ambiguous=amb_pix.reshape(H, W).numpy(), proj=pr, order=idx.numpy(), min_depth_gap=gap,
                colour_clamp_margin=pr["col_margin"].numpy(), n_live=live.sum(dim=1).reshape(H, W).numpy(),
                clamped_pairs=int((live & (bl["alpha_raw"] > C_AMAX)).sum().item()),
                tile_list_max=_tile_list_max(g["rect"].numpy().astype(np.int64), W, H),
                stopped=((bl["ok"] & ~live).any(dim=1)).reshape(H, W).numpy(), w=bl["w"], live=live)
