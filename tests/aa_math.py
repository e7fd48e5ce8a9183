"""The anti-aliasing factor of GSRAST_RENDER_ANTIALIAS (include/gsrast.h), in torch -- a helper of the tests, not a test.

    rho  = det(cov2D) / det(cov2D + 0.3 I)          cov2D: the screen-space covariance BEFORE the 0.3 px^2 dilation
    comp = sqrt(max(FLOOR, rho))                     o_eff = o * comp

`comp` is fp64 and differentiable (torch autograd), built on math_renderer.project: in fp64, cov2 - C_DILATE gives the undilated values
accurately enough.  `comp32` evaluates the same chain in fp32 in the kernel's order (gsrast_preprocess.h: cov2d_eval, aa_rho), as the
fp32 reference of conftest.grad_tol."""
import numpy as np
import torch

import math_renderer as mr

FLOOR = mr.AA_FLOOR


def comp_of_cov2(a, b, c):
    """comp from the DILATED covariance entries (a, b, c) = (c00 + 0.3, c01, c11 + 0.3), any dtype."""
    d = mr.C_DILATE
    det_cov = (a - d) * (c - d) - b * b
    det_h = a * c - b * b
    rho = det_cov / det_h
    return torch.sqrt(torch.clamp(rho, min=FLOOR)), rho


def comp(means3D, scales, rotations, cam, scale_modifier=1.0, cov3D=None, clamp_grad="reference"):
    """fp64 (comp [P], rho [P]) for the scales / rotations form, or for cov3D_precomp ([P,6]: xx xy xz yy yz zz) with cov3D given.
    clamp_grad: math_renderer.project's (how the frustum-clamped t.x / t.y are differentiated)."""
    pr = mr.project(means3D, scales, rotations, cam, scale_modifier, cov3D, clamp_grad=clamp_grad)
    return comp_of_cov2(*pr["cov2"])


def comp32(means3D, scales, rotations, cam, scale_modifier=1.0, cov3D=None, clamp_grad="reference"):
    """(comp, rho) in fp32, the kernel's chain: cov3D = (S R)^T (S R), J W Sigma W^T J^T with the frustum clamp, undilated c00 / c11.
    clamp_grad as in comp: "reference" = a clamped t.x / t.y is a constant of the backward, as in the kernel (preprocess_bwd_kernel)."""
    f = torch.float32
    dev = means3D.device
    V = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float32), device=dev)
    W, H = int(cam["image_width"]), int(cam["image_height"])
    tanx, tany = np.float32(cam["tanfovx"]), np.float32(cam["tanfovy"])
    fx, fy = float(np.float32(W) / (np.float32(2.0) * tanx)), float(np.float32(H) / (np.float32(2.0) * tany))
    p = means3D.to(f)
    t = p @ V[:3, :3] + V[3, :3]
    if cov3D is None:
        Mx = mr.rotation_matrix(rotations.to(f)) * (scale_modifier * scales.to(f))[:, None, :]      # (the quaternion as given, like the kernel)
        Sigma = Mx @ Mx.transpose(1, 2)
    else:
        c = cov3D.to(f)
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    limx, limy = float(np.float32(1.3) * tanx), float(np.float32(1.3) * tany)
    tz = t[:, 2]
    txc = torch.clamp(t[:, 0] / tz, -limx, limx) * tz
    tyc = torch.clamp(t[:, 1] / tz, -limy, limy) * tz
    if clamp_grad == "reference":
        with torch.no_grad():
            clx, cly = (t[:, 0] / tz).abs() > limx, (t[:, 1] / tz).abs() > limy
        txc, tyc = torch.where(clx, txc.detach(), txc), torch.where(cly, tyc.detach(), tyc)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * txc) / (tz * tz), zero, fy / tz, -(fy * tyc) / (tz * tz)], 1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    cov2 = A @ Sigma @ A.transpose(1, 2)
    c00, c01, c11 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det_cov = c00 * c11 - c01 * c01
    det_h = (c00 + 0.3) * (c11 + 0.3) - c01 * c01
    rho = det_cov / det_h
    return torch.sqrt(torch.clamp(rho, min=FLOOR)), rho


def conditioning(means3D, scales, rotations, cam, scale_modifier=1.0, cov3D=None):
    """(c00 c11 + c01^2) / det_h in fp64: how strongly fp32 rounding of the covariance moves rho (the cancellation in det_cov)."""
    with torch.no_grad():
        a, b, c = mr.project(means3D, scales, rotations, cam, scale_modifier, cov3D)["cov2"]
        d = mr.C_DILATE
        return (((a - d) * (c - d)).abs() + b * b) / (a * c - b * b)
