"""Normal consistency, host side (no GPU): tests/normal_math.py against torch.autograd of the fp64 torch composition it restates (gsplat's
slicing form of depth_to_normal; the reference's rotation matrix), the planes whose normals are known, the per-Gaussian normal against the
eigenvector of tests/math_renderer.py's covariance, every rule's edge, the C ABI of gsrast_gaussian_normals_* / gsrast_depth_normal_* /
gsrast_normal_loss_* (declared, exported, bound, every argument error refused before any device call) and fused_normal.py's refusals.

There is no golden file: gsplat is not a dependency of the project, so the restatement is pinned to the definition in include/gsrast.h, to
torch's own autograd and to closed forms."""
import os
import re

import numpy as np
import pytest
import torch

import math_renderer as mr
import normal_math as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsrast_gaussian_normals_forward", "gsrast_gaussian_normals_backward", "gsrast_depth_normal_forward", "gsrast_depth_normal_backward",
           "gsrast_normal_loss_scratch_bytes", "gsrast_normal_loss_forward", "gsrast_normal_loss_backward")
IMAGES = [(1, 1), (2, 5), (3, 3), (5, 4), (17, 9), (67, 18)]
TX, TY = nm.TANFOV


def close(got, want, rel=1e-12):
    """agreement to `rel` of the tensor's largest entry"""
    want = np.asarray(want, np.float64)
    return np.asarray(got).shape == want.shape and float(np.abs(np.asarray(got, np.float64) - want).max(initial=0.0)) <= rel * float(np.abs(want).max(initial=0.0))


@pytest.mark.parametrize("W,H", IMAGES)
@pytest.mark.parametrize("kind", nm.FIELDS)
@pytest.mark.parametrize("weight", [False, True])
def test_image_restatement_equals_autograd_in_fp64(kind, W, H, weight):
    c = nm.make_image_case(kind, W, H)
    got, want = nm.numpy_image_run(c, weight), nm.torch_image_run(c, torch.float64, weight)
    for k, w in want.items():
        assert np.isfinite(got[k]).all() and close(got[k], w), k
    if W < 3 or H < 3:
        assert not got["n"].any() and not got["d_depth"].any() and not got["dd"].any() and not got["dN"].any() and got["loss"] == 1.0


@pytest.mark.parametrize("P", [0, 1, 5, 257])
@pytest.mark.parametrize("cam_index", [1, 4])
def test_gaussian_restatement_equals_autograd_in_fp64(P, cam_index, scenes):
    c = nm.make_gaussian_case(P, scenes.camera(cam_index, 6, 70, 45), seed=cam_index)
    got, want = nm.numpy_gaussian_run(c), nm.torch_gaussian_run(c, torch.float64)
    for k, w in want.items():
        assert np.isfinite(got[k]).all() and close(got[k], w), k
    if P >= 4:
        # unit length, as far as the camera's fp32 rotation is orthonormal (the matrix is rounded to fp32: a few 2^-24 per entry)
        assert np.abs(np.linalg.norm(np.delete(got["n"], [1, 2], axis=0), axis=1) - 1.0).max() <= 4 * 2.0 ** -23


def test_fronto_parallel_plane_gives_0_0_minus_1():
    W, H = 17, 9
    n = nm.depth_to_normal(np.full((H, W), 2.5), TX, TY)
    assert np.abs(n[:, 1:-1, 1:-1] - np.array([0.0, 0.0, -1.0])[:, None, None]).max() <= 1e-15
    assert not n[:, 0].any() and not n[:, -1].any() and not n[:, :, 0].any() and not n[:, :, -1].any()      # the one-pixel border
    t = nm.torch_depth_to_normal(torch.full((H, W), 2.5, dtype=torch.float64), TX, TY).numpy()
    assert np.abs(t - n).max() <= 1e-15


@pytest.mark.parametrize("z0,alpha,beta", [nm.PLANE, (1.0, -0.7, 0.0), (4.0, 0.0, 1.1), (0.8, 0.45, 0.6)])
def test_tilted_plane_gives_its_own_normal(z0, alpha, beta):
    """z = z0 + alpha x + beta y in view space: (alpha, beta, -1) / |.| at every pixel off the border -- central differences of points ON a
    plane lie IN the plane, whatever their spacing"""
    W, H = 33, 17
    d = nm.plane_depth(W, H, z0, alpha, beta)
    assert (d > 0.2).all()
    n = nm.depth_to_normal(d, TX, TY)
    want = np.array([alpha, beta, -1.0]) / np.sqrt(alpha * alpha + beta * beta + 1.0)
    assert np.abs(n[:, 1:-1, 1:-1] - want[:, None, None]).max() <= 1e-12


def test_gaussian_normal_is_the_covariances_smallest_axis(scenes):
    """the eigenvector of math_renderer's Sigma = R S^2 R^T with the eigenvalue min(s)^2, rotated to view space, facing the camera.  The
    bound: eigh's eigenvector error is ~ eps |Sigma| / gap, the generator keeps the gap at >= 10 % of the eigenvalue."""
    cam = scenes.camera(4, 6, 70, 45)
    c = nm.make_gaussian_case(200, cam, special=False)
    q = mr.t64(c["rotations"])
    M = mr.rotation_matrix(q / q.norm(dim=1, keepdim=True)) * mr.t64(c["scales"])[:, None, :]      # math_renderer.project_gaussians: R diag(s)
    lam, vec = np.linalg.eigh((M @ M.transpose(1, 2)).numpy())
    assert np.abs(lam[:, 0] - c["scales"].astype(np.float64).min(1) ** 2).max() <= 1e-15
    V = c["viewmatrix"].astype(np.float64)
    n = vec[:, :, 0] @ V[:3, :3]
    p = c["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    n = np.where(((n * p).sum(1) > 0)[:, None], -n, n)
    got = nm.gaussian_normals(c["means3D"], c["scales"], c["rotations"], c["viewmatrix"])
    assert np.abs(got - n).max() <= 1e-12 and ((got * p).sum(1) < 0).all()


def test_tie_flip_and_zero_quaternion_rules():
    V = np.eye(4)
    V[3, :3] = (0.0, 0.0, 5.0)      # the camera 5 units in front of the origin, looking down +z
    q = np.array([[1.0, 0.0, 0.0, 0.0]])
    run = lambda m, s, qq=q: nm.gaussian_normals(np.array([m], float), np.array([s], float), qq, V)[0]  # noqa: E731
    # a tie takes the lowest index
    assert np.array_equal(run((0.3, 0.2, 0), (0.1, 0.1, 0.5)), [-1, 0, 0]) and np.array_equal(run((0.3, 0.2, 0), (0.5, 0.1, 0.1)), [0, -1, 0])
    assert np.array_equal(run((0.3, 0.2, 0), (0.1, 0.1, 0.1)), [-1, 0, 0]) and np.array_equal(run((0.3, 0.2, 0), (0.5, 0.2, 0.1)), [0, 0, -1])
    # the sign: negated where n . p > 0, kept where < 0, and an exact 0 is left as it is
    assert np.array_equal(run((-0.3, 0, 0), (0.1, 0.2, 0.3)), [1, 0, 0]) and np.array_equal(run((0.3, 0, 0), (0.1, 0.2, 0.3)), [-1, 0, 0])
    assert np.array_equal(run((0.0, 0.7, 0), (0.1, 0.2, 0.3)), [1, 0, 0])
    t = lambda a: torch.tensor(np.array([a], float))  # noqa: E731
    assert np.array_equal(nm.torch_gaussian_normals(t((0.0, 0.7, 0)), t((0.1, 0.2, 0.3)), torch.tensor(q), torch.tensor(V)).numpy()[0], [1, 0, 0])
    # |q| = 0 and a non-finite q: a zero normal and a zero gradient; an un-normalised q: the normal of q / |q|, a gradient orthogonal to q
    for bad in ((0, 0, 0, 0), (np.nan, 0, 0, 1), (1, np.inf, 0, 0)):
        qq = np.array([bad], float)
        assert not run((0.3, 0.2, 0), (0.1, 0.2, 0.3), qq).any()
        assert not nm.gaussian_normals_backward(np.array([[0.3, 0.2, 0]]), np.array([[0.1, 0.2, 0.3]]), qq, V, np.ones((1, 3))).any()
    q1 = np.array([[0.5, -0.3, 0.8, 0.1]])
    m, s = np.array([[0.3, 0.2, 0.1]]), np.array([[0.3, 0.05, 0.2]])
    assert np.abs(nm.gaussian_normals(m, s, 37.5 * q1, V) - nm.gaussian_normals(m, s, q1, V)).max() <= 1e-15
    dq = nm.gaussian_normals_backward(m, s, 37.5 * q1, V, np.array([[0.3, -1.0, 0.5]]))
    assert dq.any() and abs((dq * q1).sum()) <= 1e-15 and close(dq * 37.5, nm.gaussian_normals_backward(m, s, q1, V, np.array([[0.3, -1.0, 0.5]])))


def _zero_everywhere(depth, at=None):
    """the normal, dL/dN and both depth gradients are exactly 0 at pixel `at` (None: everywhere), in numpy and in the torch composition"""
    H, W = depth.shape
    rng = np.random.default_rng(3)
    c = dict(tanfov=nm.TANFOV, depth=depth, normal_map=rng.normal(size=(3, H, W)), d_normals=rng.normal(size=(3, H, W)), weight=rng.uniform(0, 1, (H, W)), upstream=0.75)
    for run in (nm.numpy_image_run(c), nm.torch_image_run(c, torch.float64)):
        pick = (lambda a: a) if at is None else (lambda a: a[..., at[1], at[0]])
        assert not pick(run["n"]).any() and not pick(run["dN"]).any() and np.isfinite(run["d_depth"]).all() and np.isfinite(run["dd"]).all()
        if at is None:
            assert not run["d_depth"].any() and not run["dd"].any() and run["loss"] == 1.0
    return nm.numpy_image_run(c)


def test_pixels_without_a_normal_are_exactly_zero():
    W, H = 7, 6
    base = nm.make_depth("wavy", W, H).astype(np.float64)
    assert nm.depth_to_normal(base, TX, TY)[:, 1:-1, 1:-1].any(0).all()
    _zero_everywhere(np.zeros((H, W)))                                   # all-zero depth: nothing is covered
    _zero_everywhere(np.full((H, W), 1e-7))                              # c . c = (d^2 du dv)^2 ~ 1e-31 < 1e-24 at every pixel
    for x, y in ((0, 2), (W - 1, 3), (3, 0), (2, H - 1), (0, 0)):        # the border
        _zero_everywhere(base, (x, y))
    for bad in (0.0, -1.0, np.nan):                                      # a neighbour that is not > 0: its four neighbours lose their normal, it keeps its own
        d = base.copy()
        d[3, 3] = bad
        for x, y in ((2, 3), (4, 3), (3, 2), (3, 4)):
            run = _zero_everywhere(d, (x, y))
        assert run["n"][:, 3, 3].any() and run["d_depth"][3, 3] == 0.0 and run["dd"][3, 3] == 0.0
        assert run["n"][:, 1, 1].any() and run["d_depth"][1, 2] != 0.0


def test_symbols_are_declared_exported_and_bound(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    import capi_header
    L = rast._C.lib()
    protos = capi_header.prototypes()
    for name in SYMBOLS:
        assert name in protos and name in rast._C.SIGNATURES and name in rast._C.EXPORTS and getattr(L, name).argtypes is not None, name
    assert not any("normal" in s for s in capi_header.structs())      # plain scalars and pointers: no descriptor
    text = capi_header.text()
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6 and re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == 34 and not any("normal" in n for n in names)      # the profile table is unchanged
    units = {f: open(os.path.join(ROOT, "saro-gs_amd", "csrc", f)).read() for f in ("gsrast_capi.hip", "gsrast_train.hip")}
    assert '#include "gsrast_normal.h"' in units["gsrast_train.hip"] and "gsrast_normal.h" not in units["gsrast_capi.hip"]


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    L = rast._C.lib()
    one = 256      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731

    def gfwd(P=5, m=one, s=one, q=one, V=one, n=one):
        return L.gsrast_gaussian_normals_forward(P, m, s, q, V, n, None)

    def gbwd(P=5, m=one, s=one, q=one, V=one, g=one, dq=one):
        return L.gsrast_gaussian_normals_backward(P, m, s, q, V, g, dq, None)

    for who, call, pointers in (("gaussian_normals_forward", gfwd, "msqVn"), ("gaussian_normals_backward", gbwd, "msqVg")):
        assert call(P=-1) == -1 and err() == f"{who}: negative P"
        for p in pointers:
            assert call(**{p: None}) == -1 and err() == f"{who}: NULL required pointer", p
        assert call(P=0) == 0      # no row, no launch
    assert gfwd(P=0, m=None, s=None, q=None, n=None) == 0
    assert gbwd(dq=None) == -1 and err() == "gaussian_normals_backward: dL_drotations is NULL (it is the only gradient)"

    def dfwd(W=64, H=48, tx=0.5, ty=0.4, d=one, n=one):
        return L.gsrast_depth_normal_forward(W, H, tx, ty, d, n, None)

    def dbwd(W=64, H=48, tx=0.5, ty=0.4, d=one, g=one, dd=one):
        return L.gsrast_depth_normal_backward(W, H, tx, ty, d, g, dd, None)

    def lfwd(W=64, H=48, tx=0.5, ty=0.4, N=one, d=one, w=one, loss=one, scratch=one):
        return L.gsrast_normal_loss_forward(W, H, tx, ty, N, d, w, loss, scratch, None)

    def lbwd(W=64, H=48, tx=0.5, ty=0.4, N=one, d=one, w=one, up=one, dN=one, dd=one):
        return L.gsrast_normal_loss_backward(W, H, tx, ty, N, d, w, up, dN, dd, None)

    bad_images = [(dict(W=0), "W and H must be >= 1"), (dict(H=0), "W and H must be >= 1"), (dict(W=-3), "W and H must be >= 1"), (dict(H=-1), "W and H must be >= 1"),
                  (dict(W=32769), "W and H must be at most 32768"), (dict(H=40000), "W and H must be at most 32768")]
    bad_tans = [dict(tx=0.0), dict(ty=0.0), dict(tx=-0.5), dict(ty=-1e-9), dict(tx=float("nan")), dict(ty=float("nan")), dict(tx=float("inf")), dict(ty=float("inf"))]
    for who, call, pointers in (("depth_normal_forward", dfwd, ("d", "n")), ("depth_normal_backward", dbwd, ("d", "g")),
                                ("normal_loss_forward", lfwd, ("N", "d", "loss")), ("normal_loss_backward", lbwd, ("N", "d", "up"))):
        for bad, text in bad_images:
            assert call(**bad) == -1 and err() == f"{who}: {text}", (who, bad)
        for bad in bad_tans:
            assert call(**bad) == -1 and err() == f"{who}: tanfovx and tanfovy must be finite and > 0", (who, bad)
        for p in pointers:
            assert call(**{p: None}) == -1 and err() == f"{who}: NULL required pointer", (who, p)
    assert dbwd(dd=None) == -1 and err() == "depth_normal_backward: dL_ddepth is NULL (it is the only gradient)"
    assert lbwd(dN=None, dd=None) == -1 and err() == "normal_loss_backward: dL_dnormal_map and dL_ddepth are both NULL"
    assert lfwd(scratch=None) == -1 and err() == "normal_loss_forward: NULL scratch"
    # scratch_bytes: 0 and the reason for a refused size; one fp64 partial per 64 x 16 tile otherwise
    for bad, text in bad_images:
        assert L.gsrast_normal_loss_scratch_bytes(bad.get("W", 64), bad.get("H", 48)) == 0 and err() == f"normal_loss_scratch_bytes: {text}", bad
    assert L.gsrast_normal_loss_scratch_bytes(1, 1) == 512 and L.gsrast_normal_loss_scratch_bytes(64, 16) == 512
    assert L.gsrast_normal_loss_scratch_bytes(1920, 1080) == 30 * 68 * 8 + 64 + 256 and L.gsrast_normal_loss_scratch_bytes(32768, 32768) == 512 * 2048 * 8 + 256


class _Settings:
    def __init__(self, W, H, tanfov=nm.TANFOV, viewmatrix=None):
        self.image_width, self.image_height, (self.tanfovx, self.tanfovy), self.viewmatrix = W, H, tanfov, viewmatrix


def test_python_refusals_need_no_device(monkeypatch):
    import fused_normal as fn
    monkeypatch.setattr(fn._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    W, H, P = 64, 48, 5
    rs = _Settings(W, H, viewmatrix=torch.eye(4))
    d, N, w = torch.ones(H, W), torch.zeros(3, H, W), torch.ones(H, W)
    m, s, q = torch.zeros(P, 3), torch.ones(P, 3), torch.ones(P, 4)
    for call in (lambda: fn.depth_to_normal(d, raster_settings=rs), lambda: fn.normal_consistency_loss(N, d, raster_settings=rs),
                 lambda: fn.gaussian_normals(m, s, q, raster_settings=rs)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="tensor"):
        fn.depth_to_normal(d.numpy(), raster_settings=rs)
    # what is checked once the tensors pass for device tensors: dtype, shape, layout, the settings (the device check stubbed out)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    dn = lambda depth, r=rs: fn.depth_to_normal(depth, raster_settings=r)  # noqa: E731
    loss = lambda NN=N, dd=d, ww=None, r=rs: fn.normal_consistency_loss(NN, dd, raster_settings=r, weight=ww)  # noqa: E731
    gn = lambda mm=m, ss=s, qq=q, r=rs: fn.gaussian_normals(mm, ss, qq, raster_settings=r)  # noqa: E731
    for call, text in ((lambda: dn(d.double()), "float32"), (lambda: dn(d[:, :63]), r"\[48, 64\]"), (lambda: dn(d[None, None]), r"\[48, 64\]"),
                       (lambda: dn(torch.ones(2, H, W)), r"\[1, 48, 64\]"), (lambda: dn(torch.ones(W, H).t()), "contiguous"), (lambda: dn(torch.ones(H, 2 * W)[:, ::2]), "contiguous"),
                       (lambda: loss(NN=N[:2]), r"\[3, 48, 64\]"), (lambda: loss(NN=N.half()), "float32"), (lambda: loss(NN=torch.zeros(H, W, 3).permute(2, 0, 1)), "contiguous"),
                       (lambda: loss(dd=d[:47]), r"\[48, 64\]"), (lambda: loss(dd=d.double()), "float32"), (lambda: loss(ww=w[:, :5]), r"\[48, 64\]"),
                       (lambda: loss(ww=w.double()), "float32"), (lambda: loss(ww=torch.ones(W, H).t()), "contiguous"), (lambda: loss(ww=torch.ones(3, H, W)), r"\[1, 48, 64\]"),
                       (lambda: gn(mm=m[:, :2]), r"\[\*, 3\]"), (lambda: gn(ss=s[:4]), r"\[5, 3\]"), (lambda: gn(qq=q[:, :3]), r"\[5, 4\]"), (lambda: gn(qq=q.double()), "float32"),
                       (lambda: gn(mm=torch.zeros(3, P).t()), "contiguous"), (lambda: gn(r=_Settings(W, H, viewmatrix=np.eye(4))), "viewmatrix"),
                       (lambda: gn(r=_Settings(W, H, viewmatrix=torch.eye(3))), "viewmatrix"), (lambda: gn(r=_Settings(W, H, viewmatrix=torch.eye(4).double())), "float32"),
                       (lambda: dn(d, _Settings(W, H, (0.0, 0.4))), "tanfov"), (lambda: dn(d, _Settings(W, H, (0.5, float("nan")))), "tanfov"),
                       (lambda: dn(d, _Settings(W, H, (float("inf"), 0.4))), "tanfov"), (lambda: dn(torch.ones(1, 40000), _Settings(40000, 1)), "32768"),
                       (lambda: loss(r=_Settings(0, H)), "32768")):
        with pytest.raises(ValueError, match=text):
            call()
    # another device: the tensors of one call live on one GPU
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 1 if getattr(self, "_elsewhere", False) else 0)))
    far = torch.ones(H, W)
    far._elsewhere = True
    for call in (lambda: loss(dd=far), lambda: loss(ww=far)):
        with pytest.raises(RuntimeError, match="is on cuda:1"):
            call()
    farq = torch.ones(P, 4)
    farq._elsewhere = True
    with pytest.raises(RuntimeError, match="is on cuda:1"):
        gn(qq=farq)
    farV = torch.eye(4)
    farV._elsewhere = True
    with pytest.raises(RuntimeError, match="viewmatrix is on cuda:1"):
        gn(r=_Settings(W, H, viewmatrix=farV))
