"""-m gpu: normal consistency (csrc/gsrast_normal.h, fused_normal.py) against the fp64 restatement of tests/normal_math.py.

The bar is tests/test_gpu_bilagrid.py's and tests/test_gpu_temporal.py's, per output and gradient tensor T, evaluated per case at run time:
    max|T_hip - T_fp64| <= 4 max|T_torch32 - T_fp64| + 2^-23 max|T_fp64|,
T_torch32 = torch's fp32 CPU run of the composition of tests/normal_math.py (gsplat's slicing form of depth_to_normal, cross, F.normalize,
the mean; the reference's rotation matrix) on the same inputs.  The generators keep every case away from the rules' edges and assert it
(tests/normal_math.py), so no element is left out of a comparison, and a pixel or row without a normal is exactly 0 in every tensor.

Images: every W of (1, 2, 3, 5, 63, 64, 65, 66, 67, 130) with every H of (1, 2, 3, 4, 5, 9, 33, 70) and of TH - 1, TH, TH + 1, TH + 2, 2 TH + 3
for the kernels' tile height TH = 16, on six depth fields (a tilted plane, a smooth wavy surface, a step edge, a rectangle of zeros across a
tile corner, a NaN pixel, a negative pixel), with and without a weight.

Worst ratio e_hip / bar per tensor over the whole file, as measured on an MI355X (the summary lines of the tests, -s):
    n 0.118   d_depth 0.137   loss 0.162   dN 0.155   dd 0.107   d_rotations 0.056      (profiles/normal_overhead.json: worst_e_hip_over_bar)
    end to end: rotations 0.065   means3D 0.046   scales 0.066   opacities 0.031
The kernels evaluate in fp64 and round once, so e_hip is the rounding of the result; the ratios are 2^-24 against the bar."""
import itertools

import numpy as np
import pytest
import torch

import normal_math as nm

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SIZES = list(itertools.product(nm.WIDTHS, nm.HEIGHTS))
GAUSSIAN_ROWS = (0, 1, 63, 64, 65, 4099)


def bar_check(label, got, f64, t32, worst):
    """The bar of this file's docstring on every tensor of `got`; the worst ratio per tensor is kept in `worst` for the summary line."""
    bad = []
    for k, g in got.items():
        truth = np.asarray(f64[k], np.float64)
        g = np.asarray(g, np.float64).reshape(truth.shape)
        assert np.isfinite(truth).all() and np.isfinite(g).all(), (label, k)
        e_hip = float(np.abs(g - truth).max(initial=0.0))
        e_ref = float(np.abs(np.asarray(t32[k], np.float64).reshape(truth.shape) - truth).max(initial=0.0))
        bound = 4 * e_ref + ULP * float(np.abs(truth).max(initial=0.0))
        if bound > 0 and e_hip / bound > worst.get(k, (0.0,))[0]:
            worst[k] = (e_hip / bound, e_hip, e_ref, label)
        if not e_hip <= bound:
            bad.append((k, e_hip, e_ref, bound))
    assert not bad, (label, bad)


def summary(what, worst):
    for k, (ratio, e_hip, e_ref, label) in worst.items():
        print(f"normal {what} {k}: worst e_hip / bar {ratio:.3f} (e_hip {e_hip:.3e}, e_torch32 {e_ref:.3e}) at {label}")


class Settings:
    """What the three calls read of a GaussianRasterizationSettings."""
    def __init__(self, W, H, tanfov, viewmatrix=None):
        self.image_width, self.image_height, (self.tanfovx, self.tanfovy), self.viewmatrix = W, H, tanfov, viewmatrix


_REFERENCES = {}


def image_reference(kind, W, H):
    """(case, {weight: fp64 truth}, {weight: torch fp32}) of one image: computed once, shared by the tests, never changed"""
    key = (kind, W, H)
    if key not in _REFERENCES:
        c = nm.make_image_case(kind, W, H)
        _REFERENCES[key] = (c, {w: nm.numpy_image_run(c, w) for w in (False, True)}, {w: nm.torch_image_run(c, torch.float32, w) for w in (False, True)})
    return _REFERENCES[key]


def gaussian_reference(P, cam_index, scenes):
    key = ("gaussians", P, cam_index)
    if key not in _REFERENCES:
        c = nm.make_gaussian_case(P, scenes.camera(cam_index, 6, 70, 45), seed=cam_index)
        _REFERENCES[key] = (c, nm.numpy_gaussian_run(c), nm.torch_gaussian_run(c, torch.float32))
    return _REFERENCES[key]


def fused_image(c, gpu, weight, lead=False, need=(True, True), noncontiguous=False):
    """depth_to_normal and normal_consistency_loss of a case, forward and backward; lead: depth (and the weight) as [1, H, W]"""
    import fused_normal as fn
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    rs = Settings(c["W"], c["H"], c["tanfov"])
    shape = (1, c["H"], c["W"]) if lead else (c["H"], c["W"])
    d = t(c["depth"]).reshape(shape).requires_grad_(True)
    n = fn.depth_to_normal(d, raster_settings=rs)
    assert n.shape == (3, c["H"], c["W"]) and n.dtype == torch.float32 and n.is_contiguous()
    g = t(c["d_normals"])
    if noncontiguous:
        g = g.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        assert not g.is_contiguous()
    n.backward(g)
    assert d.grad.shape == shape
    d2, N = t(c["depth"]).reshape(shape).requires_grad_(need[1]), t(c["normal_map"]).requires_grad_(need[0])
    w = t(c["weight"]).reshape(shape).requires_grad_(True) if weight else None      # (a weight that requires a gradient gets none)
    loss = fn.normal_consistency_loss(N, d2, raster_settings=rs, weight=w)
    assert loss.shape == () and loss.dtype == torch.float32
    if any(need):
        (loss * c["upstream"]).backward()
    assert w is None or w.grad is None
    torch.cuda.synchronize()
    np_ = lambda x: None if x is None else x.detach().cpu().numpy()  # noqa: E731
    return dict(n=np_(n), d_depth=np_(d.grad).reshape(c["H"], c["W"]), loss=np_(loss), dN=np_(N.grad),
                dd=None if d2.grad is None else np_(d2.grad).reshape(c["H"], c["W"]))


def exactly_zero_where_no_normal(label, got, f64):
    """a pixel without a normal: 0 in n and dL/dN; dL/dd is 0 wherever the truth is (no stencil with a normal reads the pixel)"""
    none = ~f64["n"].any(0)
    assert not got["n"][:, none].any() and not got["dN"][:, none].any(), label
    for k in ("d_depth", "dd"):
        assert not got[k][f64[k] == 0.0].any(), (label, k)


@pytest.mark.parametrize("kind", nm.FIELDS)
def test_images_against_fp64(kind, gpu):
    worst = {}
    for i, (W, H) in enumerate(SIZES):
        c, f64, t32 = image_reference(kind, W, H)
        for weight in (False, True):
            label = f"{kind} {W}x{H} weight {weight}"
            got = fused_image(c, gpu, weight, lead=bool((i + weight) & 1))      # [H, W] and [1, H, W] in turn
            bar_check(label, got, f64[weight], t32[weight], worst)
            exactly_zero_where_no_normal(label, got, f64[weight])
        if W < 3 or H < 3:
            assert not got["n"].any() and float(got["loss"]) == 1.0, label
    if kind in ("hole", "nan", "negative"):      # the bad pixel itself has a normal (its own depth is no tap of its stencil) and no gradient
        c, f64, _ = image_reference(kind, 130, 70)
        with np.errstate(invalid="ignore"):
            bad = ~(c["depth"] > 0)
        assert bad.any() and not fused_image(c, gpu, True)["dd"][bad].any() and (kind == "hole" or f64[True]["n"][:, bad].any())
    summary(kind, worst)


def test_fronto_parallel_plane_faces_the_camera(gpu):
    import fused_normal as fn
    W, H = 67, 18
    n = fn.depth_to_normal(torch.full((H, W), 2.5, device=gpu), raster_settings=Settings(W, H, nm.TANFOV)).cpu().numpy()
    assert np.array_equal(n[:, 1:-1, 1:-1], np.broadcast_to(np.float32([0, 0, -1])[:, None, None], (3, H - 2, W - 2)))
    assert not n[:, 0].any() and not n[:, -1].any() and not n[:, :, 0].any() and not n[:, :, -1].any()


def test_fused_loss_equals_the_composition_of_depth_to_normal(gpu):
    """mean(1 - w (N . depth_to_normal(d)).sum(0)) built from the normals the device wrote (and, backward, through depth_to_normal's own
    gather), in torch on the device: the value and both gradients within the bar"""
    import fused_normal as fn
    worst = {}
    for kind, (W, H) in itertools.product(("wavy", "hole"), ((130, 70), (67, 18), (5, 5))):
        c, f64, t32 = image_reference(kind, W, H)
        t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
        rs = Settings(W, H, c["tanfov"])
        for weight in (False, True):
            N, d = t(c["normal_map"]).requires_grad_(True), t(c["depth"]).requires_grad_(True)
            dot = (N.double() * fn.depth_to_normal(d, raster_settings=rs).double()).sum(0)      # (the arithmetic around the op in fp64: the op's own error is what is measured)
            loss = (1.0 - (t(c["weight"]).double() * dot if weight else dot)).mean()
            (loss * c["upstream"]).backward()
            got = dict(loss=loss.detach().cpu().numpy(), dN=N.grad.cpu().numpy(), dd=d.grad.cpu().numpy())
            bar_check(f"composition {kind} {W}x{H} weight {weight}", got, f64[weight], t32[weight], worst)
    summary("composition", worst)


def test_a_second_run_is_bit_equal(gpu):
    for kind, W, H in (("wavy", 130, 70), ("hole", 130, 70), ("step", 67, 35)):
        c, _, _ = image_reference(kind, W, H)
        a, b = fused_image(c, gpu, True), fused_image(c, gpu, True)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (kind, k)


def test_requires_grad_combinations_unused_outputs_and_no_grad(gpu):
    import fused_normal as fn
    c, _, _ = image_reference("hole", 130, 70)
    full = fused_image(c, gpu, True)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    only_N, only_d, neither = (fused_image(c, gpu, True, need=need) for need in ((True, False), (False, True), (False, False)))
    assert only_N["dd"] is None and same(only_N["dN"], full["dN"]) and only_d["dN"] is None and same(only_d["dd"], full["dd"])
    assert neither["dN"] is None and neither["dd"] is None and same(neither["loss"], full["loss"])
    assert same(fused_image(c, gpu, True, noncontiguous=True)["d_depth"], full["d_depth"])
    rs = Settings(c["W"], c["H"], c["tanfov"])
    d, N = torch.tensor(c["depth"], device=gpu, requires_grad=True), torch.tensor(c["normal_map"], device=gpu, requires_grad=True)
    assert fn.depth_to_normal(d.detach(), raster_settings=rs).grad_fn is None
    with torch.no_grad():
        n, loss = fn.depth_to_normal(d, raster_settings=rs), fn.normal_consistency_loss(N, d, raster_settings=rs, weight=torch.tensor(c["weight"], device=gpu))
    assert n.grad_fn is None and loss.grad_fn is None and same(n.cpu().numpy(), full["n"]) and same(loss.cpu().numpy(), full["loss"])
    # an output nothing flows through: the other op's backward runs alone
    n, loss = fn.depth_to_normal(d, raster_settings=rs), fn.normal_consistency_loss(N, d, raster_settings=rs)
    loss.backward()
    assert n.grad_fn is not None and d.grad is not None and N.grad is not None


@pytest.mark.parametrize("cam_index", [1, 4])
def test_gaussian_normals_against_fp64(cam_index, scenes, gpu):
    import fused_normal as fn
    worst = {}
    for P in GAUSSIAN_ROWS:
        c, f64, t32 = gaussian_reference(P, cam_index, scenes)
        t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
        rs = Settings(70, 45, (0.5, 0.4), t(c["viewmatrix"]))
        m, s, q = t(c["means3D"]).requires_grad_(True), t(c["scales"]).requires_grad_(True), t(c["rotations"]).requires_grad_(True)
        n = fn.gaussian_normals(m, s, q, raster_settings=rs)
        assert n.shape == (P, 3) and n.dtype == torch.float32
        n.backward(t(c["d_normals"]))
        torch.cuda.synchronize()
        assert m.grad is None and s.grad is None and q.grad.shape == (P, 4)
        got = dict(n=n.detach().cpu().numpy(), d_rotations=q.grad.cpu().numpy())
        bar_check(f"P {P} camera {cam_index}", got, f64, t32, worst)
        if P >= 4:
            assert not got["n"][1:3].any() and not got["d_rotations"][1:3].any()      # the zero and the NaN quaternion
            assert got["n"][[0, 3]].any(1).all() and got["d_rotations"][[0, 3]].any(1).all()
            length = np.linalg.norm(got["n"].astype(np.float64), axis=1)
            assert np.abs(np.delete(length, [1, 2]) - 1.0).max() <= 2 * ULP
            V3 = c["viewmatrix"].astype(np.float64)[:3, :3]      # the tie row took column 0, the lowest index (up to its sign)
            col0 = nm._columns(nm._gauss(c["means3D"], c["scales"], c["rotations"], c["viewmatrix"])[1][:1], np.array([0]))[0]
            assert np.abs(np.abs(got["n"][0].astype(np.float64) @ V3.T @ col0) - 1.0) <= 1e-5
        # bit-equal again, without a graph, and under no_grad
        again = fn.gaussian_normals(m.detach(), s.detach(), q.detach(), raster_settings=rs)
        with torch.no_grad():
            quiet = fn.gaussian_normals(m, s, q, raster_settings=rs)
        assert again.grad_fn is None and quiet.grad_fn is None and torch.equal(again, n.detach()) and torch.equal(quiet, n.detach())
        q2 = q.detach().clone().requires_grad_(True)
        fn.gaussian_normals(m.detach(), s.detach(), q2, raster_settings=rs).backward(t(c["d_normals"]))
        assert torch.equal(q2.grad, q.grad)
    summary(f"gaussians camera {cam_index}", worst)


def test_what_raises(scenes, gpu):
    import fused_normal as fn
    c, _, _ = image_reference("wavy", 67, 18)
    rs = Settings(67, 18, nm.TANFOV)
    d, N = torch.tensor(c["depth"], device=gpu, requires_grad=True), torch.tensor(c["normal_map"], device=gpu, requires_grad=True)
    for out, leaf in ((fn.depth_to_normal(d, raster_settings=rs), d), (fn.normal_consistency_loss(N, d, raster_settings=rs), N)):
        (g,) = torch.autograd.grad(out, leaf, torch.ones_like(out).requires_grad_(True), create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
            g.sum().backward()
    g = nm.make_gaussian_case(65, scenes.camera(1, 6, 70, 45))
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    rsg = Settings(70, 45, (0.5, 0.4), t(g["viewmatrix"]))
    m, s, q = t(g["means3D"]), t(g["scales"]), t(g["rotations"]).requires_grad_(True)
    n = fn.gaussian_normals(m, s, q, raster_settings=rsg)
    (gq,) = torch.autograd.grad(n, q, torch.ones_like(n).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        gq.sum().backward()
    dd, Nd = d.detach(), N.detach()
    for call, err, text in ((lambda: fn.depth_to_normal(dd.cpu(), raster_settings=rs), RuntimeError, "GPU"),
                            (lambda: fn.normal_consistency_loss(Nd, dd.cpu(), raster_settings=rs), RuntimeError, "GPU|is on"),
                            (lambda: fn.normal_consistency_loss(Nd, dd, raster_settings=rs, weight=dd.cpu()), RuntimeError, "GPU|is on"),
                            (lambda: fn.depth_to_normal(dd.double(), raster_settings=rs), ValueError, "float32"),
                            (lambda: fn.depth_to_normal(dd[:, :66], raster_settings=rs), ValueError, r"\[18, 67\]"),
                            (lambda: fn.depth_to_normal(dd.t().contiguous().t(), raster_settings=rs), ValueError, "contiguous"),
                            (lambda: fn.normal_consistency_loss(Nd[:2], dd, raster_settings=rs), ValueError, r"\[3, 18, 67\]"),
                            (lambda: fn.gaussian_normals(m.cpu(), s, q, raster_settings=rsg), RuntimeError, "GPU"),
                            (lambda: fn.gaussian_normals(m, s[:, :2], q, raster_settings=rsg), ValueError, r"\[65, 3\]"),
                            (lambda: fn.gaussian_normals(m, s, q.detach().half(), raster_settings=rsg), ValueError, "float32"),
                            (lambda: fn.gaussian_normals(m, s, q, raster_settings=Settings(70, 45, (0.5, 0.4), g["viewmatrix"])), ValueError, "viewmatrix"),
                            (lambda: fn.gaussian_normals(m, s, q, raster_settings=Settings(70, 45, (0.5, 0.4), t(g["viewmatrix"]).cpu())), RuntimeError, "is on")):
        with pytest.raises(err, match=text):
            call()
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="is on"):
            fn.normal_consistency_loss(Nd, dd.to("cuda:1"), raster_settings=rs)


def test_end_to_end_gaussian_normals_render_loss(scenes, rast, gpu):
    """gaussian_normals -> render(features=, return_aux=True) -> normal_consistency_loss -> backward on 300 Gaussians at 70 x 45, against
    the same chain with the three ops replaced by the fp64 restatement on the render's own tensors, and against the same chain with them
    replaced by the torch fp32 composition on the same device: per gradient tensor
        |hip chain - fp64 chain| <= 4 |torch32 chain - fp64 chain| + 2^-23 max|fp64 chain|."""
    from conftest import settings_from
    import fused_normal as fn
    P, W, H = 300, 70, 45
    sc, cam = scenes.synth(P, 5), scenes.camera(1, 6, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    tan = (float(rs.tanfovx), float(rs.tanfovy))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    names = ("means3D", "opacities", "shs", "scales", "rotations")

    def render(leaves, features):
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros((P, 3), device=gpu, requires_grad=True), opacities=leaves["opacities"],
                                          shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"], return_aux=True, features=features)
        color, radii, depth, acc_depth, alpha, normal_map = out
        assert normal_map.shape == (3, H, W)
        return normal_map, acc_depth / alpha.clamp_min(1e-6), alpha.detach()

    def chain(kind):
        leaves = {k: t(sc[k]).requires_grad_(True) for k in names}
        if kind == "hip":
            N, d, w = render(leaves, fn.gaussian_normals(leaves["means3D"], leaves["scales"], leaves["rotations"], raster_settings=rs))
            fn.normal_consistency_loss(N, d, raster_settings=rs, weight=w).backward()
        elif kind == "torch32":
            N, d, w = render(leaves, nm.torch_gaussian_normals(leaves["means3D"], leaves["scales"], leaves["rotations"], rs.viewmatrix))
            nm.torch_normal_loss(N, d, *tan, w).backward()
        else:      # the three ops in fp64 numpy, the render between them as it is
            args = (sc["means3D"], sc["scales"], sc["rotations"], cam["viewmatrix"])
            F = t(nm.gaussian_normals(*args)).requires_grad_(True)
            N, d, w = render(leaves, F)
            dN, dd = nm.normal_loss_backward(N.detach().cpu().numpy(), d.detach().cpu().numpy(), *tan, w.cpu().numpy())
            torch.autograd.backward([N, d], [t(dN), t(dd).reshape(d.shape)])
            through_normals = nm.gaussian_normals_backward(*args, F.grad.cpu().numpy())
        torch.cuda.synchronize()
        g = {k: leaves[k].grad.double().cpu().numpy() for k in ("rotations", "means3D", "scales", "opacities")}
        if kind == "fp64":
            g["rotations"] = g["rotations"] + through_normals
        return g

    f64, hip, t32 = chain("fp64"), chain("hip"), chain("torch32")
    worst = {}
    bar_check("end to end", hip, f64, t32, worst)
    summary("end to end", worst)
    assert hip["rotations"].any() and hip["means3D"].any() and hip["scales"].any() and hip["opacities"].any()
