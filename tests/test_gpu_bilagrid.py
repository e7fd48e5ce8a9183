"""-m gpu: the bilateral-grid colour correction (csrc/gsrast_bilagrid.h, fused_bilagrid.py) against the fp64 restatement of
tests/bilagrid_math.py.

The bar is tests/test_gpu_temporal.py's, per output and gradient tensor T, evaluated per case at run time:
    max|T_hip - T_fp64| <= 4 max|T_torch32 - T_fp64| + 2^-23 max|T_fp64|,
T_torch32 = torch's fp32 CPU run of the same composition (F.grid_sample + the matrix product, and its autograd) on the same inputs.  The
factor 4 covers another summation order (the gather sums a vertex's pixels lane by lane, torch scatters them one after the other) and
FMA contraction on torch's side; the second term is one ulp of fp32 at the tensor's largest entry.  The generator keeps every pixel's
gray away from the kinks of the guidance slope (tests/bilagrid_math.py: make_case), so no pixel is excluded from a comparison.

Worst ratio e_hip / bar per tensor over the whole file, as measured on an MI355X (the summary lines of the tests, -s):
    out 0.32   d_grid 0.40   d_image 0.25   tv 0.15   d_tv 0.09      (profiles/bilagrid_overhead.json: worst_e_hip_over_bar)"""
import numpy as np
import pytest
import torch

import bilagrid_math as bm

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
GRIDS = bm.GRIDS + [(64, 64, 16)]
FRAME = (1920, 1080)
SPLITS = [0, 1, 2, 3, 7]


def bar_check(label, got, f64, t32, worst):
    """The bar of this file's docstring on every tensor of `got`; the worst ratio per tensor is kept in `worst` for the summary line."""
    bad = []
    for k, g in got.items():
        truth = np.asarray(f64[k], np.float64)
        g = np.asarray(g, np.float64).reshape(truth.shape)
        assert np.isfinite(truth).all() and np.isfinite(g).all(), (label, k)
        e_hip = float(np.abs(g - truth).max())
        e_ref = float(np.abs(np.asarray(t32[k], np.float64).reshape(truth.shape) - truth).max())
        bound = 4 * e_ref + ULP * float(np.abs(truth).max())
        if bound > 0 and e_hip / bound > worst.get(k, (0.0,))[0]:
            worst[k] = (e_hip / bound, e_hip, e_ref, label)
        if not e_hip <= bound:
            bad.append((k, e_hip, e_ref, bound))
    assert not bad, (label, bad)


def summary(what, worst):
    for k, (ratio, e_hip, e_ref, label) in worst.items():
        print(f"bilagrid {what} {k}: worst e_hip / bar {ratio:.3f} (e_hip {e_hip:.3e}, e_torch32 {e_ref:.3e}) at {label}")


def images_for(GW, GH):
    """(W, H, window): the whole frames, a 24 x 24 window inside one cell of a 1920 x 1080 frame, and one across a cell corner"""
    fw, fh = FRAME
    cx = min(max(round(fw / (GW - 1)) - 12, 0), fw - 24) if GW > 1 else 100      # the corner of cells at vertex (1, 1), or the frame's if it is the last
    cy = min(max(round(fh / (GH - 1)) - 12, 0), fh - 24) if GH > 1 else 100
    return [(1, 1, None), (7, 5, None), (16, 16, None), (17, 33, None), (64, 48, None), (130, 70, None), (5, 3, None),
            (24, 24, (700, 400, fw, fh)), (24, 24, (cx, cy, fw, fh))]


_REFERENCES = {}


def reference(GW, GH, L, W, H, window):
    """(case, fp64 truth, torch fp32) of one shape: computed once, shared by the tests, never changed"""
    key = (GW, GH, L, W, H, window)
    if key not in _REFERENCES:
        c = bm.make_case(GW, GH, L, W, H, seed=7 * GW + 3 * L + W)
        d_grid, d_image = bm.backward(c["grid"], c["image"], c["d_out"], window)
        f64 = dict(out=bm.forward(c["grid"], c["image"], window), d_grid=d_grid, d_image=d_image)
        _REFERENCES[key] = (c, f64, bm.torch_run(c["grid"], c["image"], c["d_out"], window, torch.float32))
    return _REFERENCES[key]


def fused(c, window, gpu, need_grid=True, need_image=True):
    import fused_bilagrid as fb
    grid = torch.tensor(c["grid"], device=gpu).requires_grad_(need_grid)
    image = torch.tensor(c["image"], device=gpu).requires_grad_(need_image)
    out = fb.bilagrid_apply(grid, image, window=window)
    assert out.shape == image.shape and out.dtype == torch.float32 and out.is_contiguous()
    if need_grid or need_image:
        out.backward(torch.tensor(c["d_out"], device=gpu))
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu().numpy())
    res["d_grid"] = grid.grad.cpu().numpy() if need_grid else None
    res["d_image"] = image.grad.cpu().numpy() if need_image else None
    return res


def through_c_abi(rast, c, window, splits, gpu):
    """forward and backward through the C ABI with `splits` slabs per vertex column; every output and the scratch start as NaN bytes"""
    _C = rast._C
    lib = _C.lib()
    _, Lg, GH, GW = c["grid"].shape
    H, W = c["image"].shape[1:]
    desc = _C.BilagridStruct(GW, GH, Lg, W, H, *bm.window_of(W, H, window), splits)
    grid, image, d_out = (torch.tensor(c[k], device=gpu) for k in ("grid", "image", "d_out"))
    nan = lambda like: torch.full_like(like, float("nan"))  # noqa: E731
    out, d_image, d_grid = nan(image), nan(image), nan(grid)
    nbytes = lib.gsrast_bilagrid_scratch_bytes(desc)
    assert nbytes >= 256
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
    s = _C._stream_of(gpu)
    assert lib.gsrast_bilagrid_forward(desc, grid.data_ptr(), image.data_ptr(), out.data_ptr(), s) == 0, lib.gsrast_last_error()
    assert lib.gsrast_bilagrid_backward(desc, grid.data_ptr(), image.data_ptr(), d_out.data_ptr(), d_image.data_ptr(), d_grid.data_ptr(),
                                        scratch.data_ptr(), s) == 0, lib.gsrast_last_error()
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), d_grid=d_grid.cpu().numpy(), d_image=d_image.cpu().numpy())


@pytest.mark.parametrize("GW,GH,L", GRIDS)
def test_forward_and_backward_against_fp64(GW, GH, L, gpu):
    worst = {}
    for W, H, window in images_for(GW, GH):
        c, f64, t32 = reference(GW, GH, L, W, H, window)
        label = f"grid {GW}x{GH}x{L} image {W}x{H} window {window}"
        got = fused(c, window, gpu)
        bar_check(label, got, f64, t32, worst)
        untouched = f64["d_grid"] == 0.0      # vertices no pixel reaches (cells smaller than a pixel, a window inside one cell): exactly 0
        assert not got["d_grid"][untouched].any(), label
        if (W, H) == (5, 3) and GW * GH >= 256:
            assert untouched.mean() > 0.5, label
    summary(f"{GW}x{GH}x{L}", worst)


@pytest.mark.parametrize("splits", SPLITS)
def test_slab_counts_through_the_c_abi_and_run_to_run_bits(splits, rast, gpu):
    worst = {}
    fw, fh = FRAME
    for (GW, GH, L), (W, H, window) in (((5, 3, 4), (130, 70, None)), ((16, 16, 8), (64, 48, None)), ((64, 64, 16), (17, 33, None)),
                                        ((2, 2, 2), (7, 5, None)), ((1, 1, 1), (130, 70, None)), ((3, 7, 1), (24, 24, (700, 400, fw, fh)))):
        c, f64, t32 = reference(GW, GH, L, W, H, window)
        label = f"splits {splits} grid {GW}x{GH}x{L} image {W}x{H} window {window}"
        a, b = through_c_abi(rast, c, window, splits, gpu), through_c_abi(rast, c, window, splits, gpu)
        bar_check(label, a, f64, t32, worst)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (label, k)
        assert not a["d_grid"][f64["d_grid"] == 0.0].any(), label
    summary(f"splits={splits}", worst)


def test_requires_grad_combinations_and_no_grad(gpu):
    import fused_bilagrid as fb
    c, _, _ = reference(5, 3, 4, 130, 70, None)
    full = fused(c, None, gpu)
    only_grid, only_image = fused(c, None, gpu, need_image=False), fused(c, None, gpu, need_grid=False)
    assert only_grid["d_image"] is None and np.array_equal(only_grid["d_grid"].view(np.uint32), full["d_grid"].view(np.uint32))
    assert only_image["d_grid"] is None and np.array_equal(only_image["d_image"].view(np.uint32), full["d_image"].view(np.uint32))
    neither = fused(c, None, gpu, need_grid=False, need_image=False)
    assert np.array_equal(neither["out"].view(np.uint32), full["out"].view(np.uint32))
    grid, image = torch.tensor(c["grid"], device=gpu, requires_grad=True), torch.tensor(c["image"], device=gpu, requires_grad=True)
    assert fb.bilagrid_apply(grid.detach(), image.detach()).grad_fn is None
    with torch.no_grad():
        out = fb.bilagrid_apply(grid, image)
    assert out.grad_fn is None and not out.requires_grad and np.array_equal(out.cpu().numpy().view(np.uint32), full["out"].view(np.uint32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_nan_or_inf_pixel_stays_in_its_pixel_and_its_corners(bad, gpu):
    c, _, _ = reference(5, 3, 4, 64, 48, None)
    clean = fused(c, None, gpu)
    px, py, ch = 41, 17, 1
    dirty = dict(c, image=c["image"].copy())
    dirty["image"][ch, py, px] = bad
    got = fused(dirty, None, gpu)
    keep = np.ones((48, 64), bool)
    keep[py, px] = False
    for k in ("out", "d_image"):
        assert np.array_equal(got[k][:, keep].view(np.uint32), clean[k][:, keep].view(np.uint32)), k
    assert not np.isfinite(got["out"][:, py, px]).any()
    if bad != bad:      # (an infinite pixel is clamped: its guidance slope is 0 and d image there is the finite matrix product)
        assert not np.isfinite(got["d_image"][:, py, px]).any()
    poisoned = ~np.isfinite(got["d_grid"])
    assert 0 < poisoned.sum() <= 8 * 12 and poisoned.any(axis=(0, 2, 3)).sum() <= 2      # at most two slices x four vertices x 12 channels
    # ... all of them corners of the pixel's xy cell, vertices (gx0 .. gx0 + 1, gy0 .. gy0 + 1); no other vertex column differs from the
    # clean run in a single bit (inside the cell the two slices of the pixel's true gray lose its contribution: finite, but other sums)
    gx0, gy0 = int(np.floor((px + 0.5) / 64 * 4)), int(np.floor((py + 0.5) / 48 * 2))
    corner = np.zeros_like(poisoned)
    corner[:, :, gy0:gy0 + 2, gx0:gx0 + 2] = True
    assert not (poisoned & ~corner).any()
    assert np.array_equal(got["d_grid"][~corner].view(np.uint32), clean["d_grid"][~corner].view(np.uint32))


def test_what_raises(gpu):
    import fused_bilagrid as fb
    grid, image = torch.rand(12, 4, 3, 5, device=gpu, requires_grad=True), torch.rand(3, 20, 30, device=gpu, requires_grad=True)
    out = fb.bilagrid_apply(grid, image)
    (g,) = torch.autograd.grad(out, image, torch.ones_like(out).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g.sum().backward()
    gd, im = grid.detach(), image.detach()
    for args, err, text in (((gd.cpu(), im), RuntimeError, "GPU"), ((gd, im.cpu()), RuntimeError, "GPU"),
                            ((gd.transpose(2, 3), im), ValueError, "contiguous"), ((gd, im.permute(0, 2, 1)), ValueError, "contiguous"),
                            ((gd.double(), im), ValueError, "float32"), ((gd, im.half()), ValueError, "float32"),
                            ((gd[:11], im), ValueError, "12, L, GH, GW"), ((gd, im[:2]), ValueError, r"\[3, H, W\]"), ((gd, im[0]), ValueError, r"\[3, H, W\]")):
        with pytest.raises(err, match=text):
            fb.bilagrid_apply(*args)
    with pytest.raises(ValueError, match="window"):
        fb.bilagrid_apply(gd, im, window=(0, 0, 29, 20))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="is on"):
            fb.bilagrid_apply(gd, im.to("cuda:1"))
    else:      # one visible device: the same check, on the only other device there is
        with pytest.raises(RuntimeError, match="GPU|is on"):
            fb.bilagrid_apply(gd, im.to("cpu"))


@pytest.mark.parametrize("N", [1, 3])
def test_tv_value_and_gradient(N, gpu):
    import fused_bilagrid as fb
    worst = {}
    for GW, GH, L in bm.GRIDS:
        grids = bm.make_grids(N, GW, GH, L, seed=GW + L + N)
        f64 = dict(tv=np.float64(bm.tv(grids)), d_tv=bm.tv_grad(grids) * 0.75)
        t32 = bm.torch_tv_run(grids, torch.float32)
        t32["d_tv"] = t32["d_tv"] * np.float32(0.75)
        g = torch.tensor(grids, device=gpu, requires_grad=True)
        value = fb.tv(g)
        assert value.shape == () and value.dtype == torch.float32
        (value * 0.75).backward()      # (the upstream scalar reaches the kernel)
        got = dict(tv=value.detach().cpu().numpy(), d_tv=g.grad.cpu().numpy())
        if (GW, GH, L) == (1, 1, 1):
            assert got["tv"] == 0.0 and not got["d_tv"].any()
        bar_check(f"tv N={N} grid {GW}x{GH}x{L}", got, f64, t32, worst)
        again = fb.tv(g.detach())
        assert again.grad_fn is None and torch.equal(again, value.detach())
    summary(f"tv N={N}", worst)
    m = fb.BilateralGrids(N).to(gpu)
    assert float(m.tv_loss().detach()) == 0.0


def test_module_routes_the_gradient_into_one_cameras_grid(gpu):
    import fused_bilagrid as fb
    c, f64, t32 = reference(5, 3, 4, 64, 48, None)
    m = fb.BilateralGrids(3, grid_x=5, grid_y=3, grid_w=4).to(gpu)
    with torch.no_grad():
        m.grids[1] = torch.tensor(c["grid"], device=gpu)
    out = m(torch.tensor(c["image"], device=gpu), 1)
    out.backward(torch.tensor(c["d_out"], device=gpu))
    assert not m.grids.grad[0].any() and not m.grids.grad[2].any()
    bar_check("module", dict(out=out.detach().cpu().numpy(), d_grid=m.grids.grad[1].cpu().numpy()), f64, t32, {})


def test_end_to_end_render_grid_loss(scenes, rast, gpu):
    """render (P = 3000, 64 x 48) -> BilateralGrids -> l1_dssim_loss -> backward: every leaf of the Gaussians and the grid receive finite,
    non-zero gradients; the fresh (identity) grid passes the rendered image through within the bar of this file."""
    from conftest import settings_from
    import fused_bilagrid as fb
    import fused_loss
    P, W, H = 3000, 64, 48
    sc = scenes.synth(P, 7)
    rs = settings_from(rast, scenes.camera(1, 6, W, H), sc, gpu)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    leaves = {k: t(sc[k]).requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
    color = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                                        scales=leaves["scales"], rotations=leaves["rotations"])[0]
    grids = fb.BilateralGrids(2).to(gpu)
    image = grids(color, 1)
    gt = t(np.random.default_rng(3).uniform(0, 1, (3, H, W)))
    loss = fused_loss.l1_dssim_loss(image, gt, 0.2) + 10.0 * grids.tv_loss()
    loss.backward()
    torch.cuda.synchronize()
    assert float(color.detach().max()) > 0.1
    for k, leaf in leaves.items():
        assert torch.isfinite(leaf.grad).all() and leaf.grad.any(), k
    assert torch.isfinite(grids.grids.grad).all() and grids.grids.grad[1].any() and not grids.grids.grad[0].any()
    render = color.detach().cpu().numpy()
    ident = bm.identity_grid(16, 16, 8)
    f64 = dict(out=bm.forward(ident, render))
    t32 = dict(out=bm.torch_apply(torch.tensor(ident), torch.tensor(render)).numpy())
    worst = {}
    bar_check("end to end, identity", dict(out=image.detach().cpu().numpy()), f64, t32, worst)
    summary("end to end", worst)
