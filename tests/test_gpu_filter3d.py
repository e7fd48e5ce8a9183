"""Mip-Splatting's 3-D smoothing filter on the device (-m gpu): fused_filter3d against tests/filter3d_math.py.

Sweep: filter_3D and valid are BIT-EQUAL to the fp32 restatement (every operation rounded, no FMA: the library is built with
-ffp-contract=off and IEEE division), no tolerance, no row left out.  Sizes straddle a wave (63 / 64 / 65), a 256-row workgroup
(255 / 256 / 257), 4099 is ragged over 17 workgroups, 70001 gives 274 atomic pairs, and 2048 * 256 + 257 rows is the first size at which
the sweep walks its rows in grid strides.  The cameras are read through uniform loads in one loop: there is no camera chunk to straddle.
Apply: against fp64 on the same fp32 inputs, the bars counted from at most 24 roundings of half an ulp along the longest chain:
    scales_f 2 ulp |ref|;  opacities_f, d opacities 8 ulp |ref|;  d scales 16 ulp (|g_s r| + |G prod r q^2 / s_f|),  ulp = 2^-23.
The worst ratio per tensor is printed (-s) and recorded in profiles/filter3d_overhead.json."""
import math

import numpy as np
import pytest
import torch

import filter3d_math as fm
from conftest import ATOL, RTOL, grad_tol, settings_from

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
PARAMS = [(0.2, 0.15, 0.2), (0.5, 0.0, 0.1)]      # (near, margin, variance)
_REFERENCES = {}


def sweep_reference(scenes, P, C, params=PARAMS[0]):
    """(xyz fp32, cameras, table fp32, focal_max, the fp32 restatement): computed once, shared by the tests, never changed"""
    key = (P, C, params)
    if key not in _REFERENCES:
        xyz = scenes.synth(P, seed=3)["means3D"]
        cams = fm.ring(scenes, C)
        table, fmax = fm.table_of(cams, np.float32)
        _REFERENCES[key] = (xyz, cams, table, fmax, fm.sweep(xyz, table, np.float32, fmax, *params))
    return _REFERENCES[key]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def assert_sweep(flt, ref, P):
    assert flt.filter_3D.dtype == torch.float32 and tuple(flt.filter_3D.shape) == (P, 1) and flt.valid.dtype == torch.bool and tuple(flt.valid.shape) == (P,)
    assert np.array_equal(flt.valid.cpu().numpy(), ref["valid"])
    got = flt.filter_3D.cpu().numpy()
    assert same_bits(got, ref["filter"]), f"{(got.view(np.uint32) != ref['filter'].view(np.uint32)).sum()} of {P} rows differ"


@pytest.mark.parametrize("C", [1, 2, 7, 33])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 255, 256, 257, 4099])
def test_sweep_is_bit_equal_to_the_fp32_restatement(P, C, scenes, gpu):
    import fused_filter3d as ff
    for params in PARAMS:
        xyz, cams, _, _, ref = sweep_reference(scenes, P, C, params)
        near, margin, variance = params
        flt = ff.compute_filter_3d(torch.tensor(xyz, device=gpu), ff.camera_table(cams, gpu), near=near, margin=margin, variance=variance)
        assert_sweep(flt, ref, P)


@pytest.mark.parametrize("P,C", [(70001, 33), (2048 * 256 + 257, 2)])
def test_sweep_many_workgroups_and_grid_strides(P, C, scenes, gpu):
    import fused_filter3d as ff
    xyz, cams, table, fmax, ref = sweep_reference(scenes, P, C)
    assert 0.3 < ref["valid"].mean() < 0.95
    m, tb = torch.tensor(xyz, device=gpu, requires_grad=True), ff.camera_table(cams, gpu)      # (an input that requires grad is fine: nothing is differentiable)
    flt = ff.compute_filter_3d(m, tb)
    assert_sweep(flt, ref, P)
    assert not flt.filter_3D.requires_grad and flt.filter_3D.grad_fn is None
    again = ff.compute_filter_3d(m, tb)
    assert torch.equal(again.filter_3D, flt.filter_3D) and torch.equal(again.valid, flt.valid)      # run-to-run bits
    # a plain tensor as the table: focal_max from the caller
    plain = torch.tensor(table, device=gpu)
    with pytest.raises(ValueError, match="focal_max"):
        ff.compute_filter_3d(m, plain)
    assert torch.equal(ff.compute_filter_3d(m, plain, focal_max=fmax).filter_3D, flt.filter_3D)


def test_sweep_special_rows_and_tables(scenes, rast, gpu):
    import fused_filter3d as ff
    P, C = 257, 7
    xyz, cams, table, fmax, _ = sweep_reference(scenes, P, C)
    xyz = xyz.copy()
    xyz[3] = np.nan
    xyz[64] = (np.inf, 0.0, 0.0)
    xyz[130] = (0.0, 0.0, -np.inf)
    xyz[256] = (0.1, np.nan, 0.2)
    ref = fm.sweep(xyz, table, np.float32, fmax)
    tb = ff.camera_table(cams, gpu)
    flt = ff.compute_filter_3d(torch.tensor(xyz, device=gpu), tb)
    assert_sweep(flt, ref, P)
    bad = [3, 64, 130, 256]
    assert not ref["valid"][bad].any() and (ref["filter"][bad, 0] == ref["dmax"] * ref["k"]).all() and np.isfinite(flt.filter_3D.cpu().numpy()).all()
    # the C ABI with valid = NULL: the same filter
    from diff_gaussian_rasterization_ch3 import _C
    m = torch.tensor(xyz, device=gpu)
    out = torch.full((P, 1), -1.0, device=gpu)
    scratch = torch.empty(_C.scratch_bytes("gsrast_filter3d_scratch_bytes", P, C), dtype=torch.uint8, device=gpu)
    _C.launch("gsrast_filter3d_compute", gpu, P, C, m.data_ptr(), tb.data_ptr(), 0.2, 0.15, 0.2, fmax, out.data_ptr(), None, scratch.data_ptr())
    assert torch.equal(out, flt.filter_3D)
    # a table that sees nothing (all zeros), and rows no camera sees: every value +0.0
    for m0, t0 in ((m, torch.zeros((3, 16), device=gpu)), (torch.tensor(np.tile(np.float32([[0.0, 1e6, 0.0]]), (65, 1)), device=gpu), tb)):
        none = ff.compute_filter_3d(m0, t0, focal_max=fmax)
        f0 = none.filter_3D.cpu().numpy()
        assert not none.valid.any() and not f0.any() and not np.signbit(f0).any()
    # two cameras back to back at the origin: every row is seen by exactly one of them, or by none
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.0, 1.0, size=(4099, 3)).astype(np.float32)
    R = np.stack([np.eye(3), np.diag([-1.0, 1.0, -1.0])]).astype(np.float32)
    two = ff.camera_table_from_arrays(R, np.zeros((2, 3), np.float32), [20.0, 16.0], [20.0, 16.0], [64, 130], [48, 70], device=gpu)
    assert two.focal_max == 20.0
    ref2 = fm.sweep(pts, two.cpu().numpy(), np.float32, 20.0)
    each = [fm.sweep(pts, two.cpu().numpy()[c:c + 1], np.float32, 20.0)["valid"] for c in (0, 1)]
    assert not (each[0] & each[1]).any() and each[0].sum() > 500 and each[1].sum() > 500 and np.array_equal(ref2["valid"], each[0] | each[1])
    assert_sweep(ff.compute_filter_3d(torch.tensor(pts, device=gpu), two), ref2, 4099)
    # the table of camera_table from GaussianRasterizationSettings = the one from arrays
    sc = scenes.synth(8, 0)
    from_settings = ff.camera_table([settings_from(rast, c, sc, gpu) for c in cams], gpu)
    up = [fm.UpstreamCamera(c) for c in cams]
    from_arrays = ff.camera_table_from_arrays(np.stack([u.R for u in up]), np.stack([u.T for u in up]), [u.focal_x for u in up], [u.focal_y for u in up],
                                              [u.image_width for u in up], [u.image_height for u in up], device=gpu)
    assert from_settings.is_cuda and torch.equal(from_settings, from_arrays) and torch.equal(from_settings, tb) and from_settings.focal_max == from_arrays.focal_max == fmax
    assert same_bits(tb.cpu().numpy(), table)


# ---- apply ---------------------------------------------------------------------------------------------------------------------------
WORST = {}


def apply_check(what, got, s, o, f, g_s, g_o):
    """got: dict of fp32 arrays (any of scales_f, opacities_f, d_scales, d_opacities) against fp64 on the same fp32 inputs"""
    sf, of, _ = fm.apply_fwd(s, o, f)
    ds, do, a, b = fm.apply_bwd(s, o, f, g_s, g_o)
    ref = dict(scales_f=(sf, 2 * ULP * np.abs(sf)), opacities_f=(of, 8 * ULP * np.abs(of)), d_opacities=(do, 8 * ULP * np.abs(do)), d_scales=(ds, 16 * ULP * (a + b)))
    for k, v in got.items():
        want, bar = ref[k]
        v = np.asarray(v, np.float64)
        assert v.shape == want.shape and np.isfinite(v).all(), (what, k)
        err = np.abs(v - want)
        ratio = float((err[bar > 0] / bar[bar > 0]).max(initial=0.0))
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        print(f"{what}: {k} worst error / bar = {ratio:.3f}")
        assert (err <= bar).all(), (what, k, ratio)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 4099])
def test_apply_forward_and_backward_against_fp64(P, gpu):
    import fused_filter3d as ff
    s, o, f, g_s, g_o = fm.apply_case(P, seed=P)
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    ts, to, tf = t(s).requires_grad_(True), t(o).requires_grad_(True), t(f)
    s_f, o_f = ff.apply_filter_3d(ts, to, tf)
    assert tuple(s_f.shape) == (P, 3) and tuple(o_f.shape) == (P, 1)
    torch.autograd.backward([s_f, o_f], [t(g_s), t(g_o)])
    got = dict(scales_f=s_f.detach().cpu().numpy(), opacities_f=o_f.detach().cpu().numpy(), d_scales=ts.grad.cpu().numpy(), d_opacities=to.grad.cpu().numpy())
    apply_check(f"P {P}", got, s, o, f, g_s, g_o)
    if P >= 4:      # the edge rows, exactly: s = 0, f = 0 and a zero axis with f = 0
        for row in (0, 3):
            assert np.array_equal(got["scales_f"][row], s[row]) and got["opacities_f"][row, 0] == o[row, 0]
            assert np.array_equal(got["d_scales"][row], g_s[row]) and got["d_opacities"][row, 0] == g_o[row, 0]
        assert (got["opacities_f"][1:3] > 0).all()      # the thin rows: upstream's form gives 0 there
    # filter_3D as [P]: the same bits
    s_1, o_1 = ff.apply_filter_3d(t(s), t(o), tf.reshape(P))
    assert torch.equal(s_1, s_f) and torch.equal(o_1, o_f)
    if P == 4099:
        print("worst error / bar per tensor: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_apply_autograd_surface(gpu):
    import fused_filter3d as ff
    P = 257
    s, o, f, g_s, g_o = fm.apply_case(P, seed=5)
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    tf = t(f)
    full = {}
    for need_s, need_o in ((True, True), (True, False), (False, True), (False, False)):
        ts, to = t(s).requires_grad_(need_s), t(o).requires_grad_(need_o)
        s_f, o_f = ff.apply_filter_3d(ts, to, tf)
        assert s_f.requires_grad == o_f.requires_grad == (need_s or need_o)
        if need_s or need_o:
            torch.autograd.backward([s_f, o_f], [t(g_s), t(g_o)])
        assert (ts.grad is not None) == need_s and (to.grad is not None) == need_o
        if need_s and need_o:
            full = dict(s_f=s_f.detach(), o_f=o_f.detach(), ds=ts.grad.clone(), do=to.grad.clone())
        else:      # the same bits, whichever gradients are asked for
            assert torch.equal(s_f, full["s_f"]) and torch.equal(o_f, full["o_f"])
            assert (not need_s or torch.equal(ts.grad, full["ds"])) and (not need_o or torch.equal(to.grad, full["do"]))
    # an unused output counts as zero upstream
    for use_s in (True, False):
        ts, to = t(s).requires_grad_(True), t(o).requires_grad_(True)
        s_f, o_f = ff.apply_filter_3d(ts, to, tf)
        (s_f * t(g_s)).sum().backward() if use_s else (o_f * t(g_o)).sum().backward()
        apply_check(f"only {'scales_f' if use_s else 'opacities_f'} used", dict(d_scales=ts.grad.cpu().numpy(), d_opacities=to.grad.cpu().numpy()),
                    s, o, f, g_s if use_s else None, None if use_s else g_o)
        if use_s:
            assert not to.grad.any()
    # no_grad; a non-contiguous upstream gradient; run-to-run bits
    with torch.no_grad():
        s_n, o_n = ff.apply_filter_3d(t(s).requires_grad_(True), t(o), tf)
    assert not s_n.requires_grad and s_n.grad_fn is None and torch.equal(s_n, full["s_f"]) and torch.equal(o_n, full["o_f"])
    ts, to = t(s).requires_grad_(True), t(o).requires_grad_(True)
    s_f, o_f = ff.apply_filter_3d(ts, to, tf)
    strided = t(np.ascontiguousarray(g_s.T)).t()
    assert not strided.is_contiguous()
    torch.autograd.backward([s_f, o_f], [strided, t(g_o)])
    assert torch.equal(ts.grad, full["ds"]) and torch.equal(to.grad, full["do"])
    # a double backward raises
    ts = t(s).requires_grad_(True)
    s_f, o_f = ff.apply_filter_3d(ts, t(o), tf)
    (g,) = torch.autograd.grad(s_f, ts, torch.ones_like(s_f).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g.sum().backward()
    # what raises before a launch
    ds, do = t(s), t(o)
    for call, err, text in ((lambda: ff.apply_filter_3d(ds.cpu(), do, tf), RuntimeError, "GPU"), (lambda: ff.apply_filter_3d(ds, do.cpu(), tf), RuntimeError, "GPU|is on"),
                            (lambda: ff.apply_filter_3d(ds, do, tf.cpu()), RuntimeError, "GPU|is on"), (lambda: ff.apply_filter_3d(ds.double(), do, tf), ValueError, "float32"),
                            (lambda: ff.apply_filter_3d(ds[:, :2], do, tf), ValueError, r"\[\*, 3\]"), (lambda: ff.apply_filter_3d(ds, do[:5], tf), ValueError, r"\[257, 1\]"),
                            (lambda: ff.apply_filter_3d(ds.t().contiguous().t(), do, tf), ValueError, "contiguous"),
                            (lambda: ff.compute_filter_3d(ds.cpu(), torch.zeros(2, 16, device=gpu), focal_max=1.0), RuntimeError, "GPU"),
                            (lambda: ff.compute_filter_3d(ds, torch.zeros(2, 16), focal_max=1.0), RuntimeError, "GPU|is on"),
                            (lambda: ff.compute_filter_3d(ds, torch.zeros(2, 16, device=gpu)), ValueError, "focal_max")):
        with pytest.raises(err, match=text):
            call()
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="is on"):
            ff.apply_filter_3d(ds, do.to("cuda:1"), tf)


def test_zero_filter_is_the_identity(gpu):
    import fused_filter3d as ff
    P = 4099
    s, o, _, g_s, g_o = fm.apply_case(P, seed=9, edges=False)
    s[0] = 0.0
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    ts, to = t(s).requires_grad_(True), t(o).requires_grad_(True)
    s_f, o_f = ff.apply_filter_3d(ts, to, torch.zeros((P, 1), device=gpu))
    torch.autograd.backward([s_f, o_f], [t(g_s), t(g_o)])
    assert torch.equal(s_f, ts) and torch.equal(o_f, to) and torch.equal(ts.grad, t(g_s)) and torch.equal(to.grad, t(g_o))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_filter_render_loss(scenes, rast, gpu):
    """raw leaves -> exp / sigmoid -> compute_filter_3d over 5 ring cameras -> apply_filter_3d -> GaussianRasterizer(antialiasing=True) ->
    l1_dssim_loss -> backward on 300 Gaussians at 70 x 45, against the same chain with the op replaced by its fp64 torch composition, cast
    to fp32 in front of the same HIP render."""
    import fused_filter3d as ff
    from fused_loss import l1_dssim_loss
    P, W, H = 300, 70, 45
    sc = scenes.synth(P, 5)
    cams = [scenes.camera(k, 5, W, H) for k in range(5)]
    rs = settings_from(rast, cams[1], sc, gpu)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    gt = t(np.random.default_rng(2).uniform(0.0, 1.0, size=(3, H, W)))
    raw = dict(means3D=sc["means3D"], rotations=sc["rotations"], shs=sc["shs"], scaling=np.log(sc["scales"]), opacity=np.log(sc["opacities"] / (1.0 - sc["opacities"])))
    table, fmax = fm.table_of(cams, np.float32)
    ref_filter = fm.sweep(sc["means3D"], table, np.float32, fmax)
    assert ref_filter["valid"].mean() > 0.5

    def render(leaves, scales, opacities):
        color = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros((P, 3), device=gpu, requires_grad=True), opacities=opacities,
                                            shs=leaves["shs"], scales=scales, rotations=leaves["rotations"], antialiasing=True)[0]
        return color

    def chain(kind):
        leaves = {k: t(v).requires_grad_(True) for k, v in raw.items()}
        s, o = torch.exp(leaves["scaling"]), torch.sigmoid(leaves["opacity"])
        if kind == "hip":
            flt = ff.compute_filter_3d(leaves["means3D"], ff.camera_table(cams, gpu))
            assert same_bits(flt.filter_3D.cpu().numpy(), ref_filter["filter"])
            s, o = ff.apply_filter_3d(s, o, flt.filter_3D)
        elif kind == "fp64":
            f = t(ref_filter["filter"]).double()
            s64, o64 = s.double(), o.double()
            sf = torch.sqrt(s64 * s64 + f * f)
            r = s64 / sf
            s, o = sf.float(), (o64 * ((r[:, 0] * r[:, 1]) * r[:, 2])[:, None]).float()
        elif kind == "baked":
            flt = ff.compute_filter_3d(leaves["means3D"], ff.camera_table(cams, gpu))
            b_s, b_o = ff.bake_filter_3d(leaves["scaling"], leaves["opacity"], flt.filter_3D)
            assert not b_s.requires_grad and not b_o.requires_grad
            s, o = torch.exp(b_s), torch.sigmoid(b_o)
        image = render(leaves, s, o)
        if kind in ("hip", "fp64"):
            l1_dssim_loss(image, gt).backward()
        torch.cuda.synchronize()
        grads = {k: leaves[k].grad.double().cpu().numpy() for k in ("scaling", "opacity", "rotations", "means3D")} if kind in ("hip", "fp64") else None
        return image.detach().double().cpu().numpy(), grads

    (img_ref, g_ref), (img_hip, g_hip), (img_plain, _), (img_baked, _) = chain("fp64"), chain("hip"), chain("plain"), chain("baked")
    close = lambda a, b: bool((np.abs(a - b) <= ATOL + RTOL * np.abs(b)).all())  # noqa: E731
    assert close(img_hip, img_ref)
    for k, ref in g_ref.items():
        err, tol = np.abs(g_hip[k] - ref), grad_tol(ref)
        print(f"end to end: d {k} worst error / bar = {(err / np.maximum(tol, 1e-300)).max():.3f}")
        assert ref.any() and (err <= tol).all(), k
    assert not close(img_plain, img_ref) and np.abs(img_plain - img_ref).max() > 1e-3      # the filter is not a no-op
    assert close(img_baked, img_ref)


def test_filter_follows_densification(scenes, gpu):
    """after densify_and_prune changed P the recomputed filter has the new length, and the next GaussianAdam.step() runs"""
    import densify_math as dm
    import fused_adam
    import fused_densify
    import fused_filter3d as ff
    d = dm.draw(4099, 4, "mixed", seed=8)
    leaves = {k: torch.nn.Parameter(v.clone().to(gpu)) for k, v in d["params"].items()}
    opt = fused_adam.GaussianAdam([{"params": [leaves[k]], "lr": 1e-3, "name": k} for k in dm.GROUPS], eps=1e-15)
    stats = fused_densify.DensifyStats(4099, gpu)
    stats.xyz_gradient_accum, stats.denom = d["accum"].clone().to(gpu), d["denom"].clone().to(gpu)
    table = ff.camera_table(fm.ring(scenes, 5), gpu)
    before = ff.compute_filter_3d(leaves["xyz"].detach(), table)
    counts, new = fused_densify.densify_and_prune(opt, stats, grad_threshold=d["kw"]["thr"], percent_dense=d["kw"]["tau"] / 4.0, extent=4.0,
                                                  min_opacity=d["kw"]["min_opacity"], n_split=2)
    Pn = counts["P"]
    assert Pn != 4099 and tuple(before.filter_3D.shape) == (4099, 1)
    flt = ff.compute_filter_3d(new["xyz"], table)      # (a Parameter: inputs that require grad are fine)
    assert tuple(flt.filter_3D.shape) == (Pn, 1) and tuple(flt.valid.shape) == (Pn,)
    ref = fm.sweep(new["xyz"].detach().cpu().numpy(), table.cpu().numpy(), np.float32, table.focal_max)
    assert same_bits(flt.filter_3D.cpu().numpy(), ref["filter"])
    s_f, o_f = ff.apply_filter_3d(torch.exp(new["scaling"]), torch.sigmoid(new["opacity"]), flt.filter_3D)
    (s_f.sum() + o_f.sum()).backward()
    assert new["scaling"].grad is not None and new["opacity"].grad is not None and math.isfinite(float(new["scaling"].grad.abs().sum()))
    for g in opt.param_groups:
        p = g["params"][0]
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    opt.step()
    assert torch.isfinite(new["scaling"]).all() and torch.isfinite(new["opacity"]).all()
