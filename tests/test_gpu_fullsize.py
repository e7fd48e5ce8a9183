"""-m gpu: BASELINE.json's full-size configurations.

1. Oracle equality at full size (test_full_size_oracle_equality): the CPU oracle renders 1 M Gaussians at 1080p forward +
   backward in a few seconds on the GPU box's host cores, so cfg2, cfg3, the bench workload (1 M @ 1080p) and cfg5 (3 M @ 1080p)
   are compared with it directly -- forward bit for bit, gradients within conftest.grad_tol of the fp64 truth
   (1e-5 * max|ref| + 1e-4 * |ref| per tensor: round 6 -- the absolute 1e-5 of rounds 1-5 was 40 % of the largest dL/dsh entry at
   these sizes); test_the_gradient_bar_bites shows the bar turning red for one dropped batch of one tile.
2. Size-independent properties: sortedness and partition of the binning, bounds, determinism, invariance of the forward
   under every kernel variant, linearity of the backward in the upstream gradient."""
import numpy as np
import pytest
import torch

from conftest import settings_from

pytestmark = pytest.mark.gpu

CONFIGS = [
    # BASELINE.json configs 2, 3, 5 (synthetic stand-ins of the named shapes)
    ("cfg2_mutant_100k_800", 100_000, 800, 800),
    ("cfg3_cook_spinach_1M_1352x1014", 1_000_000, 1352, 1014),
    ("cfg5_stress_3M_1080p", 3_000_000, 1920, 1080),
]


def _inputs(scenes, rast, P, W, H, dev, seed=0):
    sc = scenes.synth(P, seed)
    cam = scenes.camera(0, 1, W, H)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    rs = settings_from(rast, cam, sc, dev)
    ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    return sc, cam, rs, ten


def _forward_state(rast, rs, ten, P, W, H):
    e = torch.empty(0)
    rast._C.set_option("debug_state", 1)        # keep cov3D for the export (not stored by default)
    try:
        R, color, radii, gb, bb, ib, depth = rast._C.rasterize_gaussians(
            rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, ten["shs"], rs.sh_degree, rs.campos, False)
        st = rast._C.debug_export(P, R, W, H, gb, bb, ib)
    finally:
        rast._C.set_option("debug_state", 0)
    return R, color, radii, depth, st


FULL = CONFIGS[:2] + [("bench_1M_1080p", 1_000_000, 1920, 1080), CONFIGS[2], ("shell_1M_1080p", 1_000_000, 1920, 1080)]


@pytest.mark.parametrize("name,P,W,H", FULL, ids=[c[0] for c in FULL])
def test_full_size_oracle_equality(name, P, W, H, orc, scenes, rast, gpu):
    """HIP == oracle at BASELINE's full sizes: radii / tiles / lists / n_contrib / colour / depth / final_T bit-exact (lists on
    the reference's literal tile lists, tile_clip=0; outputs also with the product default), every gradient within
    1e-5 * max|ref| + 1e-4 * |ref| of the fp64 truth (conftest.grad_tol) with the bench's upstream gradient N(0,1)/(3HW) -- both
    renders: the uncut one and the pose's second, under the list cut."""
    from gpu_harness import bits, run_hip
    from test_gpu_parity import _check_forward_exact, _check_grads
    sc = scenes.synth_shell(P, 0) if name.startswith("shell") else scenes.synth(P, 0)     # shell: a surface-like scene, R_eff ~ R
    cam = scenes.camera(0, 1, W, H)
    g = scenes.upstream_grad(H, W, 1)
    orc.set_exp_mode(0)
    o32 = orc.render(sc, cam, g)
    if name.startswith("shell"):
        gy, gx = (H + 15) // 16, (W + 15) // 16
        nc = np.zeros((gy * 16, gx * 16), np.int64); nc[:H, :W] = o32["n_contrib"]
        r_eff = int(nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).sum())
        assert r_eff > 0.5 * o32["R"], (r_eff, o32["R"])          # the regime this scene exists for
    o64 = orc.render(sc, cam, g, f64=True)
    names = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]
    # 3 M: the product default only (the 75 M-entry literal lists are covered by the property test below) -- twice: the second render of
    # the pose runs under the list cut (include/gsrast.h: options.no_list_cut; it applies itself at these sizes) and, from 1.5 M
    # Gaussians on, with the late Gaussians' zero rows written beside the blend backward.  At 1 M the clipped run is the pose's second.
    for rnd, clip in enumerate((1, 1) if P > 2_000_000 else (0, 1)):
        h = run_hip(rast, sc, cam, gpu, dL_dcolor=g, exp_mode=0, tile_clip=clip)
        if rnd == 1 and name.startswith(("bench", "cfg5", "cfg3")):
            assert rast._C.context_query("last_late") > P // 4, "the second render of the pose was expected to run under the list cut"
        if clip == 0:
            _check_forward_exact(o32, h, clipped=False)
        else:       # clipped lists: outputs and per-Gaussian state bit for bit (the subsequence walk of check_clipped_lists is
            assert h["R"] == o32["R"]                       # a Python loop over tiles: kept for the small cases)
            np.testing.assert_array_equal(h["radii"], o32["radii"])
            np.testing.assert_array_equal(h["tiles_touched"], o32["tiles_touched"])
            for k in ("final_T", "out_color", "out_depth"):
                np.testing.assert_array_equal(bits(h[k]), bits(o32[k]), err_msg=k)
            vis = o32["radii"] > 0
            for k in ("depths", "means2D", "conic_opacity", "cov3D"):
                np.testing.assert_array_equal(bits(h[k][vis]), bits(o32[k][vis]), err_msg=k)
        _check_grads(o64, o32, h, names, strict=True)
        del h


BITES = [FULL[0], FULL[3]]


@pytest.mark.parametrize("name,P,W,H", BITES, ids=[c[0] for c in BITES])
def test_the_gradient_bar_bites(name, P, W, H, orc, scenes, rast, gpu):
    """the full-size gradient bar must be able to fail.  Option "mutate" = 1 (tests only, csrc/gsrast_capi.hip: mutate_drop_front_batch_kernel)
    makes the blend backward of ONE tile -- the image's centre tile, 1 of 2 500 / 8 160 -- miss the 64 front-most entries of its list: one
    staged batch dropped, every other (pixel, Gaussian) pair untouched (reference: backward.cu:472-557 walks the whole range).  The
    unmutated backward passes _check_grads, the mutated one must not -- at cfg2 and at cfg5 (3 M @ 1080p), where rounds 1-5's absolute
    1e-5 was of the size of the gradients themselves."""
    from gpu_harness import run_hip
    from test_gpu_parity import _check_grads
    sc = scenes.synth(P, 0)
    cam = scenes.camera(0, 1, W, H)
    g = scenes.upstream_grad(H, W, 1)
    orc.set_exp_mode(0)
    o32 = orc.render(sc, cam, g)
    o64 = orc.render(sc, cam, g, f64=True)
    names = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"]
    h = run_hip(rast, sc, cam, gpu, dL_dcolor=g, exp_mode=0, tile_clip=1)
    _check_grads(o64, o32, h, names, strict=True)
    rast._C.set_option("mutate", 1)
    try:
        hm = run_hip(rast, sc, cam, gpu, dL_dcolor=g, exp_mode=0, tile_clip=1)
    finally:
        rast._C.set_option("mutate", 0)
    np.testing.assert_array_equal(hm["out_color"].view(np.uint32), h["out_color"].view(np.uint32))      # (the forward is not touched)
    red = []
    for k in names:
        try:
            _check_grads(o64, o32, hm, [k], strict=True)
        except AssertionError:
            red.append(k)
    # every tensor the dropped pairs feed must be caught -- not a handful of rows of one of them
    assert set(red) >= {"dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"}, red
    # how many entries the mutation moved by more than the bar, and by more than rounds 1-5's absolute 1e-5 (for the record)
    ref = o64["dL_dsh"].astype(np.float64)
    err = np.abs(hm["dL_dsh"].astype(np.float64).reshape(ref.shape) - ref)
    from conftest import grad_tol
    print(f"{name}: dL/dsh entries over the scale-free bar {int((err > grad_tol(ref)).sum())}, over the absolute 1e-5 bar {int((err > 1e-5 + 1e-4 * np.abs(ref)).sum())}, max |ref| {np.abs(ref).max():.3e}")


@pytest.mark.parametrize("clip", [0, 1], ids=["literal_lists", "clipped_lists"])
@pytest.mark.parametrize("name,P,W,H", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_binning_and_image_properties(name, P, W, H, clip, scenes, rast, gpu):
    sc, cam, rs, ten = _inputs(scenes, rast, P, W, H, gpu)
    rast._C.set_option("tile_clip", clip)
    try:
        R, color, radii, depth, st = _forward_state(rast, rs, ten, P, W, H)
    finally:
        rast._C.set_option("tile_clip", 1)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert R == int(st["tiles_touched"].to(torch.int64).sum())     # num_rendered keeps the reference's meaning
    R_ref = R
    R = int((st["ranges"].to(torch.int64)[:, 1] - st["ranges"].to(torch.int64)[:, 0]).sum())   # entries actually listed
    assert (R == R_ref) if clip == 0 else (0 < R < R_ref)
    keys = st["keys_sorted"][:R]                               # (tile << 32) | depth bits, int64 view of uint64
    assert bool((keys[1:] >= keys[:-1]).all()), "sorted keys must be non-decreasing"   # tile < 2^31: sign bit clear
    tiles = keys >> 32
    ranges = st["ranges"].to(torch.int64)
    lens = ranges[:, 1] - ranges[:, 0]
    assert int(lens.sum()) == R and bool((lens >= 0).all())
    nz = lens > 0
    starts = ranges[nz, 0]
    assert bool((tiles[starts] == torch.nonzero(nz).flatten()).all()), "a tile's range starts at its own key"
    ends = ranges[nz, 1] - 1
    assert bool((tiles[ends] == torch.nonzero(nz).flatten()).all())
    # stable tie-break: equal keys keep ascending Gaussian index
    pl = st["point_list"][:R].to(torch.int64)
    same = keys[1:] == keys[:-1]
    assert bool((pl[1:][same] > pl[:-1][same]).all())
    # low key bits are the depth's float bits of the listed Gaussian
    dbits = st["depths"].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert bool(((keys & 0xFFFFFFFF) == dbits[pl]).all())
    # per-pixel bounds
    nc = st["n_contrib"].to(torch.int64)
    gy, gx = (H + 15) // 16, (W + 15) // 16
    tile_of_pixel = (torch.arange(H, device=gpu)[:, None] // 16) * gx + torch.arange(W, device=gpu)[None, :] // 16
    assert bool((nc <= lens[tile_of_pixel]).all())
    assert bool(torch.isfinite(color).all()) and float(color.min()) >= 0.0
    fT = st["final_T"]
    assert bool(((fT >= 0) & (fT <= 1)).all())
    d = depth[0]
    vis_depth = st["depths"][radii > 0]
    assert bool(((d == 15.0) | ((d >= vis_depth.min()) & (d <= vis_depth.max()))).all()), "median depth is a listed depth or the default"
    assert int((radii > 0).sum()) > 0.9 * P and T == ranges.shape[0]


def test_forward_is_deterministic_and_variant_invariant(scenes, rast, gpu):
    """1M Gaussians at 1080p: identical bits from two runs, with / without wave-level culling, with /
    without heaviest-first launch order, for 1 / 2 / 4 pixels per lane and both binning schemes (all on the
    reference's literal lists, tile_clip=0); the default row-clipped lists (tile_clip=1) must give the same
    colour / depth / transmittance bits."""
    P, W, H = 1_000_000, 1920, 1080
    sc, cam, rs, ten = _inputs(scenes, rast, P, W, H, gpu)
    _C = rast._C

    def fwd():
        R, color, radii, depth, st = _forward_state(rast, rs, ten, P, W, H)
        return R, color.clone(), depth.clone(), st["n_contrib"].clone(), st["final_T"].clone(), st["point_list"].clone(), st["ranges"].clone()

    clipped = fwd()          # product default
    _C.set_option("tile_clip", 0)
    base = fwd()
    assert clipped[0] == base[0]
    for i in (1, 2, 4):
        assert torch.equal(clipped[i], base[i]), "row-clipped lists changed an output bit"
    variants = [dict(), dict(binning=1), dict(cull=0), dict(lpt=0), dict(pixels_per_lane=1, cull=0), dict(pixels_per_lane=2, cull=0), dict(pixels_per_lane=4, cull=0)]
    try:
        for v in variants:
            for k, val in v.items():
                _C.set_option(k, val)
            got = fwd()
            assert got[0] == base[0]
            for a, b in zip(got[1:], base[1:]):
                assert torch.equal(a, b), f"forward differs under {v}"
            for k in v:
                _C.set_option(k, 1 if k in ("cull", "lpt") else 0)
    finally:
        _C.set_option("cull", 1); _C.set_option("lpt", 1); _C.set_option("pixels_per_lane", 0); _C.set_option("binning", 0)
        _C.set_option("tile_clip", 1)


@pytest.mark.parametrize("name,P,W,H", CONFIGS[:2], ids=[c[0] for c in CONFIGS[:2]])
def test_backward_is_linear_in_the_upstream_gradient(name, P, W, H, scenes, rast, gpu):
    """grad(a*g1 + b*g2) == a*grad(g1) + b*grad(g2) up to float-atomic ordering; depth gets no gradient;
    culled Gaussians get exactly zero."""
    sc, cam, rs, ten = _inputs(scenes, rast, P, W, H, gpu)
    g1 = torch.as_tensor(scenes.upstream_grad(H, W, 1), device=gpu)
    g2 = torch.as_tensor(scenes.upstream_grad(H, W, 2), device=gpu)

    def grads(g):
        leaves = {k: v.clone().requires_grad_(True) for k, v in ten.items()}
        m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii, depth = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                                          shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
        assert depth.requires_grad and not radii.requires_grad and radii.dtype == torch.int32      # (depth: as the reference, __init__.py:85-88)
        color.backward(g)
        out = {k: v.grad for k, v in leaves.items()}
        out["means2D"] = m2.grad
        return out, radii

    ga, radii = grads(g1)
    gb, _ = grads(g2)
    gc, _ = grads(2.0 * g1 - 0.5 * g2)
    dead = radii == 0
    for k in ga:
        want = 2.0 * ga[k] - 0.5 * gb[k]
        err = (gc[k] - want).abs()
        assert bool((err <= 1e-6 + 1e-3 * want.abs()).all()), (k, float(err.max()))
        assert bool(torch.isfinite(gc[k]).all())
        assert not bool(gc[k][dead].any()), k
    assert bool((ga["means2D"][:, 2] == 0).all())      # only .x/.y of the screen-space gradient are written


def test_more_than_65536_tiles(orc, scenes, rast, gpu):
    """4112 x 4112 pixels = 257 x 257 tiles: the run-compressed binning (<= 256 tile rows, 16-bit tile ids) and the
    work-bucket launch order (u16 tile ids) step aside for the instance-level sort on 32-bit tile ids and
    tile_order_kernel.  Few Gaussians, so the oracle still finishes in seconds: exact comparison."""
    from gpu_harness import bits, run_hip
    W = H = 4112
    P = 400
    sc = scenes.synth(P, 161, scale_mul=0.5)
    cam = scenes.camera(0, 1, W, H)
    g = scenes.upstream_grad(H, W, 162)
    o32 = orc.render(sc, cam, g)
    h = run_hip(rast, sc, cam, gpu, dL_dcolor=g, tile_clip=1)
    assert h["R"] == o32["R"]
    np.testing.assert_array_equal(h["point_list"], o32["point_list"])       # tile_clip has no effect on this path
    np.testing.assert_array_equal(h["ranges"], o32["ranges"])
    np.testing.assert_array_equal(h["n_contrib"], o32["n_contrib"])
    np.testing.assert_array_equal(bits(h["out_color"]), bits(o32["out_color"]))
    np.testing.assert_array_equal(bits(h["out_depth"]), bits(o32["out_depth"]))
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"):
        ref = o32[k].astype(np.float64)
        err = np.abs(h[k].astype(np.float64).reshape(ref.shape) - ref)
        assert (err <= 1e-5 + 1e-3 * np.abs(ref)).all(), (k, float(err.max()))


@pytest.mark.parametrize("W,H", [(4128, 512), (512, 4096), (4112, 3984)], ids=["258_tile_columns", "256_tile_rows", "64k_tiles_run_path"])
def test_extreme_aspect_ratios_on_the_run_path(W, H, orc, scenes, rast, gpu):
    """Run-compressed binning at its limits: more than 256 tile columns (two radix passes over the runs), exactly 256
    tile rows (8-bit row digit fully used), and just under 65536 tiles."""
    from gpu_harness import bits, run_hip
    P = 600
    sc = scenes.synth(P, 171, scale_mul=0.7)
    cam = scenes.camera(1, 3, W, H)
    g = scenes.upstream_grad(H, W, 172)
    o32 = orc.render(sc, cam, g)
    for clip in (0, 1):
        h = run_hip(rast, sc, cam, gpu, dL_dcolor=g, tile_clip=clip)
        assert h["R"] == o32["R"]
        if clip == 0:
            np.testing.assert_array_equal(h["point_list"], o32["point_list"])
            np.testing.assert_array_equal(h["ranges"], o32["ranges"])
        np.testing.assert_array_equal(bits(h["out_color"]), bits(o32["out_color"]))
        np.testing.assert_array_equal(bits(h["out_depth"]), bits(o32["out_depth"]))
        for k in ("dL_dmeans3D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations"):
            ref = o32[k].astype(np.float64)
            err = np.abs(h[k].astype(np.float64).reshape(ref.shape) - ref)
            assert (err <= 1e-5 + 1e-3 * np.abs(ref)).all(), (k, float(err.max()))


@pytest.mark.parametrize("depth_sort", [1, 0], ids=["radix", "buckets"])
@pytest.mark.parametrize("radius,short", [(4.0, True), (9.0, True), (2.6, False), (1.5, False)],
                         ids=["depths_1p7_to_6p3_three_passes", "depths_cross_8_three_passes", "wide_range_four_passes", "near_plane_four_passes"])
@pytest.mark.remembered_cut_only
def test_adaptive_depth_sort_pass_count(radius, short, depth_sort, orc, scenes, rast, gpu):
    """The depth sort of > 131072 Gaussians decides ON THE DEVICE whether its fourth 8-bit pass is needed: digits of passes 2-4
    are taken from key - base (base = smallest visible key, low byte cleared), and a key span below 2^24 is sorted after three
    passes -- also when the depths straddle a power of two (camera distance 4: 1.7 .. 6.3; distance 9: across 8).  Wide depth
    ranges run all four passes.  Either way the lists equal the oracle's 64-bit key sort entry by entry."""
    from gpu_harness import bits, run_hip
    P, W, H = 300_000, 640, 480
    sc = scenes.synth(P, 5)
    cam = scenes.camera(1, 7, W, H, radius=radius)
    o32 = orc.render(sc, cam)
    rast._C.set_option("depth_sort", depth_sort)      # 1: the radix passes this test is about; 0: the default bucket sort on the same depth ranges
    try:
        h = run_hip(rast, sc, cam, gpu, tile_clip=0)
    finally:
        rast._C.set_option("depth_sort", 0)
    d = o32["depths"][o32["radii"] > 0].view(np.uint32).astype(np.int64)
    assert ((d.max() - (d.min() & ~0xFF)) < (1 << 24)) == short           # the regime this case is meant to exercise
    assert h["R"] == o32["R"]
    np.testing.assert_array_equal(h["keys_sorted"], o32["keys_sorted"])
    np.testing.assert_array_equal(h["point_list"], o32["point_list"])
    np.testing.assert_array_equal(h["ranges"], o32["ranges"])
    np.testing.assert_array_equal(bits(h["out_color"]), bits(o32["out_color"]))


@pytest.mark.remembered_cut_only
def test_depth_sort_pass_hint_follows_the_scene(orc, scenes, rast, gpu):
    """The context remembers whether the last forward's depth keys were short and then enqueues three sort passes instead of
    four; when the next view's depth range is wide after all, the device says so in the read-back and the sort is repeated
    (redo_count).  Sequence short, short, wide, wide, short: every forward equals the oracle, exactly one redo."""
    from gpu_harness import run_hip
    P, W, H = 200_000, 480, 360
    sc = scenes.synth(P, 6)
    _C = rast._C
    want = {}
    redo0 = None
    _C.set_option("depth_sort", 1)         # the radix sort (the default bucket sort has no pass count)
    try:
        for step, radius in enumerate([4.0, 4.0, 2.6, 2.6, 4.0]):
            cam = scenes.camera(2, 7, W, H, radius=radius)
            if radius not in want:
                want[radius] = orc.render(sc, cam)
            o32 = want[radius]
            if step == 1:
                redo0 = _C.get_option("redo_count")
            h = run_hip(rast, sc, cam, gpu, tile_clip=0)            # two forwards per call (state export + autograd module)
            np.testing.assert_array_equal(h["point_list"], o32["point_list"], err_msg=f"step {step}")
            np.testing.assert_array_equal(h["ranges"], o32["ranges"])
            np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))
        assert _C.get_option("redo_count") - redo0 == 1
    finally:
        _C.set_option("depth_sort", 0)


@pytest.mark.remembered_cut_only
def test_bucket_depth_sort_overflow_falls_back_to_radix(orc, scenes, rast, gpu, scatter_form):
    """The default depth sort puts the Gaussians into ~P/256 depth buckets of fixed capacity (of equal population by a sampled depth
    histogram, round 4).  A scene whose depths pile up beyond any histogram's resolution -- here
    three thin sheets facing the camera, 20 000 Gaussians at (nearly) one depth each -- overflows a bucket: the device reports it
    with the instance counts, the forward repeats the sort with the radix passes (one redo) and the context goes straight to
    those for its next calls.  Every forward equals the oracle entry by entry; equal depths fall in index order."""
    from gpu_harness import run_hip
    P, W, H = 60_000, 480, 360
    sc = scenes.synth(P, 9)
    cam = scenes.camera(0, 5, W, H)
    # flatten the cloud onto three planes perpendicular to the viewing direction (view matrix row 2 = the depth axis)
    V = np.asarray(cam["viewmatrix"], dtype=np.float64).reshape(4, 4)       # stored transposed: V[c][r]
    axis = V[:3, 2] / np.linalg.norm(V[:3, 2])
    m = sc["means3D"].astype(np.float64)
    layer = (np.arange(P) % 3 - 1) * 0.4
    m = m - np.outer(m @ axis, axis) + np.outer(layer, axis)
    sc = dict(sc); sc["means3D"] = m.astype(np.float32)
    o32 = orc.render(sc, cam)
    nvis = int((o32["radii"] > 0).sum())
    assert nvis > 30_000 and np.unique(o32["depths"][o32["radii"] > 0]).size < nvis // 20      # many exactly equal depth keys
    _C = rast._C
    assert _C.get_option("depth_sort") == 0
    redo0 = _C.get_option("redo_count")
    try:
        for step in range(2):
            h = run_hip(rast, sc, cam, gpu, tile_clip=0)            # two forwards per call
            assert h["R"] == o32["R"]
            np.testing.assert_array_equal(h["keys_sorted"], o32["keys_sorted"], err_msg=f"step {step}")
            np.testing.assert_array_equal(h["point_list"], o32["point_list"])
            np.testing.assert_array_equal(h["ranges"], o32["ranges"])
            np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))
            if step == 0:
                # (round 4: the context's first overflow under a depth histogram that was not made for this view -- a fresh context's
                # coarse one, or another scene's range -- only re-learns the range; the second forward's fine histogram cannot pull
                # 20 000 equal keys apart either, and THAT starts the pause)
                redos = _C.get_option("redo_count") - redo0
                assert redos in (1, 2), "the first forward must have re-sorted"
                assert _C.get_option("bucket_skip") > 0
        assert _C.get_option("redo_count") - redo0 == redos, "later forwards start with the radix sort"
    finally:
        # let the context forget: an ordinary scene, until the bucket sort is tried (and kept) again
        sc2 = scenes.synth(P, 10)
        for _ in range(2100):       # 16 forwards after a first overflow; the pause doubles with every further one (capped at 4096)
            if _C.get_option("bucket_skip") == 0:
                break
            run_hip(rast, sc2, cam, gpu, tile_clip=0)
        assert _C.get_option("bucket_skip") == 0


@pytest.mark.remembered_cut_only
def test_bucket_depth_sort_ties_fall_in_index_order(orc, scenes, rast, gpu, scatter_form):
    """Every Gaussian twice (same mean, different appearance): all depth keys come in equal pairs.  The bucket sort orders a bucket by
    (depth bits, index), so the lists equal the oracle's stable 64-bit key sort entry by entry -- and no bucket overflows."""
    from gpu_harness import run_hip
    P, W, H = 30_000, 400, 300
    a, b = scenes.synth(P, 11), scenes.synth(P, 12)
    sc = {k: (np.concatenate([a[k], b[k]], axis=0) if isinstance(a[k], np.ndarray) and a[k].shape[:1] == (P,) else a[k]) for k in a}
    sc["means3D"] = np.concatenate([a["means3D"], a["means3D"]], axis=0)
    cam = scenes.camera(3, 8, W, H)
    o32 = orc.render(sc, cam)
    _C = rast._C
    redo0 = _C.get_option("redo_count")
    h = run_hip(rast, sc, cam, gpu, tile_clip=0)
    assert _C.get_option("redo_count") == redo0 and _C.get_option("bucket_skip") == 0
    assert h["R"] == o32["R"]
    np.testing.assert_array_equal(h["keys_sorted"], o32["keys_sorted"])
    np.testing.assert_array_equal(h["point_list"], o32["point_list"])
    np.testing.assert_array_equal(h["ranges"], o32["ranges"])
    np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))


@pytest.mark.remembered_cut_only
def test_bucket_depth_sort_edge_populations(orc, scenes, rast, gpu, scatter_form):
    """Bucket-sort path (P >= 32768) with nothing visible, with one visible Gaussian, and with all visible Gaussians at exactly one depth
    among culled ones: outputs equal the oracle; an empty scene renders the background."""
    from gpu_harness import run_hip
    P, W, H = 40_000, 160, 120
    cam = scenes.camera(0, 3, W, H)
    base = scenes.synth(P, 21)
    far = np.array(cam["campos"], np.float32) * 3.0                     # behind the camera (it looks at the origin)
    for nvis in (0, 1, 5000):
        sc = dict(base)
        m = np.tile(far, (P, 1)).astype(np.float32)
        m[:nvis] = base["means3D"][:nvis]
        sc["means3D"] = m
        o32 = orc.render(sc, cam)
        assert int((o32["radii"] > 0).sum()) in ((0,) if nvis == 0 else range(1, nvis + 1))
        h = run_hip(rast, sc, cam, gpu, tile_clip=0)
        assert h["R"] == o32["R"]
        np.testing.assert_array_equal(h["radii"], o32["radii"])
        np.testing.assert_array_equal(h["point_list"], o32["point_list"])
        np.testing.assert_array_equal(h["ranges"], o32["ranges"])
        np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))
    assert rast._C.get_option("bucket_skip") == 0


@pytest.mark.remembered_cut_only
def test_bucket_depth_sort_with_an_undersized_speculative_launch(orc, scenes, rast, gpu, scatter_form):
    """The bucket sort leaves the instance counts to the run emission of the speculative launch.  A view with far more instances than
    the context's capacity hint: the emission is bounded by the capacity, the counts still come out right, the launch is repeated with
    exact sizes (one redo) and the lists equal the oracle's; then a small view inside the oversized capacity."""
    from gpu_harness import run_hip
    _C = rast._C
    W, H = 320, 240
    seq = [(40_000, 0.5, 9.0), (60_000, 2.0, 4.0), (40_000, 0.5, 9.0)]       # (P, scale multiplier, camera distance)
    redo0 = _C.get_option("redo_count")
    for n, (P, sm, radius) in enumerate(seq):
        sc = scenes.synth(P, 31 + n, scale_mul=sm)
        cam = scenes.camera(n, 5, W, H, radius=radius)
        o32 = orc.render(sc, cam)
        for clip in (0, 1):
            h = run_hip(rast, sc, cam, gpu, tile_clip=clip)
            assert h["R"] == o32["R"], (n, clip)
            if clip == 0:
                np.testing.assert_array_equal(h["point_list"], o32["point_list"])
                np.testing.assert_array_equal(h["ranges"], o32["ranges"])
            np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))
    assert _C.get_option("redo_count") - redo0 >= 1 and _C.get_option("bucket_skip") == 0


@pytest.mark.remembered_cut_only
def test_bucket_depth_sort_equalises_a_peaked_depth_distribution(orc, scenes, rast, gpu, scatter_form):
    """Round 4: the depth buckets are cut by a sampled depth histogram (equal population), not into equal depth intervals.  A scene
    with 70 % of its Gaussians in a layer 0.06 deep (a wall facing the camera, normal depth profile, sigma 0.03 of a depth range of
    3.3) put ten times a bucket's capacity into a few equal-width buckets (10 000 in one of 512); now the first forward of the
    context may still fall back (its histogram has four bins per octave), the following ones -- also from other poses, and after
    the wall has moved -- keep the bucket sort (no redo, no pause) and equal the oracle entry by entry.  (What the histogram cannot
    resolve is a DISCONTINUITY of the density inside one of its bins -- a hard-edged slab: the radix path takes that)"""
    from gpu_harness import run_hip
    P, W, H = 120_000, 480, 360
    sc = scenes.synth(P, 41)
    cam0 = scenes.camera(0, 6, W, H)
    V = np.asarray(cam0["viewmatrix"], dtype=np.float64).reshape(4, 4)
    axis = V[:3, 2] / np.linalg.norm(V[:3, 2])
    rng = np.random.default_rng(42)
    m = sc["means3D"].astype(np.float64)
    wall = rng.random(P) < 0.7
    depth_off = rng.normal(0.3, 0.03, size=P)
    m[wall] = m[wall] - np.outer(m[wall] @ axis, axis) + np.outer(depth_off[wall], axis)
    sc = dict(sc); sc["means3D"] = m.astype(np.float32)
    sc["opacities"] = (sc["opacities"] * 0.05).astype(np.float32)          # (translucent: the lists are consumed deep into the wall)
    _C = rast._C
    run_hip(rast, sc, cam0, gpu, tile_clip=0)                               # lets the context learn the range (may fall back once)
    for _ in range(40):                                                    # (a pause left by another test)
        if _C.get_option("bucket_skip") == 0:
            break
        run_hip(rast, sc, cam0, gpu, tile_clip=0)
    assert _C.get_option("bucket_skip") == 0
    run_hip(rast, sc, cam0, gpu, tile_clip=0)
    redo0 = _C.get_option("redo_count")
    for k, shift in ((0, 0.0), (1, 0.0), (0, 0.35), (2, -0.2)):
        scn = dict(sc); scn["means3D"] = (m + np.outer(np.where(wall, shift, 0.0), axis)).astype(np.float32)
        cam = scenes.camera(k, 6, W, H)
        o32 = orc.render(scn, cam)
        h = run_hip(rast, scn, cam, gpu, tile_clip=0)
        assert h["R"] == o32["R"]
        np.testing.assert_array_equal(h["point_list"], o32["point_list"], err_msg=f"pose {k} shift {shift}")
        np.testing.assert_array_equal(h["ranges"], o32["ranges"])
        np.testing.assert_array_equal(h["out_color"].view(np.uint32), o32["out_color"].view(np.uint32))
    assert _C.get_option("redo_count") == redo0 and _C.get_option("bucket_skip") == 0


@pytest.mark.remembered_cut_only
def test_list_cut_engages_under_pose_alternation(scenes, rast, gpu):
    """the pose table must work in the reference's call pattern -- different cameras one after the other
    (train.py:198-226) -- not only on one repeated pose.  Four poses of a ring dealt round-robin over the 3 M-Gaussian cube (the
    diagonal views' depth histogram has a peak: rounds 2-3's equal-width depth buckets overflowed there, the forward fell back
    to the radix sort with a growing pause and the cut never engaged again): from every pose's second visit on the list cut is in
    force (more than a quarter of the Gaussians late), no forward is redone, no pause is set -- by the library's own defaults,
    no `list_cut_always`.  Outputs of a cut visit equal the first visit's bit for bit."""
    import torch
    from conftest import settings_from
    _C = rast._C
    P, W, H, V = 3_000_000, 1920, 1080, 4
    sc = scenes.synth(P, 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    e = torch.empty(0)
    cams = [scenes.camera(k, 8, W, H) for k in range(V)]
    rss = [settings_from(rast, c, sc, gpu) for c in cams]

    def render(k):
        rs = rss[k]
        R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(
            rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
            rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
        return R, color, depth, _C.context_query("last_late")

    for k in range(V):                    # lets the context size its launches and learn the depth range (first forwards may be redone)
        render(k)
    first = {}
    for k in range(V):
        first[k] = render(k)
    redo0 = _C.get_option("redo_count")
    for visit in range(3):
        for k in range(V):
            R, color, depth, late = render(k)
            assert late > P // 4, f"visit {visit} of pose {k}: the list cut is not in force (late = {late})"
            assert R == first[k][0] and torch.equal(color, first[k][1]) and torch.equal(depth, first[k][2])
    assert _C.get_option("redo_count") == redo0 and _C.get_option("bucket_skip") == 0


@pytest.mark.remembered_cut_only
def test_list_cut_pauses_itself_when_its_lists_keep_failing(scenes, rast, gpu):
    """SaRO-GS renders one camera at many timestamps, and opacity = sigmoid(.) * trbf(t) makes two visits of a pose different scenes
    (scene/saro_gaussian.py:788-831).  A failed speculation is correct but costs a whole second forward; the device reports it
    to the host (a pinned word written by the predicated second binning), and a context whose cut lists keep failing stops
    cutting: here one pose, the scene alternating between opaque and nearly transparent on every call -- by the library's own
    defaults (no list_cut_always) at most three forwards fall back before the cut pauses itself; every output equals the
    cut-less render bit for bit."""
    import torch
    from conftest import settings_from
    _C = rast._C
    P, W, H = 1_000_000, 1920, 1080
    sc = scenes.synth(P, 0)
    cam = scenes.camera(0, 8, W, H)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    thin = ten["opacities"] * 0.03
    e = torch.empty(0)
    rs = settings_from(rast, cam, sc, gpu)

    def render(op):
        R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(
            rs.bg, ten["means3D"], e, op, ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
            rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
        return R, color, depth

    _C.set_option("no_list_cut", 1)
    try:
        want = {0: render(ten["opacities"]), 1: render(thin)}
    finally:
        _C.set_option("no_list_cut", 0)
    for _ in range(3):
        render(ten["opacities"])                        # the context learns the opaque scene's cut depths
    assert _C.context_query("last_late") > P // 4 and _C.context_query("cut_pause") == 0
    fb0 = _C.context_query("cut_fallbacks")
    for i in range(24):
        k = (i + 1) % 2                                 # transparent, opaque, transparent, ...
        R, color, depth = render(thin if k else ten["opacities"])
        assert R == want[k][0] and torch.equal(color, want[k][1]) and torch.equal(depth, want[k][2]), f"call {i}"
    fallbacks = _C.context_query("cut_fallbacks") - fb0
    assert 1 <= fallbacks <= 3, fallbacks
    assert _C.context_query("cut_pause") > 0
    for _ in range(40):                                 # (leave the context as the next test expects it: the pause served)
        if _C.context_query("cut_pause") == 0:
            break
        render(ten["opacities"])


def test_list_cut_under_a_scene_that_varies_per_call(scenes, rast, gpu):
    """SaRO-GS's main training stage renders every camera at another timestamp each time -- opacity =
    sigmoid(.) * exp(-4 ((t - pos) / lifespan)^2) for every Gaussian (scene/saro_gaussian.py:791-792, :824-829), means, rotations and scales
    moved by the deformation field (:805-822) -- so two visits of a pose are different scenes and a cut depth remembered from the last
    visit is too short every other time (round 4: the context paused its cut and ran at 0.96-1.00 x the table-off rate).  Round 5: the
    remembered cut is a running maximum over visits, and a wide failure switches the context to PREDICTED cut depths, computed from the
    call's own opacities.  At 3 M Gaussians, four poses dealt round-robin, a random timestamp per call, by the library's own defaults:
    EVERY call equals its cut-less twin bit for bit, and the context does not thrash -- completion passes stay rare once the policy has
    settled (what the cut then removes in this half-transparent scene is reported, not asserted: it is little, and the policy may sit out)."""
    import torch
    import bench
    from conftest import settings_from
    _C = rast._C
    P, W, H, V = 3_000_000, 1920, 1080, 4
    sc = scenes.synth(P, 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    e = torch.empty(0)
    rss = [settings_from(rast, scenes.camera(k, 8, W, H), sc, gpu) for k in range(V)]
    deform = bench.Deformation(P, gpu, seed=11, motion=True)
    log_scale = torch.log(ten["scales"])

    def scene_at(i):
        mres, rres, trbf = deform.at(i)
        with torch.no_grad():
            rot = torch.nn.functional.normalize(ten["rotations"] + rres[:, :4])
            return ten["means3D"] + mres, ten["opacities"] * trbf, torch.exp(log_scale + rres[:, 4:]), rot

    def render(k, inp):
        rs = rss[k]
        means, op, scl, rot = inp
        R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(
            rs.bg, means, e, op, scl, rot, 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
        return R, color, depth

    def twin(k, inp):
        _C.set_option("no_list_cut", 1)
        try:
            return render(k, inp)
        finally:
            _C.set_option("no_list_cut", 0)

    n_warm, n = 10 * V, 60
    for i in range(n_warm):                       # the context sizes its launches, learns the depth range and the poses' cuts; early failures shape the policy
        render(i % V, scene_at(i))
    torch.cuda.synchronize()
    p0, cut_calls, late_sum = _C.context_query("completion_passes"), 0, 0
    for i in range(n_warm, n_warm + n):
        inp = scene_at(i)
        R, color, depth = render(i % V, inp)
        late = _C.context_query("last_late")
        cut_calls += int(late > 0); late_sum += late
        R0, color0, depth0 = twin(i % V, inp)
        assert R == R0 and torch.equal(color, color0) and torch.equal(depth, depth0), f"call {i} (late = {late})"
    torch.cuda.synchronize()
    passes = _C.context_query("completion_passes") - p0
    print(f"varying scene at 3 M: cut applied on {cut_calls} of {n} calls (mean late {late_sum // max(cut_calls, 1)}), {passes} completion passes, "
          f"pause {_C.context_query('cut_pause')}, margin {_C.context_query('cut_margin_x4')} / 4, tau_req {_C.context_query('tau_req')}, tau_force {_C.context_query('tau_force')}")
    assert passes <= n // 4, passes


def test_predicted_cut_at_full_size_without_the_pose_table(scenes, rast, gpu):
    """BASELINE cfg5 (3 M Gaussians @ 1080p) with the context's pose table switched off: every forward is a first visit.  From the third
    forward on (the context has learned the depth range and its launch sizes) the PREDICTED cut is in force by the library's own defaults --
    more than a quarter of the Gaussians late -- and every forward equals its cut-less twin bit for bit."""
    import torch
    from conftest import settings_from
    _C = rast._C
    P, W, H, V = 3_000_000, 1920, 1080, 4
    sc = scenes.synth(P, 0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    ten = {k: t(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    e = torch.empty(0)
    rss = [settings_from(rast, scenes.camera(k, 8, W, H), sc, gpu) for k in range(V)]

    def render(k):
        rs = rss[k]
        R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(
            rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
            rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
        return R, color, depth

    _C.set_option("no_order_hint", 1)
    try:
        _C.set_option("no_list_cut", 1)
        want = [render(k) for k in range(V)]
        _C.set_option("no_list_cut", 0)
        for k in range(V):
            render(k)
        p0, lates = _C.context_query("completion_passes"), []
        for visit in range(3):
            for k in range(V):
                R, color, depth = render(k)
                lates.append(_C.context_query("last_late"))
                assert R == want[k][0] and torch.equal(color, want[k][1]) and torch.equal(depth, want[k][2]), (visit, k)
        torch.cuda.synchronize()
        print("predicted cut at 3 M, table off: late per call", lates, "completion passes", _C.context_query("completion_passes") - p0, "tau_req", _C.context_query("tau_req"))
        assert min(lates) > P // 4, lates
    finally:
        _C.set_option("no_list_cut", 0)
        _C.set_option("no_order_hint", 0)


def test_stale_gradient_records_at_full_size(scenes, rast, gpu):
    """BASELINE cfg5 (3 M Gaussians @ 1080p), the library's own defaults (list cut, untouched bits, grouped per-Gaussian backward, only the
    consumed Gaussians' gradient records zeroed): a step whose state buffers were handed out full of 0xFF bytes gives the same gradients as
    a step with the records zeroed whole -- finite everywhere, the same rows zero -- directly and through the dL/dsh factor path
    (sh_factor_kernel + gsrast_sh_grad_combine read the records too)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    import view_parallel as vp
    _C = rast._C
    P, W, H = 3_000_000, 1920, 1080
    wl = bench.Workload(rast, scenes, P, W, H, 3, view_k=1, n_views=8, dev=gpu)
    wl.keep_grads = True            # (this test reads the leaves' .grad after step())
    for _ in range(3):
        wl.step(None, 1)            # (the context learns its launch sizes and the pose's cut depths)
    ref = None
    for arena_mode in (False, True):
        arena = _C.GradArena(P, 16, gpu, sh_factors=True, world=1) if arena_mode else None
        _C.set_grad_arena(arena)
        try:
            got = {}
            for sparse in (0, 1):
                _C.set_option("sparse_grec", sparse)
                _C.POISON_STATE_BUFFERS = bool(sparse)
                wl.step(arena, 1)
                if arena_mode:
                    vp.exchange_gradients(arena, wl.leaves["means3D"].detach(), 1)
                torch.cuda.synchronize()
                got[sparse] = {k: v.grad.detach().clone() for k, v in wl.leaves.items()}
                assert _C.context_query("last_late") > P // 4
        finally:
            _C.POISON_STATE_BUFFERS = False
            _C.set_option("sparse_grec", 1)
            _C.set_grad_arena(None)
        for k in got[1]:
            a, b = got[1][k].reshape(P, -1), got[0][k].reshape(P, -1)
            assert bool(torch.isfinite(a).all()), (arena_mode, k)
            assert torch.equal((a != 0).any(1), (b != 0).any(1)), (arena_mode, k)
            assert bool(((a - b).abs() <= 1e-6 + 1e-3 * b.abs()).all()), (arena_mode, k)      # (float-atomic order differs between two backwards)
            if ref is not None:
                assert bool(((a - ref[k].reshape(P, -1)).abs() <= 1e-6 + 1e-3 * a.abs()).all()), k
        ref = got[1] if ref is None else ref
