"""-m gpu: each pixel's first or heaviest K contributors (`pixel_contributors`; include/gsrast.h: gsrast_pixel_contributors,
csrc/gsrast_topk.h) against tests/topk_math.py -- torch fp64 on tests/math_renderer.py -- and against the features already merged.

Cases (contrib_math.CASES), image 70 x 45 = 5 x 3 tiles, ragged in both axes.  a: 622 Gaussians in one tile's list (more than two 256-entry
batches), pixels with up to 163 contributors, 48 % of the pixels with more than 8 and 14 % with more than 16: the weight order's
insertion runs full and drops pairs, the depth order stops filling early.  b: at most 8 contributors per pixel, 37 % of the pixels with
none: nothing is truncated at K = 16, unused slots everywhere.  (tests/test_topk_host.py asserts these facts, and that under 5 % of the
pixels are ambiguous.)

Against fp64: on the pixels that are not ambiguous (topk_math.ambiguous: math_renderer's own mask; in weight order also a gap below 1e-4
relative among the sorted top-(K + 1) weights) ids and count equal the restatement exactly and
    |w_gpu - w64| <= 4 max|w32 - w64| + 2^-23
w32 the restatement run with dtype=float32, the maximum over the case's non-ambiguous K = 16 entries (topk_math.bar; measured on the CPU:
max|w32 - w64| = 2.5e-7 ... 2.8e-7 for case a, 1.4e-6 ... 3.5e-6 for case b, a little different from one host's float32 exp to another's).
The factor 4 is the margin tests/test_gpu_contrib.py takes for the same reason: the HIP path rounds like fp32, not like the fp64 reference.
Each test prints its worst |err| / bar; measured on the MI355X: no pixel with other ids or another count, worst |err| / bar 0.25 on case a
(all three exp modes) and 0.19 / 0.25 on case b without / with antialiasing.  The grid: exp_mode 0 over both cases x antialiasing off / on x both orders x K in {1, 3, 8, 16}; exp_mode 1 and 2 -- the same
kernel with another exp, whose error shows in every K alike -- on case a (the longest lists) at K = 16, both orders, antialiasing off / on.

Against contrib (same state, no pixel weights) and in the edge cases nothing has a tolerance: the replay's w are the forward's own bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import contrib_math as cm
import topk_math as tm
from conftest import settings_from

pytestmark = pytest.mark.gpu

DENSE = ("means3D", "opacities", "shs", "scales", "rotations")


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _dense(sc, gpu):
    return {n: _t(sc[n], gpu) for n in DENSE}


def _query(rast, gpu, sc, cam, K, order, aa=False, ten=None):
    ten = ten or _dense(sc, gpu)
    pc = rast.pixel_contributors(ten["means3D"], ten["opacities"], ten["scales"], ten["rotations"], raster_settings=settings_from(rast, cam, sc, gpu),
                                 K=K, order=order, shs=ten["shs"], antialiasing=aa)
    torch.cuda.synchronize()
    return pc


def _state(rast, gpu, sc, cam, aa=False):
    """(R, color, radii, geom, binning, image, depth) of one forward-only dense render, and its settings."""
    rs = settings_from(rast, cam, sc, gpu)
    ten = _dense(sc, gpu)
    e = torch.empty(0)
    st = rast._C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                     rs.tanfovy, cam["image_height"], cam["image_width"], ten["shs"], int(sc.get("sh_degree", 3)), rs.campos, False,
                                     forward_only=True, antialiasing=aa)
    return st, rs


def _flat(x):
    """[K,H,W] -> numpy [N,K]; [H,W] -> [N]."""
    a = x.detach().cpu().numpy()
    return a.reshape(a.shape[0], -1).T if a.ndim == 3 else a.reshape(-1)


def _invariants(pc, K, order, what):
    """What holds on every pixel, ambiguous or not."""
    ids, w, cnt, radii = _flat(pc.ids), _flat(pc.weights), _flat(pc.count), pc.radii.cpu().numpy()
    assert pc.ids.dtype is torch.int32 and pc.count.dtype is torch.int32 and pc.weights.dtype is torch.float32
    assert ids.shape == w.shape == (cnt.shape[0], K), what
    used = ids >= 0
    assert (ids[~used] == -1).all() and (ids < len(radii)).all(), what
    assert np.array_equal(used, np.arange(K)[None, :] < used.sum(axis=1)[:, None]), (what, "-1 inside a pixel's list")
    assert not w[~used].any() and not np.signbit(w[~used]).any() and (w[used] > 0).all() and (w <= np.float32(0.99)).all(), what
    assert np.array_equal(used.sum(axis=1), np.minimum(K, cnt)), (what, "filled slots != min(K, count)")
    srt = np.sort(np.where(used, ids, -1 - np.arange(K)[None, :]), axis=1)      # (each unused slot a value of its own)
    assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "an id twice in one pixel")
    assert (radii[ids[used]] > 0).all(), (what, "an id of a culled Gaussian")
    if order == "weight":
        assert (w[:, 1:] <= w[:, :-1]).all(), (what, "weights not descending")
    return ids, w, cnt


def _against_fp64(rast, gpu, name, aa, exp_mode, grid):
    ref = tm.reference(name, aa)
    tol, worst32 = tm.bar(ref)
    rast._C.set_option("exp_mode", exp_mode)
    try:
        got = {(K, order): _query(rast, gpu, ref["sc"], ref["cam"], K, order, aa) for K, order in grid}
    finally:
        rast._C.set_option("exp_mode", 0)
    failures, worst = [], 0.0
    for (K, order), pc in got.items():
        what = f"case {name}, antialiasing {aa}, exp_mode {exp_mode}, K {K}, order {order}"
        radii = pc.radii.cpu().numpy()
        assert np.array_equal(radii > 0, ref["out"]["proj"]["disc"]["vis"]), "radius decision differs: pick another seed"
        ids, w, cnt = _invariants(pc, K, order, what)
        r_ids, r_w, r_cnt = (x.numpy() for x in tm.topk(ref, K, order))
        ok = ~tm.ambiguous(ref, K, order).numpy()
        assert ok.mean() > 0.95, what
        bad_ids, bad_cnt = int((ids[ok] != r_ids[ok]).any(axis=1).sum()), int((cnt[ok] != r_cnt[ok]).sum())
        err = float(np.abs(w[ok].astype(np.float64) - r_w[ok]).max())
        worst = max(worst, err / tol)
        print(f"{what}: non-ambiguous pixels {int(ok.sum())} / {ok.size}, pixels with other ids {bad_ids}, with another count {bad_cnt}, "
              f"max|w_gpu - w64| {err:.3e}, bar {tol:.3e} (max|w32 - w64| {worst32:.3e}), err / bar {err / tol:.3f}")
        if bad_ids or bad_cnt or not err <= tol:
            failures.append((what, bad_ids, bad_cnt, err, tol))
    print(f"case {name}, antialiasing {aa}, exp_mode {exp_mode}: worst err / bar {worst:.3f}")
    assert not failures, failures


# ---- 1. against the fp64 restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_against_fp64_every_k_and_order(name, aa, rast, gpu):
    _against_fp64(rast, gpu, name, aa, 0, [(K, order) for order in tm.ORDERS for K in (1, 3, 8, 16)])


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("exp_mode", [1, 2])
def test_against_fp64_the_other_exp_modes(exp_mode, aa, rast, gpu):
    _against_fp64(rast, gpu, "a", aa, exp_mode, [(16, order) for order in tm.ORDERS])


# ---- 2. against the features already merged: no tolerance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_against_contrib_on_the_same_state(name, aa, rast, gpu):
    _C = rast._C
    r = cm.reference(name, aa)
    sc, cam = r["sc"], r["cam"]
    P, H, W = sc["means3D"].shape[0], cam["image_height"], cam["image_width"]
    (R, _, radii, gb, bb, ib, _), _ = _state(rast, gpu, sc, cam, aa)
    sink = torch.full((P, 4), float("nan"), device=gpu)
    _C.contrib_stats(sink, None, R, W, H, gb, bb, ib)
    ids_w, w_w, count = _C.pixel_contributors(1, "weight", R, W, H, gb, bb, ib)
    ids_d, w_d, count_d = _C.pixel_contributors(16, "depth", R, W, H, gb, bb, ib, P=P)
    torch.cuda.synchronize()
    assert torch.equal(count, count_d) and int(count.max()) > 0
    top = torch.bincount(ids_w[0][ids_w[0] >= 0].long(), minlength=P)
    assert torch.equal(top.float(), sink[:, 3]), "slot 0 in weight order is not contrib's top Gaussian"
    assert int(count.sum()) == int(sink[:, 2].double().sum())
    if name == "b":      # at most 8 contributors per pixel: K = 16 holds every pair
        assert int(count.max()) <= 8
        used = ids_d >= 0
        assert torch.equal(torch.bincount(ids_d[used].long(), minlength=P).float(), sink[:, 2])
        wmax = torch.zeros(P, device=gpu).scatter_reduce(0, ids_d[used].long(), w_d[used], "amax", include_self=True)
        assert torch.equal(wmax, sink[:, 1]), "a weight differs from contrib's weight_max"
    else:
        assert int(count.max()) > 100 and int((count > 16).sum()) > 0


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------
def _assert_empty(pc_or_triple, K, H, W):
    ids, w, cnt = pc_or_triple[:3]
    assert tuple(ids.shape) == tuple(w.shape) == (K, H, W) and tuple(cnt.shape) == (H, W)
    assert bool((ids == -1).all()) and not bool(w.any()) and not bool(torch.signbit(w).any()) and not bool(cnt.any())


def test_no_gaussian_and_nothing_in_front_of_the_camera(rast, gpu):
    r = cm.reference("b")
    sc, cam = r["sc"], r["cam"]
    H, W = cam["image_height"], cam["image_width"]
    sc0 = {k: (v[:0] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in sc.items()}
    for K, order in ((1, "weight"), (16, "depth")):
        pc = _query(rast, gpu, sc0, cam, K, order)
        _assert_empty(pc, K, H, W)
        assert pc.radii.shape == (0,) and tuple(pc.color.shape) == (3, H, W)
    # every Gaussian mirrored through the camera centre: all behind it, no instance (R = 0)
    behind = dict(sc, means3D=(2.0 * np.asarray(cam["campos"], np.float32)[None, :] - sc["means3D"]).astype(np.float32))
    (R, _, radii, gb, bb, ib, _), _ = _state(rast, gpu, behind, cam)
    assert R == 0 and not bool(radii.any())
    for K, order in ((3, "weight"), (16, "depth")):
        _assert_empty(rast._C.pixel_contributors(K, order, R, W, H, gb, bb, ib), K, H, W)
    _assert_empty(_query(rast, gpu, behind, cam, 8, "weight"), 8, H, W)


@pytest.mark.parametrize("W,H", [(1, 1), (17, 16)])
def test_one_gaussian(W, H, rast, gpu, scenes):
    """One Gaussian at the image centre: count is 0 or 1, slot 0 holds row 0 with the pixel's alpha (T = 1 in front of it), every other slot
    is unused.  17 x 16: two tiles, the second one column wide."""
    cam = scenes.camera(1, 6, W, H)
    rng = np.random.default_rng(1)
    sc = cm._finish(rng, cam, np.array([(W - 1) / 2.0]), np.array([(H - 1) / 2.0]), np.array([3.0]), np.array([0.4]), np.array([0.8]))
    ten = _dense(sc, gpu)
    rs = settings_from(rast, cam, sc, gpu)
    with torch.no_grad():
        plain = rast.GaussianRasterizer(rs)(means3D=ten["means3D"], means2D=torch.zeros((1, 3), device=gpu), opacities=ten["opacities"], shs=ten["shs"],
                                            scales=ten["scales"], rotations=ten["rotations"], return_aux=True)
    alpha = plain[4][0]
    for K, order in ((1, "weight"), (4, "weight"), (16, "depth")):
        pc = _query(rast, gpu, sc, cam, K, order, ten=ten)
        _invariants(pc, K, order, f"one Gaussian, {W} x {H}, K {K}, {order}")
        assert int(pc.count.max()) == 1 and torch.equal(pc.count, (alpha > 0).int()) and torch.equal(pc.ids[0], torch.where(pc.count > 0, 0, -1).int())
        assert bool((pc.ids[1:] == -1).all()) and not bool(pc.weights[1:].any())
        # alpha = 1 - (1 - w): w up to the rounding of that difference
        assert float((pc.weights[0] - alpha).abs().max()) <= 2.0 ** -23, float((pc.weights[0] - alpha).abs().max())
        assert float(pc.weights[0].max()) > 0.5 and torch.equal(pc.radii, plain[1])


def test_count_null_through_the_c_abi_and_two_runs_are_equal(rast, gpu):
    _C = rast._C
    r = cm.reference("a")
    sc, cam = r["sc"], r["cam"]
    P, H, W = sc["means3D"].shape[0], cam["image_height"], cam["image_width"]
    (R, _, _, gb, bb, ib, _), _ = _state(rast, gpu, sc, cam)
    for K, order in ((5, "weight"), (16, "weight"), (7, "depth")):
        a = _C.pixel_contributors(K, order, R, W, H, gb, bb, ib)
        b = _C.pixel_contributors(K, order, R, W, H, gb, bb, ib, with_count=False, P=P)
        assert b[2] is None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # the C call itself: a NULL count, outputs inside larger allocations whose other bytes stay
        ids = torch.full((K + 2, H, W), 77, dtype=torch.int32, device=gpu)
        wts = torch.full((K + 2, H, W), 5.0, device=gpu)
        rc = _C.lib().gsrast_pixel_contributors(C.byref(_C._options_struct()), P, R, W, H, gb.data_ptr(), bb.data_ptr(), ib.data_ptr(), K, _C.TOPK_ORDERS[order],
                                                ids[1:].data_ptr(), wts[1:].data_ptr(), None, _C._stream_of(gpu))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(ids[1:K + 1], a[0]) and torch.equal(wts[1:K + 1], a[1])
        assert bool((ids[0] == 77).all()) and bool((ids[K + 1] == 77).all()) and bool((wts[0] == 5.0).all()) and bool((wts[K + 1] == 5.0).all())
    # smaller K are prefixes of K = 16, in both orders
    for order in tm.ORDERS:
        full = _C.pixel_contributors(16, order, R, W, H, gb, bb, ib)
        for K in (1, 3, 8):
            part = _C.pixel_contributors(K, order, R, W, H, gb, bb, ib)
            assert torch.equal(part[0], full[0][:K]) and torch.equal(part[1], full[1][:K]) and torch.equal(part[2], full[2])
    # two whole runs of the public call
    x, y = _query(rast, gpu, sc, cam, 16, "weight"), _query(rast, gpu, sc, cam, 16, "weight")
    assert all(torch.equal(p, q) for p, q in zip(x, y)) and int(x.count.max()) > 100


def test_raw_family_state_gives_the_dense_result(rast, gpu):
    import fused_epilogue
    _C = rast._C
    r = cm.reference("b")
    sc, cam = r["sc"], r["cam"]
    H, W = cam["image_height"], cam["image_width"]
    rs = settings_from(rast, cam, sc, gpu)
    sig = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1 - 1e-6)
    arrs = dict(xyz=sc["means3D"], rotation=sc["rotations"], scaling=np.log(sc["scales"].astype(np.float64)), opacity_logit=np.log(sig / (1 - sig)),
                features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:])
    raw = {n: (_t(arrs[n], gpu) if n in arrs else None) for n in _C.RAW_NAMES}
    R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians_raw(rs.bg, raw, 1.0, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, 3, rs.campos, forward_only=True)
    motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(raw["xyz"], raw["rotation"], raw["scaling"], raw["opacity_logit"], raw["features_dc"], raw["features_rest"])
    for K, order in ((16, "weight"), (4, "depth")):
        got = _C.pixel_contributors(K, order, R, W, H, gb, bb, ib)
        want = rast.pixel_contributors(motion, opa, scale, rot, raster_settings=rs, K=K, order=order, shs=shs)
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want[:3])) and int(got[2].max()) > 0
        assert torch.equal(color, want.color) and torch.equal(radii, want.radii)


def test_inputs_that_require_grad_an_arena_and_a_plain_forwards_outputs(rast, gpu):
    _C = rast._C
    r = cm.reference("b")
    sc, cam = r["sc"], r["cam"]
    P = sc["means3D"].shape[0]
    rs = settings_from(rast, cam, sc, gpu)
    want = _query(rast, gpu, sc, cam, 8, "weight")
    ten = {n: v.requires_grad_(True) for n, v in _dense(sc, gpu).items()}
    got = _query(rast, gpu, sc, cam, 8, "weight", ten=ten)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and not any(x.requires_grad or x.grad_fn is not None for x in got)
    assert all(v.grad is None for v in ten.values())
    arena = _C.GradArena(P, 16, gpu)
    _C.set_grad_arena(arena)
    try:
        arena.zero_grad()
        under = _query(rast, gpu, sc, cam, 8, "weight", ten=ten)
        assert not arena.dirty
    finally:
        _C.set_grad_arena(None)
    assert all(torch.equal(g, w) for g, w in zip(under, want))
    with torch.no_grad():
        plain = rast.GaussianRasterizer(rs)(means3D=ten["means3D"], means2D=torch.zeros((P, 3), device=gpu), opacities=ten["opacities"], shs=ten["shs"],
                                            scales=ten["scales"], rotations=ten["rotations"])
    assert torch.equal(want.color, plain[0]) and torch.equal(want.radii, plain[1]) and torch.equal(want.depth, plain[2])
    # without colours the query is the same; with colors_precomp the colour is that render's
    nocol = rast.pixel_contributors(ten["means3D"], ten["opacities"][:, 0], ten["scales"], ten["rotations"], raster_settings=rs, K=8)
    assert torch.equal(nocol.ids, want.ids) and torch.equal(nocol.weights, want.weights) and torch.equal(nocol.count, want.count)
    assert float(nocol.color.min()) >= 0.0 and bool((nocol.color.reshape(3, -1).max(dim=1).values <= rs.bg + 1e-6).all())      # zero colours: background x T
    # antialiasing is the render's: the weights carry the compensated opacity
    aa = _query(rast, gpu, sc, cam, 8, "weight", aa=True)
    assert not torch.equal(aa.weights, want.weights)
