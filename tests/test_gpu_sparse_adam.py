"""Sparse Adam on the device (-m gpu): GaussianAdam.step(visibility=...) against tests/sparse_adam_math.py (numpy fp64) and against the
dense step.

Sizes: 1 / 63 / 64 / 65 straddle one wave's run of 64 rows, 1000 has a ragged last run and several workgroups (256 rows each), 4099 many.
Groups and rates are tests/test_adam.py's: width 45 (f_rest) puts row boundaries inside a float4 and across the 64-row runs, the widths
1, 3 and 4 have many rows per 128-byte line.  Visible rows are held to test_adam.py's bars (displacement rtol 2e-4, atol 1.5e-6; moments
rtol 1e-5, atol 1e-6 * max); invisible rows are compared bit for bit (torch.equal on int32 views) after EVERY step."""
import numpy as np
import pytest
import torch

import sparse_adam_math as sam
from test_adam import LRS, SHAPES, _data

pytestmark = pytest.mark.gpu

PER_ROW = ("xyz", "opacity", "scaling", "rotation", "f_dc", "temporal_pos")      # the groups test_adam.py gives a per-row rate
PATTERNS = ("random22", "alternating", "row0", "last_row", "run100_300", "all_true", "all_false")
STEPS = 5


def _mask(pattern, P, t, seed=17):
    m = np.zeros(P, bool)
    if pattern == "random22":
        m = np.random.default_rng(seed + t).random(P) < 0.22
    elif pattern == "alternating":
        m[t % 2::2] = True
    elif pattern == "row0":
        m[0] = True
    elif pattern == "last_row":
        m[P - 1] = True
    elif pattern == "run100_300":
        m[100:301] = True
    elif pattern == "all_true":
        m[:] = True
    return m


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _inv(P):
    return (1.0 + 4.0 * np.random.default_rng(3).random(P)).astype(np.float32)


def _offset_leaf(a, gpu):
    """A contiguous leaf whose storage starts 4 bytes behind a 16-byte boundary: a flat buffer sliced from element 1."""
    flat = torch.zeros(a.size + 8, dtype=torch.float32, device=gpu)
    v = flat[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


def _optimizer(params, gpu, inv=None, offset=()):
    import fused_adam
    gp = {k: (_offset_leaf(v, gpu) if k in offset else torch.from_numpy(v.copy()).to(gpu)).requires_grad_(True) for k, v in params.items()}
    opt = fused_adam.GaussianAdam([{"params": [gp[k]], "lr": LRS[k], "name": k} for k in SHAPES], eps=1e-15)
    if inv is not None:
        P = inv.shape[0]
        for grp in opt.param_groups:
            if grp["name"] in PER_ROW:
                grp["lr"] = LRS[grp["name"]] * torch.from_numpy(inv).to(gpu).reshape(P, 1)
    return gp, opt


def _state(opt, gp):
    """{group: (p, exp_avg, exp_avg_sq)} as clones (zeros before the first step)."""
    out = {}
    for k, p in gp.items():
        st = opt.state.get(p)
        out[k] = (p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p), st["exp_avg_sq"].clone() if st else torch.zeros_like(p))
    return out


def _assert_rows_bit_equal(a, b, rows, what):
    rows = torch.as_tensor(rows, device=a[next(iter(a))][0].device)
    for k in a:
        for x, y, name in zip(a[k], b[k], ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(_bits(x)[rows], _bits(y)[rows]), (what, k, name)


def _assert_within_bars(opt, gp, params, ref):
    for k in SHAPES:
        got = gp[k].detach().cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(got - params[k], ref[k][0] - params[k], rtol=2e-4, atol=1.5e-6, err_msg=k)
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg"].cpu().numpy(), ref[k][1], rtol=1e-5, atol=1e-6 * np.abs(ref[k][1]).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg_sq"].cpu().numpy(), ref[k][2], rtol=1e-5, atol=1e-6 * np.abs(ref[k][2]).max(), err_msg=k)


def _run_against_math(P, pattern, gpu, offset=(), grad_offset=False):
    params, grads = _data(P, 2, STEPS)
    inv = _inv(P)
    gp, opt = _optimizer(params, gpu, inv, offset)
    ref = {k: (params[k].astype(np.float64), np.zeros(params[k].shape), np.zeros(params[k].shape)) for k in SHAPES}
    for t in range(STEPS):
        vis = _mask(pattern, P, t)
        for k in SHAPES:
            gp[k].grad = _offset_leaf(grads[t][k], gpu) if grad_offset and k in offset else torch.from_numpy(grads[t][k]).to(gpu)
            lr = LRS[k] * inv.astype(np.float64) if k in PER_ROW else LRS[k]
            ref[k] = sam.step(ref[k][0], grads[t][k], ref[k][1], ref[k][2], lr, t + 1, vis)
        before = _state(opt, gp)
        opt.step(visibility=torch.from_numpy(vis).to(gpu))
        _assert_rows_bit_equal(_state(opt, gp), before, ~vis, f"invisible rows, step {t + 1}")
    assert opt._step == STEPS
    _assert_within_bars(opt, gp, params, ref)


@pytest.mark.parametrize("P,pattern", [(P, pattern) for P in (1, 63, 64, 65, 1000, 4099) for pattern in PATTERNS
                                       if pattern != "run100_300" or P >= 1000])      # (rows 100-300 exist from P = 1000 on)
def test_masked_step_against_the_math(P, pattern, gpu):
    _run_against_math(P, pattern, gpu)


@pytest.mark.parametrize("pattern", ["random22", "alternating", "all_true"])
@pytest.mark.parametrize("grad_offset", [False, True])
def test_unaligned_group(pattern, grad_offset, gpu):
    """f_rest (width 45) -- and, second case, its gradient too -- 4 bytes off a 16-byte boundary: no float4 may be used; P = 65 keeps a second,
    one-row run behind the first."""
    _run_against_math(65, pattern, gpu, offset=("f_rest", "rotation"), grad_offset=grad_offset)


def _poisoned(a, vis, gpu):
    """a [P, ...] float32 with the invisible rows NaN and +Inf alternately."""
    a = a.copy()
    bad = np.nonzero(~vis)[0]
    a[bad[0::2]], a[bad[1::2]] = np.nan, np.inf
    return torch.from_numpy(a).to(gpu)


def test_poisoned_invisible_rows_reach_nothing(gpu):
    P = 1000
    params, grads = _data(P, 2, STEPS)
    inv = _inv(P)
    runs = {}
    for poison in (False, True):
        gp, opt = _optimizer(params, gpu, inv)
        for t in range(STEPS):
            vis = _mask("random22", P, t)
            for grp in opt.param_groups:
                k = grp["name"]
                gp[k].grad = _poisoned(grads[t][k], vis, gpu) if poison else torch.from_numpy(grads[t][k]).to(gpu)
                if k in PER_ROW:
                    rates = LRS[k] * inv.reshape(P, 1)
                    grp["lr"] = _poisoned(rates, vis, gpu) if poison else torch.from_numpy(rates).to(gpu)
            if poison:
                assert not torch.isfinite(gp["f_rest"].grad[torch.from_numpy(~vis).to(gpu)]).any()
            before = _state(opt, gp)
            opt.step(visibility=torch.from_numpy(vis).to(gpu))
            _assert_rows_bit_equal(_state(opt, gp), before, ~vis, f"invisible rows, step {t + 1}, poison {poison}")
        runs[poison] = _state(opt, gp)
    for k, triple in runs[True].items():
        for x in triple:
            assert bool(torch.isfinite(x).all()), k
    _assert_rows_bit_equal(runs[True], runs[False], np.ones(P, bool), "poisoned run against the clean one")


@pytest.mark.parametrize("dtype", [torch.bool, torch.int32])
def test_all_true_mask_is_the_dense_step(dtype, gpu):
    P, steps = 4099, 6
    params, grads = _data(P, 4, steps)
    inv = _inv(P)
    (ga, a), (gb, b) = _optimizer(params, gpu, inv), _optimizer(params, gpu, inv)
    ones = torch.ones(P, dtype=dtype, device=gpu)
    for t in range(steps):
        for k in SHAPES:
            g = torch.from_numpy(grads[t][k]).to(gpu)
            ga[k].grad, gb[k].grad = g.clone(), g.clone()
        a.step()
        b.step(visibility=ones)
    assert a._step == b._step == steps
    _assert_rows_bit_equal(_state(a, ga), _state(b, gb), np.ones(P, bool), "dense against all-true")


def test_mask_dtypes_and_shapes_agree(gpu):
    P, steps = 1000, 3
    params, grads = _data(P, 6, steps)
    inv = _inv(P)

    def forms(vis):
        i = np.arange(P)
        u8 = np.where(vis, np.where(i % 2 == 0, 1, 255), 0).astype(np.uint8)
        i32 = np.where(vis, np.where(i % 2 == 0, 1, 37), np.where(i % 2 == 0, -1, 0)).astype(np.int32)
        assert {0, 1, 255} == set(u8.tolist()) and {-1, 0, 1, 37} == set(i32.tolist())
        return {"bool": torch.from_numpy(vis), "uint8": torch.from_numpy(u8), "int32": torch.from_numpy(i32),
                "bool_P1": torch.from_numpy(vis).reshape(P, 1), "int32_P1": torch.from_numpy(i32).reshape(P, 1)}

    results = {}
    for form in forms(_mask("random22", P, 0)):
        gp, opt = _optimizer(params, gpu, inv)
        for t in range(steps):
            for k in SHAPES:
                gp[k].grad = torch.from_numpy(grads[t][k]).to(gpu)
            opt.step(visibility=forms(_mask("random22", P, t))[form].to(gpu))
        results[form] = _state(opt, gp)
    for form, st in results.items():
        _assert_rows_bit_equal(st, results["bool"], np.ones(P, bool), form)
    moved = (results["bool"]["xyz"][0] != torch.from_numpy(params["xyz"]).to(gpu)).any(dim=1).cpu().numpy()
    seen = np.any([_mask("random22", P, t) for t in range(steps)], axis=0)
    assert np.array_equal(moved, seen)


def test_mask_on_another_device_or_of_another_length_is_refused(gpu):
    params, grads = _data(10, 1, 1)
    gp, opt = _optimizer(params, gpu)
    for k in SHAPES:
        gp[k].grad = torch.from_numpy(grads[0][k]).to(gpu)
    before = _state(opt, gp)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        opt.step(visibility=torch.ones(10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="rows, the visibility mask"):
        opt.step(visibility=torch.ones(11, dtype=torch.bool, device=gpu))
    with pytest.raises(RuntimeError, match="torch.bool, torch.uint8 or torch.int32"):
        opt.step(visibility=torch.ones(10, device=gpu))
    assert opt._step == 0
    _assert_rows_bit_equal(_state(opt, gp), before, np.ones(10, bool), "a refused step")


def test_render_radii_as_the_mask(gpu, rast, scenes):
    """End to end on the smallest edge scene (tests/edge_scenes.py, case f: 3 of its 332 Gaussians lie behind the first camera's near
    plane): render -> backward -> two optimizers on identical copies.  Step 1: step() and step(visibility=radii) agree bit for bit --
    with zero moments a zero gradient moves nothing.  Step 2 from a second camera: the rows it no longer sees keep their step-1 moments
    under the masked step, while the dense step decays them."""
    import edge_scenes
    import fused_adam
    from conftest import settings_from
    c = min(edge_scenes.CASES, key=lambda c: c["P"])
    sc, cam = edge_scenes.edge_scene(scenes, c)
    cams = [cam, scenes.camera((c["k"] + 1) % c["V"], c["V"], c["W"], c["H"])]
    for cm in cams:
        cm["image_height"], cm["image_width"] = c["H"], c["W"]
    P = sc["means3D"].shape[0]
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    A = {k: t(sc[k]).requires_grad_(True) for k in names}
    B = {k: t(sc[k]).requires_grad_(True) for k in names}
    opt_a, opt_b = (fused_adam.GaussianAdam([{"params": [L[k]], "lr": 1e-4, "name": k} for k in names], eps=1e-15) for L in (A, B))
    upstream = t(scenes.upstream_grad(c["H"], c["W"], 8))

    def render_backward(cm):
        opt_a.zero_grad(); opt_b.zero_grad()
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii, _ = rast.GaussianRasterizer(settings_from(rast, cm, sc, gpu))(
            means3D=A["means3D"], means2D=means2D, opacities=A["opacities"], shs=A["shs"], scales=A["scales"], rotations=A["rotations"])
        color.backward(upstream)
        for k in names:
            B[k].grad = A[k].grad.clone()
        return radii

    radii1 = render_backward(cams[0])
    assert radii1.dtype == torch.int32 and bool((radii1 == 0).any()) and bool((radii1 > 0).any())
    opt_a.step()
    opt_b.step(visibility=radii1)
    s1a, s1b = _state(opt_a, A), _state(opt_b, B)
    _assert_rows_bit_equal(s1a, s1b, np.ones(P, bool), "step 1: dense against radii-masked")

    radii2 = render_backward(cams[1])
    lost = ((radii1 > 0) & (radii2 <= 0)).cpu().numpy()
    assert lost.any() and (radii2 > 0).any()
    opt_a.step()
    opt_b.step(visibility=radii2)
    s2a, s2b = _state(opt_a, A), _state(opt_b, B)
    _assert_rows_bit_equal(s2b, s1b, (radii2 <= 0).cpu().numpy(), "step 2: rows the second view does not see")
    lost_t = torch.from_numpy(lost).to(gpu)
    differs = [k for k in names if s1b[k][1][lost_t].any() and not torch.equal(s2a[k][1][lost_t], s2b[k][1][lost_t])]
    assert "means3D" in differs and "shs" in differs, differs
    for k in names:      # wherever the lost rows carried a moment, the dense step decayed it and the masked one did not
        if s1b[k][1][lost_t].any():
            assert k in differs, k


def test_masked_step_after_densification(gpu):
    """fused_densify.densify_and_prune on a GaussianAdam with non-zero moments (P = 300), then one masked step at the new P against
    sparse_adam_math on the gathered moments (tests/densify_math.py's closed form): the moments travelled with their rows."""
    import densify_math as dm
    from test_gpu_densify import _check_against_truth
    d = dm.draw(300, 16, "mixed", seed=8)
    opt, counts, ref, _ = _check_against_truth(d, 2, gpu)
    Pn = counts["P"]
    assert Pn != 300 and opt._step == 3
    rng = np.random.default_rng(0)
    lr_rows = (1.0 + 4.0 * rng.random(Pn)).astype(np.float32)
    vis = rng.random(Pn) < 0.22
    before_np, grads, gp = {}, {}, {}
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        gp[k] = p
        before_np[k] = p.detach().cpu().numpy().copy()
        grads[k] = (rng.normal(size=tuple(p.shape)) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32)
        p.grad = torch.from_numpy(grads[k]).to(gpu)
        g["lr"] = 1e-3 * torch.from_numpy(lr_rows).to(gpu).reshape(Pn, 1) if k in ("xyz", "opacity") else 1e-3
    before = _state(opt, gp)
    opt.step(visibility=torch.from_numpy(vis).to(gpu))
    assert opt._step == 4
    _assert_rows_bit_equal(_state(opt, gp), before, ~vis, "invisible rows after densification")
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        lr = 1e-3 * lr_rows.astype(np.float64) if k in ("xyz", "opacity") else 1e-3
        rp, rm, rv = sam.step(before_np[k], grads[k], ref[k][1].numpy(), ref[k][2].numpy(), lr, 4, vis)
        np.testing.assert_allclose(p.detach().cpu().numpy().astype(np.float64) - before_np[k], rp - before_np[k], rtol=2e-4, atol=1.5e-6, err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), rm, rtol=1e-5, atol=1e-6 * np.abs(rm).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv, rtol=1e-5, atol=1e-6 * np.abs(rv).max(), err_msg=k)
