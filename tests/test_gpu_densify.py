"""Densification on the device (-m gpu): fused_densify against the CPU restatement of tests/densify_math.py (closed form, fp64).

Sizes: 255 / 256 / 257 straddle one 256-source workgroup, 4099 is ragged over 17 of them, 70001 gives 274 workgroup sums -- more than the
256 the single-workgroup scan takes per turn, so its carry is exercised.  M = 4 / 16: f_rest rows of 9 / 45 floats beside the widths
1, 3, 4.  Inputs keep every g, max exp(scaling) and sigmoid(opacity) at least 3 % clear of its threshold by construction
(densify_math.draw; asserted with the 1e-3 margin), so no case is redrawn or left out.
Copied rows, gathered moments and counts are compared exactly; the computed rows (split xyz / scaling) at the project's bar made
scale-free as conftest.grad_tol does: ATOL * max|ref| + RTOL * |ref|."""
import math

import numpy as np
import pytest
import torch

import densify_math as dm
from conftest import ATOL, RTOL

pytestmark = pytest.mark.gpu


def _gpu_optimizer(d, gpu, step=3):
    import fused_adam
    leaves = {k: torch.nn.Parameter(v.clone().to(gpu)) for k, v in d["params"].items()}
    opt = fused_adam.GaussianAdam([{"params": [leaves[k]], "lr": 1e-3, "name": k} for k in dm.GROUPS], eps=1e-15)
    if d["moments"] is not None:
        for k, p in leaves.items():
            opt.state[p] = {"exp_avg": d["moments"][k][0].clone().to(gpu), "exp_avg_sq": d["moments"][k][1].clone().to(gpu)}
    opt._step = step
    return opt


def _gpu_stats(d, gpu):
    import fused_densify
    P = d["accum"].shape[0]
    st = fused_densify.DensifyStats(P, gpu)
    st.xyz_gradient_accum, st.denom = d["accum"].clone().to(gpu), d["denom"].clone().to(gpu)
    st.max_radii2D = torch.arange(P, dtype=torch.float32, device=gpu)
    return st


def _truth(d, N, noise):
    f64 = lambda t: None if t is None else t.double()  # noqa: E731
    params = {k: v.double() for k, v in d["params"].items()}
    moments = None if d["moments"] is None else {k: (a.double(), b.double()) for k, (a, b) in d["moments"].items()}
    return dm.closed_form(params, moments, f64(d["accum"]), f64(d["denom"]), noise.double(), N=N, prune_mask=d["prune_mask"],
                          grad_scale=f64(d["grad_scale"]), **d["kw"])


def _noise_for(d, N, seed=11):
    _, split_all, _ = dm.classify(d["params"], d["accum"], d["denom"], prune_mask=d["prune_mask"], grad_scale=d["grad_scale"], **d["kw"])
    return torch.randn(N * int(split_all.sum()), 3, generator=torch.Generator().manual_seed(seed))


def _densify(d, N, noise, gpu):
    import fused_densify
    opt, stats = _gpu_optimizer(d, gpu), _gpu_stats(d, gpu)
    counts, new = fused_densify.densify_and_prune(
        opt, stats, grad_threshold=d["kw"]["thr"], percent_dense=d["kw"]["tau"] / 4.0, extent=4.0, min_opacity=d["kw"]["min_opacity"],
        prune_mask=d["prune_mask"].to(gpu), grad_scale=None if d["grad_scale"] is None else d["grad_scale"].to(gpu), n_split=N, noise=noise.to(gpu))
    return opt, stats, counts, new


def _check_against_truth(d, N, gpu):
    assert dm.margins_ok(d, 1e-3)
    noise = _noise_for(d, N)
    ref_counts, ref, parts = _truth(d, N, noise)
    opt, stats, counts, new = _densify(d, N, noise, gpu)
    assert counts == ref_counts, (counts, ref_counts)
    n_kept, n_copied, Pn = counts["n_kept"], counts["n_kept"] + counts["n_clone"], counts["P"]
    assert opt._step == 3 and stats.P == Pn
    assert not stats.xyz_gradient_accum.any() and not stats.denom.any() and not stats.max_radii2D.any()
    assert stats.xyz_gradient_accum.shape == (Pn, 1) and stats.denom.shape == (Pn, 1) and stats.max_radii2D.shape == (Pn,)
    assert set(opt.state.keys()) == {g["params"][0] for g in opt.param_groups}
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        assert p is new[k] and isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad and p.grad is None
        assert tuple(p.shape) == (Pn,) + dm.shapes(d["params"]["f_rest"].shape[1] + 1)[k]
        got, (rp, rm, rv) = p.detach().cpu().double(), ref[k]
        assert torch.equal(got[:n_copied], rp[:n_copied]), k                 # kept originals and clones: bit copies, every role
        if k in ("xyz", "scaling"):
            tol = ATOL * float(rp.abs().max()) + RTOL * rp[n_copied:].abs() if Pn else 0
            err = (got[n_copied:] - rp[n_copied:]).abs()
            assert bool((err <= tol).all()), (k, float(err.max()))
        else:
            assert torch.equal(got[n_copied:], rp[n_copied:]), k
        st = opt.state[p]
        assert torch.equal(st["exp_avg"][:n_kept].cpu().double(), rm[:n_kept]) and torch.equal(st["exp_avg_sq"][:n_kept].cpu().double(), rv[:n_kept]), k
        assert st["exp_avg"].shape == p.shape and not st["exp_avg"][n_kept:].any() and not st["exp_avg_sq"][n_kept:].any(), k
    return opt, counts, ref, noise


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 4099, 70001])
def test_sizes_and_widths(P, M, N, gpu):
    _check_against_truth(dm.draw(P, M, "overlap" if P > 1 else "all_split", seed=P + M + N), N, gpu)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("P", [257, 4099])
@pytest.mark.parametrize("mix", dm.MIXES)
def test_class_mixes(mix, P, N, gpu):
    _check_against_truth(dm.draw(P, 4, mix, seed=31 + P + N), N, gpu)


def test_single_gaussian_of_every_class(gpu):
    for mix in ("none", "all_clone", "all_split", "all_pruned"):
        _check_against_truth(dm.draw(1, 4, mix, seed=3), 2, gpu)


def test_two_runs_are_bit_identical(gpu):
    d = dm.draw(70001, 16, "mixed", seed=9)
    noise = _noise_for(d, 2)
    a, _, ca, _ = _densify(d, 2, noise, gpu)
    b, _, cb, _ = _densify(d, 2, noise, gpu)
    assert ca == cb and ca["n_split"] > 0 and ca["n_clone"] > 0
    for ga, gb in zip(a.param_groups, b.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), ga["name"]
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.state[pa][key].view(torch.int32), b.state[pb][key].view(torch.int32)), (ga["name"], key)


def test_noise_is_drawn_like_randn_on_the_device(gpu):
    """Without `noise`, N * n_split_all rows come from torch.randn with the caller's generator: same seed, same result, and the same as
    handing that draw in."""
    import fused_densify
    d = dm.draw(4099, 4, "overlap", seed=2)
    kw = dict(grad_threshold=dm.THR, percent_dense=dm.TAU, extent=1.0, min_opacity=dm.MIN_OPACITY, n_split=2)
    outs = []
    for given in (False, True):
        opt, stats = _gpu_optimizer(d, gpu), _gpu_stats(d, gpu)
        gen = torch.Generator(device=gpu).manual_seed(5)
        n_all = int(dm.classify(d["params"], d["accum"], d["denom"], **d["kw"])[1].sum())
        extra = dict(noise=torch.randn((2 * n_all, 3), generator=gen, device=gpu)) if given else dict(generator=gen)
        counts, new = fused_densify.densify_and_prune(opt, stats, **kw, **extra)
        assert counts["n_split_all"] == n_all > counts["n_split"] > 0
        outs.append(new["xyz"].detach().clone())
    assert torch.equal(outs[0], outs[1])


def test_no_moments_and_empty_model(gpu):
    import fused_densify
    d = dm.draw(300, 4, "mixed", seed=4, with_moments=False)
    opt, counts, ref, _ = _check_no_state(d, gpu)
    assert not opt.state
    d0 = dm.draw(0, 4, "mixed", seed=4)
    opt, stats = _gpu_optimizer(d0, gpu), _gpu_stats(d0, gpu)
    counts, new = fused_densify.densify_and_prune(opt, stats, grad_threshold=dm.THR, percent_dense=dm.TAU, extent=1.0, min_opacity=dm.MIN_OPACITY)
    assert counts == dict(n_kept=0, n_clone=0, n_split=0, n_split_all=0, P=0) and all(v.shape[0] == 0 and v.is_leaf for v in new.values())


def _check_no_state(d, gpu):
    noise = _noise_for(d, 2)
    ref_counts, ref, _ = _truth(d, 2, noise)
    opt, stats, counts, new = _densify(d, 2, noise, gpu)
    assert counts == ref_counts
    n_copied = counts["n_kept"] + counts["n_clone"]
    for k in dm.GROUPS:
        assert torch.equal(new[k].detach().cpu().double()[:n_copied], ref[k][0][:n_copied]) and new[k].shape[0] == counts["P"]
    return opt, counts, ref, noise


@pytest.mark.parametrize("P", [257, 70001])
def test_prune_gathers_everything(P, gpu):
    import fused_densify
    d = dm.draw(P, 16, "mixed", seed=6)
    opt, stats = _gpu_optimizer(d, gpu), _gpu_stats(d, gpu)
    before = (stats.xyz_gradient_accum.clone(), stats.denom.clone(), stats.max_radii2D.clone())
    gen = torch.Generator().manual_seed(1)
    extras = [torch.randn(P, 1, generator=gen).to(gpu), torch.randn(P, 2, 5, generator=gen).to(gpu)]      # t_gradient_accum, and something wider
    mask = d["prune_mask"] | (torch.rand(P, generator=gen) < 0.3)
    keep = (~mask).to(gpu)
    old = {g["name"]: (g["params"][0].detach().clone(), opt.state[g["params"][0]]["exp_avg"].clone(), opt.state[g["params"][0]]["exp_avg_sq"].clone())
           for g in opt.param_groups}
    counts, new, rest = fused_densify.prune(opt, mask.to(gpu), stats=stats, extras=extras)
    n = int(keep.sum())
    assert counts == dict(n_kept=n, n_clone=0, n_split=0, n_split_all=0, P=n) and 0 < n < P
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        assert p is new[k] and p.is_leaf and torch.equal(p.detach(), old[k][0][keep])
        assert torch.equal(opt.state[p]["exp_avg"], old[k][1][keep]) and torch.equal(opt.state[p]["exp_avg_sq"], old[k][2][keep])
    for got, was in zip((stats.xyz_gradient_accum, stats.denom, stats.max_radii2D), before):
        assert got.shape == was[keep].shape and torch.equal(got, was[keep])
    assert len(rest) == 2 and all(torch.equal(r, e[keep]) for r, e in zip(rest, extras))
    assert opt._step == 3 and set(opt.state.keys()) == {g["params"][0] for g in opt.param_groups}


@pytest.mark.parametrize("P", [257, 4099])
def test_stats_update_equals_the_torch_expression(P, gpu):
    import fused_densify
    gen = torch.Generator().manual_seed(P)
    count = torch.floor(4 * torch.rand(P, generator=gen) - 0.5).clamp(min=0)          # about a third never visible
    gsum = torch.rand(P, generator=gen) * 1e-3
    radii = torch.floor(40 * torch.rand(P, generator=gen))
    vis = count > 0
    mean = gsum.clone()
    mean[vis] = mean[vis] / count[vis]                                                 # train.py:286-287
    accum0, denom0, rad0 = torch.rand(P, 1, generator=gen), torch.floor(5 * torch.rand(P, 1, generator=gen)), torch.floor(40 * torch.rand(P, generator=gen))
    want_a, want_d, want_r = accum0.clone(), denom0.clone(), rad0.clone()
    want_r[vis] = torch.max(want_r[vis], radii[vis])                                   # train.py:291
    want_a[vis] += mean.unsqueeze(1)[vis]                                              # add_densification_stats_grad
    want_d[vis] += 1
    for form in ("mean", "sum"):
        st = fused_densify.DensifyStats(P, gpu)
        st.xyz_gradient_accum, st.denom, st.max_radii2D = accum0.clone().to(gpu), denom0.clone().to(gpu), rad0.clone().to(gpu)
        out = {"visibility_count": count.to(gpu), "visibility_filter": vis.to(gpu), "radii": radii.to(gpu)}
        out["viewspace_point_grad" if form == "mean" else "viewspace_point_grad_sum"] = (mean if form == "mean" else gsum).unsqueeze(1).to(gpu)
        st.update(out)
        assert torch.equal(st.xyz_gradient_accum.cpu(), want_a) and torch.equal(st.denom.cpu(), want_d) and torch.equal(st.max_radii2D.cpu(), want_r), form
    assert int(vis.sum()) not in (0, P)


def test_adam_step_after_densification(gpu):
    """One GaussianAdam.step() on the densified model against oracle/adam_oracle.step on the restated state (tests/test_adam.py's
    tolerances): the moments arrived where the parameters did, new rows start from zero moments, the step count went on."""
    from oracle import adam_oracle
    d = dm.draw(4099, 16, "mixed", seed=8)
    opt, counts, ref, _ = _check_against_truth(d, 2, gpu)
    Pn = counts["P"]
    rng = np.random.default_rng(0)
    lr_rows = (1.0 + 4.0 * rng.random(Pn)).astype(np.float32)
    before = {}
    for g in opt.param_groups:
        p = g["params"][0]
        before[g["name"]] = p.detach().cpu().numpy().copy()
        p.grad = torch.from_numpy((rng.normal(size=tuple(p.shape)) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32)).to(gpu)
        g["lr"] = 1e-3 * torch.from_numpy(lr_rows).to(gpu).reshape(Pn, 1) if g["name"] in ("xyz", "opacity") else 1e-3
    grads = {g["name"]: g["params"][0].grad.cpu().numpy() for g in opt.param_groups}
    opt.step()
    assert opt._step == 4
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        lr = 1e-3 * lr_rows.astype(np.float64) if k in ("xyz", "opacity") else 1e-3
        rp, rm, rv = adam_oracle.step(before[k], grads[k], ref[k][1].numpy(), ref[k][2].numpy(), lr, 4)
        np.testing.assert_allclose(p.detach().cpu().numpy().astype(np.float64) - before[k], rp - before[k], rtol=2e-4, atol=1.5e-6, err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), rm, rtol=1e-5, atol=1e-6 * np.abs(rm).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv, rtol=1e-5, atol=1e-6 * np.abs(rv).max(), err_msg=k)


def test_stale_per_row_lr_is_refused_after_densification(gpu):
    d = dm.draw(257, 4, "mixed", seed=12)
    noise = _noise_for(d, 2)
    opt, _, counts, new = _densify(d, 2, noise, gpu)
    assert counts["P"] != 257
    for g in opt.param_groups:
        g["params"][0].grad = torch.zeros_like(g["params"][0])
    opt.param_groups[0]["lr"] = torch.ones(257, 1, device=gpu)
    with pytest.raises(RuntimeError, match="per-row lr"):
        opt.step()
