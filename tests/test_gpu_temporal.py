"""-m gpu: the temporal lifespan (csrc/gsrast_temporal.h, fused_temporal.py) against the fp64 restatement of tests/temporal_math.py.

The bar, per output and gradient tensor T, measured per case at run time (tests/test_gpu_mlp.py's idiom, in absolute form):
    max|T_hip - T_fp64| <= 4 max|T_torch32 - T_fp64| + 2^-23 max|T_fp64|,
T_torch32 = torch's fp32 CPU execution of the same ops on the same inputs (temporal_math.torch_gate / torch_integral).  The factor 4 covers
the other order of the few roundings per row and another libm (exp, sin, cos within an ulp or two of torch's); the second term is one ulp
of fp32 at the tensor's largest entry.  Masks are compared exactly, after the rows whose fp64 value lies in a narrow band around the
threshold have been moved out of it (at most 0.1 % of the rows, asserted)."""
import numpy as np
import pytest
import torch
from torch import nn

import temporal_math as tm

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 4099]
MULTIRES = [0, 1, 4, 8]
MIN_SCALES = [1 / 300, 0.01, 1.0]
TIMES = [0.0, 0.37, 1.0]
ULP = 2.0 ** -23
GATE_KEYS = ("lifespan", "state", "time_emb", "d_head", "d_center")


def bar_check(label, got, f64, t32, worst):
    """The bar of this file's docstring on every tensor of `got`; the worst ratio per tensor is kept in `worst` for the summary line."""
    bad = []
    for k, g in got.items():
        truth = np.asarray(f64[k], np.float64)
        g = np.asarray(g, np.float64).reshape(truth.shape)
        if truth.size == 0:
            continue
        finite = np.isfinite(truth)
        assert np.array_equal(np.isfinite(g), finite), (label, k)
        e_hip = float(np.abs(g - truth)[finite].max(initial=0.0))
        e_ref = float(np.abs(np.asarray(t32[k], np.float64).reshape(truth.shape) - truth)[finite].max(initial=0.0))
        bound = 4 * e_ref + ULP * float(np.abs(truth[finite]).max(initial=0.0))
        if bound > 0 and e_hip / bound > worst.get(k, (0.0,))[0]:
            worst[k] = (e_hip / bound, e_hip, e_ref, label)
        if not e_hip <= bound:
            bad.append((k, e_hip, e_ref, bound))
    assert not bad, (label, bad)


def torch32_gate(c, t, ms, sig):
    """torch's fp32 CPU run of the gate with multires 8 (the narrower embeddings are its leading columns) and both gradients."""
    head = torch.from_numpy(c["head"]).reshape(-1, 1).requires_grad_(True)
    center = torch.from_numpy(c["center"]).reshape(-1, 1).requires_grad_(True)
    lifespan, state, emb = tm.torch_gate(head, center, t, ms, 8, sig)
    torch.autograd.backward((lifespan, state), (torch.from_numpy(c["d_lifespan"]).reshape(-1, 1), torch.from_numpy(c["d_state"]).reshape(-1, 1)))
    return dict(lifespan=lifespan.detach().numpy(), state=state.detach().numpy(), time_emb=emb.numpy(), d_head=head.grad.numpy(), d_center=center.grad.numpy())


def fused_gate(c, t, ms, multires, sig, gpu, upstream=("d_lifespan", "d_state")):
    import fused_temporal as ft
    head = torch.tensor(c["head"], device=gpu).reshape(-1, 1).requires_grad_(True)
    center = torch.tensor(c["center"], device=gpu).reshape(-1, 1).requires_grad_(True)
    lifespan, state, emb = ft.temporal_gate(head, center, t, min_scale=ms, multires=multires, sigmoid_tcenter=sig)
    assert emb.requires_grad is False and tuple(emb.shape) == (len(c["head"]), 2 * multires + 1) and lifespan.shape == state.shape == head.shape
    outs = [o for o, k in ((lifespan, "d_lifespan"), (state, "d_state")) if k in upstream]
    torch.autograd.backward(outs, [torch.tensor(c[k], device=gpu).reshape(-1, 1) for k in upstream])
    torch.cuda.synchronize()
    return dict(lifespan=lifespan.detach().cpu().numpy(), state=state.detach().cpu().numpy(), time_emb=emb.cpu().numpy(),
                d_head=head.grad.cpu().numpy(), d_center=center.grad.cpu().numpy())


@pytest.mark.parametrize("P", ROWS)
def test_gate_forward_and_backward_against_fp64(P, gpu):
    worst = {}
    for t in TIMES:
        c, rows = tm.make_case(P, t, seed=100 + P)
        for sig in (False, True):
            for ms in MIN_SCALES:
                f64_8 = tm.gate(c["head"], c["center"], t, ms, 8, sig, c["d_lifespan"], c["d_state"])
                t32_8 = torch32_gate(c, t, ms, sig)
                for m in MULTIRES:
                    label = f"P={P} t={t} sig={int(sig)} ms={ms:.4g} multires={m}"
                    cut = lambda d: {k: (d[k][:, :2 * m + 1] if k == "time_emb" else d[k]) for k in GATE_KEYS}  # noqa: E731
                    got = fused_gate(c, t, ms, m, sig, gpu)
                    bar_check(label, got, cut(f64_8), cut(t32_8), worst)
                    if not sig and "center_t" in rows:      # center = t: distance 0 exactly
                        i = rows["center_t"]
                        assert got["state"][i, 0] == 1.0 and np.array_equal(got["time_emb"][i], np.array([0.0] + [0.0, 1.0] * m, np.float32)), label
                    if not sig and "center_40" in rows:
                        assert got["state"][rows["center_40"], 0] == 0.0, label
                # underflowed rows: gradient exactly 0 (only the state is used: the lifespan output counts as zero upstream)
                only_state = fused_gate(c, t, ms, 4, sig, gpu, upstream=("d_state",))
                under = only_state["state"].reshape(-1) == 0.0
                assert not only_state["d_head"].reshape(-1)[under].any() and not only_state["d_center"].reshape(-1)[under].any()
                assert np.isfinite(only_state["d_head"]).all() and np.isfinite(only_state["d_center"]).all()
    for k, (ratio, e_hip, e_ref, label) in worst.items():
        print(f"P={P} {k}: worst e_hip / bar {ratio:.3f} (e_hip {e_hip:.3e}, e_torch32 {e_ref:.3e}) at {label}")


def test_gate_nan_row_stays_in_its_row_and_is_dead(gpu):
    import fused_temporal as ft
    c, _ = tm.make_case(300, 0.37, seed=9)
    head, center = torch.tensor(c["head"], device=gpu).reshape(-1, 1), torch.tensor(c["center"], device=gpu).reshape(-1, 1)
    clean = ft.temporal_gate(head, center, 0.37, min_scale=0.01)
    h2, c2 = head.clone(), center.clone()
    h2[70], c2[131] = float("nan"), float("nan")
    h2.requires_grad_(True), c2.requires_grad_(True)
    got = ft.temporal_gate(h2, c2, 0.37, min_scale=0.01)
    torch.autograd.backward(got[:2], (torch.ones_like(head), torch.ones_like(head)))
    keep = torch.ones(300, dtype=torch.bool, device=gpu)
    keep[70] = keep[131] = False
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep])
    assert torch.isnan(got[0][70]).all() and torch.isnan(got[1][70]).all() and torch.isfinite(got[2][70]).all()      # the head's NaN: not in the embedding
    assert torch.isfinite(got[0][131]).all() and torch.isnan(got[1][131]).all() and torch.isnan(got[2][131]).all()
    assert torch.isfinite(h2.grad[keep]).all() and torch.isfinite(c2.grad[keep]).all()
    n, state, emb, (idx,) = ft.temporal_select(h2.detach(), c2.detach(), 0.37, [torch.arange(300, dtype=torch.float32, device=gpu)], min_scale=0.01)
    alive = (clean[1].reshape(-1) > 0.001) & keep
    assert n == int(alive.sum()) and torch.equal(idx, torch.arange(300, dtype=torch.float32, device=gpu)[alive]) and torch.isfinite(state).all()


def test_gate_requires_grad_combinations_unused_outputs_and_no_grad(gpu):
    import fused_temporal as ft
    c, _ = tm.make_case(1000, 0.37, seed=10)
    full = fused_gate(c, 0.37, 0.01, 4, True, gpu)
    ds, dl = (torch.tensor(c[k], device=gpu).reshape(-1, 1) for k in ("d_state", "d_lifespan"))
    for need_head, need_pos in ((True, False), (False, True)):
        head = torch.tensor(c["head"], device=gpu).reshape(-1, 1).requires_grad_(need_head)
        pos = torch.tensor(c["center"], device=gpu).requires_grad_(need_pos)                     # [P]: the gradient takes the input's shape
        lifespan, state, _ = ft.temporal_gate(head, pos, 0.37, min_scale=0.01, sigmoid_tcenter=True)
        torch.autograd.backward((lifespan, state), (dl, ds))
        if need_head:
            assert pos.grad is None and np.array_equal(head.grad.cpu().numpy(), full["d_head"])
        else:
            assert head.grad is None and pos.grad.shape == pos.shape and np.array_equal(pos.grad.cpu().numpy(), full["d_center"].reshape(-1))
    # only the lifespan is used: d_head = -(1 - ms) d_lifespan, nothing reaches the centre
    head = torch.tensor(c["head"], device=gpu).reshape(-1, 1).requires_grad_(True)
    pos = torch.tensor(c["center"], device=gpu).reshape(-1, 1).requires_grad_(True)
    lifespan, state, emb = ft.temporal_gate(head, pos, 0.37, min_scale=0.01, with_embedding=False)
    assert emb is None
    lifespan.backward(dl)
    assert not pos.grad.any() and torch.equal(head.grad, -(1.0 - np.float32(0.01)) * dl)
    with torch.no_grad():
        out = ft.temporal_gate(head, pos, 0.37, min_scale=0.01)
    assert all(o.grad_fn is None and not o.requires_grad for o in out) and torch.equal(out[1], state)
    # the timestamp as a one-element tensor on the device
    assert torch.equal(ft.temporal_gate(head, pos, torch.tensor([0.37], device=gpu), min_scale=0.01)[1], state)


def test_gate_bit_identical_from_run_to_run(gpu):
    c, _ = tm.make_case(4099, 0.37, seed=11)
    a, b = fused_gate(c, 0.37, 1 / 300, 8, False, gpu), fused_gate(c, 0.37, 1 / 300, 8, False, gpu)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_gate_double_backward_and_cpu_tensors_raise(gpu):
    import fused_temporal as ft
    head, pos = torch.rand(33, 1, device=gpu, requires_grad=True), torch.rand(33, 1, device=gpu, requires_grad=True)
    _, state, _ = ft.temporal_gate(head, pos, 0.5, min_scale=0.1)
    ds = torch.ones_like(state).requires_grad_(True)
    (g,) = torch.autograd.grad(state, pos, ds, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g.sum().backward()
    for args in ((head.detach().cpu(), pos.detach()), (head.detach(), pos.detach().cpu())):
        with pytest.raises(RuntimeError, match="GPU|is on cpu"):
            ft.temporal_gate(*args, 0.5, min_scale=0.1)


# ---- select ---------------------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(3,), (4,), (3,), (1,), (1, 3), (15, 3), (32,), (2, 5)]      # xyz, rotation, scaling, opacity, f_dc, f_rest, the field's feature, one more


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "runs300", "random"])
@pytest.mark.parametrize("P", [1, 257, 4099])
def test_select_equals_mask_indexing_bit_for_bit(P, pattern, gpu):
    import fused_temporal as ft
    t, ms = 0.37, 0.01
    c, _ = tm.make_case(P, t, seed=20 + P)
    rng = np.random.default_rng(P)
    head, center = c["head"].copy(), c["center"].copy()
    if pattern != "random":
        i = np.arange(P)
        alive = dict(all=i >= 0, none=i < 0, alternating=i % 2 == 0, runs300=(i // 300) % 2 == 0)[pattern]
        L = (1 - ms) * (1 - head.astype(np.float64)) + ms
        center = np.where(alive, t + 0.3 * L * rng.uniform(-1, 1, P), t + 2.0).astype(np.float32)      # state >= 0.69, or <= e^-16
    band = np.abs(tm.gate(head, center, t, ms)["state"] - 0.001) <= 1e-6
    assert band.sum() <= 0.001 * P
    center[band] = t
    want = tm.gate(head, center, t, ms)
    h, p = torch.tensor(head, device=gpu).reshape(-1, 1), torch.tensor(center, device=gpu).reshape(-1, 1)
    gen = torch.Generator().manual_seed(P)
    tensors = [torch.randn((P,) + s, generator=gen).to(gpu) for s in SELECT_SHAPES]
    _, state, emb = ft.temporal_gate(h, p, t, min_scale=ms)
    mask = state.reshape(-1) > 0.001
    assert np.array_equal(mask.cpu().numpy(), ~want["dead"])                                    # the device's mask is the fp64 mask
    n, s_sel, e_sel, sel = ft.temporal_select(h, p, t, tensors, min_scale=ms)
    assert n == int(mask.sum()) == int((~want["dead"]).sum()) and len(sel) == len(tensors)
    if pattern in ("all", "none"):
        assert n == (P if pattern == "all" else 0)
    assert tuple(s_sel.shape) == (n, 1) and torch.equal(s_sel, state[mask]) and tuple(e_sel.shape) == (n, 9) and torch.equal(e_sel, emb[mask])
    for got, src in zip(sel, tensors):
        assert got.shape == src[mask].shape and torch.equal(got, src[mask])


def test_select_refuses_what_it_cannot_move(gpu):
    import fused_temporal as ft
    h, p = torch.rand(10, 1, device=gpu), torch.rand(10, 1, device=gpu)
    with pytest.raises(RuntimeError, match="at most 14"):
        ft.temporal_select(h, p, 0.5, [torch.zeros(10, 1, device=gpu)] * 15, min_scale=0.1)
    with pytest.raises(RuntimeError, match="floats per row"):
        ft.temporal_select(h, p, 0.5, [torch.zeros(10, 65, device=gpu)], min_scale=0.1)
    with pytest.raises(RuntimeError, match="rows"):
        ft.temporal_select(h, p, 0.5, [torch.zeros(9, 3, device=gpu)], min_scale=0.1)
    n, s, e, out = ft.temporal_select(h[:0], p[:0], 0.5, [torch.zeros(0, 3, device=gpu)], min_scale=0.1)
    assert n == 0 and s.shape == (0, 1) and e.shape == (0, 9) and out[0].shape == (0, 3)


# ---- integral -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ROWS)
def test_integral_mask_inv_and_stats(P, gpu):
    import fused_temporal as ft
    worst = {}
    for sig in (False, True):
        for ms in MIN_SCALES:
            for thr, (start, end) in ((0.1, (0.0, 1.0)), (0.0025, (0.0, 1.0)), (0.0016, (0.25, 0.5))):
                label = f"P={P} sig={int(sig)} ms={ms:.4g} min_integral={thr} [{start}, {end}]"
                c, _ = tm.make_case(P, 0.37, seed=500 + P)      # (a draw whose fp64 integrals leave the band empty up to P = 257 -- one row there would already be over 0.1 % -- and hold one row at 4099)
                center, moved = c["center"].copy(), 0
                for _ in range(4):      # rows in the band around the threshold leave it
                    band = np.abs(tm.integral(c["head"], center, ms, sig, start, end) - thr) <= 1e-5
                    if not band.any():
                        break
                    moved += int(band.sum())
                    center[band] += np.float32(0.05)
                assert not band.any() and moved <= 0.001 * P, (label, moved)
                I64 = tm.integral(c["head"], center, ms, sig, start, end)
                dead64, _, _ = tm.integral_outputs(I64, thr)
                I32 = tm.torch_integral(torch.from_numpy(c["head"]), torch.from_numpy(center), ms, sig, start, end).numpy()
                h, p = torch.tensor(c["head"], device=gpu).reshape(-1, 1), torch.tensor(center, device=gpu).reshape(-1, 1)
                integral, dead, inv, stats = ft.temporal_integral(h, p, min_scale=ms, min_integral=thr, start=start, end=end, sigmoid_tcenter=sig)
                assert tuple(integral.shape) == tuple(inv.shape) == (P, 1) and dead.dtype == torch.uint8 and tuple(dead.shape) == (P,) and stats.dtype == torch.int32
                I, dead, inv, stats = integral.cpu().numpy().reshape(-1), dead.cpu().numpy().astype(bool), inv.cpu().numpy().reshape(-1), stats.cpu().numpy()
                bar_check(label, dict(integral=I), dict(integral=I64), dict(integral=I32), worst)
                assert np.array_equal(dead, dead64), label
                # stats, inv: from the device's own integral and mask
                _, inv64, (imax, n_valid) = tm.integral_outputs(I, thr)
                assert stats.view(np.float32)[0] == np.float32(imax) and stats[1] == n_valid == (~dead).sum(), label
                assert not inv[dead].any() and np.isfinite(inv).all() and (np.abs(inv - inv64) <= ULP * np.abs(inv64)).all(), label
            # nothing valid: zeros, no NaN
            integral, dead, inv, stats = ft.temporal_integral(h, p, min_scale=ms, min_integral=10.0, sigmoid_tcenter=sig)
            assert dead.all() and not inv.any() and not stats.any()
    for k, (ratio, e_hip, e_ref, label) in worst.items():
        print(f"P={P} {k}: worst e_hip / bar {ratio:.3f} (e_hip {e_hip:.3e}, e_torch32 {e_ref:.3e}) at {label}")


# ---- prune ----------------------------------------------------------------------------------------------------------------------
def test_prune_moves_parameters_moments_stats_and_inv(gpu):
    """update_learning_rate's block on a GaussianAdam over the seven groups after two steps: survivors are bit copies, inv arrives as
    [P', 1], and the next step with lr * inv matches the dense oracle (tests/test_gpu_densify.py's tolerances)."""
    import densify_math as dm
    import fused_adam
    import fused_densify
    import fused_temporal as ft
    from oracle import adam_oracle
    P, ms, thr, lr = 4099, 0.01, 0.0025, 1e-3
    rng = np.random.default_rng(31)
    shapes = dm.shapes(16)
    f = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    leaves = {k: nn.Parameter(f(rng.uniform(-0.2, 1.2, (P, 1)) if k == "temporal_pos" else rng.standard_normal((P,) + s))) for k, s in shapes.items()}
    opt = fused_adam.GaussianAdam([{"params": [leaves[k]], "lr": lr, "name": k} for k in dm.GROUPS], eps=1e-15)
    for _ in range(2):
        for p in leaves.values():
            p.grad = f(rng.standard_normal(tuple(p.shape)) * 1e-2)
        opt.step()
    head = f(rng.uniform(0, 1, (P, 1)))
    stats = fused_densify.DensifyStats(P, gpu)
    stats.xyz_gradient_accum, stats.denom, stats.max_radii2D = f(rng.random((P, 1))), f(rng.integers(0, 5, (P, 1))), f(np.arange(P))
    t_accum = f(rng.random((P, 1)))
    _, dead, inv_full, _ = ft.temporal_integral(head, leaves["temporal_pos"].detach(), min_scale=ms, min_integral=thr)
    valid = dead == 0
    n = int(valid.sum())
    assert 0 < n < P
    old = {k: (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for k, p in leaves.items()}
    old_stats = (stats.xyz_gradient_accum.clone(), stats.denom.clone(), stats.max_radii2D.clone())
    counts, new, inv, rest = ft.temporal_prune(opt, head, leaves["temporal_pos"].detach(), min_scale=ms, min_integral=thr, stats=stats, extras=[t_accum])
    assert counts["P"] == counts["n_kept"] == n and tuple(inv.shape) == (n, 1) and torch.equal(inv, inv_full[valid]) and float(inv.min()) == 1.0
    assert len(rest) == 1 and torch.equal(rest[0], t_accum[valid])
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        assert p is new[k] and torch.equal(p.detach(), old[k][0][valid])
        assert torch.equal(opt.state[p]["exp_avg"], old[k][1][valid]) and torch.equal(opt.state[p]["exp_avg_sq"], old[k][2][valid])
    for got, was in zip((stats.xyz_gradient_accum, stats.denom, stats.max_radii2D), old_stats):
        assert torch.equal(got, was[valid])
    # the per-row rates of the six groups, then one step
    grads, before = {}, {}
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        before[k] = p.detach().cpu().numpy().copy()
        grads[k] = (rng.standard_normal(tuple(p.shape)) * 1e-2).astype(np.float32)
        p.grad = f(grads[k])
        if k != "temporal_pos":
            g["lr"] = lr * inv
    opt.step()
    assert opt._step == 3
    inv_np, keep = inv.cpu().numpy().astype(np.float64).reshape(-1), valid.cpu().numpy()
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        rp, rm, rv = adam_oracle.step(before[k], grads[k], old[k][1].cpu().numpy()[keep], old[k][2].cpu().numpy()[keep], lr * inv_np if k != "temporal_pos" else lr, 3)
        np.testing.assert_allclose(p.detach().cpu().numpy().astype(np.float64) - before[k], rp - before[k], rtol=2e-4, atol=1.5e-6, err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), rm, rtol=1e-5, atol=1e-6 * np.abs(rm).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv, rtol=1e-5, atol=1e-6 * np.abs(rv).max(), err_msg=k)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
class _Heads(nn.Module):
    """The four heads at the reference's shipped widths (scene/saro_gaussian.py:104-110)."""

    def __init__(self):
        super().__init__()
        seq = lambda i, h2, o, sig: nn.Sequential(*([nn.Linear(i, 128), nn.ReLU(), nn.Linear(128, h2), nn.ReLU(), nn.Linear(h2, o)] + ([nn.Sigmoid()] if sig else [])))  # noqa: E731
        self.motion_mlp, self.rot_mlp, self.shs_mlp, self.opacity_mlp = seq(41, 128, 3, False), seq(41, 128, 7, False), seq(41, 128, 48, False), seq(32, 64, 1, True)


def test_end_to_end_feature_heads_gate_rasterizer_loss(scenes, rast, gpu):
    """random field feature -> opacity head -> temporal_gate -> three heads with x_tail = time_emb -> activate_gaussians(trbfoutput = state)
    -> GaussianRasterizer -> l1_dssim_loss -> backward, at P = 500 on 64 x 48.  The gradients on temporal_pos and on the opacity head's first
    weight against the same chain with ONLY the gate replaced by its torch ops ("fp32"), within 4 x the difference between that chain and its
    fp64 run (nn.Sequential heads and torch gate in fp64 up to the epilogue: "fp64") + one ulp of the tensor's largest entry."""
    from conftest import settings_from
    import fused_epilogue
    import fused_loss
    import fused_mlp
    import fused_temporal as ft
    P, W, H, t, ms = 500, 64, 48, 0.5, 0.3
    sc = scenes.synth(P, 77, sh_degree=3)
    rs = settings_from(rast, scenes.camera(0, 1, W, H), sc, gpu)
    rng = np.random.default_rng(78)
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=gpu)  # noqa: E731
    o = sc["opacities"].clip(1e-4, 1 - 1e-4)
    raw = dict(xyz=f(sc["means3D"]), rotation=f(sc["rotations"]), scaling=f(np.log(sc["scales"])), opacity=f(np.log(o / (1 - o))),
               f_dc=f(sc["shs"][:, :1]), f_rest=f(sc["shs"][:, 1:16]))
    feat0, pos0, gt = f(rng.standard_normal((P, 32)) * 0.5), f(rng.uniform(0, 1, (P, 1))), f(rng.uniform(0, 1, (3, H, W)))
    torch.manual_seed(79)
    init = _Heads().state_dict()

    def chain(kind):
        heads = _Heads()
        heads.load_state_dict(init)
        heads = heads.to(gpu)
        pos = pos0.clone().requires_grad_(True)
        if kind == "fp64":
            heads = heads.double()
            feat = feat0.double()
            head = heads.opacity_mlp(feat)
            _, state, emb = tm.torch_gate(head, pos.double(), t, ms, 4)
            hin = torch.cat((feat, emb), 1)
            motion, rot, shs, state = heads.motion_mlp(hin).float(), heads.rot_mlp(hin).float(), heads.shs_mlp(hin).float(), state.float()
        else:
            assert fused_mlp.convert_heads(heads) == list(fused_mlp.HEAD_NAMES)
            head = heads.opacity_mlp(feat0)
            if kind == "fused":
                _, state, emb = ft.temporal_gate(head, pos, t, min_scale=ms)
            else:
                _, state, emb = tm.torch_gate(head, pos, t, ms, 4)
            motion, rot, shs = heads.motion_mlp(feat0, emb), heads.rot_mlp(feat0, emb), heads.shs_mlp(feat0, emb)
        means3D, rots, scales, opac, sh = fused_epilogue.activate_gaussians(
            raw["xyz"], raw["rotation"], raw["scaling"], raw["opacity"], raw["f_dc"], raw["f_rest"], motion_residual=0.05 * motion,
            rot_residual=0.1 * rot, trbfoutput=state, shs_residual=0.1 * shs.reshape(P, 16, 3))
        m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color = rast.GaussianRasterizer(rs)(means3D=means3D, means2D=m2, opacities=opac, shs=sh, scales=scales, rotations=rots)[0]
        fused_loss.l1_dssim_loss(color, gt, 0.2).backward()
        torch.cuda.synchronize()
        return {"image": color.detach().double().cpu().numpy(), "temporal_pos": pos.grad.double().cpu().numpy(),
                "opacity_mlp.0.weight": dict(heads.named_parameters())["opacity_mlp.0.weight"].grad.double().cpu().numpy()}

    truth, ref, got = chain("fp64"), chain("fp32"), chain("fused")
    assert float(np.abs(truth["image"]).max()) > 0.1
    for k in ("temporal_pos", "opacity_mlp.0.weight"):
        assert np.isfinite(got[k]).all() and np.abs(got[k]).max() > 0 and np.abs(truth[k]).max() > 0, k
        diff, bound = float(np.abs(got[k] - ref[k]).max()), 4 * float(np.abs(ref[k] - truth[k]).max()) + ULP * float(np.abs(truth[k]).max())
        print(f"end to end {k}: |fused - fp32| {diff:.3e}  bar {bound:.3e}  max|truth| {np.abs(truth[k]).max():.3e}")
        assert diff <= bound, (k, diff, bound)
