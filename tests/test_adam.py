"""Fused per-row-LR Adam (third item).  CPU: the numpy oracle against torch.optim.Adam.
GPU (-m gpu): the HIP kernel against the oracle (per-row lr) and against torch.optim.Adam on the same device (scalar lr); then the dense
kernel's element-by-element path (pointers off a 16-byte boundary), ragged tails, rows without gradient, a late step count, gradients
of very different magnitude in one tensor, and the group handling (eight groups, nine, a group without gradient)."""
import numpy as np
import pytest
import torch

SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "temporal_pos": (1,)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3, "temporal_pos": 1e-4}


def _data(P, seed, steps):
    rng = np.random.default_rng(seed)
    params = {k: rng.normal(size=(P,) + s).astype(np.float32) for k, s in SHAPES.items()}
    grads = [{k: (rng.normal(size=(P,) + s) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32) for k, s in SHAPES.items()} for _ in range(steps)]
    return params, grads


def test_numpy_oracle_matches_torch_adam():
    from oracle import adam_oracle
    P, steps = 300, 4
    params, grads = _data(P, 1, steps)
    tp = {k: torch.from_numpy(v.copy()).double().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam([{"params": [tp[k]], "lr": LRS[k], "name": k} for k in SHAPES], lr=0.0, eps=1e-15)
    st = {k: (params[k].astype(np.float64), np.zeros_like(params[k], np.float64), np.zeros_like(params[k], np.float64)) for k in SHAPES}
    for t in range(steps):
        for k in SHAPES:
            tp[k].grad = torch.from_numpy(grads[t][k]).double()
            st[k] = adam_oracle.step(st[k][0], grads[t][k], st[k][1], st[k][2], LRS[k], t + 1)
        opt.step()
    for k in SHAPES:
        np.testing.assert_allclose(st[k][0], tp[k].detach().numpy(), rtol=1e-12, atol=1e-14, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1000, 4097, 4098, 4099])      # 4097-4099: the width-1 groups end 1, 2 and 3 floats into a float4
def test_hip_adam_per_row_lr(P, gpu):
    from oracle import adam_oracle
    import fused_adam
    steps = 5
    params, grads = _data(P, 2, steps)
    rng = np.random.default_rng(3)
    inv = (1.0 + 4.0 * rng.random(P)).astype(np.float32)              # inv_intergral / its minimum: >= 1
    gp = {k: torch.from_numpy(v.copy()).to(gpu).requires_grad_(True) for k, v in params.items()}
    per_row = {"xyz", "opacity", "scaling", "rotation", "f_dc", "temporal_pos"}            # saro_gaussian.py:366-398
    opt = fused_adam.GaussianAdam([{"params": [gp[k]], "lr": 0.0, "name": k} for k in SHAPES], eps=1e-15)
    for grp in opt.param_groups:
        k = grp["name"]
        grp["lr"] = LRS[k] * torch.from_numpy(inv).to(gpu).reshape(P, 1) if k in per_row else LRS[k]
    st = {k: (params[k].astype(np.float64), np.zeros_like(params[k], np.float64), np.zeros_like(params[k], np.float64)) for k in SHAPES}
    for t in range(steps):
        for k in SHAPES:
            gp[k].grad = torch.from_numpy(grads[t][k]).to(gpu)
            lr = LRS[k] * inv.astype(np.float64) if k in per_row else LRS[k]
            st[k] = adam_oracle.step(st[k][0], grads[t][k], st[k][1], st[k][2], lr, t + 1)
        opt.step()
    for k in SHAPES:
        got = gp[k].detach().cpu().numpy().astype(np.float64)
        # fp32 parameters vs the fp64 oracle: each of the 5 updates rounds p to fp32 (ulp(|p| <= 4) = 2.4e-7 ... 4.8e-7)
        ref_disp = st[k][0] - params[k]
        np.testing.assert_allclose(got - params[k], ref_disp, rtol=2e-4, atol=1.5e-6, err_msg=k)
        # moments: fp32 sums of terms of mixed sign / magnitude -- absolute error scales with the largest term
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg"].cpu().numpy(), st[k][1], rtol=1e-5, atol=1e-6 * np.abs(st[k][1]).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg_sq"].cpu().numpy(), st[k][2], rtol=1e-5, atol=1e-6 * np.abs(st[k][2]).max(), err_msg=k)


@pytest.mark.gpu
def test_hip_adam_matches_torch_adam_on_device(gpu):
    import fused_adam
    P, steps = 2000, 6
    params, grads = _data(P, 4, steps)
    a = {k: torch.from_numpy(v.copy()).to(gpu).requires_grad_(True) for k, v in params.items()}
    b = {k: torch.from_numpy(v.copy()).to(gpu).requires_grad_(True) for k, v in params.items()}
    mine = fused_adam.GaussianAdam([{"params": [a[k]], "lr": LRS[k], "name": k} for k in SHAPES], eps=1e-15)
    ref = torch.optim.Adam([{"params": [b[k]], "lr": LRS[k], "name": k} for k in SHAPES], lr=0.0, eps=1e-15)
    for t in range(steps):
        for k in SHAPES:
            g = torch.from_numpy(grads[t][k]).to(gpu)
            a[k].grad, b[k].grad = g.clone(), g.clone()
        mine.step(); ref.step()
    for k in SHAPES:
        d = (a[k] - b[k]).abs().max().item()
        assert d <= 4e-7 * max(1.0, LRS[k] / 1e-4), (k, d)
    mine.zero_grad()
    assert all(a[k].grad is None for k in SHAPES)


# ---- the dense kernel's other branches ---------------------------------------------------------------------------------------------

PER_ROW = {"xyz", "opacity", "scaling", "rotation", "f_dc", "temporal_pos"}


def _inv(P):
    return (1.0 + 4.0 * np.random.default_rng(3).random(P)).astype(np.float32)


def _offset_leaf(a, gpu):
    """A contiguous tensor whose storage starts 4 bytes behind a 16-byte boundary: a flat buffer sliced from element 1."""
    flat = torch.zeros(a.size + 8, dtype=torch.float32, device=gpu)
    v = flat[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


def _drive(gpu, params, grads, *, lrs=LRS, per_row=PER_ROW, offset=(), grad_offset=False, first_step=0, no_grad=None):
    """Steps GaussianAdam and adam_oracle side by side over `grads` (one dict per step) with per-row rates on the `per_row` groups.
    offset: groups whose parameter (grad_offset: and gradient) lies 4 bytes off alignment; first_step: the optimizer's count before the
    first step; no_grad: {step index: group} whose .grad is None in that step.  Returns (parameters, optimizer, oracle state)."""
    from oracle import adam_oracle
    import fused_adam
    P = next(iter(params.values())).shape[0]
    inv = _inv(P)
    gp = {k: (_offset_leaf(v, gpu) if k in offset else torch.from_numpy(v.copy()).to(gpu)).requires_grad_(True) for k, v in params.items()}
    opt = fused_adam.GaussianAdam([{"params": [gp[k]], "lr": 0.0, "name": k} for k in params], eps=1e-15)
    for grp in opt.param_groups:
        k = grp["name"]
        grp["lr"] = lrs[k] * torch.from_numpy(inv).to(gpu).reshape(P, 1) if k in per_row else lrs[k]
    opt._step = first_step
    st = {k: (params[k].astype(np.float64), np.zeros(params[k].shape), np.zeros(params[k].shape)) for k in params}
    for t, g in enumerate(grads):
        for k in params:
            if no_grad and no_grad.get(t) == k:
                gp[k].grad = None
                continue
            gp[k].grad = _offset_leaf(g[k], gpu) if grad_offset and k in offset else torch.from_numpy(g[k]).to(gpu)
            lr = lrs[k] * inv.astype(np.float64) if k in per_row else lrs[k]
            st[k] = adam_oracle.step(st[k][0], g[k], st[k][1], st[k][2], lr, first_step + t + 1)
        opt.step()
    assert opt._step == first_step + len(grads)
    return gp, opt, st


def _assert_bars(gp, opt, params, st):
    """test_hip_adam_per_row_lr's bars."""
    for k in params:
        got = gp[k].detach().cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(got - params[k], st[k][0] - params[k], rtol=2e-4, atol=1.5e-6, err_msg=k)
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg"].cpu().numpy(), st[k][1], rtol=1e-5, atol=1e-6 * np.abs(st[k][1]).max(), err_msg=k)
        np.testing.assert_allclose(opt.state[gp[k]]["exp_avg_sq"].cpu().numpy(), st[k][2], rtol=1e-5, atol=1e-6 * np.abs(st[k][2]).max(), err_msg=k)


def _bits(opt, gp, k):
    return [x.detach().contiguous().view(torch.int32) for x in (gp[k], opt.state[gp[k]]["exp_avg"], opt.state[gp[k]]["exp_avg_sq"])]


@pytest.mark.gpu
@pytest.mark.parametrize("grad_offset", [False, True], ids=["param_off", "param_and_grad_off"])
def test_hip_adam_unaligned_group(grad_offset, gpu):
    """f_rest and rotation -- second case: their gradients too -- 4 bytes off a 16-byte boundary: adam_step_kernel takes its
    element-by-element path for those groups.  Same bars, and the bits of the same steps on aligned copies."""
    params, grads = _data(65, 2, 5)
    gp, opt, st = _drive(gpu, params, grads, offset=("f_rest", "rotation"), grad_offset=grad_offset)
    assert gp["f_rest"].data_ptr() % 16 == 4 and gp["rotation"].data_ptr() % 16 == 4 and gp["xyz"].data_ptr() % 16 == 0
    _assert_bars(gp, opt, params, st)
    gp2, opt2, _ = _drive(gpu, params, grads)
    for k in params:
        for a, b in zip(_bits(opt, gp, k), _bits(opt2, gp2, k)):
            assert torch.equal(a, b), k


@pytest.mark.gpu
def test_hip_adam_rows_without_gradient(gpu):
    """60 % of the rows have an exactly zero gradient in every step: m = v = 0 exactly and p - lr * (0 / eps) keeps p bit for bit."""
    P, steps = 1000, 5
    params, grads = _data(P, 5, steps)
    dead = np.random.default_rng(6).random(P) < 0.6
    for g in grads:
        for k in g:
            g[k][dead] = 0.0
    gp, opt, st = _drive(gpu, params, grads)
    _assert_bars(gp, opt, params, st)
    rows = torch.from_numpy(dead).to(gpu)
    for k in params:
        p, m, v = _bits(opt, gp, k)
        assert torch.equal(p[rows], torch.from_numpy(params[k]).to(gpu).view(torch.int32)[rows]), k
        assert not m[rows].any() and not v[rows].any(), k
        assert bool((gp[k].detach()[~rows] != torch.from_numpy(params[k]).to(gpu)[~rows]).any()), k


@pytest.mark.gpu
def test_hip_adam_late_step(gpu):
    """The optimizer's count stands at 29 999 before the first step: both bias corrections are ~1 (1 - 0.999^30000 = 1 - 9e-14)."""
    P, steps = 1000, 5
    params, grads = _data(P, 7, steps)
    gp, opt, st = _drive(gpu, params, grads, first_step=29_999)
    assert opt._step == 30_004
    _assert_bars(gp, opt, params, st)


@pytest.mark.gpu
def test_hip_adam_gradient_magnitudes(gpu):
    """Per-row gradient scales from 1e-12 to 1e4 in one tensor (v from 1e-27 to 1e5 next to eps = 1e-15)."""
    P, steps = 1000, 5
    rng = np.random.default_rng(8)
    params, _ = _data(P, 8, 0)
    scale = 10.0 ** rng.permutation(np.linspace(-12.0, 4.0, P))
    grads = [{k: (rng.normal(size=(P,) + s) * scale.reshape((P,) + (1,) * len(s))).astype(np.float32) for k, s in SHAPES.items()} for _ in range(steps)]
    assert min(np.abs(g["f_rest"]).max(axis=(1, 2)).min() for g in grads) < 1e-11 and max(np.abs(g["f_rest"]).max() for g in grads) > 1e4
    gp, opt, st = _drive(gpu, params, grads)
    _assert_bars(gp, opt, params, st)
    for k in params:
        assert torch.isfinite(gp[k]).all(), k


def _nine(P, device):
    shapes = dict(SHAPES, extra=(2,), ninth=(5,))
    return shapes, {k: torch.zeros((P,) + s, device=device) for k, s in shapes.items()}


def test_adam_nine_groups_are_refused():
    import fused_adam
    _, tensors = _nine(4, "cpu")
    with pytest.raises(ValueError, match="8 groups"):
        fused_adam.GaussianAdam([{"params": [v], "lr": 1e-3, "name": k} for k, v in tensors.items()])
    fused_adam.GaussianAdam([{"params": [v], "lr": 1e-3, "name": k} for k, v in list(tensors.items())[:8]])


@pytest.mark.gpu
def test_hip_adam_eight_groups_in_one_launch(gpu):
    P, steps = 333, 5
    shapes = dict(SHAPES, extra=(2,))
    lrs = dict(LRS, extra=3e-3)
    rng = np.random.default_rng(9)
    params = {k: rng.normal(size=(P,) + s).astype(np.float32) for k, s in shapes.items()}
    grads = [{k: (rng.normal(size=(P,) + s) * 10.0 ** rng.uniform(-6, 0)).astype(np.float32) for k, s in shapes.items()} for _ in range(steps)]
    gp, opt, st = _drive(gpu, params, grads, lrs=lrs, per_row=PER_ROW | {"extra"})
    assert len(opt.param_groups) == 8
    _assert_bars(gp, opt, params, st)


@pytest.mark.gpu
def test_hip_adam_group_without_gradient_is_skipped(gpu):
    """A group whose .grad is None sits a step out (parameter and moments bit for bit) while the others step; the one global step count
    advances once, so the group's next step is bias-corrected with that count."""
    P, steps = 333, 5
    params, grads = _data(P, 10, steps)
    gp, opt, st = _drive(gpu, params, grads[:2])
    before = [x.clone() for x in _bits(opt, gp, "opacity")]
    others = [x.clone() for x in _bits(opt, gp, "xyz")]
    gp["opacity"].grad = None
    for k in SHAPES:
        if k != "opacity":
            gp[k].grad = torch.from_numpy(grads[2][k]).to(gpu)
    opt.step()
    assert opt._step == 3
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(opt, gp, "opacity")))
    assert not any(torch.equal(a, b) for a, b in zip(others, _bits(opt, gp, "xyz")))
    # the whole sequence against the oracle: opacity without gradient in step 3 and also in step 1 (no state yet)
    gp, opt, st = _drive(gpu, params, grads, no_grad={0: "opacity", 2: "opacity"})
    _assert_bars(gp, opt, params, st)
