"""MCMC densification on the device (-m gpu): fused_densify.mcmc_relocate / mcmc_grow / mcmc_inject_noise / mcmc_refine and the C calls
under them against the fp64 restatement of tests/mcmc_math.py.

Sizes: 255 / 256 / 257 straddle one 256-row workgroup, 4099 is ragged over 17 of them, 70001 gives 274 workgroup sums -- more than the
256 the single-workgroup scan takes per turn, so its carry runs -- and a total weight past 2^32, so the 64-bit prefix runs (asserted).
Groups: those of tests/densify_math.py (widths 1, 3, 4, 9 / 45), with and without moments.  Opacities are drawn at least 3 % clear of
min_opacity (asserted), so the fp32 and the fp64 sigmoid agree on who is dead; nothing is redrawn or left out.
The sampler is integer arithmetic from the weights on: the device's own q goes through the restatement's Python-integer sampler and src /
count must be EQUAL.  Copies, gathered moments and counts are compared exactly; the computed values (new opacity logit, new log-scale, the
noised xyz) at the project's bar made scale-free as conftest.grad_tol does: ATOL * max|ref| + RTOL * |ref|."""
import functools

import pytest
import torch

import densify_math as dm
import mcmc_math as mm
from conftest import ATOL, RTOL

pytestmark = pytest.mark.gpu

MIN_O = 0.005
SIZES = (1, 255, 256, 257, 4099, 70001)
PATTERNS = ("none", "all", "every_other", "one_alive", "run_boundary", "mask")
COPY_GROUPS = tuple(k for k in dm.GROUPS if k not in ("opacity", "scaling"))


@functools.lru_cache(maxsize=None)
def make_case(P, M, pattern, with_moments=True, high=False):
    """Inputs (CPU, fp32, never modified): the seven groups, moments, the dead flags and the explicit mask (pattern "mask" only)."""
    d = dm.draw(P, M, "none", seed=1000 + P + M, with_moments=with_moments)
    gen = torch.Generator().manual_seed(77 + P)
    u = torch.rand(P, generator=gen, dtype=torch.float64)
    idx = torch.arange(P)
    dead = {"none": idx < 0, "all": idx >= 0, "every_other": idx % 2 == 0, "one_alive": idx != P // 2,
            "run_boundary": (idx >= 200) & (idx < 330), "mask": torch.rand(P, generator=gen) < 0.3}[pattern]
    alive_o = (0.97 + 0.029 * u) if high else (0.01 + 0.98 * u)
    by_opacity = dead if pattern != "mask" else idx < 0
    o = torch.where(by_opacity, MIN_O * (0.05 + 0.9 * u), alive_o)
    params = dict(d["params"])
    params["opacity"] = torch.log(o / (1 - o)).float().reshape(P, 1)
    o64 = mm.sigmoid(params["opacity"]).reshape(-1)
    assert bool(((o64 - MIN_O).abs() >= 0.03 * MIN_O).all())
    assert torch.equal(o64 <= MIN_O, by_opacity)
    return dict(P=P, params=params, moments=d["moments"], dead=dead, mask=dead if pattern == "mask" else None)


def _optimizer(case, gpu, step=3):
    import fused_adam
    leaves = {k: torch.nn.Parameter(v.clone().to(gpu)) for k, v in case["params"].items()}
    opt = fused_adam.GaussianAdam([{"params": [leaves[k]], "lr": 1e-3, "name": k} for k in dm.GROUPS], eps=1e-15)
    if case["moments"] is not None:
        for k, p in leaves.items():
            opt.state[p] = {"exp_avg": case["moments"][k][0].clone().to(gpu), "exp_avg_sq": case["moments"][k][1].clone().to(gpu)}
    opt._step = step
    return opt, leaves


def _plan(opacity, gpu, min_opacity, mask=None):
    """gsrast_mcmc_plan on its own: (scratch, q as a list of ints, [n_dead, n_alive, W])."""
    import diff_gaussian_rasterization_ch3 as rast
    L = rast._C.lib()
    P = int(opacity.shape[0])
    op = opacity.to(gpu).contiguous()
    m8 = mask.to(torch.uint8).to(gpu) if mask is not None else None
    scratch = torch.empty(int(L.gsrast_mcmc_scratch_bytes(P, 0)), dtype=torch.uint8, device=gpu)
    q, counts = torch.empty(P, dtype=torch.int32, device=gpu), torch.empty(4, dtype=torch.int32, device=gpu)
    rc = L.gsrast_mcmc_plan(P, op.data_ptr(), m8.data_ptr() if m8 is not None else None, min_opacity, q.data_ptr(), scratch.data_ptr(), counts.data_ptr(),
                            torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.gsrast_last_error()
    c = [int(v) & 0xFFFFFFFF for v in counts.cpu().tolist()]
    return scratch, [int(v) & 0xFFFFFFFF for v in q.cpu().tolist()], [c[0], c[1], c[2] | (c[3] << 32)]


def _draws(n, seed, ends=True):
    d = torch.randint(0, mm.DRAW_RANGE, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    if ends and n >= 2:
        d[0], d[-1] = 0, mm.DRAW_RANGE - 1
    return d


def _close(got, ref, scale=None):
    """|got - ref| <= ATOL * max|ref| + RTOL * |ref| (fp64 tensors); returns the worst error for the message."""
    if ref.numel() == 0:
        return True, 0.0
    tol = ATOL * float((ref if scale is None else scale).abs().max()) + RTOL * ref.abs()
    err = (got - ref).abs()
    return bool((err <= tol).all()), float(err.max())


# ---- (a) weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", SIZES)
def test_weights_and_counts(P, pattern, gpu):
    case = make_case(P, 4, pattern)
    _, q, (n_dead, n_alive, W) = _plan(case["params"]["opacity"], gpu, MIN_O, case["mask"])
    dead = case["dead"]
    assert n_dead == int(dead.sum()) and n_alive == P - n_dead and W == sum(q)
    qt = torch.tensor(q, dtype=torch.float64)
    assert not qt[dead].any() and bool((qt[~dead] >= 1).all())
    o = mm.sigmoid(case["params"]["opacity"]).reshape(-1)
    ok, err = _close(qt[~dead] / mm.Q_ONE, o[~dead])
    assert ok, err
    ref_q, ref_dead = mm.weights(case["params"]["opacity"], MIN_O, case["mask"])
    # one unit of q is one ulp of an fp32 in [0.5, 1): expf, the add and the divide are within 2 + 0.5 + 0.5 ulp, the floor adds one
    assert torch.equal(ref_dead, dead) and int((qt.long() - ref_q).abs().max()) <= 8


def test_weights_past_32_bits(gpu):
    case = make_case(70001, 4, "none", True, True)
    _, q, (_, n_alive, W) = _plan(case["params"]["opacity"], gpu, MIN_O)
    assert n_alive == 70001 and W == sum(q) and W > 1 << 32 and min(q) > 0.96 * mm.Q_ONE


# ---- (b) sampling -------------------------------------------------------------------------------------------------------------
def _sample(P, n, draws, scratch, gpu):
    import diff_gaussian_rasterization_ch3 as rast
    L = rast._C.lib()
    dd = draws.to(gpu)
    src, count = torch.full((max(n, 1),), -7, dtype=torch.int32, device=gpu), torch.full((P,), -7, dtype=torch.int32, device=gpu)
    rc = L.gsrast_mcmc_sample(P, n, dd.data_ptr() if n else None, scratch.data_ptr(), src.data_ptr() if n else None, count.data_ptr(),
                              torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.gsrast_last_error()
    return src[:n].cpu().tolist(), count.cpu().tolist()


@pytest.mark.parametrize("P,pattern,high", [(1, "none", False), (255, "every_other", False), (256, "mask", False), (257, "one_alive", False),
                                             (4099, "run_boundary", False), (70001, "every_other", False), (70001, "none", True)])
def test_sampling_is_the_integer_restatement(P, pattern, high, gpu):
    case = make_case(P, 4, pattern, True, high)
    scratch, q, (_, _, W) = _plan(case["params"]["opacity"], gpu, MIN_O, case["mask"])
    assert W > 0 and (P < 70001 or W > 1 << 32)
    for n in (0, 1, 300, 2 * P):
        draws = _draws(n, seed=P + n)
        src, count = _sample(P, n, draws, scratch, gpu)
        ref_src, ref_count = mm.sample(q, draws.tolist())
        assert src == ref_src and count == ref_count, (P, n)
        assert all(q[i] > 0 for i in src)


# ---- (c, d) relocate ----------------------------------------------------------------------------------------------------------
def _relocate_and_check(case, gpu, seed=5):
    import fused_densify
    P, dead, has_m = case["P"], case["dead"], case["moments"] is not None
    opt, leaves = _optimizer(case, gpu)
    keys = set(opt.state.keys())
    n_dead = int(dead.sum())
    draws = _draws(n_dead, seed)
    mask = None if case["mask"] is None else case["mask"].to(gpu)
    counts = fused_densify.mcmc_relocate(opt, min_opacity=MIN_O, dead_mask=mask, draws=draws.to(gpu))
    noop = n_dead == 0 or n_dead == P
    assert counts == dict(n_dead=n_dead, n_alive=P - n_dead, n_relocated=0 if noop else n_dead)
    assert all(g["params"][0] is leaves[g["name"]] for g in opt.param_groups) and set(opt.state.keys()) == keys and opt._step == 3
    got = {k: leaves[k].detach().cpu() for k in dm.GROUPS}
    got_m = {k: (opt.state[leaves[k]]["exp_avg"].cpu(), opt.state[leaves[k]]["exp_avg_sq"].cpu()) for k in dm.GROUPS} if has_m else None
    if noop:
        for k in dm.GROUPS:
            assert torch.equal(got[k], case["params"][k]), k
            if has_m:
                assert torch.equal(got_m[k][0], case["moments"][k][0]) and torch.equal(got_m[k][1], case["moments"][k][1]), k
        return opt, counts
    _, q, _ = _plan(case["params"]["opacity"], gpu, MIN_O, case["mask"])
    src, count = mm.sample(q, draws.tolist())
    ref = mm.relocate(case["params"], case["moments"], dead, src, count, MIN_O)
    src_t, dead_idx = torch.tensor(src, dtype=torch.long), torch.nonzero(dead).reshape(-1)
    sampled = torch.tensor(count) > 0
    changed = dead | sampled
    assert not bool((dead & sampled).any())
    # which rows changed, exactly: a dead row's opacity rises to at least min_opacity, a source's falls
    assert torch.equal((got["opacity"] != case["params"]["opacity"]).reshape(P, -1).any(1), changed)
    for k in dm.GROUPS:
        g, x = got[k], case["params"][k]
        assert torch.equal(g[~changed], x[~changed]), k
        if k in COPY_GROUPS:
            assert torch.equal(g[dead_idx], x[src_t]) and torch.equal(g[sampled], x[sampled]), k
        else:
            ok, err = _close(g.double()[changed], ref[k][0][changed], scale=ref[k][0])
            assert ok, (k, err)
            assert torch.equal(g[dead_idx], g[src_t]), k              # a copy carries its source's new value bit for bit
        if has_m:
            for a, b in zip(got_m[k], case["moments"][k]):
                assert not a[sampled].any() and torch.equal(a[~sampled], b[~sampled]), k      # sources: zero; dead rows and the rest: their own
    return opt, counts


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("P", SIZES)
def test_relocate_sizes_and_widths(P, M, gpu):
    _relocate_and_check(make_case(P, M, "every_other" if P > 1 else "none"), gpu)


@pytest.mark.parametrize("P", [257, 4099])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_relocate_dead_patterns(pattern, P, gpu):
    _, counts = _relocate_and_check(make_case(P, 4, pattern), gpu)
    if pattern == "one_alive":
        assert counts["n_alive"] == 1 and counts["n_relocated"] == P - 1 > 51       # one source for every dead row: the ratio clamps at 51


def test_relocate_single_row_and_no_moments(gpu):
    _relocate_and_check(make_case(1, 4, "all"), gpu)
    opt, _ = _relocate_and_check(make_case(300, 4, "every_other", False), gpu)
    assert not opt.state


def test_relocate_extras_and_generator(gpu):
    """extras travel like COPY groups; without `draws` the draws are torch.randint(0, 2^62) from the caller's generator on the device."""
    import fused_densify
    case = make_case(4099, 4, "every_other")
    n_dead = int(case["dead"].sum())
    outs = []
    for given in (False, True):
        opt, leaves = _optimizer(case, gpu)
        extra = torch.arange(4099 * 2, dtype=torch.float32, device=gpu).reshape(4099, 2)
        gen = torch.Generator(device=gpu).manual_seed(9)
        kw = dict(draws=torch.randint(0, mm.DRAW_RANGE, (n_dead,), generator=gen, device=gpu, dtype=torch.int64)) if given else dict(generator=gen)
        fused_densify.mcmc_relocate(opt, min_opacity=MIN_O, extras=[extra], **kw)
        outs.append((leaves["xyz"].detach().clone(), extra))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    xyz, extra = outs[0]
    moved = torch.nonzero(case["dead"]).reshape(-1).to(gpu)
    from_row = (extra[moved, 0] / 2).long()                         # the extra names the row it was copied from
    assert torch.equal(xyz[moved], case["params"]["xyz"].to(gpu)[from_row]) and not bool(case["dead"].to(gpu)[from_row].any())
    with pytest.raises(RuntimeError, match="no group named"):
        fused_densify.mcmc_relocate(_optimizer(case, gpu)[0], names=dict(fused_densify.DEFAULT_NAMES, opacity="alpha"))


# ---- (e) grow -----------------------------------------------------------------------------------------------------------------
def _grow_and_check(case, gpu, cap_max, growth=1.05, seed=6):
    import fused_densify
    P, has_m = case["P"], case["moments"] is not None
    n = max(0, min(cap_max, int(growth * P)) - P)
    opt, leaves = _optimizer(case, gpu)
    draws = _draws(n, seed)
    counts, new, extras = fused_densify.mcmc_grow(opt, cap_max=cap_max, growth=growth, min_opacity=MIN_O, draws=draws.to(gpu))
    assert counts == dict(n_added=n, P=P + n) and extras == [] and opt._step == 3
    if n == 0:
        assert all(g["params"][0] is leaves[g["name"]] and new[g["name"]] is leaves[g["name"]] for g in opt.param_groups)
        return
    _, q, _ = _plan(case["params"]["opacity"], gpu, 0.0)
    src, count = mm.sample(q, draws.tolist())
    ref = mm.grow(case["params"], case["moments"], src, count, MIN_O)
    src_t, sampled = torch.tensor(src, dtype=torch.long), torch.tensor(count) > 0
    assert set(opt.state.keys()) == ({g["params"][0] for g in opt.param_groups} if has_m else set())
    for g in opt.param_groups:
        k, p = g["name"], g["params"][0]
        assert p is new[k] and p is not leaves[k] and isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad and p.grad is None
        assert tuple(p.shape) == (P + n,) + tuple(case["params"][k].shape[1:])
        got, x = p.detach().cpu(), case["params"][k]
        assert torch.equal(got[:P][~sampled], x[~sampled]), k
        if k in COPY_GROUPS:
            assert torch.equal(got[:P], x) and torch.equal(got[P:], x[src_t]), k
        else:
            ok, err = _close(got.double(), ref[k][0])
            assert ok, (k, err)
            assert torch.equal(got[P:], got[src_t]), k                 # new rows in draw order, copies of the UPDATED sources
            if k == "opacity":
                assert torch.equal((got[:P] != x).reshape(P, -1).any(1), sampled)      # which of the old rows changed, exactly
        if has_m:
            st = opt.state[p]
            for a, b in zip((st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()), case["moments"][k]):
                assert a.shape == p.shape and torch.equal(a[:P], b) and not a[P:].any(), k


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("P", SIZES)
def test_grow_sizes_and_widths(P, M, gpu):
    _grow_and_check(make_case(P, M, "every_other" if P > 1 else "none"), gpu, cap_max=10**9, growth=1.05 if P > 1 else 3.0)


def test_grow_cap_and_no_moments(gpu):
    case = make_case(4099, 4, "none")
    _grow_and_check(case, gpu, cap_max=4099 + 7)                    # the cap binds: 7 rows, not 204
    _grow_and_check(case, gpu, cap_max=4099)                        # cap_max <= P: nothing happens, nothing is re-installed
    _grow_and_check(case, gpu, cap_max=100)
    _grow_and_check(make_case(300, 4, "run_boundary", False), gpu, cap_max=10**9, growth=2.5)      # more new rows than old, no optimizer state


# ---- (f) noise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_row_scale", [False, True])
@pytest.mark.parametrize("P", [1, 257, 4099])
def test_noise(P, with_row_scale, gpu):
    import fused_densify
    gen = torch.Generator().manual_seed(40 + P)
    xyz, eps = torch.randn(P, 3, generator=gen), torch.randn(P, 3, generator=gen)
    rot = torch.randn(P, 4, generator=gen) * 3.0                    # unnormalised quaternions
    scaling = torch.log(0.05 + 0.45 * torch.rand(P, 3, generator=gen))
    o = 0.002 + 0.99 * torch.rand(P, generator=gen)
    solid, faint = torch.arange(P) % 3 == 1, torch.arange(P) % 3 == 0
    o[solid], o[faint] = 0.99, 0.001
    logit = torch.log(o / (1 - o)).reshape(P, 1)
    rs = (0.5 + torch.rand(P, generator=gen)) if with_row_scale else None
    scale = 20.0
    ref = mm.noise(xyz, rot, scaling, logit, eps, scale, row_scale=rs)
    x = xyz.clone().to(gpu)
    fused_densify.mcmc_inject_noise(x, rot.to(gpu), scaling.to(gpu), logit.to(gpu), scale=scale, row_scale=None if rs is None else rs.to(gpu), noise=eps.to(gpu))
    got = x.cpu().double()
    tol = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    err = (got - ref).abs()
    assert bool((err <= tol).all()), float(err.max())
    moved = (got - xyz.double())
    assert bool((moved[solid].abs() <= tol[solid]).all())          # o = 0.99: the gate is exp(-98.5)
    if faint.any():                                                  # o = 0.001: the gate is 1 / (1 + exp(-0.4)) = 0.599 of the full covariance-shaped noise
        full = mm.noise(xyz, rot, scaling, logit, eps, scale, row_scale=rs, x0=-10.0) - xyz.double()
        size = full[faint].norm(dim=1)
        big = size > 300 * float(tol.max())                          # (where the bar is under a third of a per cent of the step)
        ratio = moved[faint].norm(dim=1)[big] / size[big]
        assert bool(((ratio > 0.59) & (ratio < 0.61)).all()) and (P == 1 or int(big.sum()) > faint.sum() // 2)


def test_noise_from_the_generator_and_on_parameters(gpu):
    import fused_densify
    case = make_case(4099, 4, "none")
    outs = []
    for given in (False, True):
        _, leaves = _optimizer(case, gpu)
        gen = torch.Generator(device=gpu).manual_seed(3)
        kw = dict(noise=torch.randn((4099, 3), generator=gen, device=gpu)) if given else dict(generator=gen)
        fused_densify.mcmc_inject_noise(leaves["xyz"], leaves["rotation"], leaves["scaling"], leaves["opacity"], scale=1.0, **kw)
        assert leaves["xyz"].is_leaf and leaves["xyz"].requires_grad
        outs.append(leaves["xyz"].detach().clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0].cpu(), case["params"]["xyz"])


def test_noise_records_into_the_one_profile_table(rast, gpu):
    """The library has one timer table, whichever translation unit a call is compiled in: with the profile bit of mcmc_noise set (and no
    other), one mcmc_inject_noise shows as one launch of "mcmc_noise" in profile_read(), and the renderer's preprocess_fwd shows none."""
    import fused_densify
    _C = rast._C
    P = 256
    gen = torch.Generator().manual_seed(9)
    xyz, rot, scaling, logit = (torch.randn(P, w, generator=gen).to(gpu) for w in (3, 4, 3, 1))
    bit = list(_C.profile_read()).index("mcmc_noise")
    assert bit == 31
    _C.set_option("profile", -(1 << 31))        # bit 31 alone, as the 32-bit word the option is
    try:
        _C.profile_reset()
        fused_densify.mcmc_inject_noise(xyz, rot, scaling, logit, scale=1.0, noise=torch.randn(P, 3, generator=gen).to(gpu))
        prof = _C.profile_read()
        assert prof["mcmc_noise"][1] == 1 and prof["mcmc_noise"][0] > 0.0
        assert prof["preprocess_fwd"][1] == 0
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()


# ---- determinism and composition ----------------------------------------------------------------------------------------------
def _state(opt):
    out = []
    for g in opt.param_groups:
        p = g["params"][0]
        out.append(p.detach())
        out.extend(opt.state[p][k] for k in ("exp_avg", "exp_avg_sq"))
    return out


def test_two_runs_are_bit_identical(gpu):
    import fused_densify
    case = make_case(70001, 16, "every_other")
    n_dead = int(case["dead"].sum())
    runs = []
    for _ in range(2):
        opt, _ = _optimizer(case, gpu)
        c1 = fused_densify.mcmc_relocate(opt, min_opacity=MIN_O, draws=_draws(n_dead, 1).to(gpu))
        c2, new, _ = fused_densify.mcmc_grow(opt, cap_max=80000, min_opacity=MIN_O, draws=_draws(int(1.05 * 70001) - 70001, 2).to(gpu))
        fused_densify.mcmc_inject_noise(new["xyz"], new["rotation"], new["scaling"], new["opacity"], scale=0.5,
                                        noise=torch.randn(c2["P"], 3, generator=torch.Generator().manual_seed(3)).to(gpu))
        runs.append((c1, c2, _state(opt)))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][0]["n_relocated"] == n_dead
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_refine_then_step_render_and_densify(gpu):
    """mcmc_refine, then a GaussianAdam.step(), a render of the result at P' with the rasterizer, and densify_and_prune on the same optimizer."""
    import numpy as np
    import diff_gaussian_rasterization_ch3 as rast
    import fused_adam
    import fused_densify
    import scenes
    P, W, H = 3000, 96, 64
    sc, cam = scenes.synth(P, 7), scenes.camera(1, 6, W, H)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    o = t(sc["opacities"]).clamp(1e-4, 1 - 1e-4)
    raw = dict(xyz=t(sc["means3D"]), shs=t(sc["shs"]), opacity=torch.log(o / (1 - o)), scaling=torch.log(t(sc["scales"])), rotation=t(sc["rotations"]))
    leaves = {k: torch.nn.Parameter(v) for k, v in raw.items()}
    opt = fused_adam.GaussianAdam([{"params": [leaves[k]], "lr": 1e-3, "name": k} for k in raw], eps=1e-15)
    for p in leaves.values():
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    n_dead = int((torch.sigmoid(raw["opacity"]) <= 0.05).sum())
    counts, new = fused_densify.mcmc_refine(opt, cap_max=3100, min_opacity=0.05, generator=torch.Generator(device=gpu).manual_seed(1))
    assert counts["n_dead"] == counts["n_relocated"] == n_dead > 0 and counts["n_added"] == 100 and counts["P"] == 3100
    assert float(torch.sigmoid(new["opacity"].detach()).min()) >= 0.05 * (1 - 1e-4)          # no dead row is left
    fused_densify.mcmc_inject_noise(new["xyz"], new["rotation"], new["scaling"], new["opacity"], scale=1e-3, generator=torch.Generator(device=gpu).manual_seed(2))
    for p in new.values():
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    assert opt._step == 2 and all(bool(torch.isfinite(p).all()) for p in new.values())
    rs = rast.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(sc["bg"]), scale_modifier=1.0,
                                            viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=sc["sh_degree"], campos=t(cam["campos"]), prefiltered=False)
    color, radii, _ = rast.GaussianRasterizer(rs)(means3D=new["xyz"], means2D=torch.zeros((3100, 3), device=gpu, requires_grad=True), opacities=torch.sigmoid(new["opacity"]),
                                                  shs=new["shs"], scales=torch.exp(new["scaling"]), rotations=new["rotation"])
    assert tuple(color.shape) == (3, H, W) and radii.shape[0] == 3100 and bool(torch.isfinite(color).all()) and int((radii > 0).sum()) > 0
    stats = fused_densify.DensifyStats(3100, gpu)
    stats.xyz_gradient_accum += 1.0
    stats.denom += 1.0
    c, newer = fused_densify.densify_and_prune(opt, stats, grad_threshold=0.5, percent_dense=0.01, extent=1e9, min_opacity=0.005)
    assert c["n_clone"] == 3100 and c["P"] == 6200 and newer["xyz"].shape[0] == 6200 and opt._step == 2
