"""-m gpu: the absolute screen-space gradient (`absgrad=sink`; include/gsrast.h: GSRAST_RENDER_ABSGRAD, blend_bwd_cull_t_kernel<.., ABS>)
against tests/absgrad_math.py -- torch fp64 on tests/math_renderer.py, one differentiation per pixel.

The cases (absgrad_math.CASES) are the smallest shapes at which the kernel can still go wrong: a 32 x 32 (four tiles, every 8 x 8 block),
b 40 x 24 (ragged tiles, lanes outside the image), c one 16 x 16 tile whose 200 Gaussians every pixel walks (batches of 64, partly-alive
groups of eight), d = a with the aux outputs' gradients, e = a anti-aliased, f = a through GaussianRasterizerRaw with every residual.  The
upstream gradient is zero on the math renderer's fp32-ambiguous pixels (< 5 % of each case, asserted).  The bar is conftest.grad_tol(ref),
1e-5 max|ref| + 1e-4 |ref| with no fp32 floor: an absolute sum cancels less than the signed one that already meets it.  Measured on the
MI355X, max |err| (max |ref|): a 6.4e-5 (116), b 3.2e-5 (173), c 1.2e-6 (5.3), d 8.8e-5 (141), e 6.5e-5 (107), f 3.2e-5 (102) -- under 1 % of
the bar everywhere.

On float atomics: two backwards of the same call do not give bit-equal gradients (the four waves of a tile add into one LDS accumulator,
the tiles into one record, in whatever order they arrive -- so it was before the sink existed).  "Nothing else moves" therefore holds
bit for bit for everything the forward returns, and for the gradients within the same bar as everything else, with the same zero rows."""
import numpy as np
import pytest
import torch

import absgrad_math as am
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu

RAW_ARGS = dict(xyz="xyz", rotation="rotation", scaling="scaling", opacity="opacity_logit", features_dc="features_dc", features_rest="features_rest",
                motion_residual="motion_res", rot_residual="rot_res", trbfoutput="trbf", shs_residual="shs_res")
DENSE = ("means3D", "opacities", "shs", "scales", "rotations")


def _run(rast, gpu, name, sink=True, backwards=1):
    """One render of the case + `backwards` backwards.  dict(out = the forward's tuple, grads = {leaf: grad} + means2D, sink = the [P,2]
    tensor (pre-filled with NaN) or None, sinks = its value after each backward)."""
    r = am.reference(name)
    sc, cam, c = r["sc"], r["cam"], r["c"]
    P = c["P"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)      # noqa: E731
    rs = settings_from(rast, cam, sc, gpu)
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    s = torch.full((P, 2), float("nan"), device=gpu) if sink else None
    kw = dict(return_aux=bool(c.get("aux")), antialiasing=bool(c.get("aa")))
    if sink:
        kw["absgrad"] = s
    if c.get("raw"):
        leaves = {n: t(v).requires_grad_(True) for n, v in sc["raw"].items()}
        out = rast.GaussianRasterizerRaw(rs)(means2D=m2, **{a: leaves[n] for a, n in RAW_ARGS.items()}, **kw)
    else:
        leaves = {n: t(sc[n]).requires_grad_(True) for n in DENSE}
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                                          scales=leaves["scales"], rotations=leaves["rotations"], **kw)
    loss = (out[0] * t(r["g"])).sum()
    if c.get("aux"):
        loss = loss + (out[3][0] * t(r["gD"])).sum() + (out[4][0] * t(r["gA"])).sum()
    sinks = []
    for k in range(backwards):
        for x in list(leaves.values()) + [m2]:
            x.grad = None
        loss.backward(retain_graph=k + 1 < backwards)
        torch.cuda.synchronize()
        if sink:
            sinks.append(s.clone())
    grads = {n: x.grad.detach().clone() for n, x in leaves.items()}
    grads["means2D"] = m2.grad.detach().clone()
    return dict(out=out, grads=grads, sink=s, sinks=sinks, r=r)


def _np(x):
    return x.detach().double().cpu().numpy()


def _within_bar(got, ref, what):
    err = np.abs(got - ref)
    tol = grad_tol(ref)
    print(f"{what}: max|err| {err.max():.3e}  max|ref| {np.abs(ref).max():.3e}  worst err / bar {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (err <= tol).all(), (what, float(err.max()), float(np.abs(ref).max()))


@pytest.fixture(scope="module")
def plain_a(rast, gpu):
    """Case a with a sink, one backward: what the forced paths below are compared with."""
    return _run(rast, gpu, "a")


# ---- 1, 2, 4: against the fp64 helper; not the signed gradient; zeros and NaN --------------------------------------------------------
@pytest.mark.parametrize("name", list(am.CASES))
def test_against_the_fp64_helper(name, rast, gpu):
    h = _run(rast, gpu, name)
    r = h["r"]
    vis = r["out"]["proj"]["disc"]["vis"]
    assert r["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    radii = h["out"][1].cpu().numpy()
    assert np.array_equal(radii > 0, vis), "radius decision differs: pick another seed"
    got = _np(h["sink"])
    assert not np.isnan(got).any(), "a row of the sink was not written"
    assert not got[radii == 0].any(), "a culled Gaussian's row must be exactly zero"
    assert float(r["abs"].max()) > 0.0 and (got >= 0.0).all()
    _within_bar(got, r["abs"], f"absgrad, case {name}")
    signed = _np(h["grads"]["means2D"])[:, :2]
    # the statistic is not the signed gradient of the same backward with its sign dropped
    assert (got >= np.abs(signed) * (1.0 - 1e-4)).all()
    if name == "c":
        assert r["out"]["tile_list_max"] > 128 and not r["out"]["stopped"].any()
        assert ((got[vis] > 2.0 * np.abs(signed[vis])).any(axis=1)).mean() >= 0.1


def test_every_backward_overwrites_the_sink(rast, gpu):
    h = _run(rast, gpu, "a", backwards=2)
    a, b = _np(h["sinks"][0]), _np(h["sinks"][1])
    assert not np.isnan(b).any() and float(a.max()) > 0.0
    _within_bar(b, a, "second backward against the first")      # (it does not accumulate: twice the value is far outside)
    _within_bar(b, h["r"]["abs"], "second backward against the helper")


def test_autograd_grad_fills_the_sink_like_backward(rast, gpu, plain_a):
    r = am.reference("a")
    sc, cam, c = r["sc"], r["cam"], r["c"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)      # noqa: E731
    leaves = {n: t(sc[n]).requires_grad_(True) for n in DENSE}
    m2 = torch.zeros((c["P"], 3), device=gpu, requires_grad=True)
    s = torch.full((c["P"], 2), float("nan"), device=gpu)
    out = rast.GaussianRasterizer(settings_from(rast, cam, sc, gpu))(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], shs=leaves["shs"],
                                                                    scales=leaves["scales"], rotations=leaves["rotations"], absgrad=s)
    (g2,) = torch.autograd.grad((out[0] * t(r["g"])).sum(), [m2])
    torch.cuda.synchronize()
    assert m2.grad is None      # nothing is attached to means2D
    _within_bar(_np(s), _np(plain_a["sink"]), "autograd.grad against .backward()")


# ---- 3: nothing else moves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "d", "e", "f"], ids=["plain", "aux", "antialias", "raw"])
def test_nothing_else_moves(name, rast, gpu):
    w, wo = _run(rast, gpu, name), _run(rast, gpu, name, sink=False)
    assert len(w["out"]) == len(wo["out"])
    for a, b in zip(w["out"], wo["out"]):      # colour, radii, depth (, acc_depth, alpha): bit for bit
        assert torch.equal(a, b)
    assert set(w["grads"]) == set(wo["grads"])
    for n in w["grads"]:                        # gradients: float atomics (module docstring) -- the bar, and the same zero rows
        a, b = _np(w["grads"][n]), _np(wo["grads"][n])
        P = a.shape[0]
        assert np.array_equal((a.reshape(P, -1) != 0).any(1), (b.reshape(P, -1) != 0).any(1)), n
        _within_bar(a, b, f"{name}: {n} with a sink against without")


# ---- 5: sparse / cut paths ----------------------------------------------------------------------------------------------------------
def test_sparse_and_late_zero_paths(rast, gpu, plain_a):
    """The per-Gaussian backward's forms that do not visit every Gaussian -- the grouped one beside late_rows_zero_kernel (forced on at this
    size: late_fill_min_p = 0), over gradient records of which only the consumed Gaussians' were zeroed, in state buffers handed out full of
    NaN -- and the same pose a second time with the list cut always on: the rows nobody consumed are exactly zero, the rest within the bar of
    the unforced result."""
    _C = rast._C
    ref = _np(plain_a["sink"])
    assert _C.get_option("sparse_grec") == 1 and _C.get_option("touch_bits") == 1
    _C.set_option("late_fill_min_p", 0)
    _C.set_option("list_cut_always", 1)
    _C.POISON_STATE_BUFFERS = True
    try:
        first = _run(rast, gpu, "a")
        second = _run(rast, gpu, "a")
    finally:
        _C.POISON_STATE_BUFFERS = False
        _C.set_option("list_cut_always", 0)
        _C.set_option("late_fill_min_p", 750000)
    assert (ref == 0).all(axis=1).any(), "the case has no Gaussian that no pixel consumed"
    for h, what in ((first, "forced, first forward"), (second, "forced, second forward of the pose")):
        got = _np(h["sink"])
        assert not np.isnan(got).any()
        assert np.array_equal((got == 0).all(axis=1), (ref == 0).all(axis=1)), what
        _within_bar(got, ref, what)
    _C.set_option("dense_backward", 1)      # ... and the form that reads every Gaussian
    try:
        _within_bar(_np(_run(rast, gpu, "a")["sink"]), ref, "dense per-Gaussian backward")
    finally:
        _C.set_option("dense_backward", 0)


# ---- 6, 7: two-phase backward, GradArena ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_phase", [False, True], ids=["plain_arena", "factor_arena_two_phase"])
def test_with_a_grad_arena(two_phase, rast, gpu, plain_a):
    """The sink is no exchanged gradient and lives outside the arena.  two_phase: options.backward_phase 1 then 2 (a factor arena with a
    factor-ready hook), the sink handed to both."""
    _C = rast._C
    P = am.CASES["a"]["P"]
    arena = _C.GradArena(P, 16, gpu, sh_factors=True, world=1) if two_phase else _C.GradArena(P, 16, gpu)
    _C.set_grad_arena(arena)
    seen = []
    try:
        if two_phase:
            _C.set_factor_ready_hook(lambda ar: seen.append(1))
        arena.zero_grad()
        h = _run(rast, gpu, "a")
        assert arena.dirty, "the backward did not write into the arena"
    finally:
        _C.set_factor_ready_hook(None)
        _C.set_grad_arena(None)
    assert len(seen) == (1 if two_phase else 0)
    got = _np(h["sink"])
    assert not np.isnan(got).any()
    _within_bar(got, _np(plain_a["sink"]), "arena against no arena")
    _within_bar(_np(h["grads"]["means2D"]), _np(plain_a["grads"]["means2D"]), "means2D.grad, arena against no arena")


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------
def test_cull_0_with_a_sink_raises_and_the_process_lives_on(rast, gpu, plain_a):
    _C = rast._C
    _C.set_option("cull", 0)
    try:
        with pytest.raises(RuntimeError, match="transposed"):
            _run(rast, gpu, "a")
        _run(rast, gpu, "a", sink=False)      # (without a sink the un-culled kernels serve as ever)
    finally:
        _C.set_option("cull", 1)
    _within_bar(_np(_run(rast, gpu, "a")["sink"]), _np(plain_a["sink"]), "after the refusal")
