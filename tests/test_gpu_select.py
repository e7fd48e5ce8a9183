"""-m gpu: the differentiable row selection (fused_densify.select_rows / RowSelection over gsrast_densify_apply and gsrast_densify_scatter,
fused_temporal.temporal_rows).  The primitives move bits, so they are compared with torch's own indexing (x[mask], zeros.index_copy) and its
autograd under torch.equal, with no tolerance; tests/select_math.py and tests/test_select_host.py pin those expressions on the CPU.

The end-to-end bar is the project's existing one (tests/test_gpu_temporal.py), per tensor T, measured against the reference chain:
    max|T_selected - T_full| <= 4 max|T_full - T_fp64| + 2^-23 max|T_fp64|,
T_full = the chain through the fused kernels on all P rows, T_fp64 = the same chain with nn.Sequential heads and torch's gate in fp64 up to
the epilogue.  Weight-gradient sums re-associate over fewer rows, so bits are not demanded there; the zeros on dead rows are exact."""
import numpy as np
import pytest
import torch
from torch import nn

import select_math as sm
import temporal_math as tm

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 4099, 70001]      # 70001: 274 workgroup sums, so the scan of the sums runs a second turn with a carry
SHAPES = [((1,), torch.float32), ((3,), torch.float32), ((4,), torch.float32), ((15, 3), torch.float32), ((48,), torch.float32),
          ((64,), torch.float32), ((1,), torch.int32)]
SIXTEEN = [(s, torch.float32) for s in [(1,), (3,), (4,), (2, 5)] * 3] + [((7,), torch.float32), ((2,), torch.int32), ((1,), torch.int32), ((32,), torch.float32)]
ULP = 2.0 ** -23
_data = {}


def draw(rows, specs, seed, gpu, shared=False):
    """One tensor per (shape, dtype): normal floats; int32 over the whole range, a NaN's bit pattern among them.  `shared`: drawn once and kept
    for the other cases of the same size (the callers clone what they change)."""
    key = (rows, tuple(specs), seed)
    if key not in _data or not shared:
        gen = torch.Generator().manual_seed(seed)
        out = []
        for shape, dtype in specs:
            if dtype == torch.float32:
                out.append(torch.randn((rows,) + shape, generator=gen).to(gpu))
            else:
                t = torch.randint(-2 ** 31, 2 ** 31, (rows,) + shape, generator=gen, dtype=torch.int64).to(torch.int32)
                if rows:
                    t.reshape(-1)[0] = 0x7FC00001      # a quiet NaN's bits with a payload
                out.append(t.to(gpu))
        if not shared:
            return out
        _data[key] = out
    return _data[key]


def selection(keep, gpu, form):
    """fused_densify.select_rows over the numpy mask `keep`, in one of the accepted forms of the argument."""
    import fused_densify as fd
    mask = torch.from_numpy(np.ascontiguousarray(keep)).to(gpu)
    if form == 0:
        sel = fd.select_rows(keep=mask)
    elif form == 1:
        sel = fd.select_rows(dead=~mask)
    elif form == 2:
        sel = fd.select_rows(keep=(mask.to(torch.uint8) * 3).reshape(-1, 1))      # uint8 [P, 1]: any non-zero value keeps
    else:
        sel = fd.select_rows(dead=(~mask).to(torch.uint8) * 255)
    return sel, mask


def check_both_directions(sel, mask, specs, seed, gpu):
    """gather == x[mask], scatter == zeros.index_copy(0, rows, y), and both backwards == torch.autograd of those expressions: torch.equal."""
    P, n = int(mask.shape[0]), int(mask.sum())
    idx = mask.nonzero().reshape(-1)
    is_f = [d == torch.float32 for _, d in specs]
    xs, g_n = draw(P, specs, seed, gpu, shared=True), draw(n, [s for s, f in zip(specs, is_f) if f], seed + 1, gpu)
    ys, g_P = draw(n, specs, seed + 2, gpu), draw(P, [s for s, f in zip(specs, is_f) if f], seed + 3, gpu, shared=True)
    for fused, torch_op, src, ups in ((sel.gather, lambda x: x[mask], xs, g_n),
                                      (sel.scatter, lambda y: torch.zeros((P,) + tuple(y.shape[1:]), dtype=y.dtype, device=gpu).index_copy(0, idx, y), ys, g_P)):
        a = [x.clone().requires_grad_(f) for x, f in zip(src, is_f)]
        b = [x.clone().requires_grad_(f) for x, f in zip(src, is_f)]
        got, want = fused(*a), [torch_op(x) for x in b]
        assert len(got) == len(want)
        for o, w, f in zip(got, want, is_f):
            assert o.shape == w.shape and o.dtype == w.dtype and o.is_contiguous() and torch.equal(o, w) and o.requires_grad == f
        torch.autograd.backward([o for o, f in zip(got, is_f) if f], ups)
        torch.autograd.backward([w for w, f in zip(want, is_f) if f], ups)
        for x, r, f in zip(a, b, is_f):
            assert (x.grad is None and not f) or (x.grad.shape == x.shape and torch.equal(x.grad, r.grad))


@pytest.mark.parametrize("name", sm.PATTERNS)
@pytest.mark.parametrize("P", SIZES)
def test_primitives_equal_torch_indexing_bit_for_bit(P, name, gpu):
    keep = sm.pattern(name, P, seed=P)
    sel, mask = selection(keep, gpu, sm.PATTERNS.index(name) % 4)
    n = int(keep.sum())
    assert (sel.P, sel.count, sel.device) == (P, n, mask.device)
    assert sel.rows.dtype == torch.int32 and tuple(sel.rows.shape) == (n,) and torch.equal(sel.rows, mask.nonzero().reshape(-1).to(torch.int32))
    assert np.array_equal(sel.rows.cpu().numpy(), sm.rows(keep))
    assert sel.mask.dtype == torch.bool and torch.equal(sel.mask, mask)
    check_both_directions(sel, mask, SHAPES, 10 * P + 1, gpu)          # seven tensors, every shape, in one call per direction
    if P in (257, 70001):
        check_both_directions(sel, mask, SIXTEEN, 10 * P + 5, gpu)     # sixteen tensors in one call
    torch.cuda.synchronize()


def poison_case(gpu):
    P = 4099
    keep = sm.pattern("random", P, seed=3)
    sel, mask = selection(keep, gpu, 0)
    return P, int(keep.sum()), sel, mask


def test_poisoned_source_rows_are_never_read(gpu):
    """NaN / Inf on the rows the selection drops: the gather, and the gradient a scatter's backward gathers, stay finite."""
    P, n, sel, mask = poison_case(gpu)
    x = torch.randn(P, 48, device=gpu)
    x[~mask] = float("nan")
    x[(~mask).nonzero().reshape(-1)[::2]] = float("inf")
    x.requires_grad_(True)
    y, = sel.gather(x)
    assert torch.isfinite(y).all() and torch.equal(y, x.detach()[mask])
    y.backward(torch.randn(n, 48, device=gpu))
    assert torch.isfinite(x.grad).all() and not x.grad[~mask].any()
    r = torch.randn(n, 7, device=gpu, requires_grad=True)
    z, = sel.scatter(r)
    g = torch.randn(P, 7, device=gpu)
    g[~mask] = float("nan")
    z.backward(g)
    assert torch.isfinite(r.grad).all() and torch.equal(r.grad, g[mask])


def test_scatter_writes_positive_zero_over_whatever_the_buffer_held(gpu):
    """The rows a scatter does not select are +0.0 bit for bit (the sign bit too), over an output block that just held NaN, and so are the
    rows of a gather's backward."""
    P, n, sel, mask = poison_case(gpu)
    for w in (1, 3, 64):
        y, x, g = torch.randn(n, w, device=gpu) - 5.0, torch.randn(P, w, device=gpu, requires_grad=True), torch.randn(n, w, device=gpu)
        junk = torch.full((P, w), float("nan"), device=gpu)
        del junk                                             # (the caching allocator hands the next request of this size the same block)
        z, = sel.scatter(y)
        assert not z.view(torch.int32)[~mask].any() and torch.isfinite(z).all() and (z[mask] != 0).all()
        out, = sel.gather(x)
        junk = torch.full((P, w), -0.0, device=gpu)
        del junk
        out.backward(g)
        assert not x.grad.view(torch.int32)[~mask].any()
    none, _ = selection(sm.pattern("none", 300), gpu, 1)
    y = torch.empty(0, 5, device=gpu)
    junk = torch.full((300, 5), float("nan"), device=gpu)
    del junk
    z, = none.scatter(y)         # n_kept = 0: every row is zero-filled
    assert tuple(z.shape) == (300, 5) and not z.view(torch.int32).any()


def test_autograd_behaviour(gpu):
    P, n, sel, mask = poison_case(gpu)
    idx = mask.nonzero().reshape(-1)
    a0, b0, r0 = torch.randn(P, 3, device=gpu), torch.randn(P, 9, device=gpu), torch.randn(n, 7, device=gpu)
    ga, gb = torch.randn(n, 3, device=gpu), torch.randn(n, 9, device=gpu)
    want_a = torch.zeros(P, 3, device=gpu).index_copy(0, idx, ga)
    # requires_grad combinations: only the inputs that need a gradient get one
    for need_a, need_b in ((True, False), (False, True), (True, True)):
        a, b = a0.clone().requires_grad_(need_a), b0.clone().requires_grad_(need_b)
        oa, ob = sel.gather(a, b)
        torch.autograd.backward((oa, ob), (ga, gb))
        assert (a.grad is None) == (not need_a) and (b.grad is None) == (not need_b)
        if need_a:
            assert torch.equal(a.grad, want_a)
    a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    ia = torch.arange(P, dtype=torch.int32, device=gpu)
    oa, ob, oi = sel.gather(a, b, ia)
    assert oa.requires_grad and not oi.requires_grad and oi.grad_fn is None and torch.equal(oi, sel.rows)
    oa.backward(ga)                                           # ob is unused upstream: no launch for it, no gradient
    assert b.grad is None and torch.equal(a.grad, want_a)
    # nothing requires a gradient, and no_grad: plain tensors
    assert all(o.grad_fn is None and not o.requires_grad for o in sel.gather(a0, b0) + sel.scatter(r0))
    with torch.no_grad():
        outs = sel.gather(a, b) + sel.scatter(r0.clone().requires_grad_(True))
    assert all(o.grad_fn is None and not o.requires_grad for o in outs) and torch.equal(outs[0], a0[mask])
    # a non-contiguous upstream gradient, in both directions
    g_nc = torch.randn(3, n, device=gpu).t()
    assert not g_nc.is_contiguous()
    a = a0.clone().requires_grad_(True)
    sel.gather(a)[0].backward(g_nc)
    assert torch.equal(a.grad, torch.zeros(P, 3, device=gpu).index_copy(0, idx, g_nc))
    g_nc = torch.randn(7, P, device=gpu).t()
    r = r0.clone().requires_grad_(True)
    sel.scatter(r)[0].backward(g_nc)
    assert torch.equal(r.grad, g_nc[mask])
    # a double backward raises, in both directions
    for fn, src, rows_out in ((sel.gather, a0, n), (sel.scatter, torch.randn(n, 3, device=gpu), P)):
        x = src.clone().requires_grad_(True)
        out, = fn(x)
        up = torch.ones(rows_out, 3, device=gpu, requires_grad=True)
        (g,) = torch.autograd.grad(out, x, up, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
            g.sum().backward()
    # two runs are bit-equal, and one selection serves any number of calls in any order
    import fused_densify as fd
    again = fd.select_rows(keep=mask)
    first = sel.gather(a0, b0) + sel.scatter(r0)
    second = again.scatter(r0) + again.gather(a0, b0)
    third = sel.gather(a0, b0) + sel.scatter(r0)
    for x, y, z in zip(first, second[1:] + second[:1], third):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert torch.equal(sel.scatter(sel.gather(a0)[0])[0], a0 * mask[:, None])      # scatter after gather: the rows kept, zeros elsewhere
    # the refusals with tensors on the device
    with pytest.raises(RuntimeError, match="at most 16"):
        sel.gather(*[a0] * 17)
    with pytest.raises(RuntimeError, match="float32 or int32"):
        sel.gather(a0.double())
    with pytest.raises(RuntimeError, match=f"expected {n} rows"):
        sel.scatter(a0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sel.gather(a0.cpu())


# ---- temporal_rows --------------------------------------------------------------------------------------------------------------
def placed_case(P, pattern, t, ms):
    """tests/test_gpu_temporal.py's placement (test_select_equals_mask_indexing_bit_for_bit): no state within 1e-6 of the threshold, at most
    0.1 % of the rows moved to achieve that.  Returns (the case, head, center, the fp64 gate)."""
    c, _ = tm.make_case(P, t, seed=20 + P)
    rng = np.random.default_rng(P)
    head, center = c["head"].copy(), c["center"].copy()
    if pattern != "random":
        alive = sm.pattern(pattern, P)
        L = (1 - ms) * (1 - head.astype(np.float64)) + ms
        center = np.where(alive, t + 0.3 * L * rng.uniform(-1, 1, P), t + 2.0).astype(np.float32)      # state >= 0.69, or <= e^-16
    band = np.abs(tm.gate(head, center, t, ms)["state"] - 0.001) <= 1e-6
    assert band.sum() <= 0.001 * P
    center[band] = t
    return c, head, center, tm.gate(head, center, t, ms)


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "runs300", "random"])
@pytest.mark.parametrize("P", [0, 1, 257, 4099])
def test_temporal_rows_mask_is_the_fp64_mask_and_its_tensors_are_the_gates(P, pattern, gpu):
    import fused_temporal as ft
    t, ms = 0.37, 0.01
    c, head, center, want = placed_case(P, pattern, t, ms)
    up = [torch.tensor(c[k], device=gpu).reshape(-1, 1) for k in ("d_lifespan", "d_state")]
    results = []
    for fn in ("gate", "rows"):
        h = torch.tensor(head, device=gpu).reshape(-1, 1).requires_grad_(True)
        p = torch.tensor(center, device=gpu).reshape(-1, 1).requires_grad_(True)
        if fn == "gate":
            out = ft.temporal_gate(h, p, t, min_scale=ms)
        else:
            sel, *out = ft.temporal_rows(h, p, t, min_scale=ms)
        assert out[2].requires_grad is False and out[0].requires_grad and out[1].requires_grad
        torch.autograd.backward(out[:2], up)
        results.append([o.detach() for o in out] + [h.grad, p.grad])
    for a, b in zip(*results):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    alive = ~want["dead"]
    assert sel.P == P and sel.count == int(alive.sum()) and np.array_equal(sel.mask.cpu().numpy(), alive)
    assert np.array_equal(sel.rows.cpu().numpy(), sm.rows(alive))
    if pattern in ("all", "none"):
        assert sel.count == (P if pattern == "all" else 0)
    # the caller's own cull is OR-ed in, as bool [P] and as uint8 [P, 1]
    cull = np.arange(P) % 3 == 0
    h, p = torch.tensor(head, device=gpu).reshape(-1, 1), torch.tensor(center, device=gpu).reshape(-1, 1)
    for also in (torch.from_numpy(cull).to(gpu), (torch.from_numpy(cull).to(gpu).to(torch.uint8) * 7).reshape(-1, 1)):
        sel2, _, state2, _ = ft.temporal_rows(h, p, t, min_scale=ms, also_dead=also)
        assert np.array_equal(sel2.mask.cpu().numpy(), alive & ~cull) and sel2.count == int((alive & ~cull).sum())
        assert torch.equal(state2, results[0][1])
    # another threshold moves the mask with it
    if P:
        sel3 = ft.temporal_rows(h, p, t, min_scale=ms, threshold=0.5)[0]
        far = np.abs(want["state"] - 0.5) > 1e-6             # (fp32's state is within a few 1e-7 of the fp64 one)
        assert np.array_equal(sel3.mask.cpu().numpy()[far], (want["state"] > 0.5)[far]) and far.sum() >= 0.999 * P


# ---- end to end -----------------------------------------------------------------------------------------------------------------
class _Heads(nn.Module):
    """The four heads at the reference's shipped widths (scene/saro_gaussian.py:104-110)."""

    def __init__(self):
        super().__init__()
        seq = lambda i, h2, o, sig: nn.Sequential(*([nn.Linear(i, 128), nn.ReLU(), nn.Linear(128, h2), nn.ReLU(), nn.Linear(h2, o)] + ([nn.Sigmoid()] if sig else [])))  # noqa: E731
        self.motion_mlp, self.rot_mlp, self.shs_mlp, self.opacity_mlp = seq(41, 128, 3, False), seq(41, 128, 7, False), seq(41, 128, 48, False), seq(32, 64, 1, True)


LEAVES = ("xyz", "rotation", "scaling", "opacity", "f_dc", "f_rest")
COMPARED = ("image", "temporal_pos", "opacity_mlp.0.weight", "motion_mlp.0.weight", "xyz")


def test_end_to_end_heads_on_alive_rows_and_everything_compact(scenes, rast, gpu):
    """tests/test_gpu_temporal.py's end-to-end chain (feature -> opacity head -> gate -> three heads -> activate_gaussians -> GaussianRasterizer ->
    l1_dssim_loss -> backward, P = 500 on 64 x 48) with about half the rows dead at the view's time (state <= e^-16; the others >= 0.69), three
    times through the fused kernels: on all rows ("full"), pattern (A) -- the three heads on the alive rows, their residuals scattered -- and
    pattern (B) -- heads, epilogue and rasterizer on the alive rows.  (A) and (B) against "full" within this file's bar; every leaf gradient
    exactly 0 on the dead rows in all three; (B)'s scattered radii equal the full chain's on the alive rows.
    The figures are printed per tensor before the assertion."""
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
    raw0 = dict(xyz=f(sc["means3D"]), rotation=f(sc["rotations"]), scaling=f(np.log(sc["scales"])), opacity=f(np.log(o / (1 - o))),
                f_dc=f(sc["shs"][:, :1]), f_rest=f(sc["shs"][:, 1:16]))
    alive_np = rng.random(P) < 0.5
    # lifespan >= min_scale = 0.3 and <= 1 whatever the head says: |d| <= 0.09 gives state >= exp(-4 * 0.3^2) > 0.69, d = 2 gives state <= e^-16
    pos_np = np.where(alive_np, t + 0.09 * rng.uniform(-1, 1, P), t + 2.0)
    feat0, pos0, gt = f(rng.standard_normal((P, 32)) * 0.5), f(pos_np.reshape(P, 1)), f(rng.uniform(0, 1, (3, H, W)))
    alive = torch.from_numpy(alive_np).to(gpu)
    torch.manual_seed(79)
    init = _Heads().state_dict()

    def chain(kind):
        heads = _Heads()
        heads.load_state_dict(init)
        heads = heads.to(gpu)
        pos = pos0.clone().requires_grad_(True)
        raw = {k: v.clone().requires_grad_(True) for k, v in raw0.items()}
        feat, src, n, sel = feat0, raw, P, None
        if kind == "fp64":
            heads = heads.double()
            head = heads.opacity_mlp(feat0.double())
            _, state, emb = tm.torch_gate(head, pos.double(), t, ms, 4)
            hin = torch.cat((feat0.double(), emb), 1)
            motion, rot, shs, state = heads.motion_mlp(hin).float(), heads.rot_mlp(hin).float(), heads.shs_mlp(hin).float(), state.float()
        else:
            assert fused_mlp.convert_heads(heads) == list(fused_mlp.HEAD_NAMES)
            head = heads.opacity_mlp(feat0)
            if kind == "full":
                _, state, emb = ft.temporal_gate(head, pos, t, min_scale=ms)
            else:
                sel, _, state, emb = ft.temporal_rows(head, pos, t, min_scale=ms)
                assert torch.equal(sel.mask, alive)
                if kind == "A":
                    feat, emb = sel.gather(feat0, emb)
                else:
                    n = sel.count
                    feat, emb, state, *moved = sel.gather(feat0, emb, state, *[raw[k] for k in LEAVES])
                    src = dict(zip(LEAVES, moved))
            motion, rot, shs = heads.motion_mlp(feat, emb), heads.rot_mlp(feat, emb), heads.shs_mlp(feat, emb)
            if kind == "A":
                motion, rot, shs = sel.scatter(motion, rot, shs)      # zero residual on the dead rows, which do not render
        means3D, rots, scales, opac, sh = fused_epilogue.activate_gaussians(
            src["xyz"], src["rotation"], src["scaling"], src["opacity"], src["f_dc"], src["f_rest"], motion_residual=0.05 * motion,
            rot_residual=0.1 * rot, trbfoutput=state, shs_residual=0.1 * shs.reshape(n, 16, 3))
        m2 = torch.zeros((n, 3), device=gpu, requires_grad=True)
        color, radii = rast.GaussianRasterizer(rs)(means3D=means3D, means2D=m2, opacities=opac, shs=sh, scales=scales, rotations=rots)[:2]
        if kind == "B":
            radii, = sel.scatter(radii)
        fused_loss.l1_dssim_loss(color, gt, 0.2).backward()
        torch.cuda.synchronize()
        params = dict(heads.named_parameters())
        out = {"image": color.detach(), "temporal_pos": pos.grad, "opacity_mlp.0.weight": params["opacity_mlp.0.weight"].grad,
               "motion_mlp.0.weight": params["motion_mlp.0.weight"].grad, "radii": radii}
        out.update({k: raw[k].grad for k in LEAVES})
        assert all(v is not None for v in out.values()), kind
        return {k: (v.double().cpu().numpy() if k != "radii" else v.cpu().numpy()) for k, v in out.items()}

    truth, full, got_a, got_b = chain("fp64"), chain("full"), chain("A"), chain("B")
    dead = ~alive_np
    assert 0.4 * P < dead.sum() < 0.6 * P
    for name, got in (("full", full), ("A", got_a), ("B", got_b)):
        assert float(np.abs(got["image"]).max()) > 0.1, name
        for k in LEAVES + ("temporal_pos",):
            assert got[k].shape[0] == P and np.isfinite(got[k]).all() and not got[k][dead].any(), (name, k)      # exactly zero on the dead rows
            assert np.abs(got[k]).max() > 0, (name, k)
    assert (full["radii"][alive_np] > 0).any() and np.array_equal(got_b["radii"][alive_np], full["radii"][alive_np]) and not got_b["radii"][dead].any()
    # (A): the rasterizer still sees P rows; a dead row's radius is that of its undeformed Gaussian (zero residuals), so only the alive rows' are pinned
    assert got_a["radii"].shape == (P,) and np.array_equal(got_a["radii"][alive_np], full["radii"][alive_np])
    bad = []
    for name, got in (("A", got_a), ("B", got_b)):
        for k in COMPARED:
            assert np.abs(truth[k]).max() > 0, k
            diff = float(np.abs(got[k] - full[k]).max())
            bound = 4 * float(np.abs(full[k] - truth[k]).max()) + ULP * float(np.abs(truth[k]).max())
            print(f"end to end ({name}) {k}: |selected - full| {diff:.3e}  bar {bound:.3e}  max|truth| {np.abs(truth[k]).max():.3e}")
            if not diff <= bound:
                bad.append((name, k, diff, bound))
    assert not bad, bad
