"""-m gpu: the bf16 path of the fused 3-layer head (csrc/gsrast_mlp_bf16.h, fused_mlp.py precision="bf16") against the rounding model
restated in tests/mlp_bf16_math.py.

1. Exact cases.  Dyadic inputs (mlp_bf16_math.make_dyadic_case, which asserts what makes them exact) make every product and every
   partial sum representable in fp32, so neither the summation order nor the accumulator's width can show and every rounding sees the
   same input as the model's: the GPU must give the fp64 model's VALUES on every output and gradient, no tolerance (+0 and -0 are one
   value).  All seven shapes run without their Sigmoid.  One assumption is unmeasured before this test: that the matrix instruction is
   exact on exactly representable sums.
2. Generic floats (mlp_math.make_case), all shapes, the sigmoid heads included.  Per tensor T
       r = |T_gpu - T_model|_2 / |T_model|_2   against the model with fp64 accumulation,       r <= 4 R + 2^-23,
   R = the largest r of the model itself evaluated with fp32 accumulation, over 8 random k orders, all tensors and all row counts of the
   shape -- computed here.  The only legitimate differences are the fp32 summation order and the rare bf16 rounding or ReLU decision it
   flips; those are Poisson-rare per case, hence the pooling.  The factor 4 is the project's margin for another summation order.
3. Behaviour: fp32 through the new calls keeps the existing path's bits, run-to-run bits, requires_grad combinations, the tail, NaN rows,
   refusals, no_grad, unaligned parameters, convert_heads, one end-to-end step."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from torch import nn

import mlp_bf16_math as bm
import mlp_math as mm

pytestmark = pytest.mark.gpu

HEADS = [(32, 9, 128, 128, 3, False), (32, 9, 128, 128, 7, False), (32, 9, 128, 128, 48, False), (32, 0, 128, 64, 1, True)]
CORNERS = [(1, 0, 32, 32, 1, False), (64, 0, 128, 128, 64, False), (5, 3, 96, 32, 17, True)]
SHAPES = HEADS + CORNERS
ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 513, 1000, 4099]
ULP = 2.0 ** -23
GRADS = ("dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")
_sid = lambda s: "-".join(str(int(v)) for v in s)  # noqa: E731


def dev_inputs(c, gpu):
    return {k: (None if v is None else torch.tensor(v, device=gpu)) for k, v in c.items()}


def run_module(c, sigmoid, gpu, precision="bf16", need_x=True, need_w=True, workgroups=0):
    """Through fused_mlp3."""
    import fused_mlp
    t = dev_inputs(c, gpu)
    t["x"].requires_grad_(need_x)
    for k in PARAMS:
        t[k].requires_grad_(need_w)
    y = fused_mlp.fused_mlp3(t["x"], *[t[k] for k in PARAMS], x_tail=t["x_tail"], sigmoid_out=sigmoid, precision=precision, workgroups=workgroups)
    if need_x or need_w:
        y.backward(t["dy"])
    torch.cuda.synchronize()
    out = dict(y=y.detach().cpu().numpy())
    for k, name in zip(("x",) + PARAMS, GRADS):
        if t[k].grad is not None:
            out[name] = t[k].grad.cpu().numpy()
    return out


def run_raw(rast, shape, sigmoid, c, gpu, workgroups, precision=1, want=GRADS, old_calls=False):
    """Through the C ABI with an explicit workgroup count: the _p calls, or (old_calls) the calls without a precision."""
    _C = rast._C
    L = _C.lib()
    d_x, d_tail, h1, h2, d_out = shape[:5]
    t = dev_inputs(c, gpu)
    n = int(t["x"].shape[0])
    y = torch.empty((n, d_out), device=gpu)
    shapes = dict(dx=(n, d_x), dw1=(h1, d_x + d_tail), db1=(h1,), dw2=(h2, h1), db2=(h2,), dw3=(d_out, h2), db3=(d_out,))
    g = {k: torch.full(shapes[k], float("nan"), device=gpu) for k in want}
    d = _C.Mlp3Struct(n, d_x, d_tail, h1, h2, d_out, int(sigmoid))
    for k in ("x", "x_tail") + PARAMS + ("dy",):
        if t[k] is not None and t[k].numel():
            setattr(d, k, t[k].data_ptr())
    d.y = y.data_ptr() if n else None
    for k, v in g.items():
        setattr(d, k, v.data_ptr() if v.numel() else None)
    s = torch.cuda.current_stream(gpu).cuda_stream
    if old_calls:
        scratch = torch.empty(L.gsrast_mlp3_scratch_bytes(C.byref(d), workgroups), dtype=torch.uint8, device=gpu)
        assert L.gsrast_mlp3_forward(C.byref(d), workgroups, s) == 0, L.gsrast_last_error()
        assert L.gsrast_mlp3_backward(C.byref(d), workgroups, scratch.data_ptr(), s) == 0, L.gsrast_last_error()
    else:
        scratch = torch.empty(L.gsrast_mlp3_scratch_bytes_p(C.byref(d), precision, workgroups), dtype=torch.uint8, device=gpu)
        assert scratch.numel() > 0
        assert L.gsrast_mlp3_forward_p(C.byref(d), precision, workgroups, s) == 0, L.gsrast_last_error()
        assert L.gsrast_mlp3_backward_p(C.byref(d), precision, workgroups, scratch.data_ptr(), s) == 0, L.gsrast_last_error()
    torch.cuda.synchronize()
    out = dict(y=y.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in g.items()})
    return out


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


# ---- 1. exact cases ----------------------------------------------------------------------------------------------------------------
def dyadic(shape, n):
    return bm.make_dyadic_case(*shape[:5], n, seed=1000 + 7 * n + shape[4])


def check_exact(label, got, model):
    bad = []
    for k, g in got.items():
        want = np.asarray(model[k], np.float64)
        assert g.shape == want.shape and g.dtype == np.float32, (label, k)
        wrong = ~(g.astype(np.float64) == want)      # (a NaN is wrong; +0 == -0)
        if wrong.any():
            at = tuple(int(v) for v in np.argwhere(wrong)[0])
            bad.append((k, int(wrong.sum()), at, float(g[at]), float(want[at])))
    assert not bad, (label, bad)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_exact_cases_through_the_module(shape, n, gpu):
    c, model = dyadic(shape, n)
    got = run_module(c, False, gpu)
    assert set(got) == set(("y",) + GRADS)
    check_exact(f"{_sid(shape)} N={n}", got, model)


@pytest.mark.parametrize("workgroups", [1, 2, 3])
@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_exact_cases_few_workgroups_many_tiles_each(shape, n, workgroups, rast, gpu):
    """Several tiles per workgroup and several launches per call, a ragged last tile, a reduction over more than one partial."""
    c, model = dyadic(shape, n)
    check_exact(f"{_sid(shape)} N={n} wg={workgroups}", run_raw(rast, shape, False, c, gpu, workgroups), model)


# ---- 2. generic floats ---------------------------------------------------------------------------------------------------------------
_generic = {}


def l2_err(got, truth):
    truth = np.asarray(truth, np.float64)
    scale = float(np.sqrt((truth ** 2).sum()))
    return float(np.sqrt(((np.asarray(got, np.float64).reshape(truth.shape) - truth) ** 2).sum())) / scale if scale > 0 else 0.0


def generic(shape):
    """Per shape, once: the inputs and the fp64-accumulated model of every row count, and R (this file's docstring)."""
    if shape in _generic:
        return _generic[shape]
    d_x, d_tail, h1, h2, d_out, sig = shape
    cases = {n: mm.make_case(d_x, d_tail, h1, h2, d_out, n, seed=2000 + 7 * n + d_out) for n in ROWS}
    args = lambda c: (c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], sig)  # noqa: E731
    models = {n: bm.forward_backward(*args(c), acc="fp64") for n, c in cases.items()}

    def one_order(o):
        rng = np.random.default_rng(9000 + o)
        worst = 0.0
        for n, c in cases.items():
            m32 = bm.forward_backward(*args(c), acc="fp32", order=rng)
            worst = max([worst] + [l2_err(m32[k], models[n][k]) for k in bm.NAMES])
        return worst

    with ThreadPoolExecutor(8) as pool:      # (numpy releases the interpreter in its loops)
        R = max(pool.map(one_order, range(8)))
    for d in list(cases.values()) + list(models.values()):
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
    _generic[shape] = (cases, models, R)
    return _generic[shape]


def check_generic(label, got, model, R):
    bad = []
    for k, g in got.items():
        g = np.asarray(g)
        assert g.shape == model[k].shape and np.isfinite(g).all(), (label, k)
        if not np.abs(model[k]).max(initial=0.0) > 0:
            assert not g.any(), (label, k, "must be exactly zero")
            continue
        r = l2_err(g, model[k])
        print(f"{label} {k}: r {r:.3e}  R {R:.3e}  bar {4 * R + ULP:.3e}")
        if not r <= 4 * R + ULP:
            bad.append((k, r))
    assert not bad, (label, R, bad)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_generic_floats_against_the_model(shape, n, gpu):
    cases, models, R = generic(shape)
    check_generic(f"{_sid(shape)} N={n}", run_module(cases[n], shape[5], gpu), models[n], R)


# ---- 3. behaviour -----------------------------------------------------------------------------------------------------------------
def test_fp32_through_the_new_calls_keeps_the_existing_bits(rast, gpu):
    for shape in (HEADS[2], HEADS[3]):
        c = generic(shape)[0][1000]
        for wg in (0, 2):
            old = run_raw(rast, shape, shape[5], c, gpu, wg, old_calls=True)
            assert same_bits(old, run_raw(rast, shape, shape[5], c, gpu, wg, precision=0)), (shape, wg)
        assert same_bits(run_raw(rast, shape, shape[5], c, gpu, 0, old_calls=True), run_module(c, shape[5], gpu, precision="fp32")), shape
        # and bf16 is another computation: the option is not ignored
        assert not np.array_equal(run_module(c, shape[5], gpu, precision="bf16")["y"], old["y"])


def test_bit_identical_from_run_to_run(rast, gpu):
    shape = HEADS[2]
    c = generic(shape)[0][4099]
    a, b = run_module(c, False, gpu), run_module(c, False, gpu)
    assert set(a) == set(("y",) + GRADS) and same_bits(a, b)
    r1, r2 = run_raw(rast, shape, False, c, gpu, 2), run_raw(rast, shape, False, c, gpu, 2)
    assert same_bits(r1, r2)
    # y and dx are per row: they do not depend on the workgroup count at all
    assert np.array_equal(a["y"].view(np.uint32), r1["y"].view(np.uint32)) and np.array_equal(a["dx"].view(np.uint32), r1["dx"].view(np.uint32))


@pytest.mark.parametrize("shape", [HEADS[2], HEADS[3]], ids=_sid)
def test_requires_grad_combinations(shape, rast, gpu):
    cases, models, R = generic(shape)
    c, model = cases[1000], models[1000]
    full = run_module(c, shape[5], gpu)
    no_dx = run_module(c, shape[5], gpu, need_x=False)
    assert "dx" not in no_dx and all(np.array_equal(no_dx[k], full[k]) for k in no_dx)
    frozen = run_module(c, shape[5], gpu, need_w=False)
    assert set(frozen) == {"y", "dx"} and np.array_equal(frozen["dx"], full["dx"])
    # one layer's parameters only, through the C ABI: the others' pointers are NULL and nothing is written for them
    for want in (("dw2", "db2"), ("db3",), ("dw1",), ("dx", "dw3")):
        part = run_raw(rast, shape, shape[5], c, gpu, 0, want=want)
        assert set(part) == set(("y",) + want)
        check_generic(f"{_sid(shape)} want={want}", part, model, R)
        assert all(np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)) for k in part), want


def test_tail_equals_the_explicit_cat_bit_for_bit(gpu):
    import fused_mlp
    for shape in (HEADS[2], CORNERS[2]):
        t = dev_inputs(generic(shape)[0][1000], gpu)
        p = [t[k].requires_grad_(True) for k in PARAMS]
        a = fused_mlp.fused_mlp3(t["x"], *p, x_tail=t["x_tail"], sigmoid_out=shape[5], precision="bf16")
        a.backward(t["dy"])
        ga = [q.grad.clone() for q in p]
        for q in p:
            q.grad = None
        b = fused_mlp.fused_mlp3(torch.cat((t["x"], t["x_tail"]), 1), *p, sigmoid_out=shape[5], precision="bf16")
        b.backward(t["dy"])
        assert torch.equal(a, b) and all(torch.equal(u, q.grad) for u, q in zip(ga, p))


def test_a_nan_row_stays_in_its_row(gpu):
    import fused_mlp
    shape = HEADS[0]
    t = dev_inputs(generic(shape)[0][129], gpu)
    p = [t[k] for k in PARAMS]
    clean = fused_mlp.fused_mlp3(t["x"], *p, x_tail=t["x_tail"], precision="bf16")
    x = t["x"].clone()
    x[70, 3] = float("nan")
    y = fused_mlp.fused_mlp3(x, *p, x_tail=t["x_tail"], precision="bf16")
    keep = torch.arange(129, device=gpu) != 70
    assert torch.isnan(y[70]).all() and torch.equal(y[keep], clean[keep])


def test_tensors_on_another_device_and_a_double_backward_raise(gpu):
    import fused_mlp
    t = dev_inputs(generic(HEADS[0])[0][33], gpu)
    for on_cpu in PARAMS + ("x_tail",):
        args = {k: (t[k].cpu() if k == on_cpu else t[k]) for k in PARAMS + ("x_tail",)}
        with pytest.raises(RuntimeError, match=on_cpu + " is on cpu"):
            fused_mlp.fused_mlp3(t["x"], *[args[k] for k in PARAMS], x_tail=args["x_tail"], precision="bf16")
    x = t["x"].clone().requires_grad_(True)
    y = fused_mlp.fused_mlp3(x, *[t[k] for k in PARAMS], x_tail=t["x_tail"], precision="bf16")
    dy = t["dy"].clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        gx.sum().backward()
    assert dy.grad is None


def test_no_grad_forward(gpu):
    import fused_mlp
    shape = HEADS[2]
    c = generic(shape)[0][1000]
    t = dev_inputs(c, gpu)
    for k in PARAMS:
        t[k].requires_grad_(True)
    with torch.no_grad():
        y = fused_mlp.fused_mlp3(t["x"], *[t[k] for k in PARAMS], x_tail=t["x_tail"], precision="bf16")
    torch.cuda.synchronize()
    assert y.requires_grad is False and y.grad_fn is None
    assert np.array_equal(y.cpu().numpy(), run_module(c, False, gpu)["y"])


def test_parameters_at_odd_float_offsets_of_a_flat_buffer(gpu):
    """Parameters that are views into one flat buffer at offsets that are no multiple of 16 bytes: the bits of aligned parameters."""
    import fused_mlp
    for shape in (HEADS[2], CORNERS[1]):
        t = dev_inputs(generic(shape)[0][1000], gpu)
        flat = torch.zeros(sum(t[k].numel() + 8 for k in PARAMS) + 8, device=gpu)
        views, at = [], 1
        for k in PARAMS:
            v = flat[at:at + t[k].numel()].view_as(t[k])
            v.copy_(t[k])
            assert v.data_ptr() % 16 != 0 and v.is_contiguous()
            views.append(v.requires_grad_(True))
            at = (at + t[k].numel() + 3) // 4 * 4 + 1
        aligned = [t[k].clone().requires_grad_(True) for k in PARAMS]
        xa, xb = t["x"].clone().requires_grad_(True), t["x"].clone().requires_grad_(True)
        ya = fused_mlp.fused_mlp3(xa, *views, x_tail=t["x_tail"], sigmoid_out=shape[5], precision="bf16")
        yb = fused_mlp.fused_mlp3(xb, *aligned, x_tail=t["x_tail"], sigmoid_out=shape[5], precision="bf16")
        ya.backward(t["dy"])
        yb.backward(t["dy"])
        torch.cuda.synchronize()
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
        for v, a in zip(views, aligned):
            assert torch.equal(v.grad, a.grad)


class _Heads(nn.Module):
    """The four heads at the reference's shipped widths."""

    def __init__(self):
        super().__init__()
        seq = lambda i, h2, o, sig: nn.Sequential(*([nn.Linear(i, 128), nn.ReLU(), nn.Linear(128, h2), nn.ReLU(), nn.Linear(h2, o)] + ([nn.Sigmoid()] if sig else [])))  # noqa: E731
        self.motion_mlp, self.rot_mlp, self.shs_mlp, self.opacity_mlp = seq(41, 128, 3, False), seq(41, 128, 7, False), seq(41, 128, 48, False), seq(32, 64, 1, True)


def test_convert_heads_bf16_equals_the_function(gpu):
    import fused_mlp
    torch.manual_seed(5)
    heads = _Heads().to(gpu)
    assert fused_mlp.convert_heads(heads, precision="bf16") == list(fused_mlp.HEAD_NAMES)
    feat, temb = torch.randn(777, 32, device=gpu), torch.randn(777, 9, device=gpu)
    for name in fused_mlp.HEAD_NAMES:
        m = getattr(heads, name)
        assert m.precision == "bf16"
        tail = None if name == "opacity_mlp" else temb
        l1, l2, l3 = m._modules["0"], m._modules["2"], m._modules["4"]
        want = fused_mlp.fused_mlp3(feat, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, x_tail=tail, sigmoid_out=m.sigmoid_out, precision="bf16")
        assert torch.equal(m(feat, tail), want), name
        other = fused_mlp.fused_mlp3(feat, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, x_tail=tail, sigmoid_out=m.sigmoid_out)
        assert not torch.equal(want, other), name


def test_end_to_end_field_bf16_heads_rasterizer_loss(scenes, rast, gpu):
    """fused_hexplane field -> the four heads in bf16 -> GaussianRasterizerRaw with the residuals -> l1_dssim_loss -> backward:
    a finite loss and a finite, non-zero gradient on every leaf."""
    from conftest import settings_from
    import fused_hexplane
    import fused_loss
    import fused_mlp
    P, W, H = 500, 64, 64
    sc = scenes.synth(P, 77, sh_degree=3)
    cam = scenes.camera(0, 1, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    rng = np.random.default_rng(78)
    f = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=gpu)  # noqa: E731
    raw = dict(xyz=f(sc["means3D"]), rotation=f(sc["rotations"]), scaling=f(np.log(sc["scales"])),
               opacity=f(np.log(sc["opacities"].clip(1e-4, 1 - 1e-4) / (1 - sc["opacities"].clip(1e-4, 1 - 1e-4)))),
               f_dc=f(sc["shs"][:, :1]), f_rest=f(sc["shs"][:, 1:16]))
    planes = [[torch.tensor(rng.normal(size=(1, 32, 25 if b == 3 else 32, 25 if a == 3 else 32)).astype(np.float32) * 0.5, device=gpu, requires_grad=True)
               for (a, b) in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))]]
    pts, levels = f(rng.uniform(0, 1, size=(P, 4))), f(np.concatenate([rng.uniform(0, 5, size=(P, 3)), np.zeros((P, 1))], 1))
    temb = f(rng.standard_normal((P, 9)))
    gt = f(rng.uniform(0, 1, size=(3, H, W)))
    torch.manual_seed(79)
    heads = _Heads().to(gpu)
    assert fused_mlp.convert_heads(heads, precision="bf16") == list(fused_mlp.HEAD_NAMES)
    feat = fused_hexplane.interpolate_ms_features(pts, planes, 2, True, levels, None)
    motion, rot, shs, trbf = heads.motion_mlp(feat, temb), heads.rot_mlp(feat, temb), heads.shs_mlp(feat, temb), heads.opacity_mlp(feat)
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    color = rast.GaussianRasterizerRaw(rs)(raw["xyz"], m2, raw["rotation"], raw["scaling"], raw["opacity"], raw["f_dc"], raw["f_rest"],
                                           motion_residual=0.05 * motion, rot_residual=0.1 * rot, trbfoutput=trbf,
                                           shs_residual=0.1 * shs.reshape(P, 16, 3))[0]
    loss = fused_loss.l1_dssim_loss(color, gt, 0.2)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(loss.detach()) > 0
    leaves = dict(heads.named_parameters())
    leaves.update({f"plane{k}": p for k, p in enumerate(planes[0])})
    assert len(leaves) == 24 + 6
    for name, p in leaves.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
