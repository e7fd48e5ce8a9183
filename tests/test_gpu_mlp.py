"""-m gpu: the fused 3-layer head (csrc/gsrast_mlp.h, fused_mlp.py) against the fp64 restatement of tests/mlp_math.py.

The bar, per output and gradient tensor T, measured per case at run time:
    e(T) = max|T - fp64 restatement| / max|fp64 restatement|,    e_hip <= 4 e_ref + 2^-23,
e_ref = the same quantity for the SAME nn.Sequential evaluated by torch in fp32 on the CPU.  The factor 4 covers the other summation
order (the matrix instruction's k-ordered chain, then the tile-by-tile and workgroup-by-workgroup sums, against torch's blocked sums): the
error of a sum of terms of random sign moves by about that much between orders.  2^-23 is one ulp of fp32 at the tensor's largest entry.
Where the restatement is all zero (N = 0) the result must be exactly zero."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import mlp_math as mm

pytestmark = pytest.mark.gpu

HEADS = [(32, 9, 128, 128, 3, False), (32, 9, 128, 128, 7, False), (32, 9, 128, 128, 48, False), (32, 0, 128, 64, 1, True)]
CORNERS = [(1, 0, 32, 32, 1, False), (64, 0, 128, 128, 64, False), (5, 3, 96, 32, 17, True)]
SHAPES = HEADS + CORNERS
ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 1000, 4099]
ULP = 2.0 ** -23
GRADS = ("dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")
_sid = lambda s: "-".join(str(int(v)) for v in s)  # noqa: E731
_cache = {}


def reference(shape, n):
    """The case's inputs, the fp64 restatement and the torch fp32 CPU nn.Sequential's results: computed once, shared, never written."""
    key = (shape, n)
    if key in _cache:
        return _cache[key]
    d_x, d_tail, h1, h2, d_out, sig = shape
    c = mm.make_case(d_x, d_tail, h1, h2, d_out, n, seed=1000 + 7 * n + d_out)
    f64 = mm.forward_backward(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], sig)
    seq = nn.Sequential(*([nn.Linear(d_x + d_tail, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(), nn.Linear(h2, d_out)] + ([nn.Sigmoid()] if sig else [])))
    with torch.no_grad():
        for lin, w, b in ((seq[0], "w1", "b1"), (seq[2], "w2", "b2"), (seq[4], "w3", "b3")):
            lin.weight.copy_(torch.from_numpy(c[w]))
            lin.bias.copy_(torch.from_numpy(c[b]))
    x = torch.from_numpy(c["x"]).requires_grad_(True)
    y = seq(x if c["x_tail"] is None else torch.cat((x, torch.from_numpy(c["x_tail"])), 1))
    y.backward(torch.from_numpy(c["dy"]))
    t32 = dict(y=y.detach(), dx=x.grad, dw1=seq[0].weight.grad, db1=seq[0].bias.grad, dw2=seq[2].weight.grad, db2=seq[2].bias.grad,
               dw3=seq[4].weight.grad, db3=seq[4].bias.grad)
    t32 = {k: v.numpy() for k, v in t32.items()}
    for d in (c, f64, t32):
        for v in d.values():
            if v is not None:
                v.setflags(write=False)
    _cache[key] = (c, f64, t32)
    return _cache[key]


def rel_err(got, truth):
    truth = np.asarray(truth, np.float64)
    scale = float(np.abs(truth).max(initial=0.0))
    return (float(np.abs(np.asarray(got, np.float64).reshape(truth.shape) - truth).max(initial=0.0)) / scale) if scale > 0 else 0.0


def check(label, got, f64, t32):
    """The bar of this file's docstring on every tensor in `got`; prints both numbers."""
    bad = []
    for k, g in got.items():
        g = np.asarray(g)
        assert g.shape == f64[k].shape and np.isfinite(g).all(), (label, k)
        if not np.abs(f64[k]).max(initial=0.0) > 0:
            assert not g.any(), (label, k, "must be exactly zero")
            continue
        e_ref, e_hip = rel_err(t32[k], f64[k]), rel_err(g, f64[k])
        print(f"{label} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bar {4 * e_ref + ULP:.3e}")
        if e_ref == 0.0:
            if e_hip != 0.0:
                bad.append((k, e_hip, e_ref))
        elif not e_hip <= 4 * e_ref + ULP:
            bad.append((k, e_hip, e_ref))
    assert not bad, (label, bad)


def dev_inputs(c, gpu):
    return {k: (None if v is None else torch.tensor(v, device=gpu)) for k, v in c.items()}


def run_module(shape, c, gpu, need_x=True, need_w=True):
    """Through fused_mlp3 (default workgroup count)."""
    import fused_mlp
    t = dev_inputs(c, gpu)
    t["x"].requires_grad_(need_x)
    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        t[k].requires_grad_(need_w)
    y = fused_mlp.fused_mlp3(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], t["w3"], t["b3"], x_tail=t["x_tail"], sigmoid_out=shape[5])
    if need_x or need_w:
        y.backward(t["dy"])
    torch.cuda.synchronize()
    out = dict(y=y.detach().cpu().numpy())
    for k, name in (("x", "dx"), ("w1", "dw1"), ("b1", "db1"), ("w2", "dw2"), ("b2", "db2"), ("w3", "dw3"), ("b3", "db3")):
        if t[k].grad is not None:
            out[name] = t[k].grad.cpu().numpy()
    return out


def run_raw(rast, shape, c, gpu, workgroups, want=GRADS):
    """Through the C ABI with an explicit workgroup count."""
    _C = rast._C
    L = _C.lib()
    d_x, d_tail, h1, h2, d_out, sig = shape
    t = dev_inputs(c, gpu)
    n = int(t["x"].shape[0])
    y = torch.empty((n, d_out), device=gpu)
    shapes = dict(dx=(n, d_x), dw1=(h1, d_x + d_tail), db1=(h1,), dw2=(h2, h1), db2=(h2,), dw3=(d_out, h2), db3=(d_out,))
    g = {k: torch.full(shapes[k], float("nan"), device=gpu) for k in want}
    d = _C.Mlp3Struct(n, d_x, d_tail, h1, h2, d_out, int(sig))
    for k in ("x", "x_tail", "w1", "b1", "w2", "b2", "w3", "b3", "dy"):
        if t[k] is not None and t[k].numel():
            setattr(d, k, t[k].data_ptr())
    d.y = y.data_ptr() if n else None
    for k, v in g.items():
        setattr(d, k, v.data_ptr() if v.numel() else None)
    scratch = torch.empty(L.gsrast_mlp3_scratch_bytes(C.byref(d), workgroups), dtype=torch.uint8, device=gpu)
    assert scratch.numel() > 0
    s = torch.cuda.current_stream(gpu).cuda_stream
    assert L.gsrast_mlp3_forward(C.byref(d), workgroups, s) == 0, L.gsrast_last_error()
    assert L.gsrast_mlp3_backward(C.byref(d), workgroups, scratch.data_ptr(), s) == 0, L.gsrast_last_error()
    torch.cuda.synchronize()
    out = dict(y=y.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in g.items()})
    return out


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_forward_and_backward_against_fp64(shape, n, gpu):
    c, f64, t32 = reference(shape, n)
    check(f"{_sid(shape)} N={n}", run_module(shape, c, gpu), f64, t32)


@pytest.mark.parametrize("workgroups", [1, 2, 3])
@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_few_workgroups_many_tiles_each(shape, n, workgroups, rast, gpu):
    """Several tiles per workgroup, a ragged last tile, a reduction over more than one partial."""
    c, f64, t32 = reference(shape, n)
    check(f"{_sid(shape)} N={n} wg={workgroups}", run_raw(rast, shape, c, gpu, workgroups), f64, t32)


def _edge_case(gpu, w1, b1, w2, b2, x):
    """32 -> 32 -> 32 -> 1 with chosen first layers, ones behind them; fused against torch on the device and the restatement."""
    import fused_mlp
    f = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu).requires_grad_(True)  # noqa: E731
    p = [f(w1), f(b1), f(w2), f(b2), f(np.ones((1, 32))), f(np.zeros(1))]
    xt = f(x)
    fused_mlp.fused_mlp3(xt, *p).sum().backward()
    torch.cuda.synchronize()
    g = mm.forward_backward(x, w1, b1, w2, b2, np.ones((1, 32)), np.zeros(1), np.ones((len(x), 1)))
    return xt, p, g


def test_relu_at_exactly_zero_passes_no_gradient(gpu):
    """Row 0 has every first-layer pre-activation exactly 0 (x = 0, b1 = 0): no gradient through it, as torch; row 1 is ordinary."""
    w1 = np.linspace(0.5, 2.0, 32 * 4).reshape(32, 4)
    x = np.array([[0.0] * 4, [1.0, 2.0, 3.0, 4.0]])
    xt, p, g = _edge_case(gpu, w1, np.zeros(32), np.ones((32, 32)) / 32, np.ones(32), x)
    assert not xt.grad[0].any() and xt.grad[1].all()
    only_row1 = mm.forward_backward(x[1:], w1, np.zeros(32), np.ones((32, 32)) / 32, np.ones(32), np.ones((1, 32)), np.zeros(1), np.ones((1, 1)))
    assert np.allclose(p[0].grad.cpu().numpy(), only_row1["dw1"], rtol=1e-6, atol=0) and np.allclose(p[0].grad.cpu().numpy(), g["dw1"], rtol=1e-6, atol=0)
    assert np.array_equal(p[1].grad.cpu().numpy(), np.full(32, 1.0, np.float32))      # db1: row 1 alone, 32 x (1 / 32) = 1


def test_all_negative_hidden_layer_gives_exact_zero_weight_gradient(gpu):
    """h1 = relu(negative) = 0 everywhere: dW2 = dh2 h1^T is exactly 0, and so are dW1, db1 and dx behind the dead layer; db2 is not."""
    rng = np.random.default_rng(3)
    x = np.abs(rng.standard_normal((200, 4)))
    xt, p, g = _edge_case(gpu, -np.abs(rng.standard_normal((32, 4))), -np.ones(32), rng.standard_normal((32, 32)), np.ones(32), x)
    for k in (0, 1, 2):
        assert not p[k].grad.any(), k
    assert not xt.grad.any() and p[3].grad.all() and not g["dw2"].any()


def test_bit_identical_from_run_to_run(rast, gpu):
    shape = (32, 9, 128, 128, 48, False)
    c, _, _ = reference(shape, 4099)
    a, b = run_module(shape, c, gpu), run_module(shape, c, gpu)
    assert set(a) == set(("y",) + GRADS)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    r1, r2 = run_raw(rast, shape, c, gpu, 2), run_raw(rast, shape, c, gpu, 2)
    for k in r1:
        assert np.array_equal(r1[k].view(np.uint32), r2[k].view(np.uint32)), ("workgroups = 2", k)
    # y and dx are per row: they do not depend on the workgroup count at all
    assert np.array_equal(a["y"].view(np.uint32), r1["y"].view(np.uint32)) and np.array_equal(a["dx"].view(np.uint32), r1["dx"].view(np.uint32))


@pytest.mark.parametrize("shape", [HEADS[2], HEADS[3]], ids=_sid)
def test_requires_grad_combinations(shape, rast, gpu):
    n = 1000
    c, f64, t32 = reference(shape, n)
    full = run_module(shape, c, gpu)
    no_dx = run_module(shape, c, gpu, need_x=False)
    assert "dx" not in no_dx and all(np.array_equal(no_dx[k], full[k]) for k in no_dx)
    frozen = run_module(shape, c, gpu, need_w=False)
    assert set(frozen) == {"y", "dx"} and np.array_equal(frozen["dx"], full["dx"])
    # one layer's parameters only, through the C ABI: the others' pointers are NULL and nothing is written for them
    for want in (("dw2", "db2"), ("db3",), ("dw1",), ("dx", "dw3")):
        part = run_raw(rast, shape, c, gpu, 0, want)
        check(f"{_sid(shape)} want={want}", part, f64, t32)


def test_no_grad_forward_allocates_nothing_proportional_to_n_but_y(gpu):
    import fused_mlp
    shape = HEADS[2]
    n = 200000
    t = dev_inputs(mm.make_case(*shape[:5], n, seed=5), gpu)
    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        t[k].requires_grad_(True)
    call = lambda: fused_mlp.fused_mlp3(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], t["w3"], t["b3"], x_tail=t["x_tail"])  # noqa: E731
    with torch.no_grad():
        call()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(gpu)
        base = torch.cuda.memory_allocated(gpu)
        y = call()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(gpu) - base
    assert y.requires_grad is False and y.grad_fn is None
    assert peak <= n * shape[4] * 4 + (1 << 20), peak                   # y itself (38.4 MB), nothing else of that order (h1 alone would be 102 MB)
    # and with gradients: what the graph keeps is y only -- no hidden activation (x, the tail and the parameters are the caller's tensors)
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    y2 = call()
    torch.cuda.synchronize()
    assert y2.requires_grad and torch.cuda.max_memory_allocated(gpu) - base <= n * shape[4] * 4 + (1 << 20)


def test_tail_equals_the_explicit_cat_bit_for_bit(gpu):
    import fused_mlp
    for shape in (HEADS[2], CORNERS[2]):
        c, _, _ = reference(shape, 1000)
        t = dev_inputs(c, gpu)
        p = [t[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
        a = fused_mlp.fused_mlp3(t["x"], *p, x_tail=t["x_tail"], sigmoid_out=shape[5])
        b = fused_mlp.fused_mlp3(torch.cat((t["x"], t["x_tail"]), 1), *p, sigmoid_out=shape[5])
        assert torch.equal(a, b)


def test_non_contiguous_inputs_are_made_contiguous(gpu):
    """As fused_hexplane does with its inputs: a strided view gives the result of its contiguous copy, gradient included."""
    import fused_mlp
    shape = HEADS[0]
    c, _, _ = reference(shape, 129)
    t = dev_inputs(c, gpu)
    p = [t[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    wide = torch.zeros((129, 64), device=gpu)
    wide[:, ::2] = t["x"]
    xv = wide[:, ::2].requires_grad_(True)
    tail_t = t["x_tail"].t().contiguous().t()
    assert not xv.is_contiguous() and not tail_t.is_contiguous()
    xc = t["x"].clone().requires_grad_(True)
    a = fused_mlp.fused_mlp3(xv, *p, x_tail=tail_t)
    b = fused_mlp.fused_mlp3(xc, *p, x_tail=t["x_tail"])
    a.backward(t["dy"])
    b.backward(t["dy"])
    assert torch.equal(a, b) and torch.equal(xv.grad, xc.grad)
    w1_t = t["w1"].t().contiguous().t()
    assert not w1_t.is_contiguous() and torch.equal(fused_mlp.fused_mlp3(xc, w1_t, *p[1:], x_tail=t["x_tail"]), b)


class _Heads(nn.Module):
    """The four heads at the reference's shipped widths (scene/saro_gaussian.py:104-110)."""

    def __init__(self):
        super().__init__()
        seq = lambda i, h2, o, sig: nn.Sequential(*([nn.Linear(i, 128), nn.ReLU(), nn.Linear(128, h2), nn.ReLU(), nn.Linear(h2, o)] + ([nn.Sigmoid()] if sig else [])))  # noqa: E731
        self.motion_mlp, self.rot_mlp, self.shs_mlp, self.opacity_mlp = seq(41, 128, 3, False), seq(41, 128, 7, False), seq(41, 128, 48, False), seq(32, 64, 1, True)


def test_end_to_end_field_heads_rasterizer_loss(scenes, rast, gpu):
    """fused_hexplane field -> the four heads -> GaussianRasterizerRaw with the residuals -> l1_dssim_loss -> backward, at P = 500 on 64 x 64:
    convert_heads' heads against the same chain with the nn.Sequential heads in fp32 (the reference) and in fp64 (the truth of the bar)."""
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
    planes0 = [rng.normal(size=(1, 32, 25 if b == 3 else 32, 25 if a == 3 else 32)).astype(np.float32) * 0.5
               for (a, b) in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))]
    pts, levels = f(rng.uniform(0, 1, size=(P, 4))), f(np.concatenate([rng.uniform(0, 5, size=(P, 3)), np.zeros((P, 1))], 1))
    temb = f(rng.standard_normal((P, 9)))
    gt = f(rng.uniform(0, 1, size=(3, H, W)))
    torch.manual_seed(79)
    init = _Heads().state_dict()

    def chain(kind):
        heads = _Heads()
        heads.load_state_dict(init)
        heads = heads.to(gpu)
        dt = torch.float64 if kind == "fp64" else torch.float32
        if kind == "fp64":
            heads = heads.double()
        if kind == "fused":
            assert fused_mlp.convert_heads(heads) == list(fused_mlp.HEAD_NAMES)
        planes = [[torch.tensor(p, device=gpu, requires_grad=True) for p in planes0]]
        feat = fused_hexplane.interpolate_ms_features(pts, planes, 2, True, levels, None)
        if kind == "fused":
            motion, rot, shs, trbf = heads.motion_mlp(feat, temb), heads.rot_mlp(feat, temb), heads.shs_mlp(feat, temb), heads.opacity_mlp(feat)
        else:
            hin = torch.cat((feat.to(dt), temb.to(dt)), 1)
            motion, rot, shs, trbf = (heads.motion_mlp(hin).float(), heads.rot_mlp(hin).float(), heads.shs_mlp(hin).float(),
                                      heads.opacity_mlp(feat.to(dt)).float())
        m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color = rast.GaussianRasterizerRaw(rs)(raw["xyz"], m2, raw["rotation"], raw["scaling"], raw["opacity"], raw["f_dc"], raw["f_rest"],
                                               motion_residual=0.05 * motion, rot_residual=0.1 * rot, trbfoutput=trbf,
                                               shs_residual=0.1 * shs.reshape(P, 16, 3))[0]
        fused_loss.l1_dssim_loss(color, gt, 0.2).backward()
        torch.cuda.synchronize()
        out = {"image": color.detach().cpu().numpy()}
        out.update({f"plane{k}": p.grad.cpu().numpy() for k, p in enumerate(planes[0])})
        out.update({name: p.grad.double().cpu().numpy() for name, p in heads.named_parameters()})
        return out

    truth, ref, got = chain("fp64"), chain("fp32"), chain("fused")
    assert set(got) == set(ref) == set(truth) and len(got) == 1 + 6 + 24
    assert float(np.abs(truth["image"]).max()) > 0.1 and all(np.abs(v).max() > 0 for v in truth.values())
    check("end to end", got, truth, ref)


def test_parameters_at_odd_float_offsets_of_a_flat_buffer(gpu):
    """Parameters that are views into one flat buffer at offsets that are no multiple of 16 bytes (a flat gradient bucket's layout): the
    weight loads take their 4-byte form; same bits as with aligned parameters, outputs and gradients."""
    import fused_mlp
    for shape in (HEADS[2], CORNERS[1]):
        c, f64, t32 = reference(shape, 1000)
        t = dev_inputs(c, gpu)
        names = ("w1", "b1", "w2", "b2", "w3", "b3")
        flat = torch.zeros(sum(t[k].numel() + 8 for k in names) + 8, device=gpu)
        views, at = [], 1
        for k in names:
            v = flat[at:at + t[k].numel()].view_as(t[k])
            v.copy_(t[k])
            assert v.data_ptr() % 16 != 0 and v.is_contiguous()
            views.append(v.requires_grad_(True))
            at = (at + t[k].numel() + 3) // 4 * 4 + 1      # the next offset: 1 float past a multiple of 4 floats
        aligned = [t[k].clone().requires_grad_(True) for k in names]
        xa, xb = t["x"].clone().requires_grad_(True), t["x"].clone().requires_grad_(True)
        ya = fused_mlp.fused_mlp3(xa, *views, x_tail=t["x_tail"], sigmoid_out=shape[5])
        yb = fused_mlp.fused_mlp3(xb, *aligned, x_tail=t["x_tail"], sigmoid_out=shape[5])
        ya.backward(t["dy"])
        yb.backward(t["dy"])
        torch.cuda.synchronize()
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
        for v, a in zip(views, aligned):
            assert torch.equal(v.grad, a.grad)
        got = dict(y=ya.detach().cpu().numpy(), dx=xa.grad.cpu().numpy())
        got.update({g: v.grad.cpu().numpy() for g, v in zip(GRADS[1:], views)})
        check(f"{_sid(shape)} unaligned parameters", got, f64, t32)


def test_nan_goes_through_the_relus_as_in_torch(gpu):
    """A NaN in one input row: that row of y is NaN (torch.relu passes NaN on), every other row keeps its bits; y and every gradient are
    NaN exactly where the nn.Sequential's are (the weight gradients that sum over the row)."""
    import fused_mlp
    shape = HEADS[0]
    c, _, _ = reference(shape, 129)
    t = dev_inputs(c, gpu)
    p = [t[k].clone().requires_grad_(True) for k in ("w1", "b1", "w2", "b2", "w3", "b3")]
    clean = fused_mlp.fused_mlp3(t["x"], *p, x_tail=t["x_tail"])
    x = t["x"].clone()
    x[70, 3] = float("nan")
    x.requires_grad_(True)
    y = fused_mlp.fused_mlp3(x, *p, x_tail=t["x_tail"])
    y.backward(t["dy"])
    torch.cuda.synchronize()
    keep = torch.arange(129, device=gpu) != 70
    assert torch.isnan(y[70]).all() and torch.equal(y[keep], clean[keep])
    assert torch.isfinite(x.grad[keep]).all()      # (row 70's own dx is finite too: the masks pass, the weights are finite -- compared with torch below)
    seq = nn.Sequential(nn.Linear(41, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 3)).to(gpu)
    with torch.no_grad():
        for lin, k in ((seq[0], 0), (seq[2], 2), (seq[4], 4)):
            lin.weight.copy_(p[k])
            lin.bias.copy_(p[k + 1])
    xs = x.detach().clone().requires_grad_(True)
    ys = seq(torch.cat((xs, t["x_tail"]), 1))
    ys.backward(t["dy"])
    assert torch.equal(torch.isnan(ys), torch.isnan(y)) and torch.equal(torch.isnan(xs.grad), torch.isnan(x.grad))
    for mine, theirs in zip(p, seq.parameters()):
        assert torch.equal(torch.isnan(mine.grad), torch.isnan(theirs.grad))


def test_tensors_on_another_device_and_a_double_backward_raise(gpu):
    import fused_mlp
    shape = HEADS[0]
    c, _, _ = reference(shape, 33)
    t = dev_inputs(c, gpu)
    names = ("w1", "b1", "w2", "b2", "w3", "b3")
    for on_cpu in names + ("x_tail",):
        args = {k: (t[k].cpu() if k == on_cpu else t[k]) for k in names + ("x_tail",)}
        with pytest.raises(RuntimeError, match=on_cpu + " is on cpu"):
            fused_mlp.fused_mlp3(t["x"], *[args[k] for k in names], x_tail=args["x_tail"])
    x = t["x"].clone().requires_grad_(True)
    y = fused_mlp.fused_mlp3(x, *[t[k] for k in names], x_tail=t["x_tail"])
    dy = t["dy"].clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):      # (never a silent wrong second derivative)
        gx.sum().backward()
    assert dy.grad is None
