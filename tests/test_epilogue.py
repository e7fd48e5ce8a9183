"""Fused activation / deformation epilogue (the "next" row before the rasterizer).

CPU: the numpy oracle against an independently written torch restatement of the reference's formulation
(scene/saro_gaussian.py:807-847, activations :39-47) and its autograd.  GPU (-m gpu): the HIP kernels through the
autograd wrapper against both, forward and backward, in every combination of present / absent residuals."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _inputs(P, M, seed):
    rng = np.random.default_rng(seed)
    d = dict(
        xyz=rng.normal(size=(P, 3)), motion_res=0.05 * rng.normal(size=(P, 3)),
        rotation=rng.normal(size=(P, 4)), rot_res=0.1 * rng.normal(size=(P, 7)),
        scaling=rng.normal(-3.0, 1.0, size=(P, 3)), opacity=rng.normal(0.0, 2.0, size=(P, 1)),
        trbf=rng.uniform(0.0, 1.0, size=(P, 1)),
        f_dc=rng.uniform(-1.7, 1.7, size=(P, 1, 3)), f_rest=0.1 * rng.normal(size=(P, M - 1, 3)),
        shs_res=0.05 * rng.normal(size=(P, M, 3)))
    d["rotation"][0] = 0.0; d["rot_res"][0, :4] = 0.0        # a zero quaternion: normalize clamps at eps
    return {k: v.astype(np.float32) for k, v in d.items()}


def torch_epilogue(t, use):
    """The reference's own formulation, in torch (written for this test)."""
    motion = t["xyz"] + t["motion_res"] if use["motion_res"] else t["xyz"]
    if use["rot_res"]:
        rot = F.normalize(t["rotation"] + t["rot_res"][:, :4])
        scale = torch.exp(t["scaling"] + t["rot_res"][:, 4:])
    else:
        rot, scale = F.normalize(t["rotation"]), torch.exp(t["scaling"])
    opa = torch.sigmoid(t["opacity"]) * t["trbf"] if use["trbf"] else torch.sigmoid(t["opacity"])
    shs = torch.cat((t["f_dc"], t["f_rest"]), dim=1)
    if use["shs_res"]:
        shs = shs + t["shs_res"]
    return motion, rot, scale, opa, shs


COMBOS = [dict(zip(("motion_res", "rot_res", "trbf", "shs_res"), c)) for c in itertools.product((True, False), repeat=4)]


@pytest.mark.parametrize("use", [COMBOS[0], COMBOS[-1], COMBOS[5]], ids=["all", "none", "mixed"])
def test_numpy_oracle_matches_torch_restatement(use):
    from oracle import epilogue_oracle as eo
    P, M = 257, 16
    inp = _inputs(P, M, 5)
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in inp.items()}
    outs = torch_epilogue(t, use)
    o = eo.forward(inp["xyz"], inp["rotation"], inp["scaling"], inp["opacity"], inp["f_dc"], inp["f_rest"],
                   motion_res=inp["motion_res"] if use["motion_res"] else None, rot_res=inp["rot_res"] if use["rot_res"] else None,
                   trbf=inp["trbf"] if use["trbf"] else None, shs_res=inp["shs_res"] if use["shs_res"] else None)
    for name, a in zip(("motion", "rot", "scale", "opacity", "shs"), outs):
        np.testing.assert_allclose(o[name][1:], a.detach().numpy()[1:], rtol=1e-13, atol=1e-15, err_msg=name)
    rng = np.random.default_rng(6)
    ups = [torch.from_numpy(rng.normal(size=tuple(a.shape))) for a in outs]
    torch.autograd.backward(outs, ups)
    b = eo.backward(inp["rotation"], inp["scaling"], inp["opacity"], inp["rot_res"] if use["rot_res"] else None,
                    inp["trbf"] if use["trbf"] else None, ups[1].numpy(), ups[2].numpy(), ups[3].numpy())
    np.testing.assert_allclose(b["rotation"], t["rotation"].grad.numpy(), rtol=1e-10, atol=1e-12)      # row 0 (clamped norm: g / eps) included
    np.testing.assert_allclose(b["scaling"], t["scaling"].grad.numpy(), rtol=1e-12)
    np.testing.assert_allclose(b["logit"], t["opacity"].grad.numpy(), rtol=1e-12, atol=1e-15)
    if use["trbf"]:
        np.testing.assert_allclose(b["trbf"], t["trbf"].grad.numpy(), rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("use", COMBOS, ids=["".join("1" if v else "0" for v in c.values()) for c in COMBOS])
@pytest.mark.parametrize("P,M", [(1000, 16), (333, 9)])
def test_hip_epilogue_matches_reference_formulation(use, P, M, gpu):
    from oracle import epilogue_oracle as eo
    import fused_epilogue
    inp = _inputs(P, M, 9)
    dev = gpu
    t = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in inp.items()}
    outs = fused_epilogue.activate_gaussians(
        t["xyz"], t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"],
        motion_residual=t["motion_res"] if use["motion_res"] else None, rot_residual=t["rot_res"] if use["rot_res"] else None,
        trbfoutput=t["trbf"] if use["trbf"] else None, shs_residual=t["shs_res"] if use["shs_res"] else None)
    o = eo.forward(inp["xyz"], inp["rotation"], inp["scaling"], inp["opacity"], inp["f_dc"], inp["f_rest"],
                   motion_res=inp["motion_res"] if use["motion_res"] else None, rot_res=inp["rot_res"] if use["rot_res"] else None,
                   trbf=inp["trbf"] if use["trbf"] else None, shs_res=inp["shs_res"] if use["shs_res"] else None)
    for name, a in zip(("motion", "rot", "scale", "opacity", "shs"), outs):
        got = a.detach().cpu().numpy().astype(np.float64)
        sl = slice(1, None) if name == "rot" else slice(None)     # row 0: zero quaternion (0/eps), checked below
        np.testing.assert_allclose(got[sl], o[name][sl], rtol=3e-6, atol=1e-7, err_msg=name)
    assert not outs[1][0].any()                                    # normalize(0) = 0
    # backward against torch autograd of the reference's formulation on the same device (fp32) and the fp64 oracle
    rng = np.random.default_rng(10)
    ups = [torch.from_numpy(rng.normal(size=tuple(a.shape)).astype(np.float32)).to(dev) for a in outs]
    torch.autograd.backward(outs, ups)
    t2 = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in inp.items()}
    torch.autograd.backward(torch_epilogue(t2, use), ups)
    for k in t:
        used = use.get(k, True)
        if not used:
            assert t[k].grad is None
            continue
        a, b = t[k].grad, t2[k].grad
        assert torch.allclose(a, b, rtol=2e-5, atol=1e-6), (k, float((a - b).abs().max()))      # row 0 (clamped norm: g * 1e12) included
    b64 = eo.backward(inp["rotation"], inp["scaling"], inp["opacity"], inp["rot_res"] if use["rot_res"] else None,
                      inp["trbf"] if use["trbf"] else None, ups[1].cpu().numpy(), ups[2].cpu().numpy(), ups[3].cpu().numpy())
    np.testing.assert_allclose(t["scaling"].grad.cpu().numpy(), b64["scaling"], rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(t["opacity"].grad.cpu().numpy(), b64["logit"], rtol=3e-5, atol=1e-7)
    np.testing.assert_allclose(t["rotation"].grad.cpu().numpy(), b64["rotation"], rtol=3e-5, atol=1e-6)


def _use(**kw):
    u = dict(motion_res=True, rot_res=True, trbf=True, shs_res=True)
    u.update(kw)
    return u


def _hip_epilogue(t, use):
    import fused_epilogue
    return fused_epilogue.activate_gaussians(
        t["xyz"], t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"],
        motion_residual=t["motion_res"] if use["motion_res"] else None, rot_residual=t["rot_res"] if use["rot_res"] else None,
        trbfoutput=t["trbf"] if use["trbf"] else None, shs_residual=t["shs_res"] if use["shs_res"] else None)


def _leaves(inp, dev, dtype=torch.float32):
    return {k: torch.from_numpy(v).to(device=dev, dtype=dtype).requires_grad_(True) for k, v in inp.items()}


def _upstreams(outs, seed, dev):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.normal(size=tuple(a.shape)).astype(np.float32)).to(dev) for a in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False], ids=["rot_res", "no_rot_res"])
def test_hip_epilogue_zero_and_tiny_quaternions(with_res, gpu):
    """|x| < 1e-12: F.normalize divides by the clamped norm and autograd does not differentiate it -- forward x / 1e-12, backward g * 1e12,
    the copy into d_rot_residual[:, :4] included.  Against torch autograd of F.normalize in fp64 (values ~1e12: relative bar)."""
    inp = _inputs(6, 4, 31)
    tiny = np.array([[0, 0, 0, 0], [3e-13, 0, 0, 0], [1e-20, 1e-20, 0, 0]], np.float32)
    if with_res:                                   # the SUM is tiny: the clamp acts on rotation + residual
        inp["rotation"][:3] = inp["rot_res"][:3, :4] = 0.5 * tiny
    else:
        inp["rotation"][:3] = tiny
    use = _use(rot_res=with_res)
    t = _leaves(inp, gpu)
    outs = _hip_epilogue(t, use)
    ups = _upstreams(outs, 32, gpu)
    torch.autograd.backward(outs, ups)
    t64 = _leaves(inp, "cpu", torch.float64)
    o64 = torch_epilogue(t64, use)
    torch.autograd.backward(o64, [u.cpu().double() for u in ups])
    x64 = (inp["rotation"].astype(np.float64) + (inp["rot_res"][:, :4] if with_res else 0.0))
    assert (np.linalg.norm(x64[:3], axis=1) < 1e-12).all() and (np.linalg.norm(x64[3:], axis=1) > 1e-3).all()
    np.testing.assert_allclose(outs[1].detach().cpu().numpy(), o64[1].detach().numpy(), rtol=3e-5, atol=0)
    np.testing.assert_allclose(o64[1].detach().numpy()[:3], x64[:3] / 1e-12, rtol=1e-12, atol=0)                  # forward: x / eps
    want = t64["rotation"].grad.numpy()
    np.testing.assert_allclose(want[:3], ups[1].cpu().numpy()[:3].astype(np.float64) * 1e12, rtol=1e-12)          # backward: g / eps
    np.testing.assert_allclose(t["rotation"].grad.cpu().numpy(), want, rtol=3e-5, atol=1e-6)
    if with_res:
        np.testing.assert_allclose(t["rot_res"].grad.cpu().numpy(), t64["rot_res"].grad.numpy(), rtol=3e-5, atol=1e-6)
        assert torch.equal(t["rot_res"].grad[:, :4], t["rotation"].grad)
    else:
        assert t["rot_res"].grad is None


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [True, False], ids=["shs_res", "no_shs_res"])
@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_hip_epilogue_sh_row_lengths(M, P, with_res, gpu):
    """M = 1: an empty features_rest (a null pointer), rows of 3 floats; M = 2: 6 floats, one float per lane; M = 4: 12 floats, one float4
    per lane with 9 floats of features_rest per row."""
    from oracle import epilogue_oracle as eo
    inp = _inputs(P, M, 33)
    use = _use(shs_res=with_res)
    t = _leaves(inp, gpu)
    assert tuple(t["f_rest"].shape) == (P, M - 1, 3)
    outs = _hip_epilogue(t, use)
    o = eo.forward(inp["xyz"], inp["rotation"], inp["scaling"], inp["opacity"], inp["f_dc"], inp["f_rest"], motion_res=inp["motion_res"],
                   rot_res=inp["rot_res"], trbf=inp["trbf"], shs_res=inp["shs_res"] if with_res else None)
    for name, a in zip(("motion", "rot", "scale", "opacity", "shs"), outs):
        assert tuple(a.shape) == o[name].shape
        np.testing.assert_allclose(a.detach().cpu().numpy(), o[name], rtol=3e-6, atol=1e-7, err_msg=name)
    cat = np.concatenate([inp["f_dc"], inp["f_rest"]], axis=1)
    assert np.array_equal(outs[4].detach().cpu().numpy(), cat + inp["shs_res"] if with_res else cat)        # one fp32 addition: exact
    ups = _upstreams(outs, 34, gpu)
    torch.autograd.backward(outs, ups)
    assert tuple(t["f_rest"].grad.shape) == (P, M - 1, 3) and tuple(t["f_dc"].grad.shape) == (P, 1, 3)
    assert torch.equal(t["f_dc"].grad, ups[4][:, :1]) and torch.equal(t["f_rest"].grad, ups[4][:, 1:])
    assert torch.equal(t["shs_res"].grad, ups[4]) if with_res else t["shs_res"].grad is None
    b64 = eo.backward(inp["rotation"], inp["scaling"], inp["opacity"], inp["rot_res"], inp["trbf"],
                      ups[1].cpu().numpy(), ups[2].cpu().numpy(), ups[3].cpu().numpy())
    np.testing.assert_allclose(t["rotation"].grad.cpu().numpy(), b64["rotation"], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(t["scaling"].grad.cpu().numpy(), b64["scaling"], rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(t["opacity"].grad.cpu().numpy(), b64["logit"], rtol=3e-5, atol=1e-7)


OUTPUTS = ("motion", "rot", "scale", "opacity", "shs")


@pytest.mark.gpu
@pytest.mark.parametrize("sel", [(0,), (1,), (2,), (3,), (4,), (1, 4)], ids=lambda s: "+".join(OUTPUTS[i] for i in s))
def test_hip_epilogue_missing_upstream_gradients(sel, gpu):
    """Backward from some outputs only: the others' upstream gradients arrive as None (null pointers in the kernel) and count as zero.
    Inputs nothing reaches: exact zeros from the backward kernel (rotation, scaling, opacity, rot_residual, trbfoutput), None for the
    inputs whose gradient is a view of an absent upstream (xyz, motion_residual, features_dc, features_rest, shs_residual) -- as
    fused_epilogue.activate_gaussians documents."""
    from oracle import epilogue_oracle as eo
    P, M = 300, 4
    inp = _inputs(P, M, 35)
    t = _leaves(inp, gpu)
    outs = _hip_epilogue(t, _use())
    ups = _upstreams(outs, 36, gpu)
    torch.autograd.backward([outs[i] for i in sel], [ups[i] for i in sel])
    up64 = [ups[i].cpu().numpy().astype(np.float64) if i in sel else np.zeros(tuple(outs[i].shape)) for i in range(5)]
    b64 = eo.backward(inp["rotation"], inp["scaling"], inp["opacity"], inp["rot_res"], inp["trbf"], up64[1], up64[2], up64[3])
    g = lambda k: t[k].grad.cpu().numpy()  # noqa: E731
    np.testing.assert_allclose(g("rotation"), b64["rotation"], rtol=3e-5, atol=1e-6)
    np.testing.assert_allclose(g("scaling"), b64["scaling"], rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(g("opacity"), b64["logit"], rtol=3e-5, atol=1e-7)
    np.testing.assert_allclose(g("trbf"), b64["trbf"], rtol=3e-5, atol=1e-7)
    np.testing.assert_allclose(g("rot_res"), np.concatenate([b64["rotation"], b64["scaling"]], axis=1), rtol=3e-5, atol=1e-6)
    if 1 not in sel:
        assert not g("rotation").any() and not g("rot_res")[:, :4].any()
    if 2 not in sel:
        assert not g("scaling").any() and not g("rot_res")[:, 4:].any()
    if 3 not in sel:
        assert not g("opacity").any() and not g("trbf").any()
    for k in ("xyz", "motion_res"):
        assert torch.equal(t[k].grad, ups[0]) if 0 in sel else t[k].grad is None, k
    if 4 in sel:
        assert torch.equal(t["f_dc"].grad, ups[4][:, :1]) and torch.equal(t["f_rest"].grad, ups[4][:, 1:]) and torch.equal(t["shs_res"].grad, ups[4])
    else:
        assert t["f_dc"].grad is None and t["f_rest"].grad is None and t["shs_res"].grad is None


@pytest.mark.gpu
def test_hip_epilogue_saturating_logits_and_log_scales(gpu):
    """sigmoid and exp where fp32 saturates: exp(104) and exp(90) overflow inside the sigmoid (opacity 0), exp(-20) vanishes next to 1
    (opacity 1, zero gradient), exp(89) is inf and exp(-104) is 0 as a scale.  Against the fp32 torch restatement on the same device."""
    logits, log_scales = (-104.0, -90.0, -20.0, 20.0, 90.0, 104.0), (-104.0, -90.0, 88.0, 89.0)
    P, M = 24, 4
    inp = _inputs(P, M, 37)
    r = np.arange(P)
    inp["opacity"][:, 0] = np.array(logits, np.float32)[r % 6]
    inp["trbf"][:, 0] = ((r // 6) % 2).astype(np.float32)                          # every logit with trbf 0 and with trbf 1
    inp["scaling"][:] = np.array(log_scales, np.float32)[(r[:, None] + np.arange(3)[None]) % 4]
    inp["rot_res"][:, 4:] = 0.0
    inp["rotation"][0] = [1.0, 0.5, -0.5, 0.25]                                   # (_inputs zeroes row 0: not this test's subject)
    use = _use()
    t, t2 = _leaves(inp, gpu), _leaves(inp, gpu)
    outs, ref = _hip_epilogue(t, use), torch_epilogue(t2, use)
    for name, a, b in zip(OUTPUTS, outs, ref):
        assert not torch.isnan(a).any() and bool((torch.isfinite(a) | ~torch.isfinite(b)).all()), name
        assert torch.allclose(a, b, rtol=3e-6, atol=1e-7), name
    assert int(torch.isinf(outs[2]).sum()) == int(torch.isinf(ref[2]).sum()) == int((inp["scaling"] == 89.0).sum()) > 0
    assert not outs[3].detach().cpu().numpy()[inp["trbf"][:, 0] == 0].any()         # trbf 0: opacity exactly 0
    ups = _upstreams(outs, 38, gpu)
    torch.autograd.backward(outs, ups)
    torch.autograd.backward(ref, ups)
    for k in t:
        a, b = t[k].grad, t2[k].grad
        assert not torch.isnan(a).any() and bool((torch.isfinite(a) | ~torch.isfinite(b)).all()), k
        assert torch.allclose(a, b, rtol=2e-5, atol=1e-6), (k, a, b)


def _offset_view(a, dev):
    """A contiguous tensor whose storage starts 4 bytes behind a 16-byte boundary: a flat buffer sliced from element 1."""
    flat = torch.zeros(a.numel() + 8, dtype=torch.float32, device=dev)
    v = flat[1:1 + a.numel()].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v.detach()


@pytest.mark.gpu
def test_hip_epilogue_quaternions_off_the_16_byte_boundary(gpu):
    """rotation and the upstream gradient of rot are read as float4.  A contiguous view 4 bytes into a larger buffer goes through the wrapper
    (which copies it) with the bits of an aligned copy; the C entry points refuse such a pointer instead of handing it to the kernel."""
    from diff_gaussian_rasterization_ch3 import _C
    P, M = 257, 4
    inp = _inputs(P, M, 39)
    runs = {}
    for off in (False, True):
        t = _leaves(inp, gpu)
        if off:
            t["rotation"] = _offset_view(t["rotation"].detach(), gpu).requires_grad_(True)
        outs = _hip_epilogue(t, _use())
        ups = _upstreams(outs, 40, gpu)
        if off:
            ups[1] = _offset_view(ups[1], gpu)
        torch.autograd.backward(outs, ups)
        runs[off] = [a.detach() for a in outs] + [t[k].grad for k in sorted(t)]
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the C ABI: every buffer is real device memory with room behind it, only the address is off
    buf = lambda n: torch.zeros(n + 8, dtype=torch.float32, device=gpu)  # noqa: E731
    B = {k: buf(P * w) for k, w in dict(xyz=3, rotation=4, scaling=3, opacity=1, f_dc=3, f_rest=9, motion=3, rot=4, scale=3, opa=1, shs=12,
                                        d_rot=4, d_rotation=4, d_scaling=3, d_logit=1).items()}
    L = _C.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def fwd(**shift):
        p = {k: v.data_ptr() + shift.get(k, 0) for k, v in B.items()}
        return L.gsrast_activate_forward(P, M, p["xyz"], None, p["rotation"], None, p["scaling"], p["opacity"], None, p["f_dc"], p["f_rest"], None,
                                         p["motion"], p["rot"], p["scale"], p["opa"], p["shs"], stream)

    def bwd(**shift):
        p = {k: v.data_ptr() + shift.get(k, 0) for k, v in B.items()}
        return L.gsrast_activate_backward(P, p["rotation"], None, p["scale"], p["opacity"], None, p["d_rot"], None, None,
                                          p["d_rotation"], p["d_scaling"], None, p["d_logit"], None, stream)

    with torch.cuda.device(gpu):
        assert fwd() == 0 and bwd() == 0
        assert fwd(rotation=4) == -1 and fwd(rot=8) == -1                        # GSRAST_E_ARG
        assert bwd(rotation=4) == -1 and bwd(d_rot=12) == -1 and bwd(d_rotation=4) == -1
    torch.cuda.synchronize(gpu)


@pytest.mark.gpu
def test_epilogue_feeds_the_rasterizer(scenes, rast, gpu):
    """End to end: raw parameters -> fused epilogue -> rasterizer -> backward reaches the raw parameters."""
    from conftest import settings_from
    import fused_epilogue
    P, W, H = 2000, 96, 64
    sc = scenes.synth(P, 121)
    cam = scenes.camera(0, 1, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)  # noqa: E731
    raw = dict(xyz=tt(sc["means3D"]), rotation=tt(sc["rotations"]) * 2.0, scaling=torch.log(tt(sc["scales"])),
               opacity=torch.logit(tt(sc["opacities"]).clamp(1e-4, 1 - 1e-4)), f_dc=tt(sc["shs"][:, :1]), f_rest=tt(sc["shs"][:, 1:]))
    raw = {k: v.requires_grad_(True) for k, v in raw.items()}
    motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(raw["xyz"], raw["rotation"], raw["scaling"], raw["opacity"],
                                                                      raw["f_dc"], raw["f_rest"])
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    color, radii, depth = rast.GaussianRasterizer(rs)(means3D=motion, means2D=m2, opacities=opa, shs=shs, scales=scale, rotations=rot)
    color.sum().backward()
    for k, v in raw.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0, k
    assert torch.allclose(shs, tt(sc["shs"])) and torch.allclose(scale, tt(sc["scales"]), rtol=1e-5)
