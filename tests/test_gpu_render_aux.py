"""-m gpu: the differentiable alpha and accumulated-depth outputs (return_aux=True; include/gsrast.h: GSRAST_RENDER_AUX,
both families).

    acc_depth = sum_i alpha_i T_i z_i     alpha = 1 - T_final

over the colour's contributors and early stop.  Their exact specification needs no new oracle: acc_depth is the first channel of a plain
render whose colours are the Gaussians' view-space depths on a black background, alpha the complement of final_T -- and with the depths
computed in torch from means3D, autograd of that second render is the truth for the gradients."""
import numpy as np
import pytest
import torch

import math_renderer as mr
from conftest import grad_tol, settings_from
from edge_scenes import clamped_mask, edge_scene

pytestmark = pytest.mark.gpu

SHAPES = [("cfg2_100k_800", 100_000, 800, 800), ("cfg3_1M_1352x1014", 1_000_000, 1352, 1014)]
LEAVES = ("means3D", "opacities", "shs", "scales", "rotations")


def _setup(scenes, rast, dev, P, W, H, seed=0, bg=None, k=0, V=1):
    sc = scenes.synth(P, seed)
    cam = scenes.camera(k, V, W, H)
    rs = settings_from(rast, cam, sc, dev, bg=bg)
    return sc, cam, rs


def _leaves(sc, dev, names=LEAVES):
    return {n: torch.as_tensor(np.ascontiguousarray(sc[n]), dtype=torch.float32, device=dev).requires_grad_(True) for n in names}


def _render(rast, rs, t, m2, return_aux=False, colors=None, cov3D=None):
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"])
    kw.update(colors_precomp=colors) if colors is not None else kw.update(shs=t["shs"])
    kw.update(cov3D_precomp=cov3D) if cov3D is not None else kw.update(scales=t["scales"], rotations=t["rotations"])
    return rast.GaussianRasterizer(rs)(**kw, return_aux=return_aux)


def _view_z(means3D, rs):
    V = rs.viewmatrix                       # transposed storage: row vector @ V
    return means3D @ V[:3, 2] + V[3, 2]


def _state(rast, rs, sc, dev, P, W, H, colors=None, aux=True):
    """The library's own forward (aux or plain) + debug_export of its state."""
    e = torch.empty(0)
    t = {n: torch.as_tensor(np.ascontiguousarray(sc[n]), dtype=torch.float32, device=dev) for n in LEAVES}
    out = rast._C.rasterize_gaussians(rs.bg, t["means3D"], e if colors is None else colors, t["opacities"], t["scales"], t["rotations"],
                                      1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W,
                                      t["shs"] if colors is None else e, rs.sh_degree, rs.campos, False, aux=aux)
    st = rast._C.debug_export(P, out[0], W, H, out[3], out[4], out[5])
    return out, st


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _close(a, b, ref32=None, what=""):
    a = a.detach().double().cpu().numpy(); b = b.detach().double().cpu().numpy()
    tol = grad_tol(b, None if ref32 is None else ref32.detach().double().cpu().numpy())
    err = np.abs(a - b)
    assert (err <= tol).all(), (what, float(err.max()), float(np.abs(b).max()))


@pytest.mark.parametrize("cut", [True, False], ids=["list_cut", "no_list_cut"])
@pytest.mark.parametrize("name,P,W,H", SHAPES, ids=[s[0] for s in SHAPES])
def test_default_outputs_and_colour_gradients_are_untouched(name, P, W, H, cut, scenes, rast, gpu):
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    g = torch.from_numpy(scenes.upstream_grad(H, W, 1)).to(gpu)
    rast._C.set_option("no_list_cut", 0 if cut else 1)
    try:
        runs = []
        for aux, zero_aux in ((False, False), (False, False), (True, False), (True, True)):
            for _ in range(2):      # the pose's second render is the one the list cut applies to
                t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
                out = _render(rast, rs, t, m2, return_aux=aux)
            loss = (out[0] * g).sum()
            if zero_aux:            # the aux backward kernel with zero upstream: the same gradients
                loss = loss + (out[3] * 0.0).sum() + (out[4] * 0.0).sum()
            loss.backward()
            torch.cuda.synchronize()
            runs.append((out, {n: t[n].grad for n in LEAVES}, m2.grad))
    finally:
        rast._C.set_option("no_list_cut", 0)
    (o_a, g_a, m_a), (_, g_b, m_b) = runs[0], runs[1]
    for o, gr, m in runs[2:]:
        for k in range(3):
            assert np.array_equal(_bits(o[k]), _bits(o_a[k])), k
        for n in LEAVES:
            _close(gr[n], g_a[n], ref32=g_b[n], what=n)        # (floor: the plain backward's own run-to-run spread, float atomics)
        _close(m, m_a, ref32=m_b, what="means2D")


@pytest.mark.parametrize("exp_mode", [0, 2])
@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)], ids=["black", "white"])
def test_forward_identities_are_exact(bg, exp_mode, scenes, rast, gpu):
    P, W, H = 100_000, 800, 800
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H, bg=np.array(bg, np.float32))
    rast._C.set_option("exp_mode", exp_mode)
    try:
        out, st = _state(rast, rs, sc, gpu, P, W, H)
        acc, alpha = out[7], out[8]
        assert np.array_equal(_bits(alpha.reshape(H, W)), _bits(1.0 - st["final_T"].reshape(H, W)))
        z = st["depths"].reshape(P, 1).expand(P, 3).contiguous()
        rs0 = settings_from(rast, cam, sc, gpu, bg=np.zeros(3, np.float32))
        plain, _ = _state(rast, rs0, sc, gpu, P, W, H, colors=z, aux=False)
        assert np.array_equal(_bits(acc[0]), _bits(plain[1][0]))
        assert float(alpha.min()) >= 0.0 and float(alpha.max()) < 1.0 and float(alpha.mean()) > 0.05
        assert float(acc.max()) > 0.0
    finally:
        rast._C.set_option("exp_mode", 0)


def _cov6(sc):
    q = sc["rotations"].astype(np.float64); q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * sc["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


@pytest.mark.parametrize("colour,geom", [("sh", "sr"), ("precomp", "sr"), ("sh", "cov3D"), ("precomp", "cov3D")])
def test_gradients_equal_the_two_render_identity(colour, geom, scenes, rast, gpu):
    P, W, H = 100_000, 800, 800
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H, seed=3, bg=np.array([0.2, 0.5, 0.9], np.float32))
    rs0 = settings_from(rast, cam, sc, gpu, bg=np.zeros(3, np.float32))
    rng = np.random.default_rng(5)
    gC = torch.from_numpy(scenes.upstream_grad(H, W, 6)).to(gpu)
    gD = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    gA = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    rgb = rng.uniform(0.0, 1.0, size=(P, 3)).astype(np.float32)
    cov = _cov6(sc)

    def leaves():
        t = _leaves(sc, gpu)
        t["rgb"] = torch.from_numpy(rgb).to(gpu).requires_grad_(True)
        t["cov3D"] = torch.from_numpy(cov).to(gpu).requires_grad_(True)
        return t, torch.zeros((P, 3), device=gpu, requires_grad=True)

    def kw(t):
        return dict(colors=t["rgb"] if colour == "precomp" else None, cov3D=t["cov3D"] if geom == "cov3D" else None)

    names = ["means3D", "opacities"] + (["shs"] if colour == "sh" else ["rgb"]) + (["scales", "rotations"] if geom == "sr" else ["cov3D"])
    results = []
    for rep in range(2):
        # (a) one aux render
        ta, ma = leaves()
        c, _, _, acc, alpha = _render(rast, rs, ta, ma, return_aux=True, **kw(ta))
        ((c * gC).sum() + (acc * gD).sum() + (alpha * gA).sum()).backward()
        # (b) the colour render + a render of (z, 1, 0) on black
        tb, mb = leaves()
        c2, _, _ = _render(rast, rs, tb, mb, **kw(tb))
        z = _view_z(tb["means3D"], rs)
        zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
        c3, _, _ = _render(rast, rs0, tb, mb, colors=zc, cov3D=kw(tb)["cov3D"])
        ((c2 * gC).sum() + (c3[0:1] * gD).sum() + (c3[1:2] * gA).sum()).backward()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(c), _bits(c2))
        results.append(({n: ta[n].grad for n in names}, ma.grad, {n: tb[n].grad for n in names}, mb.grad))
    (ga, ma, gb, mb), (_, _, gb2, mb2) = results
    for n in names:
        assert float(gb[n].abs().max()) > 0.0, n
        _close(ga[n], gb[n], ref32=gb2[n], what=n)
    _close(ma, mb, ref32=mb2, what="means2D")


SMALL = [
    dict(P=300, seed=21, W=64, H=48, k=1, V=5, deg=3, smul=0.8, bg=(0.1, 0.2, 0.3), omul=1.0),
    dict(P=150, seed=23, W=48, H=64, k=0, V=4, deg=1, smul=1.6, bg=(1.0, 1.0, 1.0), omul=1.0),
    dict(P=500, seed=24, W=80, H=64, k=2, V=6, deg=0, smul=0.7, bg=(0.0, 0.5, 0.0), omul=0.5),
]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: f"P{c['P']}_deg{c['deg']}")
def test_aux_outputs_and_gradients_against_fp64_math(c, scenes, rast, gpu):
    sc, cam = edge_scene(scenes, c)
    P, W, H, deg = sc["means3D"].shape[0], c["W"], c["H"], c["deg"]
    # truth: alpha = 1 - final_T, acc_depth = the colour of a (z, 0, 0) render on black, z differentiable
    t64 = {n: torch.as_tensor(np.asarray(sc[n], np.float64)).requires_grad_(True) for n in ("means3D", "scales", "rotations", "opacities", "shs")}
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    ref = mr.render(t64["means3D"], t64["scales"], t64["rotations"], t64["opacities"], t64["shs"], deg, cam, sc["bg"], ndc_offset=off,
                    clamp_grad="reference")
    V = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float64))
    z = t64["means3D"] @ V[:3, 2] + V[3, 2]
    zc = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1)
    refd = mr.render(t64["means3D"], t64["scales"], t64["rotations"], t64["opacities"], t64["shs"], deg, cam, np.zeros(3),
                     colors_precomp=zc, ndc_offset=off, clamp_grad="reference")
    amb = ref["ambiguous"] | refd["ambiguous"]
    assert amb.mean() < 0.05
    keep = ~amb
    rng = np.random.default_rng(c["seed"] + 3)
    gD = rng.normal(size=(H, W)); gA = rng.normal(size=(H, W))
    gD[amb] = 0.0; gA[amb] = 0.0
    alpha64 = 1.0 - ref["final_T"]
    ((refd["color"][0] * torch.as_tensor(gD)).sum() + (alpha64 * torch.as_tensor(gA)).sum()).backward()

    rs = settings_from(rast, cam, sc, gpu)
    t = _leaves(sc, gpu)
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    _, radii, _, acc, alpha = _render(rast, rs, t, m2, return_aux=True)
    gD32 = torch.from_numpy(gD.astype(np.float32)).to(gpu)[None]; gA32 = torch.from_numpy(gA.astype(np.float32)).to(gpu)[None]
    ((acc * gD32).sum() + (alpha * gA32).sum()).backward()
    # the fp32 floor: the same gradients through the long-standing colour path ((z, 1, 0) on black, z from torch)
    t2 = _leaves(sc, gpu)
    m22 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    rs0 = settings_from(rast, cam, sc, gpu, bg=np.zeros(3, np.float32))
    zz = _view_z(t2["means3D"], rs0)
    c3, _, _ = _render(rast, rs0, t2, m22, colors=torch.stack([zz, torch.ones_like(zz), torch.zeros_like(zz)], 1))
    ((c3[0:1] * gD32).sum() + (c3[1:2] * gA32).sum()).backward()
    torch.cuda.synchronize()

    assert np.array_equal(radii.cpu().numpy() > 0, ref["proj"]["disc"]["vis"]), "radius decision differs: pick another seed"
    np.testing.assert_allclose(alpha[0].detach().cpu().numpy()[keep], alpha64.detach().numpy()[keep], rtol=0, atol=2e-6)
    acc_ref = refd["color"][0].detach().numpy()
    np.testing.assert_allclose(acc[0].detach().cpu().numpy()[keep], acc_ref[keep], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(acc_ref).max())))
    cl = clamped_mask(sc, cam)      # the frustum-clamped rows once more, as a tensor of their own: their gradients are small
    assert cl.sum() >= 16
    for n in ("means3D", "opacities", "scales", "rotations"):
        want = t64[n].grad.numpy()
        got = t[n].grad.detach().double().cpu().numpy().reshape(want.shape)
        f32 = t2[n].grad.detach().double().cpu().numpy().reshape(want.shape)
        for what, sel in ((n, np.ones(P, bool)),) + (((n + ", clamped rows", cl),) if n == "means3D" else ()):
            tol = grad_tol(want[sel], f32[sel])
            assert (np.abs(got[sel] - want[sel]) <= tol).all(), (what, float(np.abs(got[sel] - want[sel]).max()), float(np.abs(want[sel]).max()))
    assert float(np.abs(t64["means3D"].grad.numpy()).max()) > 1e-3
    assert float(np.abs(t64["means3D"].grad.numpy()[cl]).max()) > 0.0
    assert float(t["shs"].grad.abs().max()) == 0.0
    want2 = off.grad.numpy()
    got2 = m2.grad[:, :2].double().cpu().numpy()
    assert (np.abs(got2 - want2) <= grad_tol(want2, m22.grad[:, :2].double().cpu().numpy())).all()


def test_depth_or_alpha_only_losses_train_the_geometry(scenes, rast, gpu):
    P, W, H = 100_000, 800, 800
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    _, _, _, acc, alpha = _render(rast, rs, t, m2, return_aux=True)
    acc.mean().backward()
    assert float(t["means3D"].grad.abs().max()) > 0.0 and float(t["opacities"].grad.abs().max()) > 0.0
    assert float(t["shs"].grad.abs().max()) == 0.0
    t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    _, _, _, acc, alpha = _render(rast, rs, t, m2, return_aux=True)
    alpha.sum().backward()
    assert float(t["shs"].grad.abs().max()) == 0.0
    assert float(t["opacities"].grad.abs().max()) > 0.0 and float(m2.grad.abs().max()) > 0.0


def test_raw_path_matches_epilogue_then_rasterizer(scenes, rast, gpu):
    import fused_epilogue
    from test_gpu_raw import _raw_scene, _tensors
    P, W, H, M, deg = 3000, 160, 112, 16, 3
    sc, raw = _raw_scene(scenes, P, 401, M, deg)
    cam = scenes.camera(1, 4, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    use = dict(motion_res=True, rot_res=True, trbf=True, shs_res=True)
    g = torch.from_numpy(scenes.upstream_grad(H, W, 402)).to(gpu)
    rng = np.random.default_rng(403)
    gD = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    gA = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    outs, grads = [], []
    for rep in range(3):
        t, kw = _tensors(raw, use, gpu)
        m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        if rep == 0:
            o = rast.GaussianRasterizerRaw(rs)(t["xyz"], m2, t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], **kw, return_aux=True)
        else:
            motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(t["xyz"], t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], **kw)
            o = rast.GaussianRasterizer(rs)(means3D=motion, means2D=m2, opacities=opa, shs=shs, scales=scale, rotations=rot, return_aux=True)
        ((o[0] * g).sum() + (o[3] * gD).sum() + (o[4] * gA).sum()).backward()
        torch.cuda.synchronize()
        outs.append(o); grads.append(dict({k: t[k].grad for k in t}, m2=m2.grad))
    for k in range(5):
        assert np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])), k
    for k in grads[0]:
        a, b, b2 = grads[0][k], grads[1][k], grads[2][k]
        sl = slice(1, None) if k in ("rotation", "rot_res") else slice(None)     # row 0: a zero quaternion, x / eps
        _close(a[sl], b[sl], ref32=b2[sl], what=k)


def test_full_size_under_the_list_cut(scenes, rast, gpu):
    P, W, H = 3_000_000, 1920, 1080
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    rng = np.random.default_rng(9)
    gC = torch.from_numpy(scenes.upstream_grad(H, W, 1)).to(gpu)
    gD = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    gA = torch.from_numpy(rng.normal(size=(1, H, W)).astype(np.float32) / (H * W)).to(gpu)
    _state(rast, rs, sc, gpu, P, W, H)                           # the pose's first render: its cut depths are remembered
    out, st = _state(rast, rs, sc, gpu, P, W, H)
    assert rast._C.context_query("last_late") > 0, "the second render of the pose was expected to run under the list cut"
    acc, alpha = out[7], out[8]
    assert np.array_equal(_bits(alpha.reshape(H, W)), _bits(1.0 - st["final_T"].reshape(H, W)))
    z = st["depths"].reshape(P, 1).expand(P, 3).contiguous()
    rs0 = settings_from(rast, cam, sc, gpu, bg=np.zeros(3, np.float32))
    plain, _ = _state(rast, rs0, sc, gpu, P, W, H, colors=z, aux=False)
    assert np.array_equal(_bits(acc[0]), _bits(plain[1][0]))
    del out, st, plain, z
    # gradients: finite, and a retain_graph second backward gives the first one's
    t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    _render(rast, rs, _leaves(sc, gpu), torch.zeros((P, 3), device=gpu))          # (the pose again: the autograd render is a cut one)
    c, _, _, acc, alpha = _render(rast, rs, t, m2, return_aux=True)
    assert rast._C.context_query("last_late") > 0
    loss = (c * gC).sum() + (acc * gD).sum() + (alpha * gA).sum()
    loss.backward(retain_graph=True)
    first = {n: t[n].grad.clone() for n in LEAVES}
    first_m2 = m2.grad.clone()
    for n in LEAVES:
        assert bool(torch.isfinite(first[n]).all()), n
        t[n].grad = None
    m2.grad = None
    loss.backward()
    torch.cuda.synchronize()
    for n in LEAVES:
        _close(t[n].grad, first[n], what=n)
    _close(m2.grad, first_m2, what="means2D")
