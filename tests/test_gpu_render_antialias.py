"""-m gpu: anti-aliased rendering (antialiasing=True; include/gsrast.h: GSRAST_RENDER_ANTIALIAS, the flags word of the call records).

    o_eff = o * comp,   comp = sqrt(max(0.000025, det cov2D / det(cov2D + 0.3 I)))      (cov2D before the dilation)

replaces the opacity in every downstream use; nothing else of the state changes.  So an anti-aliased render IS the plain render whose
opacities are the o_eff the forward left in its state -- bit for bit -- and its gradients are that plain render's plus the filter's own
term g * o * d(comp)/d(theta), g = dL/do_eff, with dL/do = g * comp.  tests/aa_math.py holds comp in fp64 (and in fp32, the floor of the
bar); math_renderer checks the whole chain independently on small scenes."""
import numpy as np
import pytest
import torch

import aa_math
import math_renderer as mr
from conftest import grad_tol, settings_from
from edge_scenes import clamped_mask, edge_scene

pytestmark = pytest.mark.gpu

LEAVES = ("means3D", "opacities", "shs", "scales", "rotations")
EPS32 = float(np.finfo(np.float32).eps)


def _setup(scenes, rast, dev, P, W, H, seed=0, bg=None, k=0, V=1):
    sc = scenes.synth(P, seed)
    cam = scenes.camera(k, V, W, H)
    return sc, cam, settings_from(rast, cam, sc, dev, bg=bg)


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)


def _leaves(sc, dev, names=LEAVES):
    return {n: _t(sc[n], dev).requires_grad_(True) for n in names}


def _render(rast, rs, t, m2, aa, aux=False, colors=None, cov3D=None, opacities=None):
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"] if opacities is None else opacities)
    kw.update(colors_precomp=colors) if colors is not None else kw.update(shs=t["shs"])
    kw.update(cov3D_precomp=cov3D) if cov3D is not None else kw.update(scales=t["scales"], rotations=t["rotations"])
    return rast.GaussianRasterizer(rs)(**kw, return_aux=aux, antialiasing=aa)


def _state(rast, rs, t, P, W, H, aa, aux=False, colors=None, cov3D=None, opacities=None):
    """The library's own forward + debug_export of its state.  t: float32 device tensors (LEAVES)."""
    e = torch.empty(0)
    with torch.no_grad():
        out = rast._C.rasterize_gaussians(
            rs.bg, t["means3D"].detach(), e if colors is None else colors.detach(), (t["opacities"] if opacities is None else opacities).detach(),
            e if cov3D is not None else t["scales"].detach(), e if cov3D is not None else t["rotations"].detach(), 1.0,
            e if cov3D is None else cov3D.detach(), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W,
            t["shs"].detach() if colors is None else e, rs.sh_degree, rs.campos, False, aux=aux, antialiasing=aa)
        st = rast._C.debug_export(P, out[0], W, H, out[3], out[4], out[5])
    return out, st


def _o_eff(rast, rs, t, P, W, H, colors=None, cov3D=None):
    """([P,1] o_eff, visible [P] bool numpy): the o_eff an anti-aliased forward leaves in its state (conic_opacity.w); a culled Gaussian
    keeps its opacity (never read)."""
    out, st = _state(rast, rs, t, P, W, H, True, colors=colors, cov3D=cov3D)
    vis = out[2] > 0
    return torch.where(vis[:, None], st["conic_opacity"][:, 3:4], t["opacities"].detach()).contiguous(), vis.cpu().numpy()


def _bits(x):
    return x.detach().contiguous().cpu().numpy().view(np.uint32)


def _np(x):
    return x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _close(a, b, floor=None, what=""):
    """|a - b| <= conftest.grad_tol(b), its fp32 floor taken from `floor` (an array as far from b as fp32 may be)."""
    a, b = _np(a).reshape(-1), _np(b).reshape(-1)
    tol = grad_tol(b, None if floor is None else np.asarray(floor, np.float64).reshape(-1))
    err = np.abs(a - b)
    assert (err <= tol).all(), (what, float(err.max()), float(np.abs(b).max()), int((err > tol).sum()))


def _cov6(sc):
    q = sc["rotations"].astype(np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * sc["scales"].astype(np.float64)[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


# ---- 1. the default path ------------------------------------------------------------------------------------------------------------------
def test_default_path_and_flags_zero_are_todays_calls(scenes, rast, gpu):
    """antialiasing=False is today's call, with the flags word 0 / AUX: outputs bitwise, gradients within the plain backward's own
    run-to-run spread (its float atomics)."""
    P, W, H = 100_000, 800, 800
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    g = _t(scenes.upstream_grad(H, W, 1), gpu)
    rng = np.random.default_rng(2)
    gD, gA = _t(rng.normal(size=(1, H, W)) / (H * W), gpu), _t(rng.normal(size=(1, H, W)) / (H * W), gpu)

    def run(aux, kw):
        t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        out = rast.GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t["shs"], scales=t["scales"],
                                          rotations=t["rotations"], return_aux=aux, **kw)
        loss = (out[0] * g).sum() + (((out[3] * gD).sum() + (out[4] * gA).sum()) if aux else 0.0)
        loss.backward()
        torch.cuda.synchronize()
        return out, {n: t[n].grad for n in LEAVES}, m2.grad

    for aux in (False, True):
        base, base2 = run(aux, {}), run(aux, {})
        runs = [run(aux, dict(antialiasing=False)), run(aux, {})]
        for out, gr, m in runs:
            for k in range(len(out)):
                assert np.array_equal(_bits(out[k]), _bits(base[0][k])), (aux, k)
            for n in LEAVES:
                _close(gr[n], base[1][n], floor=_np(base2[1][n]), what=n)
            _close(m, base[2], floor=_np(base2[2]), what="means2D")


# ---- 2. the state -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,share", [(800, 800, 0.05), (200, 150, 0.4)], ids=["800x800", "200x150"])
def test_state_differs_from_the_plain_one_in_the_opacity_alone(W, H, share, scenes, rast, gpu):
    """The state of an anti-aliased forward: means2D, conic, radii, depths, tiles bit-identical to the plain forward's; conic_opacity.w / o
    is the fp64 comp within what fp32 rounding of the covariance allows.  `share`: visible Gaussians the filter dims by > 1 % (800 x 800)
    resp. > 10 % (200 x 150) -- the same scene seen at a quarter of the resolution, where its splats are a few pixels wide."""
    P = 100_000
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    t = {n: _t(sc[n], gpu) for n in LEAVES}
    (o0, s0), (o1, s1) = _state(rast, rs, t, P, W, H, False), _state(rast, rs, t, P, W, H, True)
    assert np.array_equal(o0[2].cpu().numpy(), o1[2].cpu().numpy())
    vis = (o1[2] > 0).cpu().numpy()
    assert vis.mean() > 0.9
    for k in ("means2D", "depths"):
        assert np.array_equal(_bits(s0[k])[vis], _bits(s1[k])[vis]), k
    assert np.array_equal(_bits(s0["conic_opacity"][:, :3])[vis], _bits(s1["conic_opacity"][:, :3])[vis])
    assert np.array_equal(s0["tiles_touched"].cpu().numpy(), s1["tiles_touched"].cpu().numpy())
    assert np.array_equal(_bits(s0["conic_opacity"][:, 3])[vis], _bits(t["opacities"][:, 0])[vis])      # (the plain state: o itself)
    t64 = {n: torch.as_tensor(sc[n], dtype=torch.float64) for n in ("means3D", "scales", "rotations")}
    c64, _ = aa_math.comp(t64["means3D"], t64["scales"], t64["rotations"], cam)
    cond = aa_math.conditioning(t64["means3D"], t64["scales"], t64["rotations"], cam)
    c64, cond = c64.numpy()[vis], cond.numpy()[vis]
    ratio = _np(s1["conic_opacity"][:, 3])[vis] / _np(t["opacities"][:, 0])[vis]
    tol = 4 * EPS32 + 64 * EPS32 * cond / (2 * c64)
    err = np.abs(ratio - c64)
    assert (err <= tol).all(), (float(err.max()), float((err / tol).max()))
    q = 0.99 if W == 800 else 0.9
    assert float((c64 < q).mean()) >= share, float((c64 < q).mean())


# ---- 3. the exact forward identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp_mode", [0, 2])
@pytest.mark.parametrize("cut", [True, False], ids=["list_cut", "no_list_cut"])
@pytest.mark.parametrize("W,H", [(800, 800), (200, 150)], ids=["800x800", "200x150"])
def test_antialiased_render_is_the_plain_render_at_o_eff(W, H, cut, exp_mode, scenes, rast, gpu):
    P = 100_000
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H, bg=np.array([0.2, 0.5, 0.9], np.float32))
    t = {n: _t(sc[n], gpu) for n in LEAVES}
    rast._C.set_option("exp_mode", exp_mode)
    rast._C.set_option("no_list_cut", 0 if cut else 1)
    rast._C.set_option("list_cut_always", 1 if cut else 0)
    try:
        for _ in range(2):          # (the pose's second render is the one the list cut applies to)
            aa, st = _state(rast, rs, t, P, W, H, True, aux=True)
        late_aa = rast._C.context_query("last_late")
        oe = torch.where((aa[2] > 0)[:, None], st["conic_opacity"][:, 3:4], t["opacities"]).contiguous()
        plain, _ = _state(rast, rs, t, P, W, H, False, aux=True, opacities=oe)
        late_plain = rast._C.context_query("last_late")
    finally:
        rast._C.set_option("exp_mode", 0)
        rast._C.set_option("no_list_cut", 0)
        rast._C.set_option("list_cut_always", 0)
    if cut:
        assert max(late_aa, late_plain) > 0, "the renders were expected to run under the list cut"
    for k in (1, 2, 6, 7, 8):       # colour, radii, median depth, acc_depth, alpha
        assert np.array_equal(_bits(aa[k]), _bits(plain[k])), k
    assert float((oe != t["opacities"]).float().mean()) > 0.5


# ---- 4. the gradients: two-render identity -----------------------------------------------------------------------------------------------
def _filter_term(sel, gO, t, cam, geom, dtype):
    """g * o * d(comp)/d(theta) over the Gaussians `sel` (bool [P]): autograd of sum(g * o * comp(theta)) in fp64 (CPU) or fp32 (device)."""
    dev = torch.device("cpu") if dtype is torch.float64 else t["means3D"].device
    names = ("means3D",) + (("cov3D",) if geom == "cov3D" else ("scales", "rotations"))
    th = {n: t[n].detach().to(dev, dtype).clone().requires_grad_(True) for n in names}
    idx = torch.as_tensor(sel, device=dev).nonzero()[:, 0]
    fn = aa_math.comp if dtype is torch.float64 else aa_math.comp32
    c, _ = fn(th["means3D"][idx], th["scales"][idx] if geom == "sr" else None, th["rotations"][idx] if geom == "sr" else None, cam,
              cov3D=th["cov3D"][idx] if geom == "cov3D" else None)
    w = (gO.detach().to(dev, dtype)[:, 0] * t["opacities"].detach().to(dev, dtype)[:, 0])[idx]
    (w * c).sum().backward()
    full = torch.ones(t["means3D"].shape[0], dtype=dtype, device=dev)
    full[idx] = c.detach()
    return {n: th[n].grad for n in names}, full


def _expect(rast, rs, cam, t_of, P, W, H, g, geom, colour, names):
    """The anti-aliased render's gradients predicted from two plain renders at o_eff (loss = sum(colour * g)).  Returns a dict:
    exp[n]   plain gradient + the fp64 filter term (dL/do: g * fp64 comp)                  -- what the kernels must produce
    floor[n] exp[n] + the plain backward's run-to-run spread + |fp32 - fp64 filter term|     -- the fp32 floor of the bar
    pred32[n] plain gradient + the fp32 filter term (dL/do: g * o_eff / o)                   -- the whole prediction in fp32
    corr64[n] the fp64 filter term alone;  colour: the first plain render's."""
    t0, _ = t_of()
    kw = lambda t: dict(colors=t["rgb"] if colour == "precomp" else None, cov3D=t["cov3D"] if geom == "cov3D" else None)  # noqa: E731
    oe, vis = _o_eff(rast, rs, t0, P, W, H, **kw(t0))
    runs = []
    for _ in range(2):
        tb, mb = t_of()
        oe_leaf = oe.clone().requires_grad_(True)
        c2 = _render(rast, rs, tb, mb, False, opacities=oe_leaf, **kw(tb))[0]
        (c2 * g).sum().backward()
        torch.cuda.synchronize()
        runs.append(({n: tb[n].grad for n in names}, mb.grad, oe_leaf.grad, c2))
    gO = runs[0][2]
    corr64, c64 = _filter_term(vis, gO, t0, cam, geom, torch.float64)
    corr32, _ = _filter_term(vis, gO, t0, cam, geom, torch.float32)
    r = dict(exp={}, floor={}, pred32={}, corr64={}, colour=runs[0][3])
    for n in names:
        a, b = _np(runs[0][0][n]), _np(runs[1][0][n])
        c64n, c32n = (_np(corr64[n]).reshape(a.shape), _np(corr32[n]).reshape(a.shape)) if n in corr64 else (0.0 * a, 0.0 * a)
        r["exp"][n] = a + c64n
        r["floor"][n] = r["exp"][n] + np.abs(b - a) + np.abs(c32n - c64n)
        r["pred32"][n] = a + c32n
        r["corr64"][n] = c64n
    # dL/do = g * comp; the fp32 comp is o_eff / o
    o = t0["opacities"].detach()
    r["exp"]["opacities"] = _np(gO)[:, 0:1] * c64.numpy()[:, None]
    r["pred32"]["opacities"] = _np(gO * (oe / o))
    r["floor"]["opacities"] = r["exp"]["opacities"] + np.abs(r["pred32"]["opacities"] - r["exp"]["opacities"]) + np.abs(_np(runs[1][2] - gO))
    a, b = _np(runs[0][1]), _np(runs[1][1])
    r["exp"]["means2D"], r["floor"]["means2D"], r["pred32"]["means2D"] = a, a + np.abs(b - a), a
    return r


@pytest.mark.parametrize("W,H", [(800, 800), (200, 150)], ids=["800x800", "200x150"])
@pytest.mark.parametrize("colour,geom", [("sh", "sr"), ("precomp", "sr"), ("sh", "cov3D"), ("precomp", "cov3D")])
def test_gradients_equal_the_plain_render_at_o_eff_plus_the_filter_term(colour, geom, W, H, scenes, rast, gpu):
    P = 100_000
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H, seed=3, bg=np.array([0.2, 0.5, 0.9], np.float32))
    g = _t(scenes.upstream_grad(H, W, 6), gpu)
    rng = np.random.default_rng(5)
    rgb = _t(rng.uniform(0.0, 1.0, size=(P, 3)), gpu)
    cov = _t(_cov6(sc), gpu)

    def t_of():
        t = _leaves(sc, gpu)
        t["rgb"] = rgb.clone().requires_grad_(True)
        t["cov3D"] = cov.clone().requires_grad_(True)
        return t, torch.zeros((P, 3), device=gpu, requires_grad=True)

    names = ["means3D"] + (["shs"] if colour == "sh" else ["rgb"]) + (["scales", "rotations"] if geom == "sr" else ["cov3D"])
    ta, ma = t_of()
    kw = dict(colors=ta["rgb"] if colour == "precomp" else None, cov3D=ta["cov3D"] if geom == "cov3D" else None)
    c = _render(rast, rs, ta, ma, True, **kw)[0]
    (c * g).sum().backward()
    torch.cuda.synchronize()
    r = _expect(rast, rs, cam, t_of, P, W, H, g, geom, colour, names)
    assert np.array_equal(_bits(c), _bits(r["colour"]))
    for n in names + ["opacities", "means2D"]:
        assert float(np.abs(r["exp"][n]).max()) > 0.0, n
        _close(ta[n].grad if n != "means2D" else ma.grad, r["exp"][n], floor=r["floor"][n], what=n)
    # (the filter term is not lost in the bar: it moves the geometry gradients by more than the bar allows)
    if W == 200:
        assert any((np.abs(r["corr64"][n]) > grad_tol(r["exp"][n], r["floor"][n])).any() for n in names if n in ("means3D", "scales", "rotations", "cov3D"))


# ---- 5. an independent fp64 check ---------------------------------------------------------------------------------------------------------
SMALL = [dict(P=600, seed=31, W=96, H=64, k=1, V=5, deg=3, smul=0.6, bg=(0.1, 0.2, 0.3)),
         dict(P=400, seed=33, W=64, H=48, k=2, V=6, deg=1, smul=0.8, bg=(1.0, 1.0, 1.0))]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: f"P{c['P']}_{c['W']}x{c['H']}")
def test_against_the_fp64_math_renderer(c, scenes, rast, gpu):
    sc, cam = edge_scene(scenes, c)      # (needles, near-plane Gaussians and Gaussians outside the frustum clamp among them)
    P, W, H, deg = sc["means3D"].shape[0], c["W"], c["H"], c["deg"]
    t64 = {n: torch.as_tensor(np.asarray(sc[n], np.float64)).requires_grad_(True) for n in LEAVES}
    off = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
    vis = mr.project(t64["means3D"].detach(), t64["scales"].detach(), t64["rotations"].detach(), cam)["disc"]["vis"]
    idx = torch.as_tensor(vis).nonzero()[:, 0]
    comp, rho = aa_math.comp(t64["means3D"][idx], t64["scales"][idx], t64["rotations"][idx], cam, clamp_grad="reference")
    assert float((comp < 0.9).double().mean()) > 0.1
    o_eff = t64["opacities"][:, 0].index_put((idx,), t64["opacities"][idx, 0] * comp)[:, None]
    ref = mr.render(t64["means3D"], t64["scales"], t64["rotations"], o_eff, t64["shs"], deg, cam, sc["bg"], ndc_offset=off,
                    clamp_grad="reference")
    amb = ref["ambiguous"]
    assert amb.mean() < 0.05
    g = scenes.upstream_grad(H, W, c["seed"] + 1).astype(np.float64)
    g[:, amb] = 0.0
    (ref["color"] * torch.as_tensor(g)).sum().backward()

    rs = settings_from(rast, cam, sc, gpu)
    g32 = _t(g, gpu)
    t = _leaves(sc, gpu)
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    col, radii, _ = _render(rast, rs, t, m2, True)
    (col * g32).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy() > 0, vis), "radius decision differs: pick another seed"
    keep = ~amb
    np.testing.assert_allclose(_np(col)[:, keep], ref["color"].detach().numpy()[:, keep], rtol=0, atol=4e-6)
    # the fp32 floor: the two-render prediction (plain renders at o_eff + the fp32 filter term)
    def t_of():
        return _leaves(sc, gpu), torch.zeros((P, 3), device=gpu, requires_grad=True)
    pred32 = _expect(rast, rs, cam, t_of, P, W, H, g32, "sr", "sh", ["means3D", "shs", "scales", "rotations"])["pred32"]
    # Gaussians within rounding of the floor are excluded: there the kernel's fp32 rho may fall on either side of it
    cond = aa_math.conditioning(t64["means3D"].detach()[idx], t64["scales"].detach()[idx], t64["rotations"].detach()[idx], cam).numpy()
    near_floor = np.zeros(P, bool)
    near_floor[idx.numpy()] = np.abs(rho.detach().numpy() - aa_math.FLOOR) <= 64 * EPS32 * (cond + 1.0)
    cl = clamped_mask(sc, cam)      # the frustum-clamped rows once more, as a tensor of their own: their gradients are small
    assert (cl & ~near_floor).sum() >= 16
    for n in ("means3D", "opacities", "shs", "scales", "rotations"):
        want = t64[n].grad.numpy().reshape(P, -1)
        got = _np(t[n].grad).reshape(P, -1)
        f32 = _np(pred32[n]).reshape(P, -1)
        for what, sel in ((n, ~near_floor),) + (((n + ", clamped rows", cl & ~near_floor),) if n == "means3D" else ()):
            tol = grad_tol(want[sel], f32[sel])
            assert (np.abs(got[sel] - want[sel]) <= tol).all(), (what, float(np.abs(got[sel] - want[sel]).max()), float(np.abs(want[sel]).max()))
    assert float(np.abs(t64["means3D"].grad.numpy()).max()) > 1e-3
    assert float(np.abs(t64["means3D"].grad.numpy()[cl & ~near_floor]).max()) > 0.0
    want2, got2 = off.grad.numpy(), _np(m2.grad[:, :2])
    assert (np.abs(got2 - want2) <= grad_tol(want2, _np(pred32["means2D"])[:, :2])).all()


# ---- 6. the raw path ---------------------------------------------------------------------------------------------------------------------
def test_raw_path_matches_epilogue_then_rasterizer(scenes, rast, gpu):
    import fused_epilogue
    from test_gpu_raw import _raw_scene, _tensors
    P, W, H, M, deg = 3000, 80, 56, 16, 3      # (half the resolution of the raw tests: splats of a few pixels, where the filter acts)
    sc, raw = _raw_scene(scenes, P, 401, M, deg)
    cam = scenes.camera(1, 4, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    use = dict(motion_res=True, rot_res=True, trbf=True, shs_res=True)
    g = _t(scenes.upstream_grad(H, W, 402), gpu)
    rng = np.random.default_rng(403)
    gD, gA = _t(rng.normal(size=(1, H, W)) / (H * W), gpu), _t(rng.normal(size=(1, H, W)) / (H * W), gpu)
    for aux in (False, True):
        outs, grads = [], []
        for rep in range(3):
            t, kw = _tensors(raw, use, gpu)
            m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
            if rep == 0:
                o = rast.GaussianRasterizerRaw(rs)(t["xyz"], m2, t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], **kw,
                                                   return_aux=aux, antialiasing=True)
            else:
                motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(t["xyz"], t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], **kw)
                o = rast.GaussianRasterizer(rs)(means3D=motion, means2D=m2, opacities=opa, shs=shs, scales=scale, rotations=rot,
                                                return_aux=aux, antialiasing=True)
            loss = (o[0] * g).sum() + (((o[3] * gD).sum() + (o[4] * gA).sum()) if aux else 0.0)
            loss.backward()
            torch.cuda.synchronize()
            outs.append(o); grads.append(dict({k: t[k].grad for k in t}, m2=m2.grad))
        for k in range(len(outs[0])):
            assert np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])), (aux, k)
        for k in grads[0]:
            a, b, b2 = grads[0][k], grads[1][k], grads[2][k]
            sl = slice(1, None) if k in ("rotation", "rot_res") else slice(None)     # row 0: a zero quaternion, x / eps
            _close(a[sl], b[sl], floor=_np(b2[sl]), what=(aux, k))
    # (not vacuous: the anti-aliased raw render differs from the plain one)
    t, kw = _tensors(raw, use, gpu)
    p = rast.GaussianRasterizerRaw(rs)(t["xyz"], torch.zeros((P, 3), device=gpu), t["rotation"], t["scaling"], t["opacity"], t["f_dc"], t["f_rest"], **kw)
    assert not np.array_equal(_bits(p[0]), _bits(outs[0][0]))


# ---- 7. under the list cut, pose table shared across modes -----------------------------------------------------------------------------
def test_list_cut_and_pose_table_shared_by_plain_and_antialiased_renders(scenes, rast, gpu):
    P, W, H = 1_000_000, 1352, 1014
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    t = {n: _t(sc[n], gpu) for n in LEAVES}
    rast._C.set_option("no_list_cut", 1)
    try:
        ref = {aa: _state(rast, rs, t, P, W, H, aa, aux=True)[0] for aa in (False, True)}
    finally:
        rast._C.set_option("no_list_cut", 0)
    rast._C.set_option("list_cut_always", 1)
    try:
        late = []
        for aa in (False, True, True, False, True):
            out, _ = _state(rast, rs, t, P, W, H, aa, aux=True)
            late.append(rast._C.context_query("last_late"))
            for k in (1, 2, 6, 7, 8):
                assert np.array_equal(_bits(out[k]), _bits(ref[aa][k])), (aa, k)
    finally:
        rast._C.set_option("list_cut_always", 0)
    assert max(late[1:]) > 0, "the renders were expected to run under the list cut"
    assert not np.array_equal(_bits(ref[True][1]), _bits(ref[False][1]))


# ---- 8. two-phase backward and the gradient arena ----------------------------------------------------------------------------------------
def test_two_phase_backward_and_grad_arena(scenes, rast, gpu):
    _C = rast._C
    P, W, H = 100_000, 200, 150
    sc, cam, rs = _setup(scenes, rast, gpu, P, W, H)
    g = _t(scenes.upstream_grad(H, W, 11), gpu)

    def run():
        t = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
        c = _render(rast, rs, t, m2, True)[0]
        c.backward(g)
        torch.cuda.synchronize()
        return {n: t[n].grad.clone() for n in LEAVES}, m2.grad.clone(), t

    base, base_m2, _ = run()
    base2, base2_m2, _ = run()

    def same(gr, m2, what):
        for n in LEAVES:
            _close(gr[n], base[n], floor=_np(base2[n]), what=(what, n))
        _close(m2, base_m2, floor=_np(base2_m2), what=(what, "means2D"))

    for factors in (False, True):
        arena = _C.GradArena(P, 16, gpu, sh_factors=factors, world=1)
        _C.set_grad_arena(arena)
        try:
            for two_phase in ((False, True) if factors else (False,)):
                seen = []
                if two_phase:
                    _C.set_factor_ready_hook(lambda ar: seen.append(1))
                arena.zero_grad()
                try:
                    gr, m2, t = run()
                finally:
                    _C.set_factor_ready_hook(None)
                if factors:
                    assert len(seen) == (1 if two_phase else 0)
                    gr["shs"] = _C.sh_grad_combine(arena, t["means3D"].detach(), arena.factor, 1, 1.0).clone()
                same(gr, m2, ("factors" if factors else "arena", two_phase))
        finally:
            _C.set_grad_arena(None)


# ---- 9. degenerate input ----------------------------------------------------------------------------------------------------------------
def test_needles_on_the_floor(scenes, rast, gpu):
    """Needles with two zero scales: a rank-1 screen-space covariance, fp32 det_cov within rounding of zero -- comp exactly on the
    floor, no covariance term (the gradients are the plain render's at o_eff), nothing non-finite."""
    P, W, H = 3000, 160, 112
    sc = scenes.synth(P, 61, scale_mul=0.8)
    cam = scenes.camera(0, 3, W, H)
    rs = settings_from(rast, cam, sc, gpu)
    n_needle = 40
    rng = np.random.default_rng(62)
    sc["scales"][:n_needle] = np.c_[rng.uniform(0.005, 0.02, n_needle), np.zeros((n_needle, 2))].astype(np.float32)
    sc["means3D"][:n_needle] = rng.uniform(-0.6, 0.6, (n_needle, 3)).astype(np.float32)     # (inside the view)
    t = {n: _t(sc[n], gpu) for n in LEAVES}
    out, st = _state(rast, rs, t, P, W, H, True, aux=True)
    vis = (out[2] > 0).cpu().numpy()
    needle = np.zeros(P, bool); needle[:n_needle] = True
    assert (vis & needle).sum() >= n_needle // 2
    o = sc["opacities"][:, 0].astype(np.float32)
    floor_o = o * np.sqrt(np.float32(aa_math.FLOOR))
    got = st["conic_opacity"][:, 3].cpu().numpy()
    sel = vis & needle
    assert np.array_equal(got[sel].view(np.uint32), floor_o[sel].view(np.uint32))
    assert not np.array_equal(got[vis & ~needle].view(np.uint32), floor_o[vis & ~needle].view(np.uint32))
    for k in (1, 6, 7, 8):
        assert bool(torch.isfinite(out[k]).all()), k
    g = _t(scenes.upstream_grad(H, W, 63), gpu)
    tl = _leaves(sc, gpu); m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    c = _render(rast, rs, tl, m2, True)[0]
    (c * g).sum().backward()
    torch.cuda.synchronize()
    for n in LEAVES:
        assert bool(torch.isfinite(tl[n].grad).all()), n
    assert bool(torch.isfinite(m2.grad).all())

    def t_of():
        return _leaves(sc, gpu), torch.zeros((P, 3), device=gpu, requires_grad=True)
    names = ["means3D", "shs", "scales", "rotations"]
    r = _expect(rast, rs, cam, t_of, P, W, H, g, "sr", "sh", names)
    # the needles' rows: the plain render's gradient at o_eff -- the filter term is zero on the floor
    assert float(np.abs(r["exp"]["opacities"][sel]).max()) > 0.0
    for n in names + ["opacities"]:
        if n in r["corr64"]:
            assert not r["corr64"][n].reshape(P, -1)[sel].any(), n
        _close(_np(tl[n].grad).reshape(P, -1)[sel], r["exp"][n].reshape(P, -1)[sel], floor=r["floor"][n].reshape(P, -1)[sel], what=("needle", n))
