"""-m gpu: the stand-alone projection (fused_project.project_gaussians / screen_flow; include/gsrast.h: gsrast_project_forward / _backward,
csrc/gsrast_project.h) against the renderer's own state, bit for bit, and against tests/project_math.py -- torch fp64 on
tests/math_renderer.project_gaussians, with its fp32 replay as the floor of conftest.grad_tol.

Scenes (project_math.SCENES): the six edge_scenes.CASES (332-1532 Gaussians, images 50 x 37 to 96 x 64, needles, near-plane rows, frustum-
clamped rows, a cov3D case, scale_modifier 0.7) and contrib_math.CASES a and b (b: 1726 of 2000 rows culled).  Every test prints its figures
before it asserts."""
import numpy as np
import pytest
import torch

import project_math as pjm
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fp():
    import fused_project
    return fused_project


def _t(a, gpu, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu).requires_grad_(grad)


def _np(x):
    return x.detach().double().cpu().numpy()


def _bits(x):
    return x.detach().contiguous().cpu().numpy().view(np.uint32 if x.dtype == torch.float32 else np.int32)


def _inputs(ref, gpu, grad=False, rows=None):
    """{leaf: device tensor} of a scene (its first `rows` rows), and the keyword arguments project_gaussians takes them as."""
    cut = slice(None) if rows is None else slice(0, rows)
    x = {n: _t(ref["sc"][n][cut], gpu, grad) for n in ref["leaves"]}
    kw = dict(cov3D_precomp=x["cov3D"]) if "cov3D" in x else dict(scales=x["scales"], rotations=x["rotations"])
    return x, kw


def _project(fp, rast, gpu, ref, aa=True, grad=False, rows=None, rs=None):
    x, kw = _inputs(ref, gpu, grad, rows)
    rs = rs if rs is not None else settings_from(rast, ref["cam"], ref["sc"], gpu)
    return fp.project_gaussians(x["means3D"], raster_settings=rs, antialiasing=aa, **kw), x, rs


def _backward(p, up, gpu, rows=None):
    cut = slice(None) if rows is None else slice(0, rows)
    torch.autograd.backward([getattr(p, k) for k in pjm.OUTPUTS], [_t(up[k][cut], gpu) for k in pjm.OUTPUTS])


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1. bit-equality with the renderer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialiasing"])
@pytest.mark.parametrize("name", pjm.SCENES)
def test_the_projection_is_the_renderers_bit_for_bit(rast, fp, gpu, name, aa):
    ref = pjm.reference(name)
    sc, P = ref["sc"], ref["sc"]["means3D"].shape[0]
    p, x, rs = _project(fp, rast, gpu, ref, aa=aa)
    e = torch.empty(0)
    cov = "cov3D" in x
    opac = _t(sc["opacities"], gpu)
    with torch.no_grad():
        out = rast._C.rasterize_gaussians(
            rs.bg, x["means3D"], _t(sc["rgb"], gpu) if cov else e, opac, e if cov else x["scales"], e if cov else x["rotations"], rs.scale_modifier,
            x["cov3D"] if cov else e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width,
            e if cov else _t(sc["shs"], gpu), rs.sh_degree, rs.campos, False, antialiasing=aa)
        st = rast._C.debug_export(P, out[0], rs.image_width, rs.image_height, out[3], out[4], out[5])
    torch.cuda.synchronize()
    vis = p.radii > 0
    print(f"{name} aa={aa}: {int(vis.sum())} of {P} rows visible, scale_modifier {rs.scale_modifier}")
    assert 0 < int(vis.sum()) < P
    assert torch.equal(p.radii, out[2])                                                         # every row
    assert _same_bits(p.means2D[vis], st["means2D"][vis]) and _same_bits(p.depths[vis], st["depths"][vis])
    assert _same_bits(p.conics[vis], st["conic_opacity"][vis, :3])
    if aa:
        assert _same_bits((opac[:, 0] * p.compensation)[vis], st["conic_opacity"][vis, 3])      # one fp32 product
    else:
        assert p.compensation is None
    for k in pjm.OUTPUTS[:3] + (("compensation",) if aa else ()):                               # a culled row is exactly +0.0
        assert not _bits(getattr(p, k)[~vis]).any(), k


# ---- 2. values against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pjm.SCENES)
def test_values_against_fp64(rast, fp, gpu, name):
    ref = pjm.reference(name)
    r64, r32 = ref["r64"], ref["r32"]
    p, _, _ = _project(fp, rast, gpu, ref)
    for k in pjm.OUTPUTS:
        err, tol = np.abs(_np(getattr(p, k)) - r64["values"][k]), grad_tol(r64["values"][k], r32["values"][k])
        print(f"{name} {k}: max|err| {err.max():.3e} max|ref| {np.abs(r64['values'][k]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (name, k, float(err.max()), float((err / tol).max()))
    firm = pjm.radius_firm(r64["disc"])
    print(f"{name} radii: {int((~firm).sum())} of {len(firm)} rows left out ({(~firm).mean():.4f})")
    assert (~firm).mean() <= 0.02
    assert np.array_equal(p.radii.cpu().numpy().astype(np.int64)[firm], r64["disc"]["radius"][firm])


# ---- 3. gradients -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pjm.SCENES)
def test_gradients_against_fp64(rast, fp, gpu, name):
    """Random upstream on all four outputs (project_math.upstream); every leaf within conftest.grad_tol(ref, ref32), the frustum-clamped
    rows once more as a tensor of their own, culled rows exactly zero -- and the other clamp convention (clamp_grad="true") outside the
    same bar on the clamped rows."""
    ref = pjm.reference(name)
    r64, r32, true64, true32 = ref["r64"], ref["r32"], ref["true64"], ref["true32"]
    p, x, _ = _project(fp, rast, gpu, ref, grad=True)
    _backward(p, ref["up"], gpu)
    torch.cuda.synchronize()
    vis, cl = r64["vis"], r64["disc"]["clamped"] & r64["vis"]
    assert np.array_equal((p.radii > 0).cpu().numpy(), vis), "a row's visibility differs from the fp64 decision"
    assert ("cov3D" in x) == (name == "d_precomp_colour_cov3D")
    for n in ref["leaves"]:
        got, want = _np(x[n].grad), r64["grads"][n]
        for what, rows in (("all rows", slice(None)), ("clamped rows", cl)):
            if what == "clamped rows" and not cl.any():
                continue
            err, tol = np.abs(got[rows] - want[rows]), grad_tol(want[rows], r32["grads"][n][rows])
            print(f"{name} dL/d{n} {what}: max|err| {err.max():.3e} max|ref| {np.abs(want[rows]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
            assert (err <= tol).all(), (name, n, what, float(err.max()), float((err / tol).max()))
        assert np.abs(want).max() > 0 and not _bits(x[n].grad[torch.as_tensor(~vis)]).any(), (name, n)
    if cl.any():
        other = true64["grads"]["means3D"][cl]
        beyond = np.abs(_np(x["means3D"].grad)[cl] - other) > grad_tol(other, true32["grads"]["means3D"][cl])
        print(f"{name}: {int(cl.sum())} clamped rows, {int(beyond.sum())} entries outside the bar around the other convention")
        assert beyond.any()                  # the same comparison against the other convention fails


# ---- 4. row counts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(scenes):
    """4200 Gaussians at 96 x 64, every fifth pushed out to four times its distance from the centre (off screen, or behind the camera):
    the rows the wave and workgroup tails are cut from, culled lanes among the visible ones in every wave."""
    sc, cam = scenes.synth(4200, 5, sh_degree=0, scale_mul=2.0), scenes.camera(1, 5, 96, 64)
    sc["means3D"][2::5] *= 4.0
    return dict(sc=sc, cam=cam, leaves=("means3D", "scales", "rotations"), up=pjm.upstream({k: np.ones(s, np.float32) for k, s in zip(
        pjm.OUTPUTS, ((4200, 2), (4200,), (4200, 3), (4200,)))}))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4099])
def test_row_counts(rast, fp, gpu, big, n):
    full, xf, rs = _project(fp, rast, gpu, big, grad=True)
    _backward(full, big["up"], gpu)
    p, x, _ = _project(fp, rast, gpu, big, grad=True, rows=n, rs=rs)
    _backward(p, big["up"], gpu, rows=n)
    torch.cuda.synchronize()
    assert 0 < int((full.radii > 0).sum()) < 4200
    for k in pjm.OUTPUTS + ("radii",):
        assert getattr(p, k).shape[0] == n and _same_bits(getattr(p, k), getattr(full, k)[:n]), k
    for name in big["leaves"]:
        assert x[name].grad.shape == x[name].shape and _same_bits(x[name].grad, xf[name].grad[:n]), name


# ---- 5. the autograd surface --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b_deg1_white_50x37", "d_precomp_colour_cov3D"])
def test_autograd_surface(rast, fp, gpu, name):
    ref = pjm.reference(name)
    up = ref["up"]
    full, xf, rs = _project(fp, rast, gpu, ref, grad=True)
    _backward(full, up, gpu)
    # two runs are bit-equal, values and gradients
    again, xa, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs)
    _backward(again, up, gpu)
    assert all(_same_bits(getattr(full, k), getattr(again, k)) for k in pjm.OUTPUTS + ("radii",))
    assert all(_same_bits(xf[n].grad, xa[n].grad) for n in ref["leaves"])
    assert full.radii.dtype == torch.int32 and not full.radii.requires_grad and full.means2D.requires_grad
    # gradients go only to the leaves that require them
    for wanted in ref["leaves"]:
        x, kw = _inputs(ref, gpu)
        x[wanted].requires_grad_(True)
        p = fp.project_gaussians(x["means3D"], raster_settings=rs, antialiasing=True, **kw)
        _backward(p, up, gpu)
        assert _same_bits(x[wanted].grad, xf[wanted].grad) and all(x[n].grad is None for n in ref["leaves"] if n != wanted), wanted
    # an unused output counts as zero upstream: the sum of the four single-output gradients is the joint one, up to the adds' rounding
    parts = []
    for k in pjm.OUTPUTS:
        p, x, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs)
        getattr(p, k).backward(_t(up[k], gpu))
        parts.append(_np(x["means3D"].grad))
    joint = _np(xf["means3D"].grad)
    assert all(np.abs(q).max() > 0 for q in parts) and np.abs(sum(parts) - joint).max() <= 1e-5 * np.abs(joint).max()
    # without antialiasing: no compensation, the other three outputs and their gradients unchanged in value
    p, x, _ = _project(fp, rast, gpu, ref, aa=False, grad=True, rs=rs)
    torch.autograd.backward([p.means2D, p.depths, p.conics], [_t(up[k], gpu) for k in pjm.OUTPUTS[:3]])
    assert p.compensation is None and all(_same_bits(getattr(p, k), getattr(full, k)) for k in ("means2D", "depths", "conics", "radii"))
    assert np.abs(_np(x["means3D"].grad) - (joint - parts[3])).max() <= 1e-5 * np.abs(joint).max()
    # no_grad: values only
    with torch.no_grad():
        p, _, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs)
    assert not p.means2D.requires_grad and all(_same_bits(getattr(p, k), getattr(full, k)) for k in pjm.OUTPUTS + ("radii",))
    # non-contiguous upstream gradients
    p, x, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs)
    wide = {k: torch.stack([_t(up[k], gpu), torch.zeros_like(_t(up[k], gpu))], dim=-1)[..., 0] for k in pjm.OUTPUTS}
    assert not wide["conics"].is_contiguous()
    torch.autograd.backward([getattr(p, k) for k in pjm.OUTPUTS], [wide[k] for k in pjm.OUTPUTS])
    assert all(_same_bits(x[n].grad, xf[n].grad) for n in ref["leaves"])
    # a double backward raises
    p, x, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs)
    (g,) = torch.autograd.grad(p.means2D, x["means3D"], _t(up["means2D"], gpu, True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # camera tensors that require grad: the call works, they get nothing
    rs_g = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True))
    p, x, _ = _project(fp, rast, gpu, ref, grad=True, rs=rs_g)
    _backward(p, up, gpu)
    assert rs_g.viewmatrix.grad is None and rs_g.projmatrix.grad is None and _same_bits(x["means3D"].grad, xf["means3D"].grad)
    # a NaN mean in one row: that row is culled with zero outputs and zero gradients, every other row keeps its bits
    row = int(torch.nonzero(full.radii > 0)[3])
    bad = dict(ref, sc=dict(ref["sc"], means3D=ref["sc"]["means3D"].copy()))
    bad["sc"]["means3D"][row, 1] = np.nan
    p, x, _ = _project(fp, rast, gpu, bad, grad=True, rs=rs)
    _backward(p, up, gpu)
    torch.cuda.synchronize()
    others = torch.arange(len(full.radii), device=gpu) != row
    assert int(p.radii[row]) == 0 and all(not _bits(getattr(p, k)[row]).any() for k in pjm.OUTPUTS)
    assert all(_same_bits(getattr(p, k)[others], getattr(full, k)[others]) for k in pjm.OUTPUTS + ("radii",))
    for n in ref["leaves"]:
        assert not _bits(x[n].grad[row]).any() and _same_bits(x[n].grad[others], xf[n].grad[others]), n
    # tensors on the host beside tensors on the device
    x, kw = _inputs(ref, gpu)
    with pytest.raises(RuntimeError, match="GPU"):
        fp.project_gaussians(x["means3D"], raster_settings=rs, **{k: v.cpu() for k, v in kw.items()})
    with pytest.raises(RuntimeError, match="viewmatrix is on"):
        fp.project_gaussians(x["means3D"], raster_settings=rs._replace(viewmatrix=rs.viewmatrix.cpu()), **kw)


# ---- 6. end to end: two projections -> screen_flow -> features= -> L1 against a target flow map ---------------------------------------
def test_flow_rendered_through_features_end_to_end(rast, fp, gpu):
    ref = pjm.flow_reference()
    sc, cam, r64, r32 = ref["sc"], ref["cam"], ref["r64"], ref["r32"]
    rs = settings_from(rast, cam, sc, gpu)
    m0 = _t(sc["means3D"], gpu, True)
    m1 = _t((sc["means3D"].astype(np.float64) + np.asarray(pjm.FLOW_SHIFT)).astype(np.float32), gpu, True)
    s, q, o, shs = (_t(sc[n], gpu) for n in ("scales", "rotations", "opacities", "shs"))
    p0 = fp.project_gaussians(m0, s, q, raster_settings=rs)
    p1 = fp.project_gaussians(m1, s, q, raster_settings=rs)
    flow, valid = fp.screen_flow(p0, p1)
    out = rast.GaussianRasterizer(rs)(means3D=m0, means2D=torch.zeros((len(m0), 3), device=gpu, requires_grad=True), opacities=o, shs=shs, scales=s,
                                      rotations=q, features=flow)
    fmap = out[-1]
    ((fmap - _t(ref["target"], gpu)).abs() * _t(ref["keep"], gpu)).sum().backward()
    torch.cuda.synchronize()
    keep = ref["keep"] > 0
    print(f"flow: {int(valid.sum())} of {len(m0)} rows valid, {keep.mean():.4f} of the pixels kept, max|map| {np.abs(r64['map']).max():.3f} px, "
          f"map max|err| {np.abs(_np(fmap) - r64['map'])[:, keep].max():.3e}")
    assert np.array_equal(valid.cpu().numpy(), r64["valid"]) and keep.mean() > 0.95
    assert np.abs(_np(flow) - r64["flow"]).max() <= 1e-4 * np.abs(r64["flow"]).max()
    for name, leaf in (("m0", m0), ("m1", m1)):
        want = r64["grads"][name]
        err, tol = np.abs(_np(leaf.grad) - want), grad_tol(want, r32["grads"][name])
        print(f"flow dL/d{name}: max|err| {err.max():.3e} max|ref| {np.abs(want).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
        assert np.abs(want).max() > 0 and (err <= tol).all(), (name, float(err.max()), float((err / tol).max()))
