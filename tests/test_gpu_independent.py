"""-m gpu: the HIP renderer through GaussianRasterizer against tests/math_renderer.py (torch fp64, autograd, no tile lists, written from
the mathematics) DIRECTLY -- the plain colour path, which every other -m gpu test compares with oracle/gsrast_oracle.c only.  The
oracle and csrc/gsrast_preprocess.h are one transcription of the reference typed twice; the math renderer shares no derivation with
either.  The oracle appears here only as the fp32 floor of conftest.grad_tol.

Every case is an edge scene (tests/edge_scenes.py: needles, near-plane Gaussians, and Gaussians outside the frustum clamp, whose
dL/dmeans3D is judged a second time as a tensor of its own -- `preprocess_bwd_kernel`'s xgm / ygm branch, backward.cu:172-176, :262-264).

The colour / alpha / depth bars are 4 x the largest |oracle32 - math| over the unambiguous pixels of the six cases (the HIP forward is
bit-equal to the fp32 oracle in exp mode 0, so that is the kernels' own floor), never below the 2e-6 * max(1, max|ref|) of
test_gpu_render_aux.py.  Measured on the CPU (max over the unambiguous pixels; the largest |ref| of the quantity in brackets):

    case   colour (max|ref|)      1 - final_T     median depth: abs (max|ref|), relative
    a      7.25e-07 (0.74)        1.99e-07        1.95e-07 (4.0)   5.5e-07
    b      5.81e-07 (0.78)        9.02e-08        1.94e-07 (3.2)   5.5e-07
    c      1.60e-06 (0.70)        3.05e-07        3.44e-07 (4.9)   4.0e-07
    d      5.08e-07 (0.76)        2.12e-07        2.32e-07 (3.9)   8.6e-08
    e      1.59e-06 (0.82)        5.75e-07        2.64e-07 (15)    7.4e-07
    f      1.69e-06 (0.76)        3.53e-08        1.98e-07 (3.1)   8.1e-08

(how: edge_scenes.reference, with oracle.render's fp32 build standing where the device stands in the test; tools/README.md).  So the colour
bar is 4 x 1.69e-06 = 6.8e-06 and the alpha bar 4 x 5.75e-07 = 2.3e-06, both above the aux test's 2e-6.  The median depth is ONE Gaussian's
view-space z, the fp32 value of an fp64 one: the aux test's form, rtol = 1e-5 with atol = 2e-6 * max(1, max|ref|) (the largest relative
error above belongs to a near-plane Gaussian at z = 0.26)."""
import numpy as np
import pytest
import torch

import math_renderer as mr
from conftest import grad_tol, settings_from
from edge_scenes import CASES, case_inputs as _case_inputs, reference as _reference, t64 as _t64      # noqa: F401

pytestmark = pytest.mark.gpu

COLOUR_FLOOR, ALPHA_FLOOR = 1.69e-06, 5.75e-07      # measured, see the docstring


def _bar(floor, ref):
    return max(4.0 * floor, 2e-6 * max(1.0, float(np.abs(ref).max())))


ORACLE_KEYS = dict(means3D="dL_dmeans3D", opacities="dL_dopacity", shs="dL_dsh", rgb="dL_dcolors", cov3D="dL_dcov3D", scales="dL_dscales",
                   rotations="dL_drotations")


def _oracle32(orc, r):
    """The fp32 build of the oracle on the case: its gradients are the fp32 floor of conftest.grad_tol."""
    sc = r["sc"]
    o = orc.render(sc, r["cam"], r["g"], colors_precomp=sc.get("rgb"), cov3D_precomp=sc.get("cov3D"))
    f = {n: o[ORACLE_KEYS[n]].astype(np.float64).reshape(r["want"][n].shape) for n in r["names"]}
    f["means2D"] = o["dL_dmeans2D"][:, :2].astype(np.float64)
    return o, f


def _assert_non_vacuous(c, r):
    out, want = r["out"], r["want"]["means3D"]
    assert (~r["keep"]).mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    assert out["min_depth_gap"] > 2e-6, "two Gaussians closer in depth than fp32 resolves: pick another seed"
    assert out["n_live"].max() >= 5
    assert float(np.abs(want).max()) > 1e-3
    cl = r["clamped"]
    assert int((np.abs(want[cl]).max(axis=1) > 0).sum()) >= 16, "too few clamped Gaussians with a gradient"
    assert float(np.abs(want[cl]).max()) > 1e-3 * float(np.abs(want).max()), "the clamped rows' own bar would be vacuous"
    if c.get("long"):
        assert out["tile_list_max"] > 256 and out["n_live"].max() > 128
    if c.get("saturate"):
        assert out["clamped_pairs"] > 0 and int((out["stopped"] & r["keep"]).sum()) >= 100
    if c.get("dark"):
        vis = out["proj"]["disc"]["vis"]
        assert float((_channel_clamped(c, r)[vis].any(axis=1)).mean()) >= 0.2


def _channel_clamped(c, r):
    """bool [P, 3]: SH colour + 0.5 below zero (forward.cu:60-70), firmly (not within fp32 rounding of it)."""
    sc = r["sc"]
    d = _t64(sc["means3D"]) - _t64(r["cam"]["campos"])
    raw = (mr.sh_colour(c["deg"], _t64(sc["shs"]), d / torch.linalg.norm(d, dim=1, keepdim=True)) + 0.5).numpy()
    return raw < -1e-5


def _compare(c, r, got, f32, radii, colour, depth, alpha):
    """got / f32: gradients of the side under test and of the fp32 oracle, float64 numpy, by leaf name (+ "means2D")."""
    out, keep, want = r["out"], r["keep"], r["want"]
    d = out["proj"]["disc"]
    assert np.array_equal(radii > 0, d["vis"]), "radius decision differs: pick another seed"
    firm = (d["radius_margin"] > 1e-4) & (d["rect_margin"] > 1e-5)
    assert firm.mean() > 0.98
    np.testing.assert_array_equal(radii[firm], d["radius"][firm])
    ref = out["color"].detach().numpy()
    np.testing.assert_allclose(colour[:, keep], ref[:, keep], rtol=0, atol=_bar(COLOUR_FLOOR, ref))
    if alpha is not None:
        np.testing.assert_allclose(alpha[keep], 1.0 - out["final_T"].detach().numpy()[keep], rtol=0, atol=_bar(ALPHA_FLOOR, 1.0))
    dref = out["depth"].numpy()
    np.testing.assert_allclose(depth[keep], dref[keep], rtol=1e-5, atol=2e-6 * max(1.0, float(np.abs(dref).max())))
    for n in r["names"] + ["means2D"]:
        err = np.abs(got[n] - want[n])
        assert (err <= grad_tol(want[n], f32[n])).all(), (n, float(err.max()), float(np.abs(want[n]).max()))
    cl = r["clamped"]
    err = np.abs(got["means3D"][cl] - want["means3D"][cl])
    assert (err <= grad_tol(want["means3D"][cl], f32["means3D"][cl])).all(), ("means3D, clamped rows", float(err.max()), float(np.abs(want["means3D"][cl]).max()))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_hip_against_the_fp64_math_renderer(c, scenes, rast, orc, gpu):
    r = _reference(scenes, c)
    _assert_non_vacuous(c, r)
    sc, cam, names = r["sc"], r["cam"], r["names"]
    P = sc["means3D"].shape[0]
    rs = settings_from(rast, cam, sc, gpu)
    t = {n: torch.as_tensor(np.ascontiguousarray(sc[n]), dtype=torch.float32, device=gpu).requires_grad_(True) for n in names}
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"])
    kw.update(colors_precomp=t["rgb"], cov3D_precomp=t["cov3D"]) if c.get("precomp") else kw.update(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    res = rast.GaussianRasterizer(rs)(**kw, return_aux=bool(c.get("aux")))
    (res[0] * torch.from_numpy(r["g"]).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    got = {n: t[n].grad.detach().double().cpu().numpy().reshape(r["want"][n].shape) for n in names}
    got["means2D"] = m2.grad[:, :2].double().cpu().numpy()
    _, f32 = _oracle32(orc, r)
    _compare(c, r, got, f32, res[1].cpu().numpy(), res[0].detach().double().cpu().numpy(), res[2][0].detach().double().cpu().numpy(),
             res[4][0].detach().double().cpu().numpy() if c.get("aux") else None)
    if c.get("dark"):      # a channel clamped at zero passes no gradient to its coefficients: exactly none
        dead = _channel_clamped(c, r)
        assert dead.sum() > 0 and not got["shs"].transpose(0, 2, 1)[dead].any()
