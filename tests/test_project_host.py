"""CPU: the stand-alone projection (fused_project.py; include/gsrast.h: gsrast_project_forward / _backward) -- its fp64 side
(tests/project_math.py) against a plain torch composition written without the shared helper, that the GPU bar can tell the two
frustum-clamp conventions apart, the C surface, and every refusal before a device call.  (The kernels: tests/test_gpu_project.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import capi_header as hdr
import project_math as pjm
from conftest import ROOT, grad_tol

PROFILE_NAMES = 34


# ---- the fp64 side ------------------------------------------------------------------------------------------------------------------
def _plain(sc, cam, up, rows):
    """The projection of `rows` written out in float64 torch, no math_renderer: values and autograd gradients (no frustum clamp, so it
    holds for rows inside 1.3 x the field of view; scale_modifier = 1).  The conic's gradient is scaled by det^2 / (det^2 + 1e-7)."""
    f = lambda a: torch.as_tensor(np.asarray(a, np.float64))      # noqa: E731
    m, s, q = (f(sc[n]).requires_grad_(True) for n in ("means3D", "scales", "rotations"))
    V, Pm = f(cam["viewmatrix"]), f(cam["projmatrix"])
    W, H = int(cam["image_width"]), int(cam["image_height"])
    tanx, tany = float(np.float32(cam["tanfovx"])), float(np.float32(cam["tanfovy"]))
    eps, dil = float(np.float32(0.0000001)), float(np.float32(0.3))
    out = {k: [] for k in pjm.OUTPUTS}
    for i in rows:
        p = torch.cat([m[i], torch.ones(1, dtype=torch.float64)])
        hom, t = p @ Pm, (p @ V)[:3]
        ndc = hom[:2] / (hom[3] + eps)
        pix = torch.stack([((ndc[0] + 1.0) * W - 1.0) * 0.5, ((ndc[1] + 1.0) * H - 1.0) * 0.5])
        r, x, y, z = q[i]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
        M = R * s[i][None, :]
        Sigma = M @ M.T
        fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
        zero = torch.zeros((), dtype=torch.float64)
        J = torch.stack([fx / t[2], zero, -fx * t[0] / (t[2] * t[2]), zero, fy / t[2], -fy * t[1] / (t[2] * t[2])]).reshape(2, 3)
        A = J @ V[:3, :3].T
        cov = A @ Sigma @ A.T
        c00, c01, c11 = cov[0, 0], cov[0, 1], cov[1, 1]
        a, b, c = c00 + dil, c01, c11 + dil
        det0 = (a * c - b * b).detach()
        reg = det0 * det0 / (det0 * det0 + eps)
        ar, br, cr = (v.detach() + reg * (v - v.detach()) for v in (a, b, c))      # the value of v, reg times its gradient
        det = ar * cr - br * br
        out["means2D"].append(pix)
        out["depths"].append(t[2])
        out["conics"].append(torch.stack([cr / det, -br / det, ar / det]))
        out["compensation"].append(torch.sqrt((c00 * c11 - b * b) / (a * c - b * b)))
    vals = {k: torch.stack(v) for k, v in out.items()}
    sum((vals[k] * f(up[k][rows])).sum() for k in pjm.OUTPUTS).backward()
    return {k: v.detach().numpy() for k, v in vals.items()}, dict(means3D=m.grad.numpy(), scales=s.grad.numpy(), rotations=q.grad.numpy())


@pytest.mark.parametrize("name", ["contrib_a", "contrib_b"])
def test_the_wrapper_agrees_with_a_plain_composition(name):
    """Rows that are visible, not frustum-clamped and above the compensation's floor, at scale_modifier = 1: there the reference's
    conventions and the plain derivative coincide (but for the conic's det^2 factor, which the composition restates)."""
    ref = pjm.reference(name)
    r64, disc = ref["r64"], ref["r64"]["disc"]
    assert ref["cam"]["scale_modifier"] == 1.0
    rows = np.nonzero(disc["vis"] & ~disc["clamped"] & ~ref["r64"]["decisions"]["floor"].numpy())[0]
    assert len(rows) >= 100
    vals, grads = _plain(ref["sc"], ref["cam"], ref["up"], rows)
    for k in pjm.OUTPUTS:
        want = r64["values"][k][rows]
        assert np.abs(vals[k] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
    for n in ref["leaves"]:
        want = r64["grads"][n][rows]
        assert np.abs(grads[n][rows] - want).max() <= 1e-12 * np.abs(want).max(), n
        assert not r64["grads"][n][~disc["vis"]].any()      # culled rows: exactly zero


def test_culled_rows_are_zero_and_the_scenes_are_what_the_gpu_tests_assume():
    n_clamped = []
    for name in pjm.SCENES:
        ref = pjm.reference(name)
        vis = ref["r64"]["vis"]
        for k in pjm.OUTPUTS:
            assert not ref["r64"]["values"][k][~vis].any() and not ref["r32"]["values"][k][~vis].any()
        for n in ref["leaves"]:
            assert not ref["r64"]["grads"][n][~vis].any()
        firm = pjm.radius_firm(ref["r64"]["disc"])
        assert (~firm).mean() <= 0.02, (name, (~firm).mean())
        n_clamped.append(int((ref["r64"]["disc"]["clamped"] & vis).sum()))
    assert all(25 <= n <= 40 for n in n_clamped[:6]), n_clamped      # every edge scene has its frustum-clamped rows
    b = pjm.reference("contrib_b")
    assert (~b["r64"]["vis"]).sum() == 1726 and len(b["r64"]["vis"]) == 2000
    assert "cov3D" in pjm.reference("d_precomp_colour_cov3D")["leaves"]
    assert pjm.reference("e_scale_modifier_0.7")["cam"]["scale_modifier"] == 0.7


@pytest.mark.parametrize("name", pjm.SCENES[:6])
def test_the_bar_tells_the_two_clamp_conventions_apart(name):
    """On the frustum-clamped rows clamp_grad="reference" and "true" differ by more than conftest.grad_tol allows: a kernel
    that followed the other convention would fail tests/test_gpu_project.py.  Values are those of one function."""
    ref = pjm.reference(name)
    cl = ref["r64"]["disc"]["clamped"] & ref["r64"]["vis"]
    assert cl.sum() >= 25
    for k in pjm.OUTPUTS:
        assert np.array_equal(ref["r64"]["values"][k], ref["true64"]["values"][k])
    want, other, f32 = ref["r64"]["grads"]["means3D"][cl], ref["true64"]["grads"]["means3D"][cl], ref["r32"]["grads"]["means3D"][cl]
    assert (np.abs(other - want) > grad_tol(want, f32)).sum() >= 25               # the GPU test's bar, on the tensor of the clamped rows
    assert (np.abs(other - want) > grad_tol(other, ref["true32"]["grads"]["means3D"][cl])).sum() >= 25      # ... and around the other convention
    full = np.abs(ref["true64"]["grads"]["means3D"] - ref["r64"]["grads"]["means3D"]) > grad_tol(ref["r64"]["grads"]["means3D"], ref["r32"]["grads"]["means3D"])
    assert full.any() and not full[~cl].any()                                      # ... and on the whole tensor
    assert (np.abs(f32 - want) <= grad_tol(want, f32)).all()                      # ... while fp32 rounding alone stays inside it
    assert np.array_equal(ref["r64"]["grads"]["means3D"][~cl], ref["true64"]["grads"]["means3D"][~cl])


# ---- the C surface --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(rast):
    _C = rast._C
    L = _C.lib()
    text = hdr.text()
    assert L.gsrast_abi_version() == _C.ABI_VERSION == 6 and re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    assert re.search(r"#define\s+GSRAST_PROJECT_ANTIALIAS\s+1u\b", text) and _C.PROJECT_ANTIALIAS == 1
    protos = hdr.prototypes()
    raw = C.CDLL(_C.LIB_PATH)
    for name in ("gsrast_project_forward", "gsrast_project_backward"):
        assert protos[name] == ("int", ["const gsrast_project*", "void*"]) and hasattr(raw, name)
        assert _C.SIGNATURES[name] == (C.c_int, (C.c_void_p, C.c_void_p))
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == PROFILE_NAMES and not any("project" in n for n in names)      # the launches are not in the profile table
    # the descriptor: the header's fields in the header's order, each of its C type's ctypes type
    body = re.search(r"struct gsrast_project\s*\{(.*?)\};", text, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        ctype, field = hdr._declarator(first)
        fields.append((field, ctype))
        fields += [(re.fullmatch(r"\s*\**\s*(\w+)\s*", p).group(1), ctype.rstrip("*") + "*" * p.count("*")) for p in more]
    have = _C.ProjectStruct._fields_
    assert [n for n, _ in fields] == [n for n, _ in have] and len(have) == 26
    for (name, ctype), (_, bound) in zip(fields, have):
        assert bound is hdr.allowed(ctype, _C)[0], (name, ctype, bound)
    assert "gsrast_project.h" in open(os.path.join(ROOT, "saro-gs_amd", "csrc", "gsrast_capi.hip")).read()


def _descriptor(rast, **over):
    one = 256      # any non-NULL, 16-byte aligned value: never dereferenced on the host
    d = rast._C.ProjectStruct()
    d.P, d.width, d.height, d.tanfovx, d.tanfovy, d.scale_modifier = 10, 64, 48, 0.5, 0.4, 1.0
    for k in ("viewmatrix", "projmatrix", "means3D", "scales", "rotations", "means2D", "depths", "conics", "radii", "dL_dmeans2D", "dL_dmeans3D"):
        setattr(d, k, one)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    L = rast._C.lib()
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    AA = rast._C.PROJECT_ANTIALIAS

    def call(fn, **over):
        d = _descriptor(rast, **over)
        return getattr(L, fn)(C.addressof(d), None)

    for who in ("project_forward", "project_backward"):
        fn = "gsrast_" + who
        assert getattr(L, fn)(None, None) == -1 and err() == f"{who}: NULL descriptor"
        assert call(fn, P=-1) == -1 and who in err() and "negative P" in err()
        for bad in (dict(width=0), dict(height=-3)):
            assert call(fn, **bad) == -1 and who in err() and "zero-size image" in err(), bad
        for bad in (dict(tanfovx=0.0), dict(tanfovy=-1.0), dict(tanfovx=float("nan"))):
            assert call(fn, **bad) == -1 and "must be positive" in err(), bad
        assert call(fn, means3D=None) == -1 and "NULL means3D" in err()
        for p in ("viewmatrix", "projmatrix"):
            assert call(fn, **{p: None}) == -1 and "NULL viewmatrix / projmatrix" in err(), p
        for p in ("scales", "rotations"):      # exactly one of the pair
            assert call(fn, **{p: None}) == -1 and "scales and rotations go together" in err(), p
        assert call(fn, scales=None, rotations=None) == -1 and "exactly one of" in err()              # neither form
        assert call(fn, cov3D_precomp=256) == -1 and "exactly one of" in err()                          # both forms
        for bad in (260, 264, 257):
            assert call(fn, rotations=bad) == -1 and "16-byte aligned" in err(), bad
            assert call(fn, dL_drotations=bad) == -1 and "16-byte aligned" in err(), bad
        for flags in (2, 0x10, 0x80000000, AA | 4):
            assert call(fn, flags=flags) == -1 and who in err() and "unknown bits" in err(), flags
        assert call(fn, P=0, compensation=256 if who == "project_forward" else None, flags=AA) == 0      # nothing to launch: OK without a device
        assert call(fn, P=0, scales=None, rotations=None, cov3D_precomp=256) == 0
    for p in ("means2D", "depths", "conics", "radii"):
        assert call("gsrast_project_forward", **{p: None}) == -1 and "NULL means2D / depths / conics / radii" in err(), p
    assert call("gsrast_project_forward", flags=AA) == -1 and "NULL compensation with GSRAST_PROJECT_ANTIALIAS" in err()
    assert call("gsrast_project_forward", compensation=256) == -1 and "compensation without GSRAST_PROJECT_ANTIALIAS" in err()
    assert call("gsrast_project_backward", dL_dcompensation=256) == -1 and "dL_dcompensation without GSRAST_PROJECT_ANTIALIAS" in err()
    assert call("gsrast_project_backward", dL_dmeans3D=None) == -1 and "no gradient output" in err()
    assert call("gsrast_project_backward", P=0, dL_dmeans3D=None, dL_dscales=256) == 0
    assert call("gsrast_project_backward", P=0, dL_dmeans2D=None, dL_dcompensation=256, flags=AA) == 0      # upstream gradients are optional


def test_python_refusals_need_no_device(rast, monkeypatch):
    import fused_project as fp
    monkeypatch.setattr(fp._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    monkeypatch.setattr(fp._C, "launch", lambda *a: pytest.fail("a refusal reached a launch"))
    rs = rast.GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=0.5, tanfovy=0.4, bg=torch.zeros(3), scale_modifier=1.0,
                                            viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False)
    m, s, q, cov = torch.rand(10, 3), torch.rand(10, 3), torch.rand(10, 4), torch.rand(10, 6)
    go = lambda *a, **k: fp.project_gaussians(*a, raster_settings=rs, **k)      # noqa: E731
    for args in ((m,), (m, s), (m, None, q), (m, s, q, cov), (m, s, None, cov)):      # GaussianRasterizer.forward's "exactly one of"
        with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
            go(*args)
    with pytest.raises(RuntimeError, match="GPU"):      # CPU tensors
        go(m, s, q)
    with pytest.raises(RuntimeError, match="GPU"):
        go(m, None, None, cov)
    for bad in (m.double(), m.half(), m.int()):           # not float32
        with pytest.raises(ValueError, match="means3D must be float32"):
            go(bad, s, q)
    with pytest.raises(ValueError, match="scales must be float32"):
        go(m, s.double(), q)
    with pytest.raises(ValueError, match="cov3D_precomp must be float32"):
        go(m, None, None, cov.double())
    for name, args in (("means3D", (torch.rand(10, 4), s, q)), ("means3D", (torch.rand(10), s, q)), ("scales", (m, torch.rand(9, 3), q)),
                       ("rotations", (m, s, torch.rand(10, 3))), ("cov3D_precomp", (m, None, None, torch.rand(10, 5)))):      # wrong shape
        with pytest.raises(ValueError, match=f"{name} must be \\["):
            go(*args)
    for name, args in (("means3D", (torch.rand(3, 10).T, s, q)), ("rotations", (m, s, torch.rand(10, 8)[:, ::2])),
                       ("cov3D_precomp", (m, None, None, torch.rand(6, 10).T))):                                              # not contiguous
        with pytest.raises(ValueError, match=f"{name} must be contiguous"):
            go(*args)
    with pytest.raises(ValueError, match="must be a tensor"):
        go(m, s, [1.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="rows"):
        z = torch.zeros
        fp.screen_flow(fp.Projection(z(4, 2), z(4), z(4, 3), z(4, dtype=torch.int32), None), fp.Projection(z(5, 2), z(5), z(5, 3), z(5, dtype=torch.int32), None))
    assert fp.Projection._fields == ("means2D", "depths", "conics", "radii", "compensation")
    assert "get none" in fp.project_gaussians.__doc__ and "NOT differentiated" in fp.project_gaussians.__doc__


def test_screen_flow_on_the_host():
    """flow = p1.means2D - p0.means2D where both radii > 0, +0.0 elsewhere, differentiable through both (plain torch: runs anywhere)."""
    import fused_project as fp
    a, b = torch.rand(6, 2, requires_grad=True), torch.rand(6, 2, requires_grad=True)
    r0, r1 = torch.tensor([3, 0, 2, 1, 0, 5], dtype=torch.int32), torch.tensor([1, 4, 0, 2, 0, 1], dtype=torch.int32)
    z = torch.zeros
    flow, valid = fp.screen_flow(fp.Projection(a, z(6), z(6, 3), r0, None), fp.Projection(b, z(6), z(6, 3), r1, None))
    assert valid.tolist() == [True, False, False, True, False, True] and valid.dtype == torch.bool
    assert torch.equal(flow[valid], (b - a)[valid]) and not flow[~valid].any() and not torch.signbit(flow[~valid]).any()
    g = torch.rand(6, 2)
    (flow * g).sum().backward()
    assert torch.equal(b.grad, g * valid[:, None]) and torch.equal(a.grad, -g * valid[:, None])
