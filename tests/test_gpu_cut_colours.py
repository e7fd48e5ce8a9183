"""-m gpu: the list cut's colour kernels at every colour input and degree, against the CPU oracle.

Under the list cut (include/gsrast.h: options.no_list_cut) the forward evaluates colours with preprocess_color_compact_kernel
(csrc/gsrast_preprocess.h) for the EARLY Gaussians only; the late candidates' colours come from a second, predicated launch of that kernel over
`skip2`, and after a redo the whole set is coloured by the plain kernel: the three color_kernels(...) call sites of csrc/gsrast_capi.hip
(tests/variant_table.py: COLOR_LAUNCHES / COLOR_CALLS name the case below that reaches each).  The compacting kernel has code of its own for
colors_precomp, rows of more than PP_SH_MAX floats (read in place), rows that are no multiple of four floats, an unaligned `shs` base,
shdA == nullptr (degree 0 or a forward nobody differentiates), the RAW gathers with and without shs_res, the predicated launch, and a last
1024-Gaussian block that holds a single Gaussian.  All of them run here under the plan a caller of the product gets: debug_state = 0.

Scene (one throughout): scenes.synth(33 * 1024 + 1, 977, sh_degree=deg, scale_mul=1.3), opacity logits + 2, scenes.camera(2, 5, 200, 150):
13 x 10 ragged tiles, P just above the bucket depth sort's minimum (the cut rides on it), 33 blocks of the compacting kernel and one Gaussian
in the 34th.  On the CPU oracle (fp32 build): R = 333 863, 33 458 visible rows, 5 409 rows with a non-zero gradient, every pixel of 129 of
the 130 tiles stops before the end of its list (mean list length 2568, mean deepest consumed entry 413).  Asserted per case from the oracle:
at least 100 fully stopped tiles, at least half of the visible rows with an all-zero gradient.

Per case, with poisoned state buffers (every buffer handed out full of 0xFF bytes), list_cut_always = 1, debug_state = 0:
  visit 0     direct call, no_list_cut = 1: R, colour, depth, radii, and every visible row's exported rgb / clamped bit-equal to the oracle;
  visits 1, 2 direct calls under the cut: last_late > 0; colour, depth, radii, n_contrib, final_T bit-equal to visit 0; 0 < n_poison <= last_late,
              n_poison = the visible rows whose exported rgb is still the poison (gsrast_debug_export copies the colour record of every row with
              tiles != 0 verbatim): the proof that the compacting kernel ran and skipped them; every other visible row's rgb / clamped is the oracle's;
  visit 3     the module call under the cut, every leaf requiring grad: colour bit-equal; gradients at the bar of test_gpu_parity._check_grads
              (conftest.grad_tol) against the fp64 oracle; every row whose fp64 gradient is all-zero in dL_dmeans2D and dL_dopacity is exactly
              zero and finite in every HIP gradient -- a late Gaussian's poisoned colour, clamp byte and direction derivatives reach nothing;
  visit 4     the same call under torch.no_grad(): shdA == nullptr in the compacting kernel; the image is bit-equal.
The two other call sites have a test each: the completion pass's predicated launch (test_fallback_colours_the_late_gaussians: a scene turned
transparent) and the plain kernels behind the compacting one in front of a redo (test_redo_colours_every_gaussian: a scene grown past the
speculative launch's capacity, in a context of its own); a forward takes one or the other, never both.
The raw cases render the oracle on the activated attributes the device produced (fused_epilogue.activate_gaussians, itself checked against
oracle/epilogue_oracle.py by tests/test_epilogue.py) and chain the gradients back through epilogue_oracle.backward, as tests/test_gpu_raw.py.

Measured on the MI355X (one run; every test prints its figures)
----------------------------------------------------------------
test_cut_colours_against_the_oracle: last_late = 18 806 and n_poison = 18 806 in every case and on every visit 1 - 4 (the geometry is the same
scene's; every late Gaussian is a visible one).  Worst gradient err / bar of visit 3, and the tensor that has it (float atomics: a figure
moves by a few hundredths from run to run):
    shs_M16_deg0   0.122 rotations     shs_M1_deg0    0.118 rotations     shs_M16_deg3_unaligned     0.065 shs
    shs_M16_deg1   0.135 rotations     shs_M4_deg1    0.111 means3D       colors_precomp             0.117 rotations
    shs_M16_deg2   0.089 scales        shs_M9_deg2    0.084 means2D       cov3D_precomp              0.069 cov3D_precomp
    shs_M16_deg3   0.065 shs           shs_M25_deg3   0.114 rotations     colors_and_cov3D_precomp   0.082 means2D
    raw_M4_deg1    0.078 scaling       raw_M4_deg1_shs_res   0.067 f_dc
test_fallback_colours_the_late_gaussians: under the stale cut the thin scene's forward finds 20 281 late Gaussians, cut_fallbacks rises by one,
n_poison = 0 afterwards (every Gaussian was coloured after all); the module call that follows runs uncut (last_late 0).  Worst gradient
err / bar on the thin scene: shs_M16_deg1 0.151 rotations, shs_M25_deg3 0.130 rotations, colors_precomp 0.121 means2D.
test_redo_colours_every_gaussian, the same in the three cases: the module call on the 1.6 x scene finds 16 135 late Gaussians, redo_count 0 -> 1;
the direct call on the 2.6 x scene 14 620, redo_count 1 -> 2, n_poison 0 (18 806 under the cut that held).  Worst gradient err / bar on the
1.6 x scene: shs_M16_deg2 0.072 scales, shs_M25_deg3 0.083 rotations, colors_precomp 0.095 rotations.
test_camera_path_under_the_predicted_cut: last_late per frame (n_poison the same, except on a context's first frames, where it is up to 5 % less)
    shs_M16_deg0     19628 20000 19830 15223 12933 13086 12634 13258 13241 13269 13125 12388
    shs_M25_deg3     16177 16101 14252 13284 11365 11482 11784 11804 11843 11989 11756 11720
    colors_precomp   17382 17509 15677 14270 14158 14690 14265 14010 13277 13237 13243 13334
test_debug_state_masks_the_compacting_kernel: last_late 18 806 with n_poison 0 under debug_state = 1, against 18 806 / 18 806 without.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from conftest import settings_from
from gpu_harness import bits
from test_gpu_parity import _check_grads

pytestmark = pytest.mark.gpu

P, W, H = 33 * 1024 + 1, 200, 150
POISON = np.uint32(0xFFFFFFFF)
DENSE_NAMES = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity", shs="dL_dsh", colors_precomp="dL_dcolors",
                   scales="dL_dscales", rotations="dL_drotations", cov3D_precomp="dL_dcov3D")

# name: M, active degree, and what the case is about
CASES = {
    "shs_M16_deg0": dict(M=16, deg=0), "shs_M16_deg1": dict(M=16, deg=1), "shs_M16_deg2": dict(M=16, deg=2), "shs_M16_deg3": dict(M=16, deg=3),
    "shs_M1_deg0": dict(M=1, deg=0), "shs_M4_deg1": dict(M=4, deg=1), "shs_M9_deg2": dict(M=9, deg=2), "shs_M25_deg3": dict(M=25, deg=3),
    "shs_M16_deg3_unaligned": dict(M=16, deg=3, unaligned=True),
    "colors_precomp": dict(M=16, deg=3, rgb=True), "cov3D_precomp": dict(M=16, deg=3, cov=True),
    "colors_and_cov3D_precomp": dict(M=16, deg=3, rgb=True, cov=True),
    "raw_M4_deg1": dict(M=4, deg=1, raw=True), "raw_M4_deg1_shs_res": dict(M=4, deg=1, raw=True, shs_res=True),
}
FALLBACK_CASES = ("shs_M16_deg1", "shs_M25_deg3", "colors_precomp")
PREDICTED_CASES = ("shs_M16_deg0", "shs_M25_deg3", "colors_precomp")


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


# ---- the cases' inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    """dict(sc, cam, arrays: leaf name -> float32 array, raw, deg, unaligned).  `arrays` are the tensors the HIP call is given."""
    import scenes
    from oracle import oracle as orc
    c = CASES[name]
    M, deg = c["M"], c["deg"]
    sc = scenes.synth(P, 977, sh_degree=deg, scale_mul=1.3)
    sc["opacities"] = (1.0 / (1.0 + np.exp(-(np.log(sc["opacities"] / (1.0 - sc["opacities"])) + 2.0)))).astype(np.float32)
    if c.get("raw"):
        sc["shs"] = np.ascontiguousarray(sc["shs"][:, :M])
    elif M != 16:      # as tests/test_gpu_parity.py::test_sh_row_lengths builds them
        rng = np.random.default_rng(M)
        shs = np.zeros((P, M, 3), np.float32)
        shs[:, 0] = rng.uniform(-1.7, 1.7, size=(P, 3))
        shs[:, 1:] = rng.normal(0, 0.2, size=(P, M - 1, 3))
        sc["shs"] = shs
    cam = scenes.camera(2, 5, W, H)
    out = dict(sc=sc, cam=cam, raw=bool(c.get("raw")), deg=deg, unaligned=bool(c.get("unaligned")), kw={})
    if c.get("raw"):
        op = sc["opacities"].astype(np.float64)
        arrays = dict(xyz=sc["means3D"], rotation=sc["rotations"], scaling=np.log(sc["scales"].astype(np.float64)), opacity=np.log(op / (1.0 - op)),
                      f_dc=sc["shs"][:, :1], f_rest=sc["shs"][:, 1:])
        if c.get("shs_res"):
            arrays["shs_res"] = 0.03 * np.random.default_rng(979).normal(size=(P, M, 3))
        out["arrays"] = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
        return out
    rng = np.random.default_rng(980)      # as tests/test_gpu_fuzz.py builds them
    arrays = dict(means3D=sc["means3D"], opacities=sc["opacities"])
    if c.get("rgb"):
        arrays["colors_precomp"] = out["kw"]["colors_precomp"] = rng.uniform(0, 1, size=(P, 3)).astype(np.float32)
    else:
        arrays["shs"] = sc["shs"]
    if c.get("cov"):
        arrays["cov3D_precomp"] = out["kw"]["cov3D_precomp"] = np.ascontiguousarray(orc.forward(sc, cam)["cov3D"]).astype(np.float32)
    else:
        arrays.update(scales=sc["scales"], rotations=sc["rotations"])
    out["arrays"] = arrays
    return out


GROWN = dict(grown=1.6, grown_again=2.6)      # scale factors: R = 333 863 -> 638 063 -> 1 260 177 on the oracle, each more than 1.25 x the one before + 4096


def _variant(inp, kind):
    """None: the case's scene.  "thin": the scene turned transparent (tests/test_gpu_parity.py: _list_cut_body) -- every tile consumes far more
    of its list than the cut remembers.  "grown" / "grown_again": every Gaussian 1.6 x / 2.6 x as large -- more instances than the capacity the
    forward before left (gsrast_policy.h: grow_capacity), so the speculative launch does not fit."""
    if kind is None:
        return inp
    assert not inp["raw"] and "scales" in inp["arrays"]
    out = dict(inp)
    if kind == "thin":
        out["sc"] = dict(inp["sc"], opacities=(inp["sc"]["opacities"] * 0.04).astype(np.float32))
        out["arrays"] = dict(inp["arrays"], opacities=out["sc"]["opacities"])
    else:
        out["sc"] = dict(inp["sc"], scales=(inp["sc"]["scales"] * np.float32(GROWN[kind])).astype(np.float32))
        out["arrays"] = dict(inp["arrays"], scales=out["sc"]["scales"])
    return out


def _leaves(inp, gpu, grad):
    """Fresh tensors of the case's inputs (+ the means2D sink), each requiring grad if `grad`."""
    ten = {}
    for k, a in inp["arrays"].items():
        if k == "shs" and inp["unaligned"]:      # a contiguous view that starts 4 bytes into its (256-byte aligned) buffer
            buf = torch.zeros(a.size + 1, dtype=torch.float32, device=gpu)
            x = buf[1:].view(a.shape)
            x.copy_(_t(a, gpu))
            assert x.is_contiguous() and x.data_ptr() % 16 == 4
        else:
            x = _t(a, gpu)
        ten[k] = x.requires_grad_(grad)
    ten["means2D"] = torch.zeros((P, 3), dtype=torch.float32, device=gpu, requires_grad=grad)
    return ten


# ---- the references: computed once per case, shared, never written ------------------------------------------------------------------------------
_REFS = {}


def _reference(name, gpu, variant=None, upstream=None):
    """(o32, o64, r32, r64): the oracle's fp32 render and its fp64 truth (with gradients if `upstream`), and both builds' gradients under the
    names of the case's leaves."""
    key = (name, variant, upstream is not None)
    if key not in _REFS:
        from oracle import oracle as orc
        inp = _variant(_inputs(name), variant)
        sc, a = inp["sc"], inp["arrays"]
        if inp["raw"]:      # the oracle renders the activated attributes the device produced: no 1-ulp input difference flips a radius
            import fused_epilogue
            with torch.no_grad():
                motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(*[_t(a[k], gpu) for k in ("xyz", "rotation", "scaling", "opacity", "f_dc", "f_rest")],
                                                                                 shs_residual=_t(a["shs_res"], gpu) if "shs_res" in a else None)
            sc = dict(sc, means3D=motion.cpu().numpy(), rotations=rot.cpu().numpy(), scales=scale.cpu().numpy(), opacities=opa.cpu().numpy(), shs=shs.cpu().numpy())
        o32 = orc.render(sc, inp["cam"], upstream, **inp["kw"])
        o64 = orc.render(sc, inp["cam"], upstream, f64=True, **inp["kw"]) if upstream is not None else None
        r = []
        for o in (o32, o64):
            if upstream is None:
                r.append(None)
            elif inp["raw"]:
                from oracle import epilogue_oracle as eo
                b = eo.backward(a["rotation"], a["scaling"], a["opacity"], None, None, o["dL_drotations"].astype(np.float64), o["dL_dscales"].astype(np.float64),
                                o["dL_dopacity"].astype(np.float64).reshape(P, 1))
                g = dict(xyz=o["dL_dmeans3D"], rotation=b["rotation"], scaling=b["scaling"], opacity=b["logit"].reshape(P, 1), f_dc=o["dL_dsh"][:, :1],
                         f_rest=o["dL_dsh"][:, 1:], means2D=o["dL_dmeans2D"])
                if "shs_res" in a:
                    g["shs_res"] = o["dL_dsh"]
                r.append({k: np.asarray(v, dtype=np.float64) for k, v in g.items()})
            else:
                r.append({k: np.asarray(o[DENSE_NAMES[k]], dtype=np.float64) for k in list(a) + ["means2D"]})
        _REFS[key] = (o32, o64, r[0], r[1])
    return _REFS[key]


def _preconditions(o32, o64):
    """What makes the scene a test of the cut, from the oracle: tiles whose every pixel stops inside its list, visible rows nobody consumes."""
    gx = (W + 15) // 16
    rg = o32["ranges"].reshape(-1, 2).astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    deepest = np.zeros(rg.shape[0], np.int64)
    np.maximum.at(deepest, ((ys // 16) * gx + xs // 16).ravel(), o32["n_contrib"].astype(np.int64).ravel())
    stopped = int((deepest < rg[:, 1] - rg[:, 0]).sum())
    vis = o32["radii"] > 0
    zero = ~((o64["dL_dmeans2D"].reshape(P, -1) != 0).any(1) | (o64["dL_dopacity"].reshape(P, -1) != 0).any(1))
    print(f"oracle: R {o32['R']}, {int(vis.sum())} visible rows, {int((~zero).sum())} rows with a gradient, {stopped} of {rg.shape[0]} tiles fully stopped")
    assert rg.shape[0] == 130 and stopped >= 100
    assert not (~zero & ~vis).any() and int((zero & vis).sum()) * 2 >= int(vis.sum())
    return zero


# ---- the HIP calls -------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _switched(rast, **options):
    """Process-wide switches whose default is 0 (list_cut_always, no_list_cut, debug_state), and the poisoned state buffers."""
    _C = rast._C
    _C.POISON_STATE_BUFFERS = True
    try:
        for k, v in options.items():
            _C.set_option(k, v)
        yield
    finally:
        _C.POISON_STATE_BUFFERS = False
        for k in options:
            _C.set_option(k, 0)


def _direct(rast, gpu, inp, size=None, cam=None):
    """One _C.rasterize_gaussians* call and the fields of its state that a cut state lays out like an uncut one."""
    _C = rast._C
    cam = inp["cam"] if cam is None else cam
    w, h = size or (W, H)
    rs = settings_from(rast, cam, inp["sc"], gpu)
    ten = _leaves(inp, gpu, False)
    e = torch.empty(0)
    if inp["raw"]:
        raw = dict(xyz=ten["xyz"], rotation=ten["rotation"], scaling=ten["scaling"], opacity_logit=ten["opacity"], features_dc=ten["f_dc"],
                   features_rest=ten["f_rest"], shs_res=ten.get("shs_res"))
        state = _C.rasterize_gaussians_raw(rs.bg, raw, 1.0, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, h, w, inp["deg"], rs.campos)
    else:
        state = _C.rasterize_gaussians(rs.bg, ten["means3D"], ten.get("colors_precomp", e), ten["opacities"], ten.get("scales", e), ten.get("rotations", e), 1.0,
                                       ten.get("cov3D_precomp", e), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, h, w, ten.get("shs", e), inp["deg"], rs.campos, False)
    R, color, radii, gb, bb, ib, depth = state
    late = _C.context_query("last_late")
    st = _C.debug_export(P, R, w, h, gb, bb, ib)
    torch.cuda.synchronize()
    out = dict(R=R, late=late, color=color.cpu().numpy(), depth=depth.cpu().numpy(), radii=radii.cpu().numpy())
    out.update({k: st[k].cpu().numpy() for k in ("rgb", "clamped", "tiles_touched", "n_contrib", "final_T")})
    return out


def _module(rast, gpu, inp, upstream=None):
    """The module call a caller of the product makes: with `upstream` every leaf requires grad and the gradients come back under the leaves'
    names (float64 arrays); without it the call runs under torch.no_grad()."""
    grad = upstream is not None
    rs = settings_from(rast, inp["cam"], inp["sc"], gpu)
    with contextlib.nullcontext() if grad else torch.no_grad():
        ten = _leaves(inp, gpu, grad)
        if inp["raw"]:
            out = rast.GaussianRasterizerRaw(rs)(ten["xyz"], ten["means2D"], ten["rotation"], ten["scaling"], ten["opacity"], ten["f_dc"], ten["f_rest"],
                                                 shs_residual=ten.get("shs_res"))
        else:
            out = rast.GaussianRasterizer(rs)(**{k: v for k, v in ten.items()})
        late = rast._C.context_query("last_late")
        grads = None
        if grad:
            out[0].backward(_t(upstream, gpu))
            torch.cuda.synchronize()
            grads = {k: x.grad.detach().double().cpu().numpy() for k, x in ten.items()}
    torch.cuda.synchronize()
    return dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), depth=out[2].detach().cpu().numpy(), late=late, grads=grads)


# ---- checks ----------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, keys, what):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


def _poisoned_rows(d):
    return (bits(d["rgb"]) == POISON).all(axis=1)


def _check_colours(d, o32, what, cut):
    """Every visible row's exported colour and clamp flags are the oracle's -- under a cut: every visible row the colour kernel did not skip.
    Returns the number of skipped visible rows."""
    vis = o32["radii"] > 0
    poison = _poisoned_rows(d)
    if not cut:
        assert not poison.any(), f"{what}: {int(poison.sum())} exported rgb rows hold the poison"
    ok = vis & ~poison
    assert np.array_equal(bits(d["rgb"][ok]), bits(np.ascontiguousarray(o32["colors"][ok]))), f"{what}: rgb"
    assert np.array_equal(d["clamped"][ok], o32["clamped"][ok]), f"{what}: clamped"
    return int((vis & poison).sum())


def _check_gradients(h, ref, zero, what):
    """test_gpu_parity._check_grads on the case's tensors; the rows nobody consumes exact zeros.  Prints and returns the worst err / bar that
    _check_grads itself found."""
    o32, o64, r32, r64 = ref
    for k, g in h["grads"].items():
        assert g is not None and np.isfinite(g).all(), f"{what}: {k} is not finite"
        assert not g.reshape(P, -1)[zero].any(), f"{what}: {k} has {int(g.reshape(P, -1)[zero].any(1).sum())} non-zero rows that nothing consumes"
    names = list(h["grads"])
    conditioning = "cov3D_precomp" in names      # tests/test_gpu_fuzz.py: aniso > 10 or (P > 30000 and (use_cov or aniso >= 10 or scale_mul >= 8))
    worst = _check_grads(r64, r32, h["grads"], names, strict=False, conditioning=conditioning)
    print(f"{what}: worst gradient err / bar {worst[0]:.3f} ({worst[1]})")
    return worst


def _zero_rows(o32, o64):
    """bool [P]: the rows whose fp64 gradient is all-zero in dL_dmeans2D and dL_dopacity -- nothing consumes them (no culled row is among the others)."""
    zero = ~((o64["dL_dmeans2D"].reshape(P, -1) != 0).any(1) | (o64["dL_dopacity"].reshape(P, -1) != 0).any(1))
    assert not (~zero & ~(o32["radii"] > 0)).any()
    return zero


UPSTREAM_SEED = 978


def _upstream():
    import scenes
    return scenes.upstream_grad(H, W, UPSTREAM_SEED) * (H * W)


def _uncut_then_cut(rast, gpu, inp, o32, what, visits=2):
    """Visit 0 (no_list_cut = 1) against the oracle, then `visits` direct calls under the cut.  Returns (visit 0, [(last_late, n_poison)])."""
    _C = rast._C
    _C.set_option("no_list_cut", 1)
    try:
        v0 = _direct(rast, gpu, inp)
    finally:
        _C.set_option("no_list_cut", 0)
    assert v0["late"] == 0 and v0["R"] == o32["R"]
    assert np.array_equal(v0["radii"], o32["radii"])
    assert np.array_equal(bits(v0["color"]), bits(o32["out_color"])) and np.array_equal(bits(v0["depth"]), bits(o32["out_depth"])), f"{what}: visit 0"
    assert np.array_equal(v0["tiles_touched"].view(np.uint32), o32["tiles_touched"])
    _check_colours(v0, o32, f"{what}, visit 0", cut=False)
    figures = []
    for visit in range(1, visits + 1):
        v = _direct(rast, gpu, inp)
        assert v["late"] > 0, f"{what}: visit {visit} was expected to run under the list cut"
        assert v["R"] == v0["R"]
        _same(v, v0, ("color", "depth", "radii", "n_contrib", "final_T", "tiles_touched"), f"{what}, visit {visit}")
        n_poison = _check_colours(v, o32, f"{what}, visit {visit}", cut=True)
        print(f"{what}, visit {visit}: last_late {v['late']}, n_poison {n_poison}")
        assert 0 < n_poison <= v["late"], (what, visit, n_poison, v["late"])
        figures.append((v["late"], n_poison))
    return v0, figures


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.remembered_cut_only
@pytest.mark.parametrize("name", list(CASES))
def test_cut_colours_against_the_oracle(name, orc, rast, gpu):
    inp = _inputs(name)
    g = _upstream()
    ref = _reference(name, gpu, upstream=g)
    o32, o64 = ref[0], ref[1]
    zero = _preconditions(o32, o64)
    with _switched(rast, list_cut_always=1):
        v0, figures = _uncut_then_cut(rast, gpu, inp, o32, name)
        # visit 3: the module call under the cut, with a backward
        h = _module(rast, gpu, inp, g)
        print(f"{name}, visit 3: last_late {h['late']}")
        assert h["late"] > 0
        _same(h, v0, ("color", "depth", "radii"), f"{name}, visit 3")
        _check_gradients(h, ref, zero, f"{name}, visit 3")
        # visit 4: nobody differentiates -- no direction derivatives are stored
        e = _module(rast, gpu, inp)
        print(f"{name}, visit 4: last_late {e['late']}")
        assert e["late"] > 0 and e["grads"] is None
        _same(e, v0, ("color", "depth", "radii"), f"{name}, visit 4")


@pytest.mark.remembered_cut_only
@pytest.mark.parametrize("name", FALLBACK_CASES)
def test_fallback_colours_the_late_gaussians(name, orc, rast, gpu):
    """The scene turns transparent under a stale cut: the blend finds the cut lists too short and the completion pass runs -- the late candidates'
    colours come from the predicated launch of the compacting kernel over `skip2` (the pass's emission counts cut_fallbacks; a forward that takes
    it does not go through exact_redo: test_redo_colours_every_gaussian has that call site).  Fewer rows keep the poison than under the cut
    that held, each of the others has the oracle's colour; image, depth and final_T equal the thin scene's oracle; the module call that
    follows meets the gradient bar on it."""
    _C = rast._C
    inp, thin = _inputs(name), _variant(_inputs(name), "thin")
    g = _upstream()
    o32 = _reference(name, gpu, upstream=g)[0]
    ref2 = _reference(name, gpu, "thin", upstream=g)
    t32 = ref2[0]
    zero = _zero_rows(ref2[0], ref2[1])
    with _switched(rast, list_cut_always=1):
        _, figures = _uncut_then_cut(rast, gpu, inp, o32, name, visits=1)
        fb0 = _C.context_query("cut_fallbacks")
        v = _direct(rast, gpu, thin)
        fb1 = _C.context_query("cut_fallbacks")
        n_poison = _check_colours(v, t32, f"{name}, thin", cut=True)
        print(f"{name}, thin scene under the stale cut: last_late {v['late']}, cut_fallbacks {fb0} -> {fb1}, n_poison {n_poison}")
        assert fb1 == fb0 + 1
        assert v["late"] > 0 and n_poison < figures[0][1], "the predicated launch over skip2 was expected to colour late Gaussians"
        assert v["R"] == t32["R"] and np.array_equal(v["radii"], t32["radii"])
        assert np.array_equal(bits(v["color"]), bits(t32["out_color"])) and np.array_equal(bits(v["depth"]), bits(t32["out_depth"]))
        assert np.array_equal(bits(v["final_T"]), bits(np.asarray(t32["final_T"], dtype=np.float32)))
        h = _module(rast, gpu, thin, g)
        print(f"{name}, thin scene, module call: last_late {h['late']}, cut_fallbacks {_C.context_query('cut_fallbacks')}")
        assert np.array_equal(bits(h["color"]), bits(t32["out_color"])) and np.array_equal(bits(h["depth"]), bits(t32["out_depth"]))
        assert np.array_equal(h["radii"], t32["radii"])
        _check_gradients(h, ref2, zero, f"{name}, thin scene")


REDO_CASES = ("shs_M16_deg2", "shs_M25_deg3", "colors_precomp")


@pytest.mark.remembered_cut_only
@pytest.mark.parametrize("name", REDO_CASES)
def test_redo_colours_every_gaussian(name, orc, rast, gpu):
    """The scene grows under a remembered cut: the forward runs the compacting kernel on the early Gaussians, then learns that the instances
    do not fit the capacity its speculative launch was sized for and repeats binning and blend from the full lists (exact_redo) -- in front of
    which the plain colour kernel colours EVERY Gaussian, behind the compacting one.  A context of its own, so that the capacity hint is the
    base scene's whatever ran before: R = 333 863 leaves a capacity of 421 424; the grown scenes have 638 063 and 1 260 177 instances.
      module call on the 1.6 x scene, with a backward: redo_count + 1 under a cut (last_late > 0: without the predicted cut only a pose whose
        cut depths are remembered has late Gaussians, and then the plan has cut_colors as in the visits before); colour, depth, radii equal
        the grown scene's oracle; gradients at the bar, zero rows exact -- the backward on a redone state takes no row for a late one;
      direct call on the 2.6 x scene: redo_count + 1 under a cut again; n_poison == 0 -- the plain kernel coloured the whole set -- and every
        visible row's exported rgb / clamped, the image, depth and final_T are the oracle's."""
    _C = rast._C
    inp = _inputs(name)
    g = _upstream()
    o32 = _reference(name, gpu, upstream=g)[0]
    ref1 = _reference(name, gpu, "grown", upstream=g)
    g32 = ref1[0]
    b32 = _reference(name, gpu, "grown_again")[0]
    assert g32["R"] > o32["R"] + o32["R"] // 4 + 4096 and b32["R"] > g32["R"] + g32["R"] // 4 + 4096      # gsrast_policy.h: grow_capacity
    zero = _zero_rows(ref1[0], ref1[1])
    ctx = _C.Context()
    try:
        with ctx, _switched(rast, list_cut_always=1):
            _direct(rast, gpu, inp)      # (a context's first forward has no capacity hint: it is not speculative and not cut)
            _, figures = _uncut_then_cut(rast, gpu, inp, o32, name, visits=1)
            redo0 = _C.context_query("redo_count")
            h = _module(rast, gpu, _variant(inp, "grown"), g)
            redo1 = _C.context_query("redo_count")
            print(f"{name}, 1.6 x scene, module call: last_late {h['late']}, redo_count {redo0} -> {redo1}")
            assert redo1 == redo0 + 1 and h["late"] > 0
            assert np.array_equal(h["radii"], g32["radii"])
            assert np.array_equal(bits(h["color"]), bits(g32["out_color"])) and np.array_equal(bits(h["depth"]), bits(g32["out_depth"]))
            _check_gradients(h, ref1, zero, f"{name}, 1.6 x scene")
            v = _direct(rast, gpu, _variant(inp, "grown_again"))
            redo2 = _C.context_query("redo_count")
            n_poison = _check_colours(v, b32, f"{name}, 2.6 x scene", cut=False)
            print(f"{name}, 2.6 x scene: last_late {v['late']}, redo_count {redo1} -> {redo2}, n_poison {n_poison} (under the cut that held: {figures[0]})")
            assert redo2 == redo1 + 1 and v["late"] > 0 and n_poison == 0
            assert v["R"] == b32["R"] and np.array_equal(v["radii"], b32["radii"])
            assert np.array_equal(bits(v["color"]), bits(b32["out_color"])) and np.array_equal(bits(v["depth"]), bits(b32["out_depth"]))
            assert np.array_equal(bits(v["final_T"]), bits(np.asarray(b32["final_T"], dtype=np.float32)))
    finally:
        ctx.close()


PRED_W, PRED_H = 232, 136        # (an image size no other test uses: this test's poses are the only ones in its table)


@pytest.mark.parametrize("name", PREDICTED_CASES)
def test_camera_path_under_the_predicted_cut(name, rast, gpu, orc, scenes):
    """Twelve consecutive poses of a 360-pose ring, none rendered twice: the cut depths are PREDICTED (option tau_cut), the compacting kernel
    colours the early Gaussians of a pose the context has never seen.  Every frame bit-equal to the same frame without a cut, the last one to
    the oracle.  (No exact counts: the predicted cut is on, as in the product.)"""
    _C = rast._C
    inp = _inputs(name)
    first = 200 + 30 * PREDICTED_CASES.index(name)      # (every case its own poses: none is in the context's table when it is rendered)
    frames = list(range(first, first + 12))
    cams = {k: scenes.camera(k, 360, PRED_W, PRED_H) for k in frames}
    keys = ("color", "depth", "radii", "n_contrib", "final_T")
    with _switched(rast, list_cut_always=1):
        outs = {k: _direct(rast, gpu, inp, (PRED_W, PRED_H), cams[k]) for k in frames}
        n_poison = {k: int((_poisoned_rows(outs[k]) & (outs[k]["radii"] > 0)).sum()) for k in frames}
        print(f"{name}: last_late per frame", [outs[k]["late"] for k in frames], "n_poison", [n_poison[k] for k in frames])
        for k in frames[2:]:      # the first frame of a context is not cut, the second predicts from a depth range learned on one forward
            assert outs[k]["late"] > 0, k
            assert 0 < n_poison[k] <= outs[k]["late"], (k, n_poison[k], outs[k]["late"])      # the compacting kernel ran (cut_colors under a predicted cut) and skipped them
        _C.set_option("no_list_cut", 1)
        try:
            for k in frames:
                full = _direct(rast, gpu, inp, (PRED_W, PRED_H), cams[k])
                assert full["late"] == 0 and full["R"] == outs[k]["R"]
                _same(outs[k], full, keys, f"{name}, frame {k}")
        finally:
            _C.set_option("no_list_cut", 0)
    k = frames[-1]
    o = orc.render(inp["sc"], cams[k], **inp["kw"])
    assert outs[k]["R"] == o["R"] and np.array_equal(outs[k]["radii"], o["radii"])
    assert np.array_equal(bits(outs[k]["color"]), bits(o["out_color"])) and np.array_equal(bits(outs[k]["depth"]), bits(o["out_depth"]))
    _check_colours(outs[k], o, f"{name}, frame {k}", cut=True)


@pytest.mark.remembered_cut_only
def test_debug_state_masks_the_compacting_kernel(orc, rast, gpu):
    """The diagnostic plan, pinned: under debug_state the cut is applied (last_late > 0) but every Gaussian is coloured -- no exported row keeps
    the poison -- and the image is the same.  It also shows that the n_poison assertion above tells the two plans apart."""
    name = "shs_M16_deg3"
    inp = _inputs(name)
    o32 = _reference(name, gpu, upstream=_upstream())[0]
    with _switched(rast, list_cut_always=1):
        v0, figures = _uncut_then_cut(rast, gpu, inp, o32, name, visits=1)
        rast._C.set_option("debug_state", 1)
        try:
            v = _direct(rast, gpu, inp)
        finally:
            rast._C.set_option("debug_state", 0)
        n_poison = _check_colours(v, o32, f"{name}, debug_state = 1", cut=True)
        print(f"{name}, debug_state = 1: last_late {v['late']}, n_poison {n_poison} (debug_state = 0: {figures[0]})")
        assert v["late"] > 0 and n_poison == 0
        _same(v, v0, ("color", "depth", "radii", "n_contrib", "final_T"), f"{name}, debug_state = 1")
