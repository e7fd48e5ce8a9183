"""-m gpu: the per-Gaussian blend-weight statistics (`contrib=sink`, `pixel_weights=`; include/gsrast.h: gsrast_contrib_stats,
csrc/gsrast_contrib.h) against tests/contrib_math.py -- torch fp64 on tests/math_renderer.py.

Cases (contrib_math.CASES), image 70 x 45 = 5 x 3 tiles, ragged in both axes.  a: 700 Gaussians, 622 of them in one tile's list (more than
two 256-entry batches, walked by pixels that never saturate), Gaussians over four and more tiles, an opaque stack that ends its pixels early,
Gaussians behind the camera and off screen.  b: 2000 sparse Gaussians, at most 54 per tile, two empty tiles, three workgroups of the finish
kernel.  pixel_weights = ~ambiguous (under 5 % of each case, asserted).  Columns 2 and 3 must equal the reference exactly.

Tolerance of columns 0 and 1: 4 x the fp32 restatement's own error, the margin tests/test_gpu_independent.py takes for the same reason (the
HIP path rounds like fp32, not like the fp64 reference).  Measured on the CPU, max |contrib_math(float32) - contrib_math(float64)| over the
cases and variants below, as a max|ref| + r |ref| (r: the largest relative error among rows above a tenth of the column's maximum, a: what
that leaves of the other rows):
    col 0 weight_sum   a = 3.35e-7   r = 2.26e-6          col 1 weight_max   a = 8.3e-7   r = 1.41e-5
(worst rows: case b, small Gaussians whose few pixels sit on the steep flank of exp).  Measured on the MI355X, worst |err| / bar over all
cases and variants: see the figures each test prints.

Checks without a reference are bit-exact or identities: every accumulation across waves and tiles is an integer atomic."""
import functools

import numpy as np
import pytest
import torch

import contrib_math as cm
from conftest import settings_from

pytestmark = pytest.mark.gpu

BAR = {0: (3.35e-7, 2.26e-6), 1: (8.3e-7, 1.41e-5)}      # column: (a, r); the test bar is 4 x (a max|ref| + r |ref|)
DENSE = ("means3D", "opacities", "shs", "scales", "rotations")


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _render(rast, gpu, sc, cam, *, sink="nan", weights=None, aa=False, precomp=False, raw=False, aux=False, absgrad=False, grad=False, rows=None):
    """One forward (+ one backward with `grad`).  sink: "nan" = a fresh [P,4] tensor full of NaN, None = no contrib, or a tensor.
    Returns dict(out, sink, grads, absgrad)."""
    P = sc["means3D"].shape[0]
    rs = settings_from(rast, cam, sc, gpu)
    if isinstance(sink, str):
        sink = torch.full((P if rows is None else rows, 4), float("nan"), device=gpu)
    kw = dict(return_aux=aux, antialiasing=aa)
    view = None
    if sink is not None:
        view = sink[:P]
        kw["contrib"] = view
        if weights is not None:
            kw["pixel_weights"] = weights if isinstance(weights, torch.Tensor) else _t(weights, gpu)
    ag = torch.full((P, 2), float("nan"), device=gpu) if absgrad else None
    if absgrad:
        kw["absgrad"] = ag
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=grad)
    if raw:
        sig = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1 - 1e-6)
        arrs = dict(xyz=sc["means3D"], rotation=sc["rotations"], scaling=np.log(sc["scales"].astype(np.float64)), opacity=np.log(sig / (1 - sig)),
                    features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:])
        leaves = {n: _t(v, gpu).requires_grad_(grad) for n, v in arrs.items()}
        out = rast.GaussianRasterizerRaw(rs)(means2D=m2, **leaves, **kw)
    else:
        leaves = {n: _t(sc[n], gpu).requires_grad_(grad) for n in DENSE}
        col = dict(colors_precomp=_t(np.clip(sc["shs"][:, 0] * 0.28 + 0.5, 0, 1), gpu).requires_grad_(grad)) if precomp else dict(shs=leaves["shs"])
        if precomp:
            leaves["shs"] = col["colors_precomp"]
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], scales=leaves["scales"],
                                          rotations=leaves["rotations"], **col, **kw)
    grads = None
    if grad:
        g = torch.as_tensor(np.random.default_rng(5).normal(size=tuple(out[0].shape)), dtype=torch.float32, device=gpu)
        loss = (out[0] * g).sum()
        if aux:
            loss = loss + (out[3] * g[:1]).sum() + (out[4] * g[1:2]).sum()
        loss.backward()
        grads = {n: x.grad.detach().clone() for n, x in leaves.items()}
        grads["means2D"] = m2.grad.detach().clone()
    torch.cuda.synchronize()
    return dict(out=out, sink=sink, view=view, grads=grads, absgrad=ag, leaves=leaves)


@functools.lru_cache(maxsize=None)
def _float_weights(name):
    """A non-trivial weight map in (0, 1), zero on the ambiguous pixels, and its float64 table."""
    r = cm.reference(name)
    H, W = r["amb"].shape
    fw = (0.05 + 0.9 * np.random.default_rng(9).uniform(size=(H, W))).astype(np.float32)
    fw[r["amb"]] = 0.0
    table, _, _ = cm.contrib(r["sc"], r["cam"], pixel_weights=fw, render_out=r["out"])
    return fw, table


def _check_table(got, ref, what):
    assert not np.isnan(got).any(), "a row of the sink was not written"
    worst = 0.0
    for col, (a, r) in BAR.items():
        err = np.abs(got[:, col] - ref[:, col])
        tol = 4.0 * (a * np.abs(ref[:, col]).max() + r * np.abs(ref[:, col]))
        worst = max(worst, float((err / tol).max()))
        print(f"{what}: col {col} max|err| {err.max():.3e} max|ref| {np.abs(ref[:, col]).max():.3e} worst err / bar {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (what, col, float(err.max()), float((err / tol).max()))
    for col in (2, 3):
        assert np.array_equal(got[:, col], ref[:, col]), (what, col, int((got[:, col] != ref[:, col]).sum()))
    return worst


def _np(x):
    return x.detach().double().cpu().numpy()


# ---- against the fp64 reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "antialias", "colors_precomp", "float_weights"])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_against_the_fp64_reference(name, variant, rast, gpu):
    aa = variant == "antialias"
    r = cm.reference(name, aa)
    assert r["amb"].mean() < 0.05, "too many pixels with an fp32-ambiguous decision"
    weights, ref = (r["weights"], r["table"]) if variant != "float_weights" else _float_weights(name)
    h = _render(rast, gpu, r["sc"], r["cam"], weights=weights, aa=aa, precomp=variant == "colors_precomp")
    radii = h["out"][1].cpu().numpy()
    assert np.array_equal(radii > 0, r["out"]["proj"]["disc"]["vis"]), "radius decision differs: pick another seed"
    got = _np(h["sink"])
    _check_table(got, ref, f"case {name}, {variant}")
    assert not got[radii == 0].any() and (got[radii > 0][:, 2] == 0).any()      # culled rows; listed, but never blended
    assert (got[:, 1] <= np.float32(0.99)).all() and (got[:, 2] >= got[:, 3]).all() and (got[:, 0] <= got[:, 1] * got[:, 2] * (1 + 1e-6)).all()
    if name == "a":
        assert r["out"]["tile_list_max"] > 600 and (got[:, 2] > 4 * 256).sum() >= 4


# ---- without a reference: bit-exact, or identities ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp_mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_runs_are_bit_identical_and_ones_are_no_weights(name, exp_mode, rast, gpu):
    """In every exp_mode: the replay's alpha and T are the forward's own, whichever exp both use, so no bar here depends on that exp's accuracy."""
    r = cm.reference(name)
    rast._C.set_option("exp_mode", exp_mode)
    try:
        a = _render(rast, gpu, r["sc"], r["cam"])
        b = _render(rast, gpu, r["sc"], r["cam"])
        ones = _render(rast, gpu, r["sc"], r["cam"], weights=np.ones(r["amb"].shape, np.float32)[None])      # ([1,H,W] is accepted too)
        aux = _render(rast, gpu, r["sc"], r["cam"], aux=True)
    finally:
        rast._C.set_option("exp_mode", 0)
    assert not torch.isnan(a["sink"]).any() and float(a["sink"][:, 2].max()) > 0
    assert torch.equal(a["sink"], b["sink"]) and torch.equal(a["sink"], ones["sink"])
    # sum col0 = sum (1 - T_final): the aux output's alpha, to 1e-5 relative; sum col3 = pixels with a contributor
    assert torch.equal(aux["sink"], a["sink"])
    alpha = _np(aux["out"][4])
    s0 = _np(a["sink"])[:, 0].sum()
    print(f"case {name}, exp_mode {exp_mode}: |sum col 0 - sum alpha| / sum alpha {abs(s0 - alpha.sum()) / alpha.sum():.3e}")
    assert abs(s0 - alpha.sum()) <= 1e-5 * alpha.sum(), (s0, alpha.sum())
    assert _np(a["sink"])[:, 3].sum() == (alpha > 0).sum()


def test_low_level_call_touched_rows_and_no_write_past_P(rast, gpu):
    """The binding's own entry (_C.contrib_stats on the state _C.rasterize_gaussians returns) gives the module's result; a non-zero row only
    where gsrast_touched_rows allows one; rows >= P of a larger allocation keep their contents."""
    _C = rast._C
    r = cm.reference("a")
    sc, cam = r["sc"], r["cam"]
    P, H, W = sc["means3D"].shape[0], cam["image_height"], cam["image_width"]
    mod = _render(rast, gpu, sc, cam, rows=P + 3)
    assert torch.isnan(mod["sink"][P:]).all() and not torch.isnan(mod["sink"][:P]).any()
    rs = settings_from(rast, cam, sc, gpu)
    e = torch.empty(0)
    ten = {n: _t(sc[n], gpu) for n in DENSE}
    R, color, radii, gb, bb, ib, depth = _C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix,
                                                                rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, ten["shs"], 3, rs.campos, False)
    big = torch.full((P + 5, 4), -7.0, device=gpu)
    _C.contrib_stats(big[:P], None, R, W, H, gb, bb, ib)
    flags = torch.zeros(P, dtype=torch.uint8, device=gpu)
    assert _C.lib().gsrast_touched_rows(P, gb.data_ptr(), flags.data_ptr(), _C._stream_of(gpu)) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[:P], mod["sink"][:P]) and (big[P:] == -7.0).all()
    nonzero = (big[:P] != 0).any(dim=1)
    assert not (nonzero & (flags == 0)).any(), "a non-zero row for a Gaussian no pixel consumed"
    assert int(nonzero.sum()) > 600


@pytest.mark.remembered_cut_only
def test_list_cut_is_bit_identical_to_no_list_cut(rast, gpu, scenes):
    """The list cut needs the bucket depth sort, which runs from 32768 Gaussians on: 50 000 Gaussians at 256 x 192 with raised opacities (most
    tiles saturate), the shape at which tests/test_gpu_raw.py puts a pose under the cut.  The first render, without the cut, leaves the
    pose's cut depths; the next ones leave the late Gaussians out of the lists and must give the same table bit for bit."""
    _C = rast._C
    P, W, H = 50_000, 256, 192
    sc = scenes.synth(P, 451)
    sc["opacities"] = (1.0 / (1.0 + np.exp(-(np.log(sc["opacities"] / (1.0 - sc["opacities"])) + 2.0)))).astype(np.float32)
    cam = scenes.camera(2, 5, W, H)
    _C.set_option("list_cut_always", 1)
    try:
        _C.set_option("no_list_cut", 1)
        try:
            full = _render(rast, gpu, sc, cam)
            assert _C.context_query("last_late") == 0
        finally:
            _C.set_option("no_list_cut", 0)
        for visit in range(2):
            cut = _render(rast, gpu, sc, cam)
            late = _C.context_query("last_late")
            assert late > 0, "the repeated pose was expected to run under the list cut"
            assert torch.equal(cut["out"][0], full["out"][0])
            assert torch.equal(cut["sink"], full["sink"]), f"visit {visit}: {int((cut['sink'] != full['sink']).any(dim=1).sum())} rows differ"
    finally:
        _C.set_option("list_cut_always", 0)
    assert not torch.isnan(full["sink"]).any() and float(full["sink"][:, 2].max()) > 0
    assert int((full["sink"][:, 2] == 0).sum()) > P // 4      # the occluded Gaussians


def test_raw_path_is_bit_identical_to_activate_then_plain(rast, gpu):
    import fused_epilogue
    r = cm.reference("b")
    sc, cam = r["sc"], r["cam"]
    P = sc["means3D"].shape[0]
    raw = _render(rast, gpu, sc, cam, raw=True, weights=r["weights"])
    lv = raw["leaves"]
    motion, rot, scale, opa, shs = fused_epilogue.activate_gaussians(lv["xyz"], lv["rotation"], lv["scaling"], lv["opacity"], lv["features_dc"], lv["features_rest"])
    sink = torch.full((P, 4), float("nan"), device=gpu)
    out = rast.GaussianRasterizer(settings_from(rast, cam, sc, gpu))(means3D=motion, means2D=torch.zeros((P, 3), device=gpu), opacities=opa, shs=shs, scales=scale,
                                                                     rotations=rot, contrib=sink, pixel_weights=_t(r["weights"], gpu))
    torch.cuda.synchronize()
    assert torch.equal(out[0], raw["out"][0]) and torch.equal(sink, raw["sink"]) and float(sink[:, 2].max()) > 0


def test_empty_scene_and_one_pixel(rast, gpu, scenes):
    r = cm.reference("b")
    sc0 = {k: (v[:0] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in r["sc"].items()}
    h = _render(rast, gpu, sc0, r["cam"])
    assert h["sink"].shape == (0, 4)
    cam1 = scenes.camera(1, 6, 1, 1)
    sc = scenes.synth(50, 3, scale_mul=3.0)
    a = _render(rast, gpu, sc, cam1, aux=True)
    got = _np(a["sink"])
    assert not np.isnan(got).any() and got[:, 2].max() == 1.0 and got[:, 3].sum() == 1.0
    assert abs(got[:, 0].sum() - float(a["out"][4].sum())) <= 1e-5 * got[:, 0].sum()
    zero = _render(rast, gpu, sc, cam1, weights=np.zeros((1, 1), np.float32))
    assert not zero["sink"].any()


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves_and_no_launch_without_a_sink(rast, gpu):
    """contrib with absgrad, return_aux and a backward: colour, aux outputs, the absgrad sink's zero rows and every gradient's zero rows are the
    call's without contrib; outputs bit for bit.  (Gradients: two backwards of one call already differ in their last bits -- float atomics,
    tests/test_gpu_absgrad.py -- so "bit-identical" can only be asked of what the forward returns; the gradients are held to 1e-5 max + 1e-4.)
    The profile table counts one launch of each new kernel per call with a sink and none without."""
    _C = rast._C
    r = cm.reference("a")
    _C.set_option("profile", -1)
    try:
        _C.profile_reset()
        wo = _render(rast, gpu, r["sc"], r["cam"], sink=None, aux=True, absgrad=True, grad=True)
        prof = _C.profile_read()
        assert prof["contrib_blend"][1] == 0 and prof["contrib_finish"][1] == 0 and prof["blend_fwd"][1] >= 1
        w = _render(rast, gpu, r["sc"], r["cam"], aux=True, absgrad=True, grad=True, weights=r["weights"])
        prof = _C.profile_read()
        assert prof["contrib_blend"][1] == 1 and prof["contrib_finish"][1] == 1
    finally:
        _C.set_option("profile", 0)
        _C.profile_reset()
    for a, b in zip(w["out"], wo["out"]):
        assert torch.equal(a, b)
    _check_table(_np(w["sink"]), r["table"], "with absgrad, aux and a backward")
    pairs = [(w["grads"][n], wo["grads"][n], n) for n in w["grads"]] + [(w["absgrad"], wo["absgrad"], "absgrad")]
    for a, b, n in pairs:
        a, b = _np(a), _np(b)
        P = a.shape[0]
        assert np.array_equal((a.reshape(P, -1) != 0).any(1), (b.reshape(P, -1) != 0).any(1)), n
        assert (np.abs(a - b) <= 1e-5 * np.abs(b).max() + 1e-4 * np.abs(b)).all(), n


def test_under_no_grad_with_camera_grads_and_an_arena(rast, gpu):
    _C = rast._C
    r = cm.reference("b")
    ref = _render(rast, gpu, r["sc"], r["cam"], weights=r["weights"])["sink"]
    with torch.no_grad():
        ng = _render(rast, gpu, r["sc"], r["cam"], weights=r["weights"])["sink"]
    assert torch.equal(ng, ref)
    _check_table(_np(ng), r["table"], "under no_grad")
    # camera_grads (the settings' matrices as differentiable inputs) and an installed GradArena
    P = r["sc"]["means3D"].shape[0]
    rs = settings_from(rast, r["cam"], r["sc"], gpu)
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    arena = _C.GradArena(P, 16, gpu)
    _C.set_grad_arena(arena)
    try:
        arena.zero_grad()
        leaves = {n: _t(r["sc"][n], gpu).requires_grad_(True) for n in DENSE}
        sink = torch.full((P, 4), float("nan"), device=gpu)
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=torch.zeros((P, 3), device=gpu, requires_grad=True), opacities=leaves["opacities"],
                                          shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"], camera_grads=True, contrib=sink,
                                          pixel_weights=_t(r["weights"], gpu))
        out[0].sum().backward()
        torch.cuda.synchronize()
        assert arena.dirty and rs.viewmatrix.grad is not None
    finally:
        _C.set_grad_arena(None)
    assert torch.equal(sink, ref)


def test_prune_carries_contrib_stats(rast, gpu):
    """fused_densify.prune gathers a ContribStats like the DensifyStats beside it (not reset), and the negated keep mask is a prune mask."""
    import fused_densify
    r = cm.reference("b")
    P = r["sc"]["means3D"].shape[0]
    sink = _render(rast, gpu, r["sc"], r["cam"])["sink"]
    cs = fused_densify.ContribStats(P, gpu)
    cs.update(sink)
    cs.update(sink)
    assert torch.equal(cs.views, 2.0 * (sink[:, 2] > 0)) and torch.equal(cs.weight_max, sink[:, 1]) and torch.equal(cs.pixel_count, 2 * sink[:, 2])
    keep = cs.keep_mask_by_rank("weight_sum", 0.1)
    assert int(keep.sum()) == 200 and bool((cs.weight_sum[keep].min() >= cs.weight_sum[~keep].max()))
    before_sums, before_max = cs.sums.clone(), cs.weight_max.clone()
    params = [torch.nn.Parameter(_t(r["sc"]["means3D"], gpu)), torch.nn.Parameter(_t(r["sc"]["opacities"], gpu))]
    opt = torch.optim.Adam([dict(params=[params[0]], name="xyz"), dict(params=[params[1]], name="opacity")], lr=1e-3)
    ds = fused_densify.DensifyStats(P, gpu)
    counts, new, rest = fused_densify.prune(opt, ~keep, ds, contrib=cs)
    torch.cuda.synchronize()
    assert counts["P"] == 200 and cs.P == 200 and ds.P == 200 and rest == [] and new["xyz"].shape == (200, 3)
    assert torch.equal(cs.sums, before_sums[keep]) and torch.equal(cs.weight_max, before_max[keep])
    assert torch.equal(new["xyz"].detach(), params[0].detach()[keep])
