"""-m gpu: the replays and every gradient source of the backward on the states whose rows are NOT all visited -- touched bits, sparsely
zeroed gradient records, the grouped backward, the list cut.  tests/test_sparse_states_host.py asserts on the CPU what this file relies on
(which Gaussians contribute to nothing, that the upstream gradients vanish on the ambiguous pixels) and holds the helpers both share.

Between phase 1 and phase 2 of the backward, features_bwd_kernel and distort_bwd_kernel add to the gradient records the blend backward
filled; the aux gradients add to float 9; preprocess_bwd_kernel<.., POSE> sums the camera's gradient over the rows it visits; and
distort_fwd_kernel / pixel_topk_kernel replay the forward's lists.  All of it is right only if (i) every Gaussian a replay adds to is a
touched one (its record was zeroed, phase 2 visits it), (ii) nothing a replay reads was left unwritten for rows the forward skipped, and
(iii) the rows nobody visits come out as exact zeros in every output.

Cases: contrib_math.CASES a and b (70 x 45, 5 x 3 ragged tiles; 12 / 32 and 57 / 58 visible Gaussians that contribute to nothing without /
with antialiasing, 28 and 1726 culled ones) and posegrad_math's dense and raw cases for the camera; sections 1, 2 and 4 stay under 2000
Gaussians.  Section 3 is the shape at which tests/test_gpu_contrib.py and tests/test_gpu_raw.py put a pose under the list cut (50 000
Gaussians, 256 x 192, opacity logits + 2).

1. The touched bits (gsrast_touched_rows) contain every replay's contributors, in every exp mode, with antialiasing, in both families.
2. Every gradient source over poisoned, sparsely zeroed records in the three forms of the per-Gaussian backward, against fp64 at
   conftest.grad_tol(r64, r32); exact zeros on the rows that contribute to nothing; the same non-zero rows as with sparse_grec = 0.
3. Replays and gradients on list-cut states against the uncut visit: forward bit for bit; gradients at the cut-against-uncut bar of
   tests/test_gpu_raw.py, 1e-5 max|ref| + 1e-4 |ref|, beside the uncut render's own run-to-run difference in the same expression.
4. A second backward (retain_graph) on a state with features, distortion and aux.

The launch counts of section 2 are a test of their own (test_launch_counts_show_what_ran), so that a count that is not what was expected
does not hide a gradient.  It found the one thing this file changed in the library: see its docstring.

Measured on the MI355X (one run; every test prints its figures)
----------------------------------------------------------------
Section 1, flagged rows that contribute to nothing (a cost, not an error), the same in the three exp modes and both families:
    case a  plain 12 of 672 flagged (660 contribute; every visible row is flagged)      antialias 25 of 667 (642 contribute; 5 visible rows not flagged)
    case b  plain  2 of 219 flagged (217 contribute; 55 visible rows not flagged)       antialias  0 of 216 (216 contribute; 58 visible rows not flagged)
Section 2, worst gradient err / bar per source -- the same to three digits in the grouped, the sparse and the dense form:
    source                       case a          case b                    source                        worst
    features C = 5               0.021 means2D   0.096 features            camera, dense (posegrad a)    0.130 scales
    features C = 40              0.025 features  0.126 means3D             camera, raw   (posegrad b)    0.256 scaling
    distortion                   0.109 means3D   0.123 rotations           everything, case a, mode 1    0.063 rotation
    distortion + colour + aux    0.019 rotations 0.156 rotations           everything, case a, mode 2    0.047 rotation
    aux                          0.033 scales    0.130 scales
    everything, mode 0           0.047 xyz       0.107 xyz
Section 3, 28 050 late Gaussians of 50 000 (27 926 - 27 953 in the other variants); |cut - uncut| / bar for visit 1 (grouped) and visit 2
(dense_backward = 1), and the uncut render's own |second backward - first| / bar, the bar being 1e-5 max|ref| + 1e-4 |ref|:
    tensor       visit 1   visit 2   run to run          tensor        visit 1   visit 2   run to run
    means3D      0.002     0.001     0.002               features      0.004     0.004     0.002
    opacities    0.002     0.001     0.001               viewmatrix    0.024     0.011     0.032
    scales       0.045     0.008     0.045               projmatrix    0.002     0.002     0.002
    rotations    0.068     0.013     0.068               campos        0.001     0.001     0.002
    shs          0.002     0.002     0.002               means2D       0.003     0.001     0.002
The cut's difference is the run-to-run difference (float atomics; the figures move from run to run, another run gave 0.038 / 0.011 / 0.031
for rotations); no tensor's run-to-run ratio comes near a quarter of the bar.
Section 4: both backwards 0.049 (means2D) of the fp64 bar; dL_dfeatures of the second against the first 0.002 of it."""
import contextlib

import numpy as np
import pytest
import torch

import contrib_math as cm
import distort_math as dm
import features_math as fm
import posegrad_math as pm
import test_sparse_states_host as host
import variant_table as vt
from conftest import grad_tol, settings_from

pytestmark = pytest.mark.gpu

FORMS = dict(grouped=dict(late_fill_min_p=0), sparse=dict(late_fill_min_p=1 << 30), dense=dict(dense_backward=1))
SOURCES = ("features5", "features40", "distortion", "distortion_aux", "aux", "everything")
# (source, case, exp_mode): cases a and b in mode 0 (the camera source on posegrad_math's dense case a and raw case b); case a alone in modes 1 and 2, all at once
RUNS = [(src, name, 0) for src in SOURCES for name in cm.CASES] + [("pose_dense", "a", 0), ("pose_raw", "b", 0), ("everything", "a", 1), ("everything", "a", 2)]


def _t(a, gpu):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)


def _np(x):
    return x.detach().double().cpu().numpy()


@contextlib.contextmanager
def _options(rast, **switches):
    """The switches variant_table.switched does not list (test_sparse_states_host.SWITCH_DEFAULTS), their defaults back on the way out."""
    assert set(switches) <= set(host.SWITCH_DEFAULTS), set(switches) - set(host.SWITCH_DEFAULTS)
    try:
        for k, v in switches.items():
            rast._C.set_option(k, v)
        yield
    finally:
        for k in switches:
            rast._C.set_option(k, host.SWITCH_DEFAULTS[k])


@contextlib.contextmanager
def _poisoned(rast):
    """Every state buffer is handed out full of 0xFF bytes: a record nobody zeroed holds NaN."""
    rast._C.POISON_STATE_BUFFERS = True
    try:
        yield
    finally:
        rast._C.POISON_STATE_BUFFERS = False


def _launches(rast):
    import test_gpu_variants as tgv
    return tgv._launches(rast)


def _rows(a):
    """bool [P]: the rows of a [P, ...] array with a non-zero entry."""
    a = np.asarray(a)
    return (a.reshape(a.shape[0], -1) != 0).any(axis=1)


# ---- one render through the module, every keyword ---------------------------------------------------------------------------------------------
def _render(rast, gpu, sc, cam, *, F=None, distortion=False, aux=False, aa=False, raw=False, camera=False, contrib=False, absgrad=False):
    """One forward with every leaf requiring grad.  dict(color, radii, depth, acc, alpha, fmap, dmap, leaves, m2, F, rs, sink, abs)."""
    P = sc["means3D"].shape[0]
    rs = settings_from(rast, cam, sc, gpu)
    if camera:
        rs = rs._replace(**{k: getattr(rs, k).clone().requires_grad_(True) for k in pm.CAMERA})
    kw = dict(return_aux=aux, antialiasing=aa, distortion=distortion)
    Ft = None
    if F is not None:
        Ft = _t(F, gpu).requires_grad_(True)
        kw["features"] = Ft
    if camera:
        kw["camera_grads"] = True
    sink = torch.full((P, 4), float("nan"), device=gpu) if contrib else None
    if contrib:
        kw["contrib"] = sink
    ab = torch.full((P, 2), float("nan"), device=gpu) if absgrad else None
    if absgrad:
        kw["absgrad"] = ab
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    if raw:
        leaves = {n: _t(v, gpu).requires_grad_(True) for n, v in fm.raw_arrays(sc).items()}
        out = rast.GaussianRasterizerRaw(rs)(means2D=m2, **leaves, **kw)
    else:
        leaves = {n: _t(sc[n], gpu).requires_grad_(True) for n in fm.DENSE}
        out = rast.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"], scales=leaves["scales"],
                                          rotations=leaves["rotations"], shs=leaves["shs"], **kw)
    out = list(out)
    assert len(out) == 3 + 2 * int(aux) + int(F is not None) + int(distortion)
    h = dict(color=out[0], radii=out[1], depth=out[2], acc=None, alpha=None, fmap=None, dmap=None, leaves=leaves, m2=m2, F=Ft, rs=rs, sink=sink, abs=ab, camera=camera)
    k = 3
    if aux:
        h["acc"], h["alpha"] = out[3], out[4]
        k = 5
    if F is not None:
        h["fmap"] = out[k]
        k += 1
    if distortion:
        h["dmap"] = out[k]
    return h


def _loss(h, up, gpu):
    """sum color g0 + sum distort gd + sum acc_depth gD + sum alpha gA + sum feature_map g1, over the upstream gradients `up` holds."""
    loss = 0.0
    for key, x in (("g0", h["color"]), ("gd", h["dmap"]), ("g1", h["fmap"])):
        if key in up:
            assert x is not None, key
            loss = loss + (x * _t(up[key], gpu)).sum()
    for key, x in (("gD", h["acc"]), ("gA", h["alpha"])):
        if key in up:
            assert x is not None, key
            loss = loss + (x[0] * _t(up[key], gpu)).sum()
    return loss


def _collect(h):
    """What one backward left: dict(grads {leaf, means2D [P,2], features}, m2 [P,3], camera {..} or None, abs [P,2] or None)."""
    z = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else _np(x.grad)      # noqa: E731
    torch.cuda.synchronize()
    grads = {n: z(x) for n, x in h["leaves"].items()}
    m2 = z(h["m2"])
    grads["means2D"] = m2[:, :2]
    if h["F"] is not None:
        grads["features"] = z(h["F"])
    cam = {k: z(getattr(h["rs"], k)) for k in pm.CAMERA} if h["camera"] else None
    return dict(grads=grads, m2=m2, camera=cam, abs=None if h["abs"] is None else _np(h["abs"]), radii=h["radii"].cpu().numpy(),
                sink=None if h["sink"] is None else h["sink"].clone())


def _clear(h):
    for x in list(h["leaves"].values()) + [h["m2"], h["F"]] + ([getattr(h["rs"], k) for k in pm.CAMERA] if h["camera"] else []):
        if x is not None:
            x.grad = None


def _worst(got, want, tol):
    return float((np.abs(got - want) / np.maximum(tol, 1e-300)).max())


def _against_fp64(got, r64, r32, what):
    """Every tensor of r64 within conftest.grad_tol(r64, r32); returns (the worst err / bar, its tensor)."""
    worst = (0.0, "")
    for n, w in r64.items():
        assert n in got, (what, n, "the device side produced no gradient of this name")
        want = np.asarray(w, np.float64).reshape(got[n].shape)
        tol = grad_tol(want, np.asarray(r32[n], np.float64).reshape(got[n].shape) if r32 is not None and n in r32 else None)
        ratio = _worst(got[n], want, tol)
        worst = max(worst, (ratio, n))
        assert np.abs(want).max() > 0 or n in ("shs", "features_dc", "features_rest", "shs_res"), (what, n)
        assert ratio <= 1.0, (what, n, ratio, float(np.abs(got[n] - want).max()), float(np.abs(want).max()))
    return worst


# ---- 1. the touched bits contain every replay's contributors ------------------------------------------------------------------------------------
def _state(rast, gpu, sc, cam, raw, aa, aux=False):
    """One low-level forward a backward could follow (forward_only = False).  (the state tuple, the tensors it reads, P)."""
    _C = rast._C
    rs = settings_from(rast, cam, sc, gpu)
    H, W, P = cam["image_height"], cam["image_width"], sc["means3D"].shape[0]
    e = torch.empty(0)
    if raw:
        arrs = fm.raw_arrays(sc)
        arrs["opacity_logit"] = arrs.pop("opacity")
        ten = {n: (_t(arrs[n], gpu) if n in arrs else None) for n in _C.RAW_NAMES}
        st = _C.rasterize_gaussians_raw(rs.bg, ten, 1.0, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, rs.sh_degree, rs.campos, aux=aux, antialiasing=aa)
    else:
        ten = {n: _t(sc[n], gpu) for n in fm.DENSE}
        st = _C.rasterize_gaussians(rs.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                    rs.tanfovy, H, W, ten["shs"], rs.sh_degree, rs.campos, False, aux=aux, antialiasing=aa)
    return st, ten, P


def _touched(rast, gpu, P, gb):
    flags = torch.zeros(P, dtype=torch.uint8, device=gpu)
    assert rast._C.lib().gsrast_touched_rows(P, gb.data_ptr(), flags.data_ptr(), rast._C._stream_of(gpu)) == 0
    torch.cuda.synchronize()
    return flags.cpu().numpy()


@pytest.mark.parametrize("family", ["dense", "raw"])
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_touched_bits_contain_every_replays_contributors(name, mode, aa, family, rast, gpu):
    """On the state one forward left: the flag is 1 on every row contrib_stats counts a pixel for and on every id pixel_contributors(16,
    "depth") returns, 0 on every culled row; in exp_mode 0 the contributors off the ambiguous pixels are the fp64 table's.  With
    touch_bits = 0 every flag is 1 (SC_TOUCH_VALID is off).  A flagged row that contributes to nothing is a cost, not an error: printed."""
    _C = rast._C
    r, rows = cm.reference(name, aa), host.rows_of_case(name, aa)
    sc, cam = r["sc"], r["cam"]
    H, W = cam["image_height"], cam["image_width"]
    assert int(rows["nothing"].sum()) >= 10 and int(rows["culled"].sum()) == host.CULLED[name] and rows["amb"].mean() <= 0.007
    with vt.switched(rast, dict(exp_mode=mode)):
        st, ten, P = _state(rast, gpu, sc, cam, family == "raw", aa)
        R, radii, gb, bb, ib = st[0], st[2], st[3], st[4], st[5]
        flags = _touched(rast, gpu, P, gb)
        sink, sink_w = torch.full((P, 4), float("nan"), device=gpu), torch.full((P, 4), float("nan"), device=gpu)
        _C.contrib_stats(sink, None, R, W, H, gb, bb, ib)
        ids, _, count = _C.pixel_contributors(16, "depth", R, W, H, gb, bb, ib, P=P)
        _C.contrib_stats(sink_w, _t(r["weights"], gpu), R, W, H, gb, bb, ib)
        torch.cuda.synchronize()
        with _options(rast, touch_bits=0):
            st0, ten0, _ = _state(rast, gpu, sc, cam, family == "raw", aa)
            flags0 = _touched(rast, gpu, P, st0[3])
    what = f"case {name}, exp_mode {mode}, {'antialias' if aa else 'plain'}, {family}"
    radii, sink, sink_w, ids = radii.cpu().numpy(), _np(sink), _np(sink_w), ids.cpu().numpy()
    assert np.array_equal(radii > 0, rows["vis"]), "radius decision differs: pick another seed"
    assert not np.isnan(sink).any() and set(np.unique(flags)) <= {0, 1}
    contributing = sink[:, 2] > 0
    assert int(contributing.sum()) > 100 and int(count.max()) > 0
    assert (flags[contributing] == 1).all(), (what, int((flags[contributing] == 0).sum()), "Gaussians that contribute to a pixel have no touched bit")
    listed = np.unique(ids[ids >= 0])
    assert len(listed) > 100 and (flags[listed] == 1).all(), (what, "an id of pixel_contributors has no touched bit")
    assert contributing[listed].all(), (what, "an id of pixel_contributors that contrib_stats counts no pixel for")
    assert not flags[radii == 0].any(), (what, "a culled row is flagged")
    if mode == 0:
        assert np.array_equal(sink_w[:, 2] > 0, r["table"][:, 2] > 0), (what, "the contributors off the ambiguous pixels are not the fp64 table's")
        assert np.array_equal(sink_w[:, 2] > 0, rows["contributing"])
    idle = int(((flags == 1) & ~contributing).sum())
    print(f"{what}: {int((flags == 1).sum())} of {P} rows flagged, {int(contributing.sum())} contribute, {idle} flagged rows contribute to nothing "
          f"({int(((flags == 0) & (radii > 0)).sum())} visible rows are not flagged)")
    assert (flags0 == 1).all(), (what, "touch_bits = 0: a flag is not 1")


# ---- 2. every gradient source over poisoned, sparsely zeroed records, in every backward form ----------------------------------------------------
_sources, _runs = {}, {}


def _source(src, name):
    """dict(sc, cam, kw = _render's keywords, up = the upstream gradients, r64 / r32 = the fp64 / fp32 gradients, rows, bwd = (features_bwd,
    distort_bwd) launches of one backward) of a loss source on a case; the camera source: dict(pose = its reference, rows, bwd)."""
    if (src, name) in _sources:
        return _sources[src, name]
    if src.startswith("pose_"):
        import test_gpu_variants as tgv
        kind = src[len("pose_"):]
        assert host.POSE_LETTERS[kind] == name
        s = dict(pose=tgv._pose_reference(kind), rows=host.rows_of_pose_case(name), bwd=(0, 0))
    elif src.startswith("features"):
        rf = fm.reference(name, int(src[len("features"):]), colour_loss=False)
        s = dict(sc=rf["sc"], cam=rf["cam"], kw=dict(F=rf["F"]), up=dict(g1=rf["r64"]["g1"]), r64=rf["r64"]["grads"], r32=rf["r32"]["grads"], amb=rf["r64"]["amb"], bwd=(1, 0))
    elif src == "distortion":
        rd = dm.reference(name, "plain", colour_loss=False)
        s = dict(sc=rd["sc"], cam=rd["cam"], kw=dict(distortion=True), up=dict(gd=rd["r64"]["g"]["gd"]), r64=rd["r64"]["grads"], r32=rd["r32"]["grads"], amb=rd["r64"]["amb"], bwd=(0, 1))
    elif src == "distortion_aux":
        rd = dm.reference(name, "return_aux")
        s = dict(sc=rd["sc"], cam=rd["cam"], kw=dict(distortion=True, aux=True), up=dict(rd["r64"]["g"]), r64=rd["r64"]["grads"], r32=rd["r32"]["grads"], amb=rd["r64"]["amb"], bwd=(0, 1))
    elif src == "aux":
        a = host.aux_only(name)
        s = dict(sc=a["sc"], cam=a["cam"], kw=dict(aux=True), up=dict(gD=a["g"]["gD"], gA=a["g"]["gA"]), r64=a["r64"]["grads"], r32=a["r32"]["grads"], amb=a["r64"]["amb"], bwd=(0, 0))
    else:
        assert src == "everything"
        e = host.everything(name)
        rf = e["rf"]
        s = dict(sc=rf["sc"], cam=rf["cam"], kw=dict(F=rf["F"], distortion=True, aux=True, aa=True, raw=True, camera=True, contrib=True, absgrad=True),
                 up=dict(g1=rf["r64"]["g1"], g0=rf["r64"]["g0"], gd=e["g"]["gd"], gD=e["g"]["gD"], gA=e["g"]["gA"]),
                 r64=host.summed(rf["r64"]["grads"], e["d64"]["grads"]), r32=host.summed(rf["r32"]["grads"], e["d32"]["grads"]), amb=e["d64"]["amb"], bwd=(1, 1))
    if "rows" not in s:
        s["rows"] = host.rows_of_case(name, bool(s["kw"].get("aa")))
        assert np.array_equal(s["amb"], s["rows"]["amb"]), (src, name, "the source's reference masks other pixels than the pair table")
    _sources[src, name] = s
    return s


def _execute(rast, gpu, s, mode, form, sparse):
    """One forward + backward of a source under poisoned state buffers; dict(_collect's, counts)."""
    import test_gpu_posegrad as tgp
    with _poisoned(rast), _options(rast, sparse_grec=sparse), vt.switched(rast, dict(exp_mode=mode, **FORMS[form])), _launches(rast) as n:
        if "pose" in s:
            r = s["pose"]
            rs = tgp._settings(rast, r["cam"], r["sc"], gpu, grad=True)
            run = tgp._render(rast, r, rs, gpu, True)
            m2 = _np(run["m2"].grad)
            grads = {k: _np(x.grad) for k, x in run["leaves"].items()}
            grads["means2D"] = m2[:, :2]
            got = dict(grads=grads, m2=m2, camera=tgp._camera_grads(rs), abs=None, sink=None, radii=run["res"][1].cpu().numpy())
        else:
            h = _render(rast, gpu, s["sc"], s["cam"], **s["kw"])
            _loss(h, s["up"], gpu).backward()
            got = _collect(h)
    got["counts"] = n
    return got


def _run(rast, gpu, src, name, mode, form):
    """(with sparse_grec = 1, with sparse_grec = 0) of one source in one backward form, once per process."""
    key = (src, name, mode, form)
    if key not in _runs:
        s = _source(src, name)
        assert rast._C.get_option("sparse_grec") == 1 and rast._C.get_option("touch_bits") == 1
        _runs[key] = (_execute(rast, gpu, s, mode, form, 1), _execute(rast, gpu, s, mode, form, 0))
    return _runs[key]


def _expected_launches(s, form, sparse):
    return dict(late_rows_zero=int(form == "grouped"), grec_zero_touched=int(sparse), features_bwd=s["bwd"][0], distort_bwd=s["bwd"][1], blend_bwd=1, preprocess_bwd=1)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("src,name,mode", RUNS, ids=[f"{s}-{n}-mode{m}" for s, n, m in RUNS])
def test_gradient_sources_over_sparse_records(src, name, mode, form, rast, gpu):
    """Poisoned state buffers, sparse_grec = 1: every gradient finite and within grad_tol(r64, r32) of the fp64 reference of the source's own
    test file (all at once: the sum of the parts' fp64 gradients; modes 1 and 2: the mode-0 reference, which the default kernels of those
    modes meet with mode 0's margin -- tests/test_gpu_variants.py); the rows of the Gaussians that contribute to nothing exactly zero in every
    leaf, means2D.grad, dL_dfeatures and the absgrad sink; the non-zero rows those of the same run with sparse_grec = 0."""
    s = _source(src, name)
    got, got0 = _run(rast, gpu, src, name, mode, form)
    rows = s["rows"]
    what = f"{src}, case {name}, exp_mode {mode}, {form}"
    assert int(rows["nothing"].sum()) >= 10 and int(rows["culled"].sum()) >= 1 and rows["amb"].mean() < 0.05
    if "pose" in s:
        upstream = [s["pose"]["r64"][k] for k in ("g", "gD", "gA")]
    else:
        upstream = list(s["up"].values())
        assert int(rows["culled"].sum()) == host.CULLED[name] and rows["amb"].mean() <= 0.007
    assert all(not np.asarray(g)[..., rows["amb"]].any() for g in upstream if g is not None), "an upstream gradient is not zero on the ambiguous pixels"
    assert np.array_equal(got["radii"] > 0, rows["vis"]), "radius decision differs: pick another seed"
    tensors = dict(got["grads"], m2=got["m2"])
    tensors0 = dict(got0["grads"], m2=got0["m2"])
    if got["abs"] is not None:
        tensors["absgrad"], tensors0["absgrad"] = got["abs"], got0["abs"]
    for n, a in tensors.items():
        assert np.isfinite(a).all(), (what, n, int((~np.isfinite(a)).sum()), "entries are not finite")
    if "pose" in s:
        r = s["pose"]
        worst = _against_fp64(got["grads"], r["leaf64"], r["leaf32"], what)
        assert set(got["grads"]) == set(r["leaf64"])
        for k in pm.CAMERA:
            want = r["r64"]["want"][k]
            ratio = _worst(got["camera"][k], want, grad_tol(want, r["r32"]["want"][k]))
            worst = max(worst, (ratio, k))
            assert np.isfinite(got["camera"][k]).all() and ratio <= 1.0, (what, k, ratio)
        assert np.abs(got["camera"]["viewmatrix"]).max() > 0 and not got["camera"]["viewmatrix"][:, 3].any() and not got["camera"]["projmatrix"][:, 2].any()
    else:
        worst = _against_fp64(got["grads"], s["r64"], s["r32"], what)
        assert set(got["grads"]) == set(s["r64"]), (set(got["grads"]) ^ set(s["r64"]))
    dead = rows["culled"] | rows["nothing"]
    for n, a in tensors.items():
        assert not _rows(a)[dead].any(), (what, n, int(_rows(a)[dead].sum()), "rows of Gaussians that contribute to nothing are not zero")
        assert np.array_equal(_rows(a), _rows(tensors0[n])), (what, n, "the non-zero rows differ from those with sparse_grec = 0")
    if got["abs"] is not None:      # no fp64 reference of the sink at this shape: against the run whose records were zeroed whole, tests/test_gpu_absgrad.py's bar
        assert (got["abs"] >= 0).all() and got["abs"].max() > 0
        ratio = _worst(got["abs"], got0["abs"], grad_tol(got0["abs"]))
        assert ratio <= 1.0, (what, "absgrad sink", ratio)
    if got["sink"] is not None:     # the contrib sink is the forward's: no backward form may move it
        assert not torch.isnan(got["sink"]).any() and torch.equal(got["sink"], got0["sink"]) and float(got["sink"][:, 2].max()) > 0
    if src == "everything":         # (no fp64 camera reference for this combination: tests/test_gpu_features.py::test_every_keyword_at_once asserts the same)
        cam = got["camera"]
        assert all(np.isfinite(v).all() for v in cam.values()) and np.abs(cam["viewmatrix"]).max() > 0
        assert not cam["viewmatrix"][:, 3].any() and not cam["projmatrix"][:, 2].any()
    print(f"{what}: worst gradient err / bar {worst[0]:.3f} ({worst[1]}); {int(dead.sum())} rows contribute to nothing, {int(rows['nothing'].sum())} of them visible")


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_counts_show_what_ran(form, rast, gpu):
    """The profile window of every run of the test above: late_rows_zero 1 in the grouped form and 0 in the others, grec_zero_touched 1 with
    sparse_grec = 1 and 0 with 0, one features_bwd / distort_bwd per source that has one, one blend and one per-Gaussian backward.

    A backward with a feature or distortion gradient runs in two phases around the replays' backward; this test found that the plan took the
    grouped form in a one-phase call only (late_rows_zero 0 for features, distortion and everything at once, with late_fill_min_p = 0), so
    the grouped kernel never ran behind a replay.  gsrast_policy.h now asks for it in whichever call runs the per-Gaussian backward -- phase
    2 of two included (tests/test_policy.py::test_backward_plan_late_fill_conditions)."""
    misses = []
    for src, name, mode in RUNS:
        s = _source(src, name)
        for sparse, got in zip((1, 0), _run(rast, gpu, src, name, mode, form)):
            want = _expected_launches(s, form, sparse)
            n = {k: got["counts"][k] for k in want}
            print(f"{src}, case {name}, exp_mode {mode}, {form}, sparse_grec {sparse}: " + " ".join(f"{k} {v}" for k, v in n.items()))
            if n != want:
                misses.append((src, name, mode, f"sparse_grec {sparse}", {k: (n[k], want[k]) for k in want if n[k] != want[k]}))
    assert not misses, misses


# ---- 3. replays and gradients on list-cut states ------------------------------------------------------------------------------------------------
CUT_P, CUT_W, CUT_H = 50_000, 256, 192


def _cut_scene(scenes):
    sc = scenes.synth(CUT_P, 451)
    sc["opacities"] = (1.0 / (1.0 + np.exp(-(np.log(sc["opacities"] / (1.0 - sc["opacities"])) + 2.0)))).astype(np.float32)
    return sc, scenes.camera(2, 5, CUT_W, CUT_H)


def _visit(rast, gpu, sc, cam, raw, aa, Ft):
    """One low-level forward and every replay on its state.  (dict of named tensors, last_late)."""
    _C = rast._C
    H, W = cam["image_height"], cam["image_width"]
    st, ten, P = _state(rast, gpu, sc, cam, raw, aa, aux=True)
    late = _C.context_query("last_late")
    R, color, radii, gb, bb, ib, depth, acc, alpha = st
    out = dict(color=color, radii=radii, depth=depth, acc_depth=acc, alpha=alpha)
    out["distort_map"], out["moments"] = _C.distortion_forward(P, R, W, H, gb, bb, ib, gpu)
    out["feature_map"] = _C.features_forward(Ft, R, W, H, gb, bb, ib)
    for K, order in ((16, "weight"), (16, "depth"), (3, "weight")):
        out[f"ids_{K}_{order}"], out[f"weights_{K}_{order}"], out[f"count_{K}_{order}"] = _C.pixel_contributors(K, order, R, W, H, gb, bb, ib, P=P)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}, late, R


def _assert_same(cut, full, what):
    for k in full:
        assert torch.equal(cut[k], full[k]), (what, k, int((cut[k] != full[k]).sum()), "entries differ from the uncut visit")


@pytest.mark.remembered_cut_only
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("family", ["dense", "raw"])
def test_replays_on_list_cut_states_are_the_uncut_visits(family, aa, rast, gpu, scenes):
    """Visit 0 without the cut leaves the pose's cut depths; visits 1 and 2 leave the late Gaussians out of the lists, the colour kernel and
    the binning records.  Colour, depth, radii, acc_depth, alpha, the distortion map and its moments, the feature map (C = 19) and
    pixel_contributors (K = 16 in both orders, K = 3 by weight: ids, weights, count) of both cut visits are the uncut visit's bit for bit."""
    _C = rast._C
    sc, cam = _cut_scene(scenes)
    Ft = _t(fm.features_of(CUT_P, 19), gpu)
    with _options(rast, list_cut_always=1):
        with _options(rast, no_list_cut=1):
            full, late, R0 = _visit(rast, gpu, sc, cam, family == "raw", aa, Ft)
        assert late == 0
        for visit in (1, 2):
            cut, late, R = _visit(rast, gpu, sc, cam, family == "raw", aa, Ft)
            assert late > 0, "the repeated pose was expected to run under the list cut"
            print(f"{family}, {'antialias' if aa else 'plain'}, visit {visit}: {late} late Gaussians of {CUT_P}, {R} instances listed (uncut {R0})")
            _assert_same(cut, full, f"{family}, antialiasing {aa}, visit {visit}")
    assert not torch.isnan(full["distort_map"]).any() and float(full["distort_map"].max()) > 0 and float(full["feature_map"].abs().max()) > 0.5
    assert int(full["count_16_depth"].max()) > 16 and not torch.isnan(full["moments"]).any()


@pytest.mark.remembered_cut_only
def test_a_redone_cut_leaves_the_uncut_replays(rast, gpu, scenes):
    """The scene turns nearly transparent between two visits (tests/test_gpu_parity.py::test_list_cut_under_a_changing_scene's edit): the cut
    is applied, found too short and redone from the full lists (cut_fallbacks + 1); the distortion map, its moments and pixel_contributors
    after the redo are the uncut render's of the new scene bit for bit."""
    _C = rast._C
    sc, cam = _cut_scene(scenes)
    Ft = _t(fm.features_of(CUT_P, 19), gpu)
    thin = dict(sc, opacities=(sc["opacities"] * 0.02).astype(np.float32))
    with _options(rast, list_cut_always=1):
        with _options(rast, no_list_cut=1):
            _, late, _ = _visit(rast, gpu, sc, cam, False, False, Ft)
        assert late == 0
        _, late, _ = _visit(rast, gpu, sc, cam, False, False, Ft)
        assert late > 0
        fb0 = _C.context_query("cut_fallbacks")
        cut, late, _ = _visit(rast, gpu, thin, cam, False, False, Ft)
        assert late > 0, "the cut was expected to be applied to the changed scene"
        assert _C.context_query("cut_fallbacks") == fb0 + 1, "the cut was expected to be found too short and redone"
        with _options(rast, no_list_cut=1):
            full, late, _ = _visit(rast, gpu, thin, cam, False, False, Ft)
        assert late == 0
    _assert_same(cut, full, "after the redo")
    assert float(full["distort_map"].max()) > 0 and int(full["count_16_depth"].max()) > 16


@pytest.mark.remembered_cut_only
def test_gradients_on_list_cut_states(rast, gpu, scenes):
    """Loss on colour + distortion map + feature map + acc_depth + alpha with camera_grads, poisoned buffers: two uncut backwards (visit 0's
    inputs twice, for the run-to-run difference), then visit 1 with the grouped backward and visit 2 with dense_backward = 1, both under the
    cut.  Every leaf, dL_dfeatures and the three camera gradients: the uncut visit's zero rows, exact zeros on every row no pixel blends
    (the late Gaussians among them: the contrib sink of the same render counts no pixel for them), values within 1e-5 max|ref| + 1e-4 |ref|
    of the uncut visit.  Prints, per tensor, the cut's and the run-to-run difference as a share of that bar."""
    _C = rast._C
    sc, cam = _cut_scene(scenes)
    H, W = CUT_H, CUT_W
    rng = np.random.default_rng(453)
    up = dict(g0=scenes.upstream_grad(H, W, 452) * (H * W), g1=rng.normal(size=(19, H, W)), gd=rng.normal(size=(H, W)), gD=rng.normal(size=(H, W)) * 0.25,
              gA=rng.normal(size=(H, W)))
    F = fm.features_of(CUT_P, 19)

    def visit(form):
        with vt.switched(rast, form):
            h = _render(rast, gpu, sc, cam, F=F, distortion=True, aux=True, camera=True, contrib=True)
            late = _C.context_query("last_late")
            _loss(h, up, gpu).backward()
            got = _collect(h)
        got["late"], got["out"] = late, {k: h[k].detach().clone() for k in ("color", "radii", "depth", "acc", "alpha", "fmap", "dmap")}
        return got

    with _poisoned(rast), _options(rast, list_cut_always=1):
        with _options(rast, no_list_cut=1):
            ref, again = visit({}), visit({})
        assert ref["late"] == 0 and again["late"] == 0
        cuts = [("visit 1, grouped", visit(FORMS["grouped"])), ("visit 2, dense", visit(FORMS["dense"]))]
    flat = lambda g: dict(g["grads"], m2=g["m2"], **g["camera"])      # noqa: E731
    want, noise = flat(ref), flat(again)
    blended = _np(ref["sink"])[:, 2] > 0
    assert not torch.isnan(ref["sink"]).any() and int(blended.sum()) > 1000 and int((~blended).sum()) > CUT_P // 4
    for what, got in cuts:
        assert got["late"] > 0, "the repeated pose was expected to run under the list cut"
        for k, v in ref["out"].items():
            assert torch.equal(got["out"][k], v), (what, k)
        # a late Gaussian is in no list of this visit, so this visit's sink counts no pixel for it -- and the sink is the uncut visit's:
        # the late rows are among the rows no pixel blends
        assert torch.equal(got["sink"], ref["sink"]), what
        assert int((~blended).sum()) >= got["late"] + int((ref["radii"] == 0).sum())
        g = flat(got)
        worst = (0.0, "")
        for n, w in want.items():
            assert np.isfinite(g[n]).all(), (what, n)
            tol = grad_tol(w)                                     # 1e-5 max|ref| + 1e-4 |ref|
            ratio, run_to_run = _worst(g[n], w, tol), _worst(noise[n], w, tol)
            worst = max(worst, (ratio, n))
            print(f"{what}: {n} max|ref| {np.abs(w).max():.3e} cut against uncut / bar {ratio:.3f}, uncut run to run / bar {run_to_run:.3f}")
            assert np.abs(w).max() > 0, n
            if n not in pm.CAMERA:
                assert np.array_equal(_rows(g[n]), _rows(w)), (what, n, "the zero rows are not the uncut visit's")
                assert not _rows(g[n])[~blended].any() and not _rows(w)[~blended].any(), (what, n, "a row no pixel blends is not zero")
            else:                                                 # the camera: the same entries are zero (viewmatrix's last column, projmatrix's third)
                assert np.array_equal(g[n] != 0, w != 0), (what, n)
            assert ratio <= 1.0, (what, n, ratio, run_to_run)
        print(f"{what}: {got['late']} late Gaussians; worst cut against uncut / bar {worst[0]:.3f} ({worst[1]})")


# ---- 4. a second backward on the same state ------------------------------------------------------------------------------------------------------
def test_second_backward_on_a_state_with_features_and_distortion(rast, gpu):
    """Case a, features C = 19 + distortion + aux + colour, retain_graph, poisoned buffers: the second backward finds records the first one
    used (it zero-fills all of them by memset, no second grec_zero_touched) and runs both replays' backward again.  Every gradient of both
    backwards within grad_tol of fp64, the first backward's zero rows, dL_dfeatures overwritten and not accumulated."""
    t = host.retained("a")
    rf = t["rf"]
    r64, r32 = host.summed(rf["r64"]["grads"], t["d64"]["grads"]), host.summed(rf["r32"]["grads"], t["d32"]["grads"])
    up = dict(g1=rf["r64"]["g1"], g0=rf["r64"]["g0"], gd=t["g"]["gd"], gD=t["g"]["gD"], gA=t["g"]["gA"])
    rows = host.rows_of_case("a")
    with _poisoned(rast), _launches(rast) as n:
        h = _render(rast, gpu, rf["sc"], rf["cam"], F=rf["F"], distortion=True, aux=True)
        loss = _loss(h, up, gpu)
        loss.backward(retain_graph=True)
        first = _collect(h)
        _clear(h)
        loss.backward()
        second = _collect(h)
    assert n["features_bwd"] == 2 and n["distort_bwd"] == 2 and n["blend_bwd"] == 2 and n["preprocess_bwd"] == 2, n
    assert n["grec_zero_touched"] == 1 and n["features_fwd"] == 1 and n["distort_fwd"] == 1, n
    dead = rows["culled"] | rows["nothing"]
    for what, got in (("first backward", first), ("second backward", second)):
        assert all(np.isfinite(a).all() for a in got["grads"].values()) and np.isfinite(got["m2"]).all(), what
        worst = _against_fp64(got["grads"], r64, r32, what)
        print(f"{what}: worst gradient err / bar {worst[0]:.3f} ({worst[1]})")
        for name, a in dict(got["grads"], m2=got["m2"]).items():
            assert not _rows(a)[dead].any(), (what, name)
    for name, a in dict(second["grads"], m2=second["m2"]).items():
        assert np.array_equal(_rows(a), _rows(dict(first["grads"], m2=first["m2"])[name])), (name, "the second backward's zero rows are not the first's")
    wF = np.asarray(r64["features"])
    ratio = _worst(second["grads"]["features"], first["grads"]["features"], grad_tol(wF, r32["features"]))
    print(f"dL_dfeatures, second backward against the first: worst |difference| / bar {ratio:.3f}")
    assert ratio <= 1.0 and (np.abs(wF) > 100 * grad_tol(wF, r32["features"])).any()      # (accumulated, it would be twice the first)
