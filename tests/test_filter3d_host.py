"""Mip-Splatting's 3-D smoothing filter, host side (no GPU): tests/filter3d_math.py against a literal transcription of upstream's
``compute_3D_filter`` loop and its two getters (fp64 torch on the CPU, and torch.autograd of the sqrt(det1 / det2) composition), the fp32
bit model against the fp64 sweep, the edge rows, the C ABI of gsrast_filter3d_* (declared, exported, bound, every argument error refused
before any device call) and fused_filter3d.py's refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

import filter3d_math as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gsrast_filter3d_scratch_bytes", "gsrast_filter3d_compute", "gsrast_filter3d_apply_forward", "gsrast_filter3d_apply_backward")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def sweeps(scenes):
    """per case of fm.SWEEP_CASES: (xyz fp32, table fp64 of fp32 values, focal_max, cameras, the fp32 run, the fp64 run), computed once"""
    out = {}
    for P, V, radius in fm.SWEEP_CASES:
        xyz = scenes.synth(P, seed=3)["means3D"]
        cams = fm.ring(scenes, V, radius)
        table, fmax = fm.table_of(cams)
        out[(P, V, radius)] = (xyz, table, fmax, cams, fm.sweep(xyz, table, np.float32, fmax), fm.sweep(xyz, table, np.float64, fmax))
    return out


@pytest.mark.parametrize("case", fm.SWEEP_CASES)
def test_fp64_sweep_equals_the_upstream_loop(case, sweeps):
    xyz, table, fmax, cams, _, r64 = sweeps[case]
    filt, valid = fm.upstream_compute_3D_filter(torch.tensor(xyz, dtype=torch.float64), [fm.UpstreamCamera(c) for c in cams], torch.float64)
    sure = ~r64["ambiguous"]
    assert r64["ambiguous"].mean() <= 0.02
    assert np.array_equal(valid.numpy()[sure], r64["valid"][sure])
    want = filt.numpy()[sure]
    assert (np.abs(r64["filter"][sure] - want) <= 1e-12 * np.abs(want)).all()
    assert 0.5 < r64["valid"].mean() < 0.95      # both branches are populated


@pytest.mark.parametrize("case", fm.SWEEP_CASES)
def test_fp32_sweep_meets_fp64(case, sweeps):
    xyz, table, _, _, r32, r64 = sweeps[case]
    frac = r64["ambiguous"].mean()
    print(f"case {case}: ambiguous {100 * frac:.2f} %, valid {r64['valid'].mean():.2f}, valid differences {(r32['valid'] != r64['valid']).sum()}")
    assert frac <= 0.02      # a condition, not a measurement
    assert np.array_equal(r32["valid"], r64["valid"])
    rows = ~r64["ambiguous"] & r64["valid"]
    cam = table[r64["cam"][rows]]
    x = xyz[rows].astype(np.float64)
    bar = 4 * ULP * (np.abs(x[:, 0] * cam[:, 2]) + np.abs(x[:, 1] * cam[:, 5]) + np.abs(x[:, 2] * cam[:, 8]) + np.abs(cam[:, 11]))
    err = np.abs(r32["dist"][rows].astype(np.float64) - r64["dist"][rows])
    print(f"  worst |dist32 - dist64| / bar = {(err / bar).max():.3f}")
    assert (err <= bar).all()


def test_apply_restatement_equals_autograd_of_upstreams_composition():
    s, o, f, g_s, g_o = (a.astype(np.float64) for a in fm.apply_case(20000, seed=1, edges=False))
    ts, to = torch.tensor(s, requires_grad=True), torch.tensor(o, requires_grad=True)
    tf = torch.tensor(f)
    want_s, want_o = fm.upstream_scaling(ts, tf), fm.upstream_opacity(to, ts, tf)
    (want_s * torch.tensor(g_s)).sum().add((want_o * torch.tensor(g_o)).sum()).backward()
    sf, of, _ = fm.apply_fwd(s, o, f)
    ds, do, _, _ = fm.apply_bwd(s, o, f, g_s, g_o)
    worst = 0.0
    for got, want in ((sf, want_s), (of, want_o), (ds, ts.grad), (do, to.grad)):
        want = want.detach().numpy()
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f"worst relative difference to autograd: {worst:.2e}")
    assert worst <= 1e-12


def test_edge_rows_are_exact():
    s, f, o = (np.float64(fm.EDGE_ROWS[k]) for k in ("s", "f", "o"))
    g_s, g_o = np.full((4, 3), 0.5), np.full((4, 1), -2.0)
    sf, of, coef = fm.apply_fwd(s, o, f)
    ds, do, _, _ = fm.apply_bwd(s, o, f, g_s, g_o)
    # s = 0, f = 0: s_f = 0, o_f = o, d s = g_s, d o = g_o
    assert not sf[0].any() and of[0, 0] == o[0] and np.array_equal(ds[0], g_s[0]) and do[0, 0] == g_o[0, 0]
    # one zero axis with f = 0: that axis's ratio is 1, the others' too (s / s)
    assert np.array_equal(sf[3], s[3]) and of[3, 0] == o[3] and np.array_equal(ds[3], g_s[3])
    assert np.isfinite(sf).all() and np.isfinite(of).all() and np.isfinite(ds).all() and np.isfinite(do).all()


def test_thin_rows_stay_finite_in_fp32_where_upstreams_form_does_not():
    """the ratio form evaluated in fp32 (numpy, the kernel's expressions) meets fp64 on the thin rows; the transcription's fp32 gives 0 or
    NaN there -- the deviation, pinned"""
    s32, f32, o32 = np.float32(fm.EDGE_ROWS["s"][1:3]), np.float32(fm.EDGE_ROWS["f"][1:3]), np.float32(fm.EDGE_ROWS["o"][1:3])
    sf = np.sqrt(s32 * s32 + (f32 * f32)[:, None])
    r = s32 / sf
    of = o32 * ((r[:, 0] * r[:, 1]) * r[:, 2])
    assert sf.dtype == np.float32 and of.dtype == np.float32
    _, want, _ = fm.apply_fwd(s32, o32, f32)
    assert np.isfinite(of).all() and (of > 0).all() and np.abs(of - want[:, 0]).max() <= 8 * ULP * np.abs(want).max()
    assert (np.abs(of - want[:, 0]) <= 8 * ULP * np.abs(want[:, 0])).all()
    up = fm.upstream_opacity(torch.tensor(o32)[:, None], torch.tensor(s32), torch.tensor(f32)[:, None]).numpy()[:, 0]
    assert up.dtype == np.float32 and all(v == 0.0 or math.isnan(v) for v in up)


def test_sweep_edge_rows(scenes):
    cams = fm.ring(scenes, 5)
    table, fmax = fm.table_of(cams)
    xyz = scenes.synth(64, seed=3)["means3D"].copy()
    xyz[3] = np.nan
    xyz[5] = (np.inf, 0.0, 0.0)
    xyz[7] = (0.0, -np.inf, 0.1)
    for dt in (np.float32, np.float64):
        r = fm.sweep(xyz, table, dt, fmax)
        assert r["valid"].sum() > 30 and not r["valid"][[3, 5, 7]].any()
        assert (r["filter"][[3, 5, 7], 0] == r["dmax"] * r["k"]).all() and np.isfinite(r["filter"]).all() and r["filter"].dtype == dt
    # no valid row: all zeros (upstream raises)
    far = np.tile(np.float32([[0.0, 1e6, 0.0]]), (17, 1))      # far below every camera of the ring: off every screen
    r = fm.sweep(far, table, np.float32, fmax)
    assert not r["valid"].any() and not r["filter"].any() and not np.signbit(r["filter"]).any()
    with pytest.raises(RuntimeError):
        fm.upstream_compute_3D_filter(torch.tensor(far), [fm.UpstreamCamera(c) for c in cams])
    # a table that sees nothing
    r = fm.sweep(xyz, np.zeros((3, 16)), np.float32, fmax)
    assert not r["valid"].any() and not r["filter"].any()


def test_symbols_are_declared_exported_and_bound(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    import capi_header
    L = rast._C.lib()
    protos = capi_header.prototypes()
    for name in SYMBOLS:
        assert name in protos and name in rast._C.SIGNATURES and name in rast._C.EXPORTS and getattr(L, name).argtypes is not None, name
    assert not any("filter3d" in s for s in capi_header.structs())      # plain scalars and pointers: no descriptor
    text = capi_header.text()
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6 and re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == 34 and not any("filter3d" in n for n in names)      # the profile table is unchanged
    units = {f: open(os.path.join(ROOT, "saro-gs_amd", "csrc", f)).read() for f in ("gsrast_capi.hip", "gsrast_train.hip")}
    assert '#include "gsrast_filter3d.h"' in units["gsrast_train.hip"] and "gsrast_filter3d.h" not in units["gsrast_capi.hip"]


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    L = rast._C.lib()
    one = 256      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")

    def comp(P=5, C=3, m=one, t=one, near=0.2, margin=0.15, variance=0.2, focal_max=100.0, f=one, v=one, scratch=one):
        return L.gsrast_filter3d_compute(P, C, m, t, near, margin, variance, focal_max, f, v, scratch, None)

    who = "filter3d_compute"
    assert comp(P=-1) == -1 and err() == f"{who}: negative P"
    for C in (0, -2):
        assert comp(C=C) == -1 and err() == f"{who}: C must be >= 1"
    for name in ("near", "variance", "focal_max"):
        for bad in (0.0, -1.0, nan, inf, -inf):
            assert comp(**{name: bad}) == -1 and err() == f"{who}: {name} must be finite and > 0", (name, bad)
    for bad in (-1e-9, nan, inf):
        assert comp(margin=bad) == -1 and err() == f"{who}: margin must be finite and >= 0", bad
    for p in "mtf":
        assert comp(**{p: None}) == -1 and err() == f"{who}: NULL required pointer", p
    assert comp(scratch=None) == -1 and err() == f"{who}: NULL scratch"
    assert comp(P=0) == 0 and comp(P=0, m=None, f=None, v=None, scratch=None) == 0      # no row, no launch
    assert comp(P=0, near=nan) == -1      # (the scalars are checked whatever P is)

    def fwd(P=5, s=one, o=one, f=one, sf=one, of=one):
        return L.gsrast_filter3d_apply_forward(P, s, o, f, sf, of, None)

    def bwd(P=5, s=one, o=one, f=one, gs=one, go=one, ds=one, do=one):
        return L.gsrast_filter3d_apply_backward(P, s, o, f, gs, go, ds, do, None)

    for who, call, pointers in (("filter3d_apply_forward", fwd, ("s", "o", "f", "sf", "of")), ("filter3d_apply_backward", bwd, ("s", "o", "f"))):
        assert call(P=-1) == -1 and err() == f"{who}: negative P"
        for p in pointers:
            assert call(**{p: None}) == -1 and err() == f"{who}: NULL required pointer", (who, p)
        assert call(P=0) == 0
    assert bwd(ds=None, do=None) == -1 and err() == "filter3d_apply_backward: d_scales and d_opacities are both NULL"
    assert bwd(P=0, ds=None, do=None) == -1

    assert L.gsrast_filter3d_scratch_bytes(-1, 3) == 0 and err() == "filter3d_scratch_bytes: negative P"
    assert L.gsrast_filter3d_scratch_bytes(5, 0) == 0 and err() == "filter3d_scratch_bytes: C must be >= 1"
    assert L.gsrast_filter3d_scratch_bytes(0, 1) >= 8 and L.gsrast_filter3d_scratch_bytes(3000000, 300) >= 8


class _Cam:
    def __init__(self, cam):
        self.__dict__.update(cam)


def test_camera_tables_on_the_cpu(scenes):
    """the table's layout and focal_max need no GPU: built on the CPU device, from dicts, objects and arrays alike"""
    import fused_filter3d as ff
    cams = fm.ring(scenes, 4)
    want, fmax = fm.table_of(cams, np.float32)
    for table in (ff.camera_table(cams, "cpu"), ff.camera_table([_Cam(c) for c in cams], "cpu"),
                  ff.camera_table([dict(c, viewmatrix=torch.tensor(c["viewmatrix"])) for c in cams], "cpu")):
        assert table.dtype == torch.float32 and tuple(table.shape) == (4, 16) and np.array_equal(table.numpy(), want) and table.focal_max == fmax
    up = [fm.UpstreamCamera(c) for c in cams]
    arr = ff.camera_table_from_arrays(np.stack([u.R for u in up]), np.stack([u.T for u in up]), [u.focal_x for u in up], [u.focal_y for u in up],
                                      [u.image_width for u in up], [u.image_height for u in up], device="cpu")
    assert np.array_equal(arr.numpy(), want) and arr.focal_max == fmax
    one = ff.camera_table_from_arrays(torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), 100.0, 90.0, 64, 48)
    assert one.focal_max == 100.0 and one[:, 12:].tolist() == [[100.0, 90.0, 64.0, 48.0]] * 2
    for bad in (lambda: ff.camera_table([], "cpu"), lambda: ff.camera_table_from_arrays(np.zeros((2, 3, 3)), np.zeros((2, 3)), 1.0, 1.0, 4, 4),
                lambda: ff.camera_table_from_arrays(torch.zeros(2, 3, 4), torch.zeros(2, 3), 1.0, 1.0, 4, 4),
                lambda: ff.camera_table_from_arrays(torch.zeros(2, 3, 3), torch.zeros(3, 3), 1.0, 1.0, 4, 4),
                lambda: ff.camera_table_from_arrays(torch.zeros(2, 3, 3), torch.zeros(2, 3), [1.0, 2.0, 3.0], 1.0, 4, 4),
                lambda: ff.camera_table_from_arrays(torch.zeros(2, 3, 3), torch.zeros(2, 3), 0.0, 1.0, 4, 4)):
        with pytest.raises(ValueError):
            bad()


def test_python_refusals_need_no_device(monkeypatch):
    import fused_filter3d as ff
    monkeypatch.setattr(ff._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    P = 5
    m, s, o, f = torch.zeros(P, 3), torch.ones(P, 3), torch.ones(P, 1), torch.ones(P, 1)
    table = torch.zeros(2, 16)
    for call in (lambda: ff.compute_filter_3d(m, table, focal_max=10.0), lambda: ff.apply_filter_3d(s, o, f), lambda: ff.bake_filter_3d(s, o, f)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="tensor"):
        ff.apply_filter_3d(s.numpy(), o, f)
    # what is checked once the tensors pass for device tensors: dtype, shape, layout, the scalars (the device check stubbed out)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    comp = lambda mm=m, tt=table, **kw: ff.compute_filter_3d(mm, tt, **dict(dict(focal_max=10.0), **kw))  # noqa: E731
    app = lambda ss=s, oo=o, fff=f: ff.apply_filter_3d(ss, oo, fff)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    for call, text in ((lambda: comp(mm=m.double()), "float32"), (lambda: comp(mm=m[:, :2]), r"\[\*, 3\]"), (lambda: comp(mm=torch.zeros(3, P).t()), "contiguous"),
                       (lambda: comp(tt=torch.zeros(2, 15)), r"\[\*, 16\]"), (lambda: comp(tt=table.double()), "float32"), (lambda: comp(tt=torch.zeros(0, 16)), "at least one camera"),
                       (lambda: comp(tt=torch.zeros(16, 2).t()), "contiguous"), (lambda: comp(focal_max=None), "focal_max"),
                       (lambda: comp(near=0.0), "near"), (lambda: comp(near=nan), "near"), (lambda: comp(variance=-1.0), "variance"), (lambda: comp(variance=inf), "variance"),
                       (lambda: comp(focal_max=0.0), "focal_max"), (lambda: comp(margin=-0.1), "margin"), (lambda: comp(margin=nan), "margin"),
                       (lambda: app(ss=s.half()), "float32"), (lambda: app(ss=s[:, :2]), r"\[\*, 3\]"), (lambda: app(ss=torch.ones(3, P).t()), "contiguous"),
                       (lambda: app(oo=o[:4]), r"\[5, 1\]"), (lambda: app(oo=o[:, 0]), r"\[5, 1\]"), (lambda: app(oo=o.double()), "float32"),
                       (lambda: app(fff=f[:3]), r"\[5, 1\]"), (lambda: app(fff=f[:3, 0]), r"\[5\]"), (lambda: app(fff=f.double()), "float32"),
                       (lambda: app(fff=torch.ones(P, 2)[:, :1]), "contiguous")):
        with pytest.raises(ValueError, match=text):
            call()
    # another device: the tensors of one call live on one GPU
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 1 if getattr(self, "_elsewhere", False) else 0)))
    far_t, far_o, far_f = torch.zeros(2, 16), torch.ones(P, 1), torch.ones(P, 1)
    far_t._elsewhere = far_o._elsewhere = far_f._elsewhere = True
    for call in (lambda: comp(tt=far_t), lambda: app(oo=far_o), lambda: app(fff=far_f)):
        with pytest.raises(RuntimeError, match="is on cuda:1"):
            call()
