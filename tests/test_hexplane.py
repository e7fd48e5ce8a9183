"""Mip-mapped feature-plane lookup of the residual field (first item): the HIP kernels through
saro-gs_amd/fused_hexplane.py against oracle/texture_oracle.py (numpy fp64 restatement of the published texture op, pinned
against torch in tests/test_oracle_texture.py).  Tolerances: values 1e-5 abs; gradients 1e-5 of the largest entry (texel
gradients are sums over hundreds of points) -- and beside them, element by element,
    |T_gpu - T_64|_i <= 4 rho32 2^-24 s_i + 2^-24 |T_64|_i
with s_i from the oracle's absolute companion and rho32 the fp32 restatement's own worst error in units of 2^-24 s_i on the
same case (_bar): the first bar is absolute and set by the tensor's largest entry (texel gradients reach tens, so it sits
near 3e-4 on entries of order 1e-2); the second sees a dropped corner or a wrong weight on a thin top level.  A set of exact
cases (dyadic inputs) is compared with no tolerance at all.  What is covered, and the two branches that are not: see the
list above test_thin_and_odd_topped_stacks."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import texture_oracle as tor


def _points(rng, N, n_levels):
    uv = rng.uniform(-0.05, 1.05, size=(N, 2)).astype(np.float32)
    uv[:6] = [[0, 0], [1, 1], [0.5, 0.5], [1.0, 0.25], [0.25, 0.0], [0.999999, 0.000001]]
    lv = rng.uniform(-0.5, n_levels + 0.7, size=(N, 2)).astype(np.float32)
    lv[6:10] = [[0, 3], [n_levels, n_levels], [0.25, 0.5], [n_levels - 0.25, n_levels + 3]]
    return uv, lv


def _close(got, want, tol, what):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.0e} * {scale:.3g}"


E24 = 2.0 ** -24
N_ORDERS = 8          # point orders of the fp32 restatement's texel gradient
MIN_SAFE = 0.90       # the safe mask must keep this share of a case's points


def _rho(t, t64, s, rows=None):
    """worst |t - t64|_i / (2^-24 s_i) over the elements with s_i > 0 (rows: a mask over the leading axis)."""
    err = np.abs(np.asarray(t, np.float64) - t64)
    if rows is not None:
        err, s = err[rows], s[rows]
    pos = s > 0.0
    return float((err[pos] / (E24 * s[pos])).max(initial=0.0))


def _bar(got, t64, s, rho32, what, rows=None):
    """|T_gpu - T_64|_i <= 4 rho32 2^-24 s_i + 2^-24 |T_64|_i, s_i from the oracle's absolute companion, rho32 the worst
    |err_i| / (2^-24 s_i) of the oracle's fp32 restatement on the same case; an element with s_i = 0 must be exactly 0.
    (4: the suite's factor for a kernel whose summation order no restatement shares -- float atomics, register runs of up to
    256 pairs, explicit FMAs.)  Prints rho_gpu / rho32, the figure DESIGN_LOG.md records."""
    got = np.asarray(got, np.float64)
    if rows is not None:
        got, t64, s = got[rows], t64[rows], s[rows]
    assert got.shape == t64.shape == s.shape, (what, got.shape, t64.shape, s.shape)
    assert np.all(got[s == 0.0] == 0.0), f"{what}: non-zero where nothing was summed"
    rho_gpu = _rho(got, t64, s)
    ratio = rho_gpu / rho32 if rho32 > 0 else (np.inf if rho_gpu > 0 else 0.0)
    print(f"RHO {what}: rho32 {rho32:.3f} rho_gpu {rho_gpu:.3f} ratio {ratio:.3f}")
    err = np.abs(got - t64)
    bound = 4.0 * rho32 * E24 * s + E24 * np.abs(t64)
    bad = err > bound
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements over the bar; worst at {k}: got {got[k]!r} want {t64[k]!r} "
                             f"err {err[k]:.3e} bound {bound[k]:.3e} s {s[k]:.3e}; rho32 {rho32:.3f} rho_gpu {rho_gpu:.3f}")


def _safe(uv, bias, W, H, mm):
    """Rows where the oracle's discrete choices (floor of the texel coordinate and of the level) are the same in fp32: away
    from texel centres and integral levels by more than fp32 resolution.  Only the uv and bias gradients need it."""
    safe = np.ones(uv.shape[0], bool)
    sizes = tor.mip_sizes(W, H, mm)
    for (w, h) in sizes:
        for k, e in ((0, w), (1, h)):
            x = uv[:, k].astype(np.float64) * e - 0.5
            safe &= (np.abs(x - np.round(x)) > 1e-3) | (x < -1e-3) | (x > e - 1 + 1e-3)
    if len(sizes) > 1:                   # (a plane without a stack has no level to choose)
        safe &= np.abs(bias - np.round(bias)) > 1e-4
    return safe


class _PlaneRef:
    """One plane's inputs and everything the comparisons need, computed once on the CPU: the fp64 oracle, its absolute
    companion s, and rho32 per tensor from the fp32 restatement (N_ORDERS point orders for the texel gradient)."""

    def __init__(self, tex, uv, lv, dy, mm, seed=0, safe=None):
        self.tex, self.uv, self.lv, self.dy, self.mm = tex, uv, lv, dy, mm              # tex [C,H,W]
        C, H, W = tex.shape
        hwc = np.transpose(tex, (1, 2, 0))
        self.bias = bias = lv.min(axis=1)
        self.first = lv[:, 0] <= lv[:, 1]                                                # the bias gradient's column: cu on a tie
        self.r64 = tor.texture(hwc, uv, bias, mm, dy)
        self.s = tor.texture(hwc, uv, bias, mm, dy, absolute=True)
        self.safe = _safe(uv, bias, W, H, mm) if safe is None else safe
        rng = np.random.default_rng(seed)
        r32 = tor.texture(hwc, uv, bias, mm, dy, dtype=np.float32)
        self.r32 = r32
        self.rho = [_rho(r32[0], self.r64[0], self.s[0]), _rho(r32[1], self.r64[1], self.s[1]),
                    _rho(r32[2], self.r64[2], self.s[2], self.safe), _rho(r32[3], self.r64[3], self.s[3], self.safe)]
        for _ in range(N_ORDERS - 1):
            d = tor.texture(hwc, uv, bias, mm, dy, dtype=np.float32, order=rng.permutation(uv.shape[0]))[1]
            self.rho[1] = max(self.rho[1], _rho(d, self.r64[1], self.s[1]))

    def check(self, got, what, old_bars=True):
        """got = (features, dtex [C,H,W], d_uv [N,2], d_lv [N,2]) from the GPU."""
        o, gtex, dp, dl = got
        out, dtex, duv, dbias = self.r64
        dtex_g = np.transpose(gtex, (1, 2, 0))
        got_bias = np.where(self.first, dl[:, 0], dl[:, 1])
        other = np.where(self.first, dl[:, 1], dl[:, 0])
        safe = self.safe
        assert safe.mean() >= MIN_SAFE, f"{what}: the safe mask keeps {safe.mean():.3f} of the points"
        if old_bars:
            _close(o, out, 1e-5, "features")
            _close(dtex_g, dtex, 1e-5, "dL/dtex")
            _close(dp[safe], duv[safe], 2e-5, "dL/duv")
            _close(got_bias[safe], dbias[safe], 2e-5, "dL/dbias")
        assert np.all(other == 0.0)
        _bar(o, out, self.s[0], self.rho[0], what + " features")
        _bar(dtex_g, dtex, self.s[1], self.rho[1], what + " dtex")
        _bar(dp, duv, self.s[2], self.rho[2], what + " duv", safe)
        _bar(got_bias, dbias, self.s[3], self.rho[3], what + " dbias", safe)


def _run_plane(gpu, ref, scatter, dy=None):
    """forward + backward of one plane through fused_hexplane.texture_planes; numpy (features, dtex [C,H,W], d_uv, d_lv)."""
    import fused_hexplane
    from diff_gaussian_rasterization_ch3 import _C
    assert _C.lib().gsrast_set_option(b"hexplane_scatter", int(scatter)) == 0
    try:
        g = torch.tensor(ref.tex[None], device=gpu, requires_grad=True)
        p = torch.tensor(ref.uv, device=gpu, requires_grad=True)
        l = torch.tensor(ref.lv, device=gpu, requires_grad=True)
        o = fused_hexplane.texture_planes(p, l, [g], [(0, 1)], [ref.mm], [0], ref.tex.shape[0])
        o.backward(torch.tensor(ref.dy, device=gpu) if dy is None else dy)
        torch.cuda.synchronize()
    finally:
        _C.lib().gsrast_set_option(b"hexplane_scatter", 0)
    return o.detach().cpu().numpy(), g.grad[0].cpu().numpy(), p.grad.cpu().numpy(), l.grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _first_day_ref(W, H, C, mm, N, seed):
    """The cases of test_single_plane_against_oracle (shared by its two scatter forms)."""
    rng = np.random.default_rng(seed)
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    tex = rng.normal(size=(C, H, W)).astype(np.float32)
    uv, lv = _points(rng, N, n_levels)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    return _PlaneRef(tex, uv, lv, dy, mm, seed)


def _plane_case(gpu, W, H, C, mm, N, seed, scatter, new_bars=True):
    """The first day's comparison (1e-5 / 2e-5 of the tensor's largest entry; the uv / bias gradients where the oracle's
    discrete choices are the same in fp32, the bias gradient's other column exactly 0), and beside it the per-element bars."""
    if new_bars:
        ref = _first_day_ref(W, H, C, mm, N, seed)
        ref.check(_run_plane(gpu, ref, scatter), f"{W}x{H} C{C} mm{mm} N{N} scatter{scatter}")
        return
    rng = np.random.default_rng(seed)
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    tex = rng.normal(size=(C, H, W)).astype(np.float32)
    uv, lv = _points(rng, N, n_levels)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    bias = lv.min(axis=1)
    out, dtex, duv, dbias = tor.texture(np.transpose(tex, (1, 2, 0)), uv, bias, mm, dy)
    ref = types.SimpleNamespace(tex=tex, uv=uv, lv=lv, dy=dy, mm=mm)
    o, gtex, dp, dl = _run_plane(gpu, ref, scatter)
    _close(o, out, 1e-5, "features")
    _close(np.transpose(gtex, (1, 2, 0)), dtex, 1e-5, "dL/dtex")
    safe = _safe(uv, bias, W, H, mm)
    _close(dp[safe], duv[safe], 2e-5, "dL/duv")
    first = lv[:, 0] <= lv[:, 1]
    _close(np.where(first, dl[:, 0], dl[:, 1])[safe], dbias[safe], 2e-5, "dL/dbias")
    assert np.all(np.where(first, dl[:, 1], dl[:, 0]) == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,C,mm", [(64, 64, 32, 7), (32, 8, 16, 7), (16, 25, 32, 0), (8, 2, 4, 7), (128, 128, 8, 7), (64, 128, 64, 0),
                                      (256, 256, 32, 7), (1, 1, 4, 7)])
@pytest.mark.parametrize("scatter", [0, 1])
def test_single_plane_against_oracle(gpu, W, H, C, mm, scatter):
    """scatter 0 = sorted runs (default), 1 = direct global atomics."""
    _plane_case(gpu, W, H, C, mm, 3001, W * 7 + H + C + mm, scatter)


@pytest.mark.gpu
def test_large_plane(gpu):
    _plane_case(gpu, 512, 512, 32, 7, 20000, 5, 0, new_bars=False)      # (first day's bars only: eight fp32 restatements of 20 000 points on 512 x 512 x 32 are not quick)
    _plane_case(gpu, 512, 512, 32, 7, 20000, 6, 1, new_bars=False)


def _field(rng, reso, C, mults):
    return [[rng.normal(size=(1, C, (reso[b] * m if b < 3 else reso[b]), (reso[a] * m if a < 3 else reso[a]))).astype(np.float32)
             for (a, b) in tor.PLANES] for m in mults]


@pytest.mark.gpu
@pytest.mark.parametrize("reso,C,mults", [([64, 64, 64, 25], 32, (1,)), ([16, 16, 16, 10], 16, (1, 2, 4)), ([64, 64, 64, 128], 32, (1, 2))])
def test_field_against_oracle(gpu, reso, C, mults):
    """interpolate_ms_features (hexplane.py:95-139): 6 planes x scales in one launch, and dL/dgrid of every plane."""
    import fused_hexplane
    rng = np.random.default_rng(len(mults) * 100 + C)
    grids = _field(rng, reso, C, mults)
    N = 5000
    pts = rng.uniform(0, 1, size=(N, 4)).astype(np.float32)
    levels = np.concatenate([rng.uniform(0, np.log2(reso[0]), size=(N, 3)), np.zeros((N, 1))], axis=1).astype(np.float32)   # get_level :237-249
    dy = rng.normal(size=(N, C * len(mults))).astype(np.float32)
    want, dg, _, _ = tor.interpolate_ms_features(pts, [[g[0] for g in gs] for gs in grids], levels, dy)
    params = [[torch.tensor(g, device=gpu, requires_grad=True) for g in gs] for gs in grids]
    out = fused_hexplane.interpolate_ms_features(torch.tensor(pts, device=gpu), params, 2, True, torch.tensor(levels, device=gpu), None)
    assert tuple(out.shape) == (N, C * len(mults))
    out.backward(torch.tensor(dy, device=gpu))
    _close(out.detach().cpu().numpy(), want, 1e-5, "features")
    for s, gs in enumerate(params):
        for ci, g in enumerate(gs):
            _close(g.grad[0].cpu().numpy(), dg[s][ci], 1e-5, f"dL/dgrid scale {s} plane {ci}")


@pytest.mark.gpu
def test_reference_call_shapes_and_layouts(gpu):
    """grid_sample_wrapper mirror (hexplane.py:26-60); channels_last parameters are used in place and receive their gradient;
    summed scales / concat_planes variants of interpolate_ms_features."""
    import fused_hexplane
    rng = np.random.default_rng(11)
    C, N = 8, 700
    tex = rng.normal(size=(1, C, 32, 16)).astype(np.float32)
    uv = rng.uniform(0, 1, size=(N, 2)).astype(np.float32)
    lv = rng.uniform(0, 4, size=(N, 2)).astype(np.float32)
    want = tor.texture(np.transpose(tex[0], (1, 2, 0)), uv, lv.min(1), 7)
    g = torch.tensor(tex, device=gpu).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    o = fused_hexplane.grid_sample_wrapper(g, torch.tensor(uv, device=gpu), torch.tensor(lv, device=gpu), True)
    assert tuple(o.shape) == (N, C)
    _close(o.detach().cpu().numpy(), want, 1e-5, "wrapper")
    o.sum().backward()
    assert g.grad.shape == g.shape
    _, dtex, _, _ = tor.texture(np.transpose(tex[0], (1, 2, 0)), uv, lv.min(1), 7, np.ones((N, C)))
    _close(g.grad[0].cpu().numpy(), np.transpose(dtex, (2, 0, 1)), 1e-5, "channels_last grad")
    o0 = fused_hexplane.grid_sample_wrapper(g, torch.tensor(uv, device=gpu), torch.tensor(lv, device=gpu), False)
    _close(o0.detach().cpu().numpy(), tor.texture(np.transpose(tex[0], (1, 2, 0)), uv, lv.min(1), 0), 1e-5, "time-plane wrapper")
    # summed scales (concat_features=False) and space|time blocks (concat_planes=True)
    grids = _field(rng, [8, 8, 8, 6], 4, (1, 2))
    pts = rng.uniform(0, 1, size=(N, 4)).astype(np.float32)
    levels = np.concatenate([rng.uniform(0, 3, size=(N, 3)), np.zeros((N, 1))], axis=1).astype(np.float32)
    params = [[torch.tensor(x, device=gpu) for x in gs] for gs in grids]
    per = [[tor.texture(np.transpose(gs[ci][0], (1, 2, 0)), pts[:, list(c)], levels[:, list(c)].min(1), 7 if 3 not in c else 0)
            for ci, c in enumerate(tor.PLANES)] for gs in grids]
    tp, tl = torch.tensor(pts, device=gpu), torch.tensor(levels, device=gpu)
    summed = fused_hexplane.interpolate_ms_features(tp, params, 2, False, tl, None)
    _close(summed.cpu().numpy(), sum(sum(p) for p in per), 1e-5, "summed scales")
    blocks = fused_hexplane.interpolate_ms_features(tp, params, 2, True, tl, None, concat_planes=True)
    want_b = np.concatenate([np.concatenate([p[0] + p[1] + p[3], p[2] + p[4] + p[5]], axis=1) for p in per], axis=1)
    _close(blocks.cpu().numpy(), want_b, 1e-5, "concat_planes")
    one = fused_hexplane.interpolate_ms_features(tp, params, 2, True, tl, 1)
    _close(one.cpu().numpy(), sum(per[0]), 1e-5, "num_levels=1")


@pytest.mark.gpu
def test_errors_and_empty(gpu):
    import fused_hexplane
    g = torch.zeros((1, 4, 10, 12), device=gpu)
    uv = torch.rand((5, 2), device=gpu)
    with pytest.raises(RuntimeError, match="odd extent"):
        fused_hexplane.texture_planes(uv, uv, [g], [(0, 1)], [7], [0], 4)       # 6x5 cannot be halved
    fused_hexplane.texture_planes(uv, uv, [g], [(0, 1)], [1], [0], 4)            # one level is fine
    with pytest.raises(RuntimeError, match="power of two"):
        fused_hexplane.texture_planes(uv, uv, [torch.zeros((1, 12, 8, 8), device=gpu)], [(0, 1)], [0], [0], 12)
    with pytest.raises(RuntimeError, match="GPU"):
        fused_hexplane.texture_planes(uv.cpu(), uv.cpu(), [g.cpu()], [(0, 1)], [0], [0], 4)
    e = torch.zeros((0, 2), device=gpu)
    gg = torch.ones((1, 4, 8, 8), device=gpu, requires_grad=True)
    o = fused_hexplane.texture_planes(e, e, [gg], [(0, 1)], [7], [0], 4)
    assert tuple(o.shape) == (0, 4)
    o.sum().backward()
    assert float(gg.grad.abs().max()) == 0.0
    # non-finite coordinates stay inside the plane (clamped), no fault
    bad = torch.tensor([[float("nan"), float("inf")], [-float("inf"), 0.5]], device=gpu)
    o = fused_hexplane.texture_planes(bad, torch.zeros_like(bad), [gg], [(0, 1)], [7], [0], 4)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all()


# ---- every kernel branch: thin and non-power-of-two stacks, row counts, the shipped 24-plane field ---------------------
# Coverage, by kernel (csrc/gsrast_hexplane.h):
#   hex_mip_build / hex_mip_pull   quad, horizontal-only (16 x 1, 8 x 2) and VERTICAL-only halving (2 x 8, 1 x 16), with points on the
#                                  top two levels; even extents with an odd top (24 x 40 -> 3 x 5, 20 x 4, 12 x 10, 6 x 2)
#   hex_sample_fwd                 1 .. 24 planes, blocks concatenated / summed / space | time, a block after a gap (zeros between)
#   hex_keys / hex_grad_tex_sorted runs that end inside, at and after the 256-pair chunk border (N = 255 / 256 / 257 / 513; six planes
#                                  at N = 42 / 43 / 85 / 86), one key over many chunks (2000 points in one cell, 600 copies of one point),
#                                  every position of a pair's 2 x 2 inside the run's 4 x 4 window, dy rows of zeros
#   hex_grad_tex_global            the same cases (hexplane_scatter = 1)
#   hex_grad_uv                    several planes per column (dp / dl accumulate), the bias gradient's column (smaller level, cu on a
#                                  tie), d_pts without d_levels and the reverse, N = 1 at C = 64 (a whole wave shadows one point),
#                                  mips_built = 0
# Two branches stay uncovered, on purpose:
#   * code = 32, "outside the 4 x 4 window" (hex_keys_kernel, and the direct-atomics net of the sorted kernel): unreachable.  With
#     wa = 2 wb, x0 = 2 x1 + 0.5 before the clamps, so floor(x0) - 2 floor(x1) is 0, 1 or 2, the clamps keep it there, and it is 0
#     when both extents are 1.
#   * the key_bits > 32 fallback to global atomics: needs more than 2^26 texels in a plane, which hex_check refuses.
def _points2(rng, N, n_levels, tie=0.1):
    """Like _points, at any N, with the bias (the smaller level) uniform over [-0.5, n_levels + 0.7] so the top two levels get their
    share, either column the smaller one, and ties (the bias gradient then belongs to column 0)."""
    uv = rng.uniform(-0.05, 1.05, size=(N, 2)).astype(np.float32)
    bias = rng.uniform(-0.5, n_levels + 0.7, size=N)
    other = bias + rng.uniform(0.0, 1.5, size=N)
    lv = np.where((rng.random(N) < 0.5)[:, None], np.stack([bias, other], 1), np.stack([other, bias], 1)).astype(np.float32)
    t = rng.random(N) < tie
    lv[t, 1] = lv[t, 0]
    if N >= 200:
        uv[:6] = [[0, 0], [1, 1], [0.5, 0.5], [1.0, 0.25], [0.25, 0.0], [0.999999, 0.000001]]
        lv[6:10] = [[0, 3], [n_levels, n_levels], [0.25, 0.5], [n_levels - 0.25, n_levels + 3]]
    return uv, lv


def _generic_ref(W, H, C, mm, N, seed, top_two=True):
    rng = np.random.default_rng(seed)
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    tex = rng.normal(size=(C, H, W)).astype(np.float32)
    uv, lv = _points2(rng, N, n_levels)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    ref = _PlaneRef(tex, uv, lv, dy, mm, seed)
    if top_two and n_levels >= 1 and N >= 64:
        b = ref.bias
        assert np.sum((b > n_levels - 1) & (b < n_levels)) >= 5 and np.sum(b >= n_levels) >= 5 and np.sum((lv[:, 0] == lv[:, 1]) & (b > 0) & (b < n_levels)) >= 3
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,C,mm,N", [(2, 8, 4, 7, 400), (1, 16, 4, 7, 400), (16, 1, 8, 7, 400),                     # vertical-only / horizontal-only halving
                                        (24, 40, 8, 3, 600), (20, 4, 4, 2, 400), (12, 10, 4, 1, 400), (6, 2, 4, 1, 400),   # even extents, odd top
                                        (2, 2, 64, 7, 1)])
def test_thin_and_odd_topped_stacks(gpu, W, H, C, mm, N):
    """Vertical halving (pw == 1, ph > 1) of the mip build and of the pull-down, and stacks over extents that are even but no powers
    of two, with points on the top two levels; N = 1 at C = 64."""
    ref = _generic_ref(W, H, C, mm, N, 1000 * W + 10 * H + C + mm)
    for scatter in (0, 1):
        ref.check(_run_plane(gpu, ref, scatter), f"{W}x{H} C{C} mm{mm} N{N} scatter{scatter}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("C", [4, 64])
def test_row_counts(gpu, C, N):
    """One 16 x 16 plane: rows around the wave, the 256-thread block and the 256-pair chunk of the sorted walk (E = N here)."""
    ref = _generic_ref(16, 16, C, 7, N, 77 * C + N)
    for scatter in (0, 1):
        ref.check(_run_plane(gpu, ref, scatter), f"16x16 C{C} N{N} scatter{scatter}")


@pytest.mark.gpu
def test_concentrated_points(gpu):
    """What the sorted-run kernel was written for: thousands of pairs under one key, over many 256-pair chunks.  64 x 64, C = 32:
    2000 points inside one texel cell of level 3 with levels in [2, 3), then 600 exact copies of one point."""
    rng = np.random.default_rng(64)
    tex = rng.normal(size=(32, 64, 64)).astype(np.float32)
    N = 2000
    uv = (np.array([2.55, 5.55]) / 8.0 + rng.uniform(0.0, 0.9, size=(N, 2)) / 8.0).astype(np.float32)       # level 3 (8 x 8): x in (2.05, 2.95), y in (5.05, 5.95)
    x3 = uv.astype(np.float64) * 8 - 0.5
    assert np.all(np.floor(x3) == [2, 5])
    lv = np.stack([rng.uniform(2.0, 3.0, size=N), rng.uniform(2.0, 5.0, size=N)], 1).astype(np.float32)
    lv[:, 0] = np.minimum(lv[:, 0], np.float32(2.999))
    dy = rng.normal(size=(N, 32)).astype(np.float32)
    ref = _PlaneRef(tex, uv, lv, dy, 7, 1)
    assert np.all((ref.bias >= 2) & (ref.bias < 3))
    for scatter in (0, 1):
        ref.check(_run_plane(gpu, ref, scatter), f"one cell scatter{scatter}")
    uv1 = np.tile(np.array([[0.3371, 0.7127]], np.float32), (600, 1))
    lv1 = np.tile(np.array([[1.375, 4.0]], np.float32), (600, 1))
    ref = _PlaneRef(tex, uv1, lv1, rng.normal(size=(600, 32)).astype(np.float32), 7, 2)
    for scatter in (0, 1):
        ref.check(_run_plane(gpu, ref, scatter), f"600 copies scatter{scatter}")


@pytest.mark.gpu
def test_upstream_gradient_forms(gpu):
    """dy with half of its rows exactly zero (the global-atomics kernel skips them lane by lane), all zero (exact-zero gradients), and
    handed over non-contiguous."""
    rng = np.random.default_rng(12)
    W, H, C, mm, N = 32, 16, 8, 7, 700
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    tex = rng.normal(size=(C, H, W)).astype(np.float32)
    uv, lv = _points2(rng, N, n_levels)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    dy[rng.random(N) < 0.5] = 0.0
    half = _PlaneRef(tex, uv, lv, dy, mm, 3)
    full = _PlaneRef(tex, uv, lv, rng.normal(size=(N, C)).astype(np.float32), mm, 4)
    for scatter in (0, 1):
        half.check(_run_plane(gpu, half, scatter), f"half-zero dy scatter{scatter}")
        o, gtex, dp, dl = _run_plane(gpu, half, scatter, dy=torch.zeros((N, C), device=gpu))
        assert not gtex.any() and not dp.any() and not dl.any()
        wide = torch.zeros((C, 2 * N), device=gpu)
        wide[:, ::2] = torch.tensor(full.dy, device=gpu).t()
        view = wide[:, ::2].t()                       # [N, C] with strides (2, 2 N)
        assert not view.is_contiguous()
        full.check(_run_plane(gpu, full, scatter, dy=view), f"strided dy scatter{scatter}")


# ---- exact cases: no tolerance ------------------------------------------------------------------------------------------
def _exact_ref(W, H, C, N, seed, top=None):
    """Inputs on which every intermediate of the op is a dyadic rational that fp32 holds exactly: power-of-two extents, texels and dy
    small integers, uv = (k + 1/2 + j/8) / W (texel coordinate k + j/8 at level 0: texel centres included), level fractions in
    {0, 1/4, 1/2} (integral levels included).  Asserted: the fp32 and the fp64 restatement agree bit for bit, under two point
    orders -- so any order of exact operations gives the same bits, and the GPU must give them too."""
    rng = np.random.default_rng(seed)
    n_levels = len(tor.mip_sizes(W, H, 7)) - 1
    tex = rng.integers(-2, 3, size=(C, H, W)).astype(np.float32)
    uv = np.stack([(rng.integers(0, W, N) + 0.5 + rng.integers(0, 8, N) / 8.0) / W, (rng.integers(0, H, N) + 0.5 + rng.integers(0, 8, N) / 8.0) / H], 1)
    assert np.array_equal(uv.astype(np.float32).astype(np.float64), uv)
    uv = uv.astype(np.float32)
    bias = rng.integers(0, (n_levels if top is None else top) + 1, N) + rng.choice([0.0, 0.25, 0.5], N)      # (top: the finest levels only, where a deep stack's weights still fit 24 bits)
    other = bias + rng.choice([0.0, 0.25, 1.0], N)
    lv = np.where((rng.random(N) < 0.5)[:, None], np.stack([bias, other], 1), np.stack([other, bias], 1)).astype(np.float32)
    dy = rng.integers(-2, 3, size=(N, C)).astype(np.float32)
    hwc = np.transpose(tex, (1, 2, 0))
    r64 = tor.texture(hwc, uv, lv.min(1), 7, dy)
    for order in (None, rng.permutation(N)):
        r32 = tor.texture(hwc, uv, lv.min(1), 7, dy, dtype=np.float32, order=order)
        for a, b, name in zip(r32, r64, ("features", "dtex", "duv", "dbias")):
            assert np.array_equal(a.astype(np.float64), b), f"exact case {W}x{H}: the fp32 restatement rounds in {name}"
    ref = types.SimpleNamespace(tex=tex, uv=uv, lv=lv, dy=dy, mm=7, r64=r64, first=lv[:, 0] <= lv[:, 1])
    return ref


def _check_exact(ref, got, what):
    o, gtex, dp, dl = got
    out, dtex, duv, dbias = ref.r64
    assert np.array_equal(o.astype(np.float64), out), what + " features"
    assert np.array_equal(np.transpose(gtex, (1, 2, 0)).astype(np.float64), dtex), what + " dtex"
    assert np.array_equal(dp.astype(np.float64), duv), what + " duv"
    assert np.array_equal(np.where(ref.first, dl[:, 0], dl[:, 1]).astype(np.float64), dbias), what + " dbias"
    assert np.all(np.where(ref.first, dl[:, 1], dl[:, 0]) == 0.0), what


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,C", [(2, 8, 4), (1, 16, 4), (16, 1, 4), (8, 2, 4), (16, 16, 4), (64, 64, 32)])
def test_exact_single_plane(gpu, W, H, C):
    """Bit for bit against fp64, on texel centres and integral levels too, where no mask and no tolerance is needed."""
    ref = _exact_ref(W, H, C, 300, W * 100 + H, top=2 if W == 64 else None)      # (64 x 64: levels 0 .. 3; below, the weights need more than 24 bits)
    for scatter in (0, 1):
        _check_exact(ref, _run_plane(gpu, ref, scatter), f"{W}x{H} scatter{scatter}")


# ---- the field: six planes per scale, up to the shipped four scales ---------------------------------------------------
class _FieldRef:
    """interpolate_ms_features on one set of inputs: fp64 oracle, absolute companion, rho32 per tensor (features, every grid,
    d_pts, d_levels), the rows that are safe for every plane.  grids[scale][plane] = [1, C, H, W] fp32."""

    def __init__(self, grids, pts, levels, dy, concat_features=True, concat_planes=False, seed=0, n_orders=N_ORDERS, rho=True):
        self.grids, self.pts, self.levels, self.dy, self.cf, self.cp = grids, pts, levels, dy, concat_features, concat_planes
        g3 = [[g[0] for g in gs] for gs in grids]
        kw = dict(concat_features=concat_features, concat_planes=concat_planes)
        self.r64 = tor.interpolate_ms_features(pts, g3, levels, dy, **kw)
        safe = np.ones(pts.shape[0], bool)
        for gs in g3:
            for ci, (cu, cv) in enumerate(tor.PLANES):
                safe &= _safe(pts[:, [cu, cv]], np.minimum(levels[:, cu], levels[:, cv]), gs[ci].shape[2], gs[ci].shape[1], 7 if 3 not in (cu, cv) else 0)
        self.safe = safe
        if not rho:
            return
        self.s = tor.interpolate_ms_features(pts, g3, levels, dy, absolute=True, **kw)
        rng = np.random.default_rng(seed)
        self.rho_f = self.rho_p = self.rho_l = 0.0
        self.rho_g = [[0.0] * 6 for _ in grids]
        for k in range(n_orders):
            r32 = tor.interpolate_ms_features(pts, g3, levels, dy, dtype=np.float32, order=rng.permutation(pts.shape[0]) if k else None, **kw)
            if k == 0:
                self.rho_f = _rho(r32[0], self.r64[0], self.s[0])
                self.rho_p = _rho(r32[2], self.r64[2], self.s[2], safe)
                self.rho_l = _rho(r32[3], self.r64[3], self.s[3], safe)
            for si in range(len(grids)):
                for ci in range(6):
                    self.rho_g[si][ci] = max(self.rho_g[si][ci], _rho(r32[1][si][ci], self.r64[1][si][ci], self.s[1][si][ci]))

    def check(self, got, what):
        out, grads, dp, dl = got
        f, dg, d_pts, d_levels = self.r64
        assert out.shape == f.shape
        assert self.safe.mean() >= MIN_SAFE, f"{what}: the safe mask keeps {self.safe.mean():.3f} of the points"
        _close(out, f, 1e-5, "features")
        _bar(out, f, self.s[0], self.rho_f, what + " features")
        for si, gs in enumerate(grads):
            for ci, g in enumerate(gs):
                _close(g, dg[si][ci], 1e-5, f"dL/dgrid scale {si} plane {ci}")
                _bar(g, dg[si][ci], self.s[1][si][ci], self.rho_g[si][ci], what + f" dgrid[{si}][{ci}]")
        if dp is not None:
            _close(dp[self.safe], d_pts[self.safe], 2e-5, "d_pts")
            _bar(dp, d_pts, self.s[2], self.rho_p, what + " d_pts", self.safe)
        if dl is not None:
            _close(dl[self.safe], d_levels[self.safe], 2e-5, "d_levels")
            _bar(dl, d_levels, self.s[3], self.rho_l, what + " d_levels", self.safe)
            assert np.all(dl[:, 3] == 0.0)                                  # the time planes have no mip stack: no bias gradient from them


def _run_field(gpu, ref, scatter, grad_pts=True, grad_levels=True):
    import fused_hexplane
    from diff_gaussian_rasterization_ch3 import _C
    assert _C.lib().gsrast_set_option(b"hexplane_scatter", int(scatter)) == 0
    try:
        params = [[torch.tensor(g, device=gpu, requires_grad=True) for g in gs] for gs in ref.grids]
        tp = torch.tensor(ref.pts, device=gpu, requires_grad=grad_pts)
        tl = torch.tensor(ref.levels, device=gpu, requires_grad=grad_levels)
        out = fused_hexplane.interpolate_ms_features(tp, params, 2, ref.cf, tl, None, concat_planes=ref.cp)
        out.backward(torch.tensor(ref.dy, device=gpu))
        torch.cuda.synchronize()
    finally:
        _C.lib().gsrast_set_option(b"hexplane_scatter", 0)
    return (out.detach().cpu().numpy(), [[g.grad[0].cpu().numpy() for g in gs] for gs in params],
            None if tp.grad is None else tp.grad.cpu().numpy(), None if tl.grad is None else tl.grad.cpu().numpy())


N_TIES = 40


def _field_inputs(rng, N, top):
    """pts a little beyond [0, 1]; spatial levels over [-0.3, top + 0.5] (the top levels of the finest scale get points); the time
    level 0 in half of the rows (what get_level gives) and above the spatial ones in others; the first N_TIES rows have
    levels[0] == levels[1] > levels[2], all strictly inside (0, 3): plane (0, 1)'s bias gradient belongs to column 0, and column 1,
    the larger one in plane (1, 2) as well, gets exactly 0."""
    pts = rng.uniform(-0.02, 1.02, size=(N, 4)).astype(np.float32)
    lv = rng.uniform(-0.3, top + 0.5, size=(N, 4))
    lv[:, 3] = np.where(rng.random(N) < 0.5, 0.0, rng.uniform(0.0, top + 1.0, size=N))
    n = min(N_TIES, N // 2)
    lv[:n, 0] = lv[:n, 1] = rng.uniform(1.2, 2.8, size=n)
    lv[:n, 2] = rng.uniform(0.1, 1.1, size=n)
    return pts, lv.astype(np.float32), n


def _check_ties(ref, dl, n):
    lv = ref.levels
    assert n > 0 and np.all((lv[:n, 0] == lv[:n, 1]) & (lv[:n, 2] < lv[:n, 1]) & (lv[:n, 2] > 0))
    assert np.all(dl[:n, 1] == 0.0) and np.all(ref.r64[3][:n, 1] == 0.0)
    assert np.count_nonzero(dl[:n, 0]) >= n // 2 and np.count_nonzero(dl[:n, 2]) >= n // 2


@pytest.mark.gpu
@pytest.mark.parametrize("reso,C", [([8, 8, 8, 5], 32), ([16, 16, 16, 6], 8)])
def test_shipped_four_scale_field(gpu, reso, C):
    """The reference's configuration (arguments/__init__.py:83-89, hexplane.py:168): 24 planes, multires (1, 2, 4, 8), F = 4 C,
    concatenated -- the launch HEX_MAX_PLANES was sized for, refused by gsrast_hexplane_scratch_bytes until now.  Features, all 24
    grid gradients, d_pts and d_levels against the oracle."""
    rng = np.random.default_rng(reso[0] + C)
    grids = _field(rng, reso, C, (1, 2, 4, 8))
    N = 1500
    pts, levels, n = _field_inputs(rng, N, np.log2(reso[0] * 8))
    dy = rng.normal(size=(N, 4 * C)).astype(np.float32)
    ref = _FieldRef(grids, pts, levels, dy, seed=C)
    for scatter in (0, 1):
        got = _run_field(gpu, ref, scatter)
        assert got[0].shape == (N, 4 * C)
        ref.check(got, f"24 planes reso {reso[0]} C{C} scatter{scatter}")
        _check_ties(ref, got[3], n)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [42, 43, 85, 86])
def test_field_row_counts(gpu, N):
    """Six planes: E = 6 N crosses the 256-pair chunk of the sorted walk between 42 and 43, and 512 between 85 and 86."""
    rng = np.random.default_rng(N)
    grids = _field(rng, [8, 8, 8, 4], 4, (1,))
    pts, levels, n = _field_inputs(rng, N, 3)
    ref = _FieldRef(grids, pts, levels, rng.normal(size=(N, 4)).astype(np.float32), seed=N)
    for scatter in (0, 1):
        got = _run_field(gpu, ref, scatter)
        ref.check(got, f"6 planes N{N} scatter{scatter}")
        _check_ties(ref, got[3], n)


@pytest.mark.gpu
@pytest.mark.parametrize("concat_features,concat_planes", [(False, False), (True, True), (False, True)])
def test_layout_gradients(gpu, concat_features, concat_planes):
    """Backward of the summed-scales and of the space | time block layouts (the forward alone was tested)."""
    rng = np.random.default_rng(5 + 2 * concat_features + concat_planes)
    C, N = 4, 700
    grids = _field(rng, [8, 8, 8, 6], C, (1, 2))
    pts, levels, n = _field_inputs(rng, N, 4)
    F, _ = tor.field_layout(2, C, concat_features, concat_planes)
    ref = _FieldRef(grids, pts, levels, rng.normal(size=(N, F)).astype(np.float32), concat_features, concat_planes, seed=1)
    for scatter in (0, 1):
        got = _run_field(gpu, ref, scatter)
        ref.check(got, f"concat_features={concat_features} concat_planes={concat_planes} scatter{scatter}")
        _check_ties(ref, got[3], n)


@pytest.mark.gpu
def test_requires_grad_combinations(gpu):
    """d_pts without d_levels, the reverse, both, neither: a gradient that is returned equals the both-on run bit for bit (the uv
    kernel has one writer per row, no atomics), one that is not asked for is None."""
    rng = np.random.default_rng(21)
    grids = _field(rng, [8, 8, 8, 4], 8, (1, 2))
    pts, levels, n = _field_inputs(rng, 300, 4)
    ref = _FieldRef(grids, pts, levels, rng.normal(size=(300, 16)).astype(np.float32), rho=False)
    both = _run_field(gpu, ref, 0, True, True)
    assert both[2] is not None and both[3] is not None and both[2].any() and both[3].any()
    _close(both[2][ref.safe], ref.r64[2][ref.safe], 2e-5, "d_pts")
    _close(both[3][ref.safe], ref.r64[3][ref.safe], 2e-5, "d_levels")
    for gp, gl in ((True, False), (False, True), (False, False)):
        got = _run_field(gpu, ref, 0, gp, gl)
        assert np.array_equal(got[0], both[0])
        assert (got[2] is None) == (not gp) and (got[3] is None) == (not gl)
        if gp:
            assert np.array_equal(got[2].view(np.uint32), both[2].view(np.uint32))
        if gl:
            assert np.array_equal(got[3].view(np.uint32), both[3].view(np.uint32))
        _close(got[1][1][3], ref.r64[1][1][3], 1e-5, "a grid gradient, whatever else is asked for")


def _exact_field_ref(seed, N=200):
    """The exact case of the field: reso [8, 8, 8, 4], mults (1, 2) -- coordinates on the 1/8 sub-grid of the finer scale's texels."""
    rng = np.random.default_rng(seed)
    reso, C = [8, 8, 8, 4], 4
    grids = [[rng.integers(-2, 3, size=(1, C, (reso[b] * m if b < 3 else reso[b]), (reso[a] * m if a < 3 else reso[a]))).astype(np.float32)
              for (a, b) in tor.PLANES] for m in (1, 2)]
    pts = np.concatenate([(rng.integers(0, 16, size=(N, 3)) + 0.5 + rng.integers(0, 8, size=(N, 3)) / 8.0) / 16.0,
                          (rng.integers(0, 4, size=(N, 1)) + 0.5 + rng.integers(0, 8, size=(N, 1)) / 8.0) / 4.0], axis=1)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    levels = np.concatenate([rng.integers(0, 3, size=(N, 3)) + rng.choice([0.0, 0.25, 0.5], size=(N, 3)), rng.choice([0.0, 1.25], size=(N, 1))], axis=1)
    levels[:20, 1] = levels[:20, 0]
    dy = rng.integers(-2, 3, size=(N, 2 * C)).astype(np.float32)
    pts, levels = pts.astype(np.float32), levels.astype(np.float32)
    ref = _FieldRef(grids, pts, levels, dy, rho=False)
    g3 = [[g[0] for g in gs] for gs in grids]
    for order in (None, rng.permutation(N)):
        r32 = tor.interpolate_ms_features(pts, g3, levels, dy, dtype=np.float32, order=order)
        same = [np.array_equal(r32[0].astype(np.float64), ref.r64[0]), np.array_equal(r32[2].astype(np.float64), ref.r64[2]),
                np.array_equal(r32[3].astype(np.float64), ref.r64[3])] + [np.array_equal(a.astype(np.float64), b) for x, y in zip(r32[1], ref.r64[1]) for a, b in zip(x, y)]
        assert all(same), f"exact field: the fp32 restatement rounds ({same})"
    return ref


@pytest.mark.gpu
def test_exact_field(gpu):
    """Six planes x two scales, bit for bit: features, all twelve grid gradients, d_pts and d_levels (ties and integral levels included)."""
    ref = _exact_field_ref(8)
    f, dg, d_pts, d_levels = ref.r64
    for scatter in (0, 1):
        out, grads, dp, dl = _run_field(gpu, ref, scatter)
        assert np.array_equal(out.astype(np.float64), f), "features"
        for si in range(2):
            for ci in range(6):
                assert np.array_equal(grads[si][ci].astype(np.float64), dg[si][ci]), (si, ci)
        assert np.array_equal(dp.astype(np.float64), d_pts), "d_pts"
        assert np.array_equal(dl.astype(np.float64), d_levels), "d_levels"


# ---- the C ABI itself: mips_built = 0, and nothing written past scratch_bytes ------------------------------------------
def _capi_call(gpu, texs, cols, mms, offs, F, pts, lv, dy, forward=True, mips_built=1, want_uv=True):
    """gsrast_hexplane_forward / _backward through ctypes on a scratch buffer of exactly scratch_bytes bytes, 0xFF-filled, with a
    4 KB patterned guard behind it.  texs: [H, W, C] GPU tensors.  Returns (features | None, grads, d_pts, d_levels, guard intact)."""
    from diff_gaussian_rasterization_ch3 import _C
    L = _C.lib()
    N, D = pts.shape
    Cn = texs[0].shape[2]
    grads = [torch.full_like(t, float("nan")) for t in texs]
    arr = (_C.PlaneStruct * len(texs))()
    for i, t in enumerate(texs):
        arr[i] = _C.PlaneStruct(t.data_ptr(), grads[i].data_ptr(), t.shape[1], t.shape[0], cols[i][0], cols[i][1], mms[i], offs[i])
    nbytes = L.gsrast_hexplane_scratch_bytes(len(texs), arr, Cn, N)
    assert nbytes > 0, L.gsrast_last_error()
    buf = torch.full((nbytes + 4096,), 0xFF, dtype=torch.uint8, device=gpu)
    pattern = (torch.arange(4096, device=gpu) * 7 % 251).to(torch.uint8)
    buf[nbytes:] = pattern
    stream = torch.cuda.current_stream(gpu).cuda_stream
    out = None
    with torch.cuda.device(gpu):
        if forward:
            out = torch.full((N, F), float("nan"), device=gpu)
            assert L.gsrast_hexplane_forward(N, D, Cn, F, len(texs), arr, pts.data_ptr(), lv.data_ptr(), out.data_ptr(), buf.data_ptr(), stream) == 0, L.gsrast_last_error()
        d_pts, d_lv = (torch.full_like(pts, float("nan")), torch.full_like(lv, float("nan"))) if want_uv else (None, None)
        rc = L.gsrast_hexplane_backward(N, D, Cn, F, len(texs), arr, pts.data_ptr(), lv.data_ptr(), dy.data_ptr(), d_pts.data_ptr() if want_uv else None,
                                        d_lv.data_ptr() if want_uv else None, mips_built, buf.data_ptr(), stream)
        assert rc == 0, L.gsrast_last_error()
    torch.cuda.synchronize()
    return out, grads, d_pts, d_lv, bool(torch.equal(buf[nbytes:], pattern))


@pytest.mark.gpu
def test_capi_mips_not_built(gpu):
    """mips_built = 0 (Python always passes 1): the backward rebuilds the value stacks itself, on a scratch buffer that holds 0xFF
    bytes.  d_pts / d_levels equal the mips_built = 1 run bit for bit, dtex is within the bar."""
    ref = _generic_ref(32, 8, 8, 7, 500, 328)
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    tex = [t(np.ascontiguousarray(np.transpose(ref.tex, (1, 2, 0))))]
    args = (gpu, tex, [(0, 1)], [7], [0], 8, t(ref.uv), t(ref.lv), t(ref.dy))
    out, g1, dp1, dl1, ok1 = _capi_call(*args, forward=True, mips_built=1)
    _, g0, dp0, dl0, ok0 = _capi_call(*args, forward=False, mips_built=0)
    assert ok1 and ok0
    assert torch.equal(dp0.view(torch.int32), dp1.view(torch.int32)) and torch.equal(dl0.view(torch.int32), dl1.view(torch.int32))
    for g, dp, dl, what in ((g1, dp1, dl1, "mips_built=1"), (g0, dp0, dl0, "mips_built=0")):
        ref.check((out.cpu().numpy(), g[0].permute(2, 0, 1).cpu().numpy(), dp.cpu().numpy(), dl.cpu().numpy()), "C ABI " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 257])
def test_capi_scratch_guard_one_plane(gpu, N):
    """A 4 KB patterned guard right behind scratch_bytes bytes is intact after forward + backward."""
    ref = _generic_ref(16, 16, 4, 7, N, 90 + N)
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    tex = [t(np.ascontiguousarray(np.transpose(ref.tex, (1, 2, 0))))]
    out, g, dp, dl, intact = _capi_call(gpu, tex, [(0, 1)], [7], [0], 4, t(ref.uv), t(ref.lv), t(ref.dy))
    assert intact
    ref.check((out.cpu().numpy(), g[0].permute(2, 0, 1).cpu().numpy(), dp.cpu().numpy(), dl.cpu().numpy()), f"C ABI guard N{N}")


@pytest.mark.gpu
def test_capi_scratch_guard_24_planes(gpu):
    rng = np.random.default_rng(24)
    C, N = 4, 300
    grids = _field(rng, [8, 8, 8, 5], C, (1, 2, 4, 8))
    pts, levels, _ = _field_inputs(rng, N, 6)
    dy = rng.normal(size=(N, 4 * C)).astype(np.float32)
    f, dg, d_pts, d_levels = tor.interpolate_ms_features(pts, [[g[0] for g in gs] for gs in grids], levels, dy)
    t = lambda a: torch.tensor(a, device=gpu)  # noqa: E731
    texs = [t(np.ascontiguousarray(np.transpose(g[0], (1, 2, 0)))) for gs in grids for g in gs]
    cols = [c for _ in grids for c in tor.PLANES]
    mms = [7 if 3 not in c else 0 for c in cols]
    offs = [si * C for si in range(4) for _ in range(6)]
    out, g, dp, dl, intact = _capi_call(gpu, texs, cols, mms, offs, 4 * C, t(pts), t(levels), t(dy))
    assert intact
    _close(out.cpu().numpy(), f, 1e-5, "features")
    for k, gk in enumerate(g):
        _close(gk.permute(2, 0, 1).cpu().numpy(), dg[k // 6][k % 6], 1e-5, f"dgrid {k}")


@pytest.mark.gpu
def test_block_rules_and_uncovered_columns(gpu):
    """Planes that share a block but are not adjacent, or blocks that partly overlap, are refused (the forward would overwrite one
    plane's sum with another's); columns no plane covers read 0, whatever the allocator hands out."""
    import fused_hexplane
    rng = np.random.default_rng(3)
    C, N = 4, 300
    g = [torch.tensor(rng.normal(size=(1, C, 8, 8)).astype(np.float32), device=gpu, requires_grad=True) for _ in range(3)]
    uv = torch.rand((N, 2), device=gpu)
    lv = torch.rand((N, 2), device=gpu) * 3
    with pytest.raises(RuntimeError, match="must be adjacent"):
        fused_hexplane.texture_planes(uv, lv, g, [(0, 1)] * 3, [7] * 3, [0, 4, 0], 8)
    with pytest.raises(RuntimeError, match="equal or disjoint"):
        fused_hexplane.texture_planes(uv, lv, [torch.zeros((1, 8, 8, 8), device=gpu)] * 2, [(0, 1)] * 2, [7] * 2, [0, 4], 16)
    with pytest.raises(RuntimeError, match="feature block outside the row"):
        fused_hexplane.texture_planes(uv, lv, g[:1], [(0, 1)], [7], [8], 8)
    adjacent = fused_hexplane.texture_planes(uv, lv, g, [(0, 1)] * 3, [7] * 3, [0, 0, 4], 8)              # the same planes in an accepted order
    want = [tor.texture(np.transpose(x.detach().cpu().numpy()[0], (1, 2, 0)), uv.cpu().numpy(), lv.cpu().numpy().min(1), 7) for x in g]
    _close(adjacent.detach().cpu().numpy(), np.concatenate([want[0] + want[1], want[2]], axis=1), 1e-5, "adjacent blocks")
    for _ in range(2):
        poison = torch.full((N, 16), float("nan"), device=gpu)      # the block the next torch.empty of this size gets back
        del poison
        o = fused_hexplane.texture_planes(uv, lv, g[:2], [(0, 1)] * 2, [7] * 2, [4, 12], 16)
        got = o.detach().cpu().numpy()
        assert np.all(got[:, 0:4] == 0.0) and np.all(got[:, 8:12] == 0.0)
        _close(got[:, 4:8], want[0], 1e-5, "block after a gap")
        _close(got[:, 12:16], want[1], 1e-5, "last block")
    o.sum().backward()
    assert torch.isfinite(g[0].grad).all() and torch.isfinite(g[1].grad).all()
