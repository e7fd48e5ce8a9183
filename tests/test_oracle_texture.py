"""CPU: pins oracle/texture_oracle.py's structure (box-average mip stack, border-clamped bilinear with half-texel
centres, level lerp, and all three gradients) against torch's own avg_pool2d + grid_sample + autograd in fp64.
(The dependency it restates, nvdiffrast, is absent from the image: see the oracle's header.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import texture_oracle as tor


def torch_texture(tex, uv, bias, max_mip_level):
    """tex [H,W,C] (requires_grad ok), uv [N,2], bias [N]: pyramid by avg_pool2d, border bilinear per level, lerp."""
    t = tex.permute(2, 0, 1)[None]                     # [1,C,H,W]
    mips = [t]
    while (mips[-1].shape[2] > 1 or mips[-1].shape[3] > 1) and len(mips) - 1 < max_mip_level:
        h, w = mips[-1].shape[2:]
        mips.append(F.avg_pool2d(mips[-1], (2 if h > 1 else 1, 2 if w > 1 else 1)))
    n = len(mips) - 1
    fl = bias.clamp(0.0, float(n))
    l0 = fl.detach().floor().long()
    l1 = torch.clamp(l0 + 1, max=n)
    f = fl - l0
    grid = (2.0 * uv - 1.0)[None, None]                # [1,1,N,2]
    per_level = [F.grid_sample(m, grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].t() for m in mips]
    stack = torch.stack(per_level)                     # [L,N,C]
    idx = torch.arange(uv.shape[0])
    a, b = stack[l0, idx], stack[l1, idx]
    return a + f[:, None] * (b - a)


@pytest.mark.parametrize("W,H,C,mm", [(16, 16, 5, 7), (32, 8, 3, 7), (8, 32, 4, 2), (12, 10, 3, 0), (64, 64, 4, 3), (4, 1, 2, 7)])
def test_oracle_matches_torch_autograd(W, H, C, mm):
    rng = np.random.default_rng(W * 131 + H)
    N = 400
    tex = rng.normal(size=(H, W, C))
    uv = rng.uniform(-0.1, 1.1, size=(N, 2))           # some points beyond the border (clamp)
    uv[:5] = [[0.0, 0.0], [1.0, 1.0], [0.5 / W, 0.5 / H], [1 - 0.5 / W, 0.3], [0.3, 1.0]]
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    bias = rng.uniform(-0.5, n_levels + 0.7, size=N)
    bias[5:9] = [0.0, float(n_levels), 0.25, n_levels - 0.25]
    dy = rng.normal(size=(N, C))
    out, dtex, duv, dbias = tor.texture(tex, uv, bias, mm, dy)
    t = torch.tensor(tex, requires_grad=True)
    u = torch.tensor(uv, requires_grad=True)
    b = torch.tensor(bias, requires_grad=True)
    o = torch_texture(t, u, b, mm)
    o.backward(torch.tensor(dy))
    assert np.abs(out - o.detach().numpy()).max() < 1e-12
    assert np.abs(dtex - t.grad.numpy()).max() < 1e-11
    # torch's border mode lets the uv gradient through at an exactly-clamped coordinate on the inside; the restated op zeroes
    # it there (i1 = i0).  Compare away from exact clamps.
    inside = np.ones(N, bool)
    inside[:5] = False
    assert np.abs(duv - u.grad.numpy())[inside].max() < 1e-9
    # bias gradient: torch's clamp passes gradient at the closed ends, the op's `flevel > 0` test does not; and an exactly
    # integral level has f = 0 (single level).  Compare strictly inside.
    strict = (bias > 0) & (bias < n_levels) & (bias != np.floor(bias))
    if n_levels:
        assert np.abs(dbias - b.grad.numpy())[strict].max() < 1e-10
    assert np.all(dbias[~((bias > 0) & (bias < n_levels))] == 0.0)


def test_mip_rules():
    assert tor.mip_sizes(64, 64, 7) == [(64 >> l, 64 >> l) for l in range(7)]
    assert tor.mip_sizes(512, 512, 7)[-1] == (4, 4)
    assert tor.mip_sizes(64, 150, 0) == [(64, 150)]
    assert tor.mip_sizes(8, 2, 7) == [(8, 2), (4, 1), (2, 1), (1, 1)]
    with pytest.raises(ValueError):
        tor.mip_sizes(12, 10, 7)                       # 6x5: odd extent cannot be halved
    rng = np.random.default_rng(0)
    d = [rng.normal(size=(8 >> l, 8 >> l, 2)) for l in range(4)]
    tex = rng.normal(size=(8, 8, 2))
    # pull_down is the transpose of build_mips: <build(tex), d> == <tex, pull_down(d)> (+ level 0 identity)
    lhs = sum((m * g).sum() for m, g in zip(tor.build_mips(tex, 3), d))
    assert abs(lhs - (tex * tor.pull_down(d)).sum()) < 1e-12


def test_field_layout():
    """interpolate_ms_features: planes summed per scale, scales concatenated, time planes unmipped (hexplane.py:95-139)."""
    rng = np.random.default_rng(3)
    reso = [8, 8, 8, 6]
    grids = [[rng.normal(size=(3, reso[b] * m, reso[a] * m if a < 3 else reso[a])) if b < 3 else rng.normal(size=(3, reso[b], reso[a] * m))
              for (a, b) in tor.PLANES] for m in (1, 2)]
    N = 50
    pts = rng.uniform(0, 1, size=(N, 4))
    levels = np.concatenate([rng.uniform(0, 3, size=(N, 3)), np.zeros((N, 1))], axis=1)
    f = tor.interpolate_ms_features(pts, grids, levels)
    assert f.shape == (N, 6)
    want = sum(tor.texture(np.transpose(grids[1][ci], (1, 2, 0)), pts[:, list(c)], levels[:, list(c)].min(1), 7 if 3 not in c else 0)
               for ci, c in enumerate(tor.PLANES))
    assert np.abs(f[:, 3:] - want).max() < 1e-12
    dy = rng.normal(size=(N, 6))
    f2, dg, _, _ = tor.interpolate_ms_features(pts, grids, levels, dy)
    assert np.abs(f2 - f).max() == 0 and dg[1][2].shape == grids[1][2].shape
    # gradient check by linearity: <dy, F(G + E) - F(G)> == <dG, E>
    E = [[rng.normal(size=g.shape) for g in gs] for gs in grids]
    f3 = tor.interpolate_ms_features(pts, [[g + e for g, e in zip(gs, es)] for gs, es in zip(grids, E)], levels)
    lhs = (dy * (f3 - f)).sum()
    rhs = sum((d * e).sum() for ds, es in zip(dg, E) for d, e in zip(ds, es))
    assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs))


def _small_field(rng, reso, C, mults):
    return [[rng.normal(size=(C, reso[b] * m if b < 3 else reso[b], reso[a] * m if a < 3 else reso[a])) for (a, b) in tor.PLANES] for m in mults]


def _torch_field(pts, grids, levels, concat_features, concat_planes):
    """The fp64 torch composition: torch_texture per plane with the bias torch.min over the plane's two level columns
    (hexplane.py:46), six planes summed per block, blocks laid out like hexplane.py:95-139."""
    C = grids[0][0].shape[0]
    F_, offs = tor.field_layout(len(grids), C, concat_features, concat_planes)
    blocks = {}
    for s, gs in enumerate(grids):
        for ci, (cu, cv) in enumerate(tor.PLANES):
            bias = torch.min(levels[:, [cu, cv]], dim=-1).values
            o = torch_texture(gs[ci].permute(1, 2, 0), pts[:, [cu, cv]], bias, 7 if 3 not in (cu, cv) else 0)
            blocks[offs[s][ci]] = blocks[offs[s][ci]] + o if offs[s][ci] in blocks else o
    assert sorted(blocks) == list(range(0, F_, C))
    return torch.cat([blocks[k] for k in sorted(blocks)], dim=1)


@pytest.mark.parametrize("concat_features,concat_planes", [(True, False), (False, False), (True, True), (False, True)])
def test_field_gradients_match_torch_autograd(concat_features, concat_planes):
    """d_pts / d_levels (sums over the planes sharing a column, bias gradient to the smaller level column, cu on a tie) and
    every layout of interpolate_ms_features, against autograd of the torch composition.  Bars: the ones of
    test_oracle_matches_torch_autograd above."""
    rng = np.random.default_rng(17 + 2 * concat_features + concat_planes)
    grids = _small_field(rng, [8, 8, 8, 6], 4, (1, 2))
    N = 300
    pts = rng.uniform(-0.1, 1.1, size=(N, 4))
    levels = np.concatenate([rng.uniform(0.05, 2.95, size=(N, 3)), np.zeros((N, 1))], axis=1)     # strictly inside (0, n_levels), time level 0
    levels[:40, 1] = levels[:40, 0]                       # ties cu == cv of plane (0, 1), and of (0, 2) / (1, 2) below
    levels[20:60, 2] = levels[20:60, 0]
    levels[60:70, 2] = levels[60:70, 1]
    assert not np.any(levels[:, :3] == np.floor(levels[:, :3]))
    F_, _ = tor.field_layout(2, 4, concat_features, concat_planes)
    dy = rng.normal(size=(N, F_))
    f, dg, d_pts, d_levels = tor.interpolate_ms_features(pts, grids, levels, dy, concat_features, concat_planes)
    assert f.shape == (N, F_) == {(True, False): (N, 8), (False, False): (N, 4), (True, True): (N, 16), (False, True): (N, 8)}[(concat_features, concat_planes)]
    assert np.array_equal(f, tor.interpolate_ms_features(pts, grids, levels, None, concat_features, concat_planes))
    tg = [[torch.tensor(g, requires_grad=True) for g in gs] for gs in grids]
    tp, tl = torch.tensor(pts, requires_grad=True), torch.tensor(levels, requires_grad=True)
    o = _torch_field(tp, tg, tl, concat_features, concat_planes)
    o.backward(torch.tensor(dy))
    assert np.abs(f - o.detach().numpy()).max() < 1e-12
    for s in range(2):
        for ci in range(6):
            assert np.abs(dg[s][ci] - tg[s][ci].grad.numpy()).max() < 1e-11, (s, ci)
    assert np.abs(d_pts - tp.grad.numpy()).max() < 1e-9
    assert np.abs(d_levels - tl.grad.numpy()).max() < 1e-10
    assert np.all(d_levels[:, 3] == 0.0) and np.any(d_levels[:40, 0] != 0.0)
    # a tie inside (0, n): all of the plane's bias gradient in the lower column.  Rows 0..19 tie columns 0 and 1 only, so column 1
    # holds nothing but plane (1, 2)'s share, which is 0 where level 2 is the smaller
    rows = np.nonzero(levels[:20, 2] < levels[:20, 1])[0]
    assert rows.size and np.all(d_levels[rows, 1] == 0.0)


@pytest.mark.parametrize("W,H,C,mm", [(16, 16, 4, 7), (2, 8, 4, 7), (24, 40, 3, 3), (12, 10, 3, 0)])
def test_restatement_options(W, H, C, mm):
    """dtype / order / absolute of texture(): the fp32 restatement is the same function in fp32; a point order moves nothing but
    the texel gradient's rounding; the absolute companion bounds every element and equals the plain result on non-negative data."""
    rng = np.random.default_rng(W + 3 * H)
    N = 500
    n_levels = len(tor.mip_sizes(W, H, mm)) - 1
    tex = rng.normal(size=(H, W, C)).astype(np.float32)
    uv = rng.uniform(-0.05, 1.05, size=(N, 2)).astype(np.float32)
    bias = rng.uniform(-0.5, n_levels + 0.7, size=N).astype(np.float32)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    r64 = tor.texture(tex, uv, bias, mm, dy)
    perm = rng.permutation(N)
    p64 = tor.texture(tex, uv, bias, mm, dy, order=perm)
    assert np.array_equal(p64[0], r64[0]) and np.array_equal(p64[2], r64[2]) and np.array_equal(p64[3], r64[3])
    assert np.abs(p64[1] - r64[1]).max() < 1e-11
    r32 = tor.texture(tex, uv, bias, mm, dy, dtype=np.float32)
    assert all(x.dtype == np.float32 for x in r32)
    assert np.array_equal(tor.texture(tex, uv, bias, mm, dtype=np.float32), r32[0])
    s = tor.texture(tex, uv, bias, mm, dy, absolute=True)
    for name, a, b in zip(("features", "dtex", "duv", "dbias"), s, r64):
        assert a.shape == b.shape and np.all(a >= 0.0), name
        assert np.all(np.abs(b) <= a + 1e-12 * a.max()), name
    # what the companion is for: the fp32 restatement's error, element by element, is a modest multiple of 2^-24 s_i for the tensors no
    # discrete choice enters (features, dtex).  Each is a sum of <= 8 N products of <= 5 factors: N * 2^-24 s_i bounds it with room
    for name, a, b, c in zip(("features", "dtex"), s[:2], r64[:2], r32[:2]):
        assert np.all(np.abs(c - b) <= N * 2.0 ** -24 * a), name
        assert np.all(c[a == 0.0] == 0.0), name
    pos = tor.texture(np.abs(tex), uv, bias, mm, np.abs(dy))
    assert np.array_equal(s[0], pos[0]) and np.array_equal(s[1], pos[1])
    # the field: absolute and fp32 variants keep the nesting and the routing of the bias gradient
    grids = _small_field(rng, [4, 4, 4, 3], 4, (1, 2))
    pts = rng.uniform(0, 1, size=(50, 4))
    levels = np.concatenate([rng.uniform(0, 2, size=(50, 3)), np.zeros((50, 1))], axis=1)
    dyf = rng.normal(size=(50, 8))
    a = tor.interpolate_ms_features(pts, grids, levels, dyf, absolute=True)
    b = tor.interpolate_ms_features(pts, grids, levels, dyf)
    c = tor.interpolate_ms_features(pts, grids, levels, dyf, dtype=np.float32, order=rng.permutation(50))
    for k in (0, 2, 3):
        assert np.all(np.abs(b[k]) <= a[k] + 1e-12 * a[k].max()) and c[k].dtype == np.float32 and c[k].shape == b[k].shape
    assert np.all(np.abs(c[0] - b[0]) <= 50 * 2.0 ** -24 * a[0])
    assert np.all(a[3][:, 3] == 0.0) and np.all(b[3][a[3] == 0.0] == 0.0) and np.any(a[3][:, :3] == 0.0)
    assert all(np.all(np.abs(y) <= x + 1e-12 * x.max()) for xs, ys in zip(a[1], b[1]) for x, y in zip(xs, ys))
