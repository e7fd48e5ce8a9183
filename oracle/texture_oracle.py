"""TEST INFRASTRUCTURE ONLY (oracle): numpy fp64 restatement of the mip-mapped plane lookup the reference's residual
field performs through `nvdiffrast.torch.texture` (last item).  Only tests/, __graft_entry__.smoke()
and bench.py's baseline legs may import this file; the product path (saro-gs_amd/fused_hexplane.py over
csrc/gsrast_hexplane.h) never does.

PARITY UNPINNED against the dependency itself: nvdiffrast is neither vendored in /root/reference nor installed in this
image, and the reference pins no version of it (README.md:29 only links its install page), so its binary cannot be run here.
What is restated is its PUBLISHED algorithm (NVlabs/nvdiffrast, texture op, `filter_mode='linear-mipmap-linear'`,
`boundary_mode='clamp'`, mip level from `mip_level_bias` only), anchored on the reference's own call site:

  scene/hexplane.py:26-60   grid_sample_wrapper: tex = grid[1,C,H,W] -> [1,H,W,C]; uv = coords; bias = min over the
                            plane's two coordinates of `levels`; boundary_mode="clamp"; max_mip_level = 7 (spatial
                            plane) or 0 (plane with a time axis); filter_mode left at 'auto' = linear-mipmap-linear
                            because a bias is given
  scene/hexplane.py:95-139  interpolate_ms_features: six planes (itertools.combinations(range(4), 2)) summed per scale,
                            scales concatenated
  scene/hexplane.py:237-249 get_level: level = log2(2 * clamp(scale) / base_scale), 0 for the time axis

Published algorithm, as restated here:
  * mip stack: level l+1 = 2x2 box average of level l (2x1 / 1x2 when one extent is already 1); built while either
    extent is > 1 and l < max_mip_level; an odd extent > 1 cannot be halved (the op rejects it: error here as well)
  * level: flevel = clamp(bias, 0, n_levels); level0 = floor(flevel); if flevel > 0: level1 = min(level0 + 1, n_levels),
    f = flevel - level0; else single level
  * per level: texel space u = uv.x * w - 0.5, clamped to [0, w - 1]; i0 = floor(u), i1 = i0 + 1 unless the clamp hit
    (then i1 = i0: zero uv gradient), fractional weights; bilinear; out = a + f * (b - a)
  * gradients: to the texels of both levels (then pulled down the stack to level 0, the transpose of the box average),
    to uv (bilinear slope * extent, 0 where clamped), to the bias (sum_c dy_c (b_c - a_c) where f > 0)

Beside the fp64 restatement the same functions give, for the tests' per-element bars, an fp32 restatement (dtype=np.float32; the
texel gradient summed in a chosen point order) and the ABSOLUTE COMPANION (absolute=True: every term replaced by its absolute
value, the size of what was summed into each element); interpolate_ms_features covers the summed-scales and space | time
layouts and returns d_pts / d_levels as well.

The structure (box-average pyramid, border-clamped half-texel-centred bilinear, level lerp) is pinned against torch's own
`avg_pool2d` + `grid_sample(padding_mode='border', align_corners=False)` + autograd in tests/test_oracle_texture.py.
"""
import itertools

import numpy as np


def mip_sizes(W, H, max_mip_level):
    """[(w, h)] for levels 0..n_levels."""
    sizes = [(int(W), int(H))]
    w, h = int(W), int(H)
    while (w > 1 or h > 1) and len(sizes) - 1 < max_mip_level:
        if (w > 1 and (w & 1)) or (h > 1 and (h & 1)):
            raise ValueError(f"mip level {len(sizes) - 1} has an odd extent ({w}x{h}): limit max_mip_level")
        w, h = max(w >> 1, 1), max(h >> 1, 1)
        sizes.append((w, h))
    return sizes


def build_mips(tex, max_mip_level, dtype=np.float64):
    """tex [H, W, C] -> list of levels, every operation in `dtype`."""
    T = np.dtype(dtype).type
    tex = np.asarray(tex, dtype)
    H, W, _ = tex.shape
    out = [tex]
    for (w, h) in mip_sizes(W, H, max_mip_level)[1:]:
        p = out[-1]
        ph, pw = p.shape[:2]
        if pw > 1 and ph > 1:
            n = T(0.25) * (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2])
        elif pw > 1:
            n = T(0.5) * (p[:, 0::2] + p[:, 1::2])
        else:
            n = T(0.5) * (p[0::2] + p[1::2])
        assert n.shape[:2] == (h, w) and n.dtype == tex.dtype
        out.append(n)
    return out


def pull_down(dmips, dtype=np.float64):
    """Transpose of build_mips: gradient of all levels -> gradient of level 0."""
    T = np.dtype(dtype).type
    d = [np.array(x, dtype) for x in dmips]
    for l in range(len(d) - 1, 0, -1):
        g, p = d[l], d[l - 1]
        ph, pw = p.shape[:2]
        if pw > 1 and ph > 1:
            for dy, dx in itertools.product((0, 1), (0, 1)):
                p[dy::2, dx::2] += T(0.25) * g
        elif pw > 1:
            p[:, 0::2] += T(0.5) * g
            p[:, 1::2] += T(0.5) * g
        else:
            p[0::2] += T(0.5) * g
            p[1::2] += T(0.5) * g
    return d[0]


def _level_terms(uv, w, h):
    T = uv.dtype.type
    u = uv[:, 0] * T(w) - T(0.5)
    v = uv[:, 1] * T(h) - T(0.5)
    u = np.minimum(np.maximum(u, T(0.0)), T(w - 1.0))
    v = np.minimum(np.maximum(v, T(0.0)), T(h - 1.0))
    cu = (u == 0.0) | (u == w - 1.0)
    cv = (v == 0.0) | (v == h - 1.0)
    iu0 = np.floor(u).astype(np.int64)
    iv0 = np.floor(v).astype(np.int64)
    iu1 = iu0 + np.where(cu, 0, 1)
    iv1 = iv0 + np.where(cv, 0, 1)
    return iu0, iu1, iv0, iv1, u - iu0.astype(uv.dtype), v - iv0.astype(uv.dtype)


def _levels(bias, n_levels, dtype=np.float64):
    T = np.dtype(dtype).type
    fl = np.minimum(np.maximum(np.asarray(bias, dtype), T(0.0)), T(n_levels))
    l0 = np.floor(fl).astype(np.int64)
    two = fl > 0.0
    l1 = np.where(two, np.minimum(l0 + 1, n_levels), 0)
    f = np.where(two, fl - l0.astype(dtype), T(0.0))
    return l0, l1, f


def texture(tex, uv, bias, max_mip_level, dy=None, dtype=np.float64, order=None, absolute=False):
    """tex [H,W,C], uv [N,2], bias [N] -> out [N,C]; with dy [N,C] also (dtex [H,W,C], duv [N,2], dbias [N]).

    dtype     every operation in that type (np.float32: the same arithmetic as a plain fp32 program would do it; the texel
              gradient is then summed point by point in fp32, in the order of `order`)
    order     a permutation of the points: the order in which their contributions reach the texel gradient (nothing else
              depends on it; outputs per point come back in the caller's order)
    absolute  the ABSOLUTE COMPANION: the same formulas with every term replaced by its absolute value.  All interpolation
              weights are non-negative, so out is the lookup of |tex| and dtex is the texel gradient of |dy|; a texel
              difference b - a becomes |b| + |a| in the uv slopes and in the bias gradient.  It is the size s_i of what
              was summed into element i: an fp32 evaluation errs by a small multiple of 2^-24 s_i, whatever cancelled."""
    if order is not None:
        order = np.asarray(order)
        inv = np.empty_like(order)
        inv[order] = np.arange(order.size)
        r = texture(tex, np.asarray(uv)[order], np.asarray(bias)[order], max_mip_level, None if dy is None else np.asarray(dy)[order],
                    dtype=dtype, absolute=absolute)
        return r[inv] if dy is None else (r[0][inv], r[1], r[2][inv], r[3][inv])
    T = np.dtype(dtype).type
    if absolute:
        tex = np.abs(np.asarray(tex, dtype))
    mips = build_mips(tex, max_mip_level, dtype)
    uv = np.asarray(uv, dtype)
    N, C = uv.shape[0], mips[0].shape[2]
    l0, l1, f = _levels(bias, len(mips) - 1, dtype)
    sgn = T(1.0) if absolute else T(-1.0)        # a difference b - a is b + sgn * a
    want = dy is not None
    if want:
        dy = np.asarray(dy, dtype)
        if absolute:
            dy = np.abs(dy)
        dm = [np.zeros_like(m) for m in mips]
        duv = np.zeros((N, 2), dtype)
    vals = {}
    for which, lv in ((0, l0), (1, l1)):
        B = np.zeros((N, C), dtype)
        for l in np.unique(lv):
            sel = np.nonzero(lv == l)[0] if which == 0 else np.nonzero((lv == l) & (f > 0.0))[0]
            if sel.size == 0:
                continue
            m = mips[l]
            h, w = m.shape[:2]
            iu0, iu1, iv0, iv1, fu, fv = _level_terms(uv[sel], w, h)
            a00, a10, a01, a11 = m[iv0, iu0], m[iv0, iu1], m[iv1, iu0], m[iv1, iu1]
            fu_, fv_ = fu[:, None], fv[:, None]
            top = a00 + (a10 - a00) * fu_
            bot = a01 + (a11 - a01) * fu_
            B[sel] = top + (bot - top) * fv_
            if want:
                one = T(1.0)
                wl = (one - f[sel]) if which == 0 else f[sel]
                g = dy[sel] * wl[:, None]
                np.add.at(dm[l], (iv0, iu0), g * (one - fu_) * (one - fv_))
                np.add.at(dm[l], (iv0, iu1), g * fu_ * (one - fv_))
                np.add.at(dm[l], (iv1, iu0), g * (one - fu_) * fv_)
                np.add.at(dm[l], (iv1, iu1), g * fu_ * fv_)
                # a clamped axis has i1 == i0: its difference is 0 (and stays 0 in the absolute companion)
                dx0, dx1 = np.where(iu1 != iu0, 1, 0).astype(dtype)[:, None], np.where(iv1 != iv0, 1, 0).astype(dtype)[:, None]
                dBdu = (dx0 * (a10 + sgn * a00) * (one - fv_) + dx0 * (a11 + sgn * a01) * fv_) * T(w)
                dBdv = (dx1 * (a01 + sgn * a00) * (one - fu_) + dx1 * (a11 + sgn * a10) * fu_) * T(h)
                duv[sel, 0] += (g * dBdu).sum(1, dtype=dtype)
                duv[sel, 1] += (g * dBdv).sum(1, dtype=dtype)
        vals[which] = B
    two = (f > 0.0)[:, None]
    out = np.where(two, vals[0] + f[:, None] * (vals[1] - vals[0]), vals[0])
    if not want:
        return out
    dbias = np.where(f > 0.0, (dy * (vals[1] + sgn * vals[0])).sum(1, dtype=dtype), T(0.0))
    return out, pull_down(dm, dtype), duv, dbias


PLANES = list(itertools.combinations(range(4), 2))      # scene/hexplane.py:105-107: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)


def field_layout(n_scales, C, concat_features=True, concat_planes=False):
    """(feature width, offsets[scale][plane]) of scene/hexplane.py:95-139: the six planes of a scale are summed into one
    block (concat_planes: planes 0, 1, 3 = space into one block, 2, 4, 5 = those with the time axis into the next, :121-125);
    the scales' blocks are concatenated (concat_features) or summed."""
    groups = [[0, 1, 3], [2, 4, 5]] if concat_planes else [list(range(len(PLANES)))]
    per_scale = C * len(groups)
    offs = [[(s * per_scale if concat_features else 0) + next(gi for gi, g in enumerate(groups) if ci in g) * C
             for ci in range(len(PLANES))] for s in range(n_scales)]
    return (per_scale * n_scales if concat_features else per_scale), offs


def interpolate_ms_features(pts, ms_grids, levels, dy=None, concat_features=True, concat_planes=False, dtype=np.float64, order=None,
                            absolute=False):
    """scene/hexplane.py:95-139; the defaults concat_features=True, concat_planes=False are the values ScaleAwareResField
    fixes (:168-169).  pts [N,4] in texture coordinates, ms_grids[scale][plane] = [C, H, W] (the parameter's layout without
    its leading 1), levels [N,4].  Returns features [N, F]; with dy [N, F] also the per-grid gradients (same nesting) and
    d_pts [N,4], d_levels [N,4]: sums over the planes that share a column; a plane's bias is min(levels[cu], levels[cv]), so
    its bias gradient goes to the smaller of the two level columns, to cu on a tie (what torch.min does).
    dtype / order / absolute: as in texture()."""
    T = np.dtype(dtype).type
    pts = np.asarray(pts, dtype)
    levels = np.asarray(levels, dtype)
    N = pts.shape[0]
    C = ms_grids[0][0].shape[0]
    F, offs = field_layout(len(ms_grids), C, concat_features, concat_planes)
    f = np.zeros((N, F), dtype)
    dgrids = []
    d_pts, d_levels = np.zeros((N, 4), dtype), np.zeros((N, 4), dtype)
    for s, grids in enumerate(ms_grids):
        dg = []
        for ci, comb in enumerate(PLANES):
            cu, cv = comb
            off = offs[s][ci]
            tex = np.transpose(np.asarray(grids[ci], dtype), (1, 2, 0))                # hexplane.py:35 permute(0,2,3,1)
            bias = np.minimum(levels[:, cu], levels[:, cv])                            # hexplane.py:46
            mm = 7 if 3 not in comb else 0                                             # hexplane.py:55, :117
            if dy is None:
                f[:, off:off + C] += texture(tex, pts[:, [cu, cv]], bias, mm, dtype=dtype, absolute=absolute)
                continue
            o, dt, duv, db = texture(tex, pts[:, [cu, cv]], bias, mm, np.asarray(dy)[:, off:off + C], dtype=dtype, order=order, absolute=absolute)
            f[:, off:off + C] += o
            dg.append(np.transpose(dt, (2, 0, 1)))
            d_pts[:, cu] += duv[:, 0]
            d_pts[:, cv] += duv[:, 1]
            to_v = levels[:, cv] < levels[:, cu]
            d_levels[:, cu] += np.where(to_v, T(0.0), db)
            d_levels[:, cv] += np.where(to_v, db, T(0.0))
        dgrids.append(dg)
    return f if dy is None else (f, dgrids, d_pts, d_levels)
