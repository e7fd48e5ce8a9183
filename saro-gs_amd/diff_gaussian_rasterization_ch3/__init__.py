"""diff_gaussian_rasterization_ch3 -- drop-in replacement, MI355X (gfx950) native.

Same import name and public surface as the rasterizer the SaRO-GS renderer imports
(/root/reference/renderer/__init__.py:32):

    from diff_gaussian_rasterization_ch3 import GaussianRasterizationSettings, GaussianRasterizer

so ``renderer.train_render`` / ``test_render`` and ``scene/saro_gaussian.py`` can call it unchanged.
Behaviour follows /root/reference/submodules/gaussian_rasterization_ch3/
diff_gaussian_rasterization_ch3/__init__.py (cited below as REF:line):

* ``GaussianRasterizationSettings`` -- NamedTuple with the reference's eleven fields in the
  reference's order (REF:134-145).
* ``GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
  scales=None, rotations=None, cov3D_precomp=None)`` -> ``(color[3,H,W], radii[P] int32,
  depth[1,H,W])`` (REF:163-196, REF:85).  Exactly one of (shs, colors_precomp) and exactly one of
  ((scales, rotations), cov3D_precomp) must be given, otherwise ``Exception`` (REF:167-171).
* autograd: gradients flow to means3D, means2D (a [P,3] tensor whose [:, :2] drives densification),
  shs / colors_precomp, opacities, scales, rotations, cov3D_precomp; depth and radii carry no
  gradient (REF:88, REF:120-130).
* ``GaussianRasterizer.markVisible(positions)`` (REF:152-161).
* not in the reference: ``forward(..., return_aux=True)`` (also ``rasterize_gaussians`` and ``GaussianRasterizerRaw``) returns
  ``(color, radii, depth, acc_depth[1,H,W], alpha[1,H,W])`` -- alpha = 1 - T_final and the accumulated depth
  sum_i alpha_i T_i z_i (not normalised: expected depth = acc_depth / alpha), both differentiable like the colour
  (include/gsrast.h: GSRAST_RENDER_AUX).  The median ``depth`` keeps the reference's zero gradient.
* not in the reference: ``forward(..., antialiasing=True)`` (keyword-only, default False; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, and together with ``return_aux``) -- upstream 3DGS's ``antialiasing``, the 2-D Mip filter of
  Mip-Splatting: each Gaussian's opacity is scaled by sqrt(det cov2D / det(cov2D + 0.3 I)) so that the 0.3 px^2 dilation does not
  inflate small or distant Gaussians; differentiable, also through that factor (include/gsrast.h: GSRAST_RENDER_ANTIALIAS).  Train
  and evaluate with the same setting.
* not in the reference: ``forward(..., absgrad=sink)`` (keyword-only, default None; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, together with ``return_aux`` and ``antialiasing``) -- the absolute screen-space gradient of AbsGS
  (gsplat's ``absgrad``): `sink` is a caller-owned contiguous float32 ``[P, 2]`` tensor on the render's device, and every backward of
  that render OVERWRITES it with sum over pixels |d loss_pixel / d means2D[:, :2]|, in the units of ``means2D.grad`` (>= its absolute
  value; zero for Gaussians no pixel used).  Nothing is attached to ``means2D``; ``.backward()`` and ``torch.autograd.grad`` fill it
  alike.  A wrong shape / dtype / device / layout raises ``ValueError`` at forward time (include/gsrast.h: GSRAST_RENDER_ABSGRAD).
* not in the reference: ``forward(..., camera_grads=True)`` (keyword-only, default False; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, together with ``return_aux``, ``antialiasing``, ``absgrad`` and a ``GradArena``) -- gradients for the camera:
  ``raster_settings.viewmatrix``, ``.projmatrix`` and ``.campos`` are differentiated as three independent inputs, each only if it
  requires grad (gsplat's gradients on ``viewmats``).  A caller that builds ``projmatrix = viewmatrix @ projection`` and
  ``campos = inverse(viewmatrix)[3, :3]`` from a pose parameter gets that parameter's gradient through autograd.  tanfovx / tanfovy
  are not differentiated.  When none of the three requires grad the call is the plain one (include/gsrast.h: GSRAST_RENDER_POSEGRAD).
* not in the reference: ``forward(..., contrib=sink)`` (keyword-only, default None; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, together with ``return_aux``, ``antialiasing``, ``absgrad``, ``camera_grads`` and a ``GradArena``) -- per-Gaussian
  blend-weight statistics for importance pruning.  `sink` is a caller-owned contiguous float32 ``[P, 4]`` tensor on the render's device, and THE
  FORWARD overwrites it, on the current stream, behind everything it enqueued there (also under ``torch.no_grad()``); nothing is attached to
  the graph.  For one finished forward, take pixel p inside the image and Gaussian i.  i CONTRIBUTES to p when the forward blended it
  there: its position in the tile's list in force is below n_contrib[p] and it passed the forward's per-pair tests --
  power <= 0 && power >= threshold;  alpha = min(0.99, opacity * exp(power)) >= 1/255;  T * (1 - alpha) >= 1e-4
  (the terminating entry does not contribute).  Its weight is w_ip = alpha_ip * T_ip, T_ip the transmittance in front of it.
  m_p = pixel_weights[p] clamped to [0, 1]; without pixel_weights m_p = 1.  A pixel with m_p = 0 counts in no column.  One row per Gaussian:
  col 0 ``weight_sum`` = sum over p of m_p * w_ip;  col 1 ``weight_max`` = max over pixels with m_p > 0 of w_ip (unweighted);
  col 2 ``pixel_count`` = number of pixels with m_p > 0 that i contributes to;  col 3 ``top_count`` = number of those pixels where w_ip is
  the largest of the pixel's contributors (first in list order on a tie).  Gaussians that nobody consumed -- culled, off screen, late
  under the list cut, or listed behind every pixel's stop -- get a zero row.  The counts are float32: exact up to 2^24, rounded above.
  The result is bit-identical from run to run.  ``pixel_weights=w`` (keyword-only, default None; only legal together with ``contrib``): a
  float32 ``[H, W]`` or ``[1, H, W]`` tensor on the same device, e.g. a loss map or a mask.  A wrong shape / dtype / device / layout raises
  ``ValueError`` at call time, before any launch.  With ``contrib=None`` nothing is launched or allocated that was not before
  (include/gsrast.h: gsrast_contrib_stats; fused_densify.ContribStats accumulates the rows over views).
* not in the reference: ``forward(..., features=F)`` (keyword-only, default None; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, together with ``return_aux``, ``antialiasing``, ``absgrad``, ``camera_grads`` and ``contrib``) -- an arbitrary
  per-Gaussian vector blended with the colour's own weights (gsplat's N-channel ``colors``): semantic or language features, decoder
  features, motion, normals, uncertainty.  `F` is a contiguous float32 ``[P, C]`` tensor on the render's device, 1 <= C <= 64, and the
  returned tuple gets ``feature_map[C, H, W]`` APPENDED (behind ``alpha`` with ``return_aux=True``):
  feature_map[c][p] = sum_i alpha_ip * T_ip * F[i][c] over the Gaussians the forward blended at p (the contributors defined under
  ``contrib``), with the opacity the render used (anti-aliasing compensation included).  There is no background term: composite with
  ``1 - alpha`` of ``return_aux`` if one is wanted.  The map is differentiable: `F` receives sum_p w_ip * dL/dfeature_map, and
  ``means2D.grad``, ``opacities.grad``, the geometry leaves and the camera gradients of ``camera_grads=True`` include the map's loss
  (the backward then runs the blend phase, adds the map's terms to the per-Gaussian gradient records, and runs the per-Gaussian phase).
  ``absgrad`` stays a statistic of the colour and the aux outputs only.  With a ``GradArena`` installed ``features`` raises
  ``RuntimeError`` (the arena drives the two phases itself).  Under ``torch.no_grad()`` it is forward only.  A wrong shape / dtype /
  device / layout / C raises ``ValueError`` at call time, before any launch.  With ``features=None`` nothing is launched or allocated
  that was not before and the autograd node is the same (include/gsrast.h: gsrast_features_forward / gsrast_features_backward).
* not in the reference: ``forward(..., distortion=True)`` (keyword-only, default False; also ``rasterize_gaussians`` and
  ``GaussianRasterizerRaw``, together with ``return_aux``, ``antialiasing``, ``camera_grads``, ``contrib`` and ``features``) -- the
  depth-distortion map of Mip-NeRF 360 (gsplat's ``distloss`` / ``render_distort``, 2DGS's distortion term), the regulariser against
  floaters and semi-transparent shells.  The returned tuple gets ``distort_map[H, W]`` APPENDED as its LAST element (behind
  ``feature_map`` when both are asked for):  distort_map[p] = sum_i sum_j w_ip w_jp |z_i - z_j|  over the Gaussians the forward blended at
  p (the contributors defined under ``contrib``), w = alpha T with the opacity the render used, z the raw view-space depth that
  ``acc_depth`` sums (no near / far or NDC mapping, no background term); a pixel with fewer than two contributors reads 0.  The map is
  differentiable: ``means2D.grad``, ``opacities.grad``, the geometry leaves and the camera gradients of ``camera_grads=True`` include its
  loss, through the weights and through z (the backward runs the blend phase, adds the map's terms to the per-Gaussian gradient records
  -- beside the feature map's, if any -- and runs the per-Gaussian phase).  ``absgrad`` stays a statistic of the colour and the aux
  outputs only.  With a ``GradArena`` installed ``distortion=True`` raises ``RuntimeError``.  Under ``torch.no_grad()`` it is forward only.
  Its gradient needs the culled blend kernels (``options.cull != 0``, the default): ``RuntimeError`` otherwise.  With
  ``distortion=False`` nothing is launched or allocated that was not before (include/gsrast.h: gsrast_distortion_forward /
  gsrast_distortion_backward).
* not in the reference: ``pixel_contributors(means3D, opacities, scales, rotations, raster_settings=rs, K=8, order="weight")`` -- a call of
  its own, not a ``forward`` keyword: each pixel's heaviest (``order="weight"``) or first (``order="depth"``) K contributing Gaussians,
  their weights alpha T and the pixel's number of contributors, as ``PixelContributors(ids[K,H,W] int32, weights[K,H,W], count[H,W]
  int32, color, depth, radii)``; 1 <= K <= 16, unused slots hold -1 / +0.0.  One forward-only render and one replay of its blend; nothing
  is differentiable (include/gsrast.h: gsrast_pixel_contributors; the function's docstring has the definition).

The compute is in ``libgsrast_hip.so`` (hand-written HIP kernels behind the C ABI of
``include/gsrast.h``), reached through ``_C`` (ctypes).  There is no CPU / PyTorch fallback.
"""
from __future__ import annotations

import inspect
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _C

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "pixel_contributors", "PixelContributors"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool


def _no_arena_for_aux():
    if _C._grad_arena is not None:
        raise RuntimeError("return_aux=True is not supported with a GradArena installed (multi-GPU / view_parallel training): "
                           "uninstall it with _C.set_grad_arena(None) for renders that need acc_depth / alpha")


class _Request(NamedTuple):
    """What one render was asked for besides its inputs: `return_aux` and the keyword-only render options, parsed and checked once
    (_parse_request) and handed to the autograd node as ONE argument -- a tuple, so autograd sees no tensor in it.
    `distortion` is NOT one of the six fields (tests pin them as a tuple): it is a class attribute, False here and True in the subclass
    _DistortionRequest, so equality, repr and _asdict do not show it -- compare type(req) or req.distortion; _replace / _make keep the type."""
    return_aux: bool                            # two more outputs (acc_depth, alpha), two more incoming gradients
    antialiasing: bool                          # the backward must know how the state was filled
    absgrad: Optional[torch.Tensor]             # the caller's [P,2] sink (not a saved tensor: every backward writes it)
    contrib: Optional[torch.Tensor]             # the [P,4] sink of the blend-weight statistics, which the forward overwrites
    pixel_weights: Optional[torch.Tensor]       # its per-pixel weights (only legal with `contrib`)
    camera: bool                                # the backward also differentiates the camera
    distortion = False                          # (no field: _DistortionRequest)


class _DistortionRequest(_Request):
    """A _Request that also asks for the depth-distortion map: one more output (distort_map, the last), one more incoming gradient, one more
    saved tensor.  The record keeps its six fields; the bit travels in the record's type."""
    __slots__ = ()
    distortion = True


_RENDER_OPTIONS = frozenset(("antialiasing", "absgrad", "camera_grads", "contrib", "pixel_weights", "features", "distortion"))


def _parse_request(raster_settings, P: int, device, return_aux: bool = False, **render_options):
    """(the _Request, the four fixed trailing inputs of the autograd node) of one render of P Gaussians on `device`: the one place that reads
    `return_aux` and the keyword-only `antialiasing` (default False), `absgrad` (None), `camera_grads` (False), `contrib` (None),
    `pixel_weights` (None), `features` (None) and `distortion` (False).  GaussianRasterizer.forward / GaussianRasterizerRaw.forward take them through
    **render_options: those methods' keyword defaults (__kwdefaults__) are published as {"return_aux": False} alone.  In this order: an
    unknown keyword is a TypeError; a bad sink, bad weights, bad features or a `distortion` that is no bool a ValueError, before anything is
    launched; `return_aux`, `features` or `distortion` with a GradArena installed a RuntimeError.  The trailing inputs are (features, viewmatrix, projmatrix, campos), None where
    unused: the settings' three camera tensors once more, as differentiable inputs, if camera_grads is true and any of them requires grad --
    else the record's `camera` is False and the node, its arguments and its launches are the plain call's."""
    if not _RENDER_OPTIONS.issuperset(render_options):
        raise TypeError(f"forward() got an unexpected keyword argument {sorted(set(render_options) - _RENDER_OPTIONS)[0]!r}")
    get = render_options.get
    absgrad, contrib, pixel_weights, features = get("absgrad"), get("contrib"), get("pixel_weights"), get("features")
    if absgrad is not None:
        _C.check_absgrad(absgrad, P, device)
    _C.check_contrib(contrib, pixel_weights, P, int(raster_settings.image_height), int(raster_settings.image_width), device)
    if features is not None:
        _C.check_features(features, P, device)
        _C.no_arena_for_features()
    distortion = get("distortion", False)
    if not isinstance(distortion, bool):
        raise ValueError(f"distortion must be True or False (got {type(distortion).__name__})")
    if distortion:
        _C.no_arena_for_distortion()
    if return_aux:
        _no_arena_for_aux()
    cam = (raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.campos)
    camera = bool(get("camera_grads", False)) and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam)
    req = (_DistortionRequest if distortion else _Request)(bool(return_aux), bool(get("antialiasing", False)), absgrad, contrib, pixel_weights, camera)
    return req, (features,) + (cam if camera else (None, None, None))


def _after_forward(ctx, rs, req: _Request, features, state, *family_saved):
    """What both nodes do with what their family's _C.rasterize_gaussians* returned (`state`): the statistics and the feature map of the
    request, what the backward must remember, and the outputs (color, radii, depth[, acc_depth, alpha][, feature_map][, distort_map]).  Saved,
    in this fixed layout: radii, the three state buffers, features (None without), the distortion map's moments (None without), then the
    family's own tensors (None for an absent one)."""
    num_rendered, color, radii, geom_buf, bin_buf, img_buf, depth, *aux_out = state
    if req.contrib is not None:                # filled HERE, from the state the call above left: no backward is needed, none is affected
        _C.contrib_stats(req.contrib, req.pixel_weights, num_rendered, rs.image_width, rs.image_height, geom_buf, bin_buf, img_buf)
    # features: one more output, one more incoming gradient, one more saved tensor
    feat_out = () if features is None else (_C.features_forward(features, num_rendered, rs.image_width, rs.image_height, geom_buf, bin_buf, img_buf),)
    # distortion: one more output (the last), one more incoming gradient, one more saved tensor (the moments its backward reads)
    dist_out, moments = (), None
    if req.distortion:
        dmap, moments = _C.distortion_forward(int(radii.shape[0]), num_rendered, rs.image_width, rs.image_height, geom_buf, bin_buf, img_buf, color.device)
        dist_out = (dmap,)
    ctx.raster_settings, ctx.req, ctx.num_rendered = rs, req, num_rendered
    ctx.gs_options = _C.current_options()      # the backward runs on autograd's thread: it must use THIS thread's options
    ctx.gs_options["forward_only"] = int(not any(ctx.needs_input_grad))   # (a backward then cannot happen; kept consistent anyway)
    ctx.gs_backwards = 0                       # backwards run on this state (retain_graph): only the first finds zeroed records
    ctx.save_for_backward(radii, geom_buf, bin_buf, img_buf, features, moments, *family_saved)
    # depth stays "differentiable" as in the reference (REF:85-88: it is returned by the Function, its incoming gradient is ignored): a
    # loss built from depth alone runs a backward that yields zero gradients there, and does here (round 6; rounds 1-5 marked it
    # non-differentiable, which raised instead).  radii is int32: never differentiable.
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)     # no zero-filled [1,H,W] / [P] gradients for the two outputs nothing flows through
    return (color, radii, depth, *aux_out, *feat_out, *dist_out)


def _before_backward(ctx, grad_out_color, grad_aux: tuple):
    """What both nodes do in front of their family's _C.*_backward: (the colour's gradient, (radii, geom_buf, bin_buf, img_buf), the
    family's saved tensors, the call's keyword arguments) from the incoming gradients and the layout _after_forward saved."""
    req, rs = ctx.req, ctx.raster_settings
    radii, geom_buf, bin_buf, img_buf, features, moments, *family_saved = ctx.saved_tensors
    grad_aux, grad_dist = (grad_aux[:-1], grad_aux[-1]) if req.distortion else (grad_aux, None)           # (None = zero: today's call)
    grad_aux, grad_map = (grad_aux[:-1], grad_aux[-1]) if features is not None else (grad_aux, None)      # (None = zero: today's call)
    grad_acc_depth, grad_alpha = grad_aux or (None, None)      # (None = zero; both None: the plain backward)
    if grad_out_color is None:      # a loss that reaches this node through depth (or the aux outputs) only: the reference sees a zero colour gradient (REF:88)
        grad_out_color = torch.zeros((_C.NUM_CHANNELS, rs.image_height, rs.image_width), device=radii.device)
    kw = dict(options=ctx.gs_options, first_backward=ctx.gs_backwards == 0, dL_dacc_depth=grad_acc_depth, dL_dalpha=grad_alpha,
              antialiasing=req.antialiasing, absgrad=req.absgrad)
    if req.camera:                  # (without: the call is the plain one, as before the keyword existed)
        kw["camera_grads"] = True
    if grad_map is not None:
        kw["features"] = (features, grad_map)
    if grad_dist is not None:
        kw["distortion"] = (moments, grad_dist)
    return grad_out_color, (radii, geom_buf, bin_buf, img_buf), family_saved, kw


def _optional_grads(ctx, first: int, grad_features, grad_camera) -> tuple:
    """The node's gradients for its four fixed trailing inputs (input `first` onwards): dL_dfeatures or None, then each camera tensor's
    gradient in its own shape and dtype -- None for one that does not require grad, and for all three without req.camera."""
    rs = ctx.raster_settings
    if not ctx.req.camera:
        return (grad_features, None, None, None)
    return (grad_features,) + tuple(g.reshape(t.shape).to(t.dtype) if ctx.needs_input_grad[first + 1 + k] else None
                                    for k, (g, t) in enumerate(zip(grad_camera, (rs.viewmatrix, rs.projmatrix, rs.campos))))


class _RasterizeGaussians(torch.autograd.Function):
    """Opaque-state autograd node: forward saves the three state buffers the native library
    filled, backward hands them back (REF:42-132).  `req`: the render's _Request; behind it the four fixed optional differentiable
    inputs (_parse_request), None where unused."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, req, features, viewmatrix, projmatrix, campos):
        rs = raster_settings
        ar = _C._grad_arena
        if ar is not None and ar.sh_factors and sh.numel() != 0 and sh.requires_grad and not sh.is_leaf:
            # factor mode completes shs.grad later (sh_grad_combine writes the arena): that only reaches the parameters if
            # shs itself is the leaf.  cat(features_dc, features_rest) (get_features) would copy the unfinished buffer.
            raise RuntimeError("GradArena(sh_factors=True) needs the rasterizer's `shs` to be a leaf tensor; for "
                               "cat(features_dc, features_rest) or shs + residual use GradArena(sh_factors=False) + "
                               "view_parallel.allreduce_mean_inplace")
        state = _C.rasterize_gaussians(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
            rs.sh_degree, rs.campos, rs.prefiltered, forward_only=not any(ctx.needs_input_grad), aux=req.return_aux, antialiasing=req.antialiasing)
        # opacities are not saved: the state buffer keeps them next to the conic (REF:84)
        return _after_forward(ctx, rs, req, features, state, colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, _grad_depth, *grad_aux):
        rs = ctx.raster_settings
        grad_out_color, (radii, geom_buf, bin_buf, img_buf), (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh), kw = \
            _before_backward(ctx, grad_out_color, grad_aux)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
         grad_scales, grad_rotations, *more) = _C.rasterize_gaussians_backward(
            rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos,
            geom_buf, ctx.num_rendered, bin_buf, img_buf, **kw)
        ctx.gs_backwards += 1
        grad_features = more.pop() if "features" in kw else None
        # one gradient per forward input, in input order; absent optionals get None
        def opt(g, x):
            return g if x.numel() != 0 else None
        return (grad_means3D, grad_means2D, opt(grad_sh, sh), opt(grad_colors_precomp, colors_precomp),
                grad_opacities, opt(grad_scales, scales), opt(grad_rotations, rotations),
                opt(grad_cov3Ds_precomp, cov3Ds_precomp), None, None) + _optional_grads(ctx, 10, grad_features, more[0] if more else None)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, return_aux=False, *, antialiasing: bool = False, absgrad: Optional[torch.Tensor] = None,
                        camera_grads: bool = False, contrib: Optional[torch.Tensor] = None, pixel_weights: Optional[torch.Tensor] = None,
                        features: Optional[torch.Tensor] = None, distortion: bool = False):
    """Functional form (REF:17-39).  `return_aux` (not in the reference): also acc_depth and alpha; `antialiasing` (not in the
    reference): the opacity-compensated 2-D filter; `absgrad` (not in the reference): the [P,2] sink of the absolute screen-space
    gradient; `camera_grads` (not in the reference): gradients for raster_settings' viewmatrix / projmatrix / campos; `contrib` / `pixel_weights` (not in the reference): the
    [P,4] sink of the per-Gaussian blend-weight statistics, which the forward overwrites, and its per-pixel weights (module docstring);
    `features` (not in the reference): [P,C] per-Gaussian vectors, the result ends with their blend feature_map[C,H,W] (module docstring);
    `distortion` (not in the reference): the result ends with the depth-distortion map distort_map[H,W], behind feature_map (module docstring);
    `absgrad` stays a statistic of the colour and the aux outputs only."""
    req, optional = _parse_request(raster_settings, int(means3D.shape[0]), means3D.device, return_aux, antialiasing=antialiasing, absgrad=absgrad,
                                   camera_grads=camera_grads, contrib=contrib, pixel_weights=pixel_weights, features=features,
                                   distortion=distortion)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, req, *optional)


_EMPTY = torch.empty(0)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """bool[P]: Gaussians in front of the near plane (view-space z > 0.2)."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs: Optional[torch.Tensor] = None,
                colors_precomp: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                rotations: Optional[torch.Tensor] = None, cov3D_precomp: Optional[torch.Tensor] = None, *, return_aux: bool = False,
                **render_options):
        req, optional = _parse_request(self.raster_settings, int(means3D.shape[0]), means3D.device, return_aux, **render_options)
        have_sh, have_rgb = shs is not None, colors_precomp is not None
        if have_sh == have_rgb:
            raise Exception("Please provide exactly one of either SHs or precomputed colors!")
        have_sr = scales is not None or rotations is not None
        full_sr = scales is not None and rotations is not None
        have_cov = cov3D_precomp is not None
        if (not full_sr and not have_cov) or (have_sr and have_cov):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")

        empty = _EMPTY          # absent optional input, like the reference's torch.Tensor([]) (REF:173-183); one shared CPU tensor: nobody writes it
        return _RasterizeGaussians.apply(
            means3D, means2D,
            shs if have_sh else empty,
            colors_precomp if have_rgb else empty,
            opacities,
            scales if scales is not None else empty,
            rotations if rotations is not None else empty,
            cov3D_precomp if have_cov else empty,
            self.raster_settings, req, *optional)

    # Introspection shows the reference's signature (REF:163-165: drop-in callers -- and tests/test_api_host.py -- compare it);
    # return_aux is this package's keyword-only extension, default False (forward.__kwdefaults__), and so are antialiasing, absgrad,
    # camera_grads, contrib, pixel_weights, features and distortion, which arrive through **render_options (names and defaults: _parse_request).
    forward.__signature__ = inspect.Signature([q for q in inspect.signature(forward).parameters.values()
                                               if q.name not in ("return_aux", "render_options")])


# ---- which Gaussians a pixel sees (no counterpart in the reference; include/gsrast.h: gsrast_pixel_contributors) ---------------------------
class PixelContributors(NamedTuple):
    """What pixel_contributors returns; every tensor is detached."""
    ids: torch.Tensor          # [K,H,W] int32: rows of the inputs, -1 in an unused slot
    weights: torch.Tensor      # [K,H,W] float32: alpha T of the pair, +0.0 in an unused slot
    count: torch.Tensor        # [H,W] int32: all of the pixel's contributors, also those beyond K
    color: torch.Tensor        # [3,H,W], depth [1,H,W], radii [P] int32: the render the query ran on
    depth: torch.Tensor
    radii: torch.Tensor


def _check_query_inputs(given: list, device) -> None:
    """pixel_contributors' own ladder over (name, tensor, shapes): every one a float32 tensor in one of its `shapes` (None: any extent), then
    every one on `device`, a GPU; ValueError otherwise."""
    for name, t, shapes in given:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"pixel_contributors: {name} must be a tensor (got {type(t).__name__})")
        if not any(len(s) == t.ndim and all(w is None or w == int(n) for w, n in zip(s, t.shape)) for s in shapes):
            want = " or ".join("[" + ", ".join("M" if w is None else str(w) for w in s) + "]" for s in shapes)
            raise ValueError(f"pixel_contributors: {name} must be {want} (got {list(t.shape)})")
        if t.dtype is not torch.float32:
            raise ValueError(f"pixel_contributors: {name} must be float32 (got {t.dtype})")
    for name, t, _ in given:
        if not t.is_cuda:
            raise ValueError(f"pixel_contributors: {name} must live on a GPU (got {t.device}): there is no CPU fallback")
        if t.device != device:
            raise ValueError(f"pixel_contributors: {name} must live on {device} (got {t.device})")


def pixel_contributors(means3D, opacities, scales=None, rotations=None, *, raster_settings, K: int = 8, order: str = "weight",
                       shs=None, colors_precomp=None, cov3D_precomp=None, antialiasing: bool = False) -> PixelContributors:
    """Which Gaussians each pixel sees, and with what weight: PixelContributors(ids [K,H,W] int32, weights [K,H,W], count [H,W] int32,
    color, depth, radii) of one view (gsplat's rasterize_to_indices_in_range, the per-pixel id output many forks of the reference add):
    picking the Gaussian under a cursor, finding the floater that spoils a pixel, lifting 2-D masks or labels by vote, visibility lists.

    A pair (pixel, Gaussian) contributes as defined under ``contrib`` in the module docstring; its weight is w = alpha T with the opacity
    the render used (anti-aliasing compensation included).  ``count`` is the number of a pixel's contributors.  ``order="weight"``: slots
    0 .. min(K, count) - 1 hold the contributors with the largest w, descending, on equal w the one earlier in blend order first -- slot 0
    is the Gaussian ``contrib``'s top_count counts for the pixel.  ``order="depth"``: the slots hold the first min(K, count) contributors
    in blend order (front to back).  Unused slots hold id -1 and weight +0.0; ids are rows of the inputs; 1 <= K <= 16.

    The call runs one forward-only render under ``torch.no_grad()`` -- of ``shs`` or ``colors_precomp`` if one is given (the returned
    colour is then a plain forward's), else of zero colours -- and the query on its state.  Inputs that require grad are accepted; nothing
    is differentiable and every output is detached; a ``GradArena`` may be installed.  The result is bit-identical from run to run.
    ``ValueError`` before any launch: a K outside 1..16, an order other than "weight" / "depth", a tensor on the CPU, a wrong shape or dtype,
    both or neither of (scales, rotations) and cov3D_precomp, both shs and colors_precomp."""
    rs = raster_settings
    _C.check_pixel_contributors(K, order)
    if not isinstance(means3D, torch.Tensor) or means3D.ndim != 2 or means3D.shape[1] != 3:
        raise ValueError("pixel_contributors: means3D must be a [P, 3] tensor")
    P, dev = int(means3D.shape[0]), means3D.device
    H, W = int(rs.image_height), int(rs.image_width)
    if H <= 0 or W <= 0:
        raise ValueError(f"pixel_contributors: the image must not be empty (got {W} x {H})")
    if (scales is None) != (rotations is None) or (scales is None) == (cov3D_precomp is None):
        raise ValueError("pixel_contributors: give exactly one of the (scales, rotations) pair and cov3D_precomp")
    if shs is not None and colors_precomp is not None:
        raise ValueError("pixel_contributors: give at most one of shs and colors_precomp")
    given = [("means3D", means3D, ((P, 3),)), ("opacities", opacities, ((P, 1), (P,))), ("scales", scales, ((P, 3),)), ("rotations", rotations, ((P, 4),)),
             ("cov3D_precomp", cov3D_precomp, ((P, 6),)), ("shs", shs, ((P, None, 3),)), ("colors_precomp", colors_precomp, ((P, 3),)),
             ("raster_settings.bg", rs.bg, ((3,),)), ("raster_settings.viewmatrix", rs.viewmatrix, ((4, 4),)),
             ("raster_settings.projmatrix", rs.projmatrix, ((4, 4),)), ("raster_settings.campos", rs.campos, ((3,), (1, 3)))]
    _check_query_inputs([g for g in given if g[1] is not None or g[0] in ("means3D", "opacities")], dev)
    with torch.no_grad():
        det = lambda t: _EMPTY if t is None else t.detach()      # noqa: E731  (absent optional input: GaussianRasterizer.forward's)
        colors = torch.zeros((P, 3), dtype=torch.float32, device=dev) if shs is None and colors_precomp is None else det(colors_precomp)
        num_rendered, color, radii, geom_buf, bin_buf, img_buf, depth = _C.rasterize_gaussians(
            rs.bg, means3D.detach(), colors, opacities.detach().reshape(P, 1), det(scales), det(rotations), rs.scale_modifier, det(cov3D_precomp),
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, det(shs), rs.sh_degree, rs.campos, rs.prefiltered,
            forward_only=True, antialiasing=bool(antialiasing))
        ids, weights, count = _C.pixel_contributors(K, order, num_rendered, W, H, geom_buf, bin_buf, img_buf, P=P)
    return PixelContributors(ids, weights, count, color, depth, radii)


# ---- raw-parameter module (no counterpart in the reference: SURVEY.md 8f rank 3 as written -- the activation / deformation epilogue
# of scene/saro_gaussian.py:807-847 fused into the per-Gaussian kernels) -------------------------------------------------------------
class _RasterizeGaussiansRaw(torch.autograd.Function):
    """means2D (the gradient sink of REF:42) + the settings + the render's _Request + the inputs in _C.RAW_NAMES order (absent residuals:
    None) + the four fixed optional differentiable inputs, as _RasterizeGaussians."""

    @staticmethod
    def forward(ctx, means2D, raster_settings, req, *inputs):
        *raw_tensors, features, viewmatrix, projmatrix, campos = inputs
        rs = raster_settings
        state = _C.rasterize_gaussians_raw(
            rs.bg, dict(zip(_C.RAW_NAMES, raw_tensors)), rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width,
            rs.sh_degree, rs.campos, forward_only=not any(ctx.needs_input_grad), aux=req.return_aux, antialiasing=req.antialiasing)
        return _after_forward(ctx, rs, req, features, state, *raw_tensors)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, _grad_depth, *grad_aux):
        rs = ctx.raster_settings
        grad_out_color, (radii, geom_buf, bin_buf, img_buf), raw_tensors, kw = _before_backward(ctx, grad_out_color, grad_aux)
        raw = dict(zip(_C.RAW_NAMES, raw_tensors))
        g = _C.rasterize_gaussians_raw_backward(
            rs.bg, raw, radii, rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, rs.sh_degree,
            rs.campos, geom_buf, ctx.num_rendered, bin_buf, img_buf, **kw)
        ctx.gs_backwards += 1
        grads = tuple(None if raw[n] is None else g[n].reshape(raw[n].shape) if g[n].is_contiguous() else g[n] for n in _C.RAW_NAMES)
        return (g["dL_dmeans2D"], None, None) + grads + _optional_grads(ctx, 3 + len(_C.RAW_NAMES), g.get("features"), g.get("camera"))


class GaussianRasterizerRaw(nn.Module):
    """GaussianRasterizer for callers that hold SaRO-GS's RAW parameters: forward(xyz, means2D, rotation, scaling, opacity, features_dc,
    features_rest, motion_residual=None, rot_residual=None, trbfoutput=None, shs_residual=None) renders
    means3D = xyz + motion_residual, rotations = normalize(rotation + rot_residual[:, :4]), scales = exp(scaling + rot_residual[:, 4:]),
    opacities = sigmoid(opacity) * trbfoutput, shs = cat(features_dc, features_rest) + shs_residual (scene/saro_gaussian.py:807-847) --
    outputs bit-identical to fused_epilogue.activate_gaussians followed by GaussianRasterizer, without the activated tensors ever
    being written.  Gradients flow to every tensor given.  `return_aux=True`: (color, radii, depth, acc_depth, alpha), and the keyword-only
    `antialiasing=True` (default False), `absgrad=sink` (default None), `camera_grads=True` (default False), `contrib=sink` and `pixel_weights=w` (default None), `features=F` (default None), `distortion=True` (default False), as GaussianRasterizer."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, xyz, means2D, rotation, scaling, opacity, features_dc, features_rest, motion_residual=None, rot_residual=None,
                trbfoutput=None, shs_residual=None, *, return_aux: bool = False, **render_options):
        req, optional = _parse_request(self.raster_settings, int(xyz.shape[0]), xyz.device, return_aux, **render_options)
        raw = dict(xyz=xyz, motion_res=motion_residual, rotation=rotation, rot_res=rot_residual, scaling=scaling, opacity_logit=opacity,
                   trbf=trbfoutput, features_dc=features_dc, features_rest=features_rest, shs_res=shs_residual)
        return _RasterizeGaussiansRaw.apply(means2D, self.raster_settings, req, *[raw[n] for n in _C.RAW_NAMES], *optional)
