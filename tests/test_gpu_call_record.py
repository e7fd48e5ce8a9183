"""-m gpu: the call records of the C ABI (include/gsrast.h: gsrast_render_forward / gsrast_render_backward) driven directly through
ctypes, beside the positional gsrast_forward / gsrast_backward and the Python package, on one small scene: P = 3 000 at 150 x 100 --
neither extent a multiple of the 16-pixel tile, so partial tiles and the last column of tiles are exercised --, SH degree 3.

Forwards are compared bit for bit.  The blend backward accumulates with float atomics, so no two backwards agree to the last bit: every
comparison of gradients is `_close(got, base, floor=base2)` of tests/test_gpu_render_antialias.py, base and base2 being two runs of
the SAME call -- the floor is measured, no tolerance is fixed in advance."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_render_antialias import _bits, _close, _t

pytestmark = pytest.mark.gpu

P, W, H, D, M = 3000, 150, 100, 3, 16
SIZES = ("min", "abs", "full")


class _State:
    """Allocation callbacks over three growing device buffers, poisoned (the library must not depend on what a buffer held)."""

    def __init__(self, _C, dev):
        self.dev, self.held = dev, [None, None, None]
        self.cbs = [_C._ALLOC_FN(self._make(k)) for k in range(3)]

    def _make(self, k):
        def alloc(_ctx, nbytes):
            self.held[k] = torch.full((int(nbytes),), 255, dtype=torch.uint8, device=self.dev)
            return self.held[k].data_ptr()
        return alloc


@pytest.fixture(scope="module")
def case(scenes, rast, gpu):
    """The scene's tensors (dense and raw leaves of the same Gaussians), the camera, the upstream gradients, and the record sizes."""
    _C = rast._C
    sc, cam = scenes.synth(P, 77), scenes.camera(1, 8, W, H)
    rng = np.random.default_rng(78)
    d = {k: _t(sc[k], gpu) for k in ("means3D", "shs", "opacities", "scales", "rotations", "bg")}
    d.update(view=_t(cam["viewmatrix"], gpu), proj=_t(cam["projmatrix"], gpu), campos=_t(cam["campos"], gpu),
             dpix=_t(scenes.upstream_grad(H, W, 79), gpu), dacc=_t(rng.normal(size=(1, H, W)) / (H * W), gpu), dalpha=_t(rng.normal(size=(1, H, W)) / (H * W), gpu))
    raw = dict(xyz=d["means3D"], rotation=d["rotations"], scaling=d["scales"].log(), opacity_logit=torch.logit(d["opacities"]),
               features_dc=d["shs"][:, :1].contiguous(), features_rest=d["shs"][:, 1:].contiguous())
    B = _C.BackwardCallStruct
    sizes = dict(min=B.dL_dmean2D_abs.offset, abs=B.dL_dcamera.offset, full=C.sizeof(B))
    return dict(_C=_C, L=_C.lib(), dev=gpu, d=d, raw=raw, tan=(float(cam["tanfovx"]), float(cam["tanfovy"])), sizes=sizes, stream=_C._stream_of(gpu))


def _p(x):
    return None if x is None else x.data_ptr()


def _forward_record(c, family, flags=0, aux=False):
    """gsrast_render_forward on a record of `family`: (R, color, depth, radii, the state, acc_depth, alpha)."""
    _C, d, dev = c["_C"], c["d"], c["dev"]
    color, depth = torch.full((3, H, W), -1.0, device=dev), torch.full((1, H, W), -1.0, device=dev)
    radii = torch.full((P,), -1, dtype=torch.int32, device=dev)
    acc, alpha = (torch.full((1, H, W), -1.0, device=dev), torch.full((1, H, W), -1.0, device=dev)) if aux else (None, None)
    st = _State(_C, dev)
    rec = _C.ForwardCallStruct(struct_size=C.sizeof(_C.ForwardCallStruct), flags=flags, geometry_alloc=st.cbs[0], binning_alloc=st.cbs[1], image_alloc=st.cbs[2],
                               P=P, D=D, M=M, background=_p(d["bg"]), width=W, height=H, scale_modifier=1.0, viewmatrix=_p(d["view"]), projmatrix=_p(d["proj"]),
                               cam_pos=_p(d["campos"]), tan_fovx=c["tan"][0], tan_fovy=c["tan"][1], out_color=_p(color), out_depth=_p(depth), radii=_p(radii),
                               stream=c["stream"], out_acc_depth=_p(acc), out_alpha=_p(alpha))
    if family == "raw":
        ins = _C.RawInputsStruct(**{k: _p(v) for k, v in c["raw"].items()})
        rec.family, rec.raw = _C.FAMILY_RAW, C.pointer(ins)
    else:
        rec.family = _C.FAMILY_DENSE
        rec.means3D, rec.shs, rec.opacities, rec.scales, rec.rotations = (_p(d[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations"))
    R = c["L"].gsrast_render_forward(None, None, C.byref(rec))
    torch.cuda.synchronize()
    assert R > 0, c["L"].gsrast_last_error()
    return R, color, depth, radii, st.held, acc, alpha


def _forward_positional(c):
    _C, d, dev = c["_C"], c["d"], c["dev"]
    color, depth = torch.full((3, H, W), -1.0, device=dev), torch.full((1, H, W), -1.0, device=dev)
    radii = torch.full((P,), -1, dtype=torch.int32, device=dev)
    st = _State(_C, dev)
    R = c["L"].gsrast_forward(st.cbs[0], None, st.cbs[1], None, st.cbs[2], None, P, D, M, _p(d["bg"]), W, H, _p(d["means3D"]), _p(d["shs"]), None,
                              _p(d["opacities"]), _p(d["scales"]), 1.0, _p(d["rotations"]), None, _p(d["view"]), _p(d["proj"]), _p(d["campos"]),
                              c["tan"][0], c["tan"][1], 0, _p(color), _p(depth), _p(radii), c["stream"])
    torch.cuda.synchronize()
    assert R > 0, c["L"].gsrast_last_error()
    return R, color, depth, radii, st.held


def _same_forward(got, want, what):
    """(R, color, depth, radii[, acc, alpha]) bit for bit."""
    assert got[0] == want[0], what
    for k in range(1, len(want)):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


DENSE_OUT = dict(dL_dmean2D=(P, 3), dL_dopacity=(P, 1), dL_dmean3D=(P, 3), dL_dsh=(P, M, 3), dL_dscale=(P, 3), dL_drot=(P, 4))
RAW_OUT = dict(dL_dmean2D=(P, 3), d_xyz=(P, 3), d_rotation=(P, 4), d_scaling=(P, 3), d_opacity_logit=(P, 1), d_features_dc=(P, 1, 3), d_features_rest=(P, M - 1, 3))


def _backward_record(c, family, size, R, radii, state, flags=0, **sinks):
    """gsrast_render_backward on a record of `family` truncated to `size`; every output poisoned first.  sinks: further fields by name."""
    _C, d, dev = c["_C"], c["d"], c["dev"]
    out = {k: torch.full(s, 7.0, device=dev) for k, s in (RAW_OUT if family == "raw" else DENSE_OUT).items()}
    rec = _C.BackwardCallStruct(struct_size=c["sizes"][size], flags=flags, P=P, D=D, M=M, R=R, background=_p(d["bg"]), width=W, height=H, scale_modifier=1.0,
                                viewmatrix=_p(d["view"]), projmatrix=_p(d["proj"]), campos=_p(d["campos"]), tan_fovx=c["tan"][0], tan_fovy=c["tan"][1],
                                radii=_p(radii), geom_buffer=_p(state[0]), binning_buffer=_p(state[1]), image_buffer=_p(state[2]), dL_dpix=_p(d["dpix"]),
                                stream=c["stream"], **{k: _p(v) for k, v in sinks.items()})
    if family == "raw":
        ins = _C.RawInputsStruct(**{k: _p(v) for k, v in c["raw"].items()})
        gr = _C.RawGradsStruct(**{k: _p(v) for k, v in out.items()})
        rec.family, rec.raw, rec.raw_grads = _C.FAMILY_RAW, C.pointer(ins), C.pointer(gr)
    else:
        rec.family = _C.FAMILY_DENSE
        rec.means3D, rec.shs, rec.scales, rec.rotations = (_p(d[k]) for k in ("means3D", "shs", "scales", "rotations"))
        for k, v in out.items():
            setattr(rec, k, _p(v))
    rc = c["L"].gsrast_render_backward(None, C.byref(rec))
    torch.cuda.synchronize()
    assert rc == 0, c["L"].gsrast_last_error()
    return out


def _backward_positional(c, R, radii, state):
    d, dev = c["d"], c["dev"]
    o = {k: torch.full(s, 7.0, device=dev) for k, s in DENSE_OUT.items()}
    rc = c["L"].gsrast_backward(P, D, M, R, _p(d["bg"]), W, H, _p(d["means3D"]), _p(d["shs"]), None, _p(d["scales"]), 1.0, _p(d["rotations"]), None,
                                _p(d["view"]), _p(d["proj"]), _p(d["campos"]), c["tan"][0], c["tan"][1], _p(radii), _p(state[0]), _p(state[1]), _p(state[2]),
                                _p(d["dpix"]), _p(o["dL_dmean2D"]), None, _p(o["dL_dopacity"]), None, _p(o["dL_dmean3D"]), None, _p(o["dL_dsh"]),
                                _p(o["dL_dscale"]), _p(o["dL_drot"]), c["stream"])
    torch.cuda.synchronize()
    assert rc == 0, c["L"].gsrast_last_error()
    return o


def _package_forward(c, **kw):
    _C, d = c["_C"], c["d"]
    e = torch.empty(0, device=c["dev"])
    out = _C.rasterize_gaussians(d["bg"], d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e, d["view"], d["proj"], c["tan"][0], c["tan"][1],
                                 H, W, d["shs"], D, d["campos"], False, **kw)
    torch.cuda.synchronize()
    return out      # (R, color, radii, geom, binning, img, depth[, acc, alpha])


def test_dense_records_are_the_positional_calls_and_the_package(case):
    c = case
    pos, rec, pkg = _forward_positional(c), _forward_record(c, "dense"), _package_forward(c)
    _same_forward(rec[:4], pos[:4], "record vs gsrast_forward")
    _same_forward((pkg[0], pkg[1], pkg[6], pkg[2]), pos[:4], "rasterize_gaussians vs gsrast_forward")
    assert float(pos[1].abs().max()) > 0 and int((pos[3] > 0).sum()) > P // 2      # (something was rendered)
    R, radii, state = pos[0], pos[3], pos[4]
    base, base2 = _backward_positional(c, R, radii, state), _backward_positional(c, R, radii, state)
    for size in SIZES:
        got = _backward_record(c, "dense", size, R, radii, state)
        for k in DENSE_OUT:
            assert float(base[k].abs().max()) > 0, k
            _close(got[k], base[k], floor=base2[k].double().cpu().numpy(), what=(size, k))


def test_raw_records_are_the_package(case):
    c = case
    _C, d = c["_C"], c["d"]
    pkg = _C.rasterize_gaussians_raw(d["bg"], c["raw"], 1.0, d["view"], d["proj"], c["tan"][0], c["tan"][1], H, W, D, d["campos"])
    torch.cuda.synchronize()
    rec = _forward_record(c, "raw")
    _same_forward(rec[:4], (pkg[0], pkg[1], pkg[6], pkg[2]), "raw record vs rasterize_gaussians_raw")
    R, radii, state = pkg[0], pkg[2], (pkg[3], pkg[4], pkg[5])

    def package():
        g = _C.rasterize_gaussians_raw_backward(d["bg"], c["raw"], radii, 1.0, d["view"], d["proj"], c["tan"][0], c["tan"][1], d["dpix"], D, d["campos"],
                                                state[0], R, state[1], state[2])
        torch.cuda.synchronize()
        return g

    base, base2 = package(), package()
    names = dict(dL_dmean2D="dL_dmeans2D", d_xyz="xyz", d_rotation="rotation", d_scaling="scaling", d_opacity_logit="opacity_logit",
                 d_features_dc="features_dc", d_features_rest="features_rest")
    for size in SIZES:
        got = _backward_record(c, "raw", size, R, radii, state)
        for k, n in names.items():
            assert float(base[n].abs().max()) > 0, n
            _close(got[k], base[n], floor=base2[n].double().cpu().numpy(), what=(size, k))


def test_a_full_record_with_every_feature_is_the_package_with_the_same_switches(case):
    """AUX | ANTIALIAS | ABSGRAD | POSEGRAD on one full record (the forward takes the first two) against aux=True, antialiasing=True,
    absgrad=, camera_grads=True of the package.  The floor of every gradient is measured on two runs of the package's own call with these
    switches (the positional pair, which has none of them, measures nothing here)."""
    c = case
    _C, d, dev = c["_C"], c["d"], c["dev"]
    flags = _C.RENDER_AUX | _C.RENDER_ANTIALIAS
    pkg = _package_forward(c, aux=True, antialiasing=True)
    rec = _forward_record(c, "dense", flags, aux=True)
    _same_forward(rec[:4] + rec[5:], (pkg[0], pkg[1], pkg[6], pkg[2], pkg[7], pkg[8]), "full forward record vs the package")
    R, radii, state = pkg[0], pkg[2], (pkg[3], pkg[4], pkg[5])
    e = torch.empty(0, device=dev)

    def package():
        sink = torch.full((P, 2), 7.0, device=dev)
        g = _C.rasterize_gaussians_backward(d["bg"], d["means3D"], radii, e, d["scales"], d["rotations"], 1.0, e, d["view"], d["proj"], c["tan"][0], c["tan"][1],
                                            d["dpix"], d["shs"], D, d["campos"], state[0], R, state[1], state[2], dL_dacc_depth=d["dacc"], dL_dalpha=d["dalpha"],
                                            antialiasing=True, absgrad=sink, camera_grads=True)
        torch.cuda.synchronize()
        return dict(dL_dmean2D=g[0], dL_dopacity=g[2], dL_dmean3D=g[3], dL_dsh=g[5], dL_dscale=g[6], dL_drot=g[7], absgrad=sink, camera=torch.cat([x.reshape(-1) for x in g[8]]))

    base, base2 = package(), package()
    sink, camera = torch.full((P, 2), 7.0, device=dev), torch.full((_C.CAMERA_FLOATS,), 7.0, device=dev)
    scratch = torch.empty((int(c["L"].gsrast_pose_scratch_bytes(P)),), dtype=torch.uint8, device=dev)
    got = _backward_record(c, "dense", "full", R, radii, state, flags | _C.RENDER_ABSGRAD | _C.RENDER_POSEGRAD, dL_dacc_depth=d["dacc"], dL_dalpha=d["dalpha"],
                           dL_dmean2D_abs=sink, dL_dcamera=camera, pose_scratch=scratch)
    got.update(absgrad=sink, camera=camera)
    for k in base:
        assert float(base[k].abs().max()) > 0, k
        _close(got[k], base[k], floor=base2[k].double().cpu().numpy(), what=k)
