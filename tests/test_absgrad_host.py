"""CPU: the absolute screen-space gradient (include/gsrast.h: GSRAST_RENDER_ABSGRAD, dL_dmean2D_abs of gsrast_backward_call;
`absgrad=` of the Python package) -- the fp64 reference of tests/absgrad_math.py checks itself, the backward records refuse bad
arguments before any device work, the package refuses a bad sink at forward time, and the densification plumbing
(view_parallel.distributed_step, fused_densify.DensifyStats.update) carries the statistic.  (The records' layout and the flag values:
tests/test_capi_abi.py.)"""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import absgrad_math as am
import capi_records as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c", "d"])
def test_reference_self_check(name):
    """absgrad_of asserts that the per-pixel gradients add up to the gradient of the whole loss (1e-12); here also: the statistic
    dominates the signed gradient, is zero exactly where nothing is rendered, and the case stays under the ambiguity cap."""
    r = am.reference(name)
    a, s = r["abs"], np.abs(r["signed"])
    assert r["amb"].mean() < 0.05
    assert (a >= s * (1.0 - 1e-12)).all() and float(a.max()) > 0.0
    vis = r["out"]["proj"]["disc"]["vis"]
    assert not a[~vis].any()
    assert ((a[vis] > 2.0 * s[vis]).any(axis=1)).mean() > 0.1      # not the signed gradient with its sign dropped
    if r["c"].get("long"):
        assert r["out"]["tile_list_max"] > 128 and not r["out"]["stopped"].any()      # every pixel walks the whole list


def test_symmetric_gaussian_has_no_signed_gradient_but_an_absolute_one(scenes):
    """One isotropic Gaussian whose centre projects onto the centre of pixel (8, 8) of a 16 x 16 image, constant upstream gradient: a 2-D
    Gaussian is point-symmetric about its centre and so is the pixel grid about a pixel centre, so the pixels' pulls cancel in the signed
    sum -- the blind spot the statistic exists for."""
    W = H = 16
    cam = scenes.camera(0, 4, W, H)
    z = 4.0
    ndc = (2.0 * 8.0 + 1.0) / W - 1.0                      # pixel = ((ndc + 1) * W - 1) / 2 = 8
    view = np.array([[ndc * am.mr.F32(cam["tanfovx"]) * z, ndc * am.mr.F32(cam["tanfovy"]) * z, z, 1.0]])
    Vi = np.linalg.inv(cam["viewmatrix"].astype(np.float64))
    one3, q0 = np.full((1, 3), 0.12), np.array([[1.0, 0.0, 0.0, 0.0]])
    for _ in range(4):      # (the projection matrix has fp32 entries and p_w = 1 / (w + 1e-7): a few Newton steps put the centre ON the pixel's)
        world = (view @ Vi)[:, :3]
        pix = am.mr.project(am.t64(world), am.t64(one3), am.t64(q0), cam)["pix"].numpy()[0]
        view[0, 0] -= (pix[0] - 8.0) * z * 2.0 * am.mr.F32(cam["tanfovx"]) / W
        view[0, 1] -= (pix[1] - 8.0) * z * 2.0 * am.mr.F32(cam["tanfovy"]) / H
    sc = dict(means3D=world, scales=one3, rotations=q0, opacities=np.array([[0.7]]),
              shs=np.full((1, 16, 3), 0.0), bg=np.array([0.1, 0.2, 0.3], np.float32), sh_degree=0)
    sc["shs"][0, 0] = (0.9, -0.3, 0.5)
    c = dict(W=W, H=H, seed=0)
    r = am.absgrad_of(sc, cam, c, upstream_fn=lambda c, amb: (np.ones((3, H, W), np.float32), None, None))
    pix = r["out"]["proj"]["pix"].detach().numpy()[0]
    assert np.abs(pix - 8.0).max() < 1e-12 and r["out"]["n_live"].max() == 1 and (r["out"]["n_live"] > 0).sum() >= 9
    assert r["amb"].sum() <= 1 and r["amb"][8, 8] == r["amb"].any()      # (power = 0 at the centre pixel, whose gradient is zero: no fp32 side here)
    assert (r["abs"][0] > 0.0).all()
    assert (np.abs(r["signed"][0]) <= 1e-9 * r["abs"][0]).all(), (r["signed"], r["abs"])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_fail_before_any_device_work(L, rast):
    _C = rast._C
    one = cr.ONE
    AUX, AA, ABS = _C.RENDER_AUX, _C.RENDER_ANTIALIAS, _C.RENDER_ABSGRAD
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))

    def call(family, size, P, flags, sink=None):      # size "abs": the record truncated just behind the sink; "min": a record without it
        return cr.call(cr.backward(P, flags, family, size=size, dL_dmean2D_abs=sink), opts)

    for family in ("dense", "raw"):
        for fl in (ABS, ABS | AA):
            # the bit with a NULL sink
            rc, err = call(family, "abs", 10, fl)
            assert rc == -1 and b"NULL dL_dmean2D_abs" in err
            # the bit on a record that has no sink: an unknown bit there
            rc, err = call(family, "min", 10, fl)
            assert rc == -1 and b"unknown bits" in err and b"dL_dmean2D_abs" in err
        # a sink without the bit
        for fl in (0, AA):
            rc, err = call(family, "abs", 10, fl, one)
            assert rc == -1 and b"without GSRAST_RENDER_ABSGRAD" in err
        # unknown bits stay unknown on the longer record
        rc, err = call(family, "abs", 10, ABS | 0x8, one)
        assert rc == -1 and b"unknown bits" in err
        # the bit where the transposed blend backward would not run: cull = 0 (GSRAST_RENDER_AUX's rule), the ablation kernels
        opts.cull = 0
        rc, err = call(family, "abs", 10, ABS, one)
        assert rc == -1 and b"transposed" in err and b"cull" in err
        L.gsrast_options_init(C.byref(opts))
        for abl in (1, 2):
            _C.set_option("ablate", abl)
            try:
                rc, err = call(family, "abs", 10, ABS, one)
                assert rc == -1 and b"transposed" in err
            finally:
                _C.set_option("ablate", 0)
        # a good combination reaches the ordinary checks (here: the negative P), with and without the bit
        rc, err = call(family, "abs", -1, ABS, one)
        assert rc == -1 and b"ABSGRAD" not in err and b"unknown bits" not in err
        rc, err = call(family, "abs", -1, 0)
        assert rc == -1 and b"ABSGRAD" not in err
        # P = 0: nothing to do, no device touched
        assert call(family, "abs", 0, ABS, one)[0] == 0
    # the forward has no use for the bit: mask it off (include/gsrast.h)
    rc, err = cr.call(cr.forward(10, ABS), opts)
    assert rc == -1 and b"unknown bits" in err


def test_backward_plan_takes_the_transposed_kernel_only_for_the_new_symbols(L, rast):
    """gsrast_debug_backward_plan (without 32 in words[5]) stands for a record without a sink: it refuses the bit, and plans every other call as before."""
    _C = rast._C
    opts = _C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    fn = C.CDLL(_C.LIB_PATH).gsrast_debug_backward_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(_C.OptionsStruct), C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    words = (C.c_int * 7)(1000, 3, 5000, 64, 64, 2, 1)
    assert fn(C.byref(opts), 0, words, None) >= 0
    assert fn(C.byref(opts), _C.RENDER_ABSGRAD, words, None) == -1 and b"unknown bits" in L.gsrast_last_error()


# ---- the Python package -------------------------------------------------------------------------------------------------------------
def test_python_refuses_a_bad_sink_at_forward_time(rast):
    _C = rast._C
    P, cpu = 7, torch.device("cpu")
    good = torch.zeros((P, 2))
    _C.check_absgrad(None, P, cpu)
    _C.check_absgrad(good, P, cpu)
    bad = dict(shape=torch.zeros((P, 3)), rows=torch.zeros((P + 1, 2)), flat=torch.zeros(P * 2), dtype=torch.zeros((P, 2), dtype=torch.float64),
               layout=torch.zeros((2, P)).T, device=torch.zeros((P, 2), device="meta"), grad=torch.zeros((P, 2), requires_grad=True), kind=[0.0] * P)
    for what, t in bad.items():
        with pytest.raises(ValueError, match="absgrad"):
            _C.check_absgrad(t, P, cpu)
    # through the public entry points: ValueError before anything is rendered (no GPU here)
    rs = rast.GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    m3, m2, op = torch.zeros((P, 3)), torch.zeros((P, 3)), torch.zeros((P, 1))
    e = torch.empty(0)
    for what in ("shape", "dtype", "layout"):
        with pytest.raises(ValueError, match="absgrad"):
            rast.rasterize_gaussians(m3, m2, e, torch.zeros((P, 3)), op, torch.ones((P, 3)), torch.ones((P, 4)), e, rs, absgrad=bad[what])
        with pytest.raises(ValueError, match="absgrad"):
            rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)),
                                        absgrad=bad[what])
        with pytest.raises(ValueError, match="absgrad"):
            rast.GaussianRasterizerRaw(rs)(m3, m2, torch.ones((P, 4)), torch.zeros((P, 3)), op, torch.zeros((P, 1, 3)), torch.zeros((P, 15, 3)),
                                           absgrad=bad[what])
    # the published keyword defaults do not move, and an unknown keyword is still a TypeError
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):
        assert fn.__kwdefaults__ == {"return_aux": False}
    with pytest.raises(TypeError):
        rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), abs_grad=good)
    assert rast._parse_request(rs, P, cpu)[0].absgrad is None and rast._parse_request(rs, P, cpu, absgrad=good)[0].absgrad is good


# ---- densification plumbing ---------------------------------------------------------------------------------------------------------
def test_densify_stats_key_handling():
    import fused_densify
    P = 5
    st = fused_densify.DensifyStats(P, "cpu")
    base = dict(visibility_count=torch.ones(P), radii=torch.ones(P))
    with pytest.raises(KeyError, match="viewspace_point_absgrad"):
        st.update(dict(base, viewspace_point_grad=torch.ones((P, 1))), use_absgrad=True)
    with pytest.raises(KeyError, match="viewspace_point_grad"):
        st.update(dict(base, viewspace_point_absgrad=torch.ones((P, 1))))
    # the right key is found: the call gets as far as the device check (no GPU in this test)
    for kw, step in ((dict(use_absgrad=True), dict(base, viewspace_point_absgrad=torch.ones((P, 1)))),
                     (dict(), dict(base, viewspace_point_grad=torch.ones((P, 1)), viewspace_point_absgrad=torch.ones((P, 1))))):
        with pytest.raises(RuntimeError, match="GPU"):
            st.update(step, **kw)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Model(torch.nn.Module):
    """A smooth stand-in for model + renderer (no rasterizer on the CPU): what is under test is distributed_step's bookkeeping, which
    never looks inside the render.  The "rasterizer" fills the view's absgrad sink when its backward runs, as the real one does."""

    def __init__(self, P):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.xyz = torch.nn.Parameter(torch.randn(P, 3, generator=g))

    def render_loss(self, k, with_absgrad=True):
        P = self.xyz.shape[0]
        means2D = torch.zeros((P, 3), requires_grad=True)
        vis = (self.xyz[:, 2].detach() + 0.2 * k) > -0.3
        screen = self.xyz[:, :2] * (1.0 + 0.1 * k) + means2D[:, :2]
        loss = (torch.sin(screen * (k + 1)).sum(1) * vis).sum() / P
        out = {"loss": loss, "viewspace_points": means2D, "visibility_filter": vis, "radii": (vis * (k + 2)).to(torch.int32)}
        if with_absgrad:
            sink = torch.full((P, 2), float("nan"))

            def fill(g):      # (runs inside the view's backward; returns None: the gradient passes unchanged)
                sink.copy_(g.abs() * (1.5 + k) + 0.25 * vis[:, None])

            screen.register_hook(fill)
            out["viewspace_absgrad"] = sink
        return out


def _literal_loop(model, views):
    """The per-view loop of train.py:279-292 spelled out, for the signed statistic and its absolute sibling alike."""
    gn, an, cnt = 0.0, 0.0, 0.0
    for k in views:
        out = model.render_loss(k)
        out["loss"].backward()
        gn = gn + torch.norm(out["viewspace_points"].grad[:, :2], dim=-1)
        an = an + torch.norm(out["viewspace_absgrad"][:, :2], dim=-1)
        cnt = cnt + out["visibility_filter"].to(torch.float32)
        model.xyz.grad = None
    v = cnt > 0
    gn[v] = gn[v] / cnt[v]
    an[v] = an[v] / cnt[v]
    return gn.unsqueeze(1), an.unsqueeze(1)


def _step_worker(rank, world, port, out_dir, n_views, in_flight):
    for p in (ROOT, os.path.join(ROOT, "saro-gs_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import view_parallel as vp
    torch.set_num_threads(1)
    vp.init_from_env("gloo")
    model = _Model(131)
    bucket = vp.StepBucket(dict(model.named_parameters()))
    stats = vp.distributed_step(bucket, list(range(n_views)), model.render_loss, views_in_flight=in_flight)
    plain = vp.distributed_step(bucket, list(range(n_views)), lambda k: model.render_loss(k, with_absgrad=False), views_in_flight=in_flight)
    assert "viewspace_point_absgrad" not in plain      # no sink in the views' dicts: the step's result is the one it always was
    assert torch.equal(plain["viewspace_point_grad"], stats["viewspace_point_grad"])
    torch.save({k: v.clone() for k, v in stats.items()}, os.path.join(out_dir, f"step{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_views,in_flight", [(2, 1), (1, 1), (5, 2)], ids=["one_view_per_rank", "a_rank_without_a_view", "two_views_in_flight"])
def test_distributed_step_reduces_the_absgrad_statistic(tmp_path, n_views, in_flight):
    world = 2
    mp.spawn(_step_worker, args=(world, _free_port(), str(tmp_path), n_views, in_flight), nprocs=world, join=True)
    want_g, want_a = _literal_loop(_Model(131), list(range(n_views)))
    assert float(want_a.max()) > 0.0 and not torch.isnan(want_a).any()
    for rank in range(world):
        got = torch.load(tmp_path / f"step{rank}.pt")
        assert got["viewspace_point_absgrad"].shape == (131, 1)
        np.testing.assert_allclose(got["viewspace_point_absgrad"].numpy(), want_a.numpy(), rtol=2e-6, atol=0)
        np.testing.assert_allclose(got["viewspace_point_grad"].numpy(), want_g.numpy(), rtol=2e-6, atol=1e-12)
