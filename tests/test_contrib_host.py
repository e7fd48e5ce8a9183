"""CPU: the per-Gaussian blend-weight statistics (include/gsrast.h: gsrast_contrib_stats; `contrib=` / `pixel_weights=` of the Python
package) -- the reference of tests/contrib_math.py checks itself against math_renderer.render, the two symbols are declared, bound and
refuse bad arguments before any device work, the package refuses a bad sink or bad weights at call time, and the accumulation over views
(fused_densify.ContribStats, view_parallel.reduce_contrib_stats) does what a literal loop does.  (prune()'s carry of a ContribStats needs
GPU tensors: tests/test_gpu_contrib.py.)"""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import contrib_math as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


# ---- the reference --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cm.CASES))
def test_reference_against_render(name, scenes):
    c = cm.CASES[name]
    sc, cam = cm.case_scene(scenes, c)
    tab, amb, out = cm.contrib(sc, cam)
    ft = out["final_T"].numpy()
    n_live = out["n_live"]
    assert amb.mean() < 0.05
    # sum_i col0 = sum_p (1 - final_T), the integer identities, the bounds
    assert abs(tab[:, 0].sum() - (1.0 - ft).sum()) <= 1e-12 * (1.0 - ft).sum()
    assert tab[:, 3].sum() == (n_live > 0).sum() and tab[:, 2].sum() == n_live.sum()
    assert (tab[:, 1] <= cm.mr.C_AMAX).all() and (tab[:, 2] >= tab[:, 3]).all() and (tab[:, 0] <= tab[:, 1] * tab[:, 2] * (1 + 1e-12)).all()
    assert (tab[:, 2] == np.round(tab[:, 2])).all() and (tab[:, 3] == np.round(tab[:, 3])).all()
    vis = out["proj"]["disc"]["vis"]
    assert not tab[~vis].any() and (~vis).sum() >= 14 and (tab[vis, 2] == 0).any()      # culled rows, and listed-but-never-blended ones
    if c["kind"] == "cluster":
        assert out["tile_list_max"] > 600 and out["stopped"].sum() > 20 and (tab[:, 2] > 4 * 256).sum() >= 4      # (more than four tiles' worth of pixels)
    # half the weight: half of col 0, nothing else moves
    H, W = ft.shape
    half, _, _ = cm.contrib(sc, cam, pixel_weights=np.full((H, W), 0.5), render_out=out)
    np.testing.assert_allclose(half[:, 0], 0.5 * tab[:, 0], rtol=1e-14, atol=0)
    assert np.array_equal(half[:, 1:], tab[:, 1:])
    # a rectangle of zero weights removes exactly those pixels' counts
    wts = np.ones((H, W))
    wts[10:30, 20:50] = 0.0
    cut, _, _ = cm.contrib(sc, cam, pixel_weights=wts, render_out=out)
    assert tab[:, 2].sum() - cut[:, 2].sum() == n_live[10:30, 20:50].sum()
    assert tab[:, 3].sum() - cut[:, 3].sum() == (n_live[10:30, 20:50] > 0).sum()
    assert abs((tab[:, 0].sum() - cut[:, 0].sum()) - (1.0 - ft[10:30, 20:50]).sum()) <= 1e-10 * tab[:, 0].sum()
    assert (cut[:, 2] <= tab[:, 2]).all() and (cut[:, 1] <= tab[:, 1]).all()
    # weights outside [0, 1] are clamped
    big, _, _ = cm.contrib(sc, cam, pixel_weights=np.full((H, W), 7.0), render_out=out)
    assert np.array_equal(big, tab)


def test_float32_restatement_walks_the_same_lists():
    r = cm.reference("b")
    t32, _, _ = cm.contrib(r["sc"], r["cam"], pixel_weights=r["weights"], dtype=torch.float32, render_out=r["out"])
    assert np.array_equal(t32[:, 2:], r["table"][:, 2:])
    assert 0.0 < np.abs(t32[:, :2] - r["table"][:, :2]).max() < 1e-4


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(rast, L):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    assert L.gsrast_abi_version() == 6      # (additive when it came: the version moved later, with the call records)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert "contrib_blend" in names and "contrib_finish" in names


def test_scratch_size(L):
    b = [L.gsrast_contrib_scratch_bytes(p) for p in (-5, 0, 1, 63, 64, 65, 1000, 100000, 3000000)]
    assert all(y >= x for x, y in zip(b, b[1:])) and all(x % 256 == 0 and x > 0 for x in b) and b[-1] > b[-2] > b[-3]
    assert 20 * 3000000 <= b[-1] <= 20 * 3000000 + 4 * 256


def test_bad_arguments_fail_before_any_device_work(L, rast):
    opts = rast._C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    one = C.c_void_p(4096)
    err = L.gsrast_last_error

    def call(P=10, R=5, W=64, H=48, geom=one, binning=one, img=one, wts=None, stats=one, scratch=one, o=C.byref(opts)):
        return L.gsrast_contrib_stats(o, P, R, W, H, geom, binning, img, wts, stats, scratch, None)

    assert call(P=-1) == -1 and b"negative" in err()
    assert call(R=-1) == -1 and b"negative" in err()
    assert call(W=0) == -1 and b"zero-size" in err()
    assert call(H=0) == -1 and b"zero-size" in err()
    for kw in (dict(geom=None), dict(img=None), dict(binning=None)):
        assert call(**kw) == -1 and b"NULL state buffer" in err()
    assert call(stats=None) == -1 and b"NULL stats" in err()
    assert call(scratch=None) == -1 and b"NULL scratch" in err()
    assert call(stats=C.c_void_p(4100)) == -1 and b"aligned" in err()
    opts.exp_mode = 9
    assert call() == -1 and b"exp_mode" in err()
    opts.exp_mode = 0
    # P = 0: nothing to do, no launch, whatever else is NULL; with or without an options struct
    assert call(P=0, geom=None, binning=None, img=None, stats=None, scratch=None) == 0
    assert call(P=0, o=None) == 0
    assert call(P=0, W=0) == -1      # (the sizes are checked first)


# ---- the Python package ---------------------------------------------------------------------------------------------------------------
def test_python_refuses_a_bad_sink_or_bad_weights_at_call_time(rast):
    _C = rast._C
    P, H, W, cpu = 7, 16, 16, torch.device("cpu")
    good, gw = torch.zeros((P, 4)), torch.ones((H, W))
    _C.check_contrib(None, None, P, H, W, cpu)
    _C.check_contrib(good, None, P, H, W, cpu)
    _C.check_contrib(good, gw, P, H, W, cpu)
    _C.check_contrib(good, gw[None], P, H, W, cpu)
    bad = dict(shape=torch.zeros((P, 3)), rows=torch.zeros((P + 1, 4)), flat=torch.zeros(P * 4), dtype=torch.zeros((P, 4), dtype=torch.float64),
               layout=torch.zeros((4, P)).T, device=torch.zeros((P, 4), device="meta"), grad=torch.zeros((P, 4), requires_grad=True), kind=[0.0] * P)
    for what, t in bad.items():
        with pytest.raises(ValueError, match="contrib"):
            _C.check_contrib(t, None, P, H, W, cpu)
    badw = dict(shape=torch.ones((W, H + 1)), three=torch.ones((3, H, W)), dtype=torch.ones((H, W), dtype=torch.float64), layout=torch.ones((W, H)).T,
                device=torch.ones((H, W), device="meta"), grad=torch.ones((H, W), requires_grad=True), kind=1.0)
    for what, t in badw.items():
        with pytest.raises(ValueError, match="pixel_weights"):
            _C.check_contrib(good, t, P, H, W, cpu)
    with pytest.raises(ValueError, match="only legal together with contrib"):
        _C.check_contrib(None, gw, P, H, W, cpu)
    # through the public entry points: ValueError before anything is rendered (no GPU here)
    rs = rast.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    m3, m2, op = torch.zeros((P, 3)), torch.zeros((P, 3)), torch.zeros((P, 1))
    e = torch.empty(0)
    for kw, match in [(dict(contrib=bad[k]), "contrib") for k in ("shape", "dtype", "layout")] + [(dict(contrib=good, pixel_weights=badw[k]), "pixel_weights") for k in ("shape", "dtype", "layout")] \
            + [(dict(pixel_weights=gw), "only legal")]:
        with pytest.raises(ValueError, match=match):
            rast.rasterize_gaussians(m3, m2, e, torch.zeros((P, 3)), op, torch.ones((P, 3)), torch.ones((P, 4)), e, rs, **kw)
        with pytest.raises(ValueError, match=match):
            rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), **kw)
        with pytest.raises(ValueError, match=match):
            rast.GaussianRasterizerRaw(rs)(m3, m2, torch.ones((P, 4)), torch.zeros((P, 3)), op, torch.zeros((P, 1, 3)), torch.zeros((P, 15, 3)), **kw)
    for fn in (rast.GaussianRasterizer.forward, rast.GaussianRasterizerRaw.forward):      # the published keyword defaults do not move
        assert fn.__kwdefaults__ == {"return_aux": False}
    with pytest.raises(TypeError):
        rast.GaussianRasterizer(rs)(m3, m2, op, colors_precomp=torch.zeros((P, 3)), scales=torch.ones((P, 3)), rotations=torch.ones((P, 4)), contribs=good)
    # the one parser: every default, and the sink and its weights as given
    req, slots = rast._parse_request(rs, P, cpu)
    assert req == (False, False, None, None, None, False) and req._fields == ("return_aux", "antialiasing", "absgrad", "contrib", "pixel_weights", "camera")
    assert slots == (None, None, None, None)
    req, _ = rast._parse_request(rs, P, cpu, return_aux=True, contrib=good, pixel_weights=gw)
    assert req.return_aux is True and req.contrib is good and req.pixel_weights is gw
    with pytest.raises(ValueError, match="only legal"):
        rast._parse_request(rs, P, cpu, pixel_weights=gw)


# ---- accumulation over views ----------------------------------------------------------------------------------------------------------
def _sinks(P, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        cnt = torch.randint(0, 5, (P,), generator=g).float()
        top = torch.minimum(cnt, torch.randint(0, 3, (P,), generator=g).float())
        mx = torch.rand(P, generator=g) * (cnt > 0)
        out.append(torch.stack([mx * cnt * torch.rand(P, generator=g), mx, cnt, top], 1))
    return out


def test_contrib_stats_update_against_a_literal_loop():
    import fused_densify
    P = 37
    st = fused_densify.ContribStats(P, "cpu")
    sinks = _sinks(P, 3)
    for s in sinks:
        st.update(s)
    for i in range(P):
        ws = mx = pc = tc = vw = 0.0
        for s in sinks:
            ws += float(s[i, 0]); mx = max(mx, float(s[i, 1])); pc += float(s[i, 2]); tc += float(s[i, 3]); vw += 1.0 if float(s[i, 2]) > 0 else 0.0
        assert abs(float(st.weight_sum[i]) - ws) <= 1e-6 * max(ws, 1.0)
        assert float(st.weight_max[i]) == np.float32(mx) and float(st.pixel_count[i]) == pc and float(st.top_count[i]) == tc and float(st.views[i]) == vw
    assert float(st.views.max()) == 3.0 and float(st.views.min()) < 3.0
    with pytest.raises(RuntimeError, match="sink"):
        st.update(torch.zeros((P, 3)))
    with pytest.raises(KeyError):
        st.column("nope")
    st.reset()
    assert st.P == P and not st.sums.any() and not st.weight_max.any()
    st.reset(5)
    assert st.P == 5 and st.sums.shape == (5, 4)


def test_keep_mask_by_rank_breaks_ties_by_index():
    import fused_densify
    st = fused_densify.ContribStats(8, "cpu")
    st.update(torch.tensor([[2.0, .5, 1, 0], [5.0, .5, 1, 0], [2.0, .5, 1, 0], [0.0, 0, 0, 0], [2.0, .5, 1, 0], [9.0, .5, 1, 0], [0.0, 0, 0, 0], [2.0, .5, 1, 0]]))
    # 9, 5, then the four 2.0 in index order, then the two zeros in index order
    assert st.keep_mask_by_rank("weight_sum", 0.5).tolist() == [True, True, True, False, False, True, False, False]
    assert st.keep_mask_by_rank("weight_sum", 0.51).tolist() == [True, True, True, False, True, True, False, False]      # ceil(0.51 * 8) = 5
    assert st.keep_mask_by_rank("weight_sum", 7 / 8).tolist() == [True, True, True, True, True, True, False, True]
    assert st.keep_mask_by_rank("weight_sum", 1.0).all() and not st.keep_mask_by_rank("weight_sum", 0.0).any()
    assert st.keep_mask_by_rank("pixel_count", 0.25).tolist() == [True, True, False, False, False, False, False, False]    # all ties: the lowest indices
    for col in st.COLUMNS:
        assert st.keep_mask_by_rank(col, 0.5).dtype is torch.bool
    with pytest.raises(ValueError):
        st.keep_mask_by_rank("weight_sum", 1.5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "saro-gs_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import fused_densify
    import view_parallel as vp
    vp.init_from_env("gloo")
    P = 53
    st = fused_densify.ContribStats(P, "cpu")
    for k, s in enumerate(_sinks(P, 5)):      # five views dealt round-robin
        if k % world == rank:
            st.update(s)
    vp.reduce_contrib_stats(st)
    torch.save(dict(sums=st.sums.clone(), weight_max=st.weight_max.clone(), keep=st.keep_mask_by_rank("weight_sum", 0.4)), os.path.join(out_dir, f"c{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_contrib_stats_over_gloo(tmp_path):
    import fused_densify
    world = 2
    mp.spawn(_reduce_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = fused_densify.ContribStats(53, "cpu")
    for s in _sinks(53, 5):
        want.update(s)
    got = [torch.load(tmp_path / f"c{r}.pt") for r in range(world)]
    for g in got:
        np.testing.assert_allclose(g["sums"].numpy(), want.sums.numpy(), rtol=1e-6, atol=0)
        assert torch.equal(g["weight_max"], want.weight_max)
        assert torch.equal(g["sums"][:, 1:], want.sums[:, 1:])      # the counts are integers: exact
    assert torch.equal(got[0]["sums"], got[1]["sums"]) and torch.equal(got[0]["keep"], got[1]["keep"])      # replicated ranks agree
    # without a process group the call is a no-op
    import view_parallel as vp
    before = want.sums.clone()
    vp.reduce_contrib_stats(want)
    assert torch.equal(before, want.sums)
