"""CPU: each pixel's first or heaviest K contributors (include/gsrast.h: gsrast_pixel_contributors; `pixel_contributors` of the Python
package) -- the restatement of tests/topk_math.py against a literal per-pixel loop, the facts about contrib_math's cases that
tests/test_gpu_topk.py relies on (how few pixels are ambiguous, how long the pixels' lists are), and the surface: the symbol is declared,
exported and bound, the C call refuses bad arguments before any device work, each with its text, and the Python call refuses with
ValueError before anything is rendered."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import capi_header
import contrib_math as cm
import topk_math as tm


# ---- 1. the restatement against a literal loop ------------------------------------------------------------------------------------------
def _brute(w, live, rows, K, order):
    N, G = w.shape
    ids, wts, cnt = np.full((N, K), -1, np.int64), np.zeros((N, K)), np.zeros(N, np.int64)
    for p in range(N):
        mine = [(float(w[p, g]), g) for g in range(G) if live[p, g]]      # blend order
        cnt[p] = len(mine)
        if order == "weight":
            done = []
            for x in mine:                                                 # insertion: in front of the first STRICTLY smaller one
                at = len(done)
                for k, y in enumerate(done):
                    if x[0] > y[0]:
                        at = k
                        break
                done.insert(at, x)
            mine = done
        for k, (x, g) in enumerate(mine[:K]):
            ids[p, k], wts[p, k] = rows[g], x
    return ids, wts, cnt


def _hand_made():
    """Six pixels over eight Gaussians (rows 50, 40, ...: blend order is not row order).  K = 4 below: pixel 0 an exact tie among the leaders
    and one across the K-th place, 1: n < K, 2: n = K, 3: n > K, 4: n = 0, 5: everything equal."""
    rows = np.array([50, 40, 7, 3, 90, 11, 2, 65])
    w = np.zeros((6, 8))
    live = np.zeros((6, 8), bool)
    w[0] = [0.25, 0.5, 0.25, 0.125, 0.5, 0.125, 0.125, 0.0625]; live[0] = True
    w[1, [1, 6]] = [0.1, 0.7]; live[1, [1, 6]] = True
    w[2, [0, 2, 3, 7]] = [0.2, 0.1, 0.4, 0.3]; live[2, [0, 2, 3, 7]] = True
    w[3] = [0.01, 0.3, 0.02, 0.2, 0.03, 0.1, 0.04, 0.05]; live[3] = True
    w[3, 4] = 0.9; live[3, 4] = False                                       # (a dead pair's value is never looked at)
    w[5] = 0.125; live[5] = True
    return w, live, rows


@pytest.mark.parametrize("order", tm.ORDERS)
@pytest.mark.parametrize("K", [1, 4, 8, 16])
def test_restatement_against_a_literal_loop(K, order):
    w, live, rows = _hand_made()
    ids, wts, cnt = tm.slots(w, live, rows, K, order)
    bi, bw, bc = _brute(w, live, rows, K, order)
    assert np.array_equal(ids.numpy(), bi) and np.array_equal(wts.numpy(), bw) and np.array_equal(cnt.numpy(), bc)
    assert cnt.tolist() == [8, 2, 4, 7, 0, 8]
    if K == 4 and order == "weight":
        assert ids[0].tolist() == [40, 90, 50, 7] and wts[0].tolist() == [0.5, 0.5, 0.25, 0.25]      # ties: the earlier in blend order first
        assert ids[1].tolist() == [2, 40, -1, -1] and wts[1].tolist() == [0.7, 0.1, 0.0, 0.0]
        assert ids[2].tolist() == [3, 65, 50, 7] and ids[3].tolist() == [40, 3, 11, 65] and ids[4].tolist() == [-1] * 4
        assert ids[5].tolist() == [50, 40, 7, 3]
    if K == 4 and order == "depth":
        assert ids[0].tolist() == [50, 40, 7, 3] and ids[1].tolist() == [40, 2, -1, -1] and ids[2].tolist() == [50, 7, 3, 65]
        assert ids[3].tolist() == [50, 40, 7, 3] and wts[3].tolist() == [0.01, 0.3, 0.02, 0.2]
    # float32 in, float32 out; no Gaussian at all
    assert tm.slots(torch.as_tensor(w, dtype=torch.float32), live, rows, K, order)[1].dtype is torch.float32
    e_ids, e_w, e_c = tm.slots(np.zeros((3, 0)), np.zeros((3, 0), bool), np.zeros(0, np.int64), K, order)
    assert (e_ids == -1).all() and not e_w.any() and not e_c.any() and e_ids.shape == (3, K)


def test_gap_ambiguity_looks_at_the_top_k_plus_one():
    w, live, _ = _hand_made()
    assert tm.gap_ambiguous(w, live, 1).tolist() == [True, False, False, False, False, True]      # only the leaders' tie
    w3 = np.array([[0.5, 0.3, 0.2, 0.2 * (1 - 5e-5), 0.1]])
    l3 = np.ones((1, 5), bool)
    assert tm.gap_ambiguous(w3, l3, 1).tolist() == [False] and tm.gap_ambiguous(w3, l3, 2).tolist() == [False]
    assert tm.gap_ambiguous(w3, l3, 3).tolist() == [True]                   # slot 2 against the first one left out
    l3[0, 3] = False
    assert tm.gap_ambiguous(w3, l3, 3).tolist() == [False]


# ---- 2. the cap, and the facts the GPU test relies on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("antialiasing", [False, True])
@pytest.mark.parametrize("name", list(cm.CASES))
def test_few_pixels_are_ambiguous_and_the_lists_are_what_the_gpu_test_needs(name, antialiasing):
    """Measured on the CPU, the ambiguous share at K = 16 in weight order: 0.73 %, 0.92 %, 0.10 %, 0.16 % (a, a + AA, b, b + AA); of that,
    math_renderer's own mask is 0.51 %, 0.67 %, 0.06 %, 0.16 %."""
    ref = tm.reference(name, antialiasing)
    shares = {K: float(tm.ambiguous(ref, K, "weight").float().mean()) for K in (1, 3, 8, 16)}
    print(f"case {name}, antialiasing {antialiasing}: ambiguous share by K {shares}, math_renderer's own {float(ref['amb_mr'].float().mean()):.4f}")
    assert shares[16] <= 0.05 and shares[1] <= shares[3] <= shares[8] <= shares[16]
    assert float(tm.ambiguous(ref, 16, "depth").float().mean()) <= shares[16]
    count = tm.topk(ref, 16, "weight")[2]
    assert np.array_equal(count.numpy(), ref["out"]["n_live"].reshape(-1))
    if name == "a":      # pixels far beyond 16 contributors (163 without, 112 with antialiasing), lists longer than two 256-entry batches
        assert int(count.max()) > 100 and float((count > 8).float().mean()) > 0.4 and float((count > 16).float().mean()) > 0.1
        assert ref["out"]["tile_list_max"] > 2 * 256
    else:                # nothing is truncated at K = 16 (the GPU test compares whole lists with contrib's columns there); empty pixels
        assert int(count.max()) <= 8 and float((count == 0).float().mean()) > 0.3
    # on the pixels math_renderer does not flag, float32 decides like float64: both restatements fill the same slots
    ok = ~ref["amb_mr"]
    assert bool((ref["live32"] == ref["live64"])[ok].all())
    tol, worst = tm.bar(ref)
    print(f"  max|w32 - w64| over the non-ambiguous K = 16 entries {worst:.3e} -> bar {tol:.3e}")
    assert 0.0 < worst < 1e-4 and tol == 4.0 * worst + 2.0 ** -23
    # slot 0 in weight order is contrib's top Gaussian, the depth slots' weights add up to no more than 1 - T_final
    ids, wts, _ = tm.topk(ref, 1, "weight")
    has = ids[:, 0] >= 0
    top = np.bincount(ids[has, 0].numpy(), minlength=ref["P"])
    table, _, _ = cm.contrib(ref["sc"], ref["cam"], antialiasing=antialiasing, render_out=ref["out"])
    assert np.array_equal(top, table[:, 3])
    d_w = tm.topk(ref, 16, "depth")[1]
    assert bool((d_w.sum(dim=1) <= 1.0 - torch.as_tensor(ref["out"]["final_T"]).reshape(-1) + 1e-12).all())


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(rast):
    return rast._C.lib()


def test_symbol_is_declared_exported_and_bound(rast, L):
    protos = capi_header.prototypes()
    assert protos["gsrast_pixel_contributors"] == ("int", ["const gsrast_options*", "int", "int", "int", "int", "const char*", "const char*", "const char*",
                                                           "int", "int", "int32_t*", "float*", "int32_t*", "void*"])
    restype, argtypes = rast._C.SIGNATURES["gsrast_pixel_contributors"]
    assert restype is C.c_int and len(argtypes) == 14 and "gsrast_pixel_contributors" in rast._C.EXPORTS
    assert L.gsrast_pixel_contributors.argtypes == list(argtypes)
    assert L.gsrast_abi_version() == 6 and rast._C.ABI_VERSION == 6
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == 34 and not any("topk" in n or "pixel" in n for n in names)      # (the query's launches are not in the profile table)
    assert rast._C.TOPK_MAX == tm.K_MAX == 16 and rast._C.TOPK_ORDERS == {"weight": 0, "depth": 1}
    assert "pixel_contributors" in rast.__all__ and "PixelContributors" in rast.__all__
    assert rast.PixelContributors._fields == ("ids", "weights", "count", "color", "depth", "radii")
    sig = inspect.signature(rast.pixel_contributors)
    assert list(sig.parameters) == ["means3D", "opacities", "scales", "rotations", "raster_settings", "K", "order", "shs", "colors_precomp", "cov3D_precomp",
                                    "antialiasing"]
    assert sig.parameters["K"].default == 8 and sig.parameters["order"].default == "weight" and sig.parameters["raster_settings"].kind is inspect.Parameter.KEYWORD_ONLY
    b = inspect.signature(rast._C.pixel_contributors)
    assert list(b.parameters)[:8] == ["K", "order", "R", "W", "H", "geomBuffer", "binningBuffer", "imageBuffer"]
    assert b.parameters["options"].default is None and b.parameters["with_count"].default is True
    # the render request keeps its shape: this is no forward keyword
    assert rast._Request._fields == ("return_aux", "antialiasing", "absgrad", "contrib", "pixel_weights", "camera")
    assert "topk" not in rast._RENDER_OPTIONS and "pixel_contributors" not in rast._RENDER_OPTIONS


def test_bad_arguments_fail_before_any_device_work_each_with_its_text(L, rast):
    opts = rast._C.OptionsStruct()
    L.gsrast_options_init(C.byref(opts))
    one = C.c_void_p(4096)
    err = L.gsrast_last_error

    def call(P=10, R=5, W=64, H=48, geom=one, binning=one, img=one, K=8, order=0, ids=one, weights=one, count=one, o=C.byref(opts)):
        return L.gsrast_pixel_contributors(o, P, R, W, H, geom, binning, img, K, order, ids, weights, count, None)

    assert call(P=-1) == -1 and err() == b"pixel_contributors: negative P or R"
    assert call(R=-1) == -1 and err() == b"pixel_contributors: negative P or R"
    assert call(W=0) == -1 and err() == b"pixel_contributors: zero-size image"
    assert call(H=0) == -1 and err() == b"pixel_contributors: zero-size image"
    for K in (0, -3, 17, 1 << 20):
        assert call(K=K) == -1 and err() == b"pixel_contributors: K must be 1..16"
    for order in (-1, 2, 7):
        assert call(order=order) == -1 and err() == b"pixel_contributors: order must be 0 (weight) or 1 (depth)"
    for kw in (dict(geom=None), dict(img=None), dict(binning=None)):
        assert call(**kw) == -1 and err() == b"pixel_contributors: NULL state buffer"
    assert call(ids=None) == -1 and err() == b"pixel_contributors: NULL ids"
    assert call(weights=None) == -1 and err() == b"pixel_contributors: NULL weights"
    for mode in (-1, 3, 9):
        opts.exp_mode = mode
        assert call() == -1 and err() == b"pixel_contributors: exp_mode must be 0, 1 or 2"
    opts.exp_mode = 0
    # the sizes and K are looked at first, also for a state nothing was blended in
    assert call(P=0, W=0) == -1 and call(R=0, K=0) == -1 and call(P=0, ids=None) == -1 and call(R=0, weights=None) == -1


def test_python_refuses_with_value_error_before_anything_is_rendered(rast):
    _C = rast._C
    assert _C.check_pixel_contributors(1, "weight") == 0 and _C.check_pixel_contributors(16, "depth") == 1 and _C.check_pixel_contributors(8, 1) == 1
    for K in (0, 17, -1, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="K must be"):
            _C.check_pixel_contributors(K, "weight")
    for order in ("Weight", "id", "", 2, -1, None, True, 0.0):
        with pytest.raises(ValueError, match="order must be"):
            _C.check_pixel_contributors(8, order)
    e = torch.empty(0, dtype=torch.uint8)
    with pytest.raises(ValueError, match="K must be"):
        _C.pixel_contributors(0, "weight", 5, 16, 16, e, e, e)
    with pytest.raises(ValueError, match="order must be"):
        _C.pixel_contributors(8, "nearest", 5, 16, 16, e, e, e)
    # the public call: no GPU here, so a call that passes every check of its arguments ends at "must live on a GPU"
    P, H, W = 7, 16, 16
    rs = rast.GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    m, o, s, q = torch.zeros((P, 3)), torch.zeros((P, 1)), torch.ones((P, 3)), torch.ones((P, 4))
    pc = rast.pixel_contributors
    with pytest.raises(ValueError, match="means3D must live on a GPU"):
        pc(m, o, s, q, raster_settings=rs)
    with pytest.raises(ValueError, match="means3D must live on a GPU"):      # (inputs that require grad are no refusal)
        pc(m.clone().requires_grad_(True), o[:, 0], s, q, raster_settings=rs, K=16, order="depth", shs=torch.zeros((P, 16, 3)), antialiasing=True)
    with pytest.raises(ValueError, match="K must be"):
        pc(m, o, s, q, raster_settings=rs, K=17)
    with pytest.raises(ValueError, match="K must be"):
        pc(m, o, s, q, raster_settings=rs, K=0)
    with pytest.raises(ValueError, match="order must be"):
        pc(m, o, s, q, raster_settings=rs, order="front")
    bad = [dict(means3D=torch.zeros((P, 4))), dict(means3D=torch.zeros(P * 3)), dict(means3D=[0.0]), dict(opacities=torch.zeros((P + 1, 1))),
           dict(opacities=torch.zeros((P, 2))), dict(scales=torch.ones((P, 4))), dict(rotations=torch.ones((P, 3))), dict(rotations=torch.ones((P - 1, 4))),
           dict(shs=torch.zeros((P, 16))), dict(shs=torch.zeros((P, 16, 4))), dict(colors_precomp=torch.zeros((P, 4))),
           dict(opacities=torch.zeros((P, 1), dtype=torch.float64)), dict(scales=torch.ones((P, 3), dtype=torch.float16)), dict(opacities=None)]
    for kw in bad:
        args = dict(means3D=m, opacities=o, scales=s, rotations=q)
        args.update(kw)
        with pytest.raises(ValueError, match="pixel_contributors: ") as ei:
            pc(args.pop("means3D"), args.pop("opacities"), args.pop("scales"), args.pop("rotations"), raster_settings=rs, **args)
        assert "live on a GPU" not in str(ei.value), kw
    for kw in (dict(scales=None), dict(rotations=None), dict(cov3D_precomp=torch.zeros((P, 6))), dict(scales=None, rotations=None)):
        args = dict(scales=s, rotations=q)
        args.update(kw)
        with pytest.raises(ValueError, match="exactly one of"):
            pc(m, o, raster_settings=rs, **args)
    with pytest.raises(ValueError, match="cov3D_precomp must be"):
        pc(m, o, raster_settings=rs, cov3D_precomp=torch.zeros((P, 5)))
    with pytest.raises(ValueError, match="at most one of"):
        pc(m, o, s, q, raster_settings=rs, shs=torch.zeros((P, 16, 3)), colors_precomp=torch.zeros((P, 3)))
    with pytest.raises(ValueError, match="must not be empty"):
        pc(m, o, s, q, raster_settings=rs._replace(image_width=0))
    with pytest.raises(ValueError, match="viewmatrix must be"):
        pc(m, o, s, q, raster_settings=rs._replace(viewmatrix=torch.eye(3)))
    with pytest.raises(TypeError):                                           # the settings are keyword-only
        pc(m, o, s, q, rs)
