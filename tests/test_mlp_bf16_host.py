"""bf16 path of the fused 3-layer head, host side (no GPU): the rounding function and the model of tests/mlp_bf16_math.py against torch,
the additive C ABI (gsrast_mlp3_*_p: declared, exported, refusals before any device call, precision 0 = the existing calls) and the
module's precision bookkeeping."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import mlp_bf16_math as bm
import mlp_math as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 9, 128, 128, 3, False), (32, 9, 128, 128, 7, False), (32, 9, 128, 128, 48, False), (32, 0, 128, 64, 1, True),
          (1, 0, 32, 32, 1, False), (64, 0, 128, 128, 64, False), (5, 3, 96, 32, 17, True)]
_sid = lambda s: "-".join(str(int(v)) for v in s)  # noqa: E731


def test_bf_is_torchs_conversion():
    """Random values, exact ties both ways (to even down and to even up), +-0, +-Inf, NaN, the largest finite values."""
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(200000) * np.exp(rng.uniform(-30, 30, 200000))).astype(np.float32)
    hi = rng.integers(0, 1 << 16, 4096, dtype=np.uint32) << np.uint32(16)
    ties = (hi | np.uint32(0x8000)).view(np.float32)                                        # exactly half way: low bit of the kept part 0 and 1
    near = np.concatenate(((hi | np.uint32(0x7FFF)).view(np.float32), (hi | np.uint32(0x8001)).view(np.float32)))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38, 3.3895314e38, 1.0, 1.00390625, 1.01171875], np.float32)
    for v in (rand, ties, near, special):
        want = torch.from_numpy(v.copy()).to(torch.bfloat16).to(torch.float32).numpy()
        got = bm.bf(v)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    even_down, even_up = np.array([1.00390625], np.float32), np.array([1.01171875], np.float32)      # 1 + 2^-8 -> 1;  1 + 3 2^-8 -> 1 + 2^-6
    assert bm.bf(even_down)[0] == 1.0 and bm.bf(even_up)[0] == 1.015625
    assert bm.truncate(even_up)[0] == 1.0078125 and np.signbit(bm.bf(np.array([-0.0], np.float32)))[0]
    assert (bm.bf(rand) != bm.truncate(rand)).mean() > 0.4                                     # the wrong rounding is another function


def _ste(t):
    """bf16 rounding with a straight-through gradient, on an fp64 tensor holding fp32 values."""
    return t + (t.detach().to(torch.float32).to(torch.bfloat16).to(torch.float64) - t.detach())


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_model_equals_autograd_with_straight_through_rounding(shape):
    """The fp64-accumulated model's gradients are torch.autograd's of the same composition in fp64 with every rounding straight-through.
    The inputs are dyadic-free generic floats; a1, a2, z and g1, g2, g3 are rounded to fp32 in the model and not in torch, which moves a
    result by 2^-24 relative per step -- so the torch side rounds them to fp32 straight-through as well."""
    d_x, d_tail, h1, h2, d_out, sig = shape
    c = mm.make_case(d_x, d_tail, h1, h2, d_out, 257, seed=11)
    f32ste = lambda t: t + (t.detach().to(torch.float32).to(torch.float64) - t.detach())  # noqa: E731

    class RoundGrad(torch.autograd.Function):      # identity forward; the gradient passing back is rounded to fp32, then kept and bf16-rounded
        @staticmethod
        def forward(ctx, t, box):
            ctx.box = box
            return t.view_as(t)

        @staticmethod
        def backward(ctx, g):
            g32 = g.to(torch.float32).to(torch.float64)
            ctx.box.append(g32)
            return g32.to(torch.float32).to(torch.bfloat16).to(torch.float64), None

    t64 = lambda k: torch.from_numpy(c[k]).double()  # noqa: E731
    x = t64("x").requires_grad_(True)
    p = {k: t64(k).requires_grad_(True) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    xin = x if c["x_tail"] is None else torch.cat((x, t64("x_tail")), 1)
    g = {1: [], 2: [], 3: []}
    a1 = RoundGrad.apply(f32ste(_ste(xin) @ _ste(p["w1"]).T + p["b1"]), g[1])
    a2 = RoundGrad.apply(f32ste(_ste(torch.relu(a1)) @ _ste(p["w2"]).T + p["b2"]), g[2])
    z = RoundGrad.apply(f32ste(_ste(torch.relu(a2)) @ _ste(p["w3"]).T + p["b3"]), g[3])
    y = torch.sigmoid(z) if sig else z
    y.backward(t64("dy"))
    got = bm.forward_backward(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], sig, acc="fp64")
    # the bias gradients are the sums of the UNROUNDED g: autograd's bias gradient saw the bf16-rounded one, so take the kept fp32 values
    want = dict(y=y.detach(), dx=x.grad, dw1=p["w1"].grad, dw2=p["w2"].grad, dw3=p["w3"].grad,
                db1=g[1][0].sum(0), db2=g[2][0].sum(0), db3=g[3][0].sum(0))
    for k in bm.NAMES:
        w = want[k].numpy()
        assert got[k].shape == w.shape, k
        assert np.abs(got[k] - w).max() <= 1e-12 * np.abs(w).max(), (k, float(np.abs(got[k] - w).max() / np.abs(w).max()))


def test_dyadic_generator_asserts_its_own_exactness():
    """make_dyadic_case raises unless the three accumulations agree bit for bit and enough values are changed by the rounding; the model
    under the wrong rounding differs on such a case."""
    c, m = bm.make_dyadic_case(32, 9, 128, 128, 48, 300, seed=3)
    assert np.mean(m["xt"] != m["xin"]) > 0.15 and np.abs(m["dw2"]).max() > 0
    t = bm.forward_backward(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], False, rounding=bm.truncate)
    assert all(not np.array_equal(t[k], m[k]) for k in ("y", "dx", "dw1", "dw2", "dw3"))


def test_symbols_are_declared_and_exported(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    src = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    text = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define\s+GSRAST_MLP_FP32\s+0\b", text) and re.search(r"#define\s+GSRAST_MLP_BF16\s+1\b", text)
    assert (rast._C.MLP_FP32, rast._C.MLP_BF16) == (0, 1)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert names[-2:] == ["mlp_fwd", "mlp_bwd"] and names.index("mcmc_noise") == len(names) - 3      # no profile name was added
    assert "denormal" in open(os.path.join(ROOT, "saro-gs_amd", "csrc", "gsrast_mlp_bf16.h")).read().lower()


def _desc(_C, n=1000, d_x=32, d_tail=9, h1=128, h2=128, d_out=3, sigmoid=0, **null):
    d = _C.Mlp3Struct(n, d_x, d_tail, h1, h2, d_out, sigmoid)
    for p in ("x", "x_tail", "w1", "b1", "w2", "b2", "w3", "b3", "y", "dy", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3"):
        setattr(d, p, None if null.get(p, True) is None else 256)      # any non-NULL value: never dereferenced on the host
    return d


def test_other_precisions_are_refused_by_all_three_calls(rast):
    _C = rast._C
    L = _C.lib()
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    for bad in (2, -1, 3, 255, 2**31 - 1):
        assert L.gsrast_mlp3_forward_p(C.byref(_desc(_C)), bad, 0, None) == -1 and "precision" in err() and "mlp3_forward" in err()
        assert L.gsrast_mlp3_backward_p(C.byref(_desc(_C)), bad, 0, 256, None) == -1 and "precision" in err() and "mlp3_backward" in err()
        assert L.gsrast_mlp3_scratch_bytes_p(C.byref(_desc(_C)), bad, 0) == 0 and "precision" in err() and "mlp3_scratch_bytes" in err()
        assert L.gsrast_mlp3_forward_p(None, bad, 0, None) == -1 and "precision" in err()      # (before the descriptor is looked at)


@pytest.mark.parametrize("precision", [0, 1])
def test_the_fp32_refusals_come_back_at_both_precisions(rast, precision):
    """Every argument error of the calls without a precision, with its text, and none reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 256
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    desc = lambda **kw: _desc(_C, **kw)  # noqa: E731
    calls = (("mlp3_forward", lambda d, wg=0: L.gsrast_mlp3_forward_p(C.byref(d), precision, wg, None)),
             ("mlp3_backward", lambda d, wg=0: L.gsrast_mlp3_backward_p(C.byref(d), precision, wg, one, None)),
             ("mlp3_scratch_bytes", lambda d, wg=0: -1 if L.gsrast_mlp3_scratch_bytes_p(C.byref(d), precision, wg) == 0 else 0))
    for who, call in calls:
        sizes_only = who == "mlp3_scratch_bytes"
        if not sizes_only:
            assert call(desc(n=-1)) == -1 and who in err() and "negative N" in err()
        for bad in (dict(d_x=0), dict(d_x=-3), dict(d_tail=-1)):
            assert call(desc(**bad)) == -1 and who in err() and "D_x must be >= 1 and D_tail >= 0" in err(), bad
        for bad in (dict(d_x=65, d_tail=0), dict(d_x=32, d_tail=33), dict(d_x=64, d_tail=1), dict(d_x=2**31 - 1, d_tail=2**31 - 1)):
            assert call(desc(**bad)) == -1 and "must be in [1, 64]" in err(), bad
        for h in (0, 16, 33, 127, 160, 256, -32):
            assert call(desc(h1=h)) == -1 and "one of 32, 64, 96, 128" in err(), h
            assert call(desc(h2=h)) == -1 and "one of 32, 64, 96, 128" in err(), h
        for o in (0, 65, -1):
            assert call(desc(d_out=o)) == -1 and "D_out must be in [1, 64]" in err(), o
        assert call(desc(sigmoid=2)) == -1 and "sigmoid must be 0 or 1" in err()
        for wg in (-1, 65536):
            assert call(desc(), wg) == -1 and "workgroups" in err()
        if sizes_only:
            continue
        for p in ("w1", "b1", "w2", "b2", "w3", "b3"):
            assert call(desc(**{p: None})) == -1 and "NULL weight / bias" in err(), p
        assert call(desc(x=None)) == -1 and "NULL x" in err()
        assert call(desc(x_tail=None)) == -1 and "x_tail" in err()
    assert L.gsrast_mlp3_forward_p(None, precision, 0, None) == -1 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_backward_p(None, precision, 0, one, None) == -1 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_scratch_bytes_p(None, precision, 0) == 0 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_forward_p(C.byref(desc(y=None)), precision, 0, None) == -1 and "NULL y" in err()
    assert L.gsrast_mlp3_backward_p(C.byref(desc(dy=None)), precision, 0, one, None) == -1 and "NULL dy" in err()
    assert L.gsrast_mlp3_backward_p(C.byref(desc(sigmoid=1, y=None)), precision, 0, one, None) == -1 and "needs y" in err()
    assert L.gsrast_mlp3_backward_p(C.byref(desc()), precision, 0, None, None) == -1 and "NULL scratch" in err()
    # nothing to launch: OK without a device
    assert L.gsrast_mlp3_forward_p(C.byref(desc(n=0, x=None, x_tail=None, y=None)), precision, 0, None) == 0
    nothing = {p: None for p in ("dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")}
    assert L.gsrast_mlp3_backward_p(C.byref(desc(**nothing)), precision, 0, None, None) == 0
    assert L.gsrast_mlp3_forward_p(C.byref(desc(d_tail=0, x_tail=None, n=0)), precision, 0, None) == 0


def test_scratch_at_precision_0_is_the_old_functions(rast):
    _C = rast._C
    L = _C.lib()
    for shape in SHAPES:
        for n in (0, 1, 10**6):
            for wg in (0, 1, 3, 256):
                d = _C.Mlp3Struct(n, *shape[:5], int(shape[5]))
                old = L.gsrast_mlp3_scratch_bytes(C.byref(d), wg)
                assert old > 0 and L.gsrast_mlp3_scratch_bytes_p(C.byref(d), 0, wg) == old
                b = L.gsrast_mlp3_scratch_bytes_p(C.byref(d), 1, wg)      # bf16: workgroups x parameters too, never a function of n
                assert b > 0 and b % 256 == 0 and b == L.gsrast_mlp3_scratch_bytes_p(C.byref(_C.Mlp3Struct(7, *shape[:5], int(shape[5]))), 1, wg)


def _sequential(d_in, h1, h2, d_out, sigmoid):
    return nn.Sequential(*([nn.Linear(d_in, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(), nn.Linear(h2, d_out)] + ([nn.Sigmoid()] if sigmoid else [])))


def test_precision_bookkeeping_of_the_module():
    import fused_mlp
    seq = _sequential(41, 128, 64, 7, True)
    default = fused_mlp.FusedMLP3.from_sequential(seq)
    f = fused_mlp.FusedMLP3.from_sequential(seq, precision="bf16")
    assert default.precision == "fp32" and f.precision == "bf16" and fused_mlp.FusedMLP3(41, 128, 128, 3).precision == "fp32"
    assert fused_mlp.FusedMLP3(41, 128, 128, 3, precision="bf16").precision == "bf16"
    assert all(a is b for a, b in zip(f.parameters(), seq.parameters())) and len(list(f.parameters())) == 6 and not list(f.buffers())
    assert list(f.state_dict().keys()) == list(seq.state_dict().keys()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
    assert all(torch.equal(a, b) for a, b in zip(f.state_dict().values(), default.state_dict().values()))
    assert "precision=bf16" in repr(f) and "precision=fp32" in repr(default) and "sigmoid_out=True" in repr(f)
    f.load_state_dict(default.state_dict())
    assert f.precision == "bf16"                     # a plain attribute: a checkpoint neither carries nor resets it
    f.precision = "fp32"
    assert f.precision == "fp32"
    for bad in ("fp16", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="precision"):
            fused_mlp.FusedMLP3.from_sequential(seq, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            fused_mlp.FusedMLP3(41, 128, 128, 3, precision=bad)


def test_convert_heads_precision():
    import fused_mlp

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.motion_mlp = _sequential(41, 128, 128, 3, False)
            self.shs_mlp = nn.Sequential(nn.Linear(41, 128), nn.ReLU(), nn.Linear(128, 48))      # not a 3-layer head: left alone
            self.opacity_mlp = _sequential(32, 128, 64, 1, True)

    m = Model()
    before, keys = list(m.parameters()), list(m.state_dict().keys())
    with pytest.raises(ValueError, match="precision"):
        fused_mlp.convert_heads(m, precision="half")
    assert isinstance(m.motion_mlp, nn.Sequential)                                            # refused before anything was swapped
    assert fused_mlp.convert_heads(m, precision="bf16") == ["motion_mlp", "opacity_mlp"]
    assert m.motion_mlp.precision == m.opacity_mlp.precision == "bf16" and isinstance(m.shs_mlp, nn.Sequential)
    assert all(a is b for a, b in zip(m.parameters(), before)) and list(m.state_dict().keys()) == keys
    m2 = Model()
    assert fused_mlp.convert_heads(m2) == ["motion_mlp", "opacity_mlp"] and m2.motion_mlp.precision == "fp32"
    assert fused_mlp.convert_heads(m2, ("motion_mlp",), "bf16") == []                          # already converted: left as it is


def test_a_bad_precision_string_raises_without_a_device(monkeypatch):
    import fused_mlp
    monkeypatch.setattr(fused_mlp._lib, "lib", lambda: pytest.fail("a refusal reached the library"))
    c = {k: (None if v is None else torch.from_numpy(v)) for k, v in mm.make_case(32, 9, 128, 128, 3, 10).items()}
    args = [c[k] for k in ("x", "w1", "b1", "w2", "b2", "w3", "b3")]
    for bad in ("fp16", "bfloat16", "", None, 0, 1):
        with pytest.raises(ValueError, match="precision must be one of"):
            fused_mlp.fused_mlp3(*args, x_tail=c["x_tail"], precision=bad)
    with pytest.raises(TypeError):
        fused_mlp.fused_mlp3(*args, c["x_tail"], False, 0, "bf16")                             # keyword-only
    with pytest.raises(RuntimeError, match="GPU"):
        fused_mlp.fused_mlp3(*args, x_tail=c["x_tail"], precision="bf16")                      # a good one goes on to the device check
