"""Fused 3-layer head, host side (no GPU): tests/mlp_math.py against torch.autograd of an fp64 nn.Sequential, the C ABI of gsrast_mlp3_*
(declared, exported, every argument error refused before any device call) and the module's bookkeeping (FusedMLP3.from_sequential)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import mlp_math as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 9, 128, 128, 3, False), (32, 9, 128, 128, 7, False), (32, 9, 128, 128, 48, False), (32, 0, 128, 64, 1, True),
          (1, 0, 32, 32, 1, False), (64, 0, 128, 128, 64, False), (5, 3, 96, 32, 17, True)]


def sequential(d_in, h1, h2, d_out, sigmoid, dtype=torch.float32):
    mods = [nn.Linear(d_in, h1), nn.ReLU(), nn.Linear(h1, h2), nn.ReLU(), nn.Linear(h2, d_out)] + ([nn.Sigmoid()] if sigmoid else [])
    return nn.Sequential(*mods).to(dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_restatement_equals_autograd_in_fp64(shape):
    d_x, d_tail, h1, h2, d_out, sig = shape
    c = mm.make_case(d_x, d_tail, h1, h2, d_out, 257, seed=11)
    seq = sequential(d_x + d_tail, h1, h2, d_out, sig, torch.float64)
    with torch.no_grad():
        for lin, w, b in ((seq[0], "w1", "b1"), (seq[2], "w2", "b2"), (seq[4], "w3", "b3")):
            lin.weight.copy_(torch.from_numpy(c[w]).double())
            lin.bias.copy_(torch.from_numpy(c[b]).double())
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    xin = x if c["x_tail"] is None else torch.cat((x, torch.from_numpy(c["x_tail"]).double()), 1)
    y = seq(xin)
    y.backward(torch.from_numpy(c["dy"]).double())
    want = dict(y=y.detach(), dx=x.grad, dw1=seq[0].weight.grad, db1=seq[0].bias.grad, dw2=seq[2].weight.grad, db2=seq[2].bias.grad,
                dw3=seq[4].weight.grad, db3=seq[4].bias.grad)
    got = mm.forward_backward(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], c["w3"], c["b3"], c["dy"], c["x_tail"], sig)
    for k in mm.NAMES:
        w = want[k].numpy()
        assert got[k].shape == w.shape, k
        assert np.abs(got[k] - w).max() <= 1e-12 * np.abs(w).max(), k


def test_relu_at_zero_passes_no_gradient():
    """A pre-activation of exactly 0: the restatement and torch both give 0 there."""
    w1, b1 = np.array([[1.0], [2.0]] * 16), np.zeros(32)                      # x = 0 -> a1 = 0 exactly
    w2, b2, w3, b3 = np.ones((32, 32)), np.ones(32), np.ones((1, 32)), np.zeros(1)
    g = mm.forward_backward(np.zeros((3, 1)), w1, b1, w2, b2, w3, b3, np.ones((3, 1)))
    assert not g["dw1"].any() and not g["db1"].any() and not g["dx"].any() and g["db2"].all()
    x = torch.zeros(3, 1, requires_grad=True)
    torch.relu(x @ torch.ones(1, 32)).sum().backward()
    assert not x.grad.any()


def test_symbols_are_declared_and_exported(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert names[-2:] == ["mlp_fwd", "mlp_bwd"] and names.index("mcmc_noise") == len(names) - 3      # appended: no earlier id moved


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 256      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    ptrs = ("x", "x_tail", "w1", "b1", "w2", "b2", "w3", "b3", "y", "dy", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")

    def desc(n=1000, d_x=32, d_tail=9, h1=128, h2=128, d_out=3, sigmoid=0, **null):
        d = _C.Mlp3Struct(n, d_x, d_tail, h1, h2, d_out, sigmoid)
        for p in ptrs:
            setattr(d, p, None if null.get(p, True) is None else one)
        return d

    calls = (("mlp3_forward", lambda d, wg=0: L.gsrast_mlp3_forward(C.byref(d), wg, None)),
             ("mlp3_backward", lambda d, wg=0: L.gsrast_mlp3_backward(C.byref(d), wg, one, None)),
             ("mlp3_scratch_bytes", lambda d, wg=0: -1 if L.gsrast_mlp3_scratch_bytes(C.byref(d), wg) == 0 else 0))
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
    assert L.gsrast_mlp3_forward(None, 0, None) == -1 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_backward(None, 0, one, None) == -1 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_scratch_bytes(None, 0) == 0 and "NULL descriptor" in err()
    assert L.gsrast_mlp3_forward(C.byref(desc(y=None)), 0, None) == -1 and "NULL y" in err()
    assert L.gsrast_mlp3_backward(C.byref(desc(dy=None)), 0, one, None) == -1 and "NULL dy" in err()
    assert L.gsrast_mlp3_backward(C.byref(desc(sigmoid=1, y=None)), 0, one, None) == -1 and "needs y" in err()
    assert L.gsrast_mlp3_backward(C.byref(desc()), 0, None, None) == -1 and "NULL scratch" in err()
    # nothing to launch: OK without a device
    assert L.gsrast_mlp3_forward(C.byref(desc(n=0, x=None, x_tail=None, y=None)), 0, None) == 0
    nothing = {p: None for p in ("dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")}
    assert L.gsrast_mlp3_backward(C.byref(desc(**nothing)), 0, None, None) == 0
    assert L.gsrast_mlp3_forward(C.byref(desc(d_tail=0, x_tail=None, n=0)), 0, None) == 0


def test_scratch_depends_on_workgroups_and_widths_only(rast):
    _C = rast._C
    L = _C.lib()
    params = 128 * 41 + 128 + 128 * 128 + 128 + 48 * 128 + 48
    sizes = {}
    for n in (0, 1, 10**6, 2**31 - 1):
        for wg in (1, 2, 3, 256):
            b = L.gsrast_mlp3_scratch_bytes(C.byref(_C.Mlp3Struct(n, 32, 9, 128, 128, 48, 0)), wg)
            assert b >= wg * params * 4 and b % 256 == 0 and b <= wg * params * 4 + 512
            sizes.setdefault(wg, set()).add(b)
    assert all(len(v) == 1 for v in sizes.values())
    small = L.gsrast_mlp3_scratch_bytes(C.byref(_C.Mlp3Struct(10**6, 1, 0, 32, 32, 1, 0)), 2)
    assert small < sizes[2].pop() and small >= 2 * (32 + 32 + 32 * 32 + 32 + 32 + 1) * 4
    assert L.gsrast_mlp3_scratch_bytes(C.byref(_C.Mlp3Struct(10, 32, 9, 128, 128, 48, 0)), 0) >= params * 4      # the default count


def test_from_sequential_keeps_parameters_and_keys():
    import fused_mlp
    for sig in (False, True):
        seq = sequential(41, 128, 64, 7, sig)
        seq.eval()
        f = fused_mlp.FusedMLP3.from_sequential(seq)
        assert f.sigmoid_out is sig and f.training is False
        assert len(list(f.parameters())) == 6 and all(a is b for a, b in zip(f.parameters(), seq.parameters()))
        assert list(f.state_dict().keys()) == list(seq.state_dict().keys()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
        assert [n for n, _ in f.named_parameters()] == [n for n, _ in seq.named_parameters()]
        # a checkpoint of the Sequential loads into the fused module and back
        other = sequential(41, 128, 64, 7, sig)
        f.load_state_dict(other.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(seq.parameters(), other.parameters()))      # (same objects: the Sequential changed too)
        other.load_state_dict(f.state_dict())
    own = fused_mlp.FusedMLP3(41, 128, 128, 3)
    assert list(own.state_dict().keys()) == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"] and own.sigmoid_out is False


def test_from_sequential_refuses_other_structures():
    import fused_mlp
    F = fused_mlp.FusedMLP3.from_sequential
    L, R = nn.Linear, nn.ReLU
    bad = [nn.Sequential(L(8, 32), R(), L(32, 3)),                                            # 2 layers
           nn.Sequential(L(8, 32), nn.Tanh(), L(32, 32), R(), L(32, 3)),                      # not ReLU
           nn.Sequential(L(8, 32), R(), L(32, 32), nn.LeakyReLU(), L(32, 3)),
           nn.Sequential(L(8, 32), R(), L(32, 32), R(), L(32, 3), nn.Tanh()),                 # another output activation
           nn.Sequential(L(8, 32), R(), L(32, 32), R(), L(32, 32), R(), L(32, 3)),            # 4 layers
           nn.Sequential(L(8, 48), R(), L(48, 32), R(), L(32, 3)),                            # width outside the set
           nn.Sequential(L(80, 32), R(), L(32, 32), R(), L(32, 3)),                           # D_in > 64
           nn.Sequential(L(8, 32), R(), L(32, 32), R(), L(32, 3, bias=False)),
           L(8, 3)]
    for seq in bad:
        with pytest.raises(ValueError):
            F(seq)


def test_convert_heads_swaps_only_what_matches():
    import fused_mlp

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.motion_mlp = sequential(41, 128, 128, 3, False)
            self.rot_mlp = sequential(41, 128, 128, 7, False)
            self.shs_mlp = nn.Sequential(nn.Linear(41, 128), nn.ReLU(), nn.Linear(128, 48))      # not a 3-layer head: left alone
            self.opacity_mlp = sequential(32, 128, 64, 1, True)
            self.other = sequential(41, 128, 128, 3, False)                                      # not a head's name: left alone

    m = Model()
    before = list(m.parameters())
    keys = list(m.state_dict().keys())
    opt = torch.optim.Adam([{"params": list(m.motion_mlp.parameters()), "name": "motion_mlp"}], lr=1e-3)
    assert fused_mlp.convert_heads(m) == ["motion_mlp", "rot_mlp", "opacity_mlp"]
    assert isinstance(m.motion_mlp, fused_mlp.FusedMLP3) and isinstance(m.opacity_mlp, fused_mlp.FusedMLP3) and m.opacity_mlp.sigmoid_out
    assert isinstance(m.shs_mlp, nn.Sequential) and isinstance(m.other, nn.Sequential)
    assert all(a is b for a, b in zip(m.parameters(), before)) and list(m.state_dict().keys()) == keys
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], m.motion_mlp.parameters()))
    assert fused_mlp.convert_heads(m) == []                                                      # already converted


def test_python_refusals_need_no_device(monkeypatch):
    import fused_mlp
    monkeypatch.setattr(fused_mlp._lib, "lib", lambda: pytest.fail("a refusal reached the library"))
    c = {k: (None if v is None else torch.from_numpy(v)) for k, v in mm.make_case(32, 9, 128, 128, 3, 10).items()}
    args = lambda **kw: [kw.get(k, c[k]) for k in ("x", "w1", "b1", "w2", "b2", "w3", "b3")]  # noqa: E731
    with pytest.raises(RuntimeError, match="GPU"):
        fused_mlp.fused_mlp3(*args(), x_tail=c["x_tail"])
    with pytest.raises(ValueError, match="do not chain"):
        fused_mlp.fused_mlp3(*args())                                         # w1 expects 41 columns
    with pytest.raises(ValueError, match="row count"):
        fused_mlp.fused_mlp3(*args(), x_tail=c["x_tail"][:5])
    with pytest.raises(ValueError, match="fp32"):
        fused_mlp.fused_mlp3(*args(x=c["x"].double()), x_tail=c["x_tail"])
    with pytest.raises(ValueError, match="hidden widths"):
        fused_mlp.fused_mlp3(*args(w1=torch.zeros(48, 41), b1=torch.zeros(48), w2=torch.zeros(128, 48)), x_tail=c["x_tail"])
    with pytest.raises(ValueError, match=r"must be in \[1, 64\]"):
        fused_mlp.fused_mlp3(*args(x=torch.zeros(10, 60), w1=torch.zeros(128, 69)), x_tail=c["x_tail"])
    with pytest.raises(ValueError, match="D_out"):
        fused_mlp.fused_mlp3(*args(w3=torch.zeros(65, 128), b3=torch.zeros(65)), x_tail=c["x_tail"])
