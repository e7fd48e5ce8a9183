"""Temporal lifespan, host side (no GPU): tests/temporal_math.py against torch.autograd of an fp64 torch composition of the same ops, the
embedding's layout, the sigmoid form of Q, inv = (1/I) / min(1/I), the C ABI of gsrast_temporal_* (declared, exported, bound, every
argument error refused before any device call) and the module's own refusals.

There is no golden file from the reference for these functions: its Q is a nested function hard-wired to device "cuda" and its module
does not import on a machine without CUDA, so the restatement is pinned to the formulas (include/gsrast.h) and to torch.autograd instead."""
import os
import re

import numpy as np
import pytest
import torch

import temporal_math as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("min_scale", [1 / 300, 0.01, 1.0])
@pytest.mark.parametrize("t", [0.0, 0.37, 1.0])
def test_restatement_equals_autograd_in_fp64(t, min_scale, sig):
    c, _ = tm.make_case(257, t, seed=3)
    head = torch.from_numpy(c["head"]).double().reshape(-1, 1).requires_grad_(True)
    center = torch.from_numpy(c["center"]).double().reshape(-1, 1).requires_grad_(True)
    lifespan, state, emb = tm.torch_gate(head, center, t, min_scale, 4, sig)
    torch.autograd.backward((lifespan, state), (torch.from_numpy(c["d_lifespan"]).double().reshape(-1, 1), torch.from_numpy(c["d_state"]).double().reshape(-1, 1)))
    want = dict(lifespan=lifespan.detach(), state=state.detach(), time_emb=emb, d_head=head.grad, d_center=center.grad)
    got = tm.gate(c["head"], c["center"], t, min_scale, 4, sig, c["d_lifespan"], c["d_state"])
    for k, w in want.items():
        w = w.numpy().reshape(got[k].shape)
        assert np.abs(got[k] - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0), k
    # the integral: values against the torch composition
    I = tm.torch_integral(head.detach(), center.detach(), min_scale, sig).numpy().reshape(-1)
    assert np.abs(tm.integral(c["head"], c["center"], min_scale, sig) - I).max() <= 1e-12


@pytest.mark.parametrize("multires", [0, 1, 4, 8])
def test_embedding_columns_and_frequencies(multires):
    d = np.array([0.0, 0.25, -1.5, 3.0])
    e = tm.embed(d, multires)
    assert e.shape == (4, 2 * multires + 1) and np.array_equal(e[:, 0], d)
    for k in range(multires):
        assert np.array_equal(e[:, 1 + 2 * k], np.sin(d * float(1 << k))) and np.array_equal(e[:, 2 + 2 * k], np.cos(d * float(1 << k)))      # sin before cos, exact powers of two
    assert np.array_equal(e[0], np.array([0.0] + [0.0, 1.0] * multires))
    assert np.array_equal(tm.torch_embed(torch.from_numpy(d).reshape(-1, 1), multires).numpy(), e)
    # the reference's Embedder draws its frequencies as 2 ** linspace(0, multires - 1, multires): the same exact powers
    if multires:
        assert np.array_equal((2.0 ** torch.linspace(0.0, multires - 1, steps=multires)).numpy(), 2.0 ** np.arange(multires))


def test_sigmoid_form_of_Q_equals_the_reference_form_where_that_is_not_cancelled():
    x = np.linspace(-4.0, 12.0, 4001)                    # z from -10.9 to 141: e^z stays far above 2^-53
    a, b = tm.Q(x), tm.Q_reference_form(x)
    assert np.abs(a - b).max() <= 4 * 2.0 ** -53         # (both are within a few roundings of the same number below 1)
    # where the reference's form HAS cancelled, the sigmoid form still carries the value
    far = np.array([-9.0, -12.0])
    assert (tm.Q_reference_form(far) == 0).all() and (tm.Q(far) > 0).all()
    assert tm.Q(np.array([-1e3]))[0] == 0.0 and tm.Q(np.array([1e3]))[0] == 1.0 and not np.isnan(tm.Q(np.array([-1e5, 1e5]))).any()


def test_inv_is_the_references_expression():
    c, _ = tm.make_case(4099, 0.37, seed=5)
    I = tm.integral(c["head"], c["center"], 0.01)
    dead, inv, (imax, n) = tm.integral_outputs(I, 0.0025)
    valid = ~dead
    assert 0 < n < 4099 and n == valid.sum() and imax == I[valid].max()
    ref = 1.0 / I[valid]
    ref = ref / ref.min()                                 # update_learning_rate: inv_intergral / inv_intergral.min()
    assert np.abs(inv[valid] - ref).max() <= 4 * 2.0 ** -53 * ref.max() and not inv[dead].any() and inv[valid].min() == 1.0
    dead, inv, stats = tm.integral_outputs(I, 10.0)
    assert dead.all() and not inv.any() and stats == (0.0, 0)


def test_select_keeps_index_order():
    state = np.array([0.5, 0.0005, 0.001, 0.0011, np.nan, 1.0])
    n, (a,) = tm.select(state, [np.arange(12).reshape(6, 2)])
    assert n == 3 and np.array_equal(a, [[0, 1], [6, 7], [10, 11]])


def test_symbols_are_declared_exported_and_bound(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert not any("temporal" in n for n in names)       # the launches are not in the profile table


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    L = rast._C.lib()
    one = 256      # any non-NULL, 16-byte aligned value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")

    def fwd(P=10, multires=4, sig=0, t=0.5, ms=0.01, thr=0.001, head=one, center=one, lifespan=one, state=one, emb=one, dead=one):
        return L.gsrast_temporal_gate_forward(P, multires, sig, t, ms, thr, head, center, lifespan, state, emb, dead, None)

    def bwd(P=10, sig=0, t=0.5, ms=0.01, head=one, center=one, dl=one, ds=one, d_head=one, d_center=one):
        return L.gsrast_temporal_gate_backward(P, sig, t, ms, head, center, dl, ds, d_head, d_center, None)

    def integ(P=10, sig=0, start=0.0, end=1.0, ms=0.01, mi=0.0025, head=one, center=one, integral=one, dead=one, inv=one, stats=one):
        return L.gsrast_temporal_integral(P, sig, start, end, ms, mi, head, center, integral, dead, inv, stats, None)

    for who, call in (("temporal_gate_forward", fwd), ("temporal_gate_backward", bwd), ("temporal_integral", integ)):
        assert call(P=-1) == -1 and who in err() and "negative P" in err()
        for ms in (0.0, -0.5, 1.0001, nan, inf):
            assert call(ms=ms) == -1 and who in err() and "min_scale must be in (0, 1]" in err(), ms
        assert call(sig=2) == -1 and "sigmoid_center must be 0 or 1" in err()
        for p in ("head", "center"):
            assert call(**{p: None}) == -1 and who in err() and "NULL required pointer" in err(), p
        assert call(P=0, head=None, center=None) == 0      # nothing to launch: OK without a device
    for m in (-1, 9, 100):
        assert fwd(multires=m) == -1 and "multires must be in [0, 8]" in err(), m
    for t in (nan, inf, -inf):
        assert fwd(t=t) == -1 and "t must be finite" in err()
        assert bwd(t=t) == -1 and "t must be finite" in err()
    for p in ("lifespan", "state"):
        assert fwd(**{p: None}) == -1 and "NULL required pointer" in err(), p
    for bad in (260, 264, 257):
        assert fwd(emb=bad) == -1 and "time_emb must be 16-byte aligned" in err(), bad
    for bad in (dict(start=nan), dict(end=inf), dict(start=-inf)):
        assert integ(**bad) == -1 and "start and end must be finite" in err(), bad
    assert integ(start=0.6, end=0.5) == -1 and "end < start" in err()
    for mi in (-1e-3, nan, inf):
        assert integ(mi=mi) == -1 and "min_integral" in err(), mi
    for p in ("integral", "dead", "stats"):
        assert integ(**{p: None}) == -1 and "NULL required pointer" in err(), p
    # the optional pointers are optional, and a backward with nothing wanted launches nothing
    assert bwd(d_head=None, d_center=None) == 0
    assert fwd(P=0, lifespan=None, state=None, emb=None, dead=None) == 0 and integ(P=0, integral=None, dead=None, inv=None, stats=None) == 0


def test_python_refusals_need_no_device(monkeypatch):
    import fused_temporal as ft
    monkeypatch.setattr(ft._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    head, pos = torch.rand(10, 1), torch.rand(10, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ft.temporal_gate(head, pos, 0.5, min_scale=0.01)
    with pytest.raises(RuntimeError, match="GPU"):
        ft.temporal_integral(head, pos, min_scale=0.01, min_integral=0.0025)
    with pytest.raises(RuntimeError, match="GPU"):
        ft.temporal_select(head, pos, 0.5, [], min_scale=0.01)
    for ms in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="min_scale"):
            ft.temporal_gate(head, pos, 0.5, min_scale=ms)
    for m in (-1, 9):
        with pytest.raises(ValueError, match="multires"):
            ft.temporal_gate(head, pos, 0.5, min_scale=0.01, multires=m)
    with pytest.raises(ValueError, match="finite"):
        ft.temporal_gate(head, pos, float("nan"), min_scale=0.01)
    with pytest.raises(ValueError, match="finite"):
        ft.temporal_select(head, pos, torch.tensor([float("inf")]), [], min_scale=0.01)
