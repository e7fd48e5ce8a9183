"""Sparse Adam, host side (no GPU): tests/sparse_adam_math.py pinned against torch.optim.SparseAdam and the dense oracle, the C ABI of
gsrast_adam_step_visible (declared, exported, every argument error refused before any device call), and GaussianAdam.step(visibility=)'s
refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sparse_adam_math as sam
from test_adam import LRS, SHAPES, _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_math_matches_torch_sparse_adam():
    """50 rows of width 3, lr 1e-2, eps 1e-15, 5 steps, a fresh 30 % mask each step.  The one difference is where eps is added (there
    sqrt(v) + eps before the bias correction, here after it): 1e-8 absolute on the parameters (this seed: 4.2e-9 at |p| <= 2.6)."""
    P, W, steps, lr = 50, 3, 5, 1e-2
    rng = np.random.default_rng(11)
    p0 = rng.normal(size=(P, W))
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SparseAdam([tp], lr=lr, eps=1e-15)
    p, m, v = p0.copy(), np.zeros((P, W)), np.zeros((P, W))
    seen = np.zeros(P, bool)
    for t in range(1, steps + 1):
        vis = rng.random(P) < 0.3
        g = rng.normal(size=(P, W)) * 10.0 ** rng.uniform(-6, 0, size=(P, 1))
        idx = np.nonzero(vis)[0]
        tp.grad = torch.sparse_coo_tensor(torch.from_numpy(idx[None, :]), torch.from_numpy(g[idx]), size=(P, W)).coalesce()
        opt.step()
        p, m, v = sam.step(p, g, m, v, lr, t, vis)
        seen |= vis
    assert seen.any() and not seen.all()      # (seed 11: some rows are never drawn)
    d = np.abs(p - tp.detach().numpy()).max()
    print("max |p - SparseAdam| =", d, " max |p| =", np.abs(p).max())
    assert d <= 1e-8
    assert np.array_equal(p[~seen], p0[~seen]) and not m[~seen].any() and not v[~seen].any()


def test_all_true_mask_is_the_dense_oracle():
    from oracle import adam_oracle
    P, steps = 300, 4
    params, grads = _data(P, 1, steps)
    inv = 1.0 + 4.0 * np.random.default_rng(3).random(P)
    for k in SHAPES:
        lr = LRS[k] * inv if k != "f_rest" else LRS[k]
        a = (params[k].astype(np.float64), np.zeros(params[k].shape), np.zeros(params[k].shape))
        b = a
        for t in range(steps):
            a = adam_oracle.step(a[0], grads[t][k], a[1], a[2], lr, t + 1)
            b = sam.step(b[0], grads[t][k], b[1], b[2], lr, t + 1, np.ones((P, 1), np.uint8))
        for x, y in zip(a, b):
            assert np.array_equal(x, y), k


def test_all_false_step_changes_nothing_but_counts():
    """The global step count: after one all-false step the next, all-true one is the dense oracle's step t = 2, not t = 1."""
    from oracle import adam_oracle
    P = 40
    params, grads = _data(P, 5, 2)
    for k in ("xyz", "f_rest"):
        p0, z = params[k].astype(np.float64), np.zeros(params[k].shape)
        bad = np.full(params[k].shape, np.nan)
        s1 = sam.step(p0, bad, z, z, np.full(P, np.inf), 1, np.zeros(P, bool))
        assert all(np.array_equal(x, y) for x, y in zip(s1, (p0, z, z)))
        s2 = sam.step(*s1[:1], grads[1][k], s1[1], s1[2], LRS[k], 2, np.ones(P, bool))
        want = adam_oracle.step(p0, grads[1][k], z, z, LRS[k], 2)
        not_want = adam_oracle.step(p0, grads[1][k], z, z, LRS[k], 1)
        assert all(np.array_equal(x, y) for x, y in zip(s2, want))
        assert not np.array_equal(s2[0], not_want[0])


def test_mask_conventions():
    assert sam.visible_rows(np.array([0, 1, 255], np.uint8)).tolist() == [False, True, True]
    assert sam.visible_rows(np.array([[-1], [0], [1], [37]], np.int32)).tolist() == [False, False, True, True]
    assert sam.visible_rows(np.array([True, False])).tolist() == [True, False]


def test_symbol_is_declared_and_exported(rast):
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    raw = C.CDLL(rast._C.LIB_PATH)
    n = "gsrast_adam_step_visible"
    assert re.search(r"\b" + n + r"\s*\(", text)
    assert n in rast._C.EXPORTS and hasattr(raw, n)
    assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == 10
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert C.sizeof(rast._C.AdamGroupStruct) == 5 * C.sizeof(C.c_void_p) + C.sizeof(C.c_float) + 2 * C.sizeof(C.c_int) + 4      # unchanged (+ tail padding)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert "adam_step_visible" in names and names.index("adam_step_visible") < 31      # a bit of the "profile" option's word


def test_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 16      # any non-NULL value: never dereferenced on the host
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731
    GS = _C.AdamGroupStruct

    def call(groups, visible=one, elem=1, rows=10, n_groups=None, b1=0.9, b2=0.999, step=1):
        arr = (GS * max(len(groups), 1))(*groups)
        return L.gsrast_adam_step_visible(len(groups) if n_groups is None else n_groups, arr, visible, elem, rows, b1, b2, 1e-15, step, None)

    grp = lambda rows=10, width=3, param=one: GS(param, one, one, one, None, 1e-3, rows, width)  # noqa: E731
    assert call([grp()], visible=None) == -1 and "NULL visible" in err()
    for elem in (3, 0, 2, 8):
        assert call([grp()], elem=elem) == -1 and "visible_elem_bytes must be 1 or 4" in err()
    assert call([grp()], rows=-1) == -1 and "rows out of range" in err()
    assert call([grp(), grp(rows=9)]) == -1 and "rows differ" in err()
    assert call([grp()], step=0) == -1 and "step >= 1" in err()
    # what gsrast_adam_step refuses
    assert call([grp()] * 9) == -1 and "at most 8 groups" in err()
    assert call([grp()], n_groups=-1) == -1
    assert call([grp()], b1=1.0) == -1 and call([grp()], b2=-0.1) == -1
    assert call([grp(width=0)]) == -1 and "bad group shape" in err()
    assert call([grp(width=(1 << 24) + 1)]) == -1 and "bad group shape" in err()
    assert call([grp(param=None)]) == -1 and "NULL tensor" in err()
    assert L.gsrast_adam_step_visible(1, None, one, 1, 10, 0.9, 0.999, 1e-15, 1, None) == -1
    # nothing to launch: OK without a device
    assert call([]) == 0 and call([], visible=None, rows=0) == 0
    assert call([grp(rows=0)], rows=0) == 0 and call([grp(rows=0), grp(rows=0, width=45)], visible=None, rows=0, elem=4) == 0


def _cpu_optimizer(P=4):
    import fused_adam
    ps = {k: torch.zeros((P,) + s, requires_grad=True) for k, s in SHAPES.items()}
    opt = fused_adam.GaussianAdam([{"params": [ps[k]], "lr": LRS[k], "name": k} for k in SHAPES], eps=1e-15)
    for p in ps.values():
        p.grad = torch.ones_like(p)
    return opt


def test_python_refusals_need_no_device(monkeypatch):
    import fused_adam
    monkeypatch.setattr(fused_adam._C, "lib", lambda: pytest.fail("a refusal reached the library"))
    opt = _cpu_optimizer(4)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        opt.step(visibility=torch.ones(4, dtype=torch.bool))
    for bad in (torch.ones(4), torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.int64), torch.ones(4, dtype=torch.int16)):
        with pytest.raises(RuntimeError, match="torch.bool, torch.uint8 or torch.int32"):
            opt.step(visibility=bad)
    for bad in (torch.ones(5, dtype=torch.bool), torch.ones(3, 1, dtype=torch.int32), torch.ones(0, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="rows, the visibility mask"):
            opt.step(visibility=bad)
    for bad in (torch.ones(2, 2, dtype=torch.bool), torch.ones(4, 1, 1, dtype=torch.bool), torch.tensor(True)):
        with pytest.raises(RuntimeError, match=r"shape \[P\] or \[P, 1\]"):
            opt.step(visibility=bad)
    with pytest.raises(TypeError):
        opt.step(torch.ones(4, dtype=torch.bool))       # keyword-only
    assert opt._step == 0                                # a refused step does not count


def test_groups_without_a_gradient_are_skipped_and_the_step_counts():
    opt = _cpu_optimizer(4)
    opt.zero_grad()
    opt.step(visibility=torch.ones(4, dtype=torch.bool))        # no group has a gradient: nothing to launch, as step()
    opt.step()
    assert opt._step == 2 and not opt.state
