"""The differentiable row selection, host side (no GPU): the numpy restatement of tests/select_math.py against torch.autograd of the indexing
expressions it replaces, the new C ABI entry point declared, exported and bound without a version bump or a profile name, and every refusal of
gsrast_densify_scatter and of the Python surface that needs no launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import select_math as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (3,), (15, 3), (64,)]


@pytest.mark.parametrize("name", sm.PATTERNS)
@pytest.mark.parametrize("P", [0, 1, 257, 700])
def test_restatement_equals_torch_indexing_and_its_autograd(P, name):
    keep = sm.pattern(name, P, seed=P)
    n, mask = int(keep.sum()), torch.from_numpy(keep)
    idx = torch.from_numpy(sm.rows(keep)).long()
    assert np.array_equal(sm.rows(keep), mask.nonzero().reshape(-1).numpy()) and sm.rows(keep).dtype == np.int32
    rng = np.random.default_rng(P + 1)
    for shape in SHAPES:
        x, g_n = rng.standard_normal((P,) + shape).astype(np.float32), rng.standard_normal((n,) + shape).astype(np.float32)
        y, g_P = rng.standard_normal((n,) + shape).astype(np.float32), rng.standard_normal((P,) + shape).astype(np.float32)
        xt, yt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
        got = xt[mask]
        got.backward(torch.from_numpy(g_n))
        assert np.array_equal(sm.gather(x, keep), got.detach().numpy()) and np.array_equal(sm.gather_vjp(g_n, keep), xt.grad.numpy())
        z = torch.zeros((P,) + shape).index_copy(0, idx, yt)
        z.backward(torch.from_numpy(g_P))
        assert np.array_equal(sm.scatter(y, keep), z.detach().numpy()) and np.array_equal(sm.scatter_vjp(g_P, keep), yt.grad.numpy())
        assert not np.signbit(sm.scatter(y, keep)[~keep]).any()
        # each is the other's transpose: <gather(x), g_n> = <x, scatter(g_n)> term by term
        assert np.array_equal(sm.gather(sm.scatter(y, keep), keep), y)
        assert np.array_equal((sm.gather(x, keep) * g_n).reshape(-1), sm.gather(x * sm.scatter(g_n, keep), keep).reshape(-1))
    r = np.arange(P, dtype=np.int32)
    assert np.array_equal(sm.gather(r, keep), sm.rows(keep))


def test_symbol_is_declared_exported_and_bound(rast):
    """(Every symbol declared, exported and bound with the header's types: tests/test_capi_abi.py.)"""
    L = rast._C.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)
    assert L.gsrast_abi_version() == rast._C.ABI_VERSION == 6
    assert re.search(r"#define\s+GSRAST_ABI_VERSION\s+6\b", text)
    names = [L.gsrast_profile_kernel_name(k).decode() for k in range(L.gsrast_profile_kernel_count())]
    assert len(names) == 34 and not any("scatter" in x for x in names)


def test_scatter_refusals_come_before_any_device_call(rast):
    """Every argument error returns GSRAST_E_ARG (-1) with its text; none of these calls reaches a device (there is none here)."""
    _C = rast._C
    L = _C.lib()
    one = 256      # any non-NULL value: never dereferenced on the host
    GS = _C.DensifyGroupStruct
    err = lambda: L.gsrast_last_error().decode()  # noqa: E731

    def scatter(groups, P=10, counts=(6, 0, 0, 0, 6), n_groups=None, scratch=one, null_groups=False):
        arr = None if null_groups else (GS * max(len(groups), 1))(*groups)
        ch = (C.c_uint * 5)(*counts) if counts is not None else None
        return L.gsrast_densify_scatter(P, scratch, ch, len(groups) if n_groups is None else n_groups, arr, None)

    ok = GS(one, None, None, one, None, None, 3, _C.DENSIFY_COPY)
    assert scatter([ok], P=-1) == -1 and "negative P" in err()
    assert scatter([ok], scratch=None) == -1 and "NULL scratch / counts / groups" in err()
    assert scatter([ok], counts=None) == -1 and "NULL scratch / counts / groups" in err()
    assert scatter([ok], null_groups=True) == -1 and "NULL scratch / counts / groups" in err()
    assert scatter([ok] * 17) == -1 and "at most 16 groups" in err()
    assert scatter([ok], n_groups=-1) == -1 and "at most 16 groups" in err()
    for w in (0, 65, -3):
        assert scatter([GS(one, None, None, one, None, None, w, _C.DENSIFY_COPY)]) == -1 and "width must be in [1, 64]" in err()
    for role in (_C.DENSIFY_XYZ, _C.DENSIFY_SCALING, 7, -1):
        assert scatter([GS(one, None, None, one, None, None, 3, role)]) == -1 and "COPY role" in err()
    for k in (1, 2, 4, 5):      # src_m, src_v, dst_m, dst_v
        args = [one, None, None, one, None, None, 3, _C.DENSIFY_COPY]
        args[k] = one
        assert scatter([GS(*args)]) == -1 and "moments" in err()
    assert scatter([GS(None, None, None, one, None, None, 3, _C.DENSIFY_COPY)]) == -1 and "NULL src" in err()
    assert scatter([GS(one, None, None, None, None, None, 3, _C.DENSIFY_COPY)]) == -1 and "NULL dst" in err()
    assert scatter([GS(None, None, None, None, None, None, 3, _C.DENSIFY_COPY)], counts=(0, 0, 0, 0, 0)) == -1 and "NULL dst" in err()
    for counts in ((6, 1, 0, 0, 7), (6, 0, 1, 1, 8), (6, 0, 0, 1, 6), (6, 0, 0, 0, 7), (6, 0, 0, 0, 5)):
        assert scatter([ok], counts=counts) == -1 and "prune-only plan" in err(), counts
    assert scatter([ok], counts=(11, 0, 0, 0, 11)) == -1 and "n_kept exceeds P" in err()
    assert scatter([ok, GS(one, None, None, one, None, None, 65, _C.DENSIFY_COPY)]) == -1 and "width" in err()      # every group is checked
    # what is valid and needs no device: nothing to launch
    assert scatter([], P=0, counts=None, scratch=None, null_groups=True) == 0
    assert scatter([ok], P=0, counts=(0, 0, 0, 0, 0)) == 0
    assert scatter([], P=10) == 0


def test_python_refusals_that_need_no_launch():
    import fused_densify as fd
    import fused_temporal as ft
    dev = torch.device("cuda:0")
    sel = fd.RowSelection(10, dev, None, (6, 0, 0, 0, 6))      # (no scratch: nothing below reaches a launch)
    assert (sel.P, sel.count, sel.device) == (10, 6, dev)
    with pytest.raises(AttributeError, match="immutable"):
        sel.count = 7
    for call, rows in ((sel.gather, 10), (sel.scatter, 6)):
        with pytest.raises(RuntimeError, match="17 tensors .* at most 16"):
            call(*[torch.zeros(rows, 3)] * 17)
        with pytest.raises(RuntimeError, match="1 ... 64 four-byte elements per row"):
            call(torch.zeros(rows, 65))
        with pytest.raises(RuntimeError, match="1 ... 64 four-byte elements per row"):
            call(torch.zeros(rows, 13, 5))
        with pytest.raises(RuntimeError, match=f"expected {rows} rows"):
            call(torch.zeros(rows + 1, 3))
        with pytest.raises(RuntimeError, match=f"expected {rows} rows"):
            call(torch.zeros(16 - rows, 3))                      # the other side's row count
        for dtype in (torch.float64, torch.float16, torch.int64, torch.bool):
            with pytest.raises(RuntimeError, match="float32 or int32"):
                call(torch.zeros(rows, 3, dtype=dtype))
        with pytest.raises(RuntimeError, match="must be contiguous"):
            call(torch.zeros(3, rows).t())
        for dtype in (torch.float32, torch.int32):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(torch.zeros(rows, 3, dtype=dtype))
        assert call() == ()
    # with a GradArena installed, a gathered leaf's gradient would miss the exchanged bucket: refused like features=
    from diff_gaussian_rasterization_ch3 import _C
    _C.set_grad_arena(object())
    try:
        with pytest.raises(RuntimeError, match="GradArena installed"):
            sel.gather(torch.zeros(10, 3, requires_grad=True))
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # not a leaf that requires a gradient: the ordinary checks
            sel.gather(torch.zeros(10, 3), torch.zeros(10, 3, requires_grad=True) * 2)
    finally:
        _C.set_grad_arena(None)
    with pytest.raises(ValueError, match="exactly one of keep= and dead="):
        fd.select_rows()
    with pytest.raises(ValueError, match="exactly one of keep= and dead="):
        fd.select_rows(keep=torch.zeros(4, dtype=torch.bool), dead=torch.zeros(4, dtype=torch.bool))
    for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="bool or uint8"):
            fd.select_rows(dead=bad)
        with pytest.raises(RuntimeError, match="bool or uint8"):
            fd.select_rows(keep=bad)
    for bad in (torch.zeros(4, 2, dtype=torch.bool), torch.zeros((), dtype=torch.bool), torch.zeros(4, 1, 1, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match=r"\[P\] or \[P, 1\]"):
            fd.select_rows(dead=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        fd.select_rows(keep=torch.ones(4, dtype=torch.bool))
    # temporal_rows: the caller's cull is checked against the head's rows before anything else
    h, p = torch.rand(10, 1), torch.rand(10, 1)
    with pytest.raises(RuntimeError, match="also_dead has 9 entries, expected 10 rows"):
        ft.temporal_rows(h, p, 0.5, min_scale=0.1, also_dead=torch.zeros(9, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="bool or uint8"):
        ft.temporal_rows(h, p, 0.5, min_scale=0.1, also_dead=torch.zeros(10))
    with pytest.raises(RuntimeError, match="GPU"):
        ft.temporal_rows(h, p, 0.5, min_scale=0.1, also_dead=torch.zeros(10, dtype=torch.bool))
