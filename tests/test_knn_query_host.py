"""The k-NN index query (include/gsrast.h: gsrast_knn_query; saro-gs_amd/fused_knn.py; the mmcv.ops shim) without a GPU: the fp64 brute
force the GPU tests measure against on hand-checkable inputs, the scratch size, the refusals that come before any launch, the shim."""
import numpy as np
import pytest
import torch

import knn_query_math as km


def test_brute_force_four_points_on_a_line():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0]], np.float64)
    idx, d2 = km.brute_force(pts, None, 3)
    assert idx.T.tolist() == [[0, 1, 2], [1, 0, 2], [2, 1, 0], [3, 2, 1]]          # a point is its own nearest neighbour
    assert d2.T.tolist() == [[0, 1, 9], [0, 1, 4], [0, 4, 9], [0, 16, 36]]
    idx, d2 = km.brute_force(pts, np.array([[2.5, 0, 0]]), 2)                       # another query set
    assert idx[:, 0].tolist() == [2, 1] and d2[:, 0].tolist() == [0.25, 2.25]


def test_brute_force_duplicate_pair_and_index_tie():
    pts = np.array([[5, 5, 5], [0, 0, 0], [5, 5, 5], [1, 0, 0], [-1, 0, 0]], np.float64)
    idx, d2 = km.brute_force(pts, None, 2)
    assert idx[:, 0].tolist() == [0, 2] and idx[:, 2].tolist() == [0, 2]            # slot 0 of row 2 is its duplicate with the lower index
    assert d2[:, 0].tolist() == [0, 0] and d2[:, 2].tolist() == [0, 0]
    idx, d2 = km.brute_force(pts, None, 3)
    assert idx[:, 1].tolist() == [1, 3, 4] and d2[:, 1].tolist() == [0, 1, 1]       # (1,0,0) and (-1,0,0) tie: the lower index first
    idx, _ = km.brute_force(pts[[1, 4, 3]], None, 3)
    assert idx[:, 0].tolist() == [0, 1, 2]                                          # the same tie with the rows swapped: still by index


def test_brute_force_fills_missing_slots():
    pts = np.array([[0, 0, 0], [0, 2, 0]], np.float64)
    idx, d2 = km.brute_force(pts, None, 4)
    assert idx.T.tolist() == [[0, 1, -1, -1], [1, 0, -1, -1]]
    assert d2[:2].T.tolist() == [[0, 4], [0, 4]] and np.isposinf(d2[2:]).all()
    idx, d2 = km.brute_force(np.zeros((0, 3)), pts, 2)
    assert (idx == -1).all() and np.isposinf(d2).all() and idx.shape == (2, 2)


def test_brute_force_rounds_the_inputs_to_fp32_first():
    a = np.array([[0.1, 0.2, 0.3], [16777217.0, 0, 0]], np.float64)                 # 2^24 + 1 is not an fp32
    _, d2 = km.brute_force(a, np.zeros((1, 3)), 2)
    x = np.float32(0.1).astype(np.float64), np.float32(0.2).astype(np.float64), np.float32(0.3).astype(np.float64)
    assert d2[0, 0] == x[0] * x[0] + x[1] * x[1] + x[2] * x[2] and d2[1, 0] == 16777216.0 ** 2


def test_ambiguity_mask():
    d = np.array([[0.0, 1.0, 1.0], [0.0, 1.0 + 1e-6, 1.0], [2.0, 1.1, 1.0 + 1e-5], [np.inf, np.inf, 3.0]])
    assert km.ambiguous(d).tolist() == [False, True, False]                         # an exact tie (gap 0) and a missing slot are not ambiguous


def test_scratch_bytes_is_pure_host_code(rast):
    L = rast._C.lib()
    f = L.gsrast_knn_query_scratch_bytes
    sizes = (0, 1, 1000, 1024, 1025, 100_000, 3_000_000)
    table = [[f(r, q) for q in sizes] for r in sizes]
    assert all(v > 0 and v % 256 == 0 for row in table for v in row)
    assert all(b >= a for row in table for a, b in zip(row, row[1:]))               # non-decreasing in n_query
    assert all(b >= a for col in zip(*table) for a, b in zip(col, col[1:]))         # ... and in n_ref
    assert f(100_000, 0) > f(1000, 0) and f(0, 100_000) > f(0, 1000)
    assert f(1000, 1000) >= 1000 * (16 + 16) + 1000 * 16                            # the reference's sort pairs, its records, the queries' sort pairs
    assert f(-5, 10) == f(0, 10) and f(10, -5) == f(10, 0) and f(-1, -1) == f(0, 0)  # negative sizes count as 0 (include/gsrast.h)


def test_c_entry_point_refuses_bad_arguments_before_any_device_work(rast):
    L = rast._C.lib()
    q = L.gsrast_knn_query
    for args, text in (((-1, 16, 4, 16, 2, 16, 16, 16, None), b"bad size"), ((4, 16, -1, 16, 2, 16, 16, 16, None), b"bad size"),
                       ((4, 16, 4, 16, 0, 16, 16, 16, None), b"k must be"), ((4, 16, 4, 16, 33, 16, 16, 16, None), b"k must be"),
                       ((4, 16, 4, 16, 2, None, 16, 16, None), b"NULL idx"), ((4, None, 4, 16, 2, 16, 16, 16, None), b"NULL pointer"),
                       ((4, 16, 4, 16, 2, 16, 16, None, None), b"NULL pointer"), ((4, 16, 5, None, 2, 16, 16, 16, None), b"n_query must be n_ref")):
        assert q(*args) == -1 and text in L.gsrast_last_error(), args
    assert q(4, None, 0, None, 2, None, None, None, None) == 0                      # n_query = 0: OK, nothing is touched
    assert rast._C.ABI_VERSION == 6 and L.gsrast_abi_version() == 6                  # additive: the version stays


def test_python_entry_points_raise_before_any_launch(monkeypatch, rast):
    import fused_knn
    monkeypatch.setattr(rast._C, "launch", lambda *a, **k: pytest.fail("a launch was attempted"))
    x = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused_knn.knn_query(x, None, 2)                                             # a CPU tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused_knn.knn(2, x[None], x[None], False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused_knn.knn(2, x[None])
    for k in (0, 33, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="1..32"):
            fused_knn.knn_query(x, None, k)
        with pytest.raises(ValueError, match="1..32"):
            fused_knn.knn(k, x[None], x[None])
    with pytest.raises(RuntimeError):
        fused_knn.knn_query(torch.zeros(10, 2), None, 2)
    with pytest.raises(RuntimeError):
        fused_knn.knn_query(torch.zeros(3, 10, 3), None, 2)
    with pytest.raises(RuntimeError):
        fused_knn.knn(2, torch.zeros(10, 3))


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on a GPU: the shape and k checks BEHIND the device check, still without a device."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_shape_and_k_checks_behind_the_device_check(monkeypatch, rast):
    import fused_knn
    monkeypatch.setattr(rast._C, "launch", lambda *a, **k: pytest.fail("a launch was attempted"))
    g = lambda *shape: _OnGpu(torch.zeros(*shape))  # noqa: E731
    with pytest.raises(RuntimeError, match=r"\[N, 3\]"):
        fused_knn.knn_query(g(10, 2), None, 2)
    with pytest.raises(RuntimeError, match=r"\[N, 3\]"):
        fused_knn.knn_query(g(10, 3), g(3, 4, 3), 2)
    with pytest.raises(RuntimeError, match=r"\(B, N, 3\)"):
        fused_knn.knn(2, g(10, 3))
    with pytest.raises(RuntimeError, match=r"\(B, N, 3\)"):
        fused_knn.knn(2, g(1, 3, 10), g(1, 3, 10), False)                           # the transposed layout without the flag
    with pytest.raises(RuntimeError, match=r"\(B, 3, N\)"):
        fused_knn.knn(2, g(1, 10, 3), g(1, 10, 3), True)
    with pytest.raises(RuntimeError, match="batch"):
        fused_knn.knn(2, g(2, 10, 3), g(1, 5, 3))
    with pytest.raises(ValueError, match="exceeds"):
        fused_knn.knn(5, g(1, 4, 3), g(1, 9, 3))                                    # k > N: mmcv returns meaningless zeros, this raises
    with pytest.raises(ValueError, match="exceeds"):
        fused_knn.knn(5, g(1, 3, 4), None, True)


def test_the_shim_provides_knn_and_says_what_it_is():
    import fused_knn
    import mmcv
    import mmcv.ops
    from mmcv.ops import knn
    assert knn is fused_knn.knn and mmcv.ops.knn is fused_knn.knn
    assert mmcv.__version__ == "0+gsrast.shim" and mmcv.ops.__all__ == ["knn"]
    with pytest.raises(AttributeError, match=r"shim.*mmcv\.ops\.knn"):
        mmcv.ops.ball_query
    with pytest.raises(AttributeError, match=r"shim.*mmcv\.ops\.knn"):
        mmcv.Config
    with pytest.raises(ImportError):
        from mmcv.ops import ball_query  # noqa: F401


def test_binding_table_lists_the_two_entry_points(rast):
    S = rast._C.SIGNATURES
    assert "gsrast_knn_query" in S and "gsrast_knn_query_scratch_bytes" in S and len(S["gsrast_knn_query"][1]) == 9
