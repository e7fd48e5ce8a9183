"""The truth of the k-NN query tests (tests/test_knn_query_host.py, tests/test_gpu_knn_query.py): an fp64 brute force over the
fp32-ROUNDED inputs with the (d2, index) tie rule of include/gsrast.h, and what the tests derive from it."""
import numpy as np

RTOL = 2e-6          # tests/test_knn.py:63-67: a squared distance from fp32 inputs carries below 10 * 2^-24 ~ 6e-7; a factor of three of margin
AMBIGUOUS = 4e-6     # two consecutive true distances closer than this (relatively) may be ranked either way by an fp32 search


def f32(a):
    """The fp32-rounded points as fp64: what the device is given."""
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)


def dist2(ref, query):
    """fp64 squared distances [M, N] of the fp32-rounded points."""
    r, q = f32(ref).reshape(-1, 3), f32(query).reshape(-1, 3)
    d = q[:, None, :] - r[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def brute_force(ref, query=None, k=1, chunk=256):
    """(idx int64 [k, M], d2 float64 [k, M]): for every query (None: the reference itself) the k reference points with the smallest
    (d2, index), ascending; slots j >= N hold -1 / +inf."""
    ref = np.asarray(ref).reshape(-1, 3)
    query = ref if query is None else np.asarray(query).reshape(-1, 3)
    N, M = ref.shape[0], query.shape[0]
    idx = np.full((k, M), -1, np.int64)
    d2 = np.full((k, M), np.inf, np.float64)
    n = min(k, N)
    for m0 in range(0, M, chunk):
        d = dist2(ref, query[m0:m0 + chunk])
        order = np.argsort(d, axis=1, kind="stable")[:, :n]          # stable: equal d2 keeps the lower index first
        idx[:n, m0:m0 + chunk] = order.T
        d2[:n, m0:m0 + chunk] = np.take_along_axis(d, order, axis=1).T
    return idx, d2


def ambiguous(d2_k1):
    """[M] bool from the true distances of ranks 1 .. k + 1 ([k + 1, M]): two consecutive ones satisfy 0 < gap <= AMBIGUOUS * d."""
    with np.errstate(invalid="ignore"):
        gap = d2_k1[1:] - d2_k1[:-1]                                  # (a missing slot, +inf, is not a distance: never ambiguous)
        return ((gap > 0) & np.isfinite(d2_k1[1:]) & (gap <= AMBIGUOUS * d2_k1[1:])).any(axis=0)


def check_parity(ref, query, k, idx, d2, truth_idx, truth_d2):
    """The parity checks of one result (idx, d2: [k, M] arrays from the device) against the truth at k + 1 or more ranks.  Returns the
    [M] mask of ambiguous queries.  For every query and slot: the ids of a query are distinct; the fp64 distance of the returned id equals
    the fp64 j-th smallest distance within RTOL (atol 0; exactly 0 where the truth is 0); the returned dist2 meets the same bar against the
    fp64 distance of the returned id; missing slots are -1 / +inf exactly where the truth's are; on every non-ambiguous query the ids are
    the truth's."""
    ref = np.asarray(ref).reshape(-1, 3)
    query = ref if query is None else np.asarray(query).reshape(-1, 3)
    N, M = ref.shape[0], query.shape[0]
    assert idx.shape == (k, M) and d2.shape == (k, M) and truth_d2.shape[0] >= k + 1
    n = min(k, N)
    assert (idx[n:] == -1).all() and np.isposinf(d2[n:]).all()
    got = idx[:n].astype(np.int64)
    assert ((got >= 0) & (got < N)).all()
    srt = np.sort(got, axis=0)
    assert (srt[1:] != srt[:-1]).all(), "a query returned the same id twice"
    r, q = f32(ref), f32(query)
    d = q[None, :, :] - r[got]                                        # [n, M, 3]
    own = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    want = truth_d2[:n]
    assert not own[want == 0.0].any() and not d2[:n][want == 0.0].any()
    np.testing.assert_allclose(own, want, rtol=RTOL, atol=0)
    np.testing.assert_allclose(d2[:n].astype(np.float64), own, rtol=RTOL, atol=0)
    amb = ambiguous(truth_d2[:k + 1])
    assert np.array_equal(got[:, ~amb], truth_idx[:n][:, ~amb])
    return amb
