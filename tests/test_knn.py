"""simple_knn._C.distCUDA2 (second item).  CPU: the oracle on hand-checkable inputs.
GPU (-m gpu): the HIP implementation against the exact fp64 3-NN oracle, to a purely RELATIVE bar (the compared quantity is a squared
nearest-neighbour distance: an absolute term sized by the coordinates passes zeros on clustered or offset clouds)."""
import numpy as np
import pytest
import torch


def test_oracle_known_answers():
    from oracle import knn_oracle
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [10, 10, 10]], np.float64)
    got = knn_oracle.mean_dist2(pts)
    np.testing.assert_allclose(got[0], (1 + 4 + 9) / 3.0)
    np.testing.assert_allclose(got[1], (1 + 5 + 10) / 3.0)
    np.testing.assert_allclose(got[4], (300 - 60 + 9 + 300 - 40 + 4 + 300 - 20 + 1) / 3.0)   # to (0,0,3), (0,2,0), (1,0,0)


def test_oracle_fewer_than_four_points():
    """A missing neighbour counts as FLT_MAX before the fp32 mean (the published algorithm's arithmetic): inf, inf, ~1.13e38."""
    from oracle import knn_oracle
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float64)
    assert np.isposinf(knn_oracle.mean_dist2(pts[:1])).all() and np.isposinf(knn_oracle.mean_dist2(pts[:2])).all()
    got = knn_oracle.mean_dist2(pts)
    fmax = np.float32(3.402823466e38)
    assert got.shape == (3,) and np.isfinite(got).all()
    assert got[0] == float((np.float32(1) + np.float32(4) + fmax) / np.float32(3)) and 1.13e38 < got[0] < 1.14e38
    assert knn_oracle.mean_dist2(np.vstack([pts, [[0, 0, 3]]]))[0] == (1 + 4 + 9) / 3.0          # four points: the exact mean again


def _clouds():
    rng = np.random.default_rng(7)
    yield "uniform_5k", rng.uniform(-1.3, 1.3, size=(5000, 3))
    yield "clustered", np.concatenate([rng.normal(c, 0.01, size=(700, 3)) for c in rng.uniform(-5, 5, size=(9, 3))])
    dup = rng.uniform(0, 1, size=(1500, 3)); dup[500:1000] = dup[:500]                       # exact duplicates: distance 0 counts
    yield "duplicates", dup
    line = np.zeros((3000, 3)); line[:, 0] = np.sort(rng.uniform(0, 100, 3000))              # degenerate bounding box (two flat axes)
    yield "collinear", line
    yield "tiny_4", rng.normal(size=(4, 3))
    yield "uniform_200k", rng.uniform(-50, 50, size=(200_000, 3))
    yield "boxes_edge_1025", rng.uniform(0, 1, size=(1025, 3))
    # barely more than the three neighbours; one point short of a box of 1024, one box exactly, two boxes plus one point (1025 stands above)
    for P in (5, 1023, 1024, 2049):
        yield f"uniform_P{P}", rng.uniform(-1, 1, size=(P, 3))
    yield "offset_4096", rng.uniform(0, 1, size=(6000, 3)) + 4096.0                          # differences cancel exactly (Sterbenz)
    centres = rng.uniform(-1, 1, size=(8, 3)); centres *= 100.0 / np.abs(centres).max(axis=1, keepdims=True)
    yield "two_scales", np.concatenate([rng.normal(c, 1e-4, size=(500, 3)) for c in centres])  # sigma 1e-4 at |coord| ~ 100
    plane = rng.uniform(-3, 3, size=(5000, 3)); plane[:, 2] = 0.625
    yield "plane", plane
    yield "all_identical", np.tile(rng.normal(size=(1, 3)), (2000, 1))                       # every extent 0, every Morton code 0
    g = np.arange(16, dtype=np.float64)
    yield "lattice", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)        # exact ties; every value is exactly 1
    yield "outlier_squeeze", np.concatenate([rng.uniform(0, 1, size=(5000, 3)), np.full((1, 3), 1e6)])   # all Morton codes but one collapse


@pytest.mark.gpu
@pytest.mark.parametrize("name,pts", list(_clouds()), ids=[n for n, _ in _clouds()])
def test_hip_knn_matches_exact_oracle(name, pts, gpu):
    from oracle import knn_oracle
    from simple_knn._C import distCUDA2
    p32 = pts.astype(np.float32)
    got = distCUDA2(torch.from_numpy(p32).to(gpu)).cpu().numpy().astype(np.float64)
    want = knn_oracle.mean_dist2(p32.astype(np.float64))
    # Purely relative, rtol 2e-6.  The inputs are fp32, so each coordinate difference is ONE rounding (relative to the difference itself,
    # exact where the coordinates are close: Sterbenz); each square and each of the two sums of one distance is one more; the mean is three
    # more (two sums, one division): below 10 * 2^-24 ~ 6e-7 in all.  FMA contraction would only remove roundings.  Choosing differently
    # among near-ties changes the value by no more than the tie's own gap, which is of that size.  2e-6 leaves a factor of three.
    # Where the oracle is exactly 0 (coincident points) so is the result.
    assert not got[want == 0.0].any()
    if name == "all_identical":
        assert not want.any()
    if name == "lattice":
        assert (want == 1.0).all()
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
    # and it feeds the reference's initialisation as written (scene/saro_gaussian.py:187-189)
    d2 = torch.clamp_min(torch.from_numpy(got), 0.0000001)
    assert torch.isfinite(torch.log(torch.sqrt(d2))).all()


@pytest.mark.gpu
def test_hip_knn_is_independent_of_the_input_order(gpu):
    """The three distances are summed in sorted order, each computed from the same two fp32 points: shuffling the rows of the input gives
    the same bits, shuffled."""
    from simple_knn._C import distCUDA2
    pts = dict(_clouds())["clustered"].astype(np.float32)
    perm = np.random.default_rng(11).permutation(pts.shape[0])
    a = distCUDA2(torch.from_numpy(pts).to(gpu)).cpu().numpy()
    b = distCUDA2(torch.from_numpy(pts[perm]).to(gpu)).cpu().numpy()
    assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 3])
def test_hip_knn_fewer_than_four_points(P, gpu):
    """A missing neighbour counts as FLT_MAX before the mean: inf, inf, (d1 + d2 + FLT_MAX) / 3 in fp32 (the oracle says the same)."""
    from oracle import knn_oracle
    from simple_knn._C import distCUDA2
    p32 = np.random.default_rng(13).normal(size=(P, 3)).astype(np.float32)
    got = distCUDA2(torch.from_numpy(p32).to(gpu)).cpu()
    want = knn_oracle.mean_dist2(p32.astype(np.float64))
    assert np.isposinf(want).all() if P < 3 else ((want > 1.13e38) & (want < 1.14e38)).all()
    assert np.array_equal(got.numpy().astype(np.float64), want)
    assert not torch.isnan(torch.log(torch.sqrt(torch.clamp_min(got, 0.0000001)))).any()      # scene/saro_gaussian.py:187-189


@pytest.mark.gpu
def test_hip_knn_argument_errors(gpu):
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros(10, 3))                      # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        distCUDA2(torch.zeros(10, 2, device=gpu))
    assert distCUDA2(torch.zeros(0, 3, device=gpu)).numel() == 0
