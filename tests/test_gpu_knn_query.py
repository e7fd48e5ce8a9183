"""The k-NN index query on the device (include/gsrast.h: gsrast_knn_query; fused_knn.knn_query / knn; the mmcv.ops shim) against the fp64
brute force of tests/knn_query_math.py over the fp32-rounded inputs.  Sizes are the smallest at which the search can go wrong: a box holds
1024 reference points, a wave 64 queries, a workgroup 256; the list capacities are 2, 4, 8, 16, 32 (k = 1, 2 | 3 | 8 | 16 | 32)."""
import functools

import numpy as np
import pytest
import torch

import knn_query_math as km

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 16, 32)
K_TRUTH = max(KS) + 1          # the truth is computed once per cloud, at 33 ranks, and sliced


def _cloud(name):
    """The clouds of tests/test_knn.py::_clouds (every one from its own seeded generator), fp32."""
    rng = np.random.default_rng([7, sum(name.encode())])
    if name == "uniform_5k":
        p = rng.uniform(-1.3, 1.3, size=(5000, 3))
    elif name == "clustered":
        p = np.concatenate([rng.normal(c, 0.01, size=(700, 3)) for c in rng.uniform(-5, 5, size=(9, 3))])
    elif name == "duplicates":
        p = rng.uniform(0, 1, size=(1500, 3)); p[500:1000] = p[:500]
    elif name == "collinear":
        p = np.zeros((3000, 3)); p[:, 0] = np.sort(rng.uniform(0, 100, 3000))          # a bounding box flat on two axes
    elif name == "offset_4096":
        p = rng.uniform(0, 1, size=(3000, 3)) + 4096.0
    elif name == "plane":
        p = rng.uniform(-3, 3, size=(5000, 3)); p[:, 2] = 0.625
    elif name == "all_identical":
        p = np.tile(rng.normal(size=(1, 3)), (2000, 1))                                 # every extent 0, every Morton code 0
    elif name.startswith("N"):
        p = rng.uniform(-1, 1, size=(int(name[1:]), 3))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, dtype=np.float32)


CLOUDS = ("uniform_5k", "clustered", "duplicates", "collinear", "offset_4096", "plane", "all_identical") + tuple(f"N{n}" for n in (1, 2, 31, 32, 33, 1023, 1024, 1025, 2049))
QUERY_COUNTS = (1, 63, 64, 65, 257)


def _queries(ref, M=None):
    """Every third point, jittered by 1e-3 of the cloud's extent (1e-3 where that is 0); the first M of them."""
    rng = np.random.default_rng(23)
    q = ref[::3][:M].astype(np.float64)
    scale = float((ref.max(axis=0) - ref.min(axis=0)).max()) or 1.0
    return np.ascontiguousarray(q + rng.normal(0, 1e-3 * scale, size=q.shape), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _case(name, separate, M=None):
    """(ref, query or None, truth idx, truth d2) of one cloud; computed once, shared by every k, never written to."""
    ref = _cloud(name)
    query = _queries(ref, M) if separate else None
    ti, td = km.brute_force(ref, query, K_TRUTH)
    for a in (ref, query, ti, td):
        if a is not None:
            a.setflags(write=False)
    return ref, query, ti, td


def _run(gpu, ref, query, k, return_dist2=True):
    from fused_knn import knn_query
    idx, d2 = knn_query(torch.tensor(ref, device=gpu), None if query is None else torch.tensor(query, device=gpu), k, return_dist2)      # (copies: the shared arrays are read-only)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and (d2 is None or (d2.dtype == torch.float32 and d2.shape == idx.shape))
    return idx.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


# ---- 1. the parity grid --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("separate", [False, True], ids=["self", "separate"])
@pytest.mark.parametrize("name", CLOUDS)
def test_parity_grid(name, separate, gpu):
    """Every k on every cloud, the reference querying itself and a jittered third of it querying it.  At most 1 % of a cloud's queries may
    be ambiguous (two consecutive true distances within 4e-6 of each other, where an fp32 search may rank either first): computed from
    the truth alone, these clouds give 0.59 % at worst (N = 1025, k = 32), 0.38 % for uniform 5 000 at k = 32 and 0 at k = 2."""
    ref, query, ti, td = _case(name, separate)
    M = ref.shape[0] if query is None else query.shape[0]
    for k in KS:
        idx, d2 = _run(gpu, ref, query, k)
        amb = km.check_parity(ref, query, k, idx, d2, ti, td)
        assert amb.sum() <= 0.01 * M, (k, int(amb.sum()), M)
        if query is None and name != "all_identical" and name != "duplicates":
            assert np.array_equal(idx[0], np.arange(M)) and not d2[0].any()       # a point is its own nearest neighbour


@pytest.mark.parametrize("M", QUERY_COUNTS)
def test_parity_query_counts(M, gpu):
    """One lane short of a wave, a wave, a wave and a lane, a workgroup and a lane, a single query: the idle lanes of the last wave."""
    ref, query, ti, td = _case("N2049", True, M)
    assert query.shape[0] == M
    for k in KS:
        idx, d2 = _run(gpu, ref, query, k)
        km.check_parity(ref, query, k, idx, d2, ti, td)


# ---- 2. exact-arithmetic clouds: ids compared on every query, no mask ---------------------------------------------------------------

def _lattice():
    g = np.arange(16, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def _two_scales():
    """Eight clusters of 500, sigma 1e-4, every centre coordinate in +-[70, 120]: all coordinates share the fp32 spacing 2^-17 (7.6e-6), so
    inside a cluster (12 sigma across: 160 steps) differences take 8 bits, squares 16 and their sum 18 -- exact in fp32 --, and the 32
    nearest of a point are all in its own cluster (the clusters are tens apart)."""
    rng = np.random.default_rng(29)
    centres = rng.uniform(70, 120, size=(8, 3)) * rng.choice([-1.0, 1.0], size=(8, 3))
    return np.concatenate([rng.normal(c, 1e-4, size=(500, 3)) for c in centres]).astype(np.float32)


@pytest.mark.parametrize("make", [_lattice, _two_scales], ids=["lattice_16", "two_scales"])
def test_exact_clouds_match_the_truth_entry_for_entry(make, gpu):
    """Every d2 among the candidates that matter is exact in fp32, so the fp32 search and the fp64 truth rank identically, ties included:
    the result is lexsort((index, d2))[:k] for every query.  On the lattice ties are everywhere (6 neighbours at 1, 12 at 2, 8 at 3 ...)."""
    ref = make()
    ti, td = km.brute_force(ref, None, max(KS))
    for k in KS:
        idx, d2 = _run(gpu, ref, None, k)
        assert np.array_equal(idx, ti[:k]), k
        assert np.array_equal(d2.astype(np.float64), td[:k]), k


@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_planted_tie_at_a_box_boundary_goes_to_the_lower_index(k, gpu):
    """The query is the origin.  Row 0 is A = (2, 0, 0): distance exactly 2, in a far Morton box.  The last row is B = (0, -2, 0): distance
    exactly 2 as well, in the query's own box together with k - 1 nearer points.  N = 2049 = 1024 rows with x <= 0 (the lower half of the
    grid's x range [-4, 4]: the near points, B and filler at x <= -2.5; box 0) + 1025 with x >= 2 (A and filler; boxes 1 and 2), so the box
    that holds A has the bounding box x >= 2 with y, z spanning 0: its lower bound for the origin is exactly 4 = the k-th distance once
    box 0 has been scanned.  Slot k - 1 must be A: a `>=` rejection of that box returns B."""
    rng = np.random.default_rng(31)
    near = rng.uniform(-1.0, 1.0, size=(k - 1, 3)) * [0.5, 1, 1] - [0.55, 0, 0]            # x in [-1.05, -0.05]: |.| < 1.8
    low = np.concatenate([rng.uniform(-4, -2.5, size=(1024 - k, 1)), rng.uniform(-1, 1, size=(1024 - k, 2))], axis=1)
    high = np.concatenate([rng.uniform(2, 4, size=(1024, 1)), rng.uniform(-1, 1, size=(1024, 2))], axis=1)
    low[0, 0], high[0, 0] = -4.0, 4.0                                                       # the grid is x in [-4, 4]: x = 0 falls in its lower half
    rows = np.concatenate([high, low, near])
    rows = rows[rng.permutation(rows.shape[0])]
    ref = np.concatenate([[[2.0, 0, 0]], rows, [[0, -2.0, 0]]]).astype(np.float32)
    query = np.zeros((1, 3), np.float32)
    assert ref.shape[0] == 2049 and (np.linalg.norm(near, axis=1) < 1.9).all()
    ti, td = km.brute_force(ref, query, k)
    assert ti[k - 1, 0] == 0 and td[k - 1, 0] == 4.0 and (td[:k - 1, 0] < 4.0).all()        # the truth: A, by its index
    idx, d2 = _run(gpu, ref, query, k)
    assert idx[k - 1, 0] == 0 and d2[k - 1, 0] == 4.0
    assert np.array_equal(idx, ti)


# ---- 3. queries outside the reference's bounding box ---------------------------------------------------------------------------------

def test_queries_outside_the_bounding_box(gpu):
    """257 queries at distance 10 .. 1000 from a unit cube of 3 000: every Morton code clamps to a face, an edge or a corner of the grid.
    (From so far away neighbouring ranks are closer than fp32 resolves -- most queries are ambiguous by geometry, so their ids are held
    to the distance bar only; the share of ambiguous queries is not bounded here.)"""
    rng = np.random.default_rng(37)
    ref = rng.uniform(0, 1, size=(3000, 3)).astype(np.float32)
    dirs = rng.normal(size=(257, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1] / np.sqrt(3), [-1, -1, -1] / np.sqrt(3)]
    query = (0.5 + dirs * np.geomspace(10, 1000, 257)[:, None]).astype(np.float32)
    ti, td = km.brute_force(ref, query, K_TRUTH)
    for k in (1, 3, 32):
        idx, d2 = _run(gpu, ref, query, k)
        km.check_parity(ref, query, k, idx, d2, ti, td)


# ---- 4. order independence, 5. repeatability ----------------------------------------------------------------------------------------

def test_order_independence(gpu):
    ref, query, ti, td = _case("clustered", True)
    N, M, k = ref.shape[0], query.shape[0], 8
    amb = km.ambiguous(td[:k + 1])
    idx, d2 = _run(gpu, ref, query, k)
    perm = np.random.default_rng(41).permutation(N)                 # row j of the permuted reference is row perm[j]
    idx_p, d2_p = _run(gpu, ref[perm], query, k)
    assert np.array_equal(d2_p.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(perm[idx_p[:, ~amb]], idx[:, ~amb])
    qperm = np.random.default_rng(43).permutation(M)
    idx_q, d2_q = _run(gpu, ref, query[qperm], k)
    assert np.array_equal(idx_q, idx[:, qperm]) and np.array_equal(d2_q.view(np.uint32), d2[:, qperm].view(np.uint32))
    # the self-query: permuting the cloud permutes the columns; the distances are the same bits
    sref, _, sti, std = _case("clustered", False)
    samb = km.ambiguous(std[:k + 1])
    sidx, sd2 = _run(gpu, sref, None, k)
    sidx_p, sd2_p = _run(gpu, sref[perm], None, k)
    assert np.array_equal(sd2_p.view(np.uint32), sd2[:, perm].view(np.uint32))
    ok = ~samb[perm]
    assert np.array_equal(perm[sidx_p[:, ok]], sidx[:, perm][:, ok])


@pytest.mark.parametrize("separate", [False, True], ids=["self", "separate"])
def test_two_runs_are_bit_identical(separate, gpu):
    ref, query, _, _ = _case("uniform_5k", separate)
    for k in (2, 32):
        a, b = _run(gpu, ref, query, k), _run(gpu, ref, query, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(_run(gpu, ref, query, k, return_dist2=False)[0], a[0])      # ... and without the distances


# ---- 6. fewer reference points than k; empty sets ------------------------------------------------------------------------------------

def test_missing_slots_and_empty_sets(gpu):
    from fused_knn import knn_query
    ref = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 3, 0]], device=gpu)
    idx, d2 = knn_query(ref, None, 5)
    assert idx.cpu().tolist() == [[0, 1, 2], [1, 0, 0], [2, 2, 1], [-1] * 3, [-1] * 3]
    assert d2[:3].cpu().tolist() == [[0, 0, 0], [1, 1, 9], [9, 10, 10]] and torch.isposinf(d2[3:]).all()
    q = torch.tensor([[0.0, 1, 0]] * 70, device=gpu)
    idx, d2 = knn_query(ref, q, 32)
    assert idx.shape == (32, 70) and (idx[:3].cpu() == torch.tensor([[0], [1], [2]])).all() and (idx[3:] == -1).all() and torch.isposinf(d2[3:]).all()
    assert d2[:3, 69].cpu().tolist() == [1, 2, 4]
    idx, d2 = knn_query(ref, torch.zeros((0, 3), device=gpu), 4)                          # n_query = 0
    assert idx.shape == (4, 0) and d2.shape == (4, 0) and idx.dtype == torch.int32
    idx, d2 = knn_query(torch.zeros((0, 3), device=gpu), q, 4)                            # n_ref = 0: every slot is missing
    assert idx.shape == (4, 70) and (idx == -1).all() and torch.isposinf(d2).all()
    idx, d2 = knn_query(torch.zeros((0, 3), device=gpu), None, 4, return_dist2=False)
    assert idx.shape == (4, 0) and d2 is None
    with pytest.raises(ValueError):
        knn_query(ref, None, 33)
    with pytest.raises(RuntimeError):
        knn_query(ref, torch.zeros(4, 3), 2)                                              # a CPU query set


# ---- 7. the reference's call as written, through the shim ----------------------------------------------------------------------------

def _thinning_mask(x, nearest):
    """The points whose nearest neighbour is far: the distance to `nearest`, sorted, the largest N // 4 of them kept (strictly above the
    N // 4-th largest, as the caller of knn(2, xyz, xyz, False) at helper_model.py:150 selects)."""
    d = torch.norm(x - x[nearest], dim=1)
    return (d > torch.sort(d)[0][-(x.shape[0] // 4)]).cpu().numpy()


def test_the_reference_call_through_the_shim(gpu):
    from mmcv.ops import knn
    rng = np.random.default_rng(47)
    pts = rng.uniform(-2, 2, size=(4000, 3)).astype(np.float32)
    ti, td = km.brute_force(pts, None, 3)
    assert not km.ambiguous(td).any() and (td[1] > 0).all()                               # no duplicates, no near-ties: the ids are determined
    xyzinput = torch.from_numpy(pts).float().to(gpu).unsqueeze(0).contiguous()            # 1 x N x 3
    out = knn(2, xyzinput, xyzinput, False)
    assert out.shape == (1, 2, 4000) and out.dtype == torch.int32 and not out.requires_grad and out.device == xyzinput.device
    assert np.array_equal(out[0, 0].cpu().numpy(), np.arange(4000))
    assert np.array_equal(out[0, 1].cpu().numpy(), ti[1])
    x = xyzinput[0]
    want = _thinning_mask(x, torch.from_numpy(ti[1]).to(gpu))
    assert np.array_equal(_thinning_mask(x, out[0, 1].long()), want)
    assert 4000 // 4 - 3 <= want.sum() <= 4000 // 4 - 1              # (strictly above the threshold: it and its mutual neighbour, the same distance, stay out)
    # with duplicates row 0 is not the identity: the lower index comes first
    dup = pts.copy(); dup[3000:] = dup[:1000]
    ti, td = km.brute_force(dup, None, 3)
    assert not km.ambiguous(td).any()
    out = knn(2, torch.from_numpy(dup).to(gpu)[None], None, False)                        # center_xyz None: the same self-query
    assert np.array_equal(out[0].cpu().numpy(), ti[:2])
    assert np.array_equal(out[0, 0, 3000:].cpu().numpy(), np.arange(1000)) and np.array_equal(out[0, 1, :1000].cpu().numpy(), np.arange(3000, 4000))
    with pytest.raises(ValueError):
        knn(5, xyzinput[:, :4], xyzinput)                                                 # k > N


# ---- 8. transposed, batches ----------------------------------------------------------------------------------------------------------

def test_transposed_and_batched(gpu):
    from fused_knn import knn, knn_query
    rng = np.random.default_rng(53)
    xyz = torch.from_numpy(rng.uniform(-1, 1, size=(2, 1500, 3)).astype(np.float32)).to(gpu)
    centre = torch.from_numpy(rng.uniform(-1, 1, size=(2, 300, 3)).astype(np.float32)).to(gpu)
    plain = knn(4, xyz, centre)
    assert plain.shape == (2, 4, 300)
    for b in range(2):
        assert torch.equal(plain[b], knn_query(xyz[b], centre[b], 4)[0])
    assert not torch.equal(plain[0], plain[1])
    assert torch.equal(knn(4, xyz.transpose(1, 2).contiguous(), centre.transpose(1, 2).contiguous(), True), plain)
    assert torch.equal(knn(4, xyz.transpose(1, 2), centre.transpose(1, 2), True), plain)  # (not contiguous)
    own = knn(4, xyz)
    assert own.shape == (2, 4, 1500) and torch.equal(own, knn(4, xyz, xyz)) and torch.equal(own, knn(4, xyz.transpose(1, 2).contiguous(), None, True))
    assert torch.equal(own, knn(4, xyz, xyz.clone()))                                     # another storage: the separate-query path, the same answer
    assert torch.equal(own[:, 0], torch.arange(1500, device=gpu, dtype=torch.int32).expand(2, -1))
    x64 = xyz.double().requires_grad_(True)                                               # converted as distCUDA2 converts; no graph
    assert torch.equal(knn(4, x64), own) and not knn(4, x64).requires_grad


# ---- 9. one mid-size case ------------------------------------------------------------------------------------------------------------

def test_mid_size_against_a_kd_tree(gpu):
    """60 000 uniform points: 59 boxes and 235 workgroups, so more than one box per workgroup and many rejected boxes."""
    spatial = pytest.importorskip("scipy.spatial")
    ref = np.random.default_rng(59).uniform(-10, 10, size=(60_000, 3)).astype(np.float32)
    r64 = km.f32(ref)
    td, ti = spatial.cKDTree(r64).query(r64, k=9)
    td, ti = (td.T) ** 2, ti.T
    for k in (2, 8):
        idx, d2 = _run(gpu, ref, None, k)
        got = idx.astype(np.int64)
        d = r64[None] - r64[got]
        own = (d * d).sum(-1)
        np.testing.assert_allclose(own, td[:k], rtol=km.RTOL, atol=0)                     # (the tree returns the root: its 0 squares to 0)
        np.testing.assert_allclose(d2.astype(np.float64), own, rtol=km.RTOL, atol=0)
        assert np.array_equal(got[0], np.arange(60_000))
        amb = km.ambiguous(td[:k + 1])
        assert amb.sum() <= 0.01 * 60_000 and np.array_equal(got[:, ~amb], ti[:k][:, ~amb])
