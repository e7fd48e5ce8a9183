"""TEST INFRASTRUCTURE ONLY: exact 3-nearest-neighbour mean squared distance in fp64 (scipy cKDTree), the quantity
`simple_knn._C.distCUDA2` returns (graphdeco-inria/simple-knn as shipped with 3DGS: `(best[0] + best[1] + best[2]) / 3`
over squared distances to the three nearest OTHER indices).  simple_knn is an un-vendored dependency of the reference
(/root/reference/scene/saro_gaussian.py:21) and is not in this container: parity unpinned against its binary; the search is
exact, so any exact 3-NN is the same function up to fp32 rounding (fewer than 4 points: see mean_dist2)."""
import numpy as np
from scipy.spatial import cKDTree


FLT_MAX = np.float32(3.402823466e38)


def mean_dist2(points: np.ndarray) -> np.ndarray:
    """P >= 4: the exact fp64 value.  P < 4: what the published algorithm's arithmetic gives -- its three best distances start at
    FLT_MAX and a missing neighbour leaves that in place, so the fp32 mean is inf for P = 1 and 2 (FLT_MAX + FLT_MAX overflows) and
    (d1 + d2 + FLT_MAX) / 3 ~ 1.13e38 for P = 3: large and finite or infinite, never NaN."""
    pts = np.asarray(points, np.float64)
    P = pts.shape[0]
    if P < 4:
        out = np.empty(P, np.float64)
        for i in range(P):
            d2 = np.sort(((np.delete(pts, i, axis=0) - pts[i]) ** 2).sum(axis=1)).astype(np.float32)
            best = np.concatenate([d2, np.full(3 - d2.size, FLT_MAX, np.float32)])
            with np.errstate(over="ignore"):
                out[i] = (best[0] + best[1] + best[2]) / np.float32(3.0)       # fp32, in the kernel's order
        return out
    d, _ = cKDTree(pts).query(pts, k=4)          # column 0 is the point itself (distance 0)
    d2 = np.sort(d ** 2, axis=1)[:, 1:]
    return d2.sum(axis=1) / 3.0
