"""Exact k-nearest-neighbour query on the device, with indices: the drop-in for `mmcv.ops.knn`, the un-vendored dependency the
reference imports at helper_model.py:27 and calls as knn(2, xyz, xyz, False) at :150, :207 and :354 (saro-gs_amd/mmcv is the
import-path shim over this module).

knn_query(ref [N,3], query [M,3] or None, k) -> (idx int32 [k, M], dist2 float32 [k, M] or None)      one cloud
knn(k, xyz, center_xyz=None, transposed=False) -> int32 [B, k, npoint]                                mmcv's signature and result

For every query the k reference points with the smallest (d2, index), ascending; d2 is the kernel's fp32 (dx dx + dy dy) + dz dz; equal
d2 puts the lower index first; a point is its own neighbour in a self-query (slot 0: itself, or a duplicate with a lower index); slots
beyond the reference's size hold -1 / +inf.  Non-finite coordinates are unsupported.  HIP implementation in libgsrast_hip.so
(`gsrast_knn_query`, csrc/gsrast_knn_query.h; semantics in include/gsrast.h).  No CPU fallback."""
from typing import Optional, Tuple

import torch

from diff_gaussian_rasterization_ch3 import _C as _lib

MAX_K = 32


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k must be an integer in 1..{MAX_K} (got {k!r})")
    return k


def _cloud(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"knn: {name} must be a tensor on a GPU (HIP) device; there is no CPU fallback")
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"knn: {name} must be [N, 3] (got {tuple(t.shape)})")
    return t.detach().contiguous().float()


def knn_query(ref: torch.Tensor, query: Optional[torch.Tensor] = None, k: int = 1,
              return_dist2: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(idx int32 [k, M], dist2 float32 [k, M] or None) of one cloud; query=None: the reference queries itself (M = N)."""
    k = _check_k(k)
    r = _cloud(ref, "ref")
    q = None if query is None else _cloud(query, "query")
    if q is not None and q.device != r.device:
        raise RuntimeError("knn: ref and query must be on the same device")
    N, M = int(r.shape[0]), int(r.shape[0] if q is None else q.shape[0])
    idx = torch.empty((k, M), dtype=torch.int32, device=r.device)
    dist2 = torch.empty((k, M), dtype=torch.float32, device=r.device) if return_dist2 else None
    if M == 0:
        return idx, dist2
    scratch = torch.empty(_lib.lib().gsrast_knn_query_scratch_bytes(N, M), dtype=torch.uint8, device=r.device)
    _lib.launch("gsrast_knn_query", r.device, N, _lib._ptr(r), M, None if q is None else q.data_ptr(), k, idx.data_ptr(),
                None if dist2 is None else dist2.data_ptr(), scratch.data_ptr())
    return idx, dist2


def _same_storage(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a is b) or (a.device == b.device and a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
                        and a.data_ptr() == b.data_ptr())


def knn(k: int, xyz: torch.Tensor, center_xyz: Optional[torch.Tensor] = None, transposed: bool = False) -> torch.Tensor:
    """mmcv.ops.knn: for every point of center_xyz (B, npoint, 3) its k nearest points of xyz (B, N, 3), as int32 ids (B, k, npoint);
    both (B, 3, .) when `transposed`.  center_xyz None, or the same storage as xyz: the cloud queries itself.  The result does not
    require grad.  k > N raises ValueError (mmcv returns meaningless zeros there)."""
    k = _check_k(k)
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise RuntimeError("knn: xyz must be a tensor on a GPU (HIP) device; there is no CPU fallback")
    self_query = center_xyz is None or _same_storage(xyz, center_xyz)
    if not self_query and (not isinstance(center_xyz, torch.Tensor) or not center_xyz.is_cuda):
        raise RuntimeError("knn: center_xyz must be a tensor on a GPU (HIP) device; there is no CPU fallback")
    clouds = [xyz] if self_query else [xyz, center_xyz]
    for name, t in zip(("xyz", "center_xyz"), clouds):
        if t.dim() != 3 or t.shape[1 if transposed else 2] != 3:
            raise RuntimeError(f"knn: {name} must be {'(B, 3, N)' if transposed else '(B, N, 3)'} (got {tuple(t.shape)})")
    if not self_query and center_xyz.shape[0] != xyz.shape[0]:
        raise RuntimeError("knn: xyz and center_xyz must have the same batch size")
    if transposed:
        clouds = [t.transpose(1, 2) for t in clouds]
    B, N = int(clouds[0].shape[0]), int(clouds[0].shape[1])
    if k > N:
        raise ValueError(f"knn: k = {k} exceeds the {N} points of xyz")
    npoint = N if self_query else int(clouds[1].shape[1])
    out = torch.empty((B, k, npoint), dtype=torch.int32, device=xyz.device)
    for b in range(B):
        out[b] = knn_query(clouds[0][b], None if self_query else clouds[1][b], k, return_dist2=False)[0]
    return out
