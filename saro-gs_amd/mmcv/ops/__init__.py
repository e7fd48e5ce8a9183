"""`from mmcv.ops import knn` -- the same import path and call as the reference (helper_model.py:27; knn(2, xyz, xyz, False) at :150,
:207, :354).  The function is fused_knn.knn (HIP, libgsrast_hip.so: gsrast_knn_query); nothing else of mmcv.ops exists here."""
from fused_knn import knn

__all__ = ["knn"]


def __getattr__(name):
    raise AttributeError(f"mmcv.ops.{name}: this `mmcv` is the gsrast shim (saro-gs_amd/mmcv), which provides mmcv.ops.knn and nothing else")
