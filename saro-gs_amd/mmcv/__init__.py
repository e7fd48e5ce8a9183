"""Import-path shim for the reference's un-vendored `mmcv` dependency, of which it uses one function: `from mmcv.ops import knn`
(helper_model.py:27).  NOT mmcv: for machines where the real package is absent (it needs CUDA).  A user who has the real package should
take this directory off their path."""
__version__ = "0+gsrast.shim"

from . import ops  # noqa: F401


def __getattr__(name):
    raise AttributeError(f"mmcv.{name}: this `mmcv` is the gsrast shim (saro-gs_amd/mmcv), which provides mmcv.ops.knn and nothing else")
