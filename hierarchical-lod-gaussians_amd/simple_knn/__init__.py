"""Drop-in `simple_knn` for MI355X: `simple_knn._C.distCUDA2`, the one function of the CUDA-only simple-knn extension
the reference imports (scene/gaussian_model.py:21) and calls (create_from_pcd, :848).
"""
from . import _C
from ._C import distCUDA2  # noqa: F401

__all__ = ["_C", "distCUDA2"]
