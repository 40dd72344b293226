"""`from simple_knn._C import distCUDA2` resolves to the MI355X implementation (materialrefgs_amd.knn -> libmrgs.so).

The reference imports it at the top of scene/gaussian_model.py:11 and scene/env_gaussian_model.py:20 and calls it in create_from_pcd
(:367, :147) for the initial scales; with this repository's root on the path instead of the CUDA extension
(submodules/simple-knn/spatial.cu, simple_knn.cu) those imports bind the HIP implementation unchanged.  See INTEGRATION.md.
"""
from materialrefgs_amd.knn import distCUDA2  # noqa: F401

__all__ = ["distCUDA2"]
