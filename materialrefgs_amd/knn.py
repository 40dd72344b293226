"""Initial scales of a point cloud: the mean squared distance of every point to its three nearest other points.

Mirrors `from simple_knn._C import distCUDA2` (submodules/simple-knn/spatial.cu:14-26 over simple_knn.cu:147-221), which
GaussianModel.create_from_pcd turns into the initial scales: scales = log(sqrt(clamp_min(distCUDA2(points), 1e-7)))
(scene/gaussian_model.py:367, env_gaussian_model.py:147).  The search runs in libmrgs.so (csrc/mrgs_knn.hip: Morton order, boxes of
64 points, one wavefront per box) on torch's current stream, without a host read; the values are bit-equal to the float32 brute force
of the definition (tests/knn_statement.py).  There is no CPU path and no torch fallback.
"""
import torch

from . import _lib


def distCUDA2(points):
    """points [P,3] float32 on the GPU -> [P] float32: mean of the squared distances to the three nearest other points (fewer than three
    others: the missing ones count as FLT_MAX).  The result carries no graph, as the reference's."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("distCUDA2: points must be a tensor")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"distCUDA2: points must have dimensions (num_points, 3), got {tuple(points.shape)}")
    if points.dtype is not torch.float32:
        raise TypeError(f"distCUDA2: points must be float32 (the reference reads the buffer as float), got {points.dtype}")
    if not points.is_cuda:
        raise RuntimeError("distCUDA2: points must be a CUDA(HIP) tensor: the neighbour search runs in libmrgs.so, there is no CPU path")
    L = _lib.lib()
    dev = points.device
    pts = points.detach().contiguous()
    P = pts.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=dev)
    if P == 0:
        return out
    ws = torch.empty(int(L.mrgs_knn_ws_bytes(P)), dtype=torch.uint8, device=dev)
    with _lib.guard(dev):
        _lib.check(L.mrgs_knn_mean_dist2(_lib.ptr(pts), P, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return out


mean_dist2 = distCUDA2
