"""pointnet2_ops' `ball_query` and `furthest_point_sample`, and the points of a set of depth maps.

Mirrors `from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample` (utils/ref_score_utils.py:1), a CUDA-only
extension the reference does not carry, and `get_points_from_depth` (utils/ref_score_utils.py:8-19).  The work runs in libmrgs.so
(csrc/mrgs_ballquery.hip: boxes of 64 consecutive points, boxes of 64 such boxes, one wavefront per 64 queries) on torch's current
stream, without a host read; the contracts are written out in include/mrgs.h.  The semantics restate pointnet2_ops' published kernels
and are pinned to their float32 brute force (tests/pool_statement.py): results are bit-equal to it.  Parity with the CUDA binary is
unpinned: nvcc contracts a*b+c, so a point at the rim of a ball may fall on the other side there, and its sampler's ties depend on its
block size (here: the lowest index).  The sampler keeps the published kernel's magnitude test: a point with x^2 + y^2 + z^2 <= 1e-3 is
never picked after index 0.  There is no CPU path and no torch fallback; results carry no graph.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._camconst import consts, focal

_p = _lib.ptr


def _cloud(t, what, fn):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {what} must be a tensor")
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{fn}: {what} must have dimensions (B, N, 3), got {tuple(t.shape)}")
    if t.dtype is not torch.float32:
        raise TypeError(f"{fn}: {what} must be float32 (the kernels read the buffer as float), got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{fn}: {what} must be a CUDA(HIP) tensor: the search runs in libmrgs.so, there is no CPU path")
    return t.detach().contiguous()


def _workspace(L, B, N, dev):
    return torch.empty(int(L.mrgs_ball_query_ws_bytes(B, N)), dtype=torch.uint8, device=dev)


def ball_query(radius, nsample, xyz, new_xyz):
    """xyz [B,N,3], new_xyz [B,M,3] float32 on the GPU -> int32 [B,M,nsample]: per query the first `nsample` indices k, in ascending
    order, with |new_xyz[j] - xyz[k]|^2 < radius^2 (fp32, strict), padded with the first of them; a row without one is zeros."""
    xyz, new_xyz = _cloud(xyz, "xyz", "ball_query"), _cloud(new_xyz, "new_xyz", "ball_query")
    if xyz.shape[0] != new_xyz.shape[0] or xyz.device != new_xyz.device:
        raise ValueError(f"ball_query: xyz {tuple(xyz.shape)} on {xyz.device} and new_xyz {tuple(new_xyz.shape)} on {new_xyz.device} "
                         "must share the batch size and the device")
    nsample = int(nsample)
    if nsample < 1:
        raise ValueError(f"ball_query: nsample must be at least 1, got {nsample}")
    L = _lib.lib()
    dev = xyz.device
    (B, N, _), M = xyz.shape, new_xyz.shape[1]
    idx = torch.empty((B, M, nsample), dtype=torch.int32, device=dev)
    if idx.numel() == 0:
        return idx
    ws = _workspace(L, B, N, dev)
    with _lib.guard(dev):
        _lib.check(L.mrgs_ball_query(float(radius), nsample, _p(xyz), _p(new_xyz), B, N, M, _p(idx), _p(ws), ws.numel(), _lib.stream_ptr(dev)))
    return idx


def furthest_point_sample(xyz, npoint, *, return_span=False):
    """xyz [B,N,3] float32 on the GPU -> int32 [B,npoint]: index 0, then repeatedly the point (of magnitude^2 > 1e-3) furthest from the
    picks so far, ties to the lowest index.  With return_span also float32 [B]: the distance between the first two picks (what
    ref_scores_max_pooling scales its radius by), computed on the device."""
    xyz = _cloud(xyz, "xyz", "furthest_point_sample")
    npoint = int(npoint)
    B, N, _ = xyz.shape
    if npoint < 0 or (npoint > 0 and B > 0 and N == 0):
        raise ValueError(f"furthest_point_sample: cannot pick {npoint} of {N} points")
    L = _lib.lib()
    dev = xyz.device
    idx = torch.empty((B, npoint), dtype=torch.int32, device=dev)
    span = torch.zeros(B, dtype=torch.float32, device=dev) if return_span else None
    if idx.numel():
        ws = _workspace(L, B, N, dev)
        with _lib.guard(dev):
            _lib.check(L.mrgs_furthest_point_sample(_p(xyz), B, N, npoint, _p(idx), _p(span), _p(ws), ws.numel(), _lib.stream_ptr(dev)))
    return (idx, span) if return_span else idx


def _view_table(cams, depths, H, W, dev):
    """The MrgsDepthView array of include/mrgs.h on the device, through pinned memory (torch's host allocator keeps the block until the
    asynchronous copy has run).  A camera pose held on the device costs one host read the first time."""
    table = (_lib.MrgsDepthView * len(cams))()
    for rec, cam, depth in zip(table, cams, depths):
        c = consts(cam, dev)
        if len(c.r_host) != 9 or len(c.t_host) != 3:
            raise ValueError("points_from_depth: a camera needs R [3,3] and T [3]")
        rec.depth = depth.data_ptr()
        rec.R[:], rec.T[:] = c.r_host, c.t_host
        rec.fx, rec.fy, rec.cx, rec.cy = focal(cam)
    host = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = np.frombuffer(table, dtype=np.uint8)
    return host.to(dev, non_blocking=True)


def image_size(cams):
    """(H, W) shared by all cameras of the list."""
    sizes = {(int(c.image_height), int(c.image_width)) for c in cams}
    if len(sizes) != 1:
        raise ValueError(f"the views must share one image size, got {sorted(sizes)}")
    return sizes.pop()


def check_maps(maps, what, H, W, n, fn):
    """`n` tensors of H*W elements each ([H*W], [H,W] or [1,H,W])."""
    if len(maps) != n:
        raise ValueError(f"{fn}: {len(maps)} {what} for {n} cameras")
    for i, m in enumerate(maps):
        if not torch.is_tensor(m):
            raise TypeError(f"{fn}: {what}[{i}] must be a tensor, got {type(m).__name__}")
        if m.numel() != H * W:
            raise ValueError(f"{fn}: {what}[{i}] has {m.numel()} elements, the cameras' images have {H} x {W}")
    return maps


def device_maps(maps, what, fn, dev=None):
    """Checked maps as float32 contiguous tensors of one device (`dev` when given)."""
    for i, m in enumerate(maps):
        if not m.is_cuda:
            raise RuntimeError(f"{fn}: {what}[{i}] must be a device tensor (libmrgs.so has no CPU path)")
        dev = dev or m.device
        if m.device != dev:
            raise ValueError(f"{fn}: {what}[{i}] is on {m.device}, other maps are on {dev}")
    return [_lib.f32c(m) for m in maps]


def points_from_depth(cams, depth_images):
    """float32 [len(cams) * H * W, 3]: point i*H*W + y*W + x is pixel (x, y) of view i lifted by its depth, the reference's
    get_points_from_depth (utils/ref_score_utils.py:8-19, scale = 1): ((x - Cx) / Fx z, (y - Cy) / Fy z, z), then (p - T) @ R^T.  One
    launch for all views."""
    cams = list(cams)
    if not cams:
        raise ValueError("points_from_depth: no cameras")
    H, W = image_size(cams)
    depths = device_maps(check_maps(list(depth_images), "depth_images", H, W, len(cams), "points_from_depth"), "depth_images", "points_from_depth")
    dev = depths[0].device
    with _lib.guard(dev):
        table = _view_table(cams, depths, H, W, dev)
        points = torch.empty((len(cams) * H * W, 3), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mrgs_depth_points(_p(table), len(cams), H, W, _p(points), _lib.stream_ptr(dev)))
    del depths
    return points
