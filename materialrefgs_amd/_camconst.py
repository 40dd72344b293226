"""What the host path derives from a camera object or from its intrinsics K before a launch: stated once, cached once (camera.py
states the reference's camera math; nothing else in the package turns a camera into launch constants).

`consts(cam, device)` is the camera's entry, one per camera object and device, valid while every source the camera has -- R, T, HWK[2],
world_view_transform -- carries the stamp it was built from (`_cache.derived`): a pose refined in place or new intrinsics on the same
object rebuild it.  Its fields are built at the first request; a camera class without one of the sources misses only the fields that
need it.  `kinv` and `maps_frame` are keyed by what they are made of, not by the camera: the bytes of K (views share them) and, as ever,
the addresses of the two matrices (`MiniCam.to` wraps the same device matrices anew: that must not cost the host read of a rebuild).
"""
import math
from functools import cached_property

import numpy as np
import torch

from ._cache import Bounded, derived

_CAMERAS = Bounded(4096)         # (id(camera), device) -> Consts
_BY_SOURCE = Bounded(4096)       # bytes of K -> kinv; (addresses of the view and projection matrices, W, H) -> maps_frame


def focal(cam):
    """(Fx, Fy, Cx, Cy) of scene/cameras.py:65-68."""
    W, H = int(cam.image_width), int(cam.image_height)
    fx, fy = getattr(cam, "Fx", None), getattr(cam, "Fy", None)
    if fx is None:
        fx = _fov_focal(W, cam.FoVx)
    if fy is None:
        fy = _fov_focal(H, cam.FoVy)
    return float(fx), float(fy), float(getattr(cam, "Cx", 0.5 * W)), float(getattr(cam, "Cy", 0.5 * H))


def _fov_focal(W, FoVx):
    return W / (2.0 * math.tan(FoVx * 0.5))


def fov_focal(cam):
    """(fx, fy) from the field of view and the image size alone, whatever Fx / Fy the camera carries: the "pgsr" depth's focal."""
    return _fov_focal(int(cam.image_width), cam.FoVx), _fov_focal(int(cam.image_height), cam.FoVy)


def kinv(K):
    """The nine entries of K^-1 (float32) as a tuple; cached by the intrinsics' values (a numpy inverse per view otherwise)."""
    a = np.asarray(K, dtype=np.float32)
    t = _BY_SOURCE.get(key := a.tobytes())
    if t is None:
        t = _BY_SOURCE[key] = tuple(np.linalg.inv(a).astype(np.float32).reshape(-1).tolist())
    return t


def maps_frame(view):
    """(view rotation [9], ray matrix [9], ray origin [3]) of depths_to_points (utils/point_utils.py:9-24) as host floats.  Built once
    per camera on the host (float64) from the camera's matrices: the reference rebuilds them with ~10 small GPU kernels per view."""
    wvt, fpt = view.world_view_transform, view.full_proj_transform
    W, H = int(view.image_width), int(view.image_height)

    def build():
        wv = wvt.detach().cpu().double().numpy()
        fp = fpt.detach().cpu().double().numpy()
        c2w = np.linalg.inv(wv.T)
        ndc2pix = np.array([[W / 2, 0, 0, W / 2], [0, H / 2, 0, H / 2], [0, 0, 0, 1]], dtype=np.float64).T
        intrins = ((c2w.T @ fp) @ ndc2pix)[:3, :3].T
        M = c2w[:3, :3] @ np.linalg.inv(intrins)
        return wv[:3, :3].reshape(-1).tolist(), M.reshape(-1).tolist(), c2w[:3, 3].tolist()
    return derived(_BY_SOURCE, (wvt.data_ptr(), fpt.data_ptr(), W, H), (wvt, fpt), build)


def _host_f32(t):
    """A pose array or tensor as a flat float32 host tuple (a tensor held on the device is read once)."""
    return tuple(torch.as_tensor(t).detach().to("cpu", torch.float32).reshape(-1).tolist())


class Consts:
    """The fields of one camera's entry.  It holds the camera, so the `id` in its key stays the camera's own."""

    def __init__(self, cam, device):
        self.cam, self.device = cam, device

    Kinv = cached_property(lambda s: kinv(s.cam.HWK[2]))
    # Camera.R, Camera.T as float32 contiguous device tensors (uploaded once when the pose is numpy)
    R = cached_property(lambda s: torch.as_tensor(s.cam.R, dtype=torch.float32, device=s.device).contiguous())
    T = cached_property(lambda s: torch.as_tensor(s.cam.T, dtype=torch.float32, device=s.device).contiguous())
    r_host = cached_property(lambda s: _host_f32(s.cam.R))             # the same as nine and three host floats: the pose of MrgsDepthView
    t_host = cached_property(lambda s: _host_f32(s.cam.T))
    rt_host = cached_property(lambda s: tuple(s.r_host[3 * c + r] for r in range(3) for c in range(3)))   # R^T row-major: normal prior, contact sheet
    # world_view_transform (16), R (9), T (3) as 28 host floats: pose tensors held on the device cost one host read here, none afterwards
    record_host = cached_property(lambda s: _host_f32(s.cam.world_view_transform) + s.r_host + s.t_host)

    @cached_property
    def record(self):
        """The same 28 floats as one device float32 record: a device-side concat (host tensors are uploaded asynchronously, nothing is
        read back)."""
        parts = []
        for t in (self.cam.world_view_transform, self.cam.R, self.cam.T):
            t = torch.as_tensor(t)
            if t.device != self.device:
                t = t.to(self.device, non_blocking=True)
            parts.append(t.reshape(-1).to(torch.float32))
        return torch.cat(parts)


def consts(cam, device):
    """The entry of `cam` on `device` (module docstring)."""
    hwk = getattr(cam, "HWK", None)
    srcs = (getattr(cam, "R", None), getattr(cam, "T", None), getattr(cam, "world_view_transform", None), None if hwk is None else hwk[2])
    return derived(_CAMERAS, (id(cam), device), tuple(s for s in srcs if s is not None), lambda: Consts(cam, device))
