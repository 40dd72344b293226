"""The photographs of a dataset as 8-bit planes on the device (csrc/mrgs_image.hip).

The reference keeps every view's fp32 ground truth, mask prior and normal prior in pageable host memory (scene/cameras.py:49) and uploads
them every iteration (train_refnerf.py:1176, :1212, :222-223).  A `ViewStore` uploads each file's bytes once: `add` composites (Blender
scenes) and resizes (Pillow's 8-bit BICUBIC, bit for bit) on the device and keeps byte planes, a quarter of the fp32 bytes; `fetch` turns
a view's planes into the fp32 tensors the losses read, in one launch.  Host uint8 arrays are the interface of `add`; there is no host
storage mode and no torch fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._cache import Bounded

PRECISION_BITS = 22            # Pillow's 8-bit coefficient precision: 32 - 8 - 2
OUTPUTS = ("gt", "alpha", "grey", "normal", "mask", "score")


# ---- host tables ------------------------------------------------------------------------------------------------------------------------
def _keys_cubic(t, a=-0.5):
    t = np.abs(t)
    return np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0, np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * a, 0.0))


def resize_table(in_size, out_size):
    """The coefficient table Pillow computes for BICUBIC from `in_size` to `out_size` samples, all in double: (ksize, bounds int32
    [out, 2] = (first source index, tap count), kk int32 [out, ksize] = normalised weights times 2^22, rounded half away from zero).
    The sum of the weights is taken in index order, as Pillow's loop takes it."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"materialrefgs_amd.viewstore: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    xmax = np.minimum(in_size, np.trunc(center + support + 0.5).astype(np.int64)) - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    live = taps < xmax[:, None]
    w = np.where(live, _keys_cubic(((taps + xmin[:, None]) - center[:, None] + 0.5) / fs), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        ww = ww + w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    kk = np.trunc(w * float(1 << PRECISION_BITS) + np.where(w < 0.0, -0.5, 0.5)).astype(np.int32)
    kk[~live] = 0
    return ksize, np.stack([xmin, xmax], axis=1).astype(np.int32), kk


def composite_table(white_background):
    """[256, 256] bytes indexed [colour, alpha]: readCamerasFromTransforms' float64 expression and its cast to a byte
    (scene/dataset_readers.py:278-282), evaluated once for every pair."""
    bg = np.array([1, 1, 1]) if white_background else np.array([0, 0, 0])
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    im_data = np.stack([c, c, c, a], axis=-1)
    norm_data = im_data / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    return np.ascontiguousarray(np.array(arr * 255.0, dtype=np.byte).view(np.uint8)[:, :, 0])


def normal_table():
    """float32((n / 255.) * 2. - 1) for every byte n, from numpy's float64 expression (train_refnerf.py:88, :93)."""
    n = np.arange(256, dtype=np.uint8)
    return ((n / 255.) * 2. - 1).astype(np.float32)


_TABLES = Bounded(64)          # (kind, ..., device) -> device arrays


def _device_table(key, build, dev):
    t = _TABLES.get(key + (dev,))
    if t is None:
        t = _TABLES[key + (dev,)] = build()
    return t


def _resize_tables(in_size, out_size, dev):
    def build():
        ksize, bounds, kk = resize_table(in_size, out_size)
        return ksize, torch.from_numpy(bounds).to(dev), torch.from_numpy(kk).to(dev)
    return _device_table(("resize", int(in_size), int(out_size)), build, dev)


# ---- device primitives --------------------------------------------------------------------------------------------------------------------
def _host_u8(a, what):
    a = a.numpy() if torch.is_tensor(a) and not a.is_cuda else a
    if torch.is_tensor(a):
        raise TypeError(f"materialrefgs_amd.viewstore: {what} must be a host uint8 array (the store uploads it), got a device tensor")
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0 or (a.ndim == 3 and a.shape[2] not in (1, 2, 3, 4)):
        raise ValueError(f"materialrefgs_amd.viewstore: {what} must be uint8 [H,W] or [H,W,1..4], got {a.dtype} {a.shape}")
    return a if a.ndim == 3 else a[:, :, None]


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("materialrefgs_amd.viewstore: the store lives on a GPU (libmrgs.so has no CPU path)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _check_u8(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype is torch.uint8 and t.is_contiguous()):
        raise RuntimeError(f"materialrefgs_amd.viewstore: {what} must be a contiguous uint8 device tensor")


def resize_u8(src, out_h, out_w, planar=False):
    """Device uint8 [H,W,C] (or planes [C,H,W] with planar=True), C <= 4 -> planes [C,out_h,out_w]: PIL's `resize((out_w, out_h))` on
    every channel (include/mrgs.h: mrgs_image_resize_u8)."""
    _check_u8(src, "src")
    if src.dim() != 3:
        raise ValueError(f"materialrefgs_amd.viewstore: src must have three dimensions, got {tuple(src.shape)}")
    (C, H, W) = src.shape if planar else (src.shape[2], src.shape[0], src.shape[1])
    out_h, out_w = int(out_h), int(out_w)
    dev, lib = src.device, _lib.lib()
    strides = (H * W, W, 1) if planar else (1, W * C, C)
    kx, bx, kkx = _resize_tables(W, out_w, dev) if W != out_w else (0, None, None)
    ky, by, kky = _resize_tables(H, out_h, dev) if H != out_h else (0, None, None)
    with _lib.guard(dev):
        dst = torch.empty((C, out_h, out_w), dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.mrgs_image_resize_ws_bytes(C, H, W, out_h, out_w), dtype=torch.uint8, device=dev)
        cfg = _lib.MrgsResizeConfig(C, H, W, out_h, out_w, kx, ky, 0, *strides)
        _lib.check(lib.mrgs_image_resize_u8(ctypes.byref(cfg), src.data_ptr(), _lib.ptr(bx), _lib.ptr(kkx), _lib.ptr(by), _lib.ptr(kky),
                                            _lib.ptr(ws), ws.numel(), dst.data_ptr(), _lib.stream_ptr(dev)))
    return dst


def composite_u8(rgba, white_background):
    """Device uint8 [H,W,4] -> planes [3,H,W]: the RGB image readCamerasFromTransforms builds (include/mrgs.h: mrgs_image_composite_u8)."""
    _check_u8(rgba, "rgba")
    if rgba.dim() != 3 or rgba.shape[2] != 4:
        raise ValueError(f"materialrefgs_amd.viewstore: rgba must be [H,W,4], got {tuple(rgba.shape)}")
    dev = rgba.device
    table = _device_table(("composite", bool(white_background)), lambda: torch.from_numpy(composite_table(white_background)).to(dev), dev)
    with _lib.guard(dev):
        dst = torch.empty((3,) + tuple(rgba.shape[:2]), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().mrgs_image_composite_u8(rgba.shape[0] * rgba.shape[1], rgba.data_ptr(), table.data_ptr(), dst.data_ptr(),
                                                      _lib.stream_ptr(dev)))
    return dst


def decode(*, rgb=None, alpha=None, grey_rgb=None, normal=None, mask=None, score=None, want=OUTPUTS):
    """The fp32 tensors of one view from its byte planes, in one launch (include/mrgs.h: mrgs_view_decode).  rgb [3,H,W], alpha / mask /
    score [H,W], grey_rgb [3,Hg,Wg] (rgb when None), normal [H,W,3].  Returns a dict with those of `want` whose planes were given:
    gt [3,H,W], alpha [1,H,W], grey [1,Hg,Wg], normal [H W,3], mask [H W,1] float32 and score [1,H,W] bool."""
    unknown = set(want) - set(OUTPUTS)
    if unknown:
        raise ValueError(f"materialrefgs_amd.viewstore: unknown outputs {sorted(unknown)}")
    if grey_rgb is None:
        grey_rgb = rgb
    planes = dict(gt=rgb, alpha=alpha, grey=grey_rgb, normal=normal, mask=mask, score=score)
    live = [k for k in OUTPUTS if k in want and planes[k] is not None]
    if not live:
        raise ValueError("materialrefgs_amd.viewstore: nothing to decode (no plane given for any wanted output)")
    for k in live:
        _check_u8(planes[k], k)
    first = planes[next((k for k in live if k != "grey"), "grey")]
    H, W = (first.shape[0], first.shape[1]) if first.dim() == 3 and first is normal else first.shape[-2:]
    Hg, Wg = grey_rgb.shape[-2:] if "grey" in live else (H, W)
    shapes = dict(gt=(3, H, W), alpha=(H, W), grey=(3, Hg, Wg), normal=(H, W, 3), mask=(H, W), score=(H, W))
    for k in live:
        if tuple(planes[k].shape) != shapes[k]:
            raise ValueError(f"materialrefgs_amd.viewstore: the {k} plane must be {shapes[k]}, got {tuple(planes[k].shape)}")
    dev = first.device
    out_shape = dict(gt=(3, H, W), alpha=(1, H, W), grey=(1, Hg, Wg), normal=(H * W, 3), mask=(H * W, 1), score=(1, H, W))
    with _lib.guard(dev):
        out = {k: torch.empty(out_shape[k], dtype=torch.bool if k == "score" else torch.float32, device=dev) for k in live}
        table = _device_table(("normal",), lambda: torch.from_numpy(normal_table()).to(dev), dev) if "normal" in live else None
        src = {k: _lib.ptr(planes[k]) if k in live else None for k in OUTPUTS}
        v = _lib.MrgsViewDecode(H, W, Hg, Wg, src["gt"], src["alpha"], src["grey"], src["normal"], src["mask"], src["score"], _lib.ptr(table),
                                *[_lib.ptr(out.get(k)) for k in OUTPUTS], 0)
        _lib.check(_lib.lib().mrgs_view_decode(ctypes.byref(v), _lib.stream_ptr(dev)))
    return out


# ---- the store ----------------------------------------------------------------------------------------------------------------------------
class ViewStore:
    """Byte planes of all views of a dataset on one device, keyed by a name (Scene uses (resolution_scale, uid) for photographs and the
    file stem for the prior maps)."""

    def __init__(self, device="cuda"):
        self.device = _cuda_device(device)
        self._views = {}

    def __len__(self):
        return len(self._views)

    def __contains__(self, name):
        return name in self._views

    def names(self):
        return list(self._views)

    @property
    def nbytes(self):
        seen = {}
        for v in self._views.values():
            for t in v.values():
                seen[t.data_ptr()] = t.numel()
        return sum(seen.values())

    def _upload(self, a):
        return torch.from_numpy(a).to(self.device)

    def add(self, name, image, size=None, grey_size=None, white_background=None):
        """One photograph: host uint8 [H,W,3] or [H,W,4].  `white_background` True / False composites an RGBA image onto that
        background first (Blender scenes: the result is RGB, without an alpha plane); None keeps a fourth channel as the view's alpha
        mask.  `size` (H, W): the resolution loadCam asks for, reached by Pillow's resize; `grey_size`: the resolution of the grey
        image's planes when process_image resizes a second time (ncc_scale != 1), from the same source."""
        a = _host_u8(image, "image")
        if a.shape[2] not in (3, 4):                               # process_image reads three channels: an L photograph raises there too
            raise ValueError(f"materialrefgs_amd.viewstore: a photograph is [H,W,3] or [H,W,4], got {a.shape}")
        H, W = a.shape[:2]
        src, planar = self._upload(a), False
        if white_background is not None:
            if a.shape[2] != 4:
                raise ValueError("materialrefgs_amd.viewstore: compositing needs an RGBA image")
            src, planar = composite_u8(src, white_background), True
        size = (H, W) if size is None else (int(size[0]), int(size[1]))
        planes = resize_u8(src, size[0], size[1], planar=planar)
        view = {"rgb": planes[:3]}
        if planes.shape[0] == 4:
            view["alpha"] = planes[3]
        if grey_size is not None and (int(grey_size[0]), int(grey_size[1])) != size:
            g = resize_u8(src, int(grey_size[0]), int(grey_size[1]), planar=planar)
            view["grey_rgb"] = g[:3]
        self._views.setdefault(name, {}).update(view)

    def add_prior(self, name, normal=None, mask=None, score=None):
        """Prior maps of a view at their file resolution (r = 1): normal uint8 [H,W,3], mask and score uint8 [H,W] (the channel the
        reference thresholds at 128)."""
        view = {}
        for key, a, chans in (("normal", normal, 3), ("mask", mask, 1), ("score", score, 1)):
            if a is None:
                continue
            a = _host_u8(a, key)
            if a.shape[2] != chans:
                raise ValueError(f"materialrefgs_amd.viewstore: the {key} prior must have {chans} channel(s), got {a.shape}")
            view[key] = self._upload(a if chans == 3 else a[:, :, 0])
        self._views.setdefault(name, {}).update(view)

    def has(self, name, what):
        key = {"gt": "rgb", "grey": "rgb"}.get(what, what)
        return name in self._views and key in self._views[name]

    def shape(self, name, what="rgb"):
        return tuple(self._views[name][what].shape)

    def fetch(self, name, want=OUTPUTS):
        """The fp32 tensors of view `name` that it has planes for, restricted to `want`: see `decode`.  Fresh tensors every time."""
        v = self._views[name]
        return decode(rgb=v.get("rgb"), alpha=v.get("alpha"), grey_rgb=v.get("grey_rgb"), normal=v.get("normal"), mask=v.get("mask"),
                      score=v.get("score"), want=want)
