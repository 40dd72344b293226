"""Statements of the dataset side of a view, independent of materialrefgs_amd: Pillow's 8-bit BICUBIC resize in numpy (integer arithmetic
after the coefficient tables, so equality with Pillow is exact), readCamerasFromTransforms' compositing as its literal float64 expression,
and the decode in torch CPU ops written as the reference writes them (utils/general_utils.py:21-27, utils/camera_utils.py:37,
train_refnerf.py:84-131, :193)."""
import math

import numpy as np
import torch

PRECISION_BITS = 22


def keys_cubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def coefficients(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BICUBIC over the whole axis: (ksize, bounds [out, 2], kk [out, ksize]) with
    scalar double arithmetic, one output and one tap at a time."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = [keys_cubic((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _pass(img, bounds, kk):
    """One pass along the LAST axis of an int array [..., in] -> uint8 [..., out]."""
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (x0, n) in enumerate(bounds):
        acc = (src[..., x0:x0 + n] * kk[xx, :n].astype(np.int64)).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                              # int32 accumulators suffice
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(img, out_h, out_w):
    """img uint8 [H,W] or [H,W,C] -> [out_h,out_w(,C)] as PIL.Image.resize((out_w, out_h)) (BICUBIC): horizontal pass, then vertical."""
    a = img if img.ndim == 3 else img[..., None]
    planes = np.ascontiguousarray(a.transpose(2, 0, 1))                 # [C,H,W]
    H, W = planes.shape[1:]
    if W != out_w:
        _, b, k = coefficients(W, out_w)
        planes = _pass(planes, b, k)
    if H != out_h:
        _, b, k = coefficients(H, out_h)
        planes = _pass(planes.transpose(0, 2, 1), b, k).transpose(0, 2, 1)
    out = np.ascontiguousarray(planes.transpose(1, 2, 0))
    return out if img.ndim == 3 else out[..., 0]


def composite_reference(rgba, white_background):
    """dataset_readers.py:276-282, literally; the signed bytes read back as the uint8 PIL takes them for."""
    bg = np.array([1, 1, 1]) if white_background else np.array([0, 0, 0])
    norm_data = rgba / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    with np.errstate(invalid="ignore"):
        return np.array(arr * 255.0, dtype=np.byte).view(np.uint8)


def all_pairs_rgba():
    """[256,256,4]: pixel (c, a) has colour c in all three channels and alpha a."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.ascontiguousarray(np.stack([c, c, c, a], axis=-1))


def decode_image(hwc_u8):
    """PILtoTorch after the resize: [C,H,W] float32."""
    t = torch.from_numpy(np.ascontiguousarray(hwc_u8)) / 255.0
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(dim=-1).permute(2, 0, 1)


def decode_grey(chw):
    return (0.299 * chw[0] + 0.587 * chw[1] + 0.114 * chw[2])[None]


def decode_normal(hwc_u8):
    normal = hwc_u8[..., :3].reshape(-1, 3)
    normal = (normal / 255.) * 2. - 1
    return torch.from_numpy(normal).float()


def decode_mask(hw_u8):
    mask = (hw_u8 > 128).astype(np.float32).reshape(-1, 1)
    return torch.from_numpy(mask).float()


def decode_score(hw_u8):
    return torch.from_numpy(hw_u8[..., None] > 128).bool().permute(2, 0, 1)
