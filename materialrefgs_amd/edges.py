"""The edge mask of the multi-view loss behind the reference's name: `dilated_edges_imgs` (utils/image_utils.py:109-116), which every
`calc_warp_loss` starts with when `opt.edge_aware_in_warp` is set (train_refnerf.py:447).  The reference copies the rendered normal map
to the host, runs cv2.cvtColor, cv2.Canny(0, 80) and cv2.dilate there and uploads a float64 image; here the same kind of mask comes from
four launches of libmrgs.so (csrc/mrgs_edges.hip) on torch's current stream, with no host read.  There is no torch or cv2 fallback.

The definition is this library's own (include/mrgs.h states it in integers; INTEGRATION.md section 4h lists what differs from cv2): the
8-bit quantisation wraps as numpy's `astype(np.uint8)` does on x86, the grey conversion uses OpenCV 4's coefficients, and byte parity
with a particular OpenCV build is not claimed.
"""
import torch

from . import _lib

_p = _lib.ptr


def _image(img):
    if not torch.is_tensor(img):
        raise TypeError(f"materialrefgs_amd.edges: img must be a tensor, got {type(img).__name__}")
    if img.dtype is not torch.float32:
        raise TypeError(f"materialrefgs_amd.edges: img must be float32, got {img.dtype}")
    if img.dim() != 3 or img.shape[0] != 3 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError(f"materialrefgs_amd.edges: img must have shape [3,H,W], got {tuple(img.shape)}")
    if not img.is_cuda:
        raise RuntimeError("materialrefgs_amd.edges: img must be a device tensor (libmrgs.so has no CPU path)")
    return _lib.f32c(img)


def edge_mask(img, dilate_size=4, thres1=0., thres2=80., invert=False, classes=False):
    """[H,W] torch.bool device tensor: True on the dilated Canny edges of `img` ([3,H,W] fp32 device tensor, in practice rend_normal), or
    with `invert` True everywhere else (the loss's keep mask).  The tensor is the kernel's byte buffer viewed as bool.  With `classes`
    returns (mask, classes): the [H,W] uint8 map of the non-maximum suppression, 0 none, 1 candidate, 2 strong."""
    img = _image(img)
    dev = img.device
    H, W = int(img.shape[1]), int(img.shape[2])
    lib = _lib.lib()
    with _lib.guard(dev):
        ws = torch.empty(lib.mrgs_edges_ws_bytes(H, W), dtype=torch.uint8, device=dev)
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        cls = torch.empty((H, W), dtype=torch.uint8, device=dev) if classes else None
        _lib.check(lib.mrgs_edge_mask(_p(img), H, W, int(dilate_size), float(thres1), float(thres2), int(bool(invert)), _p(out), _p(cls), _p(ws),
                                      ws.numel(), _lib.stream_ptr(dev)))
    mask = out.view(torch.bool)
    return (mask, cls) if classes else mask


def dilated_edges_imgs(img_in, dilate_size=4, thres1=0., thres2=80.):
    """utils/image_utils.py:109-116 with its return convention: the [H,W] mask as 0 / 1 in float64, on img_in's device."""
    return edge_mask(img_in, dilate_size, thres1, thres2).to(torch.float64)
