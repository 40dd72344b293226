"""The Sobel smoothness terms behind the reference's names: `smooth_loss` (utils/loss_utils.py:124-125), which train_refreal.py:1261 adds
on `base_color_map * ref_score_image`, and `first_order_edge_aware_loss` (:121-122), which `calculate_loss` (:185-197) adds on `rend_normal`
and `surf_depth`.  The pixel work runs in libmrgs.so (csrc/mrgs_smooth.hip): two launches for the values of up to four maps over the same
image and one for all of their gradient maps, with no host read, instead of a pad, a reshape and a conv2d per operand, some ten
elementwise and reduction launches and the same again in backward with a transposed convolution.  There is no torch fallback in this
module: the maps must be fp32 device tensors (a CPU tensor, another dtype or a shape that does not match H x W raises);
`materialrefgs_amd.losses` keeps the torch statement of both names for every other input.

G is kornia's `spatial_gradient(mode="sobel", normalized=True)` as `losses.spatial_gradient` restates it: the 3 x 3 Sobel pair divided by 8,
replicate border.  d|G|/dG = sign(G) with sign(0) = 0, as `torch.abs` has it.  Every term is a 0-d device tensor.  Nothing is
differentiated with respect to the image or a mask.
"""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from .priors import _prior_image

_p = _lib.ptr
MAX_ITEMS = _lib.MRGS_SMOOTH_MAX_ITEMS


class SmoothItem(NamedTuple):
    """One map of `view_smooth_terms`: data [C,H,W] (or [H,W]) fp32 on the device; mask None or H*W elements, bool or uint8, on the host or
    the device (a zero entry sets the pixel to 0 before the stencil); edge_aware: damp by exp(-|G(img)|) (C = 1 or 3) or not (C = 1..4)."""
    data: torch.Tensor
    mask: Optional[torch.Tensor] = None
    edge_aware: bool = False


def _map_f32(t, what, channels):
    """A rendered map: a float32 tensor [C,H,W] with C in `channels` ([H,W] counts as C = 1); dtype and shape first, then `_on_device`,
    as priors._map_f32 orders them."""
    if not torch.is_tensor(t):
        raise TypeError(f"materialrefgs_amd.smoothness: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype is not torch.float32:
        raise TypeError(f"materialrefgs_amd.smoothness: {what} must be float32, got {t.dtype}")
    C = t.shape[0] if t.dim() == 3 else 1
    if t.dim() not in (2, 3) or C not in channels or 0 in t.shape:
        raise ValueError(f"materialrefgs_amd.smoothness: {what} must have shape [C,H,W] with C in {tuple(channels)}, got {tuple(t.shape)}")
    return t


def _on_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"materialrefgs_amd.smoothness: {what} must be a device tensor (libmrgs.so has no CPU path)")


class _SmoothTermsFn(torch.autograd.Function):
    """One term per item from one forward; one backward launch for every gradient map that has an upstream gradient."""

    @staticmethod
    def forward(ctx, img, H, W, spec, *datas):
        ctx.set_materialize_grads(False)       # unused terms arrive as None in backward, not as zero-filled tensors
        n = len(datas)
        datas = tuple(d.contiguous() for d in datas)
        dev = datas[0].device
        cfg = _lib.MrgsSmoothConfig(H, W, 0)
        items = (_lib.MrgsSmoothItem * n)(*(_lib.MrgsSmoothItem(_p(d), _p(m), None, C, int(edge)) for d, (m, C, edge) in zip(datas, spec)))
        lib = _lib.lib()
        with _lib.guard(dev):
            ws = torch.empty(lib.mrgs_smooth_ws_bytes(H, W), dtype=torch.uint8, device=dev)
            terms = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.check(lib.mrgs_smooth_terms_forward(ctypes.byref(cfg), _p(img), items, n, _p(ws), ws.numel(), _p(terms), _lib.stream_ptr(dev)))
        ctx.cfg, ctx.spec = cfg, spec
        ctx.save_for_backward(img, *datas)
        return terms.unbind(0)                 # each term its own 0-d tensor, a view made where nothing is recorded

    @staticmethod
    def backward(ctx, *g):
        img, *datas = ctx.saved_tensors
        n = len(datas)
        table = (ctypes.c_void_p * n)()
        items = (_lib.MrgsSmoothItem * n)()
        held, grads = [], [None] * n
        for i, (d, (m, C, edge), gi) in enumerate(zip(datas, ctx.spec, g)):
            items[i] = _lib.MrgsSmoothItem(_p(d), _p(m), None, C, int(edge))
            if gi is not None and ctx.needs_input_grad[4 + i]:
                gi = _lib.f32c(gi)
                held.append(gi)
                grads[i] = torch.empty_like(d)
                table[i] = gi.data_ptr()
                items[i].g_data = grads[i].data_ptr()
        if held:
            dev = datas[0].device
            with _lib.guard(dev):
                _lib.check(_lib.lib().mrgs_smooth_terms_backward(ctypes.byref(ctx.cfg), _p(img), items, n, table, _lib.stream_ptr(dev)))
        return (None, None, None, None) + tuple(grads)


def view_smooth_terms(img=None, items=()):
    """Up to four items over the same H x W in ONE forward (two launches) and ONE backward launch; the Sobel weights of `img` [3,H,W] are
    formed once and shared by every edge-aware item.  `items`: `SmoothItem`s or (data, mask, edge_aware) tuples.  Returns a tuple of 0-d
    device tensors, one per item."""
    items = [it if isinstance(it, SmoothItem) else SmoothItem(*it) for it in items]
    if not 1 <= len(items) <= MAX_ITEMS:
        raise ValueError(f"materialrefgs_amd.smoothness: 1..{MAX_ITEMS} items a call, got {len(items)}")
    for k, it in enumerate(items):
        _map_f32(it.data, f"items[{k}].data", (1, 3) if it.edge_aware else (1, 2, 3, 4))
    H, W = (int(s) for s in items[0].data.shape[-2:])
    any_edge = any(it.edge_aware for it in items)
    for k, it in enumerate(items):
        if tuple(it.data.shape[-2:]) != (H, W):
            raise ValueError(f"materialrefgs_amd.smoothness: items[{k}].data must have shape [C,{H},{W}] as items[0].data, got {tuple(it.data.shape)}")
    if any_edge:
        if img is None:
            raise ValueError("materialrefgs_amd.smoothness: an edge-aware item needs img")
        _map_f32(img, "img", (3,))
        if tuple(img.shape) != (3, H, W):
            raise ValueError(f"materialrefgs_amd.smoothness: img must have shape {(3, H, W)}, got {tuple(img.shape)}")
        if torch.is_grad_enabled() and img.requires_grad:
            # the backward forms no gradient for the image: refuse instead of returning a silent None where the reference's line
            # differentiates both arguments (the contract of losses.fused_loss for gt)
            raise ValueError("materialrefgs_amd.smoothness: `img` requires grad, but the smoothness terms differentiate only the maps; pass "
                             "img.detach() or evaluate under torch.no_grad()")
    for k, it in enumerate(items):
        _on_device(it.data, f"items[{k}].data")
    dev = items[0].data.device
    if any_edge:
        _on_device(img, "img")
        img = img.detach().contiguous()
    else:
        img = None
    spec = []
    for k, it in enumerate(items):
        mask = None if it.mask is None else _prior_image(it.mask, f"items[{k}].mask", H * W, dev, (torch.bool, torch.uint8))
        spec.append((mask, it.data.shape[0] if it.data.dim() == 3 else 1, bool(it.edge_aware)))
    return _SmoothTermsFn.apply(img, H, W, tuple(spec), *(it.data for it in items))


def smooth_loss(data, mask=None):
    """utils/loss_utils.py:124-125 on data [C,H,W], C <= 4: the mean over C H W of |G_x| + |G_y|.  `mask` (H*W elements, bool or uint8):
    the term of data * mask, the product never formed."""
    return view_smooth_terms(None, (SmoothItem(data, mask, False),))[0]


def first_order_edge_aware_loss(data, img):
    """utils/loss_utils.py:121-122 on data [3,H,W] or [1,H,W] and img [3,H,W]: |G(data)| damped by exp(-|G(img)|), summed over the two
    directions, mean over 3 H W."""
    return view_smooth_terms(img, (SmoothItem(data, None, True),))[0]


def albedo_smooth_loss(base_color_map, ref_score_image):
    """train_refreal.py:1261: smooth_loss(render_pkg["base_color_map"] * ref_score_image), with `ref_score_image` [1,H,W] bool or uint8 on
    the host (uploaded here, as the reference's `.cuda()` does per call) or on the device (priors.to_device moves a dictionary once)."""
    return view_smooth_terms(None, (SmoothItem(base_color_map, ref_score_image, False),))[0]
