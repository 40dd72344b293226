"""The per-pixel prior terms the training scripts add to `total_loss` outside `calculate_loss`, behind the reference's names:
`mono_normal_loss` (train_refnerf.py:202-251, same body in train_glossy.py:212 and train_refreal.py:190), the mask-entropy term on
`rend_alpha` (train_refnerf.py:1210-1217, train_glossy.py:1274-1276) and the four ref-score material terms (train_refreal.py:1238-1258).
The pixel work runs in libmrgs.so (csrc/mrgs_prior.hip): two launches for the values of all three groups and one for all gradient
maps, with no host read, instead of two matmuls, four normalize calls, two boolean-index gathers (a host wait each) and some sixty
elementwise and reduction launches per iteration, and the same again in backward.  There is no torch fallback: the rendered maps must be
fp32 device tensors (a CPU tensor, another dtype or a shape that does not match H x W raises).

Differences a caller sees: every term is a 0-d device tensor (`loss_mask_entropy` may go into `tb_dict` as it is; the reference calls
`.item()`, a host wait per iteration; `float(x)` still works), the `iteration % 3000` debug PNG dump of `mono_normal_loss` is not
reproduced, and a term is NaN exactly where the reference's is (an all-zero mask, an empty ref-score set or its empty complement).

The prior images (`normal_images[name]` [H*W,3], `mask_images[name]` [H*W,1], `ref_score_images[name]` [1,H,W] bool) may be CPU tensors,
uploaded per call as the reference does (`.cuda()`), or device tensors, used as they are: `to_device(mapping, device)` moves a
dictionary once after loading.
"""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._camconst import consts

_p = _lib.ptr
_SLOTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12)       # the entries of out_terms[16] (include/mrgs.h) that are terms; the rest are denominators


class PriorTerms(NamedTuple):
    """What `view_prior_terms` returns: 0-d device tensors, None for the terms of a group that was not asked for."""
    l1_surf: Optional[torch.Tensor]            # mono_normal_loss's l1_normal, cos_normal (surf_normal) ...
    cos_surf: Optional[torch.Tensor]
    l1_rend: Optional[torch.Tensor]            # ... and l1_normal2, cos_normal2 (rend_normal)
    cos_rend: Optional[torch.Tensor]
    mask_entropy: Optional[torch.Tensor]       # loss_mask_entropy (the caller multiplies by 0.01)
    ref_metallic: Optional[torch.Tensor]       # mean over S of |refl - 0.9|
    ref_roughness: Optional[torch.Tensor]      # mean over S of |rough - 0.05|
    ref_metallic_bg: Optional[torch.Tensor]    # mean over not S of |refl - 0.05|
    ref_roughness_bg: Optional[torch.Tensor]   # mean over not S of |0.9 - rough|
    ref_sum: Optional[torch.Tensor]            # the four as the scripts add them: a1 + a2 + b1 + b2 / 2 (unweighted)


def _map_f32(t, what, shapes):
    """A rendered map: a float32 tensor of one of `shapes` (checked in the style of densify.device_f32; dtype and shape of every map
    first, then `_on_device`, so that the message names the first thing a caller has to change)."""
    if not torch.is_tensor(t):
        raise TypeError(f"materialrefgs_amd.priors: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype is not torch.float32:
        raise TypeError(f"materialrefgs_amd.priors: {what} must be float32, got {t.dtype}")
    if tuple(t.shape) not in shapes:
        raise ValueError(f"materialrefgs_amd.priors: {what} must have shape {' or '.join(str(s) for s in shapes)}, got {tuple(t.shape)}")
    return t


def _on_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"materialrefgs_amd.priors: {what} must be a device tensor (libmrgs.so has no CPU path)")


def _prior_image(t, what, numel, dev, dtypes=(torch.float32,)):
    """An entry of the prior dictionaries: `numel` elements of one of `dtypes`, on the host (uploaded here, as the reference's `.cuda()`
    does per call) or on the device."""
    if not torch.is_tensor(t):
        raise TypeError(f"materialrefgs_amd.priors: {what} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"materialrefgs_amd.priors: {what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.numel() != numel:
        raise ValueError(f"materialrefgs_amd.priors: {what} must have {numel} elements for this image size, got shape {tuple(t.shape)}")
    if t.device != dev:
        t = t.to(dev)
    t = t.detach().contiguous()
    return t.view(torch.uint8) if t.dtype is torch.bool else t


class _PriorTermsFn(torch.autograd.Function):
    """The ten terms of `_SLOTS` from one forward; one backward launch for every gradient map.  A group is off when its maps are None."""

    @staticmethod
    def forward(ctx, surf, rend, alpha, refl, rough, H, W, rt, prior, mask, amask, score):
        ctx.set_materialize_grads(False)       # unused terms arrive as None in backward, not as zero-filled tensors
        surf, rend, alpha, refl, rough = (None if t is None else t.contiguous() for t in (surf, rend, alpha, refl, rough))
        dev = next(t for t in (surf, alpha, refl) if t is not None).device
        cfg = _lib.MrgsPriorConfig(H, W, 0)
        rt_c = (ctypes.c_float * 9)(*rt) if rt is not None else None
        lib = _lib.lib()
        with _lib.guard(dev):
            ws = torch.empty(lib.mrgs_prior_ws_bytes(H, W), dtype=torch.uint8, device=dev)
            terms = torch.empty(16, dtype=torch.float32, device=dev)
            _lib.check(lib.mrgs_prior_terms_forward(ctypes.byref(cfg), rt_c, _p(surf), _p(rend), _p(prior), _p(mask), _p(alpha), _p(amask),
                                                    _p(refl), _p(rough), _p(score), _p(ws), ws.numel(), _p(terms), _lib.stream_ptr(dev)))
        ctx.cfg, ctx.rt_c = cfg, rt_c
        ctx.save_for_backward(surf, rend, alpha, refl, rough, prior, mask, amask, score, terms)
        # each term is its own 0-d tensor (a view made here, where nothing is recorded): taking one apart adds no launch in backward
        parts = terms.unbind(0)
        return tuple(parts[k] for k in _SLOTS)

    @staticmethod
    def backward(ctx, *g):
        surf, rend, alpha, refl, rough, prior, mask, amask, score, terms = ctx.saved_tensors
        table = (ctypes.c_void_p * 16)()
        held = []
        for k, gk in zip(_SLOTS, g):
            if gk is not None:
                gk = _lib.f32c(gk)
                held.append(gk)
                table[k] = gk.data_ptr()
        need = ctx.needs_input_grad
        n_up, e_up, r_up = (any(x is not None for x in g[a:b]) for a, b in ((0, 4), (4, 5), (5, 10)))
        g_surf = torch.empty_like(surf) if (surf is not None and need[0] and (g[0] is not None or g[1] is not None)) else None
        g_rend = torch.empty_like(rend) if (rend is not None and need[1] and (g[2] is not None or g[3] is not None)) else None
        g_alpha = torch.empty_like(alpha) if (alpha is not None and need[2] and e_up) else None
        some = lambda *ks: any(g[k] is not None for k in ks)          # a1 / b1 reach refl, a2 / b2 rough, the sum both
        g_refl = torch.empty_like(refl) if (refl is not None and need[3] and some(5, 7, 9)) else None
        g_rough = torch.empty_like(rough) if (rough is not None and need[4] and some(6, 8, 9)) else None
        if n_up or e_up or r_up:
            dev = terms.device
            with _lib.guard(dev):
                _lib.check(_lib.lib().mrgs_prior_terms_backward(ctypes.byref(ctx.cfg), ctx.rt_c, _p(surf), _p(rend), _p(prior), _p(mask), _p(alpha),
                                                                _p(amask), _p(refl), _p(rough), _p(score), _p(terms), table, _p(g_surf), _p(g_rend),
                                                                _p(g_alpha), _p(g_refl), _p(g_rough), _lib.stream_ptr(dev)))
        return (g_surf, g_rend, g_alpha, g_refl, g_rough) + (None,) * 7


def view_prior_terms(viewpoint_cam=None, *, surf_normal=None, rend_normal=None, normal_prior=None, normal_mask=None, rend_alpha=None,
                     alpha_mask=None, refl_strength_map=None, roughness_map=None, ref_score_image=None):
    """Any subset of the three groups in ONE forward (two launches) and ONE backward launch; what a script that uses more than one group
    should call.  Returns a `PriorTerms`.
      normal prior: viewpoint_cam (its R), surf_normal and rend_normal [3,H,W], normal_prior [H*W,3], normal_mask [H*W,1] or None;
      mask entropy: rend_alpha [1,H,W], alpha_mask (H*W elements; the same tensor as normal_mask is read once for both);
      ref score:    refl_strength_map and roughness_map [1,H,W], ref_score_image [1,H,W] bool or uint8."""
    use_n = surf_normal is not None or rend_normal is not None or normal_prior is not None
    use_e = rend_alpha is not None or alpha_mask is not None
    use_r = refl_strength_map is not None or roughness_map is not None or ref_score_image is not None
    if not (use_n or use_e or use_r):
        raise ValueError("materialrefgs_amd.priors: no group given (normal prior, mask entropy or ref score)")
    if use_n and (surf_normal is None or rend_normal is None or normal_prior is None or viewpoint_cam is None):
        raise ValueError("materialrefgs_amd.priors: the normal prior needs viewpoint_cam, surf_normal, rend_normal and normal_prior")
    if not use_n and normal_mask is not None:
        raise ValueError("materialrefgs_amd.priors: normal_mask without the normal prior's maps")
    if use_e and (rend_alpha is None or alpha_mask is None):
        raise ValueError("materialrefgs_amd.priors: the mask entropy needs rend_alpha and alpha_mask")
    if use_r and (refl_strength_map is None or roughness_map is None or ref_score_image is None):
        raise ValueError("materialrefgs_amd.priors: the ref score needs refl_strength_map, roughness_map and ref_score_image")
    first = surf_normal if use_n else (rend_alpha if use_e else refl_strength_map)
    if not torch.is_tensor(first) or first.dim() < 2:
        raise TypeError("materialrefgs_amd.priors: the rendered maps must be tensors [C,H,W]")
    H, W = (int(s) for s in first.shape[-2:])
    N = H * W
    one = ((1, H, W), (H, W))
    surf = rend = prior = mask = alpha = amask = refl = rough = score = rt = None
    if use_n:
        surf, rend = _map_f32(surf_normal, "surf_normal", ((3, H, W),)), _map_f32(rend_normal, "rend_normal", ((3, H, W),))
    if use_e:
        alpha = _map_f32(rend_alpha, "rend_alpha", one)
    if use_r:
        refl, rough = _map_f32(refl_strength_map, "refl_strength_map", one), _map_f32(roughness_map, "roughness_map", one)
    for t, what in ((surf, "surf_normal"), (rend, "rend_normal"), (alpha, "rend_alpha"), (refl, "refl_strength_map"), (rough, "roughness_map")):
        if t is not None:
            _on_device(t, what)
    dev = (surf if use_n else (alpha if use_e else refl)).device
    if use_n:
        prior = _prior_image(normal_prior, "normal_prior", 3 * N, dev)
        if normal_mask is not None:
            mask = _prior_image(normal_mask, "normal_mask", N, dev)
        rt = consts(viewpoint_cam, dev).rt_host
    if use_e:
        amask = mask if alpha_mask is normal_mask else _prior_image(alpha_mask, "alpha_mask", N, dev)
    if use_r:
        score = _prior_image(ref_score_image, "ref_score_image", N, dev, (torch.bool, torch.uint8))
    t = _PriorTermsFn.apply(surf, rend, alpha, refl, rough, H, W, rt, prior, mask, amask, score)
    none4, none5 = (None,) * 4, (None,) * 5
    return PriorTerms(*((t[0:4] if use_n else none4) + ((t[4],) if use_e else (None,)) + (t[5:10] if use_r else none5)))


def mono_normal_loss(viewpoint_cam, surf_normal, rend_normal, mask_images, normal_images, gamma, iteration, ref_mask=None, HSV_mask=None):
    """train_refnerf.py:202-251: same arguments, same 4-tuple (l1 and cos of surf_normal, then of rend_normal).  `gamma`, `ref_mask` and
    `HSV_mask` are ignored, as the reference ignores them; `iteration` only drives the reference's debug dump, which is not reproduced."""
    name = viewpoint_cam.image_name
    mask = mask_images[name] if mask_images is not None else None
    t = view_prior_terms(viewpoint_cam, surf_normal=surf_normal, rend_normal=rend_normal, normal_prior=normal_images[name], normal_mask=mask)
    return t.l1_surf, t.cos_surf, t.l1_rend, t.cos_rend


def mask_entropy_loss(rend_alpha, image_mask):
    """train_refnerf.py:1213-1215: -(m log o + (1 - m) log(1 - o)).mean() with o = rend_alpha.clamp(1e-6, 1 - 1e-6), a 0-d device tensor
    (the caller multiplies by 0.01)."""
    return view_prior_terms(rend_alpha=rend_alpha, alpha_mask=image_mask).mask_entropy


def ref_score_loss(refl_strength_map, roughness_map, ref_score_image, weight, return_terms=False):
    """train_refreal.py:1238-1258: weight * (mean_S |refl - 0.9| + mean_S |rough - 0.05| + mean_notS |refl - 0.05| + 0.5 mean_notS
    |0.9 - rough|); with return_terms also the four means, in that order."""
    t = view_prior_terms(refl_strength_map=refl_strength_map, roughness_map=roughness_map, ref_score_image=ref_score_image)
    total = weight * t.ref_sum
    return (total, t.ref_metallic, t.ref_roughness, t.ref_metallic_bg, t.ref_roughness_bg) if return_terms else total


def to_device(mapping, device):
    """A prior dictionary (image name -> tensor, None entries kept) with every tensor on `device`: call once after loading instead of
    paying an upload per iteration."""
    if mapping is None:
        return None
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in mapping.items()}
