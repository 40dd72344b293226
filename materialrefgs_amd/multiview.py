"""Multi-view material consistency loss behind the reference's names: `calc_warp_loss` (train_refnerf.py:414-739, the same body in
train_glossy.py:442-772) and its train_refreal.py:405-729 variant (`calc_warp_loss_refreal`).  The pixel work runs in libmrgs.so
(csrc/mrgs_multiview.hip): the geometric check, the sample draw, the patch warps and the three material terms are one autograd node with
one forward and one backward call, and neither reads a device value on the host.  There is no torch fallback -- CPU tensors raise.

Differences a caller sees:
  * where no pixel passes the geometric check the reference returns None for every term; here the terms are 0 with zero gradient
    (deciding on the host would cost a synchronisation).  `original_weight` is the all-zero map in both.
  * the sample draw is the device sampler's (uniform, seeded from numpy's global generator), not np.random.choice's.
  * the edge mask (the reference's `dilated_edges_imgs`, cv2 Canny + dilation on the host) is computed on the device by
    materialrefgs_amd.edges, whose definition is this library's own; a caller's `edges_fn` still takes its place.
  * use_virtul_cam, ncc_scale != 1, wo_use_geo_occ_aware and (train_refreal.py) directional_rghmtl_warp_alignment = False raise
    NotImplementedError; all four are off by default.
  * the grey-image NCC (get_consistency_loss2) is a second autograd node, `_WarpNcc`, that follows the first on the same draw and
    differentiates rend_normal / rend_distance of the view.  train_refnerf.py / train_glossy.py compute the term and never return it, so
    calc_warp_loss leaves it out; calc_warp_loss_refreal returns it.  Where no sample is used the reference returns None, here the term is
    0 with zero gradient; visual_refweight is a device map (the reference builds it on the CPU).
"""
import ctypes
import random

import numpy as np
import torch

from . import _lib, edges
from ._camconst import consts, focal


_p = _lib.ptr


def basecolor_weight(iteration, schedule):
    """get_current_basecolor_warp_weight (train_refnerf.py:664-672: 0.1; train_refreal.py:669-677: 4 -> 1.5 over 12 000 .. 20 000)."""
    if schedule == "refreal":
        if iteration < 12000:
            return 4.0
        if iteration <= 20000:
            return 4.0 - (iteration - 12000) / (20000 - 12000) * (4.0 - 1.5)
        return 1.5
    return 0.1


def mtlrgh_weight(iteration, schedule):
    """get_current_mtlrgh_warp_weight (train_refnerf.py:673-681: 0.5; train_refreal.py:678-686: 1)."""
    return 1.0 if schedule == "refreal" else 0.5


def _c(t, dtype=torch.float32):
    t = t.detach()
    return t if (t.dtype == dtype and t.is_contiguous()) else t.to(dtype).contiguous()


class _WarpLoss(torch.autograd.Function):
    """terms[4] = (geo, base colour, metallic, roughness) of view v against neighbour n; weight map [H,W] and counts[4] (n_valid,
    samples, kept samples, 0) are not differentiable."""

    @staticmethod
    def forward(ctx, depth_v, depth_n, base_v, metal_v, rough_v, base_n, metal_n, rough_n, normal_v, dist_v, fg, keep, cam_v, cam_n,
                samples, out_samples, cfg):
        ctx.set_materialize_grads(False)
        H, W = cfg.H, cfg.W
        dev = depth_v.device
        flags = cfg.flags
        mat = bool(flags & _lib.MRGS_WARP_MATERIAL)
        use_m, use_r = bool(flags & _lib.MRGS_WARP_METALLIC), bool(flags & _lib.MRGS_WARP_ROUGHNESS)
        keepers = [_c(depth_v), _c(depth_n),
                   _c(base_v) if mat else None, _c(metal_v) if use_m else None, _c(rough_v) if use_r else None,
                   _c(base_n) if mat else None, _c(metal_n) if use_m else None, _c(rough_n) if use_r else None,
                   _c(normal_v) if mat else None, _c(dist_v) if mat else None, _c(fg) if mat else None,
                   _c(keep, torch.uint8) if (mat and keep is not None) else None, cam_v, cam_n]
        names = ("depth_v", "depth_n", "base_v", "metal_v", "rough_v", "base_n", "metal_n", "rough_n", "normal_v", "distance_v", "fg_v",
                 "keep_v", "cam_v", "cam_n")
        maps = _lib.MrgsWarpMaps(**{k: _p(t) for k, t in zip(names, keepers)})
        lib = _lib.lib()
        with _lib.guard(dev):
            ws = torch.empty(lib.mrgs_warp_loss_ws_bytes(H, W, cfg.sample_num, cfg.patch_half), dtype=torch.uint8, device=dev)
            weight = torch.empty((H, W), dtype=torch.float32, device=dev)
            terms = torch.empty(4, dtype=torch.float32, device=dev)
            counts = torch.empty(4, dtype=torch.int32, device=dev)
            smp = samples if samples is not None else out_samples
            _lib.check(lib.mrgs_warp_loss_forward(ctypes.byref(cfg), ctypes.byref(maps), _p(smp), _p(ws), ws.numel(), _p(weight), _p(terms),
                                                  _p(counts), _lib.stream_ptr(dev)))
        ctx.cfg, ctx.maps = cfg, maps
        ctx.shapes = [None if t is None else t.shape for t in (depth_v, depth_n, base_v, metal_v, rough_v, base_n, metal_n, rough_n)]
        ctx.save_for_backward(ws, weight, samples, *keepers)
        ctx.mark_non_differentiable(weight, counts, ws)
        return terms, weight, counts, ws              # ws: the draw and the homographies, for _WarpNcc

    @staticmethod
    def backward(ctx, g_terms, _gw, _gc, _gws):
        nil = (None,) * 17
        if g_terms is None:
            return nil
        ws, weight, _samples, *keepers = ctx.saved_tensors     # (the saved tensors keep every pointer of ctx.maps alive)
        cfg = ctx.cfg
        dev = weight.device
        gt = _c(g_terms)
        H, W = cfg.H, cfg.W
        flags = cfg.flags
        need = ctx.needs_input_grad
        geo = bool(flags & _lib.MRGS_WARP_GEO)
        mat = bool(flags & _lib.MRGS_WARP_MATERIAL)
        use_m, use_r = bool(flags & _lib.MRGS_WARP_METALLIC), bool(flags & _lib.MRGS_WARP_ROUGHNESS)
        # the view's material maps take no gradient: the reference samples them under torch.no_grad() (train_refnerf.py:510-559)
        want = [need[0] and geo, need[1] and geo, False, False, False, need[5] and mat, need[6] and use_m, need[7] and use_r]
        chans = (1, 1, 3, 1, 1, 3, 1, 1)
        outs = [torch.empty((c, H, W) if c > 1 else (H, W), dtype=torch.float32, device=dev) if w else None for w, c in zip(want, chans)]
        with _lib.guard(dev):
            _lib.check(_lib.lib().mrgs_warp_loss_backward(ctypes.byref(cfg), ctypes.byref(ctx.maps), _p(ws), _p(weight), _p(gt),
                                                          *[_p(o) for o in outs], _lib.stream_ptr(dev)))
        grads = [None if o is None else o.view(shp) for o, shp in zip(outs, ctx.shapes)]
        return tuple(grads) + (None,) * 9


class _WarpNcc(torch.autograd.Function):
    """The grey-image patch NCC of the view pair of a completed _WarpLoss (its weight map and workspace): term[1], the ref_weight map
    [H,W], counts[2] (samples, used samples), per-sample ncc [sample_num] and use flag [sample_num] (empty unless `detail`).  Differentiable in rend_normal and
    rend_distance of the view only."""

    @staticmethod
    def forward(ctx, normal_v, dist_v, grey_v, grey_n, metal_v, metal_n, weight, warp_ws, cam_v, cam_n, samples, out_samples, cfg, ncc_weight,
                detail):
        ctx.set_materialize_grads(False)
        H, W = cfg.H, cfg.W
        dev = weight.device
        keepers = [_c(normal_v), _c(dist_v), _c(grey_v), _c(grey_n), _c(metal_v), _c(metal_n)]
        maps = _lib.MrgsWarpMaps(normal_v=_p(keepers[0]), distance_v=_p(keepers[1]), metal_v=_p(keepers[4]), metal_n=_p(keepers[5]),
                                 cam_v=_p(cam_v), cam_n=_p(cam_n))
        lib = _lib.lib()
        with _lib.guard(dev):
            ws = torch.empty(lib.mrgs_warp_ncc_ws_bytes(H, W, cfg.sample_num, cfg.patch_half), dtype=torch.uint8, device=dev)
            term = torch.empty(1, dtype=torch.float32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)
            refw = torch.empty((H, W), dtype=torch.float32, device=dev)
            # per-sample outputs only where the caller asked for them (slots past the sample count stay 0)
            ncc_s = torch.zeros(cfg.sample_num if detail else 0, dtype=torch.float32, device=dev)
            use_s = torch.zeros(cfg.sample_num if detail else 0, dtype=torch.uint8, device=dev)
            smp = samples if samples is not None else out_samples
            _lib.check(lib.mrgs_warp_ncc_forward(ctypes.byref(cfg), ctypes.byref(maps), _p(keepers[2]), _p(keepers[3]), _p(weight), _p(warp_ws),
                                                 warp_ws.numel(), _p(smp), _p(ws), ws.numel(), ncc_weight, _p(term), _p(counts), _p(refw),
                                                 _p(ncc_s) if detail else None, _p(use_s) if detail else None, _lib.stream_ptr(dev)))
        ctx.cfg, ctx.ncc_weight = cfg, ncc_weight
        ctx.shapes = (normal_v.shape, dist_v.shape)
        ctx.save_for_backward(warp_ws, ws)
        ctx.mark_non_differentiable(refw, counts, ncc_s, use_s)
        return term, refw, counts, ncc_s, use_s

    @staticmethod
    def backward(ctx, g_term, *_):
        nil = (None,) * 15
        if g_term is None:
            return nil
        warp_ws, ws = ctx.saved_tensors
        cfg = ctx.cfg
        dev = ws.device
        H, W = cfg.H, cfg.W
        need = ctx.needs_input_grad
        gn = torch.empty((3, H, W), dtype=torch.float32, device=dev) if need[0] else None
        gd = torch.empty((H, W), dtype=torch.float32, device=dev) if need[1] else None
        gt = _c(g_term)
        with _lib.guard(dev):
            _lib.check(_lib.lib().mrgs_warp_ncc_backward(ctypes.byref(cfg), _p(warp_ws), _p(ws), ctx.ncc_weight, _p(gt), _p(gn), _p(gd),
                                                         _lib.stream_ptr(dev)))
        return (None if gn is None else gn.view(ctx.shapes[0]), None if gd is None else gd.view(ctx.shapes[1])) + (None,) * 13


def _grey_image(cam):
    """The camera's grey photograph as train_refreal.py reads it (get_image()[1], scene/cameras.py), or None if it carries none."""
    if hasattr(cam, "get_image"):
        return cam.get_image()[1]
    g = getattr(cam, "original_image_gray", None)
    if g is not None:
        return g
    img = getattr(cam, "original_image", None)
    if img is None:
        return None
    return (0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2])[None]          # scene/cameras.py:63


def warp_consistency_loss(view_cam, view_pkg, nearest_cam, nearest_pkg, fg_mask, keep_mask=None, *, iteration, seed, samples=None,
                          out_samples=None, patch_size=3, sample_num=102400, pixel_noise_th=1.0, geo_weight=0.03, ncc_weight=0.15,
                          metallic_weight=0.05, roughness_weight=0.05, use_metallic_warp=True, use_roughness_warp=True, use_geo=True,
                          schedule="refnerf", grey_v=None, grey_n=None, ncc_detail=None):
    """The multi-view consistency terms of view `view_cam` (render dictionary `view_pkg`, with "rend_distance") against
    `nearest_cam` / `nearest_pkg`.  Returns (geo, base_colour, metallic, roughness, weight_map, n_valid): 0-d device tensors for the
    terms (weights a(it) * multi_view_ncc_weight and b(it) * metallic / roughness weight applied; 0 where a term is switched off),
    the detached [H,W] weight map and n_valid as a 0-d int32 device tensor.  The material terms run when iteration > 10000.
    fg_mask: [H,W] foreground of the view; keep_mask: [H,W] bool (or 0 / 1 bytes, which are used as they are), False on an edge (None:
    keep all).  `samples`: int32 pixel indices
    (y * W + x) to use instead of the device draw (tests replay a recorded draw); `out_samples`: int32 [sample_num] device tensor that
    receives the draw.  No host read.
    grey_v / grey_n ([H,W] or [1,H,W] device tensors, both or neither): the grey photographs of the two cameras.  With them the call
    returns two more values, (..., ncc, ref_weight_map): train_refreal.py's grey-image NCC term (get_consistency_loss2; weight
    ncc_weight, no schedule, live at every iteration and differentiable in view_pkg["rend_normal"] / ["rend_distance"]) on the draw of
    the material terms, and the detached [H,W] device map of visual_refweight.  `ncc_detail`: a dict that receives "ncc_s", "use_s"
    (per sample, [sample_num]) and "counts" (samples, used samples) as device tensors."""
    depth_v, depth_n = view_pkg["surf_depth"], nearest_pkg["surf_depth"]
    if not depth_v.is_cuda:
        raise RuntimeError("materialrefgs_amd.multiview needs device tensors (libmrgs.so has no CPU path)")
    if "rend_distance" not in view_pkg:
        raise ValueError("warp_consistency_loss: view_pkg has no 'rend_distance' (render with the \"pgsr\" flavour; train_refnerf.py:568)")
    if (grey_v is None) != (grey_n is None):
        raise ValueError("warp_consistency_loss: pass both grey_v and grey_n, or neither")
    if patch_size not in (1, 2, 3):
        raise ValueError(f"warp_consistency_loss: patch_size {patch_size} is not 1, 2 or 3 (one 64-lane wave covers a patch)")
    if schedule not in ("refnerf", "refreal"):
        raise ValueError(f"warp_consistency_loss: schedule {schedule!r} is not 'refnerf' or 'refreal'")
    H, W = depth_v.shape[-2:]
    if tuple(depth_n.shape[-2:]) != (H, W) or (int(view_cam.image_height), int(view_cam.image_width)) != (H, W) or \
            (int(nearest_cam.image_height), int(nearest_cam.image_width)) != (H, W):
        raise ValueError("warp_consistency_loss: both views must have the same image size")
    dev = depth_v.device
    material = iteration > 10000
    flags = (_lib.MRGS_WARP_GEO if use_geo else 0)
    if material:
        flags |= _lib.MRGS_WARP_MATERIAL | (_lib.MRGS_WARP_METALLIC if use_metallic_warp else 0) | \
            (_lib.MRGS_WARP_ROUGHNESS if use_roughness_warp else 0)
    seed = int(seed) & ((1 << 64) - 1)
    n_given = -1
    if samples is not None:
        samples = samples.to(dev, torch.int32).contiguous()
        if samples.dim() != 1 or samples.numel() > sample_num:
            raise ValueError(f"warp_consistency_loss: samples must be a 1-d list of at most sample_num = {sample_num} pixel indices")
        n_given = samples.numel()
    if out_samples is not None and (out_samples.dtype != torch.int32 or out_samples.numel() < sample_num or not out_samples.is_cuda
                                    or not out_samples.is_contiguous()):
        raise ValueError("warp_consistency_loss: out_samples must be a contiguous int32 device tensor of sample_num elements")
    a = basecolor_weight(iteration, schedule)
    b = mtlrgh_weight(iteration, schedule)
    cfg = _lib.MrgsWarpConfig(int(H), int(W), int(sample_num), int(patch_size), n_given, flags, seed & 0xFFFFFFFF, seed >> 32,
                              *focal(view_cam), *focal(nearest_cam), float(pixel_noise_th), float(geo_weight), float(a * ncc_weight),
                              float(b * metallic_weight), float(b * roughness_weight))
    fg = fg_mask.reshape(H, W) if fg_mask is not None else None
    if material and fg is None:
        raise ValueError("warp_consistency_loss: fg_mask is required for the material terms")
    keep = keep_mask.reshape(H, W) if keep_mask is not None else None
    if keep is not None and keep.device != dev:
        keep = keep.to(dev, non_blocking=True)
    if fg is not None and fg.device != dev:
        fg = fg.to(dev, non_blocking=True)
    vp, npk = view_pkg, nearest_pkg
    cam_v, cam_n = consts(view_cam, dev).record, consts(nearest_cam, dev).record
    terms, weight, counts, ws = _WarpLoss.apply(
        depth_v.reshape(H, W), depth_n.reshape(H, W), vp["diffuse_map"], vp["refl_strength_map"], vp["roughness_map"], npk["diffuse_map"],
        npk["refl_strength_map"], npk["roughness_map"], vp["rend_normal"], vp["rend_distance"], fg, keep,
        cam_v, cam_n, samples, out_samples, cfg)
    if grey_v is None:
        return terms[0], terms[1], terms[2], terms[3], weight, counts[0]
    greys = []
    for g in (grey_v, grey_n):
        if not g.is_cuda or g.numel() != H * W:
            raise ValueError("warp_consistency_loss: grey_v / grey_n must be [H,W] or [1,H,W] device tensors")
        greys.append(g.reshape(H, W))
    ncc, refw, ncc_counts, ncc_s, use_s = _WarpNcc.apply(vp["rend_normal"], vp["rend_distance"], greys[0], greys[1], vp["refl_strength_map"],
                                                         npk["refl_strength_map"], weight, ws, cam_v, cam_n, samples, out_samples, cfg,
                                                         float(ncc_weight), ncc_detail is not None)
    if ncc_detail is not None:
        ncc_detail.update(ncc_s=ncc_s, use_s=use_s, counts=ncc_counts)
    return terms[0], terms[1], terms[2], terms[3], weight, counts[0], ncc[0], refw


def _check_opt(viewpoint_cam, opt, refreal):
    if getattr(opt, "use_virtul_cam", False):
        raise NotImplementedError("calc_warp_loss: opt.use_virtul_cam (virtual neighbour cameras) is not built")
    if float(getattr(viewpoint_cam, "ncc_scale", 1.0)) != 1.0:
        raise NotImplementedError("calc_warp_loss: ncc_scale != 1 is not built")
    if getattr(opt, "wo_use_geo_occ_aware", False):
        raise NotImplementedError("calc_warp_loss: opt.wo_use_geo_occ_aware is not built")
    if refreal and not getattr(opt, "directional_rghmtl_warp_alignment", True):
        raise NotImplementedError("calc_warp_loss: opt.directional_rghmtl_warp_alignment = False is not built")


def _drop_in(viewpoint_cam, scene, opt, gaussians, pipe, render, render_pkg, mask_images, iteration, bg, use_metallic_warp,
             use_roughness_warp, edges_fn, refreal, samples, grey_v=None):
    _check_opt(viewpoint_cam, opt, refreal)
    if not render_pkg["surf_depth"].is_cuda:
        raise RuntimeError("materialrefgs_amd.multiview needs device tensors (libmrgs.so has no CPU path)")
    keep = None
    if getattr(opt, "edge_aware_in_warp", False):
        with torch.no_grad():
            if edges_fn is None:
                # the kernel's bytes as they are: _WarpLoss takes a uint8 map without a conversion launch
                keep = edges.edge_mask(render_pkg["rend_normal"], dilate_size=7, invert=True).view(torch.uint8)
            else:
                H, W = render_pkg["surf_depth"].shape[-2:]
                keep = ~torch.as_tensor(edges_fn(render_pkg["rend_normal"], dilate_size=7)).reshape(H, W).bool()
    if len(viewpoint_cam.nearest_id) == 0:
        return None
    nearest_cam = scene.getTrainCameras()[random.sample(viewpoint_cam.nearest_id, 1)[0]]
    nearest_pkg = render(nearest_cam, gaussians, pipe, bg, srgb=opt.srgb, opt=opt, wo_render_img=False)
    grey = {}
    if grey_v is not None:
        grey_n = _grey_image(nearest_cam)
        if grey_n is None:
            raise NotImplementedError("calc_warp_loss_refreal: the neighbour camera carries no image for the grey-image NCC term; pass "
                                      "without_ncc=True to train without it (INTEGRATION.md section 4h)")
        dev = render_pkg["surf_depth"].device
        grey = dict(grey_v=torch.as_tensor(grey_v).to(dev, non_blocking=True), grey_n=torch.as_tensor(grey_n).to(dev, non_blocking=True))
    seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    if iteration > 10000:
        opt.directional_rghmtl_warp_alignment = True      # train_refnerf.py:648 (the assignment sits in the material branch)
    fg = torch.as_tensor(mask_images[viewpoint_cam.image_name]) if iteration > 10000 else None
    geo, base, metal, rough, weight, _n, *ncc = warp_consistency_loss(
        viewpoint_cam, render_pkg, nearest_cam, nearest_pkg, fg, keep, iteration=iteration, seed=seed,
        patch_size=opt.multi_view_patch_size, sample_num=opt.multi_view_sample_num, pixel_noise_th=opt.multi_view_pixel_noise_th,
        samples=samples, geo_weight=opt.multi_view_geo_weight, ncc_weight=opt.multi_view_ncc_weight, metallic_weight=opt.metallic_warp_weight,
        roughness_weight=opt.roughness_warp_weight, use_metallic_warp=use_metallic_warp, use_roughness_warp=use_roughness_warp,
        use_geo=refreal, schedule="refreal" if refreal else "refnerf", **grey)
    material = iteration > 10000
    return (geo if refreal else None, base if material else None, metal if (material and use_metallic_warp) else None,
            rough if (material and use_roughness_warp) else None, weight, *ncc)


def calc_warp_loss(viewpoint_cam, scene, opt, gaussians, dataset, pipe, render, render_pkg, albeldo_images, mtl_images, rgh_images, mask_images,
                   iteration, debug_path, bg, use_metallic_warp=False, use_roughness_warp=False, *, edges_fn=None, samples=None):
    """train_refnerf.py:414-739 / train_glossy.py:442-772: (None, None, base_color_loss, metallic_warp_loss, roughness_warp_loss,
    original_weight, None, None).  `edges_fn`: a replacement for the device edge mask of opt.edge_aware_in_warp, called as the reference's
    dilated_edges_imgs is (rend_normal, dilate_size=7).
    `samples`: int32 pixel indices replacing the device draw (replays a recorded np.random.choice draw; tests)."""
    r = _drop_in(viewpoint_cam, scene, opt, gaussians, pipe, render, render_pkg, mask_images, iteration, bg, use_metallic_warp,
                 use_roughness_warp, edges_fn, False, samples)
    if r is None:
        return None, None, None, None, None, None, None, None
    _geo, base, metal, rough, weight = r
    return None, None, base, metal, rough, weight, None, None


def calc_warp_loss_refreal(viewpoint_cam, scene, opt, gaussians, dataset, pipe, render, render_pkg, albeldo_images, mtl_images, rgh_images,
                           mask_images, iteration, debug_path, bg, use_metallic_warp=False, use_roughness_warp=False, *, edges_fn=None,
                           without_ncc=False, samples=None):
    """train_refreal.py:405-729: (geo_loss, ncc_loss, base_color_loss, metallic_warp_loss, roughness_warp_loss, original_weight,
    visual_refweight, None).  ncc_loss is the grey-image NCC term (get_consistency_loss2, :707) that the training loop adds to its loss
    (:1227-1228) and whose homography trains rend_normal and rend_distance; the grey images are the cameras' own (get_image()[1], else
    original_image_gray, else the luminance of original_image).  Differences: where no sample is used ncc_loss is 0 with zero gradient
    (None in the reference), and visual_refweight is a DEVICE H x W tensor (the reference builds it on the CPU, which costs a
    synchronisation).  A camera without an image raises NotImplementedError;
    without_ncc=True leaves the term out: ncc_loss is then None and visual_refweight a CPU H x W map of zeros."""
    grey_v = None
    if not without_ncc:
        grey_v = _grey_image(viewpoint_cam)
        if grey_v is None:
            raise NotImplementedError("calc_warp_loss_refreal: the camera carries no image for the grey-image NCC term "
                                      "(get_consistency_loss2); pass without_ncc=True to train without it (INTEGRATION.md section 4h)")
    r = _drop_in(viewpoint_cam, scene, opt, gaussians, pipe, render, render_pkg, mask_images, iteration, bg, use_metallic_warp,
                 use_roughness_warp, edges_fn, True, samples, grey_v)
    H, W = render_pkg["surf_depth"].shape[-2:]
    zeros = torch.zeros(H, W) if without_ncc else torch.zeros(H, W, device=render_pkg["surf_depth"].device)
    if r is None:
        return None, None, None, None, None, None, zeros, None
    if without_ncc:
        geo, base, metal, rough, weight = r
        return geo, None, base, metal, rough, weight, zeros, None
    geo, base, metal, rough, weight, ncc, refw = r
    return geo, ncc, base, metal, rough, weight, refw, None
