"""The multi-view reflection score behind the reference's names: `calc_ref_score` (train_refreal.py:782-1001, the same body in
train_refnerf.py:791-1010 and train_glossy.py) and `get_multi_view_neighbor` (train_refreal.py:738-778).  For every pixel of a view: how
much the photographs of its neighbouring views disagree with the view's own over a plane-warped 9 x 9 patch.  It is the producer of the
`ref_score_images` that `priors.ref_score_loss` consumes.

The pixel work is one call of libmrgs.so per view (csrc/mrgs_multiview.hip, ref_score_fwd; the contract is written out at
mrgs_ref_score in include/mrgs.h): all neighbours in one gather pass with an [H,W] result, no [3,H,W,81] tensor per neighbour, no
host round trip of the maps and no gradient.  There is no torch fallback -- CPU tensors raise.

Differences a caller sees: the rendered maps stay on the device between the render pass and the score pass (the reference parks them
on the host), nothing is written to disk (the reference dumps debug PNGs), and the function's std / coefficient-of-variation / edge
experiments, none of which reaches its return value, are not built.

`ref_scores_max_pooling` and `ref_scores_max_pooling_wiht_mask` (utils/ref_score_utils.py:21-121) are the reference's step between that
score and the masks: every pixel of every view is lifted to 3D by its depth, and its score becomes the maximum over the first
n_samples = 49 points of the whole cloud, in cloud order, inside a ball around it -- pointnet2_ops' ball_query over the cloud against
itself, then a gather and a max.  Here it is two calls of libmrgs.so (csrc/mrgs_ballquery.hip; contracts at mrgs_depth_points and
mrgs_ball_max_pool in include/mrgs.h): one launch lifts all views, one fused walk keeps a running maximum per pixel, and the
[points, 49] index tensor (12.5 GB at 100 views of 800 x 800) never exists.  The values are bit-equal to the float32 brute force of
that definition on the same points (tests/pool_statement.py); parity with pointnet2_ops' CUDA binary is unpinned.
The reference's text cannot run as written, which is why `depth_images` is a required keyword here:
  * it calls the three-argument get_points_from_depth(self, fov_camera, depth) with two arguments (:41, :91);
  * it passes the score image where the depth belongs (same lines), so no depth source is named at all;
  * it indexes the (1, N) tensors total_points and ref_score with flat indices (:51, :59, :102, :110);
  * the masked variant calls `.resshape(-1)` (:90) and indexes `mask_images[mask]` with the mask itself (:92).
What is built is what those lines evidently mean: depth from the caller, points and scores as flat [N] rows.

`ref_score_mask` -- score > threshold -- is this project's own definition of the boolean map the loss takes: the reference contains no
code that thresholds the (pooled) score into the PNG masks its training script loads.  Parity unpinned.
"""
import ctypes
from collections.abc import Mapping

import numpy as np
import torch

from . import _lib, ballquery
from ._camconst import consts, focal

_p = _lib.ptr


def _cam_record(cam, device, field):
    """`record_host` (28 host floats) or `record` (device float32 [28]) of the camera's constants: world_view_transform, R, T."""
    rec = getattr(consts(cam, device), field)
    if len(rec) != 28:
        raise ValueError("reflection_score: a camera needs world_view_transform [4,4], R [3,3] and T [3]")
    return rec


def _photograph(cam):
    """The camera's colour photograph as the reference reads it (get_image()[0], scene/cameras.py:88), else original_image."""
    if hasattr(cam, "get_image"):
        return cam.get_image()[0]
    img = getattr(cam, "original_image", None)
    if img is None:
        raise ValueError("reflection_score: the camera carries no photograph (get_image() or original_image)")
    return img


def _shape(t, what, chans, H, W):
    if not torch.is_tensor(t):
        raise TypeError(f"reflection_score: {what} must be a tensor, got {type(t).__name__}")
    if t.numel() != chans * H * W or tuple(t.shape[-2:]) != (H, W):
        raise ValueError(f"reflection_score: {what} must be [{chans},{H},{W}] (all views have one image size), got {tuple(t.shape)}")


def _on_device(t, what, dev):
    if not t.is_cuda:
        raise RuntimeError(f"materialrefgs_amd.refscore: {what} must be a device tensor (libmrgs.so has no CPU path)")
    if t.device != dev:
        raise ValueError(f"reflection_score: {what} is on {t.device}, the view's surf_depth is on {dev}")
    return _lib.f32c(t)


def reflection_score(view_cam, view_pkg, neighbours, *, pixel_noise_th, patch_size=4, return_count=False):
    """score [H,W] of view `view_cam` (render dictionary `view_pkg` with "surf_depth", "rend_normal" and "rend_distance"; photograph from
    the camera) against `neighbours`, a list of (cam, surf_depth, image) visited in order.  With return_count also the int32 [H,W]
    number of neighbours that pass the reprojection check at each pixel.  Device tensors only; no host read once the cameras' records
    are cached; no gradient."""
    return _score(view_cam, view_pkg, neighbours, _photograph(view_cam), pixel_noise_th, patch_size, return_count)


def _score(view_cam, view_pkg, neighbours, image_v, pixel_noise_th, patch_size, return_count):
    for k in ("surf_depth", "rend_normal", "rend_distance"):
        if k not in view_pkg:
            raise ValueError(f"reflection_score: view_pkg has no {k!r} (render with the \"pgsr\" flavour)")
    if patch_size not in (1, 2, 3, 4):
        raise ValueError(f"reflection_score: patch_size {patch_size} is not 1, 2, 3 or 4")
    if not torch.is_tensor(view_pkg["surf_depth"]) or view_pkg["surf_depth"].dim() < 2:
        raise TypeError("reflection_score: surf_depth must be a tensor [1,H,W] or [H,W]")
    H, W = (int(s) for s in view_pkg["surf_depth"].shape[-2:])
    for c in [view_cam] + [n[0] for n in neighbours]:
        if (int(c.image_height), int(c.image_width)) != (H, W):
            raise ValueError("reflection_score: all views must have the same image size (the reference normalises a neighbour's sampling "
                             "grid with the view's H and W)")
    named = [(view_pkg["surf_depth"], "surf_depth", 1), (view_pkg["rend_normal"], "rend_normal", 3),
             (view_pkg["rend_distance"], "rend_distance", 1), (image_v, "the view's photograph", 3)]
    for i, (_cam, depth, image) in enumerate(neighbours):
        named += [(depth, f"surf_depth of neighbour {i}", 1), (image, f"photograph of neighbour {i}", 3)]
    for t, what, chans in named:
        _shape(t, what, chans, H, W)
    if not view_pkg["surf_depth"].is_cuda:
        raise RuntimeError("materialrefgs_amd.refscore needs device tensors (libmrgs.so has no CPU path)")
    dev = view_pkg["surf_depth"].device
    keep = [_on_device(t, what, dev) for t, what, _c in named]         # float32, contiguous; alive until the launch is queued
    depth_v, normal_v, dist_v, image_v = keep[:4]
    K = len(neighbours)
    table = (_lib.MrgsRefScoreNeighbour * max(K, 1))()
    for i, (cam, _d, _i) in enumerate(neighbours):
        rec = table[i]
        rec.depth, rec.image = keep[4 + 2 * i].data_ptr(), keep[5 + 2 * i].data_ptr()
        rec.cam[:] = _cam_record(cam, dev, "record_host")
        rec.fx, rec.fy, rec.cx, rec.cy = focal(cam)
    cam_v = _cam_record(view_cam, dev, "record")
    cfg = _lib.MrgsRefScoreConfig(H, W, int(patch_size), K, *focal(view_cam), float(pixel_noise_th))
    with _lib.guard(dev):
        table_dev = None
        if K:
            # through pinned memory: torch's host allocator keeps the block until the asynchronous copy has run
            host = torch.empty(ctypes.sizeof(table), dtype=torch.uint8, pin_memory=True)
            host.numpy()[:] = np.frombuffer(table, dtype=np.uint8)
            table_dev = host.to(dev, non_blocking=True)
        score = torch.empty((H, W), dtype=torch.float32, device=dev)
        count = torch.empty((H, W), dtype=torch.int32, device=dev) if return_count else None
        _lib.check(_lib.lib().mrgs_ref_score(ctypes.byref(cfg), _p(depth_v), _p(normal_v), _p(dist_v), _p(image_v), _p(cam_v), _p(table_dev),
                                            _p(score), _p(count), _lib.stream_ptr(dev)))
    del keep
    return (score, count) if return_count else score


def get_multi_view_neighbor(scene):
    """train_refreal.py:738-778: {image_name: [(index, image_name), ...]} over scene.getTrainCameras().  Host code with the reference's
    constants (at most 20 neighbours, 5-90 degrees between the optical axes with 180 / 3.14159, 0.1-1.5 between the centres) and its
    order, np.lexsort((angles, diss)): nearest centre first.  As in the reference, the cap is a minimum CARRIED from camera to camera
    (`multi_view_num = min(multi_view_num, len(...))`): a camera with few admissible neighbours shortens the list of every camera after
    it, and one with none empties them."""
    multi_view_num, max_angle, min_angle, min_dis, max_dis = 20, 90, 5, 0.1, 1.5
    cams = list(scene.getTrainCameras())
    host = lambda t: torch.as_tensor(t).detach().to("cpu")
    centers = torch.stack([host(c.camera_center).reshape(3) for c in cams], dim=0)
    rays = []
    for c in cams:
        R = host(c.R).float()
        rays.append(torch.tensor([0.0, 0.0, 1.0]).float() @ R.transpose(-1, -2))
    rays = torch.nn.functional.normalize(torch.stack(rays, dim=0), dim=-1)
    diss = torch.norm(centers[:, None] - centers[None], dim=-1).numpy()
    angles = (torch.arccos(torch.sum(rays[:, None] * rays[None], dim=-1)) * 180 / 3.14159).numpy()
    out = {}
    for i, cam in enumerate(cams):
        order = np.lexsort((angles[i], diss[i]))
        mask = (angles[i][order] < max_angle) & (diss[i][order] > min_dis) & (diss[i][order] < max_dis) & (angles[i][order] > min_angle)
        order = order[mask]
        multi_view_num = min(multi_view_num, len(order))
        out[cam.image_name] = [(int(j), cams[int(j)].image_name) for j in order[:multi_view_num]]
    return out


def _render_pgsr(cam, gaussians, pipe, bg, **kw):
    from .renderer import render_surfel
    return render_surfel(cam, gaussians, pipe, bg, flag="pgsr", **kw)


@torch.no_grad()
def calc_ref_score(scene, opt, gaussians, dataset, pipe, albeldo_images, mtl_images, rgh_images, mask_images, iteration, bg, *, render=None,
                   neighbours=None):
    """train_refreal.py:782-1001: {image_name: score [H*W]} for every training camera, the reference's signature and return value
    (patch_size 4; the unused arguments are the reference's).  Renders every camera once with `render` (default: render_surfel with the
    "pgsr" flavour, called as the reference calls it) and keeps surf_depth, rend_normal and rend_distance on the device, then one
    `reflection_score` per view against the lists of `get_multi_view_neighbor(scene)`, or against the caller's `neighbours` (the same
    mapping).  Writes no files."""
    render = render or _render_pgsr
    cams = list(scene.getTrainCameras())
    maps, images = {}, {}
    for cam in cams:
        pkg = render(cam, gaussians, pipe, bg, srgb=opt.srgb, opt=opt)
        if "rend_distance" not in pkg:
            raise ValueError("calc_ref_score: the render has no 'rend_distance' (the reference's render_surfel is the \"pgsr\" flavour)")
        maps[cam.image_name] = {k: pkg[k].detach() for k in ("surf_depth", "rend_normal", "rend_distance")}
        dev = maps[cam.image_name]["surf_depth"].device
        images[cam.image_name] = torch.as_tensor(_photograph(cam)).to(dev, non_blocking=True)
    if neighbours is None:
        neighbours = get_multi_view_neighbor(scene)
    out = {}
    for cam in cams:
        nbrs = [(cams[idx], maps[cams[idx].image_name]["surf_depth"], images[cams[idx].image_name]) for idx, _name in neighbours[cam.image_name]]
        out[cam.image_name] = _score(cam, maps[cam.image_name], nbrs, images[cam.image_name], opt.multi_view_pixel_noise_th, 4,
                                     False).reshape(-1)
    return out


def _per_view(maps, cams, what, fn):
    """The maps in camera order: by position, as the reference indexes them, or by image_name when a mapping is given."""
    if isinstance(maps, Mapping):
        missing = [c.image_name for c in cams if c.image_name not in maps]
        if missing:
            raise ValueError(f"{fn}: {what} has no entry for {missing[:3]}")
        return [maps[c.image_name] for c in cams]
    maps = list(maps)
    if len(maps) != len(cams):
        raise ValueError(f"{fn}: {len(maps)} {what} for {len(cams)} cameras")
    return maps


def _max_pool(fn, ref_score_images, mask_images, viewpoint_cam_lst, scene_extend, radius_ratio, n_samples, backend, calc_depth_points_radius,
              depth_images):
    if backend != 'ball query':
        raise NotImplementedError("Only ball query is supported")
    if depth_images is None:
        raise TypeError(f"{fn}() needs the keyword depth_images (one depth map per camera, e.g. the render's surf_depth): the reference "
                        "lifts the SCORE image where the depth belongs and calls its three-argument get_points_from_depth with two, so "
                        "it never ran and names no depth source")
    cams = list(viewpoint_cam_lst)
    if not cams:
        return {}
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"{fn}: n_samples must be at least 1, got {n_samples}")
    H, W = ballquery.image_size(cams)
    # sizes first, devices second: a wrong shape is reported as such wherever the tensors live
    named = [(what, ballquery.check_maps(_per_view(maps, cams, what, fn), what, H, W, len(cams), fn))
             for what, maps in (("ref_score_images", ref_score_images), ("depth_images", depth_images), ("mask_images", mask_images))
             if maps is not None]
    scores = ballquery.device_maps(named[0][1], named[0][0], fn)
    dev = scores[0].device
    depths = ballquery.device_maps(named[1][1], named[1][0], fn, dev)
    valid = None
    if mask_images is not None:
        for i, m in enumerate(named[2][1]):
            if not m.is_cuda or m.device != dev:
                raise RuntimeError(f"{fn}: mask_images[{i}] must be a device tensor on {dev} (libmrgs.so has no CPU path)")
        valid = torch.cat([(m.reshape(-1) != 0) for m in named[2][1]]).to(torch.uint8)
    points = ballquery.points_from_depth(cams, depths)
    score = torch.cat([s.reshape(-1) for s in scores])
    N = score.numel()
    radius_dev = None
    if calc_depth_points_radius:
        # |p[f0] - p[f1]| stays on the device; the kernel multiplies it by the ratio
        _idx, radius_dev = ballquery.furthest_point_sample(points.unsqueeze(0), 2, return_span=True)
        radius = float(radius_ratio)
    elif torch.is_tensor(scene_extend) and scene_extend.is_cuda:
        radius_dev, radius = _lib.f32c(scene_extend).reshape(-1)[:1].to(dev), float(radius_ratio)
    else:
        radius = float(scene_extend) * float(radius_ratio)
    L = _lib.lib()
    pooled = torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(int(L.mrgs_ball_query_ws_bytes(1, N)), dtype=torch.uint8, device=dev)
    with _lib.guard(dev):
        _lib.check(L.mrgs_ball_max_pool(radius, _p(radius_dev), n_samples, _p(points), _p(score), _p(valid), 1, N, _p(pooled), _p(ws), ws.numel(),
                                        _lib.stream_ptr(dev)))
    pooled = pooled.reshape(len(cams), H, W)
    return {cam.image_name: pooled[i] for i, cam in enumerate(cams)}


@torch.no_grad()
def ref_scores_max_pooling(ref_score_images, viewpoint_cam_lst, scene_extend, radius_ratio=0.1, n_samples=7 * 7, backend='ball query',
                           calc_depth_points_radius=False, *, depth_images=None):
    """utils/ref_score_utils.py:21-67: {image_name: [H,W] float32 on the device}, every pixel's score replaced by the maximum over the
    first `n_samples` points (in cloud order: view by view, row by row) of all views' depth points within the radius of its own.
    ref_score_images and depth_images: one map per camera ([H*W], [H,W] or [1,H,W]), by position in viewpoint_cam_lst or as a mapping
    by image_name (what calc_ref_score returns).  The radius is scene_extend * radius_ratio, or with calc_depth_points_radius the
    distance between the two points furthest_point_sample(points, 2) picks times radius_ratio, which never leaves the device.  A pixel
    whose ball is empty (radius 0, a non-finite depth) takes the score of point 0, as ball_query's zero row makes the reference do.
    One fused call: no [points, n_samples] index tensor exists.  No host read when the cameras' R and T are host tensors."""
    return _max_pool("ref_scores_max_pooling", ref_score_images, None, viewpoint_cam_lst, scene_extend, radius_ratio, n_samples, backend,
                     calc_depth_points_radius, depth_images)


@torch.no_grad()
def ref_scores_max_pooling_wiht_mask(ref_score_images, mask_images, viewpoint_cam_lst, scene_extend, radius_ratio=0.1, n_samples=7 * 7,
                                     backend='ball query', calc_depth_points_radius=False, *, depth_images=None):
    """utils/ref_score_utils.py:69-121 (the reference's spelling): as ref_scores_max_pooling over the pixels whose mask is nonzero only.
    Masked-out pixels are neither candidates nor queries and keep their own score; the others keep their order in the full cloud, so
    nothing is compacted; a masked-in pixel with an empty ball keeps its own score.  mask_images: by position or by image_name, as the
    other maps.  With calc_depth_points_radius the two points are sampled from the full cloud."""
    if mask_images is None:
        raise TypeError("ref_scores_max_pooling_wiht_mask: mask_images is None (use ref_scores_max_pooling)")
    return _max_pool("ref_scores_max_pooling_wiht_mask", ref_score_images, mask_images, viewpoint_cam_lst, scene_extend, radius_ratio, n_samples,
                     backend, calc_depth_points_radius, depth_images)


def ref_score_mask(score, threshold, fg_mask=None, *, shape=None):
    """[1,H,W] bool for `priors.ref_score_loss`: score > threshold, and inside `fg_mask` (H*W elements, nonzero = foreground) where one
    is given.  `score` is [H,W] or [1,H,W]; a flat [H*W] score (what calc_ref_score returns) needs shape=(H, W).  This compare is the
    project's own definition -- the reference has no code that produces its masks from the score: parity unpinned.  The reference's step
    between the score and such a compare, the 3D max-pooling across views, is ref_scores_max_pooling above."""
    if shape is None:
        if score.dim() < 2:
            raise ValueError("ref_score_mask: a flat score needs shape=(H, W)")
        shape = tuple(score.shape[-2:])
    H, W = (int(s) for s in shape)
    mask = score.reshape(1, H, W) > threshold
    if fg_mask is not None:
        mask = mask & (torch.as_tensor(fg_mask).to(score.device).reshape(1, H, W) != 0)
    return mask
