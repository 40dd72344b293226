"""Evaluation of a trained model behind the reference's names: `render_set` / `render_set_train` (eval.py:23-102: metric.txt and the image
folders), `evaluate_psnr` and the numeric part of `training_report` (train_refreal.py:1656-1735, the same in the other two scripts),
`visualize_depth` (utils/image_utils.py:73-80) and `save_image` (torchvision.utils.save_image for one image).

The per-view work after the render runs in libmrgs.so (csrc/mrgs_eval.hip): `image_metrics` is two launches that clamp both images as they
are read and write 8 numbers into a row of a device table, `to_rgb8` turns all maps of a view into PNG-ready bytes in at most two launches.
Nothing is read by the host inside the per-view loop: the table is read once after the last view, the bytes travel through a ring of two
pinned buffers and are compressed by a small thread pool while the next view renders.  PNG files are written with the standard library's
zlib; neither PIL, torchvision nor cv2 is needed.  There is no torch fallback: CPU tensors raise.

Differences from the reference (INTEGRATION.md section "Evaluation"): `fps` is 1 / mean of per-view DEVICE times (an event pair around each
render) where eval.py:39-42 times the enqueue; the depth colours come from this library's own jet table (`jet_table`, parity with cv2's
unpinned; the level of each pixel is the reference's); eval.py:56-65 pairs 13 maps with 10 folder names and would raise IndexError on the
eleventh -- here the ten named maps are written and direct_light / visibility / indirect_light go to folders of their own names when the
render's dict has them.
"""
import ctypes
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib

UNIT, NORMAL, DEPTH = _lib.MRGS_EXPORT_UNIT, _lib.MRGS_EXPORT_NORMAL, _lib.MRGS_EXPORT_DEPTH
_MODES = {"unit": UNIT, "normal": NORMAL, "depth": DEPTH, UNIT: UNIT, NORMAL: NORMAL, DEPTH: DEPTH}
# columns of an image_metrics row
PSNR_IMAGE, SSIM, L1, PSNR_CHANNELS = 0, 1, 2, 3
# eval.py:27 (the spelling of the eighth folder is the reference's) -> (key of the render's dict, mode)
DIR_NAMES = ("rgb", "gt", "normal", "surf_normal", "surf_depth", "diffuse_map", "specular_map", "albeldo_map", "roughness_map", "refl_strength_map")
_MAP_OF_DIR = {"rgb": ("render", UNIT), "normal": ("rend_normal", NORMAL), "surf_normal": ("surf_normal", NORMAL), "surf_depth": ("surf_depth", DEPTH),
               "diffuse_map": ("diffuse_map", UNIT), "specular_map": ("specular_map", UNIT), "albeldo_map": ("base_color_map", UNIT),
               "roughness_map": ("roughness_map", UNIT), "refl_strength_map": ("refl_strength_map", UNIT)}
EXTRA_DIR_NAMES = ("direct_light", "visibility", "indirect_light")     # the three maps eval.py:56 lists without a folder
METRIC_FORMAT = "psnr:{}, ssim:{}, lpips:{}, fps:{}"                   # eval.py:71-74


def _device_image(t, what, channels):
    if not torch.is_tensor(t):
        raise TypeError(f"materialrefgs_amd.evaluate: {what} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"materialrefgs_amd.evaluate: {what} must be a device tensor (libmrgs.so has no CPU path)")
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] not in channels or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"materialrefgs_amd.evaluate: {what} must have shape [C,H,W] with C in {channels}, got {tuple(t.shape)}")
    return _lib.f32c(t)


# ---- primitives -------------------------------------------------------------------------------------------------------------------------
def image_metrics(render, gt, out=None):
    """[8] device floats of one view: psnr_image, ssim, l1, psnr_channels, the three per-channel mse, 0 (include/mrgs.h:
    mrgs_eval_metrics).  render [3,H,W], gt [3,H,W] or [4,H,W] (the first three channels are used, eval.py:47); both are clamped to [0, 1]
    as they are read.  `out`: a contiguous float32 device view of 8 elements to write into (a row of a table); returned as given."""
    img = _device_image(render, "render", (3,))
    g = _device_image(gt, "gt", (3, 4))
    if g.shape[1:] != img.shape[1:] or g.device != img.device:
        raise ValueError(f"materialrefgs_amd.evaluate: render {tuple(img.shape)} on {img.device} and gt {tuple(g.shape)} on {g.device} must match")
    dev, (H, W) = img.device, img.shape[1:]
    lib = _lib.lib()
    with _lib.guard(dev):
        if out is None:
            out = torch.empty(8, dtype=torch.float32, device=dev)
        elif out.dtype is not torch.float32 or out.device != dev or out.numel() != 8 or not out.is_contiguous():
            raise ValueError("materialrefgs_amd.evaluate: `out` must be a contiguous float32 view of 8 elements on the images' device")
        ws = torch.empty(lib.mrgs_eval_metrics_ws_bytes(H, W), dtype=torch.uint8, device=dev)
        cfg = _lib.MrgsEvalConfig(H, W, 0)
        _lib.check(lib.mrgs_eval_metrics(ctypes.byref(cfg), img.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                         _lib.stream_ptr(dev)))
    return out


def to_rgb8(maps):
    """maps: (tensor, mode) pairs of one view, tensor [1,H,W] or [3,H,W] (a leading batch of 1 is dropped), mode "unit" / "normal" / "depth"
    (or UNIT / NORMAL / DEPTH) -> device uint8 [K,H,W,3], K <= 16 (include/mrgs.h: mrgs_export_rgb8)."""
    maps = list(maps)
    if not 1 <= len(maps) <= _lib.MRGS_EXPORT_MAX_MAPS:
        raise ValueError(f"materialrefgs_amd.evaluate: to_rgb8 takes 1..{_lib.MRGS_EXPORT_MAX_MAPS} maps, got {len(maps)}")
    held, table = [], (_lib.MrgsExportMap * len(maps))()
    for k, (t, mode) in enumerate(maps):
        if mode not in _MODES:
            raise ValueError(f"materialrefgs_amd.evaluate: unknown mode {mode!r}")
        t = _device_image(t, f"map {k}", (1, 3))
        if held and (t.shape[1:] != held[0].shape[1:] or t.device != held[0].device):
            raise ValueError("materialrefgs_amd.evaluate: the maps of one to_rgb8 call must share H, W and the device")
        held.append(t)
        table[k] = _lib.MrgsExportMap(t.data_ptr(), t.shape[0], _MODES[mode])
    dev, (H, W) = held[0].device, held[0].shape[1:]
    lib = _lib.lib()
    with _lib.guard(dev):
        out = torch.empty((len(maps), H, W, 3), dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.mrgs_export_ws_bytes(), dtype=torch.uint8, device=dev)
        cfg = _lib.MrgsExportConfig(H, W, len(maps), 0)
        _lib.check(lib.mrgs_export_rgb8(ctypes.byref(cfg), table, ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream_ptr(dev)))
    return out


def jet_table():
    """The 256 x 3 RGB table of DEPTH maps as a uint8 array: this library's own jet (include/mrgs.h; parity with cv2's table unpinned)."""
    buf = (ctypes.c_uint8 * 768)()
    _lib.check(_lib.lib().mrgs_eval_jet_table(buf))
    return np.frombuffer(buf, dtype=np.uint8).reshape(256, 3).copy()


def visualize_depth(depth, norm=True):
    """utils/image_utils.py:73-80 without the numpy / cv2 round trip: [3,H,W] float on the depth's device, the table bytes / 255.
    norm=False (the level is x * 255 as it is) is materialrefgs_amd.visualize's."""
    if not norm:
        from . import visualize
        return visualize.visualize_depth(depth, norm=False)
    d = depth.reshape((1,) + tuple(depth.shape[-2:])) if depth.dim() >= 2 else depth
    return to_rgb8([(d, DEPTH)])[0].permute(2, 0, 1).float() / 255.0


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, hwc_uint8, level=6):
    """8-bit RGB, non-interlaced PNG of a host uint8 [H,W,3] array (or CPU tensor), filter type 0 on every row, zlib from the standard
    library."""
    a = hwc_uint8.numpy() if torch.is_tensor(hwc_uint8) else np.asarray(hwc_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"materialrefgs_amd.evaluate: write_png takes a uint8 [H,W,3] array, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)                    # column 0: the filter type of each row
    rows[:, 1:] = a.reshape(H, 3 * W)
    png = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + \
        _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def save_image(tensor, path):
    """torchvision.utils.save_image for ONE image [1|3,H,W] or [1,1|3,H,W] on the device, by the UNIT rule."""
    write_png(path, to_rgb8([(tensor, UNIT)])[0].cpu())


class _PngWriter:
    """The bytes of one view at a time: one non-blocking copy into a ring of two pinned buffers, then one job per file on `workers` threads
    (zlib releases the interpreter lock), so that compression overlaps the next view's render."""

    def __init__(self, workers=4, level=1):
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))
        self.level = level
        self.write = write_png                                         # (path, bytes [H,W,3], level); visualize.TrainingVisualizer writes then renames
        self.ring, self.pending, self.turn = [None, None], [[], []], 0

    def submit(self, dev_u8, paths):
        slot = self.turn
        self.turn ^= 1
        for f in self.pending[slot]:                                   # the slot's previous view has left it
            f.result()
        if self.ring[slot] is None or self.ring[slot].shape != dev_u8.shape:
            self.ring[slot] = torch.empty(dev_u8.shape, dtype=torch.uint8, pin_memory=True)
        host = self.ring[slot]
        host.copy_(dev_u8, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        arr = host.numpy()

        def job(k, path):
            done.synchronize()
            self.write(path, arr[k], self.level)
        self.pending[slot] = [self.pool.submit(job, k, p) for k, p in enumerate(paths)]

    def close(self):
        try:
            for fs in self.pending:
                for f in fs:
                    f.result()
        finally:
            self.pool.shutdown(wait=True)


# ---- eval.py ------------------------------------------------------------------------------------------------------------------------------
def _view_maps(rendering, view):
    """(folder names, (tensor, mode) pairs) of one view: the ten of eval.py:27 and the extra three the render's dict has."""
    names, maps = [], []
    for d in DIR_NAMES:
        if d == "gt":
            t, mode = view.original_image[0:3], UNIT
        else:
            key, mode = _MAP_OF_DIR[d]
            t = rendering[key]
        names.append(d)
        maps.append((t, mode))
    for d in EXTRA_DIR_NAMES:
        if rendering.get(d) is not None:
            names.append(d)
            maps.append((rendering[d], UNIT))
    return names, maps


def _export_view(writer, render_path, idx, rendering, view, made):
    names, maps = _view_maps(rendering, view)
    for d in names:
        if d not in made:
            os.makedirs(os.path.join(render_path, d), exist_ok=True)
            made.add(d)
    writer.submit(to_rgb8(maps), [os.path.join(render_path, d, "{0:05d}.png".format(idx)) for d in names])


@torch.no_grad()
def render_set(model_path, views, gaussians, pipeline, background, save_ims, opt, render, lpips_fn=None, workers=4, png_level=1):
    """eval.py:23-74.  Writes model_path/metric.txt (and, with save_ims, model_path/test/renders/<folder>/<idx>.png), prints the line, and
    returns dict(psnr, ssim, lpips, fps, per_view [n,8] (image_metrics rows), per_view_lpips [n], render_ms [n]).  lpips_fn: a network
    `f(x, y)` on [1,3,H,W] device images (default: lpipsPyTorch.lpips with net_type 'vgg')."""
    if lpips_fn is None:
        from lpipsPyTorch import lpips

        def lpips_fn(x, y):
            return lpips(x, y, net_type="vgg")
    n = len(views)
    render_path = os.path.join(model_path, "test", "renders")
    writer, made = (_PngWriter(workers, png_level), set()) if save_ims else (None, None)
    table = lp = None
    events = []
    try:
        for idx, view in enumerate(views):
            view.refl_mask = None                                      # when evaluating, the reflection mask is disabled
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rendering = render(view, gaussians, pipeline, background, srgb=opt.srgb, opt=opt)
            t1.record()
            events.append((t0, t1))
            image, gt = rendering["render"], view.original_image[0:3]
            if table is None:
                table = torch.zeros((n, 8), dtype=torch.float32, device=image.device)
                lp = torch.zeros(n, dtype=torch.float32, device=image.device)
            image_metrics(image, gt, out=table[idx])
            lp[idx:idx + 1].copy_(lpips_fn(torch.clamp(image, 0.0, 1.0)[None], torch.clamp(gt, 0.0, 1.0)[None]).detach().reshape(1))
            if save_ims:
                _export_view(writer, render_path, idx, rendering, view, made)
    finally:
        if writer is not None:
            writer.close()
    if n:
        host = torch.cat([table, lp[:, None]], dim=1).cpu().numpy()   # the one host read (it also ends every render's event pair)
        per_view, per_lpips = host[:, :8], host[:, 8]
        render_ms = np.array([a.elapsed_time(b) for a, b in events], dtype=np.float64)
    else:
        per_view, per_lpips, render_ms = np.zeros((0, 8), np.float32), np.zeros(0, np.float32), np.zeros(0)
    mean = lambda v: float(np.asarray(v, dtype=np.float64).mean()) if len(v) else float("nan")
    psnr_v, ssim_v, lpip_v = mean(per_view[:, PSNR_IMAGE]), mean(per_view[:, SSIM]), mean(per_lpips)
    fps = 1.0 / (mean(render_ms) * 1e-3) if n else float("nan")
    line = METRIC_FORMAT.format(psnr_v, ssim_v, lpip_v, fps)
    print(line)
    os.makedirs(model_path, exist_ok=True)
    with open(os.path.join(model_path, "metric.txt"), "w") as f:
        f.write(line)
    return {"psnr": psnr_v, "ssim": ssim_v, "lpips": lpip_v, "fps": fps, "per_view": per_view, "per_view_lpips": per_lpips, "render_ms": render_ms}


@torch.no_grad()
def render_set_train(model_path, views, gaussians, pipeline, background, save_ims, opt, render, iteration, workers=4, png_level=1):
    """eval.py:76-102: the image folders of the training views under model_path/train/renders (nothing is measured)."""
    render_path = os.path.join(model_path, "train", "renders")
    writer, made = (_PngWriter(workers, png_level), set()) if save_ims else (None, None)
    try:
        for idx, view in enumerate(views):
            view.refl_mask = None
            rendering = render(view, gaussians, pipeline, background, srgb=opt.srgb, opt=opt)
            if save_ims:
                _export_view(writer, render_path, idx, rendering, view, made)
    finally:
        if writer is not None:
            writer.close()


# ---- train_*.py -----------------------------------------------------------------------------------------------------------------------------
def _metric_rows(cameras, gaussians, renderFunc, renderkwargs, per_view=None):
    """image_metrics of every camera into one device table, read once: float64 [n,8] on the host."""
    table = None
    for idx, viewpoint in enumerate(cameras):
        render_pkg = renderFunc(viewpoint, gaussians, **renderkwargs)
        image = render_pkg["render"]
        if table is None:
            table = torch.zeros((len(cameras), 8), dtype=torch.float32, device=image.device)
        image_metrics(image, viewpoint.original_image.to(image.device), out=table[idx])
        if per_view is not None:
            per_view(viewpoint, image)
    return table.cpu().numpy().astype(np.float64)


def _running_mean(values):
    total = 0.0
    for v in values:                                                   # `x += term.double()` per view, then `/ len`, as the scripts do
        total += float(v)
    return total / len(values)


@torch.no_grad()
def evaluate_psnr(scene, renderFunc, renderkwargs, out_dir="./outputs/evaluate", workers=4, png_level=1):
    """train_refreal.py:1716-1735: the mean over the test cameras of psnr(image, gt).mean() (`psnr_channels`) as a python float, 0.0 without
    test cameras; every render is also saved as out_dir/<image_name>.png (a failed save is skipped, as the script's bare except does)."""
    cameras = list(scene.getTestCameras())
    os.makedirs(out_dir, exist_ok=True)
    if not cameras:
        return 0.0
    writer = _PngWriter(workers, png_level)

    def save(viewpoint, image):
        try:
            writer.submit(to_rgb8([(image, UNIT)]), [os.path.join(out_dir, viewpoint.image_name + ".png")])
        except Exception:
            pass
    try:
        rows = _metric_rows(cameras, scene.gaussians, renderFunc, renderkwargs, per_view=save)
    finally:
        try:
            writer.close()
        except Exception:
            pass
    return _running_mean(rows[:, PSNR_CHANNELS])


@torch.no_grad()
def validation_report(scene, renderFunc, renderkwargs):
    """The numeric part of training_report (train_refreal.py:1663-1708): {"test": (l1, psnr), "train": (l1, psnr)} over the test cameras
    and the training cameras 5, 10, .. 25 (modulo their number); None for a set without cameras.  The TensorBoard calls stay with the
    caller."""
    train = list(scene.getTrainCameras())
    configs = (("test", list(scene.getTestCameras())), ("train", [train[idx % len(train)] for idx in range(5, 30, 5)] if train else []))
    out = {}
    for name, cameras in configs:
        if not cameras:
            out[name] = None
            continue
        rows = _metric_rows(cameras, scene.gaussians, renderFunc, renderkwargs)
        out[name] = (_running_mean(rows[:, L1]), _running_mean(rows[:, PSNR_CHANNELS]))
    return out
