"""The training contact sheet behind the reference's names: `save_training_vis` (train_refreal.py:1513-1620, train_refnerf.py:1533-1640,
train_glossy.py:1588-1695) and the three colour-map helpers it calls, `visualize_depth`, `visualize_depth2` and `visualize_d_mask`
(utils/image_utils.py:65-93).

The reference builds up to 23 fp32 images (four of them through numpy and cv2 on the host), stacks them, runs torchvision's make_grid,
F.interpolate to 2400 rows and save_image.  Here `contact_sheet` is at most two launches of libmrgs.so (csrc/mrgs_sheet.hip): every byte of
the PNG is computed from the render's own maps -- the cell's rule, make_grid's placement and the nearest-neighbour resample in one
output-driven kernel.  Nothing is read by the host; with a `TrainingVisualizer` the bytes travel through evaluate._PngWriter's pinned ring
and zlib runs on a worker thread while training goes on.  Neither cv2 nor torchvision is needed.  There is no torch fallback.

Differences from the reference (INTEGRATION.md section "The training contact sheet"): the folder is the `visualize_path` keyword where the
script reads a global `args`; the jet colours are this library's own table (evaluate.jet_table; parity with cv2's unpinned, the LEVEL of
each pixel is the reference's); parity with torchvision's make_grid binary is unpinned as well (it is not installed here): the placement
is restated from its source.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._camconst import consts
from .evaluate import _PngWriter, write_png

(UNIT, ABSDIFF, NORMAL_VIEW, DEPTH, LEVEL, DEPTH2, MASK) = (_lib.MRGS_SHEET_UNIT, _lib.MRGS_SHEET_ABSDIFF, _lib.MRGS_SHEET_NORMAL_VIEW,
                                                            _lib.MRGS_SHEET_DEPTH, _lib.MRGS_SHEET_LEVEL, _lib.MRGS_SHEET_DEPTH2, _lib.MRGS_SHEET_MASK)
MODE_NAMES = ("unit", "absdiff", "normal_view", "depth", "level", "depth2", "mask")
_MODES = {**{n: k for k, n in enumerate(MODE_NAMES)}, **{k: k for k in range(len(MODE_NAMES))}}
MAX_CELLS = _lib.MRGS_SHEET_MAX_CELLS


def sheet_layout(n, H, W, nrow=4, padding=2, height=2400):
    """(Hg, Wg, Ho, Wo): the grid torchvision.utils.make_grid builds of n images of H x W and the size :1605-1606 resamples it to, in the
    reference's own expressions on Python floats (Ho is what they give, not `height` by assumption).  height=None: no resample."""
    if n < 1:
        raise ValueError(f"materialrefgs_amd.visualize: a sheet needs at least one cell, got {n}")
    if n == 1:                                                         # make_grid returns one image as it is
        Hg, Wg = H, W
    else:
        xmaps = min(nrow, n)
        ymaps = int(math.ceil(float(n) / xmaps))
        Hg, Wg = (H + padding) * ymaps + padding, (W + padding) * xmaps + padding
    if height is None:
        return Hg, Wg, Hg, Wg
    scale = Hg / height
    return Hg, Wg, int(Hg / scale), int(Wg / scale)


def _plane(t, what, dev):
    if not torch.is_tensor(t):
        raise TypeError(f"materialrefgs_amd.visualize: {what} must be a tensor, got {type(t).__name__}")
    if dev is not None and not t.is_cuda:
        t = t.to(dev)                                                  # an optional map that arrives on the CPU (calc_warp_loss_refreal's zero weight)
    return t


def _cell_tensors(cell, k):
    t, mode = cell
    if mode not in _MODES:
        raise ValueError(f"materialrefgs_amd.visualize: unknown mode {mode!r}")
    mode = _MODES[mode]
    pair = isinstance(t, (tuple, list))
    if pair != (mode == ABSDIFF) or (pair and len(t) != 2):
        raise ValueError(f"materialrefgs_amd.visualize: cell {k}: absdiff takes a pair of tensors, every other mode one tensor")
    return (list(t) if pair else [t]), mode


def contact_sheet(cells, nrow=4, padding=2, height=2400, rot=None):
    """cells: (tensor, mode) pairs -- for "absdiff" ((a, b), mode) -- of one H x W; mode "unit" [1|3,H,W], "absdiff" two [3,H,W],
    "normal_view" [3,H,W] (needs rot, the 3x3 of a(x)), "depth" / "level" / "depth2" one channel of H W values, "mask" H W values of
    bool / uint8 / float32 -> device uint8 [Ho,Wo,3], the bytes save_image would write of the resampled grid (include/mrgs.h:
    mrgs_sheet_rgb8; sheet_layout gives Ho, Wo).  Device tensors; a cell that arrives on the CPU is uploaded to the others' device."""
    cells = [_cell_tensors(c, k) for k, c in enumerate(cells)]
    if not 1 <= len(cells) <= MAX_CELLS:
        raise ValueError(f"materialrefgs_amd.visualize: contact_sheet takes 1..{MAX_CELLS} cells, got {len(cells)}")
    dev = next((t.device for ts, _ in cells for t in ts if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        raise RuntimeError("materialrefgs_amd.visualize: the cells must be device tensors (libmrgs.so has no CPU path)")
    H = W = None
    held, table = [], (_lib.MrgsSheetCell * len(cells))()
    for k, (ts, mode) in enumerate(cells):
        ts = [_plane(t, f"cell {k}", dev) for t in ts]
        if any(t.device != dev for t in ts):
            raise ValueError("materialrefgs_amd.visualize: the cells of one sheet must share the device")
        if mode in (UNIT, ABSDIFF, NORMAL_VIEW):
            ts = [t[0] if t.dim() == 4 and t.shape[0] == 1 else t for t in ts]
            chans = (1, 3) if mode == UNIT else (3,)
            for t in ts:
                if t.dim() != 3 or t.shape[0] not in chans or t.shape[1] < 1 or t.shape[2] < 1:
                    raise ValueError(f"materialrefgs_amd.visualize: cell {k} ({MODE_NAMES[mode]}) must have shape [C,H,W] with C in {chans}, "
                                     f"got {tuple(t.shape)}")
                if H is None:
                    H, W = int(t.shape[1]), int(t.shape[2])
            channels, elem = int(ts[0].shape[0]), _lib.MRGS_SHEET_ELEM_F32
            ts = [_lib.f32c(t) for t in ts]
        else:                                                          # one value per pixel in any shape (the helpers squeeze / reshape)
            t = ts[0]
            if H is None:
                if t.dim() < 2:
                    raise ValueError(f"materialrefgs_amd.visualize: cell {k}: a sheet whose first cell is flat has no H and W")
                H, W = int(t.shape[-2]), int(t.shape[-1])
            channels = 1
            if mode == MASK and t.dtype in (torch.bool, torch.uint8):
                elem, ts = _lib.MRGS_SHEET_ELEM_U8, [t.detach().contiguous()]
            else:
                elem, ts = _lib.MRGS_SHEET_ELEM_F32, [_lib.f32c(t)]
        for t in ts:
            if t.numel() != channels * H * W or (t.dim() >= 2 and mode in (UNIT, ABSDIFF, NORMAL_VIEW) and tuple(t.shape[1:]) != (H, W)):
                raise ValueError(f"materialrefgs_amd.visualize: the cells of one sheet must share H and W: cell {k} has {tuple(t.shape)}, the sheet "
                                 f"{H} x {W}")
        held.append(ts)
        table[k] = _lib.MrgsSheetCell(ts[0].data_ptr(), ts[1].data_ptr() if len(ts) > 1 else None, channels, mode, elem, 0)
    needs_rot = any(mode == NORMAL_VIEW for _, mode in cells)
    if needs_rot and rot is None:
        raise ValueError("materialrefgs_amd.visualize: a normal_view cell needs `rot`")
    r9 = (ctypes.c_float * 9)(*(np.asarray(rot.detach().cpu() if torch.is_tensor(rot) else rot, dtype=np.float32).reshape(9).tolist()
                                if rot is not None else [0.0] * 9))
    Hg, Wg, Ho, Wo = sheet_layout(len(cells), H, W, nrow, padding, height)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"materialrefgs_amd.visualize: height {height} leaves no pixel of the {Hg} x {Wg} grid")
    sy, sx = float(np.float32(Hg) / np.float32(Ho)), float(np.float32(Wg) / np.float32(Wo))        # F.interpolate's fp32 scales
    lib = _lib.lib()
    with _lib.guard(dev):
        out = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device=dev)
        stats = any(mode in (DEPTH, DEPTH2) for _, mode in cells)
        ws = torch.empty(lib.mrgs_sheet_ws_bytes(), dtype=torch.uint8, device=dev) if stats else None
        cfg = _lib.MrgsSheetConfig(H, W, len(cells), nrow, padding, Ho, Wo, sy, sx, r9, 0)
        _lib.check(lib.mrgs_sheet_rgb8(ctypes.byref(cfg), table, _lib.ptr(ws), ws.numel() if stats else 0, out.data_ptr(), _lib.stream_ptr(dev)))
    return out


# ---- the single-map helpers of utils/image_utils.py -----------------------------------------------------------------------------------------
def _one_cell(t, mode):
    return contact_sheet([(t, mode)], nrow=1, padding=0, height=None).permute(2, 0, 1).float() / 255.0


def visualize_depth(depth, norm=True):
    """utils/image_utils.py:73-80 without the numpy / cv2 round trip: [3,H,W] float on the depth's device, the table bytes / 255."""
    return _one_cell(depth.reshape((1,) + tuple(depth.shape[-2:])), DEPTH if norm else LEVEL)


def visualize_depth2(depth):
    """utils/image_utils.py:83-93: the map clipped to [0, 6 std] before it is normalised."""
    return _one_cell(depth.reshape((1,) + tuple(depth.shape[-2:])), DEPTH2)


def visualize_d_mask(d_mask, H, W):
    """utils/image_utils.py:65-70: d_mask of H W values (bool, uint8 or float) -> [3,H,W] float."""
    return _one_cell(d_mask.reshape(H, W), MASK)


# ---- save_training_vis ------------------------------------------------------------------------------------------------------------------------
def view_rotation(viewpoint_cam, device=None):
    """`viewpoint_cam.R.T.float()` (:1519) as a float32 [3,3] host array, from the camera's constants on `device` (default: where R is)."""
    device = device or getattr(viewpoint_cam.R, "device", torch.device("cpu"))
    return np.array(consts(viewpoint_cam, device).rt_host, dtype=np.float32).reshape(3, 3)


def training_cells(viewpoint_cam, render_pkg, opt, iteration, initial_stage, d_mask=None, ref_weight=None, base_color_loss_map=None,
                   ref_score=None):
    """The (name, cell) list of :1525-1601 in the reference's order: the three stage branches, then every optional tail entry.  A cell is
    what contact_sheet takes; only the list is built here (no tensor is touched)."""
    gt, pkg = viewpoint_cam.original_image[0:3], render_pkg
    head = [("gt", (gt, UNIT)), ("render", (pkg["render"], UNIT))]
    tail = [("rend_alpha", (pkg["rend_alpha"], UNIT)), ("surf_depth", (pkg["surf_depth"], DEPTH)), ("rend_normal", (pkg["rend_normal"], NORMAL_VIEW)),
            ("surf_normal", (pkg["surf_normal"], NORMAL_VIEW)), ("error_map", ((gt, pkg["render"]), ABSDIFF))]
    if initial_stage:
        cells = head + tail
    else:                                                              # the volume stage (:1536) and the surfel stage (:1558) list the same twelve
        cells = head + [(k, (pkg[k], UNIT)) for k in ("base_color_map", "diffuse_map", "specular_map", "refl_strength_map", "roughness_map")] + tail
        if iteration <= opt.volume_render_until_iter and opt.indirect:
            cells += [(k, (pkg[k], UNIT)) for k in ("visibility", "direct_light", "indirect_light")]
    if "rend_distance" in pkg.keys():
        cells.append(("rend_distance", (pkg["rend_distance"], DEPTH)))
    if d_mask is not None:
        cells.append(("d_mask", (d_mask, MASK)))
    if ref_weight is not None:
        cells.append(("ref_weight", (ref_weight, LEVEL)))
    if base_color_loss_map is not None:
        cells.append(("base_color_loss_map", (base_color_loss_map, DEPTH2)))
    if "visibility" in pkg.keys():                                     # with opt.indirect in the volume stage the three are listed twice, as the reference does
        cells += [(k, (pkg[k], UNIT)) for k in ("visibility", "direct_light", "indirect_light")]
    if "indirect_out" in pkg.keys():
        ind = pkg["indirect_out"]
        cells += [("indirect_out.render", (ind["render"], UNIT)), ("indirect_out.specular", (ind["specular"], UNIT)),
                  ("indirect_out.rend_alpha", (ind["rend_alpha"], UNIT))]
    if ref_score is not None:
        cells.append(("ref_score", (ref_score, UNIT)))
    return cells


def write_png_atomic(path, hwc_uint8, level=6):
    """evaluate.write_png under a temporary name in the same folder, then a rename: a reader never finds a half-written file behind `path`."""
    folder, name = os.path.split(path)
    tmp = os.path.join(folder, f".{name}.{os.getpid()}.part")
    try:
        write_png(tmp, hwc_uint8, level)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


@torch.no_grad()
def save_training_vis(viewpoint_cam, gaussians, background, render_fn, pipe, opt, iteration, initial_stage, d_mask, ref_weight,
                      base_color_loss_map, render_pkg=None, ref_score=None, *, visualize_path, writer=None, height=2400):
    """train_refreal.py:1513-1620.  Writes visualize_path/{iteration:06d}.png and, outside the initial stage, {iteration:06d}_env.png (the two
    environment panoramas, nrow 1, padding 10, no resample).  writer: a TrainingVisualizer -- the call returns after enqueueing the copies;
    without one the files are written before it returns.  Returns the list of paths."""
    if render_pkg is None:
        render_pkg = render_fn(viewpoint_cam, gaussians, pipe, background, srgb=opt.srgb, opt=opt)
    # (the one-value maps come in the shapes the scripts hand over -- [H,W], [1,H,W], [H W] --: the first cell gives the sheet its H and W)
    cells = [cell for _name, cell in training_cells(viewpoint_cam, render_pkg, opt, iteration, initial_stage, d_mask, ref_weight,
                                                    base_color_loss_map, ref_score)]
    os.makedirs(visualize_path, exist_ok=True)
    jobs = [(contact_sheet(cells, nrow=4, padding=2, height=height, rot=view_rotation(viewpoint_cam, render_pkg["render"].device)),
             os.path.join(visualize_path, f"{iteration:06d}.png"))]
    if not initial_stage:
        if opt.volume_render_until_iter > opt.init_until_iter and iteration <= opt.volume_render_until_iter:
            env_dict = gaussians.render_env_map_2()
        else:
            env_dict = gaussians.render_env_map()
        env = [(env_dict["env1"].permute(2, 0, 1), UNIT), (env_dict["env2"].permute(2, 0, 1), UNIT)]
        jobs.append((contact_sheet(env, nrow=1, padding=10, height=None), os.path.join(visualize_path, f"{iteration:06d}_env.png")))
    for sheet, path in jobs:
        if writer is not None:
            writer.submit(sheet, path)
        else:
            write_png_atomic(path, sheet.cpu())
    return [path for _, path in jobs]


class TrainingVisualizer:
    """save_training_vis that does not wait for the PNG: `save(...)` takes save_training_vis' arguments (the folder is this object's) and
    returns once the sheet's copy into a pinned buffer is enqueued; zlib and the file run on `workers` threads.  Files appear under their
    final names only when complete (write_png_atomic).  `close()` waits for everything and must be called before the files are relied on."""

    def __init__(self, visualize_path, workers=1, png_level=1):
        self.visualize_path = visualize_path
        self._writer = _PngWriter(workers, png_level)
        self._writer.write = write_png_atomic
        self._closed = False

    def submit(self, sheet, path):
        self._writer.submit(sheet[None], [path])                       # [1,Ho,Wo,3]: one file of the ring's view

    def save(self, viewpoint_cam, gaussians, background, render_fn, pipe, opt, iteration, initial_stage, d_mask=None, ref_weight=None,
             base_color_loss_map=None, render_pkg=None, ref_score=None, height=2400):
        return save_training_vis(viewpoint_cam, gaussians, background, render_fn, pipe, opt, iteration, initial_stage, d_mask, ref_weight,
                                 base_color_loss_map, render_pkg, ref_score, visualize_path=self.visualize_path, writer=self, height=height)

    def close(self):
        if not self._closed:
            self._closed = True
            self._writer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
