"""Statement of the training contact sheet (csrc/mrgs_sheet.hip behind materialrefgs_amd.visualize), written from the reference's lines:
save_training_vis (train_refreal.py:1513-1620) and visualize_d_mask / visualize_depth / visualize_depth2 (utils/image_utils.py:65-93).
Runs on the CPU with torch / numpy.

fp32 statement (`sheet`): the list of float images the reference's statements build -- a(x) with torch's own matmul, the colour-map helpers
in numpy float32 with the jet table indexed where cv2.applyColorMap stood (tests/eval_statement.py: jet_table) --, torch.stack,
`make_grid` RESTATED below from torchvision's source (torchvision is not installed here: parity with its binary is unpinned, as the jet
table's with cv2), F.interpolate itself, and save_image's UNIT rule (eval_statement.unit_bytes: torch's mul(255).add_(0.5).clamp_(0, 255)
.to(uint8), NaN defined as byte 0).

float64 statement (`pre_values64`): the same arithmetic in float64 up to, but not including, the truncation -- for a normal_view cell the
value of every byte, for a depth2 cell the value of every pixel's level.

NaN: byte / level 0, skipped by min / max / std.  A mask value outside [0, 1] clamps (the reference's astype(uint8) is undefined there).

Tolerance (normal_view, depth2 only): `candidates` returns, beside the fp32 statement's bytes, the bytes one below and one above (normal_view:
the byte -+ 1; depth2: the jet row of the level -+ 1) at the places where the float64 value lies within DELTA of an integer, and the fp32
statement's bytes everywhere else; `accepts` is the comparison.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import eval_statement as es

F32 = np.float32
DELTA = 2.5e-4          # three fp32 roundings of values <= 1.5, scaled by 255, give <= ~7e-5; about three times that
EXACT, BYTEWISE, ROWWISE = 0, 1, 2


# ---- torchvision.utils.make_grid (pad_value 0, no normalisation), restated ------------------------------------------------------------------
def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), dim=0)
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    if tensor.size(0) == 1:                                             # one image: returned as it is
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def layout(n, H, W, nrow=4, padding=2, height=2400):
    """(Hg, Wg, Ho, Wo) from the grid's own shape and :1605-1606."""
    grid = make_grid(torch.zeros(n, 1, H, W), nrow=nrow, padding=padding)
    if height is None:
        return grid.shape[-2], grid.shape[-1], grid.shape[-2], grid.shape[-1]
    scale = grid.shape[-2] / height
    return grid.shape[-2], grid.shape[-1], int(grid.shape[-2] / scale), int(grid.shape[-1] / scale)


def nearest_index(out_size, in_size):
    """The source index of every destination index: min((int)floorf(dst * s), in - 1), s = (float)in / (float)out, one fp32 multiply."""
    s = F32(in_size) / F32(out_size)
    dst = np.arange(out_size, dtype=np.int64).astype(F32)
    return np.minimum(np.floor(dst * s).astype(np.int64), in_size - 1)


def resample(grid, Ho, Wo):
    return F.interpolate(grid[None], (Ho, Wo))[0]                       # :1606


# ---- the derived images --------------------------------------------------------------------------------------------------------------------
def a_view(x, rot):
    """:1521-1524 in x's dtype."""
    sz = x.shape
    x = (rot @ x.reshape(3, -1)).reshape(*sz)[[2, 1, 0], ...]
    return 0.5 * x + 0.5


def _jet_image(levels):
    """depth_c = table[levels] as the helpers return it: [3,H,W] float32, the table bytes / 255."""
    return torch.from_numpy(es.jet_table()[levels]).float().permute(2, 0, 1) / 255.


def _map2d(t, H, W):
    return np.asarray(t.detach().float().numpy() if torch.is_tensor(t) else t, dtype=F32).reshape(H, W)


def level_levels(x):
    with np.errstate(all="ignore"):
        return es._bytes(np.asarray(x, dtype=F32) * F32(255))            # (depth * 255).clip(0, 255).astype(np.uint8)


def mask_levels(m, H, W):
    m = m.detach() if torch.is_tensor(m) else torch.as_tensor(m)
    with np.errstate(all="ignore"):
        return es._bytes((m.float() * 255).numpy().astype(F32).reshape(H, W))


def _nanstd(d):
    v = d[~np.isnan(d)]
    with np.errstate(all="ignore"):
        return v.std() if v.size else d.dtype.type(np.nan)


def depth2_clipped(d):
    """image_utils.py:86-87 in d's dtype: std over the map (NaN skipped), clip to [0, 6 std]."""
    with np.errstate(all="ignore"):
        std = _nanstd(d)
        return np.clip(d, d.dtype.type(0), d.dtype.type(6) * std)


def depth2_levels(d):
    return es.depth_levels(depth2_clipped(np.asarray(d, dtype=F32)))


def depth2_pre64(d):
    """The level's value before the truncation, float64."""
    c = depth2_clipped(np.asarray(d, dtype=F32).astype(np.float64))
    with np.errstate(all="ignore"):
        mn, mx = (np.nanmin(c), np.nanmax(c)) if not np.isnan(c).all() else (np.inf, -np.inf)
        return ((c - mn) / (1e-20 + mx - mn)) * 255.0


def cell_shape(cells):
    for t, mode in cells:
        t = t[0] if isinstance(t, (tuple, list)) else t
        if t.dim() >= 2:
            return int(t.shape[-2]), int(t.shape[-1])
    raise ValueError("no cell with H and W")


def cell_image(cell, rot, H, W):
    """One entry of visualization_list: [3,H,W] float32."""
    t, mode = cell
    if mode == "unit":
        return t.float().repeat(3, 1, 1) if t.shape[0] == 1 else t.float()
    if mode == "absdiff":
        return torch.abs(t[0].float() - t[1].float())                   # :1518
    if mode == "normal_view":
        return a_view(t.float(), torch.as_tensor(rot, dtype=torch.float32))
    if mode == "depth":
        return _jet_image(es.depth_levels(_map2d(t, H, W)))
    if mode == "level":
        return _jet_image(level_levels(_map2d(t, H, W)))
    if mode == "depth2":
        return _jet_image(depth2_levels(_map2d(t, H, W)))
    if mode == "mask":
        return _jet_image(mask_levels(t, H, W))
    raise ValueError(mode)


def _near(pre):
    with np.errstate(all="ignore"):
        return np.isfinite(pre) & (np.abs(pre - np.rint(pre)) <= DELTA)


def pre_values64(cell, rot, H, W):
    """normal_view: [3,H,W] float64 values of the bytes before clamp and truncation; depth2: [H,W] values of the level."""
    t, mode = cell
    if mode == "normal_view":
        return (a_view(t.double(), torch.as_tensor(np.asarray(rot, dtype=F32)).double()) * 255 + 0.5).numpy()
    if mode == "depth2":
        return depth2_pre64(_map2d(t, H, W))
    raise ValueError(mode)


def bytes64(cell, rot, H, W):
    """The float64 statement truncated: [3,H,W] bytes (normal_view) or [H,W] levels (depth2)."""
    return es._bytes(pre_values64(cell, rot, H, W))


def cell_candidates(cell, rot, H, W):
    """(want, minus, plus, kind): uint8 [3,H,W] each and the comparison of the cell."""
    want = es.unit_bytes(cell_image(cell, rot, H, W).numpy())
    mode = cell[1]
    if mode == "normal_view":
        near = _near(pre_values64(cell, rot, H, W))
        w = want.astype(np.int64)
        return want, np.where(near, np.clip(w - 1, 0, 255), w).astype(np.uint8), np.where(near, np.clip(w + 1, 0, 255), w).astype(np.uint8), BYTEWISE
    if mode == "depth2":
        near = _near(depth2_pre64(_map2d(cell[0], H, W)))
        L = depth2_levels(_map2d(cell[0], H, W)).astype(np.int64)
        table = es.jet_table()
        lo, hi = np.where(near, np.clip(L - 1, 0, 255), L), np.where(near, np.clip(L + 1, 0, 255), L)
        return want, table[lo].transpose(2, 0, 1), table[hi].transpose(2, 0, 1), ROWWISE
    return want, want, want, EXACT


def _through(images, nrow, padding, Ho, Wo):
    """stack, make_grid, interpolate, save_image's bytes: uint8 [Ho,Wo,3]."""
    grid = make_grid(torch.stack(images, dim=0), nrow=nrow, padding=padding)
    if (Ho, Wo) != tuple(grid.shape[-2:]):
        grid = resample(grid, Ho, Wo)
    return es.unit_bytes(grid.numpy()).transpose(1, 2, 0)


def sheet(cells, nrow=4, padding=2, height=2400, rot=None, hw=None):
    """The fp32 statement: uint8 [Ho,Wo,3].  hw: (H, W) when no cell has them (a flat mask alone)."""
    H, W = hw or cell_shape(cells)
    _, _, Ho, Wo = layout(len(cells), H, W, nrow, padding, height)
    return _through([cell_image(c, rot, H, W) for c in cells], nrow, padding, Ho, Wo)


def candidates(cells, nrow=4, padding=2, height=2400, rot=None, hw=None):
    """(want, minus, plus, kind): three uint8 [Ho,Wo,3] and the per-pixel comparison [Ho,Wo] (EXACT / BYTEWISE / ROWWISE; 0 on borders and
    empty places), every one laid out and resampled as the sheet is."""
    H, W = hw or cell_shape(cells)
    _, _, Ho, Wo = layout(len(cells), H, W, nrow, padding, height)
    per = [cell_candidates(c, rot, H, W) for c in cells]
    as_img = lambda b: torch.from_numpy(np.ascontiguousarray(b)).float() / 255.       # a byte passes the UNIT rule unchanged
    outs = [_through([as_img(p[j]) for p in per], nrow, padding, Ho, Wo) for j in range(3)]
    kind = _through([as_img(np.full((3, H, W), p[3], dtype=np.uint8)) for p in per], nrow, padding, Ho, Wo)[..., 0]
    return outs[0], outs[1], outs[2], kind


def accepts(got, want, minus, plus, kind):
    """The accuracy rule: exact cells, borders and empty places equal `want`; a bytewise cell's byte equals one of the three candidates; a
    rowwise cell's pixel equals one of the three candidate rows as a whole.  Returns (ok, number of bytes that differ from want)."""
    got = np.asarray(got)
    eq = got == want
    by = eq | (got == minus) | (got == plus)
    row = eq.all(-1) | (got == minus).all(-1) | (got == plus).all(-1)
    ok = np.where(kind == EXACT, eq.all(-1), np.where(kind == BYTEWISE, by.all(-1), row))
    return bool(ok.all()), int((~eq).sum())


# ---- the list of save_training_vis ------------------------------------------------------------------------------------------------------------
def training_list(viewpoint_cam, render_pkg, opt, iteration, initial_stage, d_mask, ref_weight, base_color_loss_map, ref_score=None):
    """:1518-1601 as cells of this statement (tensors on the CPU), line by line."""
    gt = viewpoint_cam.original_image
    error_map = ((gt, render_pkg["render"]), "absdiff")                 # :1518
    a = lambda x: (x, "normal_view")                                    # :1521-1524
    rep = lambda x: (x, "unit")                                         # .repeat(3, 1, 1)
    depth = lambda x: (x, "depth")                                      # visualize_depth
    if initial_stage:
        lst = [(gt, "unit"), (render_pkg["render"], "unit"), rep(render_pkg["rend_alpha"]), depth(render_pkg["surf_depth"]),
               a(render_pkg["rend_normal"]), a(render_pkg["surf_normal"]), error_map]
    elif iteration <= opt.volume_render_until_iter:
        lst = [(gt, "unit"), (render_pkg["render"], "unit"), (render_pkg["base_color_map"], "unit"), (render_pkg["diffuse_map"], "unit"),
               (render_pkg["specular_map"], "unit"), rep(render_pkg["refl_strength_map"]), rep(render_pkg["roughness_map"]),
               rep(render_pkg["rend_alpha"]), depth(render_pkg["surf_depth"]), a(render_pkg["rend_normal"]), a(render_pkg["surf_normal"]), error_map]
        if opt.indirect:
            lst += [rep(render_pkg["visibility"]), (render_pkg["direct_light"], "unit"), (render_pkg["indirect_light"], "unit")]
    else:
        lst = [(gt, "unit"), (render_pkg["render"], "unit"), (render_pkg["base_color_map"], "unit"), (render_pkg["diffuse_map"], "unit"),
               (render_pkg["specular_map"], "unit"), rep(render_pkg["refl_strength_map"]), rep(render_pkg["roughness_map"]),
               rep(render_pkg["rend_alpha"]), depth(render_pkg["surf_depth"]), a(render_pkg["rend_normal"]), a(render_pkg["surf_normal"]), error_map]
    if "rend_distance" in render_pkg.keys():
        lst.append(depth(render_pkg["rend_distance"]))
    if d_mask is not None:
        lst.append((d_mask, "mask"))
    if ref_weight is not None:
        lst.append((ref_weight, "level"))
    if base_color_loss_map is not None:
        lst.append((base_color_loss_map, "depth2"))
    if "visibility" in render_pkg.keys():
        lst += [rep(render_pkg["visibility"]), (render_pkg["direct_light"], "unit"), (render_pkg["indirect_light"], "unit")]
    if "indirect_out" in render_pkg.keys():
        lst += [(render_pkg["indirect_out"]["render"], "unit"), rep(render_pkg["indirect_out"]["specular"]),
                rep(render_pkg["indirect_out"]["rend_alpha"])]
    if ref_score is not None:
        lst.append(rep(ref_score))
    return lst
