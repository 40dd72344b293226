"""The host side of the training contact sheet (materialrefgs_amd.visualize, csrc/mrgs_sheet.hip) without a GPU: the layout, the
statement's index rule against F.interpolate, the statement's own accuracy rule (fp32 against float64), the list save_training_vis builds,
the argument checks of mrgs_sheet_rgb8 and the writer's write-then-rename."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_statement as es  # noqa: E402
import sheet_statement as ss  # noqa: E402
from test_eval_export import read_png  # noqa: E402


# ---------------------------------------------------------------- layout
def test_layout_worked_values():
    from materialrefgs_amd import visualize as vz
    assert vz.sheet_layout(7, 800, 800) == (1606, 3210, 2400, 4797)
    assert vz.sheet_layout(12, 800, 800) == (2408, 3210, 2400, 3199)
    assert vz.sheet_layout(19, 800, 800) == (4012, 3210, 2400, 1920)
    assert vz.sheet_layout(12, 1200, 1600) == (3608, 6410, 2400, 4263)
    assert vz.sheet_layout(9, 37, 53) == (119, 222, 2400, 4477)
    assert vz.sheet_layout(1, 37, 53, height=None) == (37, 53, 37, 53)            # make_grid's early return: no border
    assert vz.sheet_layout(2, 16, 32, nrow=1, padding=10, height=None) == (62, 52, 62, 52)
    with pytest.raises(ValueError):
        vz.sheet_layout(0, 5, 7)


@pytest.mark.parametrize("n", (1, 2, 4, 5, 7, 13, 19, 32))
def test_layout_is_the_statements(n):
    from materialrefgs_amd import visualize as vz
    for (H, W) in ((5, 7), (37, 53)):
        for nrow, padding in ((4, 2), (1, 10), (8, 0)):
            for height in (2400, 301, 120, None):
                assert vz.sheet_layout(n, H, W, nrow, padding, height) == ss.layout(n, H, W, nrow, padding, height), (n, H, W, nrow, padding, height)


@pytest.mark.parametrize("sizes", ((1606, 2400), (3210, 4797), (4012, 2400), (16, 2400), (2400, 2400), (119, 301), (222, 561), (781, 120),
                                   (222, 34), (7, 7), (5, 1), (1, 9)))
def test_statement_index_rule_is_interpolates(sizes):
    """Upsampling, downsampling and equal sizes: min((int)floorf(dst * s), in - 1) with s = (float)in / (float)out in fp32."""
    n_in, n_out = sizes
    src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
    got = F.interpolate(src, (n_out, 1))[0, 0, :, 0].numpy().astype(np.int64)
    assert np.array_equal(ss.nearest_index(n_out, n_in), got)
    if n_in == n_out:
        assert np.array_equal(got, np.arange(n_in))


def test_make_grid_restated_places_cells_and_zeroes_the_rest():
    imgs = torch.arange(1, 6, dtype=torch.float32).reshape(5, 1, 1, 1).expand(5, 3, 2, 3).contiguous()
    g = ss.make_grid(imgs, nrow=4, padding=2)
    assert tuple(g.shape) == (3, 10, 22)
    for k in range(5):
        y, x = (k // 4) * 4 + 2, (k % 4) * 5 + 2
        assert (g[:, y:y + 2, x:x + 3] == k + 1).all()
    assert float(g.sum()) == 3 * 6 * (1 + 2 + 3 + 4 + 5)                            # everything else, the unused places included, is 0
    assert ss.make_grid(imgs[:1], nrow=4, padding=2).shape == (3, 2, 3)            # one image: itself


# ---------------------------------------------------------------- the statement keeps its own rule
def _unit_normals(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(3, H, W, generator=g)
    return n / n.norm(dim=0, keepdim=True)


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q.astype(np.float32)


def test_fp32_statement_satisfies_the_rule_against_float64():
    """normal_view bytes and depth2 levels of the fp32 statement equal the float64 statement's or differ by one, and only where the float64
    value lies within DELTA of an integer -- on the inputs the GPU tests use and on a larger map."""
    for (H, W), seed in (((5, 7), 1), ((37, 53), 2), ((200, 300), 3)):
        rot = _rotation(seed)
        cell = (_unit_normals(H, W, seed), "normal_view")
        want = es.unit_bytes(ss.cell_image(cell, rot, H, W).numpy()).astype(np.int64)
        pre = ss.pre_values64(cell, rot, H, W)
        d = want - ss.bytes64(cell, rot, H, W).astype(np.int64)
        assert np.abs(d).max() <= 1 and ss._near(pre)[d != 0].all()
        assert ss._near(pre).mean() < 2e-3                                          # the allowance is a small set
        g = torch.Generator().manual_seed(seed)
        m = torch.rand(1, H, W, generator=g) ** 4
        m[0, 0, 0] = 40.0                                                            # one value far above 6 std
        cell = (m, "depth2")
        L = ss.depth2_levels(m[0].numpy()).astype(np.int64)
        pre = ss.pre_values64(cell, None, H, W)
        d = L - ss.bytes64(cell, None, H, W).astype(np.int64)
        assert np.abs(d).max() <= 1 and ss._near(pre)[d != 0].all()


def test_a_table_byte_passes_the_unit_rule_unchanged():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(es.unit_bytes((torch.from_numpy(b).float() / 255.).numpy()), b)


# ---------------------------------------------------------------- the list of save_training_vis
def _pkg(H=3, W=4, extra=()):
    z3, z1 = torch.zeros(3, H, W), torch.zeros(1, H, W)
    pkg = {"render": z3 + 0.1, "rend_alpha": z1 + 0.2, "surf_depth": z1 + 0.3, "rend_normal": z3 + 0.4, "surf_normal": z3 + 0.5,
           "base_color_map": z3 + 0.6, "diffuse_map": z3 + 0.7, "specular_map": z3 + 0.8, "refl_strength_map": z1 + 0.9, "roughness_map": z1 + 1.0}
    for k in extra:
        if k == "indirect_out":
            pkg[k] = {"render": z3 + 2.0, "specular": z1 + 2.1, "rend_alpha": z1 + 2.2}
        else:
            pkg[k] = (z3 if k in ("direct_light", "indirect_light") else z1) + 3.0
    return pkg


INITIAL = [("gt", "unit"), ("render", "unit"), ("rend_alpha", "unit"), ("surf_depth", "depth"), ("rend_normal", "normal_view"),
           ("surf_normal", "normal_view"), ("error_map", "absdiff")]
FULL = [("gt", "unit"), ("render", "unit"), ("base_color_map", "unit"), ("diffuse_map", "unit"), ("specular_map", "unit"),
        ("refl_strength_map", "unit"), ("roughness_map", "unit")] + INITIAL[2:]
LIGHTS = [("visibility", "unit"), ("direct_light", "unit"), ("indirect_light", "unit")]


def _names_modes(cells):
    from materialrefgs_amd import visualize as vz
    return [(name, vz.MODE_NAMES[mode]) for name, (_t, mode) in cells]


def test_training_cells_follow_the_reference_list():
    from materialrefgs_amd import visualize as vz
    H, W = 3, 4
    cam = SimpleNamespace(original_image=torch.zeros(3, H, W) + 0.05, R=np.eye(3))
    opt = SimpleNamespace(volume_render_until_iter=100, init_until_iter=50, indirect=False)
    opt_ind = SimpleNamespace(volume_render_until_iter=100, init_until_iter=50, indirect=True)
    # the three stage branches
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 10, True)) == INITIAL
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 60, False)) == FULL                     # volume stage
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 200, False)) == FULL                    # surfel stage
    # opt.indirect in the volume stage and the later `"visibility" in render_pkg` tail: the three light maps are listed twice
    lights = ("visibility", "direct_light", "indirect_light")
    assert _names_modes(vz.training_cells(cam, _pkg(extra=lights), opt_ind, 60, False)) == FULL + LIGHTS + LIGHTS
    assert _names_modes(vz.training_cells(cam, _pkg(extra=lights), opt_ind, 200, False)) == FULL + LIGHTS
    assert _names_modes(vz.training_cells(cam, _pkg(extra=lights), opt, 60, False)) == FULL + LIGHTS
    assert _names_modes(vz.training_cells(cam, _pkg(extra=lights), opt_ind, 10, True)) == INITIAL + LIGHTS
    # every optional tail entry, alone and all together, in the reference's order
    d_mask, w, bl, rs = torch.ones(H * W, dtype=torch.bool), torch.zeros(1, H, W), torch.zeros(H, W), torch.zeros(1, H, W)
    assert _names_modes(vz.training_cells(cam, _pkg(extra=("rend_distance",)), opt, 10, True)) == INITIAL + [("rend_distance", "depth")]
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 10, True, d_mask=d_mask)) == INITIAL + [("d_mask", "mask")]
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 10, True, ref_weight=w)) == INITIAL + [("ref_weight", "level")]
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 10, True, base_color_loss_map=bl)) == INITIAL + [("base_color_loss_map", "depth2")]
    assert _names_modes(vz.training_cells(cam, _pkg(), opt, 10, True, ref_score=rs)) == INITIAL + [("ref_score", "unit")]
    ind = [("indirect_out.render", "unit"), ("indirect_out.specular", "unit"), ("indirect_out.rend_alpha", "unit")]
    assert _names_modes(vz.training_cells(cam, _pkg(extra=("indirect_out",)), opt, 200, False)) == FULL + ind
    everything = vz.training_cells(cam, _pkg(extra=("rend_distance", "indirect_out") + lights), opt_ind, 60, False, d_mask, w, bl, rs)
    assert _names_modes(everything) == FULL + LIGHTS + [("rend_distance", "depth"), ("d_mask", "mask"), ("ref_weight", "level"),
                                                        ("base_color_loss_map", "depth2")] + LIGHTS + ind + [("ref_score", "unit")]
    assert len(everything) == 26 <= vz.MAX_CELLS
    # the tensors are the render's own (nothing is copied or computed), and the statement's list agrees cell by cell
    pkg = _pkg(extra=("rend_distance", "indirect_out") + lights)
    mine = vz.training_cells(cam, pkg, opt_ind, 60, False, d_mask, w, bl, rs)
    theirs = ss.training_list(cam, pkg, opt_ind, 60, False, d_mask, w, bl, rs)
    assert len(mine) == len(theirs)
    for (name, (t, mode)), (t_ref, mode_ref) in zip(mine, theirs):
        assert vz.MODE_NAMES[mode] == mode_ref, name
        if mode_ref == "absdiff":
            assert torch.equal(t[0], t_ref[0]) and t[1] is t_ref[1]
        elif name == "gt":
            assert torch.equal(t, t_ref)
        else:
            assert t is t_ref, name
    assert mine[1][1][0] is pkg["render"] and mine[-1][1][0] is rs
    rot = vz.view_rotation(SimpleNamespace(R=np.arange(9.0).reshape(3, 3)))
    assert rot.dtype == np.float32 and np.array_equal(rot, np.arange(9.0).reshape(3, 3).T)
    assert np.array_equal(vz.view_rotation(SimpleNamespace(R=torch.arange(9.0).reshape(3, 3))), rot)


# ---------------------------------------------------------------- mrgs_sheet_rgb8's argument checks
def test_sheet_bad_arguments_are_refused_before_any_launch():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    BAD_ARG, WORKSPACE = 1, 5
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ws_need = L.mrgs_sheet_ws_bytes()
    assert ws_need > 0
    UNIT, ABSDIFF, NORMAL_VIEW, DEPTH, LEVEL, DEPTH2, MASK = range(7)

    def call(H=5, W=7, cells=((p, None, 3, 0, 0),), n=None, nrow=4, padding=2, Ho=9, Wo=11, ws=p, ws_bytes=ws_need, out=p, flags=0, size=None,
             sy=1.0, sx=1.0):
        table = (_lib.MrgsSheetCell * max(1, len(cells)))(*[_lib.MrgsSheetCell(*c, 0) for c in cells])
        cfg = _lib.MrgsSheetConfig(H, W, len(cells) if n is None else n, nrow, padding, Ho, Wo, sy, sx, (ctypes.c_float * 9)(), flags)
        if size is not None:
            cfg.struct_size = size
        return L.mrgs_sheet_rgb8(ctypes.byref(cfg), table, ws, ws_bytes, out, None)
    assert ctypes.sizeof(_lib.MrgsSheetConfig) == 80 and ctypes.sizeof(_lib.MrgsSheetCell) == 32
    assert call(size=76) == BAD_ARG                                                               # wrong struct_size
    assert call(H=0) == BAD_ARG and call(W=-1) == BAD_ARG and call(Ho=0) == BAD_ARG and call(Wo=0) == BAD_ARG     # non-positive sizes
    assert call(cells=()) == BAD_ARG and call(cells=((p, None, 3, 0, 0),) * 33) == BAD_ARG      # n_cells outside 1..32
    assert call(nrow=0) == BAD_ARG and call(padding=-1) == BAD_ARG and call(flags=1) == BAD_ARG
    assert call(cells=((None, None, 3, 0, 0),)) == BAD_ARG and call(cells=((p + 2, None, 3, 0, 0),)) == BAD_ARG   # NULL / misaligned data
    assert call(out=None) == BAD_ARG and call(out=p + 1) == BAD_ARG
    assert L.mrgs_sheet_rgb8(None, None, None, 0, p, None) == BAD_ARG
    assert call(cells=((p, None, 3, 7, 0),)) == BAD_ARG and call(cells=((p, None, 3, -1, 0),)) == BAD_ARG         # unknown mode
    assert call(cells=((p, None, 2, UNIT, 0),)) == BAD_ARG                                      # channels that do not fit the mode
    assert call(cells=((p, p, 1, ABSDIFF, 0),)) == BAD_ARG and call(cells=((p, None, 1, NORMAL_VIEW, 0),)) == BAD_ARG
    for mode in (DEPTH, LEVEL, DEPTH2, MASK):
        assert call(cells=((p, None, 3, mode, 0),)) == BAD_ARG
    assert call(cells=((p, None, 3, ABSDIFF, 0),)) == BAD_ARG                                   # ABSDIFF without its second image
    assert call(cells=((p, p + 2, 3, ABSDIFF, 0),)) == BAD_ARG
    assert call(cells=((p, None, 1, LEVEL, 1),)) == BAD_ARG and call(cells=((p, None, 1, MASK, 2),)) == BAD_ARG   # byte elements: MASK only
    assert call(Ho=30000, Wo=30000) == BAD_ARG                                                  # Ho Wo 3 beyond int32
    assert call(H=2 ** 30, nrow=1, cells=((p, None, 3, 0, 0),) * 2) == BAD_ARG                    # the grid's height beyond int32
    assert call(W=2 ** 29, nrow=4, cells=((p, None, 3, 0, 0),) * 4) == BAD_ARG                    # the grid's width beyond int32
    assert call(sy=0.0) == BAD_ARG and call(sx=float("nan")) == BAD_ARG and call(sx=float("inf")) == BAD_ARG
    # a statistics cell needs the workspace; a sheet without one does not look at it
    assert call(cells=((p, None, 1, DEPTH, 0),), ws=None) == BAD_ARG and call(cells=((p, None, 1, DEPTH2, 0),), ws=p + 8) == BAD_ARG
    assert call(cells=((p, None, 1, DEPTH, 0),), ws_bytes=ws_need - 1) == WORKSPACE
    assert call(cells=((p, None, 3, 0, 0), (p, None, 1, DEPTH2, 0)), ws_bytes=0) == WORKSPACE


def test_contact_sheet_refuses_what_it_cannot_run():
    from materialrefgs_amd import visualize as vz
    x = torch.zeros(3, 5, 7)
    with pytest.raises(RuntimeError, match="device tensors"):
        vz.contact_sheet([(x, "unit")])                                 # no CPU path
    with pytest.raises(ValueError, match="unknown mode"):
        vz.contact_sheet([(x, "jet")])
    with pytest.raises(ValueError, match="1..32"):
        vz.contact_sheet([(x, "unit")] * 33)
    with pytest.raises(ValueError, match="pair"):
        vz.contact_sheet([(x, "absdiff")])


# ---------------------------------------------------------------- write, then rename
def test_write_png_atomic_writes_then_renames(tmp_path, monkeypatch):
    from materialrefgs_amd import visualize as vz
    a = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = str(tmp_path / "000400.png")
    seen = {}
    real = vz.write_png

    def spy(p, arr, level=6):
        seen["name"] = p
        seen["final_exists_while_writing"] = os.path.exists(path)
        real(p, arr, level)
    monkeypatch.setattr(vz, "write_png", spy)
    vz.write_png_atomic(path, a, 1)
    assert seen["name"] != path and os.path.dirname(seen["name"]) == str(tmp_path) and not seen["final_exists_while_writing"]
    assert os.listdir(str(tmp_path)) == ["000400.png"]                  # the temporary name is gone
    assert np.array_equal(read_png(path)[2], a)
    # a second write replaces the file in one step; a failed write leaves the earlier file whole and no litter
    b = 255 - a
    vz.write_png_atomic(path, b)
    assert np.array_equal(read_png(path)[2], b)

    def failing(p, arr, level=6):
        with open(p, "wb") as f:
            f.write(b"\x89PNG half")
        raise OSError("disk full")
    monkeypatch.setattr(vz, "write_png", failing)
    with pytest.raises(OSError, match="disk full"):
        vz.write_png_atomic(path, a)
    assert os.listdir(str(tmp_path)) == ["000400.png"] and np.array_equal(read_png(path)[2], b)
