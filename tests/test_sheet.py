"""The training contact sheet on the GPU (csrc/mrgs_sheet.hip behind materialrefgs_amd.visualize) against tests/sheet_statement.py.

unit, absdiff, depth, level and mask cells, every border, every empty place and every resampled index equal the fp32 statement exactly.
normal_view bytes and depth2 levels equal it or differ by one, and only where the float64 statement's value before the truncation lies within
2.5e-4 of an integer (sheet_statement.accepts; tests/test_sheet_host.py asserts that the fp32 statement itself keeps that rule).

Not pinned here: that a sheet without a depth / depth2 cell is ONE launch is read off the code (the statistics launch stands behind
`if (a.n_stat)`); what is tested is that such a sheet runs without a workspace."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_statement as es  # noqa: E402
import sheet_statement as ss  # noqa: E402
from test_eval_export import _edge_values, _fill, read_png  # noqa: E402

SHAPES = ((5, 7), (37, 53))       # no plane is 16-byte aligned, output rows have odd byte counts
MODES = ("unit", "absdiff", "normal_view", "depth", "level", "depth2", "mask")


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q.astype(np.float32)


def _to_dev(cells, dev):
    return [(tuple(x.to(dev) for x in t) if isinstance(t, tuple) else t.to(dev), mode) for t, mode in cells]


def _check(cells, dev, rot=None, hw=None, **kw):
    """contact_sheet of `cells` (CPU tensors, uploaded here) against the statement under the accuracy rule; returns the bytes."""
    from materialrefgs_amd import visualize as vz
    got = vz.contact_sheet(_to_dev(cells, dev), rot=rot, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().numpy()
    want, minus, plus, kind = ss.candidates(cells, rot=rot, hw=hw, **kw)
    H, W = hw or ss.cell_shape(cells)
    for c in cells:                                                     # on these inputs the fp32 statement keeps the rule against float64
        if c[1] in ("normal_view", "depth2"):
            w32 = ss.depth2_levels(ss._map2d(c[0], H, W)) if c[1] == "depth2" else es.unit_bytes(ss.cell_image(c, rot, H, W).numpy())
            d = w32.astype(np.int64) - ss.bytes64(c, rot, H, W).astype(np.int64)
            assert np.abs(d).max() <= 1 and ss._near(ss.pre_values64(c, rot, H, W))[d != 0].all()
    assert got.shape == want.shape
    ok, n_diff = ss.accepts(got, want, minus, plus, kind)
    print(f"{len(cells)} cells {kw}: {n_diff} of {got.size} bytes differ from the fp32 statement, "
          f"{int(((minus != want) | (plus != want)).sum())} may")
    assert ok
    return got


def _mode_cell(mode, H, W, seed, finite=False, nan=False, inf=False):
    """One cell of `mode` filled with the edge values (finite=True: those of magnitude <= 2 only, for the modes whose statistics an infinity
    turns into NaN); nan / inf: the middle pixel is NaN / two pixels are +inf and -inf."""
    vals = _edge_values()
    if finite:
        vals = vals[np.abs(vals) <= 2.0]                                # (and nothing that squeezes the others into two levels)
    if mode == "unit":
        t = _fill((3 if seed % 2 else 1, H, W), vals, seed)
    elif mode == "absdiff":
        t = (_fill((3, H, W), vals, seed), _fill((3, H, W), np.concatenate([vals[np.isfinite(vals)], -vals[np.isfinite(vals)]]), seed + 100))
    elif mode == "normal_view":
        t = _fill((3, H, W), vals * 2 - 1, seed)
    else:
        t = _fill((1, H, W), vals, seed)
    if nan:
        first = t[0] if isinstance(t, tuple) else t
        first[0, H // 2, W // 2] = float("nan")
    if inf:
        first = t[0] if isinstance(t, tuple) else t
        first[0, 0, 0], first[0, H - 1, W - 1] = float("inf"), float("-inf")
    return (t, mode)


# ---------------------------------------------------------------- one cell, every mode
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_each_mode_alone(mode, shape, gpu_device):
    """One-cell sheets (make_grid returns the image: no border) on the edge values -- every k / 255 and (k +- 0.5) / 255 with their fp32
    neighbours, negatives, values above 1, +-inf -- and one NaN case per mode.  depth and depth2 take the finite values in the main case
    (an infinity makes the whole map level 0, which is the second case)."""
    H, W = shape
    rot = _rotation(7)
    table = es.jet_table()
    stats = mode in ("depth", "depth2")
    for seed in (1, 2):
        got = _check([_mode_cell(mode, H, W, seed, finite=stats)], gpu_device, rot=rot, height=None)
        assert got.shape == (H, W, 3)
        if stats:
            assert len(np.unique(got.reshape(-1, 3), axis=0)) > 4               # not a flat picture
    if stats:                                                           # (x - min) / (max - min) with an infinite bound is NaN or 0: level 0
        got = _check([_mode_cell(mode, H, W, 3, finite=True, inf=True)], gpu_device, rot=rot, height=None)
        assert (got == table[0]).all()
    got = _check([_mode_cell(mode, H, W, 4, finite=stats, nan=True)], gpu_device, rot=rot, height=None)
    at = got[H // 2, W // 2]
    if mode == "normal_view":                                           # a NaN channel makes all three of rot @ x NaN
        assert (at == 0).all()
    elif mode in ("unit", "absdiff"):                                   # the NaN sits in channel 0
        assert at[0] == 0
    else:
        assert tuple(at) == tuple(table[0])
    if stats:
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 4           # the NaN is skipped by the statistics, not spread by them


@pytest.mark.gpu
def test_every_edge_value_in_one_cell(gpu_device):
    """A shape with room for all edge values in every plane (48 x 50), the output rows split over several workgroups when resampled."""
    H, W = 48, 50
    vals = _edge_values()
    assert H * W >= len(vals)
    rot = _rotation(11)
    cells = [_mode_cell(m, H, W, 5, finite=m in ("depth", "depth2")) for m in MODES]
    assert np.isin(vals, cells[4][0].numpy()).all() and np.isin(vals, cells[6][0].numpy()).all()
    _check(cells, gpu_device, rot=rot, nrow=4, padding=2, height=None)
    _check(cells[:3], gpu_device, rot=rot, nrow=3, padding=1, height=1100)      # 1100 x 3367: four workgroups per row, the last one partial


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_depth2_clip_and_constant_map(shape, gpu_device):
    from materialrefgs_amd import visualize as vz
    H, W = shape
    g = torch.Generator().manual_seed(H)
    table = es.jet_table()
    inside = torch.rand(1, H, W, generator=g)                           # uniform: max < 6 std, nothing is clipped from above
    assert float(inside.max()) < 6 * float(inside.std(unbiased=False))
    spike = inside.clone()
    # far above 6 std: clipped.  (Among 35 values one outlier raises the std with it: 6 std stays just below an outlier of any size.)
    spike[0, 1, 2] = 50.0 if H * W > 1000 else 1000.0
    spike[0, 2, 1] = -3.0                                               # below 0: clipped to 0
    assert float(spike.max()) > 6 * float(spike.std(unbiased=False))
    const = torch.full((1, H, W), 3.25)                                 # std 0: clipped to [0, 0], 0 / 1e-20: level 0 throughout
    big_mean = torch.full((1, H, W), 4096.0) + torch.rand(1, H, W, generator=g) * 2 ** -6      # a mean far above the std: all clipped to 6 std
    for m in (inside, spike, const, big_mean, -inside):
        got = _check([(m, "depth2")], gpu_device, height=None)
        vis = vz.visualize_depth2(m.to(gpu_device))
        assert torch.equal(vis, torch.from_numpy(got).to(gpu_device).permute(2, 0, 1).float() / 255.0)
    assert float(ss._nanstd(const[0].numpy())) == 0.0
    assert (_check([(const, "depth2")], gpu_device, height=None) == table[0]).all()
    assert (_check([(-inside, "depth2")], gpu_device, height=None) == table[0]).all()
    levels = ss.depth2_levels(spike[0].numpy())
    assert levels[1, 2] == 255 and levels[2, 1] == 0 and len(np.unique(levels)) > (10 if H * W > 1000 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_element_types_and_shapes(shape, gpu_device):
    from materialrefgs_amd import visualize as vz
    H, W = shape
    g = torch.Generator().manual_seed(W)
    table = es.jet_table()
    b = torch.rand(H * W, generator=g) > 0.4
    u = torch.randint(0, 256, (H * W,), generator=g, dtype=torch.uint8)             # bytes above 1 clamp to level 255
    u[:3] = torch.tensor([0, 1, 2], dtype=torch.uint8)
    f = _fill((H * W,), _edge_values(), 9)
    for m in (b, u, f):
        got2 = _check([(m.reshape(H, W), "mask")], gpu_device, height=None)
        # a flat [H W] mask needs H and W from somewhere: the helper takes them, as the reference's does ...
        vis = vz.visualize_d_mask(m.to(gpu_device), H, W)
        assert torch.equal(vis, torch.from_numpy(got2).to(gpu_device).permute(2, 0, 1).float() / 255.0)
        # ... and in a sheet a flat mask stands behind a cell that has them
        x = torch.rand(3, H, W, generator=g)
        both = _check([(x, "unit"), (m, "mask")], gpu_device, nrow=2, padding=1, height=None)
        assert np.array_equal(both[1:1 + H, 2 + W:2 + 2 * W], got2)
    want_b = table[np.where(b.reshape(H, W).numpy(), 255, 0)]
    assert np.array_equal(_check([(b.reshape(H, W), "mask")], gpu_device, height=None), want_b)


# ---------------------------------------------------------------- grids
def _mixed_cells(n, H, W, seed):
    """n cells that cycle through the modes with inputs a render would give (and a few values outside [0, 1])."""
    g = torch.Generator().manual_seed(seed)
    cells = []
    for k in range(n):
        mode = MODES[(k + seed) % len(MODES)]
        if mode == "unit":
            t = torch.rand(3 if k % 2 else 1, H, W, generator=g) * 1.2 - 0.1
        elif mode == "absdiff":
            t = (torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g))
        elif mode == "normal_view":
            v = torch.randn(3, H, W, generator=g)
            t = v / v.norm(dim=0, keepdim=True)
        elif mode == "depth":
            t = torch.rand(1, H, W, generator=g) * 5 + 1
        elif mode == "level":
            t = torch.rand(1, H, W, generator=g) * 1.1
        elif mode == "depth2":
            t = torch.rand(1, H, W, generator=g) ** 6
        else:
            t = torch.rand(H * W, generator=g) > 0.5 if k else (torch.rand(H, W, generator=g) > 0.5)
        cells.append((t, mode))
    return cells


GRIDS = [(n, (37, 53), 4, 2, 301) for n in (1, 2, 4, 5, 7, 13, 19, 32)] + \
        [(n, (37, 53), 1, 10, None) for n in (1, 2, 4, 5, 7, 13, 19, 32)] + \
        [(7, (5, 7), 4, 2, 2400),            # the one test at the reference's height: 16 x 38 -> 2400 x 5700
         (19, (37, 53), 4, 2, 120),          # down: 197 x 222 -> 120 x 135
         (5, (37, 53), 4, 2, "equal"),       # a resample to the grid's own size is the identity
         (13, (37, 53), 4, 2, None),
         (4, (37, 53), 1, 10, 301),
         (7, (37, 53), 4, 2, 37)]            # far down: rows and columns of the grid are skipped


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRIDS, ids=lambda c: f"n{c[0]}-{c[1][0]}x{c[1][1]}-nrow{c[2]}-pad{c[3]}-h{c[4]}")
def test_grids_of_mixed_cells(case, gpu_device):
    from materialrefgs_amd import visualize as vz
    n, (H, W), nrow, padding, height = case
    Hg, Wg = ss.layout(n, H, W, nrow, padding, None)[:2]
    if height == "equal":
        height = Hg
    rot = _rotation(n)
    cells = _mixed_cells(n, H, W, n)
    got = _check(cells, gpu_device, rot=rot, nrow=nrow, padding=padding, height=height)
    assert got.shape[:2] == vz.sheet_layout(n, H, W, nrow, padding, height)[2:]
    if case[4] == "equal":
        assert got.shape[:2] == (Hg, Wg)
        assert np.array_equal(got, _check(cells, gpu_device, rot=rot, nrow=nrow, padding=padding, height=None))
    # every border byte and the empty places of the last row are 0: the cover of the cells, laid out and resampled by the statement
    cover = ss.sheet([(torch.ones(1, H, W), "unit")] * n, nrow=nrow, padding=padding, height=height)
    assert set(np.unique(cover)) <= {0, 255}
    assert (got[cover[..., 0] == 0] == 0).all()
    if n > 1:
        assert (cover == 0).any() and (got[0] == 0).all() and (got[:, 0] == 0).all()


@pytest.mark.gpu
def test_sheet_without_statistics_runs_without_a_workspace(gpu_device):
    from materialrefgs_amd import _lib
    H, W = 37, 53
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g)
    xd, yd = x.to(gpu_device), y.to(gpu_device)
    Hg, Wg, Ho, Wo = ss.layout(2, H, W, 4, 2, 90)
    out = torch.full((Ho, Wo, 3), 7, dtype=torch.uint8, device=gpu_device)
    table = (_lib.MrgsSheetCell * 2)(_lib.MrgsSheetCell(xd.data_ptr(), None, 3, _lib.MRGS_SHEET_UNIT, 0, 0),
                                     _lib.MrgsSheetCell(yd.data_ptr(), None, 1, _lib.MRGS_SHEET_LEVEL, 0, 0))
    cfg = _lib.MrgsSheetConfig(H, W, 2, 4, 2, Ho, Wo, float(np.float32(Hg) / np.float32(Ho)), float(np.float32(Wg) / np.float32(Wo)),
                               (ctypes.c_float * 9)(), 0)
    rc = _lib.lib().mrgs_sheet_rgb8(ctypes.byref(cfg), table, None, 0, out.data_ptr(), _lib.stream_ptr(gpu_device))
    assert rc == 0
    assert np.array_equal(out.cpu().numpy(), ss.sheet([(x, "unit"), (y, "level")], nrow=4, padding=2, height=90))


# ---------------------------------------------------------------- the helpers
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_helpers_against_their_statements(shape, gpu_device):
    from materialrefgs_amd import evaluate as ev
    from materialrefgs_amd import visualize as vz
    H, W = shape
    g = torch.Generator().manual_seed(H + W)
    table = torch.from_numpy(es.jet_table())
    d = torch.rand(1, H, W, generator=g) * 3 + 0.5
    # `/ 255.` on the device, where the reference divides too (image_utils.py:68, :78, :91: .float().cuda() ... / 255.)
    as_float = lambda levels: table[torch.from_numpy(levels.astype(np.int64))].to(gpu_device).permute(2, 0, 1).float() / 255.0
    for t in (d, d[0]):                                                 # [1,H,W] and [H,W], as the scripts pass them
        vis = vz.visualize_depth(t.to(gpu_device))
        assert vis.shape == (3, H, W) and vis.dtype == torch.float32 and vis.is_cuda
        assert torch.equal(vis, as_float(es.depth_levels(d[0].numpy())))
        assert torch.equal(vis, ev.visualize_depth(t.to(gpu_device)))
    w = torch.rand(1, H, W, generator=g) * 1.3 - 0.1
    want = as_float(ss.level_levels(w[0].numpy()))
    assert torch.equal(vz.visualize_depth(w.to(gpu_device), norm=False), want)
    assert torch.equal(ev.visualize_depth(w.to(gpu_device), norm=False), want)
    m = torch.rand(H * W, generator=g) > 0.3
    assert torch.equal(vz.visualize_d_mask(m.to(gpu_device), H, W), as_float(ss.mask_levels(m, H, W)))
    b = torch.rand(H, W, generator=g) ** 5
    b[H // 2, W // 2] = 9.0
    got = (vz.visualize_depth2(b.to(gpu_device)).cpu() * 255.0).round().to(torch.uint8).permute(1, 2, 0).numpy()
    ok, _ = ss.accepts(got, *[c.transpose(1, 2, 0) for c in ss.cell_candidates((b, "depth2"), None, H, W)[:3]], np.full((H, W), ss.ROWWISE))
    assert ok


# ---------------------------------------------------------------- save_training_vis
H, W = 37, 53


class View:
    def __init__(self, cam):
        for k, v in cam._asdict().items():
            setattr(self, k, v)
        self.HWK = cam.HWK
        self.original_image = None


@pytest.fixture(scope="module")
def world(gpu_device):
    import materialrefgs_amd.renderer as renderer
    from materialrefgs_amd.model import get_env_direction1, get_env_direction2
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    pc, env, _leaves = make_surfel_model(1500, max(H, W), dev, seed=2, radius_px=4.0, env_res=64, env_min=16)
    env.build_mips()
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    opt = SimpleNamespace(indirect=False, srgb=False, volume_render_until_iter=0, init_until_iter=100)
    bg = torch.zeros(3, device=dev)
    calls = []

    def render_fn(view, gaussians, pipeline, background, **kw):
        calls.append(kw)
        return dict(renderer.render_surfel(view, gaussians, pipeline, background, **kw))
    with torch.no_grad():
        d1, d2 = get_env_direction1(8, 16, dev), get_env_direction2(8, 16, dev)
        pc.render_env_map = lambda: {"env1": env(d1, mode="pure_env"), "env2": env(d2, mode="pure_env")}
        pc.render_env_map_2 = lambda: {"env1": env(d1, mode="pure_env") * 0.25, "env2": env(d2, mode="pure_env") * 0.25}
    view = View(orbit_camera(1, H, W, n_views=8).to(dev))
    with torch.no_grad():
        pkg = render_fn(view, pc, pipe, bg, srgb=False, opt=opt)
    calls.clear()
    g = torch.Generator().manual_seed(6)
    view.original_image = (pkg["render"] + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).detach()
    extras = dict(d_mask=(torch.rand(H * W, generator=g) > 0.5).to(dev), ref_weight=torch.zeros(1, H, W),         # the zero weight arrives on the CPU
                  base_color_loss_map=(torch.rand(H, W, generator=g) ** 4).to(dev), ref_score=torch.rand(1, H, W, generator=g).to(dev))
    return SimpleNamespace(pc=pc, pipe=pipe, opt=opt, bg=bg, view=view, render_fn=render_fn, calls=calls, pkg=pkg, extras=extras, dev=dev)


def _cpu(x):
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    return x.detach().cpu() if torch.is_tensor(x) else x


def _statement_sheet_ok(w, got, iteration, initial_stage, extras, height):
    from materialrefgs_amd import visualize as vz
    cam = SimpleNamespace(original_image=w.view.original_image.cpu())
    lst = ss.training_list(cam, _cpu(w.pkg), w.opt, iteration, initial_stage, _cpu(extras.get("d_mask")), _cpu(extras.get("ref_weight")),
                           _cpu(extras.get("base_color_loss_map")), _cpu(extras.get("ref_score")))
    lst = [((t.reshape(1, H, W) if mode in ("depth", "level", "depth2") else t), mode) for t, mode in lst]
    ok, n_diff = ss.accepts(got, *ss.candidates(lst, nrow=4, padding=2, height=height, rot=vz.view_rotation(w.view), hw=(H, W)))
    print(f"save_training_vis, {len(lst)} cells: {n_diff} bytes differ from the fp32 statement")
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("initial_stage", (True, False), ids=("initial", "surfel"))
def test_save_training_vis_end_to_end(initial_stage, world, tmp_path):
    from materialrefgs_amd import visualize as vz
    w = world
    folder, height, iteration = str(tmp_path / "vis"), 150, 400
    extras = {} if initial_stage else w.extras
    args = (w.view, w.pc, w.bg, w.render_fn, w.pipe, w.opt, iteration, initial_stage, extras.get("d_mask"), extras.get("ref_weight"),
            extras.get("base_color_loss_map"))
    w.calls.clear()
    paths = vz.save_training_vis(*args, w.pkg, extras.get("ref_score"), visualize_path=folder, height=height)
    assert w.calls == []                                                # a render_pkg was given: nothing is rendered
    names = ["000400.png"] if initial_stage else ["000400.png", "000400_env.png"]
    assert sorted(os.listdir(folder)) == sorted(names) and [os.path.basename(p) for p in paths] == names
    cells = [c for _, c in vz.training_cells(w.view, w.pkg, w.opt, iteration, initial_stage, **extras)]
    assert len(cells) == (7 if initial_stage else 12 + len(extras))
    direct = vz.contact_sheet(cells, nrow=4, padding=2, height=height, rot=vz.view_rotation(w.view)).cpu().numpy()
    hh, ww, got = read_png(os.path.join(folder, "000400.png"))
    assert (hh, ww) == vz.sheet_layout(len(cells), H, W, 4, 2, height)[2:] and np.array_equal(got, direct)
    assert _statement_sheet_ok(w, got, iteration, initial_stage, extras, height)
    if not initial_stage:
        env = w.pc.render_env_map()                                     # volume_render_until_iter <= init_until_iter: render_env_map, :1610-1613
        panes = lambda e: [(e[k].detach().permute(2, 0, 1).cpu(), "unit") for k in ("env1", "env2")]
        want = ss.sheet(panes(env), nrow=1, padding=10, height=None)
        hh, ww, got = read_png(os.path.join(folder, "000400_env.png"))
        assert (hh, ww) == (2 * 18 + 10, 16 + 20) and np.array_equal(got, want)
        # the other environment map under :1610's condition
        opt2 = SimpleNamespace(indirect=False, srgb=False, volume_render_until_iter=1000, init_until_iter=100)
        vz.save_training_vis(w.view, w.pc, w.bg, w.render_fn, w.pipe, opt2, 500, False, None, None, None, w.pkg, visualize_path=folder, height=height)
        env2 = w.pc.render_env_map_2()
        want2 = ss.sheet(panes(env2), nrow=1, padding=10, height=None)
        assert np.array_equal(read_png(os.path.join(folder, "000500_env.png"))[2], want2) and not np.array_equal(want2, want)
    # render_pkg=None: the call renders, with the reference's keywords, and gives the same picture
    again = str(tmp_path / "again")
    vz.save_training_vis(*args, None, extras.get("ref_score"), visualize_path=again, height=height)
    assert len(w.calls) == 1 and w.calls[0]["srgb"] is w.opt.srgb and w.calls[0]["opt"] is w.opt
    assert np.array_equal(read_png(os.path.join(again, "000400.png"))[2], got if initial_stage else direct)


@pytest.mark.gpu
def test_training_visualizer_two_saves_then_close(world, tmp_path):
    from materialrefgs_amd import visualize as vz
    w = world
    folder, height = str(tmp_path / "vis"), 150
    vis = vz.TrainingVisualizer(folder, workers=1, png_level=1)
    e = w.extras
    vis.save(w.view, w.pc, w.bg, w.render_fn, w.pipe, w.opt, 1, True, None, None, None, w.pkg, height=height)
    vis.save(w.view, w.pc, w.bg, w.render_fn, w.pipe, w.opt, 400, False, e["d_mask"], e["ref_weight"], e["base_color_loss_map"], w.pkg,
             e["ref_score"], height=height)
    vis.close()
    vis.close()                                                         # closing twice is harmless
    assert sorted(os.listdir(folder)) == ["000001.png", "000400.png", "000400_env.png"]      # no temporary name is left
    sync = str(tmp_path / "sync")
    vz.save_training_vis(w.view, w.pc, w.bg, w.render_fn, w.pipe, w.opt, 1, True, None, None, None, w.pkg, visualize_path=sync, height=height)
    vz.save_training_vis(w.view, w.pc, w.bg, w.render_fn, w.pipe, w.opt, 400, False, e["d_mask"], e["ref_weight"], e["base_color_loss_map"], w.pkg,
                         e["ref_score"], visualize_path=sync, height=height)
    for name in ("000001.png", "000400.png", "000400_env.png"):
        a, b = read_png(os.path.join(folder, name)), read_png(os.path.join(sync, name))
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2]), name
