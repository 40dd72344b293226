"""render_set / render_set_train / evaluate_psnr / validation_report (materialrefgs_amd.evaluate) on a tiny scene: the synthetic surfel
model at 3000 surfels, 64 x 64, three orbit cameras whose ground truth is a perturbed render on the device."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_eval_export import read_png  # noqa: E402

H = W = 64
KEYS = ("render", "rend_normal", "surf_normal", "surf_depth", "diffuse_map", "specular_map", "base_color_map", "roughness_map", "refl_strength_map")


class View:
    """What the render functions and eval.py read of scene/cameras.py:Camera."""

    def __init__(self, cam, name):
        for k, v in cam._asdict().items():
            setattr(self, k, v)
        self.HWK = cam.HWK
        self.image_name = name
        self.original_image = None
        self.refl_mask = "set"


@pytest.fixture(scope="module")
def world(gpu_device):
    import materialrefgs_amd.renderer as renderer
    from materialrefgs_amd.lpips import LPIPS
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    pc, env, _leaves = make_surfel_model(3000, H, dev, seed=2, radius_px=5.0, env_res=64, env_min=16)
    env.build_mips()
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    opt = SimpleNamespace(indirect=False, srgb=False)
    bg = torch.zeros(3, device=dev)
    seen = []

    def render(view, gaussians, pipeline, background, **kw):
        with torch.no_grad():
            out = dict(renderer.render_surfel(view, gaussians, pipeline, background, **kw))
        out["visibility"] = out["rend_alpha"]                          # one of the three maps eval.py lists without a folder
        seen.append({k: out[k].detach().clone() for k in KEYS + ("visibility",)})
        return out
    views = []
    g = torch.Generator().manual_seed(4)
    for i in range(3):
        v = View(orbit_camera(i, H, W, n_views=8).to(dev), f"view_{i}")
        img = render(v, pc, pipe, bg, srgb=False, opt=opt)["render"]
        gt = img + 0.1 * torch.randn(3, H, W, generator=g).to(dev)     # unclamped: some values leave [0, 1]
        v.original_image = torch.cat([gt, torch.ones_like(gt[:1])]) if i == 1 else gt      # one RGBA ground truth (eval.py:47)
        views.append(v)
    seen.clear()
    return SimpleNamespace(pc=pc, pipe=pipe, opt=opt, bg=bg, views=views, render=render, seen=seen, net=LPIPS.random(0), dev=dev)


def _expected_maps(out, view):
    return [(out["render"], "unit"), (view.original_image[0:3], "unit"), (out["rend_normal"], "normal"), (out["surf_normal"], "normal"),
            (out["surf_depth"], "depth"), (out["diffuse_map"], "unit"), (out["specular_map"], "unit"), (out["base_color_map"], "unit"),
            (out["roughness_map"], "unit"), (out["refl_strength_map"], "unit"), (out["visibility"], "unit")]


@pytest.mark.gpu
def test_render_set_numbers_and_pictures(world, tmp_path, capsys):
    from materialrefgs_amd import evaluate as ev
    w = world
    w.seen.clear()
    model_path = str(tmp_path / "model")
    res = ev.render_set(model_path, w.views, w.pc, w.pipe, w.bg, True, w.opt, w.render, lpips_fn=w.net)
    assert len(w.seen) == 3 and all(v.refl_mask is None for v in w.views)
    # the per-view rows are image_metrics and the network called directly, bit for bit
    assert res["per_view"].shape == (3, 8) and res["per_view_lpips"].shape == (3,)
    for i, (out, view) in enumerate(zip(w.seen, w.views)):
        row = ev.image_metrics(out["render"], view.original_image).cpu().numpy()
        assert np.array_equal(res["per_view"][i], row)
        direct = w.net(torch.clamp(out["render"], 0, 1)[None], torch.clamp(view.original_image[0:3], 0, 1)[None])
        assert float(direct.reshape(())) == float(res["per_view_lpips"][i])
    assert np.isfinite(res["per_view"][:, :4]).all() and (res["per_view"][:, 1] < 1).all() and (res["per_view_lpips"] > 0).all()
    # metric.txt: the reference's format string over the means of those rows (eval.py:67-74)
    text = open(os.path.join(model_path, "metric.txt")).read()
    assert capsys.readouterr().out.strip().splitlines()[-1] == text
    fields = dict(f.split(":") for f in text.split(", "))
    assert list(fields) == ["psnr", "ssim", "lpips", "fps"]
    assert float(fields["psnr"]) == res["psnr"] == float(np.array([float(x) for x in res["per_view"][:, 0]]).mean())
    assert float(fields["ssim"]) == res["ssim"] == float(np.array([float(x) for x in res["per_view"][:, 1]]).mean())
    assert float(fields["lpips"]) == res["lpips"] == float(np.array([float(x) for x in res["per_view_lpips"]]).mean())
    assert float(fields["fps"]) == res["fps"] and res["fps"] > 0 and res["render_ms"].shape == (3,) and (res["render_ms"] > 0).all()
    assert abs(res["fps"] - 1000.0 / res["render_ms"].mean()) < 1e-9 * res["fps"]
    # the ten folders of eval.py:27 and `visibility`; nothing for the maps the render does not have
    base = os.path.join(model_path, "test", "renders")
    assert sorted(os.listdir(base)) == sorted(ev.DIR_NAMES + ("visibility",))
    for i, (out, view) in enumerate(zip(w.seen, w.views)):
        want = ev.to_rgb8(_expected_maps(out, view)).cpu().numpy()
        for k, d in enumerate(ev.DIR_NAMES + ("visibility",)):
            assert sorted(os.listdir(os.path.join(base, d))) == ["00000.png", "00001.png", "00002.png"]
            h, wd, got = read_png(os.path.join(base, d, f"{i:05d}.png"))
            assert (h, wd) == (H, W) and np.array_equal(got, want[k]), (i, d)
    # the training views' folders (eval.py:76-102)
    ev.render_set_train(model_path, w.views[:2], w.pc, w.pipe, w.bg, True, w.opt, w.render, 7)
    base = os.path.join(model_path, "train", "renders")
    assert sorted(os.listdir(os.path.join(base, "surf_depth"))) == ["00000.png", "00001.png"]
    assert np.array_equal(read_png(os.path.join(base, "rgb", "00001.png"))[2], ev.to_rgb8([(w.seen[4]["render"], "unit")])[0].cpu().numpy())


class _Watched:
    """The views of a render_set call; torch's synchronisation check is on from the first view to the end of the loop."""

    def __init__(self, views):
        self.views = views

    def __len__(self):
        return len(self.views)

    def __iter__(self):
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield from self.views
        finally:
            torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
def test_render_set_without_images_writes_metric_txt_only_and_never_waits_in_the_loop(world, tmp_path):
    """save_ims=False: no file but metric.txt, and everything the loop does around the render -- the metrics, the LPIPS network, the
    copies into the table -- runs with torch.cuda.set_sync_debug_mode("error") (the render itself is exempt: it is not this module's)."""
    from materialrefgs_amd import evaluate as ev
    w = world

    def render(*a, **kw):
        torch.cuda.set_sync_debug_mode("default")
        try:
            return w.render(*a, **kw)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    w.net(w.views[0].original_image[None, 0:3], w.views[0].original_image[None, 0:3])      # the weights are on the device
    model_path = str(tmp_path / "quiet")
    try:
        res = ev.render_set(model_path, _Watched(w.views), w.pc, w.pipe, w.bg, False, w.opt, render, lpips_fn=w.net)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.get_sync_debug_mode() == 0
    assert os.listdir(model_path) == ["metric.txt"] and res["per_view"].shape == (3, 8)
    # the check is live in this build: a host read in that mode raises
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=w.dev).item()
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
def test_evaluate_psnr_and_validation_report(world, tmp_path):
    from materialrefgs_amd import evaluate as ev
    import materialrefgs_amd.renderer as renderer
    w = world
    scene = SimpleNamespace(gaussians=w.pc, getTestCameras=lambda: w.views, getTrainCameras=lambda: w.views[:2])
    kwargs = dict(pipe=w.pipe, bg_color=w.bg, srgb=False, opt=w.opt)
    calls = []

    def render_func(view, gaussians, **kw):
        out = renderer.render_surfel(view, gaussians, **kw)
        calls.append((view, out["render"].detach().clone()))
        return out

    def rows_of(calls):
        return torch.stack([ev.image_metrics(img, v.original_image).cpu().double() for v, img in calls])
    out_dir = str(tmp_path / "evaluate")
    got = ev.evaluate_psnr(scene, render_func, kwargs, out_dir=out_dir)
    assert [v for v, _ in calls] == w.views
    rows = rows_of(calls)
    want = 0.0
    for r in rows:
        want += float(r[3])                                            # psnr(image, gt).mean(), train_refreal.py:1730
    assert isinstance(got, float) and got == want / 3
    assert sorted(os.listdir(out_dir)) == ["view_0.png", "view_1.png", "view_2.png"]
    assert np.array_equal(read_png(os.path.join(out_dir, "view_2.png"))[2], ev.to_rgb8([(calls[2][1], "unit")])[0].cpu().numpy())
    calls.clear()
    rep = ev.validation_report(scene, render_func, kwargs)
    assert set(rep) == {"test", "train"}
    picks = [w.views[i % 2] for i in range(5, 30, 5)]                  # train_refreal.py:1667 over two training cameras
    assert [v for v, _ in calls] == w.views + picks
    rows = rows_of(calls)
    for name, r in (("test", rows[:3]), ("train", rows[3:])):
        l1, psnr = rep[name]
        assert abs(l1 - float(r[:, 2].mean())) < 1e-15 and abs(psnr - float(r[:, 3].mean())) < 1e-12
    empty = SimpleNamespace(gaussians=w.pc, getTestCameras=lambda: [], getTrainCameras=lambda: [])
    assert ev.evaluate_psnr(empty, renderer.render_surfel, kwargs, out_dir=out_dir) == 0.0
    assert ev.validation_report(empty, renderer.render_surfel, kwargs) == {"test": None, "train": None}
