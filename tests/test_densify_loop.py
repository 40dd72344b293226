"""The loop of tests/test_closed_loop.py with the library's own densification in it: render -> loss -> backward -> Adam over four
cameras, add_densification_stats from the render's outputs on every iteration and densify_and_prune every 20 -- what a maintainer of the
reference runs after swapping the two calls.  Small (P = 5000, 128 x 128, 60 iterations): every piece has
its exact test in tests/test_densify.py; this one is about the pieces meeting -- the statistics fed by real view-space gradients select
both a clone and a split set, the row count moves, the optimizer keeps stepping on the new parameters and the per-camera caches
neither grow nor overflow when P changes."""
from types import SimpleNamespace

import pytest
import torch

from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera

pytestmark = pytest.mark.gpu

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "refl_strength", "roughness", "ori_color", "ind_dc", "ind_rest")


def test_sixty_iterations_with_native_densification(gpu_device):
    from materialrefgs_amd import densify, losses
    from materialrefgs_amd import rasterizer as rz
    from materialrefgs_amd.optim import Adam
    from materialrefgs_amd.renderer import render_surfel
    dev = gpu_device
    torch.manual_seed(0)
    P, H, W, n_cam = 5000, 128, 128, 4
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    opt_r = SimpleNamespace(indirect=False)
    cams = [orbit_camera(v, H, W, n_views=n_cam).to(dev) for v in range(n_cam)]
    pc, env, _ = make_surfel_model(P, max(H, W), dev, seed=0, radius_px=4.0, env_res=32, env_min=8)
    targets = []
    with torch.no_grad():
        env.build_mips()
        for c in cams:
            gt = render_surfel(c, pc, pipe, bg, srgb=False, opt=opt_r)["render"].clone()
            targets.append(SimpleNamespace(original_image=gt, image_weight=losses.image_weight(gt)))
        g = torch.Generator().manual_seed(3)
        pc._features_dc.add_(0.6 * torch.randn(pc._features_dc.shape, generator=g).to(dev))
        pc._ori_color.add_(1.0 * torch.randn(pc._ori_color.shape, generator=g).to(dev))
    rates = {"xyz": 1.6e-5, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3, "refl_strength": 0.01,
             "roughness": 0.01, "ori_color": 0.01, "ind_dc": 2.5e-3, "ind_rest": 1.25e-4}
    groups = [{"params": [torch.nn.Parameter(getattr(pc, densify.group_attr(n)).detach().clone().requires_grad_(True))], "lr": rates[n], "name": n}
              for n in GROUPS]
    groups.append({"params": [env.base], "lr": 0.01, "name": "env"})
    pc.optimizer = Adam(groups, lr=0.0, eps=1e-15)
    for gr in pc.optimizer.param_groups[:-1]:
        setattr(pc, densify.group_attr(gr["name"]), gr["params"][0])
    pc.percent_dense = 0.01
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = torch.zeros(P, 1, device=dev), torch.zeros(P, 1, device=dev), torch.zeros(P, device=dev)
    loss_opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.05, normal_loss_start=0, lambda_dist=100.0, dist_loss_start=100,
                               lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                               use_perceptual_loss=False)
    rz.reset_work_hints()
    rz._PAIR_GUESS.clear()
    history, counts = [], [P]
    for it in range(1, 61):
        v = it % n_cam
        env.build_mips()
        out = render_surfel(cams[v], pc, pipe, bg, srgb=False, opt=opt_r)          # (a RasterWorkspaceOverflow inside is redone inside: nothing escapes)
        loss, _tb = losses.calculate_loss(targets[v], pc, out, loss_opt, it, targets[v].image_weight, None)
        loss.backward()
        densify.add_densification_stats(pc, out["viewspace_points"], out["visibility_filter"], out["radii"])
        pc.optimizer.step()
        pc.optimizer.zero_grad(set_to_none=True)
        history.append(float(loss))
        if it % 20 == 0:
            n = pc._xyz.shape[0]
            assert float(pc.denom.max()) >= 1.0 and float(pc.max_radii2D.max()) > 0.0 and float(pc.xyz_gradient_accum.max()) > 0.0
            # thresholds from what the loop observed, so that both sets are non-empty: the median positive g and the median max(s)
            gr = (pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0).reshape(-1)
            smax = torch.exp(pc._scaling.detach()).max(dim=1).values
            max_grad = float(gr[gr > 0].median())
            extent = float(smax.median()) / pc.percent_dense
            clone = (gr >= max_grad) & (smax <= pc.percent_dense * extent)
            split = (gr >= max_grad) & (smax > pc.percent_dense * extent)
            assert int(clone.sum()) > 0 and int(split.sum()) > 0
            n_keep, n_clone, n_child = densify.densify_and_prune(pc, max_grad, 0.005, extent, 20 if it > 20 else None)
            assert 0 < n_clone <= int(clone.sum()) and 0 < n_child <= int(split.sum()) and n_keep <= n - int(split.sum())
            counts.append(pc._xyz.shape[0])
            assert counts[-1] == n_keep + n_clone + 2 * n_child and counts[-1] != counts[-2]
            for s, shape in ((pc.xyz_gradient_accum, (counts[-1], 1)), (pc.denom, (counts[-1], 1)), (pc.max_radii2D, (counts[-1],))):
                assert tuple(s.shape) == shape and float(s.abs().sum()) == 0.0
            for grp in pc.optimizer.param_groups[:-1]:
                p = grp["params"][0]
                assert getattr(pc, densify.group_attr(grp["name"])) is p and p.shape[0] == counts[-1]
                assert pc.optimizer.state[p]["exp_avg"].shape == p.shape
    print(f"densify loop: loss {history[0]:.4f} -> {history[-1]:.4f}; surfel counts {counts}; hints {len(rz._WORK_HINTS)}")
    assert all(map(lambda x: x == x and x < 1e3, history))                        # finite throughout
    assert len(rz._WORK_HINTS) == n_cam
