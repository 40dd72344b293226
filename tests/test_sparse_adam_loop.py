"""The loop of tests/test_closed_loop.py at its sizes (20 000 surfels, 256 x 256, six cameras), 60 iterations without densification, stepped
by optim.SparseAdam with each iteration's own `visibility_filter`: the loss falls, and a surfel that no camera ever sees ends with the
parameters it started with, bit for bit, and zero moments.  The dense Adam's final loss on the same seed is printed beside it (not asserted:
the two rules are meant to differ -- dense Adam keeps moving a surfel by its decaying momentum in the iterations that do not see it)."""
from types import SimpleNamespace

import pytest
import torch

from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera

pytestmark = pytest.mark.gpu

GROUPS = [("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
          ("rotation", "_rotation"), ("refl_strength", "_refl_strength"), ("roughness", "_roughness"), ("ori_color", "_ori_color"),
          ("ind_dc", "_indirect_dc"), ("ind_rest", "_indirect_rest")]
RATES = {"xyz": 1.6e-5, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3, "refl_strength": 0.01,
         "roughness": 0.01, "ori_color": 0.01, "ind_dc": 2.5e-3, "ind_rest": 1.25e-4}
HIDDEN = 0          # the row of the surfel behind every camera


def _train(dev, sparse, iterations=60):
    from materialrefgs_amd import losses
    from materialrefgs_amd.optim import Adam, SparseAdam
    from materialrefgs_amd.renderer import render_surfel
    torch.manual_seed(0)
    P, H, W, n_cam = 20000, 256, 256, 6
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    opt_r = SimpleNamespace(indirect=False)
    cams = [orbit_camera(v, H, W, n_views=n_cam).to(dev) for v in range(n_cam)]
    pc, env, _ = make_surfel_model(P, max(H, W), dev, seed=0, radius_px=6.0, env_res=32, env_min=8)
    targets = []
    with torch.no_grad():
        # the cameras sit 4.03 from the origin at 30 degrees elevation and look at it: a point 40 up the z axis has depth 4.03 - 40 sin(30 deg) < 0
        # in every one of them
        pc._xyz[HIDDEN] = torch.tensor([0.0, 0.0, 40.0], device=dev)
        env.build_mips()
        for c in cams:
            gt = render_surfel(c, pc, pipe, bg, srgb=False, opt=opt_r)["render"].clone()
            targets.append(SimpleNamespace(original_image=gt, image_weight=losses.image_weight(gt)))
        g = torch.Generator().manual_seed(3)
        pc._features_dc.add_(0.6 * torch.randn(pc._features_dc.shape, generator=g).to(dev))
        pc._ori_color.add_(1.0 * torch.randn(pc._ori_color.shape, generator=g).to(dev))
        pc._refl_strength.add_(1.0 * torch.randn(pc._refl_strength.shape, generator=g).to(dev))
        env.base.add_(0.8 * torch.randn(env.base.shape, generator=g).to(dev))
    groups = [{"params": [torch.nn.Parameter(getattr(pc, attr).detach().clone().requires_grad_(True))], "lr": RATES[name], "name": name}
              for name, attr in GROUPS]
    groups.append({"params": [env.base], "lr": 0.01, "name": "env"})
    optimizer = (SparseAdam if sparse else Adam)(groups, lr=0.0, eps=1e-15)
    params = {gr["name"]: gr["params"][0] for gr in optimizer.param_groups}
    for name, attr in GROUPS:
        setattr(pc, attr, params[name])
    start = {name: params[name].detach()[HIDDEN].clone() for name, _ in GROUPS}
    loss_opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.05, normal_loss_start=0, lambda_dist=100.0, dist_loss_start=100,
                               lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                               use_perceptual_loss=False)
    history, seen_hidden, touched = [], False, 0.0
    for it in range(1, iterations + 1):
        v = it % n_cam
        env.build_mips()
        out = render_surfel(cams[v], pc, pipe, bg, srgb=False, opt=opt_r)
        loss, _ = losses.calculate_loss(targets[v], pc, out, loss_opt, it, targets[v].image_weight, None)
        loss.backward()
        vis = out["visibility_filter"]
        if sparse:
            optimizer.step(visibility=vis)
        else:
            optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        history.append(loss.detach())
        seen_hidden = seen_hidden | vis[HIDDEN]
        touched = touched + vis.float().mean()
    history = [float(x) for x in torch.stack(history).cpu()]
    return SimpleNamespace(history=history, optimizer=optimizer, params=params, start=start, seen_hidden=bool(seen_hidden),
                           touched=float(touched) / iterations)


def test_sixty_iterations_with_sparse_adam(gpu_device):
    r = _train(gpu_device, sparse=True)
    d = _train(gpu_device, sparse=False)
    first, last = sum(r.history[:6]) / 6, sum(r.history[-6:]) / 6          # one round of the six cameras each
    d_last = sum(d.history[-6:]) / 6
    print(f"sparse-Adam loop: loss {first:.4f} -> {last:.4f} over 60 iterations (a view touches {100 * r.touched:.2f} % of the rows); "
          f"dense Adam on the same seed ends at {d_last:.4f}")
    assert all(x == x and x < 1e3 for x in r.history)
    assert last < first, (first, last)
    assert not r.seen_hidden
    for name, _ in GROUPS:
        p = r.params[name]
        st = r.optimizer.state[p]
        assert int(st["step"]) == 60, name
        assert torch.equal(p.detach()[HIDDEN], r.start[name]), name
        assert not bool(st["exp_avg"][HIDDEN].any()) and not bool(st["exp_avg_sq"][HIDDEN].any()), name
        if name in ("xyz", "f_dc", "opacity"):
            assert bool(st["exp_avg_sq"].any()), name                       # (the step did reach the other rows)
