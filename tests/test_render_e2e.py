"""End-to-end parity of `renderer.render_surfel` (gaussian_renderer/__init__.py:225-483) against the composition of the stage
checkers (oracle/render_oracle.py): every dictionary entry and every parameter gradient, incl. the environment cubemap, with and
without opt.indirect.  The per-stage parity tests cannot see a mis-wired channel, a transposed map or a dropped gradient edge
between stages; this one can."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from materialrefgs_amd.synthetic import make_shell_scene, orbit_camera, sphere_mesh

MAP_KEYS = ("render", "refl_strength_map", "diffuse_map", "diffuse_map_ori", "specular_map", "base_color_map", "roughness_map",
            "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal")
PARAMS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest", "_refl_strength", "_roughness", "_ori_color",
          "_indirect_dc", "_indirect_rest")


def _models(P, H, W, seed, dev=None, env_res=32, env_min=8):   # 32 -> 16 -> 8: the smallest chain the reference's prefilter handles (envfilter_oracle header)
    from materialrefgs_amd.renderer import SurfelModel
    sc = make_shell_scene(P, S=0, seed=seed, radius_px=6.0, image_size=max(H, W))
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    inv_sig = lambda x: torch.log(x / (1 - x))
    raw = dict(xyz=sc.means3D.clone(), scaling=torch.log(sc.scales), rotation=sc.rotations.clone() * 1.3,   # un-normalised on purpose
               opacity=inv_sig(sc.opacities.clamp(1e-4, 1 - 1e-4)), features_dc=sc.shs[:, :1].clone(), features_rest=sc.shs[:, 1:].clone(),
               refl_strength=rnd(P, 1), roughness=rnd(P, 1), ori_color=rnd(P, 3), indirect_dc=rnd(P, 1, 3).abs() * 0.5,
               indirect_rest=rnd(P, 15, 3) * 0.02)
    env_base = rnd(6, env_res, env_res, 3)
    mk = lambda conv: SurfelModel(*[conv(raw[k]) for k in ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")],
                                  **{k: conv(raw[k]) for k in ("refl_strength", "roughness", "ori_color", "indirect_dc", "indirect_rest")})
    pc_o = mk(lambda t: t.double().requires_grad_(True))
    base_o = env_base.double().requires_grad_(True)
    if dev is None:
        return pc_o, base_o, None, None
    from materialrefgs_amd.shading import EnvLight
    pc_h = mk(lambda t: t.to(dev).requires_grad_(True))
    env = EnvLight(device=dev, min_res=env_min, max_res=env_res, trainable=True)
    with torch.no_grad():
        env.base.copy_(env_base)
    pc_h.env_map = env
    return pc_o, base_o, pc_h, env


def _loss(out, H, W, indirect, dev):
    """A loss that reads every map the training loss reads (utils/loss_utils.py:147-166) plus the material maps, with fixed weights."""
    g = torch.Generator().manual_seed(99)
    terms = []
    for k in MAP_KEYS + (("indirect_color", "direct_light") if indirect else ()):
        w = torch.rand(out[k].shape, generator=g).to(out[k].dtype).to(dev)
        terms.append((out[k] * w).sum() * (0.01 if k == "surf_depth" else 1.0))
    return sum(terms)


def test_render_surfel_oracle_runs_and_differentiates_on_cpu():
    """CPU sanity of the checker itself: keys, shapes, finite gradients on every leaf; colour-chain gradient vs a finite difference."""
    from oracle import render_oracle
    P, H, W = 300, 48, 64
    pc, base, _, _ = _models(P, H, W, seed=2)
    cam = orbit_camera(1, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    out = render_oracle.render_surfel_oracle(cam, pc, base, 8, pipe, bg, srgb=True)
    for k in MAP_KEYS:
        assert torch.isfinite(out[k]).all(), k
    loss = _loss(out, H, W, False, "cpu")
    loss.backward()
    for n in PARAMS:
        assert getattr(pc, n).grad is not None and torch.isfinite(getattr(pc, n).grad).all(), n
    assert base.grad is not None and float(base.grad.abs().sum()) > 0
    assert out["viewspace_points"].grad is not None
    # finite difference on one albedo logit (smooth path: sigmoid -> feature blend -> shading)
    i = int(torch.argmax(pc._ori_color.grad.abs().sum(1)))
    eps = 1e-3
    vals = []
    for s in (+1, -1):
        with torch.no_grad():
            pc._ori_color[i, 0] += s * eps
        o = render_oracle.render_surfel_oracle(cam, pc, base, 8, pipe, bg, srgb=True)
        vals.append(float(_loss(o, H, W, False, "cpu")))
        with torch.no_grad():
            pc._ori_color[i, 0] -= s * eps
    fd = (vals[0] - vals[1]) / (2 * eps)
    assert abs(fd - float(pc._ori_color.grad[i, 0])) < 2e-3 * max(1.0, abs(fd)), (fd, float(pc._ori_color.grad[i, 0]))


def test_leaf_gradient_helper_equals_the_plain_end_to_end_checker_on_cpu():
    """oracle/render_oracle.surfel_leaf_gradients (the full-size form: rasterizer inputs handed in, the gradient arriving there pulled back
    through the float64 glue, the levels' gradient through build_mips_backward) gives, when handed the float64 glue's own outputs, exactly
    the gradients of the plain composition render_surfel_oracle(pc, base); and the glue's truth leg (its pull-back in the reference's fp32
    torch ops) stays within fp32 distance of it."""
    from oracle import glue_oracle, render_oracle
    P, H, W = 300, 48, 64
    pc, base, _, _ = _models(P, H, W, seed=2)
    cam = orbit_camera(1, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    keys = ["render", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal"]
    out = render_oracle.render_surfel_oracle(cam, pc, base, 8, pipe, bg)
    g = torch.Generator().manual_seed(1)
    ups = [torch.rand(out[k].shape, generator=g).double() for k in keys]
    torch.autograd.backward([out[k] for k in keys], ups)
    with torch.no_grad():
        inter = glue_oracle.surfel_features_reference(pc, cam.camera_center.double())
    _, grads, info = render_oracle.surfel_leaf_gradients(cam, [getattr(pc, n).detach() for n in PARAMS], base.detach(), inter, keys, ups, pipe, bg, env_min_res=8)
    for n in render_oracle.LEAF_NAMES:
        a = getattr(pc, "_" + n).grad.numpy()
        assert np.abs(a - grads[n]).max() <= 1e-12 * max(np.abs(a).max(), 1e-30), n
    assert np.abs(base.grad.numpy() - grads["env_base"]).max() <= 1e-12 * np.abs(base.grad.numpy()).max()
    assert np.abs(out["viewspace_points"].grad.numpy() - grads["viewspace_points"]).max() == 0.0
    assert info["raster_shading_seconds"] > 0 and len(info["levels"]) == 3
    for n, lit in grads["lit32"].items():
        scale = max(np.abs(grads[n]).max(), 1e-30)
        assert np.abs(lit - grads[n]).max() <= 1e-3 * scale, n          # fp32 pull-back of a float64 upstream gradient
    hip = {n: grads[n] for n in render_oracle.LEAF_NAMES}
    rows, ok = render_oracle.leaf_gradient_report(hip, grads, render_oracle.LEAF_NAMES)
    assert ok and all(r_["err"] == 0.0 for r_ in rows.values())
    hip["rotation"] = grads["rotation"] * (1 + 3e-4)                     # a loose kernel is not excused by the truth leg
    assert not render_oracle.leaf_gradient_report(hip, grads, render_oracle.LEAF_NAMES)[1]


def _capturing_visibility(stash, real):
    """RayTracer.visibility, with the arguments of its last call kept as numpy arrays in stash["visibility_args"]."""
    def visibility(self, HWK, R, T, normal_map, render_alpha, surf_depth):
        stash["visibility_args"] = (HWK, *(a.detach().float().cpu().numpy().copy() for a in (R, T, normal_map, render_alpha, surf_depth)))
        return real(self, HWK, R, T, normal_map, render_alpha, surf_depth)
    return visibility


def _visibility_statement(mesh, args):
    """tests/visibility_statement.py on the maps a render handed to RayTracer.visibility: [H,W] float32 tensor."""
    import visibility_statement as vs
    (H, W, K), R, T, normal, alpha, surf_depth = args
    assert normal.shape == (H, W, 3) and alpha.shape[:2] == (H, W) and surf_depth.shape[-2:] == (H, W)
    return torch.from_numpy(vs.visibility(mesh[0], mesh[1], H, W, vs.kinv_f32(K), R, T, normal, alpha, surf_depth))


@pytest.mark.gpu
@pytest.mark.parametrize("indirect,srgb", [(False, False), (False, True), (True, False)])
def test_render_surfel_matches_the_composed_oracle(gpu_device, indirect, srgb):
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.renderer import render_surfel
    from oracle import render_oracle
    P, H, W = 3000, 96, 128
    pc_o, base_o, pc_h, env = _models(P, H, W, seed=1, dev=gpu_device)
    cam = orbit_camera(1, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    mesh = None
    if indirect:
        v1, t1 = sphere_mesh(24, 36, 0.9)
        v2, t2 = sphere_mesh(12, 16, 0.8)
        v2 = v2 + np.array([0.0, 2.2, 0.0], dtype=np.float32)
        mesh = (np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)]))
        pc_h.ray_tracer = RayTracer(*mesh)
    env.build_mips()
    # The rasterizer's per-gaussian inputs as the product's glue kernel produced them (fp32) are captured and handed to the checker's
    # rasterizer: a float64 evaluation of the activations differs in the last bit, which moves the rotation gradient of a 3 000-surfel
    # scene by 1e-4 of its range through the rasterizer's ill-conditioned terms -- a comparison of inputs, not of renderers (round 5
    # measured 1.1e-4 and set the bar to 3e-4 for it).  The gradient that arrives at those inputs is then pulled back through the
    # checker's float64 glue at the raw leaves (what render_oracle.surfel_leaf_gradients does at full size); the glue's own values are
    # compared in tests/test_shading.py and tests/test_reference_render.py.
    import materialrefgs_amd.renderer as renderer_mod
    from oracle import glue_oracle
    stash, glue = {}, renderer_mod.surfel_features

    def capturing(pc_, campos_, **kw):
        o = glue(pc_, campos_, **kw)
        stash["o"] = [t_.detach().cpu().double().requires_grad_(True) for t_ in o[:4]]
        return o
    renderer_mod.surfel_features = capturing
    real_visibility = RayTracer.visibility
    RayTracer.visibility = _capturing_visibility(stash, real_visibility)
    try:
        out_h = render_surfel(cam.to(gpu_device), pc_h, pipe, bg.to(gpu_device), srgb=srgb, opt=SimpleNamespace(indirect=indirect))
    finally:
        renderer_mod.surfel_features = glue
        RayTracer.visibility = real_visibility
    vis_bits = out_h["visibility"].detach().cpu()[0] if indirect else None     # compared with the oracle's own trace below
    inter_o = stash["o"]
    glue_f64 = glue_oracle.surfel_features_reference(pc_o, cam.camera_center.double())
    for a_, b_ in zip(inter_o, glue_f64):                # the captured inputs ARE the glue's values, to fp32 rounding
        assert float((a_ - b_).abs().max()) <= 2e-6 * max(1.0, float(b_.abs().max()))
    out_o = render_oracle.render_surfel_oracle(cam, pc_o, base_o, 8, pipe, bg, srgb=srgb, indirect=indirect, mesh=mesh, visibility_bits=vis_bits,
                                               raster_inputs=tuple(inter_o))
    assert set(out_o) - {"visibility_traced"} <= set(out_h), set(out_o) - set(out_h)
    assert ("specular_weight" in out_h) == indirect            # extra_dict is merged only under opt.indirect (__init__.py:472-473)
    assert torch.equal(out_h["radii"].cpu(), out_o["radii"]) and torch.equal(out_h["visibility_filter"].cpu(), out_o["visibility_filter"])
    ok = torch.ones(H, W, dtype=torch.bool)
    if indirect:
        vh, vo = out_h["visibility"].cpu()[0], out_o["visibility_traced"][0].float()
        ok = vh == vo
        assert float((~ok).float().mean()) < 2e-3           # ray set-up rounding at silhouettes only (the checker composes its rays in float64)
        assert torch.equal(vh, _visibility_statement(mesh, stash["visibility_args"]))      # the kernel's own operations on its own inputs: exact
        assert 0.02 < float((vo == 0).float().mean()) < 0.98
    keys = MAP_KEYS + (("indirect_color", "direct_light", "indirect_light") if indirect else ())
    for k in keys:
        a, b = out_h[k].detach().cpu().double(), out_o[k].detach()
        scale = max(float(b.abs().max()), 1e-6)
        tol = 2e-4 if k in ("surf_normal",) else 5e-5       # surf_normal: normalised cross product of depth differences
        d = (a - b).abs()
        if k == "rend_dist":                                # O(1e-5) values from O(1) terms: absolute bar (test_gpu_parity.DIST_ABS_TOL)
            scale, tol = 1.0, 5e-6
        bad = float((d > tol * scale).float().mean())
        assert bad < (2e-3 if k == "surf_normal" else 1e-4), (k, float(d.max()), scale, bad)
    if indirect:
        w_h = out_h["specular_weight"].detach().cpu().double()
        assert float((w_h - out_o["specular_weight"].detach()).abs().max()) < 5e-5
    # ---- gradients of one scalar that reads every map
    _loss(out_h, H, W, indirect, gpu_device).backward()
    _loss(out_o, H, W, indirect, "cpu").backward()
    torch.autograd.backward(list(glue_f64), [t_.grad for t_ in inter_o])      # ... on through the float64 glue to the raw leaves
    # bar: max-norm per tensor, relative to the tensor's largest gradient, <= 1e-4 (north_star) -- or the truth-leg rule of
    # tests/test_gpu_parity.py:97-116 applied to the glue (render_oracle.leaf_gradient_report): the kernels may be no further from the
    # float64 pull-back than the reference's own fp32 torch ops are (x 1.5).
    names = [n[1:] for n in PARAMS]
    hip = {n: getattr(pc_h, "_" + n).grad.detach().cpu().numpy() for n in names}
    total = {n: getattr(pc_o, "_" + n).grad.numpy() for n in names}
    hip["env.base"], total["env.base"] = env.base.grad.detach().cpu().numpy(), base_o.grad.numpy()
    hip["viewspace_points"], total["viewspace_points"] = out_h["viewspace_points"].grad.detach().cpu().numpy(), out_o["viewspace_points"].grad.numpy()
    total["lit32"] = render_oracle.glue_lit32_leg([getattr(pc_o, n) for n in PARAMS], cam.camera_center, [t_.grad for t_ in inter_o], total)
    rows, ok = render_oracle.leaf_gradient_report(hip, total, names + ["env.base", "viewspace_points"], bar=1e-4)
    print("\n".join(f"{n:18s} max-norm err {r_['err']:.2e}  {r_['rule']}" + (f" (fp32 torch glue {r_['lit32_err']:.2e})" if "lit32_err" in r_ else "")
                    for n, r_ in rows.items()))
    assert ok, rows


PGSR_SCENE = dict(P=3000, H=96, W=128, seed=1, view=1)      # conditioning: test_pgsr_scene_is_well_conditioned_for_the_unbiased_depth
PGSR_CASES = [("a", True, False), ("b", False, False), ("c", True, True)]       # case, _FUSE_GLUE, opt.indirect (c: the epilogue does not apply)


def _pgsr_loss(out, H, W, indirect, dev):
    """_loss plus a fixed-weight sum over the flavour's blended plane distance."""
    g = torch.Generator().manual_seed(17)
    w = torch.rand(out["rend_distance"].shape, generator=g).to(out["rend_distance"].dtype).to(dev)
    return _loss(out, H, W, indirect, dev) + (out["rend_distance"] * w).sum()


def test_pgsr_scene_is_well_conditioned_for_the_unbiased_depth():
    """The "pgsr" flavour's surf_depth is the blended plane distance divided by -(blended normal . pixel ray): a few grazing pixels can
    dominate the max-norm of a gradient, and then fp32 arithmetic anywhere in front of them -- the reference's own included -- cannot hold
    1e-4.  The scene of test_render_surfel_pgsr_matches_the_composed_oracle is measured here on the CPU: the reference's torch ops behind
    the rasterizer (glue_oracle.pgsr_allmap8, compute_2dgs_normal_and_regularizations_reference) on the checker's all-map, under the
    geometry terms of that test's loss, in float32 against float64: max-norm relative error of d loss / d all-map and of d loss / d blended
    distance over the covered pixels (an uncovered pixel is 0 x inf = NaN in the torch ops; the rasterizer's backward never reads its upstream
    gradient there).  Bound: a quarter of the gradient bar of 1e-4."""
    from oracle import glue_oracle as go, render_oracle
    P, H, W = PGSR_SCENE["P"], PGSR_SCENE["H"], PGSR_SCENE["W"]
    pc, _base, _, _ = _models(P, H, W, seed=PGSR_SCENE["seed"])
    cam = orbit_camera(PGSR_SCENE["view"], H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    with torch.no_grad():
        op, sc, rot, feat = go.surfel_features_reference(pc, cam.camera_center.double())
        feat = torch.cat((feat, go.get_distance(pc, cam)), -1)
        _color, f, allmap, _radii = render_oracle._OracleRaster.apply(pc.get_xyz, torch.zeros_like(pc._xyz), op, pc.get_features, feat, sc, rot, cam,
                                                                      pc.active_sh_degree, "fused")
    covered = allmap[1] > 0
    assert 0.2 < float(covered.double().mean()) < 1.0
    res = {}
    for dt in (torch.float64, torch.float32):
        am, rd = allmap.detach().clone().to(dt).requires_grad_(True), f[-1:].detach().clone().to(dt).requires_grad_(True)
        camd = cam._replace(world_view_transform=cam.world_view_transform.to(dt), full_proj_transform=cam.full_proj_transform.to(dt))
        reg = go.compute_2dgs_normal_and_regularizations_reference(go.pgsr_allmap8(am, rd, camd), camd, pipe)
        out = {k: torch.zeros(n, H, W, dtype=dt) for k, n in zip(MAP_KEYS, (3, 1, 3, 3, 3, 3, 1))}          # the maps the shading makes: no part here
        out.update({"rend_alpha": reg["render_alpha"], "rend_normal": reg["render_normal"], "rend_dist": reg["render_dist"],
                    "surf_depth": reg["surf_depth"], "surf_normal": reg["surf_normal"], "rend_distance": rd})
        _pgsr_loss(out, H, W, False, "cpu").backward()
        res[dt] = (am.grad.double()[:, covered], rd.grad.double()[:, covered])
    for name, a, b in zip(("all-map", "blended distance"), res[torch.float64], res[torch.float32]):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        e = float((a - b).abs().max() / a.abs().max())
        print(f"d loss / d {name}: the reference's ops in float32 are {e:.2e} from float64 (max-norm, covered pixels)")
        assert e <= 2.5e-5, (name, e)


@pytest.mark.gpu
@pytest.mark.parametrize("case,fused,indirect", PGSR_CASES)
def test_render_surfel_pgsr_matches_the_composed_oracle(gpu_device, case, fused, indirect, monkeypatch):
    """render_surfel(flag="pgsr") -- the flavour the reference ships -- against the composed checker, every map and every leaf gradient, as
    test_render_surfel_matches_the_composed_oracle does for "2dgs".  The plane distance |n_cam . c_cam| is differentiated by hand in two
    places: the glue epilogue of the rasterizer's per-gaussian backward (case a) and the glue's own backward kernel (case b; case c under
    opt.indirect, where the mirror direction and the plane distance both send a gradient to the facing normal and the <8, true, 9> blend
    instances run with live indirect channels).  The captured rows are twelve floats: columns 0..7 go to the checker's rasterizer as they
    are, column 8 is compared with glue_oracle.get_distance in float64 -- which is what the checker rasterizes, and whose gradient reaches
    the raw leaves by itself --, 9..11 are zero."""
    import materialrefgs_amd.renderer as renderer_mod
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.renderer import render_surfel
    from oracle import glue_oracle, render_oracle
    P, H, W = PGSR_SCENE["P"], PGSR_SCENE["H"], PGSR_SCENE["W"]
    pc_o, base_o, pc_h, env = _models(P, H, W, seed=PGSR_SCENE["seed"], dev=gpu_device)
    cam = orbit_camera(PGSR_SCENE["view"], H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    mesh = None
    if indirect:
        v1, t1 = sphere_mesh(24, 36, 0.9)
        v2, t2 = sphere_mesh(12, 16, 0.8)
        v2 = v2 + np.array([0.0, 2.2, 0.0], dtype=np.float32)
        mesh = (np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)]))
        pc_h.ray_tracer = RayTracer(*mesh)
    env.build_mips()
    monkeypatch.setattr(renderer_mod, "_FUSE_GLUE", fused)
    stash, glue = {}, renderer_mod.surfel_features

    def capturing(pc_, campos_, **kw):
        o = glue(pc_, campos_, **kw)
        stash["o"] = [t_.detach().cpu().double() for t_ in o[:4]]
        return o
    renderer_mod.surfel_features = capturing
    monkeypatch.setattr(RayTracer, "visibility", _capturing_visibility(stash, RayTracer.visibility))
    try:
        out_h = render_surfel(cam.to(gpu_device), pc_h, pipe, bg.to(gpu_device), srgb=False, opt=SimpleNamespace(indirect=indirect), flag="pgsr")
    finally:
        renderer_mod.surfel_features = glue
    vis_bits = out_h["visibility"].detach().cpu()[0] if indirect else None
    rows = stash["o"][3]
    assert rows.shape == (P, 12)
    inter_o = [t_.clone().requires_grad_(True) for t_ in stash["o"][:3] + [rows[:, :8]]]
    glue_f64 = glue_oracle.surfel_features_reference(pc_o, cam.camera_center.double())
    for a_, b_ in zip(inter_o, glue_f64):                # the captured inputs ARE the glue's values, to fp32 rounding
        assert float((a_ - b_).abs().max()) <= 2e-6 * max(1.0, float(b_.abs().max()))
    dist_o = glue_oracle.get_distance(pc_o, cam)
    dist_o.retain_grad()
    assert float((rows[:, 8:9] - dist_o.detach()).abs().max()) <= 2e-6 * float(dist_o.abs().max())
    assert float(rows[:, 9:].abs().max()) == 0.0
    out_o = render_oracle.render_surfel_oracle(cam, pc_o, base_o, 8, pipe, bg, srgb=False, indirect=indirect, mesh=mesh, visibility_bits=vis_bits,
                                               raster_inputs=tuple(inter_o), flag="pgsr", distance=dist_o)
    assert set(out_o) - {"visibility_traced"} <= set(out_h), set(out_o) - set(out_h)
    assert "rend_distance" in out_o and ("specular_weight" in out_h) == indirect
    assert torch.equal(out_h["radii"].cpu(), out_o["radii"]) and torch.equal(out_h["visibility_filter"].cpu(), out_o["visibility_filter"])
    if indirect:
        vh, vo = out_h["visibility"].cpu()[0], out_o["visibility_traced"][0].float()
        assert float((vh != vo).float().mean()) < 2e-3           # ray set-up rounding at silhouettes only (float64-composed rays)
        assert torch.equal(vh, _visibility_statement(mesh, stash["visibility_args"]))      # the kernel's own operations on its own inputs: exact
        print(f"case {case}: occluded share {float((vo == 0).float().mean()):.4f}")
        assert 0.02 < float((vo == 0).float().mean()) < 0.98
    keys = MAP_KEYS + ("rend_distance",) + (("indirect_color", "direct_light", "indirect_light") if indirect else ())
    for k in keys:                                          # (surf_depth: the flavour's unbiased depth)
        a, b = out_h[k].detach().cpu().double(), out_o[k].detach()
        scale = max(float(b.abs().max()), 1e-6)
        tol = 2e-4 if k in ("surf_normal",) else 5e-5       # surf_normal: normalised cross product of depth differences
        d = (a - b).abs()
        if k == "rend_dist":                                # O(1e-5) values from O(1) terms: absolute bar (test_gpu_parity.DIST_ABS_TOL)
            scale, tol = 1.0, 5e-6
        if k == "rend_distance":                            # 5e-5 of its range
            scale = float(b.max() - b.min())
        bad = float((d > tol * scale).float().mean())
        assert bad < (2e-3 if k == "surf_normal" else 1e-4), (k, float(d.max()), scale, bad)
    if indirect:
        w_h = out_h["specular_weight"].detach().cpu().double()
        assert float((w_h - out_o["specular_weight"].detach()).abs().max()) < 5e-5
    # ---- gradients of one scalar that reads every map, the blended plane distance included
    _pgsr_loss(out_h, H, W, indirect, gpu_device).backward()
    _pgsr_loss(out_o, H, W, indirect, "cpu").backward()
    g_inter = [t_.grad for t_ in inter_o]
    torch.autograd.backward(list(glue_f64), g_inter)      # ... on through the float64 glue to the raw leaves (the distance column went there by itself)
    names = [n[1:] for n in PARAMS]
    hip = {n: getattr(pc_h, "_" + n).grad.detach().cpu().numpy() for n in names}
    total = {n: getattr(pc_o, "_" + n).grad.numpy() for n in names}
    hip["env.base"], total["env.base"] = env.base.grad.detach().cpu().numpy(), base_o.grad.numpy()
    hip["viewspace_points"], total["viewspace_points"] = out_h["viewspace_points"].grad.detach().cpu().numpy(), out_o["viewspace_points"].grad.numpy()
    # the truth leg covers the plane distance: both of its pull-backs include get_distance under the gradient that arrived at the column
    total["lit32"] = render_oracle.glue_lit32_leg([getattr(pc_o, n) for n in PARAMS], cam.camera_center, g_inter, total, distance=(cam, dist_o.grad))
    rows_, ok = render_oracle.leaf_gradient_report(hip, total, names + ["env.base", "viewspace_points"], bar=1e-4)
    print(f"case {case}:\n" + "\n".join(f"{n:18s} max-norm err {r_['err']:.2e}  max|g| {float(np.abs(total[n]).max()):.3e}  {r_['rule']}" +
                                       (f" (fp32 torch glue {r_['lit32_err']:.2e})" if "lit32_err" in r_ else "") for n, r_ in rows_.items()))
    assert ok, rows_
    assert float(np.abs(dist_o.grad.numpy()).max()) > 0.0
    if indirect:
        assert float(np.abs(total["indirect_dc"]).max()) > 0.0 and float(np.abs(total["indirect_rest"]).max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("extra_reader,flag", [(False, "2dgs"), (True, "2dgs"), (False, "pgsr"), (True, "pgsr")])
def test_glue_epilogue_equals_the_two_kernel_backward(gpu_device, extra_reader, flag, monkeypatch):
    """render_surfel without opt.indirect: the rasterizer's per-gaussian backward carries on through the glue's backward in the same
    kernel (MrgsRasterGrads::glue_params: the activations' derivatives applied to the gradient row's results in registers; the
    surfel_features backward kernel is not launched) against the two-kernel path (MRGS_NO_GLUE_EPILOGUE=1).  Same forward: bit-identical
    maps.  Gradients: the epilogue is the same arithmetic compiled without FMA contraction (the rasterizer's flags), and the blend backward's
    float atomics order their sums differently in any two runs (two runs of the SAME path differ by up to 2e-6 of a tensor's largest element
    on such scenes: tools/stress_glue.py): every leaf within 1e-5 of its largest element; the indirect coefficients take exact zeros both ways.  extra_reader: a second consumer of the glue node's
    outputs (a loss on the activated opacity and the material rows) -- its share goes through the glue's own kernel and is ADDED to the
    epilogue's.  flag "pgsr" (the flavour the reference ships): rows of nine channels in twelve floats; the plane distance's gradient
    reaches the raw rotation and the centre inside the epilogue."""
    import materialrefgs_amd.renderer as renderer_mod
    from materialrefgs_amd.renderer import render_surfel
    P, H, W = 3000, 96, 128
    cam = orbit_camera(1, H, W).to(gpu_device)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(renderer_mod, "_FUSE_GLUE", fused)
        _pc_o, _base_o, pc_h, env = _models(P, H, W, seed=4, dev=gpu_device)
        env.build_mips()
        stash, glue = {}, renderer_mod.surfel_features

        def capturing(pc_, campos_, **kw):
            o = glue(pc_, campos_, **kw)
            stash["o"] = o
            return o
        renderer_mod.surfel_features = capturing
        try:
            out = render_surfel(cam, pc_h, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag=flag)
        finally:
            renderer_mod.surfel_features = glue
        loss = _loss(out, H, W, False, gpu_device)
        if flag != "2dgs":
            g = torch.Generator().manual_seed(17)
            loss = loss + (out["rend_distance"] * torch.rand(out["rend_distance"].shape, generator=g).to(gpu_device)).sum()
        if extra_reader:
            g = torch.Generator().manual_seed(3)
            C = stash["o"][3].shape[1]
            loss = loss + (stash["o"][0] * torch.rand(P, 1, generator=g).to(gpu_device)).sum() + (stash["o"][3] * torch.rand(P, C, generator=g).to(gpu_device)).sum()
        loss.backward()
        grads = {n: getattr(pc_h, n).grad.detach().clone() for n in PARAMS}
        grads["env.base"] = env.base.grad.detach().clone()
        grads["viewspace_points"] = out["viewspace_points"].grad.detach().clone()
        res[fused] = ({k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}, grads)
    (maps1, g1), (maps0, g0) = res[True], res[False]
    for k in maps0:
        assert torch.equal(maps0[k], maps1[k]), k
    for n in g0:
        assert bool(torch.isfinite(g1[n]).all()), n
        assert float((g0[n] - g1[n]).abs().max()) <= 1e-5 * max(1e-30, float(g0[n].abs().max())), (n, float((g0[n] - g1[n]).abs().max()), float(g0[n].abs().max()))
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_refl_strength", "_roughness", "_ori_color"):
        assert float(g1[n].abs().max()) > 0.0, n
    if not extra_reader:          # (the extra reader looks at the indirect rows too)
        for n in ("_indirect_dc", "_indirect_rest"):
            assert float(g0[n].abs().max()) == 0.0 and float(g1[n].abs().max()) == 0.0


@pytest.mark.gpu
def test_glue_epilogue_launches_no_glue_backward_kernel(gpu_device, monkeypatch):
    """With the epilogue the glue node's backward hands on what the rasterizer left for it: mrgs_surfel_features_backward is not called
    (counted at the ctypes boundary); without it, once."""
    import materialrefgs_amd.renderer as renderer_mod
    from materialrefgs_amd.renderer import render_surfel
    P, H, W = 2000, 64, 80
    cam = orbit_camera(2, H, W).to(gpu_device)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.zeros(3, device=gpu_device)
    L = renderer_mod._lib.lib()
    real = L.mrgs_surfel_features_backward
    for fused, want in ((True, 0), (False, 1)):
        monkeypatch.setattr(renderer_mod, "_FUSE_GLUE", fused)
        _pc_o, _base_o, pc_h, env = _models(P, H, W, seed=6, dev=gpu_device)
        env.build_mips()
        out = render_surfel(cam, pc_h, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=False))
        calls = []

        class Counting:
            def __getattr__(self, name):
                if name == "mrgs_surfel_features_backward":
                    return lambda *a: (calls.append(1), real(*a))[1]
                return getattr(L, name)
        orig_lib = renderer_mod._lib.lib
        renderer_mod._lib.lib = lambda: Counting()
        try:
            _loss(out, H, W, False, gpu_device).backward()
        finally:
            renderer_mod._lib.lib = orig_lib
        assert len(calls) == want, (fused, len(calls))
        assert pc_h._opacity.grad is not None and float(pc_h._opacity.grad.abs().max()) > 0.0
        # (opt.indirect: the blended indirect radiance is read -- never the epilogue)
    monkeypatch.setattr(renderer_mod, "_FUSE_GLUE", True)
    _pc_o, _base_o, pc_h, env = _models(P, H, W, seed=6, dev=gpu_device)
    env.build_mips()
    out = render_surfel(cam, pc_h, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=True))
    (out["render"].sum() + out["indirect_light"].sum()).backward()
    assert float(pc_h._indirect_dc.grad.abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("grad_mode", [True, False])
def test_build_mips_rebuilds_after_a_texel_write_and_skips_without_one(gpu_device, grad_mode):
    """A long-lived EnvLight that goes through build_mips() every iteration, with an in-place write of the texels between them (what the
    optimizer step does), against an EnvLight constructed afresh from a copy of the same texels in each iteration: images and levels
    bit-equal, gradients equal to rounding.  build_mips() runs under the grad mode of the render, so without gradients its "nothing to
    rebuild" stamp is on the path: it must never serve levels of texels that have since been written, and a second call with nothing
    written in between must leave the very same tensors in place.  Also: a look-up with NO forward since build_mips (env(dirs) alone)
    must see the texels the 'optimizer' just wrote."""
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.shading import EnvLight
    dev = gpu_device
    P, H, W = 20000, 256, 256
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    cam = orbit_camera(1, H, W).to(dev)
    results = {}
    for fresh in (False, True):
        _, _, pc_h, env = _models(P, H, W, seed=4, dev=dev, env_res=128, env_min=16)
        texels = env.base.detach().clone()
        rows = []
        g = torch.Generator().manual_seed(7)
        for it in range(4):
            step = 0.05 * torch.randn(env.base.shape, generator=g).to(dev)
            if fresh:
                texels.add_(step)
                env = pc_h.env_map = EnvLight(device=dev, min_res=16, max_res=128, trainable=True)
                with torch.no_grad():
                    env.base.copy_(texels)
            else:
                with torch.no_grad():
                    env.base.add_(step)                                                     # the optimizer step
            for t_ in pc_h.parameters() + [env.base]:
                t_.grad = None
            with torch.set_grad_enabled(grad_mode):
                env.build_mips()
                if not grad_mode:
                    built = list(env.specular)
                    env.build_mips()                                                        # nothing written since: nothing rebuilt
                    assert len(env.specular) == len(built) and all(a is b for a, b in zip(env.specular, built)), it
            if it == 2:
                # no rasterizer forward between build_mips and the first look at the levels
                d = torch.nn.functional.normalize(torch.randn(4096, 3, generator=g), dim=1).to(dev)
                with torch.set_grad_enabled(grad_mode):
                    look = env(d, roughness=torch.rand(4096, 1, generator=g).to(dev))
                rows.append(("fwd", look.detach().clone()))
            with torch.set_grad_enabled(grad_mode):
                out = render_surfel(cam, pc_h, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=False))
            rows += [("fwd", t_.detach().clone()) for t_ in [out["render"], out["specular_map"]] + list(env.specular)]
            if grad_mode:
                (out["render"].sum() + out["specular_map"].sum() * 0.5).backward()
                rows += [("grad", env.base.grad.clone()), ("grad", pc_h._roughness.grad.clone())]
        torch.cuda.synchronize(dev)
        results[fresh] = rows
    assert len(results[False]) == len(results[True])
    for i, ((kind, a), (_, b)) in enumerate(zip(results[False], results[True])):
        assert torch.isfinite(a).all()
        if kind == "fwd":
            assert torch.equal(a, b), i
        else:       # (texel and per-gaussian gradients are accumulated with float atomics: equal to rounding, not to the bit)
            assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-12), i


@pytest.mark.gpu
def test_a_second_backward_over_the_same_render_gets_clean_texel_gradients(gpu_device):
    """The texel-gradient buffers of render_surfel's shading backward are allocated and cleared by the FORWARD of the render (the backward
    is one launch that accumulates into them) and are good for one backward: a second backward over the retained graph must not add to
    what the first one left there."""
    from materialrefgs_amd.renderer import render_surfel
    dev = gpu_device
    P, H, W = 5000, 128, 160
    _, _, pc_h, env = _models(P, H, W, seed=6, dev=dev)
    env.build_mips()
    out = render_surfel(orbit_camera(1, H, W).to(dev), pc_h, SimpleNamespace(depth_ratio=0.0, debug=False), torch.zeros(3, device=dev), srgb=False,
                        opt=SimpleNamespace(indirect=False))
    loss = out["render"].sum() + 0.5 * out["specular_map"].sum()
    grads = []
    for _ in range(3):
        env.base.grad = None
        loss.backward(retain_graph=True)
        grads.append(env.base.grad.clone())
    assert float(grads[0].abs().max()) > 0
    for g in grads[1:]:
        assert float((g - grads[0]).abs().max()) <= 1e-5 * float(grads[0].abs().max())      # (float atomics: equal to rounding)


# ---------------------------------------------------------------------------------------------------------------- render_volume
VOL_KEYS = ("render", "refl_strength_map", "diffuse_map", "specular_map", "base_color_map", "roughness_map", "rend_alpha", "rend_normal",
            "rend_dist", "surf_depth", "surf_normal")


def test_render_volume_oracle_keeps_the_fg0_indexing_of_the_reference():
    """CPU: the checker reproduces appendix B-27 -- every gaussian is weighted with the split-sum table value of gaussian 0 -- so
    moving gaussian 0's roughness changes the specular colour of ALL gaussians, moving another one's changes only its own lookups."""
    from oracle import render_oracle
    P, H, W = 200, 32, 48
    pc, base, _, _ = _models(P, H, W, seed=3)
    cam = orbit_camera(2, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.zeros(3)
    out = render_oracle.render_volume_oracle(cam, pc, base, 8, pipe, bg)
    for k in VOL_KEYS:
        assert torch.isfinite(out[k]).all(), k
    (out["specular_map"].sum() + out["render"].sum()).backward()
    g_rough = pc._roughness.grad.abs().reshape(-1)
    assert float(g_rough[0]) > 5 * float(g_rough[1:].median())      # gaussian 0 carries everyone's table lookup
    assert base.grad is not None and float(base.grad.abs().sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("indirect,srgb,flag", [(False, False, "2dgs"), (False, True, "2dgs"), (True, False, "2dgs"), (False, False, "pgsr")])
def test_render_volume_matches_the_composed_oracle(gpu_device, indirect, srgb, flag):
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.renderer import render_volume
    from oracle import render_oracle
    P, H, W = 3000, 96, 128
    pc_o, base_o, pc_h, env = _models(P, H, W, seed=2, dev=gpu_device)
    cam = orbit_camera(1, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, use_asg=False, compute_cov3D_python=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    mesh = None
    if indirect:
        v1, t1 = sphere_mesh(24, 36, 0.9)
        v2, t2 = sphere_mesh(12, 16, 0.8)
        v2 = v2 + np.array([0.0, 2.2, 0.0], dtype=np.float32)
        mesh = (np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)]))
        pc_h.ray_tracer = RayTracer(*mesh)
    env.build_mips()
    out_h = render_volume(cam.to(gpu_device), pc_h, pipe, bg.to(gpu_device), srgb=srgb, opt=SimpleNamespace(indirect=indirect), flag=flag)
    # visibility per gaussian: take the product's bits into the checker after comparing them with the checker's own trace
    vis_bits = None
    if indirect:
        probe = render_oracle.render_volume_oracle(cam, pc_o, base_o.detach(), 8, pipe, bg, indirect=True, mesh=mesh, flag=flag)
        traced = probe["visibility_traced"].reshape(-1)
        # the product's per-gaussian visibility is not returned as such; recover it from a second call of its shading function
        from materialrefgs_amd.shading import get_full_color_volume_indirect
        with torch.no_grad():
            camd = cam.to(gpu_device)
            dirn = torch.nn.functional.normalize(pc_h.get_xyz - camd.camera_center, dim=1)
            _, _, ex = get_full_color_volume_indirect(env, pc_h.get_xyz, pc_h.get_ori_color, cam.HWK, camd.R, camd.T, pc_h.get_normal(1.0, dirn).contiguous(),
                                                      pc_h.get_opacity, refl_strength=pc_h.get_refl, roughness=pc_h.get_rough, pc=pc_h,
                                                      indirect_light=torch.zeros(P, 3, device=gpu_device))
        vis_bits = ex["visibility"].reshape(-1).cpu()
        assert float((vis_bits.double() != traced).double().mean()) < 5e-3
        assert 0.02 < float((traced == 0).double().mean()) < 0.98
    out_o = render_oracle.render_volume_oracle(cam, pc_o, base_o, 8, pipe, bg, srgb=srgb, indirect=indirect, mesh=mesh, visibility_bits=vis_bits, flag=flag)
    assert torch.equal(out_h["radii"].cpu(), out_o["radii"])
    keys = VOL_KEYS + (("visibility", "indirect_light", "direct_light") if indirect else ())
    for k in keys:
        a, b = out_h[k].detach().cpu().double(), out_o[k].detach()
        scale, tol = max(float(b.abs().max()), 1e-6), (2e-4 if k == "surf_normal" else 5e-5)
        if k == "rend_dist":
            scale, tol = 1.0, 5e-6
        bad = float(((a - b).abs() > tol * scale).float().mean())
        assert bad < (2e-3 if k == "surf_normal" else 1e-4), (k, float((a - b).abs().max()), scale, bad)
    g = torch.Generator().manual_seed(5)
    def loss(out, dev):
        tot = 0
        for k in keys:
            w = torch.rand(out[k].shape, generator=g).to(out[k].dtype).to(dev)
            tot = tot + (out[k] * w).sum() * (0.01 if k == "surf_depth" else 1.0)
        return tot
    loss(out_h, gpu_device).backward()
    g = torch.Generator().manual_seed(5)
    loss(out_o, "cpu").backward()
    rows = []
    for n, gh, go_ in [(n, getattr(pc_h, n).grad, getattr(pc_o, n).grad) for n in PARAMS if getattr(pc_o, n).grad is not None] + \
                      [("env.base", env.base.grad, base_o.grad), ("viewspace_points", out_h["viewspace_points"].grad, out_o["viewspace_points"].grad)]:
        assert gh is not None, n
        a, b = gh.detach().cpu().double(), go_
        rows.append((n, float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30), float(b.abs().max())))
    print("\n".join(f"{n:18s} max-norm err {m:.2e}  max|g| {gm:.3e}" for n, m, gm in rows))
    for n, m, gm in rows:
        assert m <= 3e-4, (n, m)


@pytest.mark.gpu
def test_pgsr_flag_adds_the_plane_distance_channel(gpu_device):
    """arguments/config.py:1 ships FLAG = "pgsr": every render function rasterizes get_distance (gaussian_renderer/__init__.py:30-40) as
    its last feature channel and returns it as "rend_distance" (:215-218, 411-413, 478-480, 744-746), and takes surf_depth from the
    flavour's unbiased depth.  The other maps do not change, and the channel equals a separate rasterization of that one quantity."""
    from materialrefgs_amd import renderer
    from materialrefgs_amd.rasterizer import GaussianRasterizer
    dev = gpu_device
    P, H, W = 1200, 40, 56
    _, _, pc, _env = _models(P, H, W, seed=5, dev=dev)
    pc.env_map_2 = pc.env_map
    cam = orbit_camera(2, H, W).to(dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    d = renderer.get_distance(1.0, pc.get_xyz, cam, pc)
    assert d.shape == (P, 1) and float(d.min()) >= 0
    rast = GaussianRasterizer(raster_settings=renderer._raster_settings(cam, pc, pipe, bg, 1.0))
    _, _, alone, _, allmap = rast(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), shs=pc.get_features, opacities=pc.get_opacity,
                                  scales=pc.get_scaling, rotations=pc.get_rotation, features=d)
    # the flavour's unbiased depth, stated here from its definition: blended distance / -(blended view-space normal . pixel ray)
    import math
    fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
    rx = (torch.arange(W, device=dev) - (W - 1) / 2) / fx
    ry = (torch.arange(H, device=dev) - (H - 1) / 2) / fy
    unbiased = torch.nan_to_num(alone / -(allmap[2] * rx[None, :] + allmap[3] * ry[:, None] + allmap[4])[None], 0, 0)
    assert float(unbiased.max()) > 1.0
    for fn, kw in ((renderer.render_initial, {}), (renderer.render_surfel, {"opt": SimpleNamespace(indirect=False)}),
                   (renderer.render_volume, {"opt": SimpleNamespace(indirect=False)})):
        a = fn(cam, pc, pipe, bg, srgb=False, **kw)
        b = fn(cam, pc, pipe, bg, srgb=False, flag="pgsr", **kw)
        assert "rend_distance" not in a and b["rend_distance"].shape == (1, H, W), fn.__name__
        assert float((b["rend_distance"] - alone).abs().max()) < 2e-5 * max(1.0, float(alone.abs().max())), fn.__name__
        for k in ("render", "rend_alpha", "rend_normal"):
            assert float((a[k] - b[k]).abs().max()) < 2e-6, (fn.__name__, k)
        # surf_depth of the flavour = nan_to_num of its eighth all-map channel (gaussian_renderer/__init__.py:64-69), not the 2dgs mix
        assert float((b["surf_depth"] - unbiased).abs().max()) < 2e-5 * float(unbiased.abs().max()), fn.__name__
        assert float((a["surf_depth"] - b["surf_depth"]).abs().max()) > 1e-3


@pytest.mark.gpu
def test_deferred_pair_count_and_its_overflow(gpu_device):
    """The render functions only BEGIN the rasterizer (mrgs_rasterize_forward_begin) and collect the pair count after the whole view has been
    queued (rasterizer.deferred_raster_count).  A view whose count outgrows the workspace guessed from the previous view is rendered again:
    same maps bit for bit, same gradients, the count reported and the guess refreshed."""
    from types import SimpleNamespace
    from materialrefgs_amd import rasterizer as rz
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    P, H, W = 20_000, 200, 200
    pc, env, leaves = make_surfel_model(P, H, dev, radius_px=3.0)
    cam = orbit_camera(1, H, W).to(dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    bg = torch.zeros(3, device=dev)
    key = (dev.index, P, H, W)

    def render():
        for t in leaves:
            t.grad = None
        env.build_mips()
        out = render_surfel(cam, pc, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=False))
        out["render"].sum().backward()
        return out["render"].detach().clone(), [t.grad.clone() for t in leaves], rz.LAST_NUM_RENDERED, out

    rz._PAIR_GUESS.pop(key, None)
    img0, g0, R0, _ = render()                        # no guess yet: two-phase path, count read in the middle
    assert R0 > 0 and rz._PAIR_GUESS[key] >= R0
    img1, g1, R1, out1 = render()                     # deferred: begun inside render_surfel, finished at its end
    assert R1 == R0 and torch.equal(img0, img1)
    assert out1["render"].grad_fn is not None
    rz._PAIR_GUESS[key] = max(R0 // 3, 1)             # a guess that cannot hold the view
    img2, g2, R2, _ = render()
    assert R2 == R0 and torch.equal(img0, img2) and rz._PAIR_GUESS[key] >= R0
    for a, b, c in zip(g0, g1, g2):
        scale = float(a.abs().max()) + 1e-30
        assert float((a - b).abs().max()) <= 1e-4 * scale and float((a - c).abs().max()) <= 1e-4 * scale      # (atomics: summation order)
    # the context by hand: nothing waits inside, finish() reports the overflow
    rz._PAIR_GUESS[key] = max(R0 // 3, 1)
    from materialrefgs_amd.renderer import render_initial
    with rz.deferred_count() as box:
        render_initial(cam, pc, pipe, bg)
        assert len(box.pending) == 1 and box.pending[0].value is None
    with pytest.raises(rz.RasterWorkspaceOverflow):
        box.finish()
    assert rz._PAIR_GUESS[key] >= R0


@pytest.mark.gpu
def test_overflowed_view_is_an_empty_render_and_the_traced_view_recovers(gpu_device):
    """What is queued behind a rasterizer whose pair guess was too small runs on a DEFINED image: the tile sort leaves every list empty
    (csrc/mrgs_binning.hip), so the blend writes the background -- no NaN rays into the tracer, no undefined maps into the shading.  The
    render function then redoes the view; through the traced view (hierarchy build + mirror rays + trace behind the rasterizer) that
    costs two views' time, not a walk of garbage rays."""
    import time
    from types import SimpleNamespace
    from materialrefgs_amd import rasterizer as rz
    from materialrefgs_amd.renderer import render_initial, render_surfel_with_envgs
    from materialrefgs_amd.surfel_tracing import HardwareRendering
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    P, H, W = 20_000, 200, 200
    pc, env, leaves = make_surfel_model(P, H, dev, radius_px=3.0)
    cam = orbit_camera(1, H, W).to(dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    bg = torch.zeros(3, device=dev)
    key = (dev.index, P, H, W)
    env.build_mips()
    with torch.no_grad():
        good = render_initial(cam, pc, pipe, bg)
        R0 = rz.LAST_NUM_RENDERED
        rz._PAIR_GUESS[key] = max(R0 // 3, 1)
        with rz.deferred_count() as box:
            bad = render_initial(cam, pc, pipe, bg)
        torch.cuda.synchronize(dev)
        for k in ("render", "rend_alpha", "rend_normal", "surf_depth"):
            assert torch.isfinite(bad[k]).all(), k
        assert float(bad["rend_alpha"].abs().max()) == 0.0 and float(good["rend_alpha"].max()) > 0.5       # an empty render, not garbage
        with pytest.raises(rz.RasterWorkspaceOverflow):
            box.finish()
        tracer = HardwareRendering().train()
        opt = SimpleNamespace(indirect=False)
        ref = render_surfel_with_envgs(tracer, cam, pc, pipe, bg, srgb=False, opt=opt)["render"].clone()
        torch.cuda.synchronize(dev)
        rz._PAIR_GUESS[key] = max(R0 // 3, 1)
        t0 = time.perf_counter()
        again = render_surfel_with_envgs(tracer, cam, pc, pipe, bg, srgb=False, opt=opt)["render"]
        torch.cuda.synchronize(dev)
        assert time.perf_counter() - t0 < 5.0
        assert torch.isfinite(again).all() and float((again - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
