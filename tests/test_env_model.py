"""EnvGaussianModel (materialrefgs_amd/env_model.py): the class surface without a GPU -- the groups of training_setup, the capture /
restore tuple, restore_from_refgs, update_env_gs's schedule with a recording stub in place of the kernels, the refusals -- and on the GPU
create_from_pcd and one end-to-end run of the last training stage's loop on the tracer's smallest scene."""
from types import SimpleNamespace

import pytest
import torch

OPT = SimpleNamespace(position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
                      features_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3, percent_dense=0.5)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
SHAPES = {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_scaling": (2,), "_rotation": (4,), "_opacity": (1,)}


def cpu_model(P=5, seed=0, dtype=torch.float32):
    from materialrefgs_amd.env_model import EnvGaussianModel
    g = torch.Generator().manual_seed(seed)
    m = EnvGaussianModel(3)
    for n in NAMES:
        setattr(m, n, torch.nn.Parameter(torch.randn((P,) + SHAPES[n], generator=g).to(dtype)))
    m.max_radii2D = torch.zeros(P)
    m.spatial_lr_scale = 2.0
    m.training_setup(OPT)
    return m


def test_training_setup_groups_getters_and_schedule():
    from materialrefgs_amd import optim
    from materialrefgs_amd.env_model import EnvGaussianModel
    m = cpu_model()
    assert isinstance(m.optimizer, optim.Adam) and m.optimizer.defaults["eps"] == 1e-15 and m.optimizer.defaults["lr"] == 0.0
    got = [(g["name"], g["lr"], g["params"][0]) for g in m.optimizer.param_groups]
    want = [("xyz", 1.6e-4 * 2.0, m._xyz), ("f_dc", 2.5e-3, m._features_dc), ("f_rest", 2.5e-3 / 20.0, m._features_rest), ("opacity", 0.05, m._opacity),
            ("scaling", 5e-3, m._scaling), ("rotation", 1e-3, m._rotation)]
    assert len(got) == 6 and all(a[0] == b[0] and a[1] == b[1] and a[2] is b[2] for a, b in zip(got, want))
    assert m.percent_dense == 0.01                                   # fixed, whatever training_args.percent_dense says
    assert (m.max_gs, m.max_gs_threshold) == (2e6, 0.9)
    for s in (m.xyz_gradient_accum, m.xyz_weight_accum, m.denom):
        assert s.shape == (5, 1) and float(s.abs().sum()) == 0.0
    # the activations by identity: surfel_tracing._raw_model's fast path asks for exactly these
    assert m.scaling_activation is torch.exp and m.opacity_activation is torch.sigmoid and m.rotation_activation is torch.nn.functional.normalize
    assert torch.equal(m.get_scaling, torch.exp(m._scaling)) and torch.equal(m.get_opacity, torch.sigmoid(m._opacity))
    assert torch.allclose(m.get_rotation.norm(dim=1), torch.ones(5)) and m.get_xyz is m._xyz and m.get_features.shape == (5, 16, 3)
    # the xyz schedule: log-linear between the two ends
    assert m.update_learning_rate(0) == pytest.approx(3.2e-4) and m.update_learning_rate(30000) == pytest.approx(3.2e-6)
    assert m.update_learning_rate(15000) == pytest.approx(3.2e-5) and m.update_learning_rate(-1) == 0.0
    assert m.optimizer.param_groups[0]["lr"] == 0.0
    # SH degree
    e = EnvGaussianModel(2)
    for want_deg in (1, 2, 2):
        e.oneupSHdegree()
        assert e.active_sh_degree == want_deg
    # the covariance's third axis is the normal; get_normal turns it towards the viewer
    m2 = cpu_model(P=3)
    with torch.no_grad():
        m2._rotation.copy_(torch.tensor([[1.0, 0, 0, 0]] * 3))
    cov = m2.get_covariance()
    assert cov.shape == (3, 4, 4) and torch.allclose(cov[:, 3, :3], m2._xyz) and torch.allclose(cov[:, 2, :3], torch.tensor([[0.0, 0, 1]] * 3))
    dirs = torch.tensor([[0.0, 0, 1], [0, 0, -1], [0, 1, 0]])        # viewing along +z: the normal faces the viewer as -z
    assert torch.allclose(m2.get_normal(1.0, dirs), torch.tensor([[0.0, 0, -1], [0, 0, 1], [0, 0, 1]]))
    m2.xyz_weight_accum, m2.xyz_gradient_accum, m2.denom = torch.tensor([[2.0], [0], [3]]), torch.tensor([[1.0], [0], [6]]), torch.tensor([[4.0], [0], [2]])
    assert m2.get_xyz_weight_avg().tolist() == [[0.5], [0.0], [1.5]] and m2.get_xyz_gradient_avg().tolist() == [[0.25], [0.0], [3.0]]


def test_capture_restore_round_trip():
    from materialrefgs_amd.env_model import EnvGaussianModel
    m = cpu_model(seed=1)
    m.active_sh_degree = 2
    m.xyz_gradient_accum += 1.0; m.xyz_weight_accum += 2.0; m.denom += 3.0; m.max_radii2D += 4.0
    for g in m.optimizer.param_groups:                               # a stepped optimizer: its state travels in the tuple
        p = g["params"][0]
        m.optimizer.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.full_like(p, 0.5), "exp_avg_sq": torch.full_like(p, 0.25)}
    cap = m.capture()
    assert len(cap) == 13 and cap[0] == 2 and cap[12] == 2.0
    assert [cap[i] is t for i, t in zip(range(1, 11), (m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity, m.max_radii2D,
                                                          m.xyz_gradient_accum, m.xyz_weight_accum, m.denom))] == [True] * 10
    assert set(cap[11]) == {"state", "param_groups"}
    n = EnvGaussianModel(3)
    n.restore(cap, OPT)
    assert n.active_sh_degree == 2 and n.spatial_lr_scale == 2.0 and all(getattr(n, a) is getattr(m, a) for a in NAMES)
    assert n.xyz_gradient_accum is m.xyz_gradient_accum and n.xyz_weight_accum is m.xyz_weight_accum and n.denom is m.denom
    assert float(n.max_radii2D[0]) == 4.0
    st = n.optimizer.state[n.optimizer.param_groups[3]["params"][0]]
    assert float(st["exp_avg"].mean()) == 0.5 and float(st["exp_avg_sq"].mean()) == 0.25 and n.optimizer.param_groups[3]["name"] == "opacity"


def test_restore_from_refgs_takes_the_22_tuple():
    from materialrefgs_amd.env_model import EnvGaussianModel
    P = 4
    t = {k: torch.nn.Parameter(torch.full((P,) + sh, float(i))) for i, (k, sh) in enumerate(
        [("xyz", (3,)), ("refl", (1,)), ("metal", (1,)), ("rough", (1,)), ("ori", (3,)), ("diffuse", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)),
         ("ind_dc", (1, 3)), ("ind_rest", (15, 3)), ("ind_asg", (32, 5)), ("scaling", (2,)), ("rotation", (4,)), ("opacity", (1,)), ("n1", (3,)),
         ("n2", (3,))])}
    accum = torch.full((P, 1), 7.0)
    args = (3, t["xyz"], t["refl"], t["metal"], t["rough"], t["ori"], t["diffuse"], t["f_dc"], t["f_rest"], t["ind_dc"], t["ind_rest"], t["ind_asg"],
            t["scaling"], t["rotation"], t["opacity"], t["n1"], t["n2"], torch.full((P,), 9.0), accum, torch.full((P, 1), 8.0), {"unused": 1}, 1.5)
    assert len(args) == 22
    m = EnvGaussianModel(3)
    m.restore_from_refgs(args, OPT)
    assert m.active_sh_degree == 3 and m.spatial_lr_scale == 1.5 and m.start_iter == 12500
    assert m._xyz is t["xyz"] and m._features_dc is t["f_dc"] and m._features_rest is t["f_rest"] and m._scaling is t["scaling"]
    assert m._rotation is t["rotation"] and m._opacity is t["opacity"] and m._metalness is t["metal"]
    assert m.xyz_gradient_accum is accum and float(m.max_radii2D.abs().sum()) == 0.0 and m.max_radii2D.shape == (P,)
    assert float(m.denom.abs().sum()) == 0.0 and m.denom.shape == (P, 1) and m.xyz_weight_accum.shape == (P, 1)      # the optimizer and these are new
    assert [g["name"] for g in m.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"] and len(m.optimizer.state) == 0
    assert m.optimizer.param_groups[0]["lr"] == 1.6e-4 * 1.5


def test_update_env_gs_schedule_with_a_recording_stub(capsys):
    from materialrefgs_amd.env_model import EnvGaussianModel

    class Recording(EnvGaussianModel):
        def __init__(self):
            super().__init__(3)
            self.calls = []

        def add_densification_stats(self, viewspace_point_tensor, update_filter, weight_accumulate=None):
            self.calls.append(("stats", viewspace_point_tensor, update_filter, weight_accumulate))

        def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size=None, split_screen_threshold=None, **kw):
            self.calls.append(("densify", max_grad, min_opacity, extent, max_screen_size, split_screen_threshold))

    m = Recording()
    for n in NAMES:
        setattr(m, n, torch.nn.Parameter(torch.zeros((3,) + SHAPES[n])))
    m.spatial_lr_scale = 1.0
    m.training_setup(OPT)
    m.start_iter = 12500
    scene = SimpleNamespace(cameras_extent=4.0)
    pkg = {"viewspace_points": "vp", "visibility_filter": "vf", "weight_accumulate": "wa"}
    run = lambda it: (m.calls.clear(), m.update_env_gs(it, OPT, scene, pkg), list(m.calls))[2]
    assert run(12501) == [("stats", "vp", "vf", "wa")]
    assert m.optimizer.param_groups[0]["lr"] == pytest.approx(m.xyz_scheduler_args(1)) and m.active_sh_degree == 0
    assert run(13000) == [("stats", "vp", "vf", "wa"), ("densify", 1e-4 / 2, 0.05, 4.0, 20, None)] and m.active_sh_degree == 1
    out = capsys.readouterr().out
    assert "Before Densify f013000: 000003 points" in out and "After Densify f013000: 000003 points" in out
    assert run(5500) == [("stats", "vp", "vf", "wa"), ("densify", 1e-4 / 2, 0.05, 4.0, None, None)]          # no screen term up to iteration 6000
    assert run(6000)[1][4] is None and run(6500)[1][4] == 20
    assert run(0) == [] and m.active_sh_degree == 2                   # 6000 raised it; iteration 0 does nothing at all
    assert run(20500)[1][0] == "densify" and run(20999) == [("stats", "vp", "vf", "wa")]
    sh = m.active_sh_degree
    assert run(21000) == [] and m.active_sh_degree == min(sh + 1, 3)  # the schedule and the SH degree go on, the policy has ended
    assert run(22500) == [] and m.optimizer.param_groups[0]["lr"] == pytest.approx(m.xyz_scheduler_args(10000))


def test_cpu_tensors_and_unserved_arguments_raise():
    from materialrefgs_amd import env_model
    m = cpu_model()
    with pytest.raises(RuntimeError, match="device tensor"):
        m.densify_and_prune(5e-5, 0.05, 5.0, 20)
    with pytest.raises(NotImplementedError, match="split_screen_threshold"):
        m.densify_and_prune(5e-5, 0.05, 5.0, 20, 0.1)
    with pytest.raises(ValueError, match="max_grad"):
        m.densify_and_prune(0.0, 0.05, 5.0, 20)
    with pytest.raises(RuntimeError, match="device tensor"):
        m.add_densification_stats(torch.zeros(5, 3), torch.ones(5, dtype=torch.bool), torch.zeros(5, 1))
    with pytest.raises(RuntimeError, match="device tensor"):
        m.prune_points(torch.zeros(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="device tensor"):
        env_model.select_kth(torch.zeros(4), 0)
    del m.optimizer.param_groups[5]
    with pytest.raises(ValueError, match="six groups"):
        m.densify_and_prune(5e-5, 0.05, 5.0, 20)
    assert not hasattr(m, "save_ply") and not hasattr(m, "load_ply")   # left out: nothing in the loop calls them


# ---------------------------------------------------------------- on the GPU ---------------------------------------------------------
@pytest.mark.gpu
def test_create_from_pcd_prune_and_reset(gpu_device):
    from materialrefgs_amd.env_model import EnvGaussianModel
    g = torch.Generator().manual_seed(0)
    pts, cols = torch.rand(500, 3, generator=g), torch.rand(500, 3, generator=g)
    m = EnvGaussianModel(3)
    m.create_from_pcd(SimpleNamespace(points=pts.numpy(), colors=cols.numpy()), 1.5, device=gpu_device)
    assert m.spatial_lr_scale == 1.5 and all(getattr(m, n).shape == (500,) + SHAPES[n] and getattr(m, n).is_cuda for n in NAMES)
    d2 = torch.cdist(pts.double(), pts.double()) ** 2
    want = d2.sort(dim=1).values[:, 1:4].mean(dim=1).clamp_min(1e-7)             # distCUDA2: the mean squared distance to the three nearest
    assert torch.allclose(m.get_scaling.detach().cpu().double(), want.sqrt()[:, None].repeat(1, 2), rtol=1e-4)
    assert torch.allclose(m.get_opacity.detach().cpu(), torch.full((500, 1), 0.1), atol=1e-6) and float(m._features_rest.abs().sum()) == 0.0
    assert torch.allclose(m._features_dc.detach().cpu()[:, 0], (cols - 0.5) / 0.28209479177387814, atol=1e-5)
    m.training_setup(SimpleNamespace(**vars(OPT)))
    sum(getattr(m, n).sum() for n in NAMES).backward()
    m.optimizer.step()
    m.xyz_weight_accum += 1.0
    # non-fp32 statistics are refused
    m.denom = m.denom.double()
    with pytest.raises(TypeError, match="float32"):
        m.densify_and_prune(5e-5, 0.05, 5.0, 20)
    m.denom = m.denom.float()
    mask = torch.zeros(500, dtype=torch.bool, device=gpu_device)
    mask[::2] = True
    kept = m._xyz.detach()[1::2].clone()
    m.prune_points(mask)
    assert torch.equal(m._xyz.detach(), kept) and m.optimizer.param_groups[0]["params"][0] is m._xyz
    assert m.optimizer.state[m._xyz]["exp_avg"].shape == (250, 3)
    assert m.xyz_weight_accum.shape == (250, 1) and float(m.xyz_weight_accum.sum()) == 250.0 and m.max_radii2D.shape == (250,)
    m.reset_opacity()
    assert float(m.get_opacity.max()) <= 0.01 + 1e-6 and m.optimizer.param_groups[3]["params"][0] is m._opacity
    assert float(m.optimizer.state[m._opacity]["exp_avg"].abs().sum()) == 0.0
    m.reset_stats()
    assert float(m.xyz_weight_accum.abs().sum()) == 0.0 and m.denom.shape == (250, 1)


@pytest.mark.gpu
def test_last_stage_loop_on_the_tracers_smallest_scene(gpu_device):
    """Five iterations of render_surfel_with_envgs_sep + backward + update_env_gs on the 700-surfel second set of tests/test_surfel_tracing.py,
    densify_and_prune called directly after the fifth (env_densify_inter is 500 iterations away), then one more render: the row counts are
    consistent everywhere, the optimizer steps and the outputs are finite."""
    from test_render_e2e import _models
    from materialrefgs_amd import renderer
    from materialrefgs_amd.env_model import EnvGaussianModel
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.surfel_tracing import HardwareRendering
    from materialrefgs_amd.synthetic import orbit_camera, make_occluder_mesh
    dev = gpu_device
    P, H, W = 1500, 40, 56
    _, _, pc, _env = _models(P, H, W, seed=6, dev=dev)
    _, _, second, _ = _models(700, H, W, seed=8, dev=dev)
    env = EnvGaussianModel(3)
    for n in NAMES:
        setattr(env, n, torch.nn.Parameter(getattr(second, n).detach().clone()))
    with torch.no_grad():
        env._xyz.mul_(2.5)                                                      # a shell around the object
    env.active_sh_degree, env.spatial_lr_scale = 3, 1.0
    env.max_radii2D = torch.zeros(700, device=dev)
    env.training_setup(OPT)
    env.start_iter = 12500
    pc.ray_tracer = RayTracer(*make_occluder_mesh(4000), device=dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    hr = HardwareRendering().train()
    scene = SimpleNamespace(cameras_extent=3.0)
    opt = SimpleNamespace(indirect=True)

    def iteration(it):
        cam = orbit_camera(it % 8, H, W).to(dev)
        out = renderer.render_surfel_with_envgs_sep(hr, env, cam, pc, pipe, bg, srgb=False, opt=opt)
        out["render"].square().mean().backward()
        traced = out["indirect_out"]
        n = env._xyz.shape[0]
        assert traced["viewspace_points"].grad.shape == (n, 3) and traced["visibility_filter"].shape == (n,) and traced["weight_accumulate"].shape == (n, 1)
        env.update_env_gs(it, opt, scene, traced)
        env.optimizer.step()
        env.optimizer.zero_grad(set_to_none=True)
        assert bool(torch.isfinite(out["render"]).all())
        return traced

    for it in range(12501, 12506):
        traced = iteration(it)
    seen = env.denom.squeeze(1) > 0
    assert int(seen.sum()) > 20 and float(env.xyz_weight_accum[seen].sum()) > 0 and float(env.xyz_gradient_accum[seen].sum()) > 0
    assert float(env.denom.max()) <= 5.0 and float(env.xyz_weight_accum[~seen].abs().sum()) == 0.0
    assert env.optimizer.param_groups[0]["lr"] == pytest.approx(env.xyz_scheduler_args(5))
    before = {n: getattr(env, n).detach().clone() for n in NAMES}
    counts = env.densify_and_prune(1e-4 / 2, 0.05, scene.cameras_extent, 20, None, seed=3)
    rows = counts.rows
    assert rows == sum(counts.segments) and rows > 0 and counts.n_stage3 > 0
    assert counts.kept["original"] <= 700 and counts.kept["original"] + counts.kept["clone"] + counts.kept["child0"] + counts.kept["child1"] + counts.children5 == rows
    for g, n in zip(env.optimizer.param_groups, ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")):
        p = g["params"][0]
        assert p is getattr(env, n) and p.shape == (rows,) + SHAPES[n] and bool(torch.isfinite(p).all())
        st = env.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert float(st["exp_avg"][counts.kept["original"]:].abs().sum()) == 0.0          # every new row starts without momentum
    for s, shape in ((env.xyz_gradient_accum, (rows, 1)), (env.denom, (rows, 1)), (env.xyz_weight_accum, (rows, 1)), (env.max_radii2D, (rows,))):
        assert s.shape == shape and float(s.abs().sum()) == 0.0
    # the unsplit originals are a subsequence of the rows before, bit for bit
    if counts.kept["original"] == 700 and rows == 700:
        assert all(torch.equal(getattr(env, n).detach(), before[n]) for n in NAMES)
    iteration(12506)
    assert env.denom.shape == (rows, 1) and float(env.denom.sum()) > 0
