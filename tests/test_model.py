"""GaussianModel (materialrefgs_amd/model.py): without a GPU the class surface -- learning rates with the reference's env2 quirk, the xyz
schedule, the SH degree, capture()'s order, the direction grids and get_normal against the reference's recorded values, the refusals -- and
on the GPU every reset method against the float64 statement, the three fused steps against the sequence of their single methods, the
optimizer surgery, and one closed training loop with densification, both reset steps and the file round trips."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import model_statement as ms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_model.npz")
ATTRS = {"xyz": ("_xyz", (3,)), "f_dc": ("_features_dc", (1, 3)), "f_rest": ("_features_rest", (15, 3)), "opacity": ("_opacity", (1,)),
         "scaling": ("_scaling", (2,)), "rotation": ("_rotation", (4,)), "refl_strength": ("_refl_strength", (1,)), "ori_color": ("_ori_color", (3,)),
         "diffuse_color": ("_diffuse_color", (3,)), "roughness": ("_roughness", (1,)), "metalness": ("_metalness", (1,)), "normal1": ("_normal1", (3,)),
         "normal2": ("_normal2", (3,)), "ind_dc": ("_indirect_dc", (1, 3)), "ind_rest": ("_indirect_rest", (15, 3)), "ind_asg": ("_indirect_asg", (32, 5))}


def build_model(P, device="cpu", values=None, optimizer_cls=None, stepped=False, seed=0):
    """A GaussianModel over random parameters (`values`: {group: numpy array} where given) with training_setup done; `stepped` gives every
    group the state of an optimizer that has taken three steps, with non-zero moments."""
    from materialrefgs_amd import checkpoint
    from materialrefgs_amd.model import GaussianModel
    g = torch.Generator().manual_seed(seed)
    m = GaussianModel(3)
    for name, (attr, shape) in ATTRS.items():
        t = torch.from_numpy(np.asarray(values[name], dtype=np.float32)) if values and name in values else torch.randn((P,) + shape, generator=g)
        setattr(m, attr, torch.nn.Parameter(t.to(device).contiguous().requires_grad_(True)))
    m.max_radii2D = torch.zeros(P, device=device)
    m.spatial_lr_scale = 2.0
    m.training_setup(checkpoint.default_training_args(), optimizer_cls=optimizer_cls)
    if stepped:
        for grp in m.optimizer.param_groups:
            for p in grp["params"]:
                m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.full_like(p, 0.5), "exp_avg_sq": torch.full_like(p, 0.25)}
    return m


# ---- host logic on CPU tensors ------------------------------------------------------------------------------------------------------------
def test_learning_rate_methods_and_the_env2_quirk():
    m = build_model(5, optimizer_cls=torch.optim.Adam)
    names = [g["name"] for g in m.optimizer.param_groups]
    assert names == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "env", "env2", "refl_strength", "ori_color", "diffuse_color", "roughness",
                     "metalness", "normal1", "normal2", "ind_dc", "ind_rest", "ind_asg"]
    assert not m._normal1.requires_grad and not m._normal2.requires_grad and m.percent_dense == 0.01
    before = {g["name"]: g["lr"] for g in m.optimizer.param_groups}
    assert before["xyz"] == 0.00016 * 2.0 and before["env2"] == 0.01
    m.set_opacity_lr(0.0)
    assert {g["name"]: g["lr"] for g in m.optimizer.param_groups} == dict(before, opacity=0.0)
    m.set_opacity_lr(0.05)
    m.frozen_gaussian_gemotry()
    frozen = {g["name"]: g["lr"] for g in m.optimizer.param_groups}
    assert all(frozen[n] == 0 for n in ("xyz", "scaling", "opacity", "rotation", "env", "env2"))
    assert all(frozen[n] == before[n] for n in names if n not in ("xyz", "scaling", "opacity", "rotation", "env", "env2"))
    assert m.lr_dict == {n: before[n] for n in ("xyz", "opacity", "scaling", "rotation", "env", "env2")}
    m.restore_gaussian_gemotry_lr()
    after = {g["name"]: g["lr"] for g in m.optimizer.param_groups}
    assert after == dict(before, env2=0)                         # the reference never restores env2 (gaussian_model.py:232-233)


def test_update_learning_rate_against_the_closed_form():
    m = build_model(3, optimizer_cls=torch.optim.Adam)
    a = SimpleNamespace(init=0.00016 * 2.0, final=0.0000016 * 2.0, steps=30000)
    for it in (0, 1, 777, 15000, 29999, 30000, 45000):
        t = min(it / a.steps, 1.0)
        want = math.exp(math.log(a.init) * (1 - t) + math.log(a.final) * t)
        assert m.update_learning_rate(it) == pytest.approx(want, rel=1e-12) and m.optimizer.param_groups[0]["lr"] == pytest.approx(want, rel=1e-12)
    assert m.update_learning_rate(-1) == 0.0


def test_sh_degree_methods_and_getters():
    from materialrefgs_amd.model import GaussianModel
    m = GaussianModel(2)
    assert (m.active_sh_degree, m.max_sh_degree, m.enlarge_scale, m.refl_msk_thr, m.rough_msk_thr, m.init_refl_value) == (0, 2, 1.5, 0.02, 0.1, 0.1)
    for want in (1, 2, 2):
        m.oneupSHdegree()
        assert m.active_sh_degree == want
    m.rstSHdegree()
    assert m.active_sh_degree == 0 and m.get_envmap is None and m.get_envmap_2 is None and m.optimizer is None
    m = build_model(6, optimizer_cls=torch.optim.Adam)
    assert torch.equal(m.get_opacity, torch.sigmoid(m._opacity)) and torch.equal(m.get_specular, torch.sigmoid(m._metalness))
    assert torch.equal(m.get_diffuse_color, torch.sigmoid(m._diffuse_color)) and torch.equal(m.get_rough, torch.sigmoid(m._roughness))
    assert m.get_features.shape == (6, 16, 3) and m.get_indirect.shape == (6, 16, 3) and m.get_asg is m._indirect_asg and m.get_xyz is m._xyz
    assert len(m.asg_param) == 3 and m.asg_param[0].shape == (32, 3)
    assert float(m.get_refl_strength_to_total) == float((torch.sigmoid(m._refl_strength) > 0.1).sum()) / 6
    assert m.scaling_activation is torch.exp and m.opacity_activation is torch.sigmoid and m.rotation_activation is torch.nn.functional.normalize
    m.init_indirect_learning_stage()
    assert torch.equal(m._indirect_dc, m._features_dc) and torch.equal(m._indirect_rest, m._features_rest) and m._indirect_dc is not m._features_dc
    m.set_requires_grad("xyz", False)
    assert not m._xyz.requires_grad
    assert m.construct_list_of_attributes()[:9] == ["x", "y", "z", "nx", "ny", "nz", "nx2", "ny2", "nz2"] and len(m.construct_list_of_attributes()) == 9 + 3 + 45 + 3 + 45 + 160 + 4 + 6 + 2 + 4


def test_capture_order_is_the_references():
    from materialrefgs_amd import checkpoint
    z = np.load(GOLDEN)
    order = [str(s) for s in z["capture_order"]]
    assert order == list(checkpoint.CAPTURE_FIELDS) + ["optimizer.state_dict()", "spatial_lr_scale"]
    m = build_model(4, optimizer_cls=torch.optim.Adam, stepped=True)
    m.active_sh_degree = 2
    m.xyz_gradient_accum += 1.0
    cap = m.capture()
    assert len(cap) == 22 and cap[0] == 2 and cap[21] == 2.0 and set(cap[20]) == {"state", "param_groups"}
    for i, name in enumerate(checkpoint.CAPTURE_FIELDS[1:], start=1):
        assert cap[i] is getattr(m, name), name
    from materialrefgs_amd.model import GaussianModel
    n = GaussianModel(3)
    n.optimizer = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])           # restore() rebuilds the same kind of optimizer
    n.restore(cap, checkpoint.default_training_args())
    assert n.active_sh_degree == 2 and n._xyz is m._xyz and n.xyz_gradient_accum is m.xyz_gradient_accum and n.spatial_lr_scale == 2.0
    assert float(n.optimizer.state[n._opacity]["exp_avg"].mean()) == 0.5 and n.update_learning_rate(0) == pytest.approx(0.00032)


def test_direction_grids_and_get_normal_against_the_reference():
    from materialrefgs_amd.model import get_env_direction1, get_env_direction2
    z = np.load(GOLDEN)
    d1, d2 = get_env_direction1(8, 16).numpy(), get_env_direction2(8, 16).numpy()
    assert d1.shape == d2.shape == (8, 16, 3)
    assert np.abs(d1 - z["env_direction1_8x16"]).max() <= 2.0 ** -22 and np.abs(d2 - z["env_direction2_8x16"]).max() <= 2.0 ** -22
    assert np.allclose(np.linalg.norm(d1, axis=-1), 1.0, atol=1e-6)
    n = 16
    values = {k: z[f"normal_in_{k}"] for k in ("xyz", "rotation", "normal1", "normal2", "scaling")}
    m = build_model(n, values=values, optimizer_cls=torch.optim.Adam)
    dirs = torch.from_numpy(z["normal_in_dirs"])
    with torch.no_grad():
        normals, delta = m.get_normal(1.0, dirs, return_delta=True)
        plain = m.get_normal(1.0, dirs)
    assert np.array_equal(delta.numpy(), z["normal_out_delta"])                      # a selection of stored rows: exact
    assert np.abs(normals.numpy() - z["normal_out"]).max() <= 1e-6 and np.abs(plain.numpy() - z["normal_out_plain"]).max() <= 1e-6
    m = build_model(2, optimizer_cls=torch.optim.Adam)
    assert m.env_directions1.shape == (256, 512, 3) and m.env_directions2.shape == (256, 512, 3) and m.env_directions1 is m.env_directions1


def test_left_out_methods_say_why():
    m = build_model(2, optimizer_cls=torch.optim.Adam)
    with pytest.raises(NotImplementedError, match="no-op in the reference"):
        m.reset_specular()
    for name in ("reset_opacity1_strategy2", "dist_rot", "dist_color2_specular", "enlarge_refl_scales2", "reset_scale2_specular"):
        with pytest.raises(NotImplementedError, match=f"GaussianModel.{name}: no training script"):
            getattr(m, name)()
    for name in ("get_points_from_depth", "get_points_depth_in_depth_map", "get_triangles"):
        with pytest.raises(NotImplementedError, match=f"GaussianModel.{name}: its only callers are native"):
            getattr(m, name)(None, None)


def test_resets_on_cpu_tensors_raise():
    m = build_model(4, optimizer_cls=torch.optim.Adam, stepped=True)
    for call in (m.reset_opacity0, m.reset_opacity1, m.reset_refl, m.reset_refl_strength, m.reset_refl_strength2, m.reset_roughness, m.reset_ori_color,
                 m.reset_features, m.dist_color, m.dist_albedo, m.reset_scale, m.enlarge_refl_scales, m.normal_propagation_step, m.opacity_reset_step,
                 lambda: m.material_reset_step(0.1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert m.active_sh_degree == 0 and m.optimizer.state[m._opacity]["step"] == 3.0


def test_exclusive_mask_is_checked_before_anything_else():
    """A mask that is not a bool / uint8 [P] tensor on the model's device is refused by every method that takes one, enlarge_refl_scales
    included, before any pointer is taken (here: on a CPU model, whose own tensors would be refused next)."""
    P = 4
    m = build_model(P, optimizer_cls=torch.optim.Adam, stepped=True)
    takers = (m.reset_opacity1, m.reset_refl, m.dist_color, m.dist_albedo, m.reset_scale, m.normal_propagation_step, m.opacity_reset_step,
              lambda exclusive_msk: m.enlarge_refl_scales(exclusive_msk=exclusive_msk), lambda exclusive_msk: m.enlarge_refl_scales(False, exclusive_msk=exclusive_msk))
    for bad in (torch.zeros(P, dtype=torch.bool), torch.zeros(P - 1, dtype=torch.bool), torch.zeros(P + 1, dtype=torch.uint8), torch.zeros(P, 1, dtype=torch.bool),
                torch.zeros(P), [False] * P):
        for call in takers:
            with pytest.raises(ValueError, match="exclusive_msk must be"):
                call(exclusive_msk=bad)
    assert float(m.optimizer.state[m._opacity]["exp_avg"].mean()) == 0.5


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
def _gpu_pair(dev, P=257, seed=4, stepped=True):
    model, excl, u = ms.random_model(P, seed)
    make = lambda: build_model(P, dev, values=model, stepped=stepped, seed=seed)
    return model, torch.from_numpy(excl).to(dev), {k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in u.items()}, excl, u, make


def _raw(m):
    return {name: getattr(m, attr).detach().cpu().numpy() for name, (attr, _s) in ATTRS.items()}


def _assert_surgery(m, before, replaced, stepped=True):
    """Replaced groups are new Parameter objects the optimizer and the model share, with zero moments and the old step; the others are untouched."""
    for grp in m.optimizer.param_groups:
        if grp["name"] in ("env", "env2"):
            continue
        p = grp["params"][0]
        assert getattr(m, ATTRS[grp["name"]][0]) is p
        assert (p is not before[grp["name"]]) == (grp["name"] in replaced), grp["name"]
        if grp["name"] in replaced:
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and before[grp["name"]] not in m.optimizer.state
        st = m.optimizer.state.get(p)
        if not stepped:
            assert st is None or len(st) == 0
            continue
        assert float(st["step"]) == 3.0 and st["exp_avg"].shape == p.shape
        if grp["name"] in replaced:
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        else:
            assert float(st["exp_avg"].mean()) == 0.5 and float(st["exp_avg_sq"].mean()) == 0.25


@pytest.mark.gpu
def test_every_method_against_the_statement(gpu_device):
    model, excl_t, u_t, excl, u, make = _gpu_pair(gpu_device)
    logit_c = lambda a: (lambda x: np.where(x == ms.L(a), 2.0 ** -24 * np.abs(x), 0.0))      # L(a) rounded once; every other element is src's bits
    cases = [
        ("reset_opacity0", lambda m: m.reset_opacity0(), lambda: ms.reset_opacity0(model), {"opacity": logit_c(0.01)}),
        ("reset_opacity1", lambda m: m.reset_opacity1(excl_t), lambda: ms.reset_opacity1(model, excl), {"opacity": logit_c(0.9)}),
        ("reset_refl", lambda m: m.reset_refl(excl_t), lambda: ms.reset_refl(model, excl), {"refl_strength": logit_c(0.1)}),
        ("reset_refl 0.3", lambda m: m.reset_refl(rst_value=0.3), lambda: ms.reset_refl(model, None, 0.3), {"refl_strength": logit_c(0.3)}),
        ("reset_refl_strength", lambda m: m.reset_refl_strength(), lambda: ms.reset_refl_strength(model), {"refl_strength": logit_c(0.01)}),
        ("reset_refl_strength2", lambda m: m.reset_refl_strength2(), lambda: ms.reset_refl_strength2(model), {"refl_strength": logit_c(0.1)}),
        ("reset_roughness", lambda m: m.reset_roughness(0.25), lambda: ms.reset_roughness(model, 0.25), {"roughness": logit_c(0.25)}),
        ("reset_ori_color", lambda m: m.reset_ori_color(noise=u_t["ori_color"]), lambda: ms.reset_ori_color(model, u["ori_color"]),
         {"ori_color": lambda x: ms.jitter_const_tol(x, 0.5, 0.05)}),
        ("reset_features", lambda m: m.reset_features(), lambda: ms.reset_features(model), {"f_dc": 0.0, "f_rest": 0.0}),
        ("dist_color", lambda m: m.dist_color(excl_t, noise=u_t["f_dc"]), lambda: ms.dist_color(model, u["f_dc"], excl), {"f_dc": ms.jitter_tol}),
        ("dist_albedo", lambda m: m.dist_albedo(noise=u_t["ori_color"]), lambda: ms.dist_albedo(model, u["ori_color"]), {"ori_color": ms.jitter_tol}),
        ("reset_scale", lambda m: m.reset_scale(excl_t), lambda: ms.reset_scale(model, excl), {"scaling": ms.enlarge_tol}),
    ]
    for name, call, statement, tols in cases:
        m = make()
        m.active_sh_degree = 2
        before = {g["name"]: g["params"][0] for g in m.optimizer.param_groups if g["name"] not in ("env", "env2")}
        old = _raw(m)
        call(m)
        want, margin = statement()
        assert margin >= 1e-3
        new = _raw(m)
        _assert_surgery(m, before, set(tols))
        for grp in ATTRS:
            if grp not in tols:
                assert np.array_equal(new[grp], old[grp]), (name, grp)
                continue
            x = want[grp]
            tol = tols[grp](x) if callable(tols[grp]) else np.full(x.shape, tols[grp])
            untouched = x == model[grp]
            assert np.array_equal(new[grp][untouched], old[grp][untouched]), (name, grp)              # bit for bit
            assert np.all(np.abs(new[grp].astype(np.float64) - x) <= tol), (name, grp)
        assert m.active_sh_degree == (0 if name == "reset_features" else 2)
    m = make()
    raw_s, _ = ms.enlarge_refl_scales(model, True, excl)
    for ret_raw, want in ((True, raw_s), (False, np.exp(raw_s))):
        got = m.enlarge_refl_scales(ret_raw=ret_raw, exclusive_msk=excl_t).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want) <= (ms.enlarge_tol(want) if ret_raw else 3 * ms.EPS * np.abs(want) * (1 + np.abs(raw_s))))
    assert m._scaling is m.optimizer.param_groups[4]["params"][0]                                        # nothing was installed


@pytest.mark.gpu
@pytest.mark.parametrize("stepped", [True, False])
def test_fused_steps_equal_the_sequence_of_single_methods(gpu_device, stepped):
    """Bit for bit under the same noise, with and without optimizer state (before the first step no moments exist and none are created)."""
    model, excl_t, u_t, excl, u, make = _gpu_pair(gpu_device, seed=9, stepped=stepped)
    runs = [
        (lambda m: m.normal_propagation_step(excl_t, noise=u_t["f_dc"]),
         lambda m: (m.reset_opacity1(excl_t), m.dist_color(excl_t, noise=u_t["f_dc"]), m.reset_scale(excl_t)), {"opacity", "f_dc", "scaling"}),
        (lambda m: m.normal_propagation_step(None, dist_color=False), lambda m: (m.reset_opacity1(), m.reset_scale()), {"opacity", "scaling"}),
        (lambda m: m.opacity_reset_step(excl_t, 0.3), lambda m: (m.reset_opacity0(), m.reset_refl(excl_t, 0.3)), {"opacity", "refl_strength"}),
        (lambda m: m.opacity_reset_step(), lambda m: (m.reset_opacity0(), m.reset_refl()), {"opacity", "refl_strength"}),
        (lambda m: m.material_reset_step(0.2, noise=u_t["ori_color"]),
         lambda m: (m.reset_ori_color(noise=u_t["ori_color"]), m.reset_refl_strength(0.1), m.reset_roughness(0.2)), {"ori_color", "refl_strength", "roughness"}),
        (lambda m: m.material_reset_step(0.2, features=True, noise=u_t["ori_color"]),
         lambda m: (m.reset_ori_color(noise=u_t["ori_color"]), m.reset_refl_strength(0.1), m.reset_roughness(0.2), m.reset_features()),
         {"ori_color", "refl_strength", "roughness", "f_dc", "f_rest"}),
    ]
    for fused, sequence, replaced in runs:
        a, b = make(), make()
        a.active_sh_degree = b.active_sh_degree = 3
        before = {g["name"]: g["params"][0] for g in a.optimizer.param_groups if g["name"] not in ("env", "env2")}
        fused(a)
        sequence(b)
        ra, rb = _raw(a), _raw(b)
        for grp in ATTRS:
            assert np.array_equal(ra[grp].view(np.uint32), rb[grp].view(np.uint32)), grp
            assert (not np.array_equal(ra[grp], model[grp].astype(np.float32))) == (grp in replaced) if grp in model else True
        _assert_surgery(a, before, replaced, stepped)
        assert a.active_sh_degree == b.active_sh_degree == (0 if "f_rest" in replaced else 3)
    # the statement agrees with the fused step, and the generator is governed by torch.manual_seed
    a = make()
    a.normal_propagation_step(excl_t, noise=u_t["f_dc"])
    want, margin = ms.normal_propagation_step(model, u["f_dc"], excl)
    assert margin >= 1e-3 and np.all(np.abs(_raw(a)["f_dc"] - want["f_dc"]) <= ms.jitter_tol(want["f_dc"]))
    drawn = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        c = make()
        c.normal_propagation_step(excl_t)
        drawn.append(_raw(c)["f_dc"])
    assert np.array_equal(drawn[0], drawn[1]) and not np.array_equal(drawn[0], drawn[2])
    with pytest.raises(ValueError, match="draw nothing"):
        make().normal_propagation_step(dist_color=False, noise={"f_dc": u_t["f_dc"]})


@pytest.mark.gpu
def test_launch_inputs_are_checked_on_a_device_model(gpu_device):
    """What would make the kernel read a host address or past an allocation raises instead: a CPU or short mask, a group or a mask input
    whose rows are not xyz's, noise of another shape.  Nothing is installed by a refused call."""
    model, excl_t, u_t, _excl, _u, make = _gpu_pair(gpu_device, P=65)
    m = make()
    before = _raw(m)
    for bad in (excl_t.cpu(), excl_t[:-1], torch.cat((excl_t, excl_t[:1])), excl_t.float()):
        for call in (m.reset_opacity1, m.reset_scale, m.normal_propagation_step, lambda exclusive_msk: m.enlarge_refl_scales(exclusive_msk=exclusive_msk)):
            with pytest.raises(ValueError, match="exclusive_msk must be"):
                call(exclusive_msk=bad)
    with pytest.raises(ValueError, match="must have shape"):
        m.dist_color(noise=u_t["f_dc"][:-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.dist_color(noise=u_t["f_dc"].cpu())
    short = lambda t: torch.nn.Parameter(t.detach()[:-1].clone())
    good = m._scaling
    m._scaling = m.optimizer.param_groups[4]["params"][0] = short(good)
    for call in (m.reset_scale, m.enlarge_refl_scales, m.normal_propagation_step):
        with pytest.raises(ValueError, match="'scaling' does not share dim 0"):
            call()
    m._scaling = m.optimizer.param_groups[4]["params"][0] = good
    for attr in ("_refl_strength", "_roughness"):
        keep = getattr(m, attr)
        setattr(m, attr, short(keep))
        for call in (m.reset_scale, m.enlarge_refl_scales, m.reset_opacity0):
            with pytest.raises(ValueError, match="must have shape"):
                call()
        setattr(m, attr, keep)
    after = _raw(m)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    m.optimizer = None                                             # enlarge_refl_scales needs no optimizer, as in the reference; a reset does
    assert m.enlarge_refl_scales(exclusive_msk=excl_t).shape == (65, 2)
    with pytest.raises(ValueError, match="training_setup"):
        m.reset_scale()


@pytest.mark.gpu
def test_glue_methods_on_the_existing_pieces(gpu_device, tmp_path):
    """prune_points, the two optimizer helpers, render_env_map[_2], update_mesh / load_mesh_from_ply and load_ply(relight=True): one call each."""
    from materialrefgs_amd import io, raytracing
    from materialrefgs_amd.model import GaussianModel, get_env_direction1, get_env_direction2
    from materialrefgs_amd.shading import EnvLight
    from materialrefgs_amd.synthetic import sphere_mesh
    dev, P = gpu_device, 65
    m = build_model(P, dev, stepped=True, seed=2)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.rand(P, 1, device=dev), torch.ones(P, 1, device=dev), torch.rand(P, device=dev)
    old = _raw(m)
    accum = m.xyz_gradient_accum.clone()
    gone = torch.arange(P, device=dev) % 3 == 0
    m.prune_points(gone)
    n = int((~gone).sum())
    for grp in m.optimizer.param_groups:
        if grp["name"] in ("env", "env2"):
            continue
        p = grp["params"][0]
        assert getattr(m, ATTRS[grp["name"]][0]) is p and p.shape[0] == n and m.optimizer.state[p]["exp_avg"].shape == p.shape
        assert np.array_equal(p.detach().cpu().numpy(), old[grp["name"]][~gone.cpu().numpy()])
    assert torch.equal(m.xyz_gradient_accum, accum[~gone]) and m.denom.shape == (n, 1) and m.max_radii2D.shape == (n,)
    new = m.replace_tensor_to_optimizer(torch.full((n, 1), 0.25, device=dev), "opacity")
    assert set(new) == {"opacity"} and new["opacity"] is m.optimizer.param_groups[3]["params"][0] and not m.optimizer.state[new["opacity"]]["exp_avg"].any()
    m._opacity = new["opacity"]
    ext = {name: torch.ones((2,) + shape, device=dev) for name, (_a, shape) in ATTRS.items()}
    grown = m.cat_tensors_to_optimizer(ext)
    assert set(grown) == set(ATTRS) and all(t.shape[0] == n + 2 for t in grown.values())
    st = m.optimizer.state[grown["xyz"]]
    assert st["exp_avg"].shape == (n + 2, 3) and not st["exp_avg"][n:].any() and float(st["exp_avg"][:n].mean()) == 0.5
    # the two environment maps through the lat-long grids
    g = torch.Generator().manual_seed(1)
    for name, p in grown.items():
        setattr(m, ATTRS[name][0], p)
    for name in ("env_map", "env_map_2"):
        env = EnvLight(path=None, device=dev, max_res=32, trainable=True)
        with torch.no_grad():
            env.base.copy_(torch.randn(env.base.shape, generator=g).to(dev))
        env.build_mips()
        setattr(m, name, env)
    with torch.no_grad():
        for render, env in ((m.render_env_map, m.env_map), (m.render_env_map_2, m.env_map_2)):
            out = render(H=8)
            assert set(out) == {"env1", "env2"} and out["env1"].shape == (8, 16, 3)
            assert torch.equal(out["env1"], env(get_env_direction1(8, 16, dev), mode="pure_env"))
            assert torch.equal(out["env2"], env(get_env_direction2(8, 16, dev), mode="pure_env"))
        assert not torch.equal(m.render_env_map(H=8)["env1"], m.render_env_map_2(H=8)["env1"])
    # the mesh
    v, t = sphere_mesh(8, 12)
    m.update_mesh(SimpleNamespace(vertices=v, triangles=t))
    assert isinstance(m.ray_tracer, raytracing.RayTracer)
    first = m.ray_tracer
    io.save_mesh_ply(str(tmp_path / "test_000007.ply"), v, t)
    m.load_mesh_from_ply(str(tmp_path), 7)
    assert isinstance(m.ray_tracer, raytracing.RayTracer) and m.ray_tracer is not first
    # relighting: the PLY with an .hdr next to it
    path = str(tmp_path / "point_cloud.ply")
    m.env_map = m.env_map_2 = None
    m.save_ply(path)
    rng = np.random.default_rng(0)
    H, W = 16, 32
    rgbe = np.concatenate([rng.integers(16, 255, (H, W, 3)), np.full((H, W, 1), 128)], -1).astype(np.uint8)     # flat RGBE scanlines, values below 1
    with open(path.replace(".ply", ".hdr"), "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
        f.write(rgbe.tobytes())
    lit = GaussianModel(3)
    lit.load_ply(path, relight=True, device=dev)
    assert lit.env_map is not None and lit.env_map_2 is None and lit.env_map.base.is_cuda and float(lit.env_map.base.detach().abs().max()) > 0
    assert torch.equal(lit._xyz.detach(), m._xyz.detach()) and lit.active_sh_degree == 3


@pytest.mark.gpu
def test_closed_loop_with_densification_resets_and_round_trips(gpu_device, tmp_path):
    """create_from_pcd -> training_setup -> 30 iterations of render_surfel, calculate_loss, backward, statistics and Adam at P ~ 2k, 64 x 64,
    with densify_and_prune at 10 and 20, opacity_reset_step at 15 and normal_propagation_step at 25 (both with an exclusive mask); then the
    PLY and the checkpoint round trips.  Every tensor stays finite, the row counts agree everywhere, the restored model renders the same bits."""
    from materialrefgs_amd import checkpoint, losses
    from materialrefgs_amd import rasterizer as rz
    from materialrefgs_amd.model import GaussianModel
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    torch.manual_seed(0)
    P, H, W, n_cam = 2000, 64, 64, 4
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    bg, opt_r = torch.zeros(3, device=dev), SimpleNamespace(indirect=False)
    cams = [orbit_camera(v, H, W, n_views=n_cam).to(dev) for v in range(n_cam)]
    truth, env, _ = make_surfel_model(P, max(H, W), dev, seed=0, radius_px=4.0, env_res=32, env_min=8)
    targets = []
    with torch.no_grad():
        env.build_mips()
        for c in cams:
            gt = render_surfel(c, truth, pipe, bg, srgb=False, opt=opt_r)["render"].clone()
            targets.append(SimpleNamespace(original_image=gt, image_weight=losses.image_weight(gt)))
    rng = np.random.default_rng(0)
    pcd = SimpleNamespace(points=truth._xyz.detach().cpu().numpy().astype(np.float64), colors=rng.random((P, 3)))
    args = SimpleNamespace(envmap_max_res=32, envmap_min_roughness=0.08, envmap_max_roughness=0.5)
    gm = GaussianModel(3)
    gm.create_from_pcd(pcd, 1.0, args, device=dev)
    assert gm._xyz.shape == (P, 3) and gm._scaling.shape == (P, 2) and gm._indirect_asg.shape == (P, 32, 5) and gm._features_rest.shape == (P, 15, 3)
    assert float(gm.get_opacity.detach().min()) == pytest.approx(0.1, abs=1e-6) and float((gm.get_ori_color.detach() - 0.5).abs().max()) <= 0.0251
    assert not torch.equal(gm._ori_color, gm._diffuse_color) and gm.env_map is not gm.env_map_2 and gm.max_radii2D.shape == (P,)
    gm.training_setup(checkpoint.default_training_args())
    loss_opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.05, normal_loss_start=0, lambda_dist=100.0, dist_loss_start=100,
                               lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                               use_perceptual_loss=False)
    rz.reset_work_hints()
    rz._PAIR_GUESS.clear()

    def consistent():
        n = gm._xyz.shape[0]
        for grp in gm.optimizer.param_groups:
            if grp["name"] in ("env", "env2"):
                continue
            p = grp["params"][0]
            assert getattr(gm, ATTRS[grp["name"]][0]) is p and p.shape[0] == n and bool(torch.isfinite(p).all()), grp["name"]
            st = gm.optimizer.state.get(p)
            if st:
                assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape
                assert bool(torch.isfinite(st["exp_avg"]).all()) and bool(torch.isfinite(st["exp_avg_sq"]).all())
        assert gm.xyz_gradient_accum.shape == (n, 1) and gm.denom.shape == (n, 1) and gm.max_radii2D.shape == (n,)
        return n

    history, counts = [], [P]
    for it in range(1, 31):
        v = it % n_cam
        gm.update_learning_rate(it)
        gm.env_map.build_mips()
        out = render_surfel(cams[v], gm, pipe, bg, srgb=False, opt=opt_r)
        loss, _tb = losses.calculate_loss(targets[v], gm, out, loss_opt, it, targets[v].image_weight, None)
        loss.backward()
        gm.add_densification_stats(out["viewspace_points"], out["visibility_filter"], out["radii"])
        gm.optimizer.step()
        gm.optimizer.zero_grad(set_to_none=True)
        history.append(float(loss))
        outside = gm._xyz.detach()[:, 2] > 0.0
        if it in (10, 20):
            gr = (gm.xyz_gradient_accum / gm.denom).nan_to_num(0.0).reshape(-1)
            smax = gm.get_scaling.detach().max(dim=1).values
            n_keep, n_clone, n_child = gm.densify_and_prune(float(gr[gr > 0].median()), 0.005, float(smax.median()) / gm.percent_dense, None)
            assert n_clone > 0 and n_child > 0
            counts.append(consistent())
            assert counts[-1] == n_keep + n_clone + 2 * n_child
        if it == 15:
            old_o, old_r = gm._opacity, gm._refl_strength
            step = float(gm.optimizer.state[old_o]["step"])
            gm.opacity_reset_step(exclusive_msk=outside)
            assert gm._opacity is not old_o and gm._refl_strength is not old_r and float(gm.get_opacity.detach().max()) <= 0.01 + 1e-6
            kept = gm._refl_strength.detach()[outside]
            assert torch.equal(kept, old_r.detach()[outside]) and float(gm.get_refl.detach()[~outside].min()) >= 0.1 - 1e-6
            st = gm.optimizer.state[gm._opacity]
            assert float(st["step"]) == step and not st["exp_avg"].any() and old_o not in gm.optimizer.state
            consistent()
        if it == 25:
            old = {k: getattr(gm, k) for k in ("_opacity", "_features_dc", "_scaling")}
            # thresholds from what the loop observed (the training scripts set them from their options), so that every mask has both kinds of rows
            gm.refl_msk_thr, gm.rough_msk_thr = float(gm.get_refl.detach().median()), float(gm.get_rough.detach().median())
            gm.normal_propagation_step(exclusive_msk=outside)
            for k, t in old.items():
                new = getattr(gm, k)
                assert new is not t and torch.equal(new.detach()[outside], t.detach()[outside]) and not torch.equal(new.detach(), t.detach()), k
            assert float(gm.get_opacity.detach()[~outside].min()) >= 0.9 - 1e-6
            consistent()
    n = consistent()
    assert all(x == x and x < 1e3 for x in history) and counts[1] != P
    print(f"model loop: loss {history[0]:.4f} -> {history[-1]:.4f}; rows {counts}")

    # ---- PLY round trip (raw values are stored as fp32: exact), with the two .map files
    path = str(tmp_path / "point_cloud" / "iteration_30" / "point_cloud.ply")
    gm.save_ply(path)
    back = GaussianModel(3)
    back.load_ply(path, args=args, device=dev)
    assert back.active_sh_degree == 3
    for name, (attr, _s) in ATTRS.items():
        assert torch.equal(getattr(back, attr).detach(), getattr(gm, attr).detach()), name
    assert torch.equal(back.env_map.base.detach(), gm.env_map.base.detach()) and torch.equal(back.env_map_2.base.detach(), gm.env_map_2.base.detach())
    other = GaussianModel(3)
    other._xyz = torch.empty(0, device=dev)
    other.load_envlight(str(tmp_path), 30, args)
    assert torch.equal(other.env_map.base.detach(), gm.env_map.base.detach())

    # ---- checkpoint round trip: the restored model renders the same image bit for bit
    with torch.no_grad():
        gm.env_map.build_mips()
        image = render_surfel(cams[0], gm, pipe, bg, srgb=False, opt=opt_r)["render"].clone()
    ckpt = str(tmp_path / "chkpnt30.pth")
    checkpoint.save_checkpoint(ckpt, gm, 30)
    twin = GaussianModel(3)
    twin.env_map, twin.env_map_2 = gm.env_map, gm.env_map_2                          # the reference's restore() needs them in place as well
    assert checkpoint.load_checkpoint(ckpt, twin, checkpoint.default_training_args(), map_location=dev) == 30
    assert twin._xyz.shape[0] == n and twin.active_sh_degree == gm.active_sh_degree and twin.xyz_gradient_accum.shape == (n, 1)
    assert float(twin.optimizer.state[twin._xyz]["step"]) == float(gm.optimizer.state[gm._xyz]["step"])
    assert torch.equal(twin.optimizer.state[twin._opacity]["exp_avg"], gm.optimizer.state[gm._opacity]["exp_avg"])
    with pytest.raises(RuntimeError, match="no xyz schedule"):                      # checkpoint.load_checkpoint sets up the optimizer alone
        twin.update_learning_rate(31)
    twin2 = GaussianModel(3)
    twin2.env_map, twin2.env_map_2 = gm.env_map, gm.env_map_2
    twin2.restore(gm.capture(), checkpoint.default_training_args())
    twin3 = GaussianModel(3)
    twin3.env_map, twin3.env_map_2 = gm.env_map, gm.env_map_2
    assert twin3.load_checkpoint(ckpt, checkpoint.default_training_args(), map_location=dev) == 30
    assert twin2.update_learning_rate(31) == twin3.update_learning_rate(31) == gm.update_learning_rate(31) > 0
    with torch.no_grad():
        for t in (twin, twin2, twin3):
            t.env_map.build_mips()
            again = render_surfel(cams[0], t, pipe, bg, srgb=False, opt=opt_r)["render"]
            assert torch.equal(again, image)
