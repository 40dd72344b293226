"""GaussianModel: the object every training script starts from (`gaussians = GaussianModel(dataset.sh_degree)`, the reference's
scene/gaussian_model.py), composed from this package's native pieces -- knn.distCUDA2 and shading.EnvLight in create_from_pcd,
checkpoint for training_setup / capture / restore, io for the PLY and the .map files, densify for densify_and_prune, the statistics and the
optimizer surgery, raytracing.RayTracer for the mesh.  Constructor, attribute names, activations and method names are the reference's.

The reset family (gaussian_model.py:532-722) runs on csrc/mrgs_model_reset.hip: every method is ONE launch that writes the new raw
values and both zeroed Adam moments, installed as new nn.Parameters the way replace_tensor_to_optimizer does.  The three blocks the
training loops build from them are one launch each as well: normal_propagation_step, opacity_reset_step, material_reset_step.
No CPU path and no torch fallback: a reset on CPU tensors raises.  Differences from the reference are listed in INTEGRATION.md section 4i.
"""
import ctypes
import math
import os

import numpy as np
import torch
from torch import nn

from . import _lib, checkpoint, densify
from . import io as _io
from .env_model import expon_lr_func, inverse_sigmoid
from .gs_utils import RGB2SH, build_scaling_rotation, flip_align_view, predefined_asg_axes, safe_normalize

_PLY_KEYS = {"xyz": "_xyz", "normal1": "_normal1", "normal2": "_normal2", "features_dc": "_features_dc", "features_rest": "_features_rest",
             "indirect_dc": "_indirect_dc", "indirect_rest": "_indirect_rest", "indirect_asg": "_indirect_asg", "opacity": "_opacity",
             "refl_strength": "_refl_strength", "metalness": "_metalness", "roughness": "_roughness", "ori_color": "_ori_color",
             "diffuse_color": "_diffuse_color", "scaling": "_scaling", "rotation": "_rotation"}
_FROZEN = ("xyz", "scaling", "opacity", "rotation", "env", "env2")


def get_env_direction1(H, W, device=None):
    """Directions [H,W,3] of a latitude-longitude image with +y up: the polar angle theta runs over the pixel centres of (0, pi) down the
    rows, the azimuth phi over the pixel centres of (-pi, pi) along the columns; (sin theta sin phi, cos theta, -sin theta cos phi)."""
    theta = torch.linspace(0.0 + 1.0 / H, 1.0 - 1.0 / H, H, device=device) * np.pi
    phi = torch.linspace(-1.0 + 1.0 / W, 1.0 - 1.0 / W, W, device=device) * np.pi
    theta, phi = theta[:, None].expand(H, W), phi[None, :].expand(H, W)
    st = torch.sin(theta)
    return torch.stack((st * torch.sin(phi), torch.cos(theta), -st * torch.cos(phi)), dim=-1)


def get_env_direction2(H, W, device=None):
    """Directions [H,W,3] of a latitude-longitude image with +z up, sampled at the END points: theta over [0, pi] down the rows, phi over
    [-pi, pi] along the columns; (sin theta cos phi, sin theta sin phi, cos theta)."""
    phi = torch.linspace(-torch.pi, torch.pi, W, device=device)[None, :].expand(H, W)
    theta = torch.linspace(0, torch.pi, H, device=device)[:, None].expand(H, W)
    st = torch.sin(theta)
    return torch.stack((st * torch.cos(phi), st * torch.sin(phi), torch.cos(theta)), dim=-1)


def _left_out(name, why):
    def method(self, *args, **kwargs):
        raise NotImplementedError(f"GaussianModel.{name}: {why}")
    method.__name__ = name
    return method


class GaussianModel:
    def setup_functions(self):
        def covariance(center, scaling, scaling_modifier, rotation):
            RS = build_scaling_rotation(torch.cat([scaling * scaling_modifier, torch.ones_like(scaling[:, :1])], dim=-1), rotation).permute(0, 2, 1)
            trans = torch.zeros((center.shape[0], 4, 4), dtype=torch.float, device=center.device)
            trans[:, :3, :3] = RS
            trans[:, 3, :3] = center
            trans[:, 3, 3] = 1
            return trans
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.covariance_activation = covariance
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.refl_activation = torch.sigmoid
        self.inverse_refl_activation = inverse_sigmoid
        self.metalness_ativation = torch.sigmoid                  # (the reference's spelling)
        self.inverse_metalness_activation = inverse_sigmoid
        self.roughness_activation = torch.sigmoid
        self.inverse_roughness_activation = inverse_sigmoid
        self.color_activation = torch.sigmoid
        self.inverse_color_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        for name in ("_xyz", "_refl_strength", "_ori_color", "_diffuse_color", "_metalness", "_roughness", "_features_dc", "_features_rest",
                     "_indirect_dc", "_indirect_rest", "_indirect_asg", "_scaling", "_rotation", "_opacity", "max_radii2D",
                     "xyz_gradient_accum", "denom", "_normal1", "_normal2"):
            setattr(self, name, torch.empty(0))
        self.optimizer = None
        self.free_radius = 0
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.init_refl_value = 0.1
        self.init_roughness_value = 0.1
        self.init_metalness_value = 0.1
        self.init_ori_color = 0
        self.enlarge_scale = 1.5
        self.refl_msk_thr = 0.02
        self.rough_msk_thr = 0.1
        self.env_map = None
        self.env_map_2 = None
        self.env_H, self.env_W = 256, 512
        self._env_directions = None        # (device, directions1, directions2) at env_H x env_W, built on first use: the reference builds
        self._asg_axes = None              # them on "cuda" in the constructor, which a machine without a GPU could not run
        self.ray_tracer = None
        self.setup_functions()

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def capture(self):
        return checkpoint.capture(self)

    def restore(self, model_args, training_args):
        checkpoint.restore(self, model_args, training_args, type(self.optimizer) if self.optimizer is not None else None)
        self._set_scheduler(training_args)

    def load_checkpoint(self, path, training_args, map_location=None):
        """train_refnerf.py:1037-1040 through restore(), so that the xyz schedule exists afterwards; returns the checkpoint's iteration."""
        model_params, first_iter = torch.load(path, map_location=map_location, weights_only=False)
        self.restore(model_params, training_args)
        return first_iter

    def _device(self):
        return self._xyz.device if self._xyz.numel() else torch.device("cuda")

    def _new_envlight(self, args, path=None):
        from .shading import EnvLight
        if path is not None:
            return EnvLight(path=path, device=self._device(), trainable=True)
        return EnvLight(path=None, device=self._device(), max_res=args.envmap_max_res, min_roughness=args.envmap_min_roughness,
                        max_roughness=args.envmap_max_roughness, trainable=True)

    def _load_map_pair(self, ply_path, args):
        if os.path.exists(ply_path.replace(".ply", "1.map")) and os.path.exists(ply_path.replace(".ply", "2.map")):
            self.env_map, self.env_map_2 = self._new_envlight(args), self._new_envlight(args)
            _io.load_env_maps(ply_path, self.env_map, self.env_map_2)
            self.env_map.build_mips()
            self.env_map_2.build_mips()

    def load_envlight(self, dir_name, iters, args):
        self._load_map_pair(os.path.join(dir_name, "point_cloud", f"iteration_{iters}", "point_cloud.ply"), args)

    # ---- learning rates ---------------------------------------------------------------------------------------------------------
    def set_opacity_lr(self, lr):
        for group in self.optimizer.param_groups:
            if group["name"] == "opacity":
                group["lr"] = lr

    def frozen_gaussian_gemotry(self):
        lr_dict = {}
        for group in self.optimizer.param_groups:
            if group["name"] in _FROZEN:
                lr_dict[group["name"]] = group["lr"]
                group["lr"] = 0
        self.lr_dict = lr_dict

    def restore_gaussian_gemotry_lr(self):
        """xyz, scaling, opacity, rotation and env get their rates back.  env2 does NOT: the reference's line for it tests
        `param_group["lr"] == "env2"` and then compares instead of assigning (gaussian_model.py:232-233), so the second environment map
        stays at rate 0 after a freeze.  Followed literally."""
        for group in self.optimizer.param_groups:
            if group["name"] in _FROZEN[:5]:
                group["lr"] = self.lr_dict[group["name"]]

    def _set_scheduler(self, training_args):
        self.xyz_scheduler_args = expon_lr_func(lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                                                lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                                                lr_delay_mult=training_args.position_lr_delay_mult, max_steps=training_args.position_lr_max_steps)

    def training_setup(self, training_args, optimizer_cls=None):
        checkpoint.training_setup(self, training_args, optimizer_cls)
        self._set_scheduler(training_args)

    def update_learning_rate(self, iteration):
        if not hasattr(self, "xyz_scheduler_args"):
            raise RuntimeError("GaussianModel.update_learning_rate: no xyz schedule yet -- it is built by GaussianModel.training_setup / restore "
                               "(checkpoint.restore and checkpoint.load_checkpoint set up the optimizer alone; use GaussianModel.load_checkpoint)")
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = self.xyz_scheduler_args(iteration)
                return group["lr"]

    # ---- getters ----------------------------------------------------------------------------------------------------------------
    get_scaling = property(lambda s: s.scaling_activation(s._scaling))
    get_rotation = property(lambda s: s.rotation_activation(s._rotation))
    get_xyz = property(lambda s: s._xyz)
    get_opacity = property(lambda s: s.opacity_activation(s._opacity))
    get_refl = property(lambda s: s.refl_activation(s._refl_strength))
    get_rough = property(lambda s: s.roughness_activation(s._roughness))
    get_ori_color = property(lambda s: s.color_activation(s._ori_color))
    get_diffuse_color = property(lambda s: s.color_activation(s._diffuse_color))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))
    get_indirect = property(lambda s: torch.cat((s._indirect_dc, s._indirect_rest), dim=1))
    get_asg = property(lambda s: s._indirect_asg)
    get_specular = property(lambda s: s.metalness_ativation(s._metalness))
    get_envmap = property(lambda s: s.env_map)
    get_envmap_2 = property(lambda s: s.env_map_2)

    @property
    def asg_param(self):
        if self._asg_axes is None or self._asg_axes[0].device != self._device():
            self._asg_axes = predefined_asg_axes(4, 8, self._device())
        return self._asg_axes

    @property
    def get_refl_strength_to_total(self):
        refl = self.get_refl
        return (refl > 0.1).sum() / refl.shape[0]

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_xyz, self.get_scaling, scaling_modifier, self._rotation)

    def get_normal(self, scaling_modifier, dir_pp_normalized, return_delta=False):
        """The surfel's third axis turned towards the viewer; with return_delta the learned offset of the side that faces the viewer
        (_normal1 where the axis was not flipped, _normal2 where it was) is added before normalising and returned as well."""
        normals_raw, positive = flip_align_view(self.get_covariance(scaling_modifier)[:, 2, :3], dir_pp_normalized)
        if not return_delta:
            return safe_normalize(normals_raw)
        delta_normal = torch.where(positive, self._normal1, self._normal2)
        return safe_normalize(delta_normal + normals_raw), delta_normal

    def _directions(self, H):
        dev = self._device()
        if H != self.env_H:
            return get_env_direction1(H, H * 2, dev), get_env_direction2(H, H * 2, dev)
        if self._env_directions is None or self._env_directions[0] != dev:
            self._env_directions = (dev, get_env_direction1(self.env_H, self.env_W, dev), get_env_direction2(self.env_H, self.env_W, dev))
        return self._env_directions[1:]

    env_directions1 = property(lambda s: s._directions(s.env_H)[0])
    env_directions2 = property(lambda s: s._directions(s.env_H)[1])

    def render_env_map(self, H=512):
        d1, d2 = self._directions(H)
        return {"env1": self.env_map(d1, mode="pure_env"), "env2": self.env_map(d2, mode="pure_env")}

    def render_env_map_2(self, H=512):
        d1, d2 = self._directions(H)
        return {"env1": self.env_map_2(d1, mode="pure_env"), "env2": self.env_map_2(d2, mode="pure_env")}

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def rstSHdegree(self):
        self.active_sh_degree = 0

    @torch.no_grad()
    def init_indirect_learning_stage(self):
        self._indirect_dc[:] = self._features_dc[:] + 0.
        self._indirect_rest[:] = self._features_rest[:] + 0.

    def set_requires_grad(self, attrib_name, state: bool):
        getattr(self, f"_{attrib_name}").requires_grad = state

    # ---- set-up -----------------------------------------------------------------------------------------------------------------
    def create_from_pcd(self, pcd, spatial_lr_scale: float, args, device="cuda"):
        """gaussian_model.py:355-415.  The two colour initialisations draw from torch's generator on the device, ori_color first, as the
        reference does; the rotations before them."""
        from .knn import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        points = torch.tensor(np.asarray(pcd.points)).float().to(device)
        color = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().to(device))
        n, dev, coeffs = points.shape[0], points.device, (self.max_sh_degree + 1) ** 2
        sh_features = torch.zeros((n, 3, coeffs), device=dev)
        sh_features[:, :3, 0] = color
        sh_indirect = torch.zeros((n, 3, coeffs), device=dev)
        print("Number of points at initialisation : ", n)
        dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 2)
        rots = torch.rand((n, 4), device=dev)
        ones = torch.ones((n, 1), dtype=torch.float, device=dev)
        opacities = self.inverse_opacity_activation(0.1 * ones)
        refl = self.inverse_refl_activation(ones * self.init_refl_value)
        metalness = self.inverse_metalness_activation(ones * self.init_metalness_value)
        roughness = self.inverse_roughness_activation(ones * self.init_roughness_value)

        def initial_colour(init_color=0.5, noise_level=0.05):
            noise = (torch.rand(n, 3, dtype=torch.float, device=dev) - 0.5) * noise_level
            return self.inverse_color_activation(torch.clamp(torch.full((n, 3), init_color, dtype=torch.float, device=dev) + noise, 0.0, 1.0))
        ori_color = initial_colour()
        diffuse_color = initial_colour()
        param = lambda t: nn.Parameter(t.contiguous().requires_grad_(True))
        self._xyz = param(points)
        self._refl_strength, self._ori_color, self._diffuse_color = param(refl), param(ori_color), param(diffuse_color)
        self._roughness, self._metalness = param(roughness), param(metalness)
        self._scaling, self._rotation, self._opacity = param(scales), param(rots), param(opacities)
        self._features_dc = param(sh_features[:, :, 0:1].transpose(1, 2))
        self._features_rest = param(sh_features[:, :, 1:].transpose(1, 2))
        self._indirect_dc = param(sh_indirect[:, :, 0:1].transpose(1, 2))
        self._indirect_rest = param(sh_indirect[:, :, 1:].transpose(1, 2))
        self._indirect_asg = param(torch.zeros((n, 32, 5), device=dev))
        self._normal1 = param(torch.zeros((n, 3), device=dev))
        self._normal2 = param(torch.zeros((n, 3), device=dev))
        self.env_map, self.env_map_2 = self._new_envlight(args), self._new_envlight(args)
        self.max_radii2D = torch.zeros((n,), device=dev)

    # ---- files ------------------------------------------------------------------------------------------------------------------
    def construct_list_of_attributes(self):
        return _io.attribute_names({k: tuple(getattr(self, a).shape) for k, a in _PLY_KEYS.items()})

    def save_ply(self, path):
        _io.save_ply(path, {k: getattr(self, a) for k, a in _PLY_KEYS.items()}, self.env_map, self.env_map_2)

    def load_ply(self, path, relight=False, args=None, device=None):
        tensors = _io.load_ply(path, self.max_sh_degree, device if device is not None else self._device())
        self.active_sh_degree = self.max_sh_degree
        for k, a in _PLY_KEYS.items():
            setattr(self, a, nn.Parameter(tensors[k].contiguous().requires_grad_(True)))
        if not relight:
            self._load_map_pair(path, args)
        else:
            self.env_map = self._new_envlight(args, path=path.replace(".ply", ".hdr"))

    def update_mesh(self, mesh):
        from .raytracing import RayTracer
        self.ray_tracer = RayTracer(np.asarray(mesh.vertices).astype(np.float32), np.asarray(mesh.triangles).astype(np.int32))

    def load_mesh_from_ply(self, model_path, iteration):
        from types import SimpleNamespace
        vertices, triangles = _io.load_mesh_ply(os.path.join(model_path, f"test_{iteration:06d}.ply"))
        self.update_mesh(SimpleNamespace(vertices=vertices, triangles=triangles))

    # ---- densification ----------------------------------------------------------------------------------------------------------
    def _rebind(self, tensors):
        for name, p in tensors.items():
            setattr(self, densify.group_attr(name), p)

    def replace_tensor_to_optimizer(self, tensor, name):
        return densify.replace_tensor_to_optimizer(self.optimizer, tensor, name)

    def cat_tensors_to_optimizer(self, tensors_dict):
        return densify.cat_tensors_to_optimizer(self.optimizer, tensors_dict)

    def prune_points(self, mask):
        tensors, (self.xyz_gradient_accum, self.denom, self.max_radii2D) = densify.prune_optimizer(
            self.optimizer, ~mask, extra=[self.xyz_gradient_accum, self.denom, self.max_radii2D])
        self._rebind(tensors)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, *, seed=None, noise=None):
        return densify.densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, seed=seed, noise=noise)

    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None):
        densify.add_densification_stats(self, viewspace_point_tensor, update_filter, radii)

    # ---- resets: one launch of mrgs_model_reset each --------------------------------------------------------------------------------
    def _launch_reset(self, items, exclusive_msk=None, seed=None, noise=None, moments=True):
        """The one place that checks the inputs of mrgs_model_reset, builds its config and items and launches it.
        items: (group name, rule, keep bits, a, b) per parameter group.  noise: {group name: device fp32 uniforms of the group's shape}
        (or one tensor when a single item draws).  moments: also write zeroed moments for the groups whose optimizer state has them.
        Returns (groups, slots, tensors) as densify._install takes them: per item the new values, then its two moments where written."""
        P = int(self._xyz.shape[0])
        dev = self._xyz.device
        excl = None
        if exclusive_msk is not None:
            if not torch.is_tensor(exclusive_msk) or not exclusive_msk.is_cuda or exclusive_msk.dtype not in (torch.bool, torch.uint8) or \
                    tuple(exclusive_msk.shape) != (P,) or exclusive_msk.device != dev:
                raise ValueError("GaussianModel: exclusive_msk must be a bool / uint8 tensor of shape [P] on the model's device")
            excl = exclusive_msk.contiguous().view(torch.uint8)
        optimizer = self.optimizer
        by_name = {g.get("name"): g for g in optimizer.param_groups} if optimizer is not None else {}
        draws = [it[0] for it in items if it[1] in (_lib.MRGS_RESET_JITTER, _lib.MRGS_RESET_JITTER_CONST)]
        if torch.is_tensor(noise):
            if len(draws) != 1:
                raise ValueError("GaussianModel: a single noise tensor serves a single drawing group; pass {group name: tensor}")
            noise = {draws[0]: noise}
        noise = dict(noise or {})
        unknown = set(noise) - set(draws)
        if unknown:
            raise ValueError(f"GaussianModel: noise given for {sorted(unknown)}, which draw nothing in this call")
        seed = densify.draw_seed(seed, needed=any(d not in noise for d in draws))
        masks = []
        for t, what in ((self._refl_strength, "_refl_strength"), (self._roughness, "_roughness")):
            t = densify.device_f32(t, what, (P, 1), who="model").detach().contiguous()
            if t.device != dev:
                raise ValueError(f"GaussianModel: {what} does not share the device with xyz")
            masks.append(t)
        refl, rough = masks
        arr = (_lib.MrgsResetItem * len(items))()
        groups, slots, out, hold = [], [], [], []
        for i, (name, rule, keep, a, b) in enumerate(items):
            g = by_name.get(name)
            if g is None and moments:
                raise ValueError(f"GaussianModel: the optimizer has no '{name}' group (call training_setup first)")
            p = g["params"][0] if g is not None else getattr(self, densify.group_attr(name))      # without an optimizer: the attribute
            src = densify.device_f32(p, f"parameter '{name}'", who="model").detach().contiguous()
            if src.dim() < 2 or src.shape[0] != P or src.device != dev:
                raise ValueError(f"GaussianModel: parameter '{name}' does not share dim 0 / the device with xyz")
            if excl is None:
                keep &= ~_lib.MRGS_RESET_KEEP_EXCLUSIVE
            dst = torch.empty_like(src)
            groups.append(g); slots.append((g, "param")); out.append(dst)
            st = optimizer.state.get(p, None) if moments else None
            m = v = None
            if st is not None and "exp_avg" in st:
                m, v = torch.empty_like(src), torch.empty_like(src)
                slots += [(g, "exp_avg"), (g, "exp_avg_sq")]; out += [m, v]
            u = noise.get(name)
            if u is not None:
                u = densify.device_f32(u, f"noise for '{name}'", src.shape, who="model").contiguous()
                if u.device != dev:
                    raise ValueError(f"GaussianModel: noise for '{name}' does not share the device with xyz")
            hold += [src, u]
            arr[i] = _lib.MrgsResetItem(src.data_ptr(), dst.data_ptr(), _lib.ptr(m), _lib.ptr(v), _lib.ptr(u), int(src.numel() // max(P, 1)) or 1,
                                        rule, keep, 0, float(a), float(b))
        cfg = _lib.MrgsResetConfig(P, refl.data_ptr(), rough.data_ptr(), _lib.ptr(excl), float(self.refl_msk_thr), float(self.rough_msk_thr), seed)
        with _lib.guard(dev):
            _lib.check(_lib.lib().mrgs_model_reset(ctypes.byref(cfg), arr, len(items), _lib.stream_ptr(dev)))
        return groups, slots, out

    def _reset(self, items, exclusive_msk=None, seed=None, noise=None):
        """_launch_reset, then the new parameters and zeroed moments go into the optimizer and the model; returns {group name: parameter}."""
        groups, slots, out = self._launch_reset(items, exclusive_msk, seed, noise)
        new = densify._install(self.optimizer, groups, slots, out)
        self._rebind(new)
        return new

    _EXCL, _ABOVE, _BELOW, _ROUGH = (_lib.MRGS_RESET_KEEP_EXCLUSIVE, _lib.MRGS_RESET_KEEP_REFL_ABOVE, _lib.MRGS_RESET_KEEP_REFL_BELOW,
                                     _lib.MRGS_RESET_KEEP_ROUGH_ABOVE)

    def _item_opacity0(self):
        return ("opacity", _lib.MRGS_RESET_CAP, 0, 0.01, 0.0)

    def _item_opacity1(self):
        return ("opacity", _lib.MRGS_RESET_LIFT, self._EXCL, 0.9, 0.0)

    def _item_refl(self, rst_value=None):
        return ("refl_strength", _lib.MRGS_RESET_FLOOR, self._EXCL, self.init_refl_value if rst_value is None else rst_value, 0.0)

    def _item_jitter(self, group):
        return (group, _lib.MRGS_RESET_JITTER, self._EXCL | self._ABOVE, 0.4, 0.0)

    def _item_scale(self):
        return ("scaling", _lib.MRGS_RESET_ENLARGE, self._EXCL | self._BELOW | self._ROUGH, self.enlarge_scale, 0.0)

    def reset_opacity0(self):
        self._reset([self._item_opacity0()])

    def reset_opacity1(self, exclusive_msk=None):
        self._reset([self._item_opacity1()], exclusive_msk)

    def reset_refl(self, exclusive_msk=None, rst_value=None):
        self._reset([self._item_refl(rst_value)], exclusive_msk)

    def reset_refl_strength(self, reset_value=0.01):
        self._reset([("refl_strength", _lib.MRGS_RESET_CONST, 0, reset_value, 0.0)])

    def reset_refl_strength2(self, reset_value=0.1):
        self._reset([("refl_strength", _lib.MRGS_RESET_FLOOR, 0, reset_value, 0.0)])

    def reset_roughness(self, reset_value=0.1):
        self._reset([("roughness", _lib.MRGS_RESET_CONST, 0, reset_value, 0.0)])

    def reset_ori_color(self, reset_value=0.5, noise_level=0.05, *, seed=None, noise=None):
        self._reset([("ori_color", _lib.MRGS_RESET_JITTER_CONST, 0, reset_value, noise_level)], seed=seed, noise=noise)

    def reset_features(self, reset_value_dc=0.0, reset_value_rest=0.0):
        self._reset([("f_dc", _lib.MRGS_RESET_FILL, 0, reset_value_dc, 0.0), ("f_rest", _lib.MRGS_RESET_FILL, 0, reset_value_rest, 0.0)])
        self.active_sh_degree = 0

    def dist_color(self, exclusive_msk=None, *, seed=None, noise=None):
        self._reset([self._item_jitter("f_dc")], exclusive_msk, seed, noise)

    def dist_albedo(self, exclusive_msk=None, *, seed=None, noise=None):
        self._reset([self._item_jitter("ori_color")], exclusive_msk, seed, noise)

    def reset_scale(self, exclusive_msk=None):
        self._reset([self._item_scale()], exclusive_msk)

    def enlarge_refl_scales(self, ret_raw=True, ENLARGE_SCALE=1.5, REFL_MSK_THR=0.02, ROUGH_MSK_THR=0.1, exclusive_msk=None):
        """The enlarged scales without installing them: raw (ret_raw) or activated.  The three keyword values are ignored in favour of the
        model's enlarge_scale, refl_msk_thr and rough_msk_thr, as in the reference.  reset_scale's launch with the same checks, nothing installed."""
        _groups, _slots, (dst,) = self._launch_reset([self._item_scale()], exclusive_msk, moments=False)
        return dst if ret_raw else torch.exp(dst)

    # ---- the blocks of the training loops, one launch each --------------------------------------------------------------------------
    def normal_propagation_step(self, exclusive_msk=None, dist_color=True, *, seed=None, noise=None):
        """reset_opacity1 + dist_color (when `dist_color`) + reset_scale (train_refnerf.py:1450-1455)."""
        items = [self._item_opacity1()] + ([self._item_jitter("f_dc")] if dist_color else []) + [self._item_scale()]
        self._reset(items, exclusive_msk, seed, noise)

    def opacity_reset_step(self, exclusive_msk=None, rst_value=None):
        """reset_opacity0 + reset_refl (train_refnerf.py:1439-1443)."""
        self._reset([self._item_opacity0(), self._item_refl(rst_value)], exclusive_msk)

    def material_reset_step(self, init_roughness_value, features=False, *, seed=None, noise=None):
        """reset_ori_color + reset_refl_strength(0.1) + reset_roughness(init_roughness_value), and reset_features with `features`:
        reset_gaussian_para / reset_gaussian_para2 of the training scripts (train_refnerf.py:1516-1531), whose two threshold assignments
        (refl_msk_thr, rough_msk_thr) stay with the caller."""
        items = [("ori_color", _lib.MRGS_RESET_JITTER_CONST, 0, 0.5, 0.05), ("refl_strength", _lib.MRGS_RESET_CONST, 0, 0.1, 0.0),
                 ("roughness", _lib.MRGS_RESET_CONST, 0, init_roughness_value, 0.0)]
        if features:
            items += [("f_dc", _lib.MRGS_RESET_FILL, 0, 0.0, 0.0), ("f_rest", _lib.MRGS_RESET_FILL, 0, 0.0, 0.0)]
        self._reset(items, seed=seed, noise=noise)
        if features:
            self.active_sh_degree = 0

    # ---- left out ---------------------------------------------------------------------------------------------------------------
    reset_specular = _left_out("reset_specular", "a no-op in the reference (it asks the optimizer for a group named 'metallness', which does "
                               "not exist, so nothing is replaced); not built")
    _UNCALLED = "no training script of the reference calls it; not built"
    reset_opacity1_strategy2 = _left_out("reset_opacity1_strategy2", _UNCALLED)
    dist_rot = _left_out("dist_rot", _UNCALLED)
    dist_color2_specular = _left_out("dist_color2_specular", _UNCALLED)
    enlarge_refl_scales2 = _left_out("enlarge_refl_scales2", _UNCALLED)
    reset_scale2_specular = _left_out("reset_scale2_specular", _UNCALLED)
    _NATIVE = "its only callers are native here ({}) and do not go through the model; not built"
    get_points_from_depth = _left_out("get_points_from_depth", _NATIVE.format("multiview.calc_warp_loss"))
    get_points_depth_in_depth_map = _left_out("get_points_depth_in_depth_map", _NATIVE.format("multiview.calc_warp_loss"))
    get_triangles = _left_out("get_triangles", _NATIVE.format("surfel_tracing.SurfelTracer"))
