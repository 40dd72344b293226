"""EnvGaussianModel: the second surfel set that the last training stage traces every pixel's mirror ray through (the reference's
scene/env_gaussian_model.py), with its per-gaussian policy on csrc/mrgs_env_densify.hip: `add_densification_stats` is one in-place launch
without a host read, `densify_and_prune` -- clone, split in 2, opacity prune, quantile-of-weights prune with split in 5, top-k visibility
cap, reset -- classify passes over per-row numbers and ONE emit pass with ONE host read.  Attribute names and activations are the
reference's, so surfel_tracing._raw_model takes its fast path.  No CPU path and no torch fallback: the tensors must live on the GPU.
env_point_cloud.ply is written and read by the module functions `save_ply(model, path)` / `load_ply(model, path)` below (on
materialrefgs_amd.io); the class itself still has no methods of those names.  Left out: env_gaussian_model3.py.
Differences from the reference are listed in INTEGRATION.md section 4e."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _lib, densify
from .gs_utils import RGB2SH, build_scaling_rotation, flip_align_view, safe_normalize

GROUP_ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
               "rotation": "_rotation"}
STATS = ("xyz_gradient_accum", "xyz_weight_accum", "denom", "max_radii2D")
_SLOTS = ("original", "clone", "child0", "child1")


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The xyz schedule: log-linear from lr_init to lr_final over max_steps, eased in by a sine over lr_delay_steps when that is > 0."""
    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return rate


def _device_f32(t, what, shape=None):
    return densify.device_f32(t, what, shape, who="env_model")


def select_kth(values, k):
    """The radix select of the two selections, on its own: (k-th smallest of the device fp32 vector `values` (k from 0), how many values
    are smaller, how many are equal).  One host read."""
    v = _device_f32(values, "values").contiguous().reshape(-1)
    n, k = int(v.numel()), int(k)
    if not 0 <= k < max(n, 1):
        raise ValueError("select_kth: k must be in [0, n)")
    if n == 0:
        raise ValueError("select_kth: no values")
    lib, dev = _lib.lib(), v.device
    with _lib.guard(dev):
        ws = torch.empty(lib.mrgs_env_select_ws_bytes(), dtype=torch.uint8, device=dev)
        out = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.mrgs_env_select(n, v.data_ptr(), k, ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream_ptr(dev)))
        host = out.cpu()
    return float(host[:1].view(torch.float32)[0]), int(host[1]), int(host[2])


def add_densification_stats(accum, denom, weight_accum, grad, update_filter, weight_accumulate=None):
    """For rows with the filter set: accum += ||grad[0:3]||_2, denom += 1, weight_accum += weight_accumulate (skipped when None).  In
    place, one launch, nothing read back."""
    P, grad, vis = densify.stats_args(grad, update_filter, ((accum, "xyz_gradient_accum"), (denom, "denom"), (weight_accum, "xyz_weight_accum")),
                                      who="env_model")
    dev = grad.device
    if weight_accumulate is not None:
        weight_accumulate = _device_f32(weight_accumulate, "weight_accumulate").detach().contiguous()
        if weight_accumulate.numel() != P:
            raise ValueError("add_densification_stats: weight_accumulate must hold one value per row")
    with _lib.guard(dev):
        _lib.check(_lib.lib().mrgs_env_densify_stats(P, grad.data_ptr(), vis.data_ptr(), _lib.ptr(weight_accumulate), accum.data_ptr(),
                                                     denom.data_ptr(), weight_accum.data_ptr(), _lib.stream_ptr(dev)))


def _counts(raw):
    f32 = lambda bits: float(np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
    seg = raw[:24]
    return SimpleNamespace(rows=raw[24], segments=tuple(seg), kept=dict(zip(_SLOTS, seg[:4])), children5=sum(seg[4:]), n_clone=raw[25],
                           n_split=raw[26], n_stage3=raw[27], n_pruned4=raw[28], n_split4=raw[29], n_pruned5=raw[30], q=f32(raw[31]),
                           W0=f32(raw[32]), W1=f32(raw[33]), W4=f32(raw[34]), cut=f32(raw[35]), rows_before_cap=raw[36], capped=bool(raw[37]))


def save_ply(model, path):
    """EnvGaussianModel.save_ply (scene/env_gaussian_model.py:212-229; Scene.save writes env_point_cloud.ply with it) as a function of the
    model: the class has no method of this name (tests/test_env_model.py holds it to that)."""
    from . import io
    io.save_env_ply(path, {"xyz": model._xyz, "features_dc": model._features_dc, "features_rest": model._features_rest, "opacity": model._opacity,
                           "scaling": model._scaling, "rotation": model._rotation})


def load_ply(model, path, device="cuda"):
    """EnvGaussianModel.load_ply (:236-277) as a function of the model: the parameters on `device` with requires_grad, active_sh_degree =
    max_sh_degree."""
    from . import io
    t = io.load_env_ply(path, model.max_sh_degree, device)
    for key, attr in (("xyz", "_xyz"), ("features_dc", "_features_dc"), ("features_rest", "_features_rest"), ("opacity", "_opacity"),
                      ("scaling", "_scaling"), ("rotation", "_rotation")):
        setattr(model, attr, nn.Parameter(t[key].requires_grad_(True)))
    model.active_sh_degree = model.max_sh_degree


class EnvGaussianModel:
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
        self.rotation_activation = torch.nn.functional.normalize

    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity") + STATS:
            setattr(self, name, torch.empty(0))
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.start_iter = 0
        self.max_gs = 2e6
        self.max_gs_threshold = 0.9
        self.setup_functions()

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
                self.max_radii2D, self.xyz_gradient_accum, self.xyz_weight_accum, self.denom, self.optimizer.state_dict(), self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
         self.max_radii2D, xyz_gradient_accum, xyz_weight_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        self.training_setup(training_args)
        self.xyz_gradient_accum, self.xyz_weight_accum, self.denom = xyz_gradient_accum, xyz_weight_accum, denom
        self.optimizer.load_state_dict(opt_dict)

    @torch.no_grad()
    def restore_from_refgs(self, model_args, opt, anchored_lst=[]):
        """From the 22-tuple of GaussianModel.capture(): geometry, colour SH and metalness are taken over, the optimizer is new."""
        (self.active_sh_degree, self._xyz, _refl, self._metalness, _rough, _ori, _diffuse, self._features_dc, self._features_rest, _ind_dc, _ind_rest,
         _ind_asg, self._scaling, self._rotation, self._opacity, _n1, _n2, self.max_radii2D, xyz_gradient_accum, _denom, _opt_dict,
         self.spatial_lr_scale) = model_args
        self.training_setup(opt, anchored_lst=anchored_lst)
        self.max_radii2D = torch.zeros((self.get_xyz.shape[0]), device=self._xyz.device)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.start_iter = 12500

    # ---- getters ----------------------------------------------------------------------------------------------------------------
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_xyz_weight_avg(self):
        avg = self.xyz_weight_accum / self.denom
        avg[avg.isnan()] = 0.0
        return avg

    def get_xyz_gradient_avg(self):
        avg = self.xyz_gradient_accum / self.denom
        avg[avg.isnan()] = 0.0
        return avg

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_xyz, self.get_scaling, scaling_modifier, self._rotation)

    def get_normal(self, scaling_modifier, dir_pp_normalized):
        """The surfel's third axis, flipped towards the viewer (no `return_delta`: the reference's reads attributes this class does not have)."""
        normals_raw, _positive = flip_align_view(self.get_covariance(scaling_modifier)[:, 2, :3], dir_pp_normalized)
        return safe_normalize(normals_raw)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- set-up -----------------------------------------------------------------------------------------------------------------
    def create_from_pcd(self, pcd, spatial_lr_scale: float, device="cuda"):
        from .knn import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        points = torch.tensor(np.asarray(pcd.points)).float().to(device)
        color = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().to(device))
        n = points.shape[0]
        features = torch.zeros((n, 3, (self.max_sh_degree + 1) ** 2), device=points.device)
        features[:, :3, 0] = color
        print("Number of points at initialisation : ", n)
        dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 2)
        rots = torch.rand((n, 4), device=points.device)
        opacities = self.inverse_opacity_activation(0.1 * torch.ones((n, 1), dtype=torch.float, device=points.device))
        self._xyz = nn.Parameter(points.requires_grad_(True))
        self._features_dc = nn.Parameter(features[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(features[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opacities.requires_grad_(True))
        self.max_radii2D = torch.zeros((n,), device=points.device)

    def training_setup(self, training_args, lr_downfactor_geo=5., anchored_lst=[]):
        from .optim import default_optimizer_cls
        self.percent_dense = 0.01                      # the reference fixes it here, whatever training_args.percent_dense says
        n, dev = self.get_xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.xyz_weight_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        groups = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.features_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.features_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
        ]
        self.optimizer = default_optimizer_cls(training_args)(groups, lr=0.0, eps=1e-15)     # optimizer_type == "sparse_adam": SparseAdam
        self.xyz_scheduler_args = expon_lr_func(lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                                                lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                                                lr_delay_mult=training_args.position_lr_delay_mult, max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = self.xyz_scheduler_args(iteration)
                return group["lr"]

    # ---- the per-gaussian policy ------------------------------------------------------------------------------------------------------
    def reset_opacity(self):
        opacities_new = self.inverse_opacity_activation(torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01))
        self._opacity = densify.replace_tensor_to_optimizer(self.optimizer, opacities_new, "opacity")["opacity"]

    def reset_stats(self):
        n, dev = self.get_xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)
        self.xyz_weight_accum = torch.zeros((n, 1), device=dev)

    def prune_points(self, mask):
        tensors, extra = densify.prune_optimizer(self.optimizer, ~mask, extra=[getattr(self, s) for s in STATS])
        for name, p in tensors.items():
            setattr(self, GROUP_ATTRS[name], p)
        for s, t in zip(STATS, extra):
            setattr(self, s, t)

    def add_densification_stats(self, viewspace_point_tensor, update_filter, weight_accumulate=None):
        grad = viewspace_point_tensor.grad if viewspace_point_tensor.grad is not None else viewspace_point_tensor
        if grad.requires_grad:
            raise RuntimeError("add_densification_stats: viewspace_point_tensor has no .grad yet (call it after backward())")
        add_densification_stats(self.xyz_gradient_accum, self.denom, self.xyz_weight_accum, grad, update_filter, weight_accumulate)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size=None, split_screen_threshold=None, *, seed=None, noise=None,
                          noise4=None):
        """The six-stage chain (include/mrgs.h states it) with ONE host read.  Rebinds the six parameters, the optimizer's groups and state
        and the four statistics (zero, new length); returns the counts (rows, per-segment rows, what each stage did, q, W0, W1, W4).
        seed: 64-bit key of the counter generator for both generations of offsets; None draws it from torch's CPU default generator.
        noise [P,2,2] / noise4 [P,4,5,2]: device fp32 standard normals indexed by SOURCE row (and slot), used instead of the generator."""
        if split_screen_threshold is not None:
            raise NotImplementedError("EnvGaussianModel.densify_and_prune: split_screen_threshold is None in the reference's only call; "
                                      "no other value is served")
        max_grad, min_opacity, extent = float(max_grad), float(min_opacity), float(extent)
        if not max_grad > 0.0:
            raise ValueError("densify_and_prune: max_grad must be > 0")
        optimizer = self.optimizer
        groups = list(optimizer.param_groups)
        if [g["name"] for g in groups] != list(GROUP_ATTRS):
            raise ValueError("densify_and_prune: the optimizer must hold the six groups of training_setup")
        P = int(self._xyz.shape[0])
        dev = self._xyz.device
        src, slots, data = densify.emit_sources(optimizer, groups, P, dev, who="env_model")
        xyz, scaling, rotation, opacity = data["xyz"], data["scaling"], data["rotation"], data["opacity"]
        stats = []
        for s in STATS:
            t = _device_f32(getattr(self, s), s).contiguous()
            if t.numel() != P:
                raise ValueError(f"densify_and_prune: {s} must hold one value per row")
            stats.append(t)
        accum, weight, denom, radii = stats
        if noise is not None:
            noise = _device_f32(noise, "noise", (P, 2, 2)).contiguous()
        if noise4 is not None:
            noise4 = _device_f32(noise4, "noise4", (P, 4, 5, 2)).contiguous()
        seed = densify.draw_seed(seed, needed=noise is None or noise4 is None)
        raw = [0] * _lib.MRGS_ENV_DENSIFY_COUNTS
        if P > 0:
            lib = _lib.lib()
            flags = _lib.MRGS_ENV_DENSIFY_SCREEN if max_screen_size is not None else 0
            cfg = _lib.MrgsEnvDensifyConfig(flags, P, int(self.max_gs * self.max_gs_threshold), max_grad, min_opacity,
                                            float(self.percent_dense) * extent, 0.1 * extent, float(max_screen_size or 0.0), 0.0,
                                            xyz.data_ptr(), scaling.data_ptr(), rotation.data_ptr())
            with _lib.guard(dev):
                stream = _lib.stream_ptr(dev)
                ws = torch.empty(lib.mrgs_env_densify_ws_bytes(P), dtype=torch.uint8, device=dev)
                cnt = torch.empty(_lib.MRGS_ENV_DENSIFY_COUNTS, dtype=torch.int64, device=dev)
                _lib.check(lib.mrgs_env_densify_classify(ctypes.byref(cfg), accum.data_ptr(), denom.data_ptr(), radii.data_ptr(), weight.data_ptr(),
                                                         scaling.data_ptr(), opacity.data_ptr(), ws.data_ptr(), ws.numel(), cnt.data_ptr(), stream))
                raw = [int(c) for c in cnt.tolist()]                       # the one host read of the whole operation
                new = densify.emit_and_install(optimizer, groups, src, slots, raw[24], lambda arr, n: lib.mrgs_env_densify_emit(
                    ctypes.byref(cfg), ws.data_ptr(), raw[24], arr, n, seed, _lib.ptr(noise), _lib.ptr(noise4), stream))
            for name, p in new.items():
                setattr(self, GROUP_ATTRS[name], p)
        self.reset_stats()
        return _counts(raw)

    @torch.no_grad()
    def update_env_gs(self, iter, opt, scene, render_pkg):
        """One iteration of the environment set's policy: the learning rate, the SH degree every 1000 iterations, the statistics of every
        traced iteration and densify_and_prune every 500, all of it ending at iteration 21000."""
        env_densify_until_iter = 24000
        env_densify_inter = 500
        env_opacity_reset_inter = 6000
        env_densify_grad_thres = 1e-4 / 2
        env_min_opacity = 0.05
        size_threshold = 20 if iter > env_opacity_reset_inter else None
        screen_threshold = None

        self.update_learning_rate(iter - self.start_iter)
        if iter > 0 and iter % 1000 == 0:
            self.oneupSHdegree()
        if iter >= 21000:
            return
        if iter > 0 and iter < env_densify_until_iter:
            self.add_densification_stats(render_pkg["viewspace_points"], render_pkg["visibility_filter"], render_pkg["weight_accumulate"])
        if iter > 0 and iter < env_densify_until_iter and iter % env_densify_inter == 0:
            print("Before Densify f{:06d}: {:06d} points".format(iter, self.get_xyz.shape[0]))
            self.densify_and_prune(max_grad=env_densify_grad_thres, min_opacity=env_min_opacity, extent=scene.cameras_extent,
                                   max_screen_size=size_threshold, split_screen_threshold=screen_threshold)
            print("After Densify f{:06d}: {:06d} points".format(iter, self.get_xyz.shape[0]))
