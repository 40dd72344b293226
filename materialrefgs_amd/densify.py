"""Row compaction for densify / prune and the optimizer surgery around it, mirroring
GaussianModel._prune_optimizer / prune_points / cat_tensors_to_optimizer / replace_tensor_to_optimizer
(scene/gaussian_model.py:856-960).  `compact_rows` drops the rows of many tensors at once (csrc/mrgs_optim.hip: one scan of the
mask, one host read of the survivor count, one gather launch) where the reference runs `tensor[mask]` ~50 times; the functions
below keep the reference's dictionary-of-named-groups protocol so that its densification logic can call them unchanged.
`densify_and_prune` and `add_densification_stats` (csrc/mrgs_densify.hip) are that logic itself: selection, clone, split with its sampled
offsets and the combined prune in one classify and one emit pass with one host read, and the two per-iteration statistics lines in one
launch with none.  No CPU path: the tensors must live on the GPU."""
import ctypes
from typing import Dict, Iterable, List, Sequence, Tuple

import torch
from torch import nn

from . import _lib

SKIP_GROUPS = ("mlp", "env", "env2")          # not per-gaussian (gaussian_model.py:858, 909)


def compact_rows(tensors: Sequence[torch.Tensor], keep: torch.Tensor) -> Tuple[List[torch.Tensor], int]:
    """[t[keep] for t in tensors] for 4-byte-element tensors sharing their first dimension; returns (new tensors, survivor count)."""
    if len(tensors) == 0:
        return [], int(keep.sum())
    n = int(keep.shape[0])
    dev = keep.device
    if not keep.is_cuda:
        raise RuntimeError("materialrefgs_amd.densify needs device tensors (libmrgs.so has no CPU path)")
    k8 = keep.to(torch.uint8).contiguous()
    src = []
    for t in tensors:
        if t.shape[0] != n or t.element_size() != 4 or t.device != dev:
            raise ValueError("compact_rows: tensors must have 4-byte elements, live on the mask's device and share dim 0 with it")
        src.append(t.detach().contiguous())
    lib = _lib.lib()
    with _lib.guard(dev):
        st = _lib.stream_ptr(dev)
        ws = torch.empty(lib.mrgs_compact_ws_bytes(n), dtype=torch.uint8, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.mrgs_compact_count(n, ctypes.c_void_p(k8.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                          ctypes.c_void_p(cnt.data_ptr()), st))
        m = int(cnt.item())                                    # the one host read of the whole operation
        out = [torch.empty((m,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in src]
        arr = (_lib.MrgsCompactTensor * len(src))()
        for i, (s, d) in enumerate(zip(src, out)):
            arr[i] = _lib.MrgsCompactTensor(s.data_ptr(), d.data_ptr(), int(s.numel() // max(n, 1)))
        if m > 0:
            _lib.check(lib.mrgs_compact_rows(n, ctypes.c_void_p(k8.data_ptr()), ctypes.c_void_p(ws.data_ptr()), arr, len(src), st))
    return out, m


def _per_gaussian_groups(optimizer) -> Iterable[dict]:
    for group in optimizer.param_groups:
        if group.get("name") in SKIP_GROUPS:
            continue
        assert len(group["params"]) == 1
        yield group


def prune_optimizer(optimizer, keep: torch.Tensor, extra: Sequence[torch.Tensor] = ()):
    """_prune_optimizer (:856-874) for every per-gaussian group at once.  `extra`: further per-gaussian tensors to compact with the same
    mask (xyz_gradient_accum, denom, max_radii2D of prune_points :900-905).  Returns (optimizable_tensors, compacted extras)."""
    groups = list(_per_gaussian_groups(optimizer))
    tensors, slots = [], []
    for g in groups:
        p = g["params"][0]
        st = optimizer.state.get(p, None)
        tensors.append(p.data); slots.append((g, "param"))
        if st is not None and "exp_avg" in st:
            tensors.append(st["exp_avg"]); slots.append((g, "exp_avg"))
            tensors.append(st["exp_avg_sq"]); slots.append((g, "exp_avg_sq"))
    n_model = len(tensors)
    out, _m = compact_rows(tensors + list(extra), keep)
    return _install(optimizer, groups, slots, out[:n_model]), out[n_model:]


def _install(optimizer, groups, slots, tensors):
    """Put the new tensors (one per slot = (group, "param" | "exp_avg" | "exp_avg_sq", ...)) into the optimizer: a new nn.Parameter per
    group, its state entry re-keyed to it.  Returns {group name: parameter}."""
    new = {}
    for slot, t in zip(slots, tensors):
        new.setdefault(id(slot[0]), {})[slot[1]] = t
    optimizable = {}
    for g in groups:
        old = g["params"][0]
        st = optimizer.state.get(old, None)
        vals = new[id(g)]
        if st is not None:
            if "exp_avg" in vals:
                st["exp_avg"], st["exp_avg_sq"] = vals["exp_avg"], vals["exp_avg_sq"]
            del optimizer.state[old]
        g["params"][0] = nn.Parameter(vals["param"].requires_grad_(True))
        if st is not None:
            optimizer.state[g["params"][0]] = st
        optimizable[g["name"]] = g["params"][0]
    return optimizable


def cat_tensors_to_optimizer(optimizer, tensors_dict: Dict[str, torch.Tensor]):
    """cat_tensors_to_optimizer (:907-929): append rows, zero moments for the new ones."""
    optimizable = {}
    for g in _per_gaussian_groups(optimizer):
        ext = tensors_dict[g["name"]]
        old = g["params"][0]
        st = optimizer.state.get(old, None)
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del optimizer.state[old]
        g["params"][0] = nn.Parameter(torch.cat((old.data, ext), dim=0).requires_grad_(True))
        if st is not None:
            optimizer.state[g["params"][0]] = st
        optimizable[g["name"]] = g["params"][0]
    return optimizable


def replace_tensor_to_optimizer(optimizer, tensor: torch.Tensor, name: str):
    """replace_tensor_to_optimizer (:840-854): new values for one group, moments reset."""
    optimizable = {}
    for g in optimizer.param_groups:
        if g.get("name") == name:
            old = g["params"][0]
            st = optimizer.state.get(old, None)
            if st is not None:
                st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(tensor), torch.zeros_like(tensor)
                del optimizer.state[old]
            g["params"][0] = nn.Parameter(tensor.requires_grad_(True))
            if st is not None:
                optimizer.state[g["params"][0]] = st
            optimizable[name] = g["params"][0]
    return optimizable


# ---- densify_and_prune and the per-iteration statistics (csrc/mrgs_densify.hip) -----------------------------------------------------
# optimizer group name -> GaussianModel attribute, for the sixteen per-gaussian groups of training_setup (gaussian_model.py:422-447);
# any other per-gaussian group maps to "_" + name (group_attr)
GROUP_ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
               "rotation": "_rotation", "refl_strength": "_refl_strength", "ori_color": "_ori_color", "diffuse_color": "_diffuse_color",
               "roughness": "_roughness", "metalness": "_metalness", "normal1": "_normal1", "normal2": "_normal2",
               "ind_dc": "_indirect_dc", "ind_rest": "_indirect_rest", "ind_asg": "_indirect_asg"}
_ROLES = {"xyz": _lib.MRGS_DENSIFY_XYZ, "scaling": _lib.MRGS_DENSIFY_SCALING}


def group_attr(name: str) -> str:
    return GROUP_ATTRS.get(name, "_" + name)


def device_f32(t, what, shape=None, who="densify"):
    """`t` if it is a float32 device tensor (of `shape`); `who`: the module whose name the message carries."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"materialrefgs_amd.{who}: {what} must be a device tensor (libmrgs.so has no CPU path)")
    if t.dtype is not torch.float32:
        raise TypeError(f"materialrefgs_amd.{who}: {what} must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"materialrefgs_amd.{who}: {what} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def emit_sources(optimizer, groups, P, dev, who="densify"):
    """What an emit pass reads, for both models: (src, slots, data) -- every group's parameter and, where the optimizer has stepped, its
    two moments, contiguous; one slot (group, "param" | "exp_avg" | "exp_avg_sq", role) per source; {group name: parameter data}."""
    src, slots, data = [], [], {}
    for g in groups:
        p = g["params"][0]
        device_f32(p, f"parameter '{g['name']}'", who=who)
        if p.shape[0] != P or p.device != dev:
            raise ValueError(f"densify_and_prune: parameter '{g['name']}' does not share dim 0 / the device with xyz")
        src.append(p.detach().contiguous()); slots.append((g, "param", _ROLES.get(g["name"], _lib.MRGS_DENSIFY_COPY)))
        data[g["name"]] = src[-1]
        st = optimizer.state.get(p, None)
        if st is not None and "exp_avg" in st:
            for kind in ("exp_avg", "exp_avg_sq"):
                src.append(device_f32(st[kind], f"{kind} of '{g['name']}'", p.shape, who).contiguous())
                slots.append((g, kind, _lib.MRGS_DENSIFY_MOMENT))
    for name, width in (("xyz", 3), ("scaling", 2), ("rotation", 4), ("opacity", 1)):
        device_f32(data[name], name, (P, width), who)
    return src, slots, data


def draw_seed(seed, needed=True):
    """The 64-bit key of the split offsets' generator; None with `needed` draws it from torch's CPU default generator (no device sync)."""
    if seed is None and needed:
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    return int(seed or 0) & 0xFFFFFFFFFFFFFFFF


def emit_and_install(optimizer, groups, src, slots, m, emit_call):
    """The emit pass of both models: allocates one m-row output per source, hands emit_call(tensors, n_tensors) the MrgsDensifyTensor
    list (it returns the library's status) and puts the outputs into the optimizer.  Returns {group name: parameter}."""
    P, dev = int(src[0].shape[0]), src[0].device
    out = [torch.empty((m,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in src]
    arr = (_lib.MrgsDensifyTensor * len(src))()
    for i, (s, d, slot) in enumerate(zip(src, out, slots)):
        arr[i] = _lib.MrgsDensifyTensor(s.data_ptr(), d.data_ptr(), int(s.numel() // P), slot[2])
    _lib.check(emit_call(arr, len(src)))
    return _install(optimizer, groups, slots, out)


def stats_args(grad, update_filter, stats, who="densify"):
    """The checks both add_densification_stats share.  stats: ((tensor, name), ...), accum first.  Returns (P, grad, filter as uint8)."""
    P = int(stats[0][0].shape[0])
    grad = device_f32(grad, "the view-space gradient", (P, 3), who).contiguous()
    for t, what in stats:
        device_f32(t, what, who=who)
        if t.numel() != P or not t.is_contiguous():
            raise ValueError(f"add_densification_stats: {what} must be a contiguous [P,1] tensor")
    if not update_filter.is_cuda or update_filter.dtype not in (torch.bool, torch.uint8) or tuple(update_filter.shape) != (P,):
        raise ValueError("add_densification_stats: update_filter must be a device bool / uint8 tensor of shape [P]")
    return P, grad, update_filter.contiguous().view(torch.uint8)


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, *, N=2, seed=None, noise=None):
    """GaussianModel.densify_and_prune (gaussian_model.py:1043-1057) in one classify and one emit pass with ONE host read (the three
    counts); put `return densify.densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size)` into the method.

    `model`: any object with the reference's attributes -- optimizer, percent_dense, xyz_gradient_accum, denom, max_radii2D and one
    tensor per per-gaussian optimizer group (GROUP_ATTRS / group_attr; the groups of SKIP_GROUPS are left alone).  Rebinds those
    attributes, the optimizer's param_groups / state (new nn.Parameters, as prune_optimizer does; works before the first step, when
    there are no moments) and the three statistics tensors (zero, new length).  Returns (n_keep, n_clone, n_child): surviving unsplit
    originals, surviving clones, split rows with surviving children; the result holds n_keep + n_clone + N n_child rows in that order,
    children as repeat(N, 1) orders them.  Moments travel with originals and are zero for every new row.

    max_screen_size: only its truth value matters, as in the reference -- truthy adds the world-space term max(s) > 0.1 extent to the
    prune.  The reference's screen-space term `max_radii2D > max_screen_size` reads a vector that densification_postfix has zeroed
    twice by then, so it never fires; it does not here either.
    seed: the 64-bit key of the split offsets' counter generator (Philox4x32-10 over (row, child)); None draws it from torch's CPU
    default generator, so torch.manual_seed governs the call like the reference's torch.normal.  noise: device fp32 [P, N, 2] standard
    normals indexed by SOURCE row, used instead of the generator.  Does not call torch.cuda.empty_cache()."""
    max_grad, min_opacity, extent, N = float(max_grad), float(min_opacity), float(extent), int(N)
    if not max_grad > 0.0:
        raise ValueError("densify_and_prune: max_grad must be > 0 (with max_grad <= 0 the reference would split its own clones)")
    if not 1 <= N <= 8:
        raise ValueError("densify_and_prune: N must be in 1..8")
    if max_screen_size and not extent > 0.0:
        raise ValueError("densify_and_prune: extent must be > 0 when max_screen_size is given")
    optimizer = model.optimizer
    groups = list(_per_gaussian_groups(optimizer))
    names = [g["name"] for g in groups]
    for need in ("xyz", "scaling", "rotation", "opacity"):
        if need not in names:
            raise ValueError(f"densify_and_prune: the optimizer has no '{need}' group")
    for g in groups:
        if not hasattr(model, group_attr(g["name"])):
            raise AttributeError(f"densify_and_prune: group '{g['name']}' is per-gaussian but the model has no attribute {group_attr(g['name'])}")
    by_name = {g["name"]: g["params"][0] for g in groups}
    P = int(by_name["xyz"].shape[0])
    dev = by_name["xyz"].device
    src, slots, data = emit_sources(optimizer, groups, P, dev)
    xyz, scaling, rotation, opacity = data["xyz"], data["scaling"], data["rotation"], data["opacity"]
    accum = device_f32(model.xyz_gradient_accum, "xyz_gradient_accum").contiguous()
    denom = device_f32(model.denom, "denom").contiguous()
    if accum.numel() != P or denom.numel() != P:
        raise ValueError("densify_and_prune: xyz_gradient_accum and denom must hold one value per row")
    if noise is not None:
        noise = device_f32(noise, "noise", (P, N, 2)).contiguous()
    seed = draw_seed(seed, needed=noise is None)
    counts = (0, 0, 0)
    if P > 0:
        lib = _lib.lib()
        cfg = _lib.MrgsDensifyConfig(N, P, max_grad, min_opacity, float(model.percent_dense) * extent, 0.1 * extent if max_screen_size else 0.0,
                                     xyz.data_ptr(), scaling.data_ptr(), rotation.data_ptr())
        with _lib.guard(dev):
            stream = _lib.stream_ptr(dev)
            ws = torch.empty(lib.mrgs_densify_ws_bytes(P), dtype=torch.uint8, device=dev)
            cnt = torch.empty(3, dtype=torch.int64, device=dev)
            _lib.check(lib.mrgs_densify_classify(ctypes.byref(cfg), accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(), opacity.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), cnt.data_ptr(), stream))
            counts = tuple(int(c) for c in cnt.tolist())             # the one host read of the whole operation
            host = (_lib.c_int64 * 3)(*counts)
            new = emit_and_install(optimizer, groups, src, slots, counts[0] + counts[1] + N * counts[2], lambda arr, n: lib.mrgs_densify_emit(
                ctypes.byref(cfg), ws.data_ptr(), host, arr, n, seed, _lib.ptr(noise), stream))
        for name, p in new.items():
            setattr(model, group_attr(name), p)
    rows = counts[0] + counts[1] + N * counts[2]
    model.xyz_gradient_accum = torch.zeros((rows, 1), device=dev)
    model.denom = torch.zeros((rows, 1), device=dev)
    model.max_radii2D = torch.zeros((rows,), device=dev)
    return counts


def add_densification_stats(model_or_tensors, viewspace_point_tensor, update_filter, radii=None):
    """The two per-iteration statistics lines of the training loops in one in-place launch without a host read:
        model.add_densification_stats(viewspace_point_tensor, visibility_filter)                  (gaussian_model.py:1059-1061)
        model.max_radii2D[visibility_filter] = max(model.max_radii2D[visibility_filter], radii[visibility_filter])
    For rows with the filter set: xyz_gradient_accum += the 2-norm of ALL THREE columns of the view-space gradient (the reference's
    line; upstream 2DGS takes two), denom += 1, max_radii2D = max(max_radii2D, radii).  radii=None leaves max_radii2D alone.
    model_or_tensors: a model with those three attributes or a tuple (xyz_gradient_accum, denom[, max_radii2D]).
    viewspace_point_tensor: the tensor whose .grad [P,3] is read (a tensor without one is taken as the gradient itself);
    update_filter: bool or uint8 [P] (the render's "visibility_filter"); radii: int32 [P]."""
    if isinstance(model_or_tensors, (tuple, list)):
        accum, denom = model_or_tensors[0], model_or_tensors[1]
        max_radii = model_or_tensors[2] if len(model_or_tensors) > 2 else None
    else:
        accum, denom = model_or_tensors.xyz_gradient_accum, model_or_tensors.denom
        max_radii = getattr(model_or_tensors, "max_radii2D", None)
    grad = viewspace_point_tensor.grad if viewspace_point_tensor.grad is not None else viewspace_point_tensor
    if grad.requires_grad:
        raise RuntimeError("add_densification_stats: viewspace_point_tensor has no .grad yet (call it after backward())")
    P, grad, vis = stats_args(grad, update_filter, ((accum, "xyz_gradient_accum"), (denom, "denom")))
    dev = grad.device
    if radii is not None:
        if max_radii is None:
            raise ValueError("add_densification_stats: radii given but there is no max_radii2D to update")
        device_f32(max_radii, "max_radii2D", (P,))
        if not radii.is_cuda or radii.dtype is not torch.int32 or tuple(radii.shape) != (P,) or not max_radii.is_contiguous():
            raise ValueError("add_densification_stats: radii must be a device int32 tensor of shape [P] and max_radii2D contiguous")
        radii = radii.contiguous()
    with _lib.guard(dev):
        _lib.check(_lib.lib().mrgs_densify_stats(P, grad.data_ptr(), vis.data_ptr(), _lib.ptr(radii), accum.data_ptr(), denom.data_ptr(),
                                                 _lib.ptr(max_radii) if radii is not None else None, _lib.stream_ptr(dev)))
