"""Optimizer of the training loop: `Adam` is a drop-in for the `torch.optim.Adam(l, lr=0.0, eps=1e-15)` that
GaussianModel.training_setup builds (scene/gaussian_model.py:417-453).  Same constructor, `param_groups` and per-parameter
`state` keys ("step", "exp_avg", "exp_avg_sq"), so the reference's densification helpers that edit the optimizer in place
(`replace_tensor_to_optimizer`, `_prune_optimizer`, `cat_tensors_to_optimizer`, gaussian_model.py:866-960) and its checkpoints
(`optimizer.state_dict()` inside chkpnt*.pth) keep working.  `step()` updates every parameter tensor of every group with ONE
kernel launch (csrc/mrgs_optim.hip) instead of 6-8 elementwise passes per tensor; CPU parameters raise (no fallback).

`SparseAdam` is the same optimizer with `step(visibility=...)`: the per-gaussian groups are stepped only in the rows a view touched
(`mrgs_adam_step_rows`); every other row keeps its parameters and both moments bit for bit."""
import ctypes

import torch

from . import _lib
from .densify import SKIP_GROUPS


def _check_param(p):
    if not p.is_cuda:
        raise RuntimeError("materialrefgs_amd.optim.Adam updates device tensors only (libmrgs.so has no CPU path)")
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError("Adam: parameters must be contiguous fp32 tensors")
    if p.grad.is_sparse:
        raise RuntimeError("Adam does not support sparse gradients")


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("the reference trains with weight_decay=0, amsgrad=False; nothing else is built")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))

    def _gather(self):
        """Every parameter that has a gradient, with its state created and its step count advanced:
        {(device, beta1, beta2, eps): [(group, p, g, m, v, lr, step), ...]}."""
        by_key = {}
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check_param(p)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = int(st["step"]) + 1
                if torch.is_tensor(st["step"]):
                    st["step"].fill_(step)
                else:
                    st["step"] = step
                g = p.grad if (p.grad.dtype == torch.float32 and p.grad.is_contiguous()) else p.grad.float().contiguous()
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous() and m.dtype == torch.float32 and v.dtype == torch.float32):
                    raise RuntimeError("Adam: optimizer state must be contiguous fp32")
                key = (p.device, float(beta1), float(beta2), float(group["eps"]))
                by_key.setdefault(key, []).append((group, p, g, m, v, float(group["lr"]), step))
        return by_key

    @staticmethod
    def _step_dense(key, items):
        """mrgs_adam_step over `items` of _gather (one launch per MRGS_ADAM_MAX_TENSORS tensors)."""
        if not items:
            return
        dev, beta1, beta2, eps = key
        arr = (_lib.MrgsAdamTensor * len(items))()
        for i, (_, p, g, m, v, lr, step) in enumerate(items):
            arr[i] = _lib.MrgsAdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, step)
        with _lib.guard(dev):
            stream = _lib.stream_ptr(dev)
            _lib.check(_lib.lib().mrgs_adam_step(arr, len(items), beta1, beta2, eps, stream))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        by_key = self._gather()
        for key, items in by_key.items():
            self._step_dense(key, items)
            del items          # the gradient copies (if any) stay alive until the launch is queued on the same stream
        return loss


def _as_masks(visibility):
    """`visibility` of SparseAdam.step as a list of at most MRGS_ADAM_ROWS_MAX_MASKS contiguous one-byte tensors of one length and
    device (bool storage is the bytes the kernel reads); more are ORed into the last one with torch first."""
    masks = [visibility] if torch.is_tensor(visibility) else list(visibility)
    if not masks:
        raise ValueError("SparseAdam.step: visibility is an empty sequence (pass None for the dense step)")
    for m in masks:
        if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"SparseAdam.step: a visibility mask must be a bool or uint8 tensor, got {getattr(m, 'dtype', type(m))}")
        if m.dim() != 1 or m.shape != masks[0].shape:
            raise ValueError(f"SparseAdam.step: visibility masks must be [P] and of one length, got {[tuple(x.shape) for x in masks]}")
        if m.device != masks[0].device:
            raise ValueError("SparseAdam.step: visibility masks must be on one device")
    masks = [m.contiguous() for m in masks]
    if len(masks) > _lib.MRGS_ADAM_ROWS_MAX_MASKS:
        last = masks[_lib.MRGS_ADAM_ROWS_MAX_MASKS - 1].view(torch.uint8).clone()
        for m in masks[_lib.MRGS_ADAM_ROWS_MAX_MASKS:]:
            last |= m.view(torch.uint8)
        masks = masks[:_lib.MRGS_ADAM_ROWS_MAX_MASKS - 1] + [last]
    return masks


class SparseAdam(Adam):
    """`Adam` whose `step(visibility=mask)` updates, in every per-gaussian group, only the rows with a non-zero mask byte: the rows
    the view of this iteration touched (`render_pkg["visibility_filter"]`).  An invisible row keeps `param`, `exp_avg` and `exp_avg_sq`
    bit for bit -- no decaying-momentum drift for surfels no camera is looking at --, a visible row gets exactly `Adam`'s update with
    the tensor's own step count, which advances on every call in which the parameter has a gradient (one count per parameter, the
    state keys of `Adam`: state dicts and checkpoints are interchangeable, a run can switch classes at any iteration).
    bias_correction=False: step_size = lr and no correction of the second moment in the MASKED groups (the plain rule of the 3DGS code
    base's sparse optimizer).  The groups named in `dense_groups` (not per-gaussian: the MLP and the environment maps) are always
    stepped like `Adam` does, in the same call; so is everything when `visibility` is None."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, bias_correction=True, dense_groups=SKIP_GROUPS):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self.bias_correction = bool(bias_correction)
        self.dense_groups = tuple(dense_groups)

    @torch.no_grad()
    def step(self, closure=None, visibility=None):
        if visibility is None:
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        masks = _as_masks(visibility)
        P = int(masks[0].shape[0])
        # everything that can be refused is refused here: _gather advances the step counts
        live = [(group.get("name"), p) for group in self.param_groups for p in group["params"] if p.grad is not None]
        for name, p in live:
            if name not in self.dense_groups and (p.dim() == 0 or p.shape[0] != P):
                raise ValueError(f"SparseAdam.step: group {name!r} holds a parameter of shape {tuple(p.shape)}, the visibility mask has "
                                 f"{P} rows (groups that are not per-gaussian belong in dense_groups={self.dense_groups})")
        for name, p in live:
            _check_param(p)
            if name not in self.dense_groups and p.device != masks[0].device:
                raise ValueError(f"SparseAdam.step: the visibility mask is on {masks[0].device}, group {name!r} on {p.device}")
        mask_ptrs = (ctypes.c_void_p * len(masks))(*[m.data_ptr() for m in masks])
        lib = _lib.lib()
        for key, items in self._gather().items():
            dev, beta1, beta2, eps = key
            dense = [it for it in items if it[0].get("name") in self.dense_groups]
            rows = [it for it in items if it[0].get("name") not in self.dense_groups and it[1].numel() > 0]
            self._step_dense(key, dense)
            if rows:                                    # (P == 0: every masked tensor is empty)
                arr = (_lib.MrgsAdamRowsTensor * len(rows))()
                for i, (_, p, g, m, v, lr, step) in enumerate(rows):
                    arr[i] = _lib.MrgsAdamRowsTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), p.numel() // P, lr, step, 0)
                with _lib.guard(dev):
                    stream = _lib.stream_ptr(dev)
                    _lib.check(lib.mrgs_adam_step_rows(arr, len(rows), P, mask_ptrs, len(masks), int(self.bias_correction), beta1, beta2, eps, stream))
            del items, dense, rows
        return loss


def default_optimizer_cls(training_args):
    """The class the training_setup functions build when none is passed: SparseAdam for training_args.optimizer_type == "sparse_adam"
    (the 3DGS code base's switch), Adam otherwise -- an absent attribute included."""
    return SparseAdam if getattr(training_args, "optimizer_type", "default") == "sparse_adam" else Adam
