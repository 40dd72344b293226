"""LPIPS with the VGG16 backbone (lpipsPyTorch/modules: networks.py:88-96, lpips.py:30-36, utils.py:6-8), the perceptual term that
utils/loss_utils.py:209-212 adds from iteration 18 000 on and the third metric of eval.py:52.  All pixel work runs in libmrgs.so
(csrc/mrgs_lpips.hip; the contract is in include/mrgs.h): thirteen 3 x 3 convolutions on the fp32 matrix instructions, the 2 x 2 maxima,
the normalised weighted distance of the five taps, and the gradient to the first image.  There is no torch fallback in this module: the
images must be fp32 device tensors.

The pretrained weights are downloads and are not part of this build; `LPIPS.load` takes them from files the user supplies (torchvision's
vgg16 state dict and the `lpips` package's vgg.pth), `LPIPS.random(seed)` gives a seeded stand-in for tests and timing.

Difference to torch: a pixel whose feature vector is all zero in either image contributes 0 and gets gradient 0 (torch's sqrt backward
gives NaN there).
"""
import ctypes
import re
import weakref

import torch

from . import _lib

_p = _lib.ptr
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)        # the convolutions inside torchvision's vgg16().features
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
CONV_STAGE = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)                 # a 2 x 2 maximum where the stage changes
TAP_CONV = (1, 3, 6, 9, 12)                                          # the taps: ReLU outputs of these convolutions
LEVEL_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 16


def random_weights(seed):
    """The seeded stand-in network: He-scaled convolutions, small biases, non-negative lin weights, drawn in float64 from a CPU generator
    and rounded once to float32 (so a float64 statement built from them states the same network)."""
    g = torch.Generator().manual_seed(int(seed))
    conv_w = [(torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float() for ci, co in CONV_CHANNELS]
    conv_b = [(0.05 * torch.randn(co, generator=g, dtype=torch.float64)).float() for _, co in CONV_CHANNELS]
    lin_w = [(torch.rand(c, generator=g, dtype=torch.float64) * (2.0 / c)).float() for c in LEVEL_CHANNELS]
    return conv_w, conv_b, lin_w


def _read(source, what):
    if source is None or isinstance(source, dict):
        return source
    try:
        sd = torch.load(source, map_location="cpu", weights_only=True)
    except FileNotFoundError as ex:
        raise FileNotFoundError(f"materialrefgs_amd.lpips: {what} file {source!r} does not exist") from ex
    if not isinstance(sd, dict):
        raise ValueError(f"materialrefgs_amd.lpips: {what} file {source!r} holds a {type(sd).__name__}, not a state dict")
    return sd


def _describe(sd):
    return ", ".join(f"{k} {tuple(v.shape)}" for k, v in sd.items() if torch.is_tensor(v)) or "nothing"


def parse_state_dicts(vgg, lin=None):
    """(conv_w[13], conv_b[13], lin_w[5]) from state dicts in any of the three key layouts: torchvision's `features.N.weight|bias` (with or
    without the prefix), the `lpips` package's `net.sliceK.N.*` with `linK.model.1.weight`, this reference's `net.layers.N.*` with
    `lin.K.1.weight` (or `K.1.weight`, the keys behind its get_state_dict).  A convolution is found by its trailing torchvision index N,
    a lin vector by its level K and its shape [1, C, 1, 1]; both are checked against the architecture's shapes."""
    convs, biases, lins = {}, {}, {}
    for sd, is_lin_source in ((vgg, False), (lin, True)):
        for key, t in (sd or {}).items():
            if not torch.is_tensor(t):
                continue
            m = re.search(r"(?:^|\.)(\d+)\.(weight|bias)$", key)
            if m and int(m.group(1)) in CONV_INDEX and not is_lin_source:
                i = CONV_INDEX.index(int(m.group(1)))
                if m.group(2) == "weight" and t.dim() == 4 and tuple(t.shape[2:]) == (3, 3):
                    convs[i] = (key, t)
                    continue
                # a bias belongs to the 3 x 3 weight beside it (a whole vgg16 state dict also holds classifier.0.bias)
                beside = sd.get(key[:-len("bias")] + "weight")
                if m.group(2) == "bias" and t.dim() == 1 and torch.is_tensor(beside) and beside.dim() == 4 and tuple(beside.shape[2:]) == (3, 3):
                    biases[i] = (key, t)
                    continue
            m = re.search(r"(?:^|\.)lins?\.?(\d)\.(?:model\.)?1\.weight$", key) or re.match(r"^(\d)\.1\.weight$", key)
            if m and t.dim() == 4 and t.shape[0] == 1 and tuple(t.shape[2:]) == (1, 1):
                lins[int(m.group(1))] = (key, t)
    found = f"found in vgg: {_describe(vgg or {})}; in lin: {_describe(lin or {})}"
    conv_w, conv_b, lin_w = [], [], []
    for i, (ci, co) in enumerate(CONV_CHANNELS):
        if i not in convs or i not in biases:
            raise ValueError(f"materialrefgs_amd.lpips: no {'weight' if i not in convs else 'bias'} of convolution features.{CONV_INDEX[i]} "
                             f"({ci} -> {co}); {found}")
        if tuple(convs[i][1].shape) != (co, ci, 3, 3) or tuple(biases[i][1].shape) != (co,):
            raise ValueError(f"materialrefgs_amd.lpips: {convs[i][0]} {tuple(convs[i][1].shape)} / {biases[i][0]} {tuple(biases[i][1].shape)} "
                             f"do not have the shapes {(co, ci, 3, 3)} / {(co,)} of features.{CONV_INDEX[i]}; {found}")
        conv_w.append(convs[i][1])
        conv_b.append(biases[i][1])
    for k, c in enumerate(LEVEL_CHANNELS):
        if k not in lins:
            raise ValueError(f"materialrefgs_amd.lpips: no lin vector of level {k} ([1, {c}, 1, 1]); {found}")
        if tuple(lins[k][1].shape) != (1, c, 1, 1):
            raise ValueError(f"materialrefgs_amd.lpips: {lins[k][0]} has shape {tuple(lins[k][1].shape)}, level {k} needs {(1, c, 1, 1)}; {found}")
        lin_w.append(lins[k][1].reshape(c))
    return conv_w, conv_b, lin_w


class _LpipsFn(torch.autograd.Function):
    """One image pair: owns the workspace with every ReLU output of x until the graph is freed."""

    @staticmethod
    def forward(ctx, net, x, y):
        terms, ws, cfg = net._forward(x, y, True)
        ctx.net, ctx.ws, ctx.cfg = net, ws, cfg
        ctx.shape = x.shape
        ctx.mark_non_differentiable(terms)
        return terms[5].clone(), terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        if g is None:
            return None, None, None
        dev = ctx.ws.device
        g = _lib.f32c(g)
        g_x = torch.empty(ctx.shape, dtype=torch.float32, device=dev)
        with _lib.guard(dev):
            _lib.check(_lib.lib().mrgs_lpips_backward(ctypes.byref(ctx.cfg), _p(ctx.net._blob(dev)), _p(ctx.ws), _p(g), _p(g_x),
                                                      _lib.stream_ptr(dev)))
        return None, g_x, None


class LPIPS:
    """`net(x, y)`: x, y [N,3,H,W] fp32 device tensors -> [N,1,1,1] distances; the gradient goes to x only.  The images are used as they
    are (`in_scale = 1`, `in_offset = 0`): `losses.lpips_loss` hands over images in [-1, 1], eval.py:52 hands [0, 1] images unscaled.
    An instance is what `losses.set_lpips_fn` takes.  `level_terms` [N,5]: the five level terms of the last call."""

    def __init__(self, conv_w, conv_b, lin_w, in_scale=1.0, in_offset=0.0):
        if len(conv_w) != 13 or len(conv_b) != 13 or len(lin_w) != 5:
            raise ValueError(f"materialrefgs_amd.lpips: 13 convolution weights, 13 biases and 5 lin vectors, got {len(conv_w)}, {len(conv_b)}, "
                             f"{len(lin_w)}")
        for i, (ci, co) in enumerate(CONV_CHANNELS):
            if tuple(conv_w[i].shape) != (co, ci, 3, 3) or tuple(conv_b[i].shape) != (co,):
                raise ValueError(f"materialrefgs_amd.lpips: convolution {i} needs shapes {(co, ci, 3, 3)} / {(co,)}, got "
                                 f"{tuple(conv_w[i].shape)} / {tuple(conv_b[i].shape)}")
        for k, c in enumerate(LEVEL_CHANNELS):
            if lin_w[k].numel() != c:
                raise ValueError(f"materialrefgs_amd.lpips: lin vector {k} needs {c} elements, got {tuple(lin_w[k].shape)}")
        self.conv_w = [t.detach().to("cpu", torch.float32).contiguous() for t in conv_w]
        self.conv_b = [t.detach().to("cpu", torch.float32).contiguous() for t in conv_b]
        self.lin_w = [t.detach().to("cpu", torch.float32).reshape(-1).contiguous() for t in lin_w]
        self.in_scale, self.in_offset = float(in_scale), float(in_offset)
        self._blobs = {}
        self._last_ws = None
        self.last_workspace_bytes = 0          # of the last call: the small workspace for a no-grad call
        self.level_terms = None

    # ---- construction -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_tensors(cls, conv_w, conv_b, lin_w, **kw):
        return cls(conv_w, conv_b, lin_w, **kw)

    @classmethod
    def random(cls, seed=0, **kw):
        return cls(*random_weights(seed), **kw)

    @classmethod
    def load(cls, vgg, lin=None, net_type="vgg", **kw):
        """vgg, lin: paths or state dicts (module docstring of `parse_state_dicts` for the key layouts); lin None: the lin vectors are in
        `vgg` too (the `lpips` package's whole state dict)."""
        if net_type != "vgg":
            raise NotImplementedError(f"materialrefgs_amd.lpips: only the vgg backbone is served, not {net_type!r}")
        vgg_sd = _read(vgg, "vgg")
        lin_sd = _read(lin, "lin")
        return cls(*parse_state_dicts(vgg_sd, lin_sd if lin_sd is not None else vgg_sd), **kw)

    # torch.nn.Module's spellings a caller of the `lpips` package uses on the network: the device follows the images
    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def eval(self):
        return self

    # ---- device side ----------------------------------------------------------------------------------------------------------------------
    def _blob(self, dev):
        blob = self._blobs.get(dev)
        if blob is None:
            lib = _lib.lib()
            with _lib.guard(dev):
                blob = torch.empty(lib.mrgs_lpips_weights_bytes(), dtype=torch.uint8, device=dev)
                held = [[t.to(dev) for t in ts] for ts in (self.conv_w, self.conv_b, self.lin_w)]
                tables = [(ctypes.c_void_p * len(ts))(*(t.data_ptr() for t in ts)) for ts in held]
                _lib.check(lib.mrgs_lpips_pack_weights(tables[0], tables[1], tables[2], _p(blob), _lib.stream_ptr(dev)))
            self._blobs[dev] = blob
        return blob

    def _forward(self, x, y, with_grad):
        """x, y [3,H,W] contiguous fp32 on one device -> (terms [6], workspace, cfg)"""
        dev = x.device
        H, W = int(x.shape[1]), int(x.shape[2])
        cfg = _lib.MrgsLpipsConfig(H, W, self.in_scale, self.in_offset, int(with_grad))
        lib = _lib.lib()
        blob = self._blob(dev)
        with _lib.guard(dev):
            ws = torch.empty(lib.mrgs_lpips_ws_bytes(H, W, int(with_grad)), dtype=torch.uint8, device=dev)
            terms = torch.empty(6, dtype=torch.float32, device=dev)
            _lib.check(lib.mrgs_lpips_forward(ctypes.byref(cfg), _p(blob), _p(x), _p(y), _p(ws), ws.numel(), _p(terms), _lib.stream_ptr(dev)))
        self._last_ws = (weakref.ref(ws), H, W, bool(with_grad))
        self.last_workspace_bytes = ws.numel()
        return terms, ws, cfg

    def __call__(self, x, y):
        for t, what in ((x, "x"), (y, "y")):
            if not torch.is_tensor(t):
                raise TypeError(f"materialrefgs_amd.lpips: {what} must be a tensor, got {type(t).__name__}")
            if t.dtype is not torch.float32:
                raise TypeError(f"materialrefgs_amd.lpips: {what} must be float32, got {t.dtype}")
            if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] < MIN_SIZE or t.shape[3] < MIN_SIZE:
                raise ValueError(f"materialrefgs_amd.lpips: {what} must have shape [N,3,H,W] with H, W >= {MIN_SIZE}, got {tuple(t.shape)}")
            if not t.is_cuda:
                raise RuntimeError(f"materialrefgs_amd.lpips: {what} must be a device tensor (libmrgs.so has no CPU path)")
        if x.shape != y.shape or x.device != y.device:
            raise ValueError(f"materialrefgs_amd.lpips: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} must match")
        grad = torch.is_grad_enabled()
        if grad and y.requires_grad:
            raise ValueError("materialrefgs_amd.lpips: `y` requires grad, but the gradient goes to x only; pass y.detach() or swap the images")
        y = y.detach()
        totals, levels = [], []
        for n in range(x.shape[0]):
            xn, yn = x[n].contiguous(), y[n].contiguous()
            if grad and xn.requires_grad:
                total, terms = _LpipsFn.apply(self, xn, yn)
            else:
                terms = self._forward(xn.detach(), yn, False)[0]
                total = terms[5]
            totals.append(total)
            levels.append(terms[:5])
        self.level_terms = torch.stack(levels).detach()
        return torch.stack(totals).reshape(-1, 1, 1, 1)

    forward = __call__

    def stored_activations(self):
        """Test accessor: the last with-grad call's 13 stored ReLU outputs of x and 5 taps of y as [H_s,W_s,C] views of the node's
        workspace; raises once the node has released it."""
        ws = self._last_ws and self._last_ws[0]()
        if ws is None or not self._last_ws[3]:
            raise RuntimeError("materialrefgs_amd.lpips: no live with-grad workspace (the autograd node has been freed)")
        _, H, W, _ = self._last_ws
        offs = (ctypes.c_size_t * 18)()
        _lib.check(_lib.lib().mrgs_lpips_ws_offsets(H, W, offs))
        f = ws.view(torch.float32)

        def view(off, s, c):
            h, w = H >> s, W >> s
            return f[off // 4: off // 4 + h * w * c].view(h, w, c)
        xs = [view(offs[i], CONV_STAGE[i], CONV_CHANNELS[i][1]) for i in range(13)]
        ys = [view(offs[13 + k], k, LEVEL_CHANNELS[k]) for k in range(5)]
        return xs, ys


_ENV = "MRGS_LPIPS_WEIGHTS"
_FROM_ENV = {}


def from_env(value):
    """The network named by MRGS_LPIPS_WEIGHTS (`file` or `vgg_file:lin_file`), built once per value."""
    net = _FROM_ENV.get(value)
    if net is None:
        vgg, _, lin = value.partition(":")
        try:
            net = LPIPS.load(vgg, lin or None)
        except (FileNotFoundError, ValueError) as ex:       # say which setting led here
            raise type(ex)(f"{_ENV}={value!r}: {ex}") from ex
        _FROM_ENV[value] = net
    return net
