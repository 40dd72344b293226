"""`from lpipsPyTorch import lpips` (eval.py:17) resolves to the MI355X implementation (materialrefgs_amd.lpips -> libmrgs.so).

The reference's package builds torchvision's VGG16 and downloads two weight files per call.  Here the network is the native one, built
once from the files named by the environment variable MRGS_LPIPS_WEIGHTS (`vgg_file` or `vgg_file:lin_file`), or whatever
`set_default_network` registered.  The images go in as they are: eval.py:52 hands [0, 1] images over unscaled, and so does this.
Only net_type 'vgg' and version '0.1' are served.  See INTEGRATION.md.
"""
import os

from materialrefgs_amd import lpips as _native

_DEFAULT = None


def set_default_network(net):
    """Register the network behind `lpips` and `LPIPS` (a materialrefgs_amd.lpips.LPIPS; None unregisters)."""
    global _DEFAULT
    _DEFAULT = net


def _network(net_type, version):
    if net_type != "vgg":
        raise NotImplementedError(f"lpipsPyTorch: only net_type 'vgg' is served by libmrgs.so, not {net_type!r}")
    if version != "0.1":
        raise NotImplementedError(f"lpipsPyTorch: only version '0.1' exists, not {version!r}")
    if _DEFAULT is not None:
        return _DEFAULT
    value = os.environ.get("MRGS_LPIPS_WEIGHTS")
    if not value:
        raise NotImplementedError("lpipsPyTorch: the VGG16 and lin weights are downloads and not part of this build; name the files in "
                                  "MRGS_LPIPS_WEIGHTS (vgg_file or vgg_file:lin_file) or call lpipsPyTorch.set_default_network(...) "
                                  "(INTEGRATION.md)")
    return _native.from_env(value)


class LPIPS:
    """The reference's criterion (lpipsPyTorch/modules/lpips.py:8-36) over the default network: `LPIPS('vgg')(x, y)` -> [1,1,1,1]."""

    def __init__(self, net_type="vgg", version="0.1"):
        self.net = _network(net_type, version)

    def to(self, *a, **k):
        return self

    def __call__(self, x, y):
        return self.net(x, y).sum(0, keepdim=True)

    forward = __call__


def lpips(x, y, net_type="vgg", version="0.1"):
    """lpipsPyTorch/__init__.py:6-21: the distance of x and y, [N,3,H,W] device tensors, summed over the batch as the reference's
    `torch.sum(torch.cat(res, 0), 0, True)` does."""
    return LPIPS(net_type, version)(x, y)


__all__ = ["lpips", "LPIPS", "set_default_network"]
