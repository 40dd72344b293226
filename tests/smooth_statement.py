"""Torch statement of the Sobel smoothness terms materialrefgs_amd.smoothness computes (csrc/mrgs_smooth.hip), and the inputs the tests
compare on.  The statement is `losses.spatial_gradient` applied exactly as the two reference lines write it (utils/loss_utils.py:121-125),
with the mask multiplied in first (train_refreal.py:1261: smooth_loss(base_color_map * ref_score_image)).  It runs in any floating dtype
and on any device: in float64 it is what the native node is compared against (autograd gives its gradients), in float32 on the device it
is the torch form a user of the scripts executes (tools/smooth_time.py).

kornia is not installed here and the reference's own two functions need it, so they cannot be run to make a fixture: the statement rests on
`losses.spatial_gradient`, which tests/test_losses.py pins on ramps against kornia's documented Sobel (normalized, replicate border).

The inputs remove the sign decision instead of excluding pixels.  |G| has a kink at 0: a near-zero response whose sign differed between
fp32 and float64 would move a gradient texel by a whole coefficient.  Every map is on the 1/4096 grid with magnitude below 16, so a Sobel
sum (eight taps, weights 1 and 2: below 2^7 in magnitude, a multiple of 2^-12) is exact in fp32 in any summation order, with or without
contraction; the fp32 and float64 responses are bit-equal, the zeros are exact zeros, and only the exp weight and the reductions round.
`check_conditions` asserts this on the inputs themselves.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from materialrefgs_amd.losses import spatial_gradient  # noqa: E402

GRID = 4096.0
LIMIT = 16.0


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def smooth_loss(data, mask=None):
    """utils/loss_utils.py:124-125 on data [C,H,W]; mask [H,W] (0 / 1, any dtype): the term of data * mask."""
    if mask is not None:
        data = data * mask.to(data.dtype)
    return spatial_gradient(data[None])[0].abs().sum(1).mean()


def first_order_edge_aware_loss(data, img):
    """utils/loss_utils.py:121-122 on data [3,H,W] or [1,H,W] (broadcast against the image's channels) and img [3,H,W]."""
    return (spatial_gradient(data[None])[0].abs() * torch.exp(-spatial_gradient(img[None])[0].abs())).sum(1).mean()


def responses(x):
    """8 G of x [C,H,W] as [C,2,H,W]: the Sobel sums themselves (the division by 8 is exact either way)."""
    return spatial_gradient(x[None])[0] * 8.0


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def _grid(t):
    return (torch.round(t.clamp(-LIMIT + 1, LIMIT - 1) * GRID) / GRID)


def flat_rect(H, W):
    """(y0, y1, x0, x1) of the rectangle every map holds a constant on (rows y0..y1-1), None where the image is too small for one with a
    texel two pixels inside."""
    if H < 9 or W < 9:
        return None
    h, w = max(5, H // 5), max(5, W // 5)
    y0, x0 = H // 3, W // 4
    return y0, y0 + h, x0, x0 + w


def inputs(H, W, seed=0):
    """`draw`, drawn again (at most 16 times) until every map's responses have both signs where the image has five pixels or more: on a
    line of five a draw in which every difference has one sign is not rare."""
    for attempt in range(16):
        out = draw(H, W, 16 * seed + attempt)
        maps = [out[k] for k in ("normal", "albedo", "depth", "single", "img")] + [out["albedo"] * out["mask"].to(torch.float32)]
        if H * W < 5 or all(bool((responses(x) > 0).any()) and bool((responses(x) < 0).any()) for x in maps):
            return out
    raise AssertionError(f"no draw of {H} x {W} with both signs in every map")


def draw(H, W, seed=0):
    """Float32 maps on the 1/4096 grid: `normal` [3,H,W] and `albedo` [3,H,W] (smooth structure plus noise), `depth` [1,H,W], `single`
    [1,H,W], `img` [3,H,W] in [0, 1], `mask` [H,W] bool (a blob and scattered holes, no hole in the flat rectangle) and its [1,H,W] form `score`; a flat
    rectangle (flat_rect) is set to a constant in every map."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * H + W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")

    small = 6.0 if min(H, W) < 9 else 1.0                           # a few pixels hold no turn of the smooth part: more noise there

    def wave(C, amp, noise, offset=0.0):
        ph = torch.rand(C, 4, generator=g, dtype=torch.float64) * 6.28
        t = torch.stack([torch.sin(0.37 * xs + 0.21 * ys + ph[c, 0]) * torch.cos(0.19 * ys - 0.05 * xs + ph[c, 1]) +
                         0.5 * torch.sin(0.11 * xs * (c + 1) - 0.29 * ys + ph[c, 2]) for c in range(C)])
        return offset + amp / small ** 2 * t + small * noise * torch.randn(C, H, W, generator=g, dtype=torch.float64)

    maps = dict(normal=wave(3, 0.6, 0.08), albedo=wave(3, 0.3, 0.05, 0.5), depth=wave(1, 2.5, 0.3, 6.0), single=wave(1, 1.0, 0.2),
                img=wave(3, 0.3, 0.06, 0.5).clamp(0, 1))
    rect = flat_rect(H, W)
    out = {}
    for k, (name, t) in enumerate(maps.items()):
        t = _grid(t)
        if rect is not None:
            y0, y1, x0, x1 = rect
            t[:, y0:y1, x0:x1] = (37 + 11 * k) / 64.0
        out[name] = t.to(torch.float32).contiguous()
        assert bool((out[name].double() == t).all())
    mask = ((ys - 0.55 * H) ** 2 / (0.35 * H + 1) ** 2 + (xs - 0.45 * W) ** 2 / (0.4 * W + 1) ** 2) < 1
    mask &= torch.rand(H, W, generator=g, dtype=torch.float64) < 0.9
    if rect is not None:
        mask[rect[0]:rect[1], rect[2]:rect[3]] = True              # the masked map is flat there too
    if H * W > 1:
        mask.view(-1)[0] = True
        mask.view(-1)[-1] = False                                  # both values occur whatever the size
    out["mask"] = mask.contiguous()
    out["score"] = mask[None].contiguous()
    return out


def check_conditions(inp):
    """What no comparison may hide, asserted on the inputs: every map on the grid and below the limit; the fp32 and the float64 Sobel sums
    bit-equal, also after the mask; at least one exact zero and both signs among the responses of every map, for every size at which
    they can hold (a zero: a one-pixel-wide image has no gradient across itself, and a flat rectangle gives both responses zero inside;
    both signs: at least five pixels).  Returns (share of exact zeros, share of negative ones among the rest) over all maps."""
    H, W = inp["mask"].shape
    zeros = negative = total = 0
    for name in ("normal", "albedo", "depth", "single", "img"):
        x = inp[name]
        assert x.dtype is torch.float32 and float(x.abs().max()) < LIMIT
        assert bool((x.double() * GRID == torch.round(x.double() * GRID)).all()), name
        variants = [x] + ([x * inp["mask"].to(torch.float32)] if name == "albedo" else [])
        for v in variants:
            r32, r64 = responses(v), responses(v.double())
            assert r32.dtype is torch.float32 and bool((r32.double() == r64).all()), name
            if H == 1 or W == 1 or flat_rect(H, W) is not None:
                assert int((r64 == 0).sum()) > 0, name
            if H * W >= 5:
                assert int((r64 > 0).sum()) > 0 and int((r64 < 0).sum()) > 0, name
            zeros += int((r64 == 0).sum()); negative += int((r64 < 0).sum()); total += r64.numel()
    rect = flat_rect(H, W)
    if rect is not None:
        y0, y1, x0, x1 = rect
        assert y1 - y0 >= 5 and x1 - x0 >= 5 and y1 < H and x1 < W
    if H * W > 1:
        assert 0 < int(inp["mask"].sum()) < H * W
    return zeros / total, negative / max(total - zeros, 1)
