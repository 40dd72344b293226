"""The torch statement of the LPIPS (VGG16) distance that csrc/mrgs_lpips.hip implements (include/mrgs.h states it in words), in float64 by
default: z-score, thirteen 3 x 3 convolutions with ReLU, four 2 x 2 maxima, the normalised weighted distance of the five taps.  Weights
come from materialrefgs_amd.lpips.random_weights (LPIPS.random's generator) or from the caller.

Decisions.  A ReLU gate and a pooling winner are discrete: a pre-activation within a rounding of 0, or two window entries within a
rounding of each other, may fall the other way in fp32, and the gradient then differs by a whole term.  `features(..., decisions=...)`
takes the gates (13 bool tensors [C,H_s,W_s]) and the winners (4 index tensors [C,H_s/2,W_s/2], 0..3 row-major inside the window) as
given: it multiplies by the given gate and gathers the given winner, so a gradient can be compared under the SAME decisions.  Every run
also reports, per layer, |pre-activation| / RMS and the gap between each window's two largest entries / RMS, the margins a differing
decision is judged by.

The all-zero rule of the head: a pixel whose feature vector is all zero in either image contributes 0 and gets gradient 0.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from materialrefgs_amd.lpips import CONV_STAGE, SCALE, SHIFT, TAP_CONV, random_weights  # noqa: F401

EPS = 1e-10


def cast_weights(weights, dtype=torch.float64):
    conv_w, conv_b, lin_w = weights
    return [w.to(dtype) for w in conv_w], [b.to(dtype) for b in conv_b], [w.to(dtype).reshape(-1) for w in lin_w]


def first_max(windows):
    """windows [4,...] (row-major inside the 2 x 2 window) -> index of the first maximum, as torch's max_pool2d backward picks it"""
    k = torch.zeros(windows.shape[1:], dtype=torch.long)
    m = windows[0]
    for j in range(1, 4):
        upd = windows[j] > m
        k = torch.where(upd, torch.full_like(k, j), k)
        m = torch.where(upd, windows[j], m)
    return k


def windows_of(a):
    """a [C,H,W] -> [4,C,H//2,W//2], the floor of an odd size dropped"""
    H2, W2 = a.shape[1] // 2 * 2, a.shape[2] // 2 * 2
    a = a[:, :H2, :W2]
    return torch.stack((a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]))


def features(weights, img, in_scale=1.0, in_offset=0.0, decisions=None):
    """img [3,H,W] in the weights' dtype.  Returns acts (13 ReLU outputs [C,H_s,W_s]), pre (13 pre-activations), gates, winners, rms
    (13 floats), gap (4 tensors: the window's largest minus second largest entry / rms of that layer), posmax (4 bool tensors)."""
    conv_w, conv_b, _ = weights
    dt = conv_w[0].dtype
    a = in_scale * img + in_offset
    # the constants are the reference's float32 buffers (networks.py:41-44) and the kernel's float literals, widened
    a = (a - torch.tensor(SHIFT, dtype=torch.float32).to(dt)[:, None, None]) / torch.tensor(SCALE, dtype=torch.float32).to(dt)[:, None, None]
    out = SimpleNamespace(acts=[], pre=[], gates=[], winners=[], rms=[], gap=[], posmax=[])
    for i in range(13):
        if i > 0 and CONV_STAGE[i] != CONV_STAGE[i - 1]:
            win = windows_of(a)
            k = first_max(win.detach()) if decisions is None else decisions.winners[len(out.winners)]
            out.winners.append(k)
            top2 = win.detach().topk(2, dim=0).values
            out.gap.append((top2[0] - top2[1]) / out.rms[-1])
            out.posmax.append(top2[0] > 0)
            a = win.gather(0, k[None])[0]
        z = F.conv2d(a[None], conv_w[i], conv_b[i], padding=1)[0]
        gate = (z.detach() > 0) if decisions is None else decisions.gates[i]
        out.pre.append(z.detach())
        out.rms.append(float(z.detach().pow(2).mean().sqrt()))
        out.gates.append(gate)
        a = z * gate.to(dt)
        out.acts.append(a)
    return out


def head_level(fx, fy, w):
    """fx, fy [C,H,W], w [C] -> the level term"""
    sx, sy = fx.pow(2).sum(0), fy.pow(2).sum(0)
    live = (sx > 0) & (sy > 0)
    nx, ny = torch.where(live, sx, torch.ones_like(sx)).sqrt(), torch.where(live, sy, torch.ones_like(sy)).sqrt()
    d = fx / (nx + EPS) - fy / (ny + EPS)
    per_pixel = (w[:, None, None] * d * d).sum(0)
    return torch.where(live, per_pixel, torch.zeros_like(per_pixel)).mean()


def lpips(weights, x, y, in_scale=1.0, in_offset=0.0, decisions=None):
    """x, y [3,H,W].  Returns total, terms [5], x and y (the `features` records); `decisions` apply to x, y decides for itself."""
    fx = features(weights, x, in_scale, in_offset, decisions)
    with torch.no_grad():
        fy = features(weights, y, in_scale, in_offset)
    terms = torch.stack([head_level(fx.acts[c], fy.acts[c], weights[2][k]) for k, c in enumerate(TAP_CONV)])
    return SimpleNamespace(total=terms.sum(), terms=terms, x=fx, y=fy)


def decisions_of(acts):
    """The decisions a run took, read from its 13 stored ReLU outputs [C,H_s,W_s]: gate = output > 0, winner = first maximum."""
    gates = [a > 0 for a in acts]
    winners = [first_max(windows_of(acts[i - 1])) for i in range(1, 13) if CONV_STAGE[i] != CONV_STAGE[i - 1]]
    return SimpleNamespace(gates=gates, winners=winners)


def differing_decisions(ref, dec):
    """ref: a pure float64 `features` record; dec: decisions of another run.  Returns (n_differing, n_total, worst margin): the margin of a
    differing gate is |pre| / rms, of a differing winner the window's gap / rms, both taken from the float64 run."""
    n_diff = n_total = 0
    worst = 0.0
    for i in range(13):
        diff = ref.gates[i] != dec.gates[i]
        n_total += diff.numel()
        n_diff += int(diff.sum())
        if diff.any():
            worst = max(worst, float((ref.pre[i].abs() / ref.rms[i])[diff].max()))
    for j in range(4):
        diff = ref.winners[j] != dec.winners[j]
        n_total += diff.numel()
        n_diff += int(diff.sum())
        if diff.any():
            worst = max(worst, float(ref.gap[j][diff].max()))
    return n_diff, n_total, worst


def conv_abs_sum(a, w, b=None):
    """sum |a| |w| (+ |b|) of a 3 x 3 convolution in float64: the scale of its rounding bound.  a [N,C,H,W], w [Co,C,3,3]"""
    return F.conv2d(a.double().abs(), w.double().abs(), None if b is None else b.double().abs(), padding=1)


def conv_bound(K):
    """K products summed by fmaf chains, and a bias: every output within 1.01 (K + 2) 2^-24 sum |a| |w|"""
    return 1.01 * (K + 2) * 2.0 ** -24
