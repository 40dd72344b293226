"""The edge mask of materialrefgs_amd.edges (include/mrgs.h: mrgs_edge_mask) in numpy, integer arrays only after the one float32 multiply
of the quantisation.  The stages are separate so that a test can enter at any of them:

    quantise(img)                     [3,H,W] float -> [3,H,W] int64 in 0..255
    grey(u)                           [3,H,W] -> [H,W]
    sobel(g)                          [H,W] -> dx, dy, m
    classes(g, thres1, thres2)        [H,W] -> [H,W] uint8: 0 none, 1 candidate, 2 strong
    hysteresis(cls)                   [H,W] -> [H,W] bool: candidates whose 8-connected component holds a strong pixel
    dilate(edge, d)                   [H,W] bool -> [H,W] bool
    edge_mask(img, d, t1, t2, invert) the chain; returns (mask bool [H,W], classes uint8 [H,W])

Hysteresis uses scipy.ndimage.label with a 3 x 3 structure.
"""
import math

import numpy as np
from scipy import ndimage


def quantise(img):
    v = np.asarray(img, dtype=np.float32) * np.float32(255.0)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (np.abs(v) < np.float32(2147483648.0))
    t = np.trunc(np.where(ok, v, np.float32(0.0))).astype(np.int64)
    return t & 255                                   # two's complement wrap: -127 -> 129


def grey(u):
    u = np.asarray(u, dtype=np.int64)
    return (9798 * u[0] + 19235 * u[1] + 3735 * u[2] + 16384) >> 15


def sobel(g):
    g = np.asarray(g, dtype=np.int64)
    H, W = g.shape
    p = np.pad(g, 1, mode="edge")
    at = lambda oy, ox: p[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    dx = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    dy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return dx, dy, np.abs(dx) + np.abs(dy)


def thresholds(thres1, thres2):
    """(low, high): the floors of the smaller and the larger threshold, clamped to [-1, 2041] -- m lies in [0, 2040], so the clamp changes
    no comparison."""
    f = lambda t: int(min(max(math.floor(min(max(t, -2.0), 4096.0)), -1), 2041))
    return f(min(thres1, thres2)), f(max(thres1, thres2))


def classes(g, thres1=0.0, thres2=80.0):
    dx, dy, m = sobel(g)
    H, W = m.shape
    low, high = thresholds(thres1, thres2)
    mp = np.pad(m, 1, mode="constant")               # m is 0 outside the image
    at = lambda oy, ox: mp[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    horiz = (m > at(0, -1)) & (m >= at(0, 1))
    vert = (m > at(-1, 0)) & (m >= at(1, 0))
    neg = (dx ^ dy) < 0                              # s = -1: compare with (y-1, x+1) and (y+1, x-1)
    diag = np.where(neg, (m > at(-1, 1)) & (m > at(1, -1)), (m > at(-1, -1)) & (m > at(1, 1)))
    peak = np.where(ay < t22, horiz, np.where(ay > t67, vert, diag))
    cand = (m > low) & peak
    return (cand.astype(np.uint8) + (cand & (m > high)).astype(np.uint8)).astype(np.uint8)


def components(cls):
    """(labels int [H,W], count): the 8-connected components of the candidates."""
    return ndimage.label(np.asarray(cls) > 0, structure=np.ones((3, 3), dtype=np.int64))


def hysteresis(cls):
    cls = np.asarray(cls)
    labels, n = components(cls)
    strong = np.zeros(n + 1, dtype=bool)
    strong[labels[cls == 2]] = True
    strong[0] = False
    return strong[labels]


def dilate(edge, d):
    edge = np.asarray(edge, dtype=bool)
    H, W = edge.shape
    a = d // 2
    out = np.zeros((H, W), dtype=bool)
    for oy in range(-a, d - a):
        for ox in range(-a, d - a):
            # out[y, x] |= edge[y + oy, x + ox] where that position lies inside the image
            ys, ye = max(0, -oy), min(H, H - oy)
            xs, xe = max(0, -ox), min(W, W - ox)
            if ys < ye and xs < xe:
                out[ys:ye, xs:xe] |= edge[ys + oy:ye + oy, xs + ox:xe + ox]
    return out


def edge_mask(img, dilate_size=4, thres1=0.0, thres2=80.0, invert=False):
    cls = classes(grey(quantise(img)), thres1, thres2)
    out = dilate(hysteresis(cls), dilate_size)
    return (~out if invert else out), cls
