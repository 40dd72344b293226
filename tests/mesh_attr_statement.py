"""The vertex attribute fusion (mrgs_vertex_fuse, include/mrgs.h) restated in float64 numpy, beside tests/mesh_statement.py whose
decisions, excluded set and scene helpers it reuses: the "texturing" rule of compute_unbounded_tsdf(..., return_rgb=True) over
compute_sdf_perframe (utils/mesh_utils.py:322-373, :402) with the start weight w0 (1: the reference's rule, 0: the plain mean).

Inputs that are fp32 on the device (points, camera matrices, depth and attribute maps) are passed as fp32 values converted to float64,
so the statement computes the exact function of the same numbers.
"""
import numpy as np

import mesh_statement as ms
from mesh_statement import EPS, _gather


def _gather_c(attr, yy, xx):
    """_gather for a channel-last map [H,W,C]: rows [n,C]."""
    H, W = attr.shape[:2]
    return attr[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]


def fuse_attributes(x, trunc, views, w0, depth_trunc=None, margin=1e-4):
    """views: list of (full_proj_transform [4,4], depth [H,W], attr [H,W,C]).  Returns dict(values [n,C], w [n], excluded [n], tol [n,C]).

    Per point a[c] = 0, w = w0; a view is accepted exactly as mesh_statement.fuse accepts it (projection, tap position, with depth_trunc the
    texel validity, sdf > -trunc); then s[c] = a00 w00 + a01 w01 + a10 w10 + a11 w11 with the depth tap's four weights, a[c] = (a[c] w +
    s[c]) / (w + 1) and, after all channels, w += 1.  `excluded` is mesh_statement.fuse's set (a decision within `margin` of its
    threshold), computed by that function itself; w equals its w - 1 + w0.

    The bound `tol` on |fp32 result - this result| per point and channel extends the derivation of mesh_statement.fuse's docstring (the
    points are given, so pos_err = 0; e = 2^-24; dp as derived there) by two lines:
      s_c = bilinear tap of channel c       ds_c <= dp_x Gx_c + dp_y Gy_c + 6 e max|texel_c|: Gx_c, Gy_c are the largest horizontal / vertical
                                            texel differences of channel c in the 4 x 4 neighbourhood of the cell, max|texel_c| is taken
                                            over the same neighbourhood; 6 e covers the weights, the four products and the three sums
      a_c' = (a_c w + s_c) / (w + 1)        err' <= (err w + ds_c) / (w + 1) + 3 e A_c, A_c the largest |texel| of channel c over all views
                                            (|a_c|, |s_c| <= A_c; product, sum, quotient)
    """
    x = np.asarray(x, np.float64)
    n = len(x)
    C = views[0][2].shape[2] if views else 0
    trunc_b = np.broadcast_to(np.asarray(trunc, np.float64), (n,))
    base = ms.fuse(x, trunc, [(M, d) for M, d, _ in views], depth_trunc=depth_trunc, margin=margin, bound=False)
    A = np.zeros(C)
    for _, _, attr in views:
        A = np.maximum(A, np.abs(np.asarray(attr, np.float64)).reshape(-1, C).max(axis=0))
    val, err, w = np.zeros((n, C)), np.zeros((n, C)), np.full(n, float(w0))
    for M, depth, attr in views:
        M, depth, attr = np.asarray(M, np.float64), np.asarray(depth, np.float64), np.asarray(attr, np.float64)
        H, W = depth.shape
        assert attr.shape == (H, W, C)
        clip = x @ M[:3] + M[3]
        z = clip[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            ndc = clip[:, :2] / z[:, None]
        mask = (ndc[:, 0] > -1) & (ndc[:, 0] < 1) & (ndc[:, 1] > -1) & (ndc[:, 1] < 1) & (z > 0)
        size = np.array([W - 1, H - 1], np.float64)
        nd = np.where(mask[:, None], ndc, 0.0)
        p = np.clip((nd + 1) * 0.5 * size, 0, size)
        f = np.floor(p)
        x0, y0 = f[:, 0].astype(np.int64), f[:, 1].astype(np.int64)
        tx, ty = p[:, 0] - f[:, 0], p[:, 1] - f[:, 1]
        w00, w01, w10, w11 = (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty
        d00, d01, d10, d11 = _gather(depth, y0, x0), _gather(depth, y0, x0 + 1), _gather(depth, y0 + 1, x0), _gather(depth, y0 + 1, x0 + 1)
        if depth_trunc is not None:
            lo, hi = np.minimum.reduce([d00, d01, d10, d11]), np.maximum.reduce([d00, d01, d10, d11])
            mask = mask & (lo > 0) & (hi <= depth_trunc)
        d = d00 * w00 + d01 * w01 + d10 * w10 + d11 * w11
        mask = mask & (d - z > -trunc_b)
        s = (_gather_c(attr, y0, x0) * w00[:, None] + _gather_c(attr, y0, x0 + 1) * w01[:, None] + _gather_c(attr, y0 + 1, x0) * w10[:, None]
             + _gather_c(attr, y0 + 1, x0 + 1) * w11[:, None])
        # the bound
        E = 4 * EPS * (np.abs(x) @ np.abs(M[:3]) + np.abs(M[3]))
        with np.errstate(divide="ignore", invalid="ignore"):
            dndc = (E[:, :2] + np.abs(ndc) * E[:, 3:4]) / np.abs(z)[:, None] + EPS * np.abs(ndc)
        dp = 0.5 * size * (np.where(mask[:, None], dndc, 0.0) + 2 * EPS * (np.abs(nd) + 1))
        Gx, Gy, amax = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C))
        for a in range(-1, 3):
            for b in range(-1, 3):
                c = _gather_c(attr, y0 + a, x0 + b)
                amax = np.maximum(amax, np.abs(c))
                if b < 2:
                    Gx = np.maximum(Gx, np.abs(_gather_c(attr, y0 + a, x0 + b + 1) - c))
                if a < 2:
                    Gy = np.maximum(Gy, np.abs(_gather_c(attr, y0 + a + 1, x0 + b) - c))
        ds = dp[:, 0:1] * Gx + dp[:, 1:2] * Gy + 6 * EPS * amax
        m = mask[:, None]
        err = np.where(m, (err * w[:, None] + ds) / (w[:, None] + 1) + 3 * EPS * A, err)
        val = np.where(m, (val * w[:, None] + s) / (w[:, None] + 1), val)
        w = np.where(mask, w + 1, w)
    ok = ~base["excluded"]
    assert (w[ok] == base["w"][ok] - 1 + w0).all()                      # the same decisions as mesh_statement.fuse, view by view
    return dict(values=val, w=w, excluded=base["excluded"], tol=err)


def analytic_attributes(i, H, W, channels):
    """Smooth maps of view i, fp32 [H,W,channels]: 0.5 + 0.4 sin(0.37 c + 0.21 x + 0.13 y + i)."""
    yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(channels), indexing="ij")
    return (0.5 + 0.4 * np.sin(0.37 * cc + 0.21 * xx + 0.13 * yy + i)).astype(np.float32)
