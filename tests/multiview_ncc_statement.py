"""Float64 torch statement of the grey-image patch NCC term of train_refreal.py's multi-view loss (get_consistency_loss2, :358-395, over
lncc, utils/loss_utils.py:230-265) for a given sample list, next to tests/multiview_statement.py whose geometry, homographies, bilinear
lookup and analytic scene it uses as they are.  It runs on any device and in any floating dtype: in float64 it is what the GPU tests
compare materialrefgs_amd.multiview against, in float32 it is the literal torch form of the reference's expressions (the truth leg and
tools/ncc_time.py).

Per sample s with P = (2 h + 1)^2 taps: r = the view's grey image at the integer texels (zero outside), q = the neighbour's at the
homography position (bilinear, zeros, align_corners; non-finite -> 0), the five patch sums of lncc exactly as it writes them,
ncc_s = clamp(1 - cross^2 / (var_r var_q + 1e-8), 0, 2); m_s = patch mean of the view's refl_strength_map + patch mean of the
neighbour's at the same positions; use_s = ncc_s < 0.9 and m_s < 0.4; ncc = ncc_w * mean over use_s of ncc_s w_s with w_s the detached
geometric weight; ref_weight_s = 1 - m_s / 2, 0 below 0.9, scattered to an H x W map (visual_refweight).  The gradient reaches
rend_normal and rend_distance of the view through the homography, nothing else.

A sample is *ambiguous* when an evaluation in another precision may decide it differently: |ncc_s - 0.9| <= delta or
|m_s - 0.4| <= delta (and, for the weight map only, |m_s - 0.2| <= delta, where ref_weight crosses 0.9).  `use_override` replaces
use_s on the ambiguous samples, because one flipped sample moves the mean's denominator for every texel.
"""
import numpy as np
import torch

from multiview_statement import _cast, analytic_pair, bilinear_zeros, geometry, homographies  # noqa: F401


def ncc_loss(N_v, dist_v, grey_v, grey_n, m_v, m_n, w, cam_v, cam_n, intr_v, intr_n, samples, *, patch_half=3, ncc_w=0.15, delta=1e-5,
             use_override=None):
    """N_v [3,H,W] and dist_v [H,W] may require grad; grey_*, m_* [H,W]; w: the weight map [H,W] of multiview_statement.geometry;
    samples: long pixel indices.  Returns a dict: ncc (0-d), ncc_s, m_s, use_s, ambiguous, ambiguous_w [S], ref_weight [H,W], n_used."""
    H, W = grey_v.shape
    dt, dev = N_v.dtype, N_v.device
    samples = samples.to(dev).long()
    zero = N_v.sum() * 0.0 + dist_v.sum() * 0.0
    e = torch.zeros(0, dtype=dt, device=dev)
    eb = torch.zeros(0, dtype=torch.bool, device=dev)
    out = dict(ncc=zero, ncc_s=e, m_s=e, use_s=eb, ambiguous=eb, ambiguous_w=eb, ref_weight=torch.zeros(H, W, dtype=dt, device=dev), n_used=0)
    if samples.numel() == 0:
        return out
    P = (2 * patch_half + 1) ** 2
    off = torch.arange(-patch_half, patch_half + 1, device=dev)
    oy, ox = torch.meshgrid(off, off, indexing="ij")
    sx, sy = samples % W, samples // W
    tx, ty = sx[:, None] + ox.reshape(1, -1), sy[:, None] + oy.reshape(1, -1)
    inside = ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)).to(dt)
    idx = ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)
    tap = lambda img: img.detach().reshape(-1)[idx] * inside
    Hs = homographies(N_v, dist_v, cam_v, cam_n, intr_v, intr_n, samples)
    homo = torch.stack([tx.to(dt), ty.to(dt), torch.ones_like(tx, dtype=dt)], -1)
    g = torch.einsum("sij,spj->spi", Hs, homo)
    gx, gy = g[..., 0] / (g[..., 2] + 1e-10), g[..., 1] / (g[..., 2] + 1e-10)
    r = tap(grey_v)
    q = bilinear_zeros(grey_n.detach().reshape(1, H, W), gx, gy)[0]
    # lncc, literally
    r_sum, q_sum, r2_sum, q2_sum, rq_sum = r.sum(-1), q.sum(-1), (r * r).sum(-1), (q * q).sum(-1), (r * q).sum(-1)
    r_avg, q_avg = r_sum / P, q_sum / P
    cross = rq_sum - q_avg * r_sum
    r_var = r2_sum - r_avg * r_sum
    q_var = q2_sum - q_avg * q_sum
    cc = cross * cross / (r_var * q_var + 1e-8)
    ncc_s = torch.clamp(1 - cc, 0.0, 2.0)
    with torch.no_grad():
        m_s = tap(m_v).mean(-1) + bilinear_zeros(m_n.detach().reshape(1, H, W), gx, gy)[0].mean(-1)
        nd = ncc_s.detach()
        use = (nd < 0.9) & (m_s < 0.4)
        amb = ((nd - 0.9).abs() <= delta) | ((m_s - 0.4).abs() <= delta)
        amb_w = amb | ((m_s - 0.2).abs() <= delta)
        if use_override is not None:
            use = torch.where(amb, use_override.to(dev).bool(), use)
        ref_weight = 1.0 - m_s / 2
        ref_weight = torch.where(ref_weight < 0.9, torch.zeros_like(ref_weight), ref_weight)
        rmap = torch.zeros(H * W, dtype=dt, device=dev)
        rmap[samples] = ref_weight
        ws = w.detach().reshape(-1)[samples].to(dt)
    n_used = int(use.sum())
    if n_used > 0:
        out["ncc"] = ncc_w * (ncc_s * ws)[use].mean()
    out.update(ncc_s=ncc_s.detach(), m_s=m_s, use_s=use, ambiguous=amb, ambiguous_w=amb_w, ref_weight=rmap.reshape(H, W), n_used=n_used)
    return out


def grey_pair(H, W, az=(30.0, 37.0), freq=None):
    """The grey photographs of analytic_pair(H, W): 0.5 + 0.25 sin(f (12 x + 8.4 y)) + 0.2 cos(f (15.6 y - 10.8 z)) of the world hit point,
    times the foreground; float32 [H,W] per view.  f grows with the resolution (f = max(1, H / 48)) so that a 7 x 7 patch spans a good
    part of a period at every size: with f = 1 at 800^2 the texture is nearly flat over a patch, the median used sample's gradient is 2e-6
    of the largest, and a gradient comparison scaled by the largest element would say little about most samples."""
    from materialrefgs_amd.camera import look_at_camera
    f = max(1.0, H / 48.0) if freq is None else freq
    out = []
    for a in az:
        cam = look_at_camera(a, 25.0, 4.0, 0.7, H, W)
        _t, hit, _n, fg = _cast(cam, H, W)
        x, y, z = hit[..., 0], hit[..., 1], hit[..., 2]
        grey = (0.5 + 0.25 * np.sin(f * (12.0 * x + 8.4 * y)) + 0.2 * np.cos(f * (15.6 * y - 10.8 * z))) * fg
        out.append(torch.tensor(grey, dtype=torch.float32))
    return out
