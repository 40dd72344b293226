"""Torch statement of the per-pixel prior terms materialrefgs_amd.priors computes (csrc/mrgs_prior.hip): the normal prior of
mono_normal_loss (train_refnerf.py:202-251), the mask-entropy term on rend_alpha (train_refnerf.py:1213-1215) and the four ref-score
means of train_refreal.py:1238-1258, stated from their definitions.  It runs on any device and in any floating dtype:
in float64 it is what the tests compare the native node against (autograd gives its gradients), in float32 it is the torch
form of the same terms, operation for operation what a user of the scripts executes (the end-to-end test's second path and tools/prior_time.py).

N = H W pixels in row-major order, F.normalize(x) = x / max(|x|, 1e-12).
  normal prior   v_p = R^T X[:,p], a = F.normalize(v), b = F.normalize(prior); with a mask m [N,1]: l1 = sum_p m_p sum_c |a_pc - b_pc| /
                 sum_p m_p, cos = sum_p m_p (1 - a_p.b_p) / sum_p m_p; without: plain means over p.
  mask entropy   o = clamp(alpha, lo, hi), lo / hi = 1e-6 / 1 - 1e-6 rounded to float32 (what the reference's float32 tensors hold);
                 L = -mean(m log o + (1 - m) log(1 - o)).
  ref score      a1 = mean_S |refl - 0.9|, a2 = mean_S |rough - 0.05|, b1 = mean_notS |refl - 0.05|, b2 = mean_notS |0.9 - rough|,
                 sum = a1 + a2 + b1 + b2 / 2.
`margin` is the distance of the inputs from every discrete decision in these expressions: the smallest of |a_pc - b_pc| over the
in-mask pixels with |v_p| > 0, of |refl - 0.9|, |rough - 0.05| on S and |refl - 0.05|, |rough - 0.9| on its complement, and of the
distance of every unsaturated alpha (one strictly between the bounds) from both clamp bounds.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LO = float(np.float32(1e-6))
HI = float(np.float32(1 - 1e-6))
NAMES = ("l1_surf", "cos_surf", "l1_rend", "cos_rend", "mask_entropy", "ref_metallic", "ref_roughness", "ref_metallic_bg", "ref_roughness_bg",
         "ref_sum")


def normal_terms(v, n, m=None):
    """(l1, cos) of the rotated normals v [N,3] against the prior n [N,3], weighted by m [N,1] (None: plain means)."""
    a, b = F.normalize(v, p=2, dim=-1), F.normalize(n, p=2, dim=-1)
    l1_p, cos_p = (a - b).abs().sum(dim=-1), 1.0 - (a * b).sum(dim=-1)
    if m is None:
        return l1_p.mean(), cos_p.mean()
    w = m.reshape(-1)
    return (w * l1_p).sum() / w.sum(), (w * cos_p).sum() / w.sum()


def prior_terms(*, R=None, surf_normal=None, rend_normal=None, prior=None, mask=None, rend_alpha=None, alpha_mask=None, refl=None, rough=None,
                score=None, terms_only=False):
    """Any subset of the groups.  surf_normal / rend_normal [3,H,W], R [3,3] (Camera.R), prior [N,3], mask [N,1] or None; rend_alpha
    [1,H,W], alpha_mask [N,1]; refl / rough [1,H,W], score [1,H,W] bool.  Returns a dict: the terms of NAMES that were asked for (0-d,
    differentiable), `margin` (float, inf when no decision was met) and `zero_surf` / `zero_rend` [N] bool (|v_p| = 0).  terms_only: only
    the reference's own lines (no margin, no zero maps: they read the device)."""
    out, margin = {}, math.inf
    if surf_normal is not None:
        rot = R.T.to(surf_normal.dtype)
        b = F.normalize(prior.detach(), p=2, dim=-1)
        inside = (mask.reshape(-1) > 0) if mask is not None else torch.ones(prior.shape[0], dtype=torch.bool, device=prior.device)
        for name, X in (("surf", surf_normal), ("rend", rend_normal)):
            v = (rot @ X.reshape(3, -1)).T                                           # [N,3], camera space
            out[f"l1_{name}"], out[f"cos_{name}"] = normal_terms(v, prior, mask)
            if terms_only:
                continue
            zero = v.detach().norm(dim=-1) == 0
            out[f"zero_{name}"] = zero
            live = inside & ~zero
            if bool(live.any()):
                margin = min(margin, float((F.normalize(v.detach(), p=2, dim=-1) - b).abs()[live].min()))
    if rend_alpha is not None:
        lo, hi = torch.tensor(LO, dtype=rend_alpha.dtype), torch.tensor(HI, dtype=rend_alpha.dtype)     # the bounds as this dtype holds them
        o, m = rend_alpha.reshape(-1).clamp(float(lo), float(hi)), alpha_mask.reshape(-1)
        out["mask_entropy"] = -(m * o.log() + (1.0 - m) * (1.0 - o).log()).mean()
        al = rend_alpha.detach().reshape(-1)
        free = (al > float(lo)) & (al < float(hi))
        if not terms_only and bool(free.any()):
            margin = min(margin, float((al[free] - float(lo)).min()), float((float(hi) - al[free]).min()))
    if refl is not None:
        S = score.bool()
        mean_over = lambda t, sel: t[sel].mean()                                     # a gather by a boolean map, as the scripts select
        out["ref_metallic"], out["ref_roughness"] = mean_over((refl - 0.9).abs(), S), mean_over((rough - 0.05).abs(), S)
        out["ref_metallic_bg"], out["ref_roughness_bg"] = mean_over((refl - 0.05).abs(), ~S), mean_over((0.9 - rough).abs(), ~S)
        out["ref_sum"] = out["ref_metallic"] + out["ref_roughness"] + out["ref_metallic_bg"] + 0.5 * out["ref_roughness_bg"]
        for t, c, sel in ((refl, 0.9, S), (rough, 0.05, S), (refl, 0.05, ~S), (rough, 0.9, ~S)):
            if not terms_only and bool(sel.any()):
                margin = min(margin, float((t.detach() - c).abs()[sel].min()))
    out["margin"] = margin
    return out


# ---- analytic inputs ------------------------------------------------------------------------------------------------------------------
def camera_rotation():
    """Camera.R of an orbit view (camera-to-world, float32): no entry is 0 or 1."""
    az, el = math.radians(37.0), math.radians(28.0)
    eye = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return torch.tensor(np.stack([right, down, fwd], axis=1), dtype=torch.float32)


def _q(t, steps):
    """Round to multiples of 1 / steps (steps = 0: leave as it is); what remains is exact in float32 (and in float16 for steps <= 64)."""
    return t if not steps else torch.round(t * steps) / steps


def analytic_inputs(H, W, seed=0, steps=0):
    """Float32 inputs of all three groups on an H x W image that meet the input conditions of tests/test_prior_terms.py:
    an object (a disc: shaded normals, alpha in [1e-3, 1 - 1e-3] with an exactly opaque core), a mask that is a wider disc with a soft
    edge of fractional values (so a ring of exact-zero rend_normal pixels lies inside the mask) and exactly 0 outside, where alpha is
    exactly 0 too; material maps with a ref-score blob.  `steps` quantises the normal maps and the prior (the fixture stores them in
    float16).  Returns a dict of float32 tensors (score: bool)."""
    g = torch.Generator().manual_seed(1000 * seed + H * 7 + W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    cy, cx, rad = 0.47 * H, 0.52 * W, 0.30 * min(H, W)
    r = torch.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)
    obj = r < rad                                                                        # where rend_normal is not zero
    m = ((1.45 * rad - r) / 3.0 + 0.5).clamp(0, 1)                                       # soft edge three pixels wide
    m = torch.round(m * 255) / 255                                                       # as a resized 8-bit mask divided by 255
    # world-space normals of a bumpy sphere cap, scaled by a coverage below one as the blended maps are
    nz = torch.sqrt((1 - (r / (1.2 * rad)) ** 2).clamp_min(0.05))
    n_cam = torch.stack([(xs - cx) / (1.2 * rad), (ys - cy) / (1.2 * rad), -nz]) + 0.15 * torch.randn(3, H, W, generator=g, dtype=torch.float64)
    R = camera_rotation().double()
    n_world = (R @ n_cam.reshape(3, -1)).reshape(3, H, W)
    cover = 0.35 + 0.6 * torch.rand(H, W, generator=g, dtype=torch.float64)
    rend = _q(n_world / n_world.norm(dim=0, keepdim=True) * cover, steps) * obj
    surf = n_world + 0.3 * torch.randn(3, H, W, generator=g, dtype=torch.float64)
    surf = _q(surf / surf.norm(dim=0, keepdim=True) * cover, steps) * (r < 1.25 * rad)     # zero further out: both maps have zero pixels
    prior = n_cam.reshape(3, -1).T + 0.35 * torch.randn(H * W, 3, generator=g, dtype=torch.float64)
    prior = _q(prior / prior.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(H * W, 1, generator=g, dtype=torch.float64)), steps)
    # keep every |a_pc - b_pc| clear of zero: draw the prior of a pixel again where a map's unit vector comes close to it in a component
    for _ in range(64):
        b = F.normalize(prior.to(torch.float32).double(), dim=-1)
        near = prior.norm(dim=-1) < 0.25
        for X in (surf, rend):
            v = (R.T @ X.to(torch.float32).double().reshape(3, -1)).T
            near |= (((F.normalize(v, dim=-1) - b).abs() < 2e-3) & (v.norm(dim=-1, keepdim=True) > 0)).any(dim=-1)
        if not bool(near.any()):
            break
        again = n_cam.reshape(3, -1).T + 0.6 * torch.randn(H * W, 3, generator=g, dtype=torch.float64)
        again = _q(again / again.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(H * W, 1, generator=g, dtype=torch.float64)), steps)
        prior = torch.where(near[:, None], again, prior)
    else:
        raise AssertionError("the prior could not be kept clear of the maps")
    # alpha: exactly 0 where the mask is exactly 0, exactly 1 in the object's core where the mask is exactly 1, else inside [1e-3, 1 - 1e-3]
    alpha = (0.02 + 0.96 * torch.sigmoid((1.1 * rad - r) / 4.0 + 0.4 * torch.randn(H, W, generator=g, dtype=torch.float64))).clamp(1e-3 + 1e-4, 1 - 1e-3 - 1e-4)
    alpha = torch.where(m == 0, torch.zeros_like(alpha), alpha)
    alpha = torch.where((r < 0.5 * rad) & (m == 1), torch.ones_like(alpha), alpha)
    # materials: smooth plus noise, kept 1e-3 clear of the four constants
    refl = (0.5 + 0.45 * torch.sin(0.31 * xs + 0.17 * ys) * torch.cos(0.23 * ys) + 0.04 * torch.randn(H, W, generator=g, dtype=torch.float64)).clamp(0.01, 0.99)
    rough = (0.5 + 0.45 * torch.cos(0.29 * xs - 0.11 * ys) + 0.04 * torch.randn(H, W, generator=g, dtype=torch.float64)).clamp(0.01, 0.99)
    for t in (refl, rough):
        for c in (0.9, 0.05):
            t += 4e-3 * ((t - c).abs() < 2e-3) * torch.where(t >= c, 1.0, -1.0)
    score = ((ys - 0.6 * H) ** 2 / (0.22 * H) ** 2 + (xs - 0.4 * W) ** 2 / (0.3 * W) ** 2) < 1
    f = lambda t: t.to(torch.float32).contiguous()
    return dict(R=camera_rotation(), surf_normal=f(surf), rend_normal=f(rend), prior=f(prior), mask=f(m.reshape(-1, 1)), rend_alpha=f(alpha[None]),
                refl=f(refl[None]), rough=f(rough[None]), score=score[None].contiguous())


def check_conditions(inp, margin):
    """The input conditions: what no comparison may hide.  `inp` as analytic_inputs returns it, `margin` from prior_terms in float64."""
    N = inp["mask"].numel()
    m, al = inp["mask"].reshape(-1).double(), inp["rend_alpha"].reshape(-1).double()
    assert margin >= 1e-4, margin
    sat0, sat1 = al <= LO, al >= HI
    assert bool((al[sat0] == 0).all()) and bool((m[sat0] == 0).all())
    assert bool((al[sat1] == 1).all()) and bool((m[sat1] == 1).all())
    assert int(sat0.sum()) > 0 and int(sat1.sum()) > 0
    free = ~(sat0 | sat1)
    assert bool((al[free] >= 1e-3).all()) and bool((al[free] <= 1 - 1e-3).all())
    zero = inp["rend_normal"].reshape(3, -1).abs().sum(0) == 0
    assert int(zero.sum()) >= 0.05 * N, int(zero.sum())
    assert int((zero & (m > 0)).sum()) >= 0.01 * N, int((zero & (m > 0)).sum())
    assert int(((m > 0) & (m < 1)).sum()) > 0                   # fractional values at the mask's edge
    S = inp["score"].reshape(-1)
    assert 0 < int(S.sum()) < N
