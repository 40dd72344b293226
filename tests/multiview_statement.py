"""Float64 torch statement of the multi-view material consistency loss (calc_warp_loss, train_refnerf.py:414-739 and
train_refreal.py:405-729) for a given sample list.  It runs on any device; the GPU tests compare materialrefgs_amd.multiview against it.

Conventions (ISSUE / INTEGRATION.md section 4h): the view's patch taps are read at their exact texels (the reference's normalise /
unnormalise round trip moves a tap by ~1e-4 px, so a reference value can differ by that fraction of the local texel difference); the
neighbour's taps are bilinear with zeros padding and align_corners; a non-finite homography position samples zero.
"""
from types import SimpleNamespace

import numpy as np
import torch


def camera_record(cam, dtype=torch.float64, device=None):
    """(Wm [4,4] row-vector world_view_transform, R [3,3], T [3]) of a scene/cameras.py camera."""
    f = lambda t: torch.as_tensor(t).to(device=device, dtype=dtype)
    return f(cam.world_view_transform), f(cam.R), f(cam.T)


def L(d):
    """train_refnerf.py:640-644."""
    return torch.where(d < 0.2, 0.2 * (d / 0.2) ** 3, d + (torch.exp(5.0 * (d - 0.2)) - 1.0) / 5.0)


def geometry(D_v, D_n, cam_v, cam_n, intr_v, intr_n, th=1.0):
    """Steps 1-6: returns (e [H,W], valid [H,W] bool, weight [H,W] detached, u [H,W,2] position in n)."""
    H, W = D_v.shape
    dt, dev = D_v.dtype, D_v.device
    Wv, Rv, Tv = cam_v
    Wn, Rn, Tn = cam_n
    fx, fy, cx, cy = intr_v
    fxn, fyn, cxn, cyn = intr_n
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    rays = torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(xs)], -1)
    pts = (rays * D_v[..., None]).reshape(-1, 3)
    X = (pts - Tv) @ Rv.transpose(0, 1)
    q = X @ Wn[:3, :3] + Wn[3, :3]
    ux = q[:, 0] * fxn / q[:, 2] + cxn
    uy = q[:, 1] * fyn / q[:, 2] + cyn
    in_n = (ux > 0) & (ux < W) & (uy > 0) & (uy < H) & (q[:, 2] > 0.1)
    grid = torch.stack([ux / ((W - 1) / 2) - 1.0, uy / ((H - 1) / 2) - 1.0], -1)
    z = torch.nn.functional.grid_sample(D_n[None, None], grid.view(1, -1, 1, 2), mode="bilinear", padding_mode="border",
                                        align_corners=True).reshape(-1)
    qp = q / q[:, 2:3] * z[:, None]
    Xp = (qp - Tn) @ Rn.transpose(0, 1)
    pv = Xp @ Wv[:3, :3] + Wv[3, :3]
    proj = torch.stack([pv[:, 0] * fx / pv[:, 2] + cx, pv[:, 1] * fy / pv[:, 2] + cy], -1)
    e = torch.norm(proj - torch.stack([xs, ys], -1).reshape(-1, 2), dim=-1)
    valid = in_n & (e < th)
    w = (1.0 / torch.exp(e)).detach()
    w = torch.where(valid, w, torch.zeros_like(w))
    return e.reshape(H, W), valid.reshape(H, W), w.reshape(H, W), torch.stack([ux, uy], -1).reshape(H, W, 2)


def homographies(N_v, dist_v, cam_v, cam_n, intr_v, intr_n, samples):
    """H_s = K_n (R_rel - t_rel n^T / d) K_v^-1 per sample (train_refnerf.py:562-586), [S,3,3]."""
    Wv, Wn = cam_v[0], cam_n[0]
    dt, dev = N_v.dtype, N_v.device
    n = N_v.reshape(3, -1)[:, samples].transpose(0, 1) @ Wv[:3, :3]
    d = dist_v.reshape(-1)[samples]
    Rr = Wn[:3, :3].transpose(0, 1) @ Wv[:3, :3]
    t = -Rr @ Wv[3, :3] + Wn[3, :3]
    M = Rr[None] - t[None, :, None] * n[:, None, :] / d[:, None, None]
    fx, fy, cx, cy = intr_v
    fxn, fyn, cxn, cyn = intr_n
    Kn = torch.tensor([[fxn, 0, cxn], [0, fyn, cyn], [0, 0, 1]], dtype=dt, device=dev)
    Kvi = torch.tensor([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], dtype=dt, device=dev)
    return Kn[None] @ M @ Kvi[None]


def bilinear_zeros(img, gx, gy):
    """grid_sample(img[None], ..., zeros, align_corners=True) at pixel positions (gx, gy) for img [C,H,W]; non-finite -> 0."""
    C, H, W = img.shape
    ok = torch.isfinite(gx) & torch.isfinite(gy) & (gx > -2) & (gx < W + 1) & (gy > -2) & (gy < H + 1)
    gx = torch.where(ok, gx, torch.full_like(gx, -10.0))
    gy = torch.where(ok, gy, torch.full_like(gy, -10.0))
    x0, y0 = torch.floor(gx), torch.floor(gy)
    fx, fy = gx - x0, gy - y0
    flat = img.reshape(C, -1)
    out = 0.0
    for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        xx, yy = (x0 + dx).long(), (y0 + dy).long()
        inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(-1)
        out = out + flat[:, idx].reshape(C, *gx.shape) * (wgt * inb)[None]
    return out


def warp_loss(D_v, D_n, N_v, dist_v, base_v, m_v, r_v, base_n, m_n, r_n, fg, keep, cam_v, cam_n, intr_v, intr_n, samples, *,
              patch_half=3, th=1.0, geo_w=0.0, base_w=1.0, metal_w=1.0, rough_w=1.0, material=True, metallic=True, roughness=True):
    """Returns a dict: geo, base, metal, rough (0-d, differentiable in the depth and material maps), weight, valid, e, keep_s (per
    sample), n_valid, and the tap positions g [S,P,2] in the neighbour.  Maps are [H,W] (base [3,H,W]); samples: long pixel indices."""
    H, W = D_v.shape
    e, valid, w, _u = geometry(D_v, D_n, cam_v, cam_n, intr_v, intr_n, th)
    nv = int(valid.sum())
    zero = D_v.sum() * 0.0
    out = dict(weight=w, valid=valid, e=e, n_valid=nv, geo=zero, base=zero, metal=zero, rough=zero, keep_s=None, g=None, excl_tap=None,
               excl_sample=None, tx=None, ty=None)
    if nv == 0:
        return out
    out["geo"] = geo_w * (w * e)[valid].mean()
    if not material:
        return out
    dt, dev = D_v.dtype, D_v.device
    samples = samples.to(dev).long()
    P = (2 * patch_half + 1) ** 2
    off = torch.arange(-patch_half, patch_half + 1, device=dev)
    oy, ox = torch.meshgrid(off, off, indexing="ij")
    sx, sy = samples % W, samples // W
    tx, ty = sx[:, None] + ox.reshape(1, -1), sy[:, None] + oy.reshape(1, -1)
    inside = ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)).to(dt)
    idx = ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)
    # the view's taps carry no gradient: the reference samples them inside its `with torch.no_grad():` block (train_refnerf.py:510-559)
    tap = lambda img: img.detach().reshape(img.shape[0] if img.dim() == 3 else 1, -1)[:, idx] * inside[None]
    Hs = homographies(N_v.detach(), dist_v.detach(), cam_v, cam_n, intr_v, intr_n, samples)
    homo = torch.stack([tx.to(dt), ty.to(dt), torch.ones_like(tx, dtype=dt)], -1)
    g = torch.einsum("sij,spj->spi", Hs, homo)
    gx, gy = g[..., 0] / (g[..., 2] + 1e-10), g[..., 1] / (g[..., 2] + 1e-10)
    out["g"] = torch.stack([gx, gy], -1)
    ws = w.reshape(-1)[samples]
    b, bn = tap(base_v), bilinear_zeros(base_n.reshape(3, H, W), gx, gy)
    out["base"] = base_w * ((b - bn).abs().mean(-1).sum(0) * ws).mean()
    keep_s = tap(fg)[0].min(-1).values > 0.99
    if keep is not None:
        keep_s = keep_s & keep.reshape(-1)[samples].bool()
    out["keep_s"] = keep_s
    if metallic:
        m, mn = tap(m_v)[0], bilinear_zeros(m_n.reshape(1, H, W), gx, gy)[0]
        M = torch.max(mn, m).detach()
        vw = M.mean(-1)
        t = vw * (m - M).abs().mean(-1) * ws + vw * (mn - M).abs().mean(-1) * ws
        out["metal"] = metal_w * L(t[keep_s]).mean()
    excl_s = torch.zeros_like(keep_s)
    if roughness:
        r, rn = tap(r_v)[0], bilinear_zeros(r_n.reshape(1, H, W), gx, gy)[0]
        mn_ = torch.min(rn, r).detach()
        t = (r - mn_).abs().mean(-1) * ws + (rn - mn_).abs().mean(-1) * ws
        out["rough"] = rough_w * L(t[keep_s]).mean()
        excl_s |= keep_s & ((t.detach() - 0.2).abs() <= 1e-5 * t.detach())
    if metallic:
        tm = (vw * (m - M).abs().mean(-1) * ws + vw * (mn - M).abs().mean(-1) * ws).detach()
        excl_s |= keep_s & ((tm - 0.2).abs() <= 1e-5 * tm)
    # Decisions an fp32 evaluation can take differently (tests/test_multiview_loss.py leaves the texels they touch out, counted):
    #  * the projective division of a tap: position error 8 eps64 (|row| + |g| |row_z|) / |z| -- a tap above 1e-6 px is ill-conditioned;
    #  * a sign of |b - b'|, |m - M|, |r - min|: b' in fp32 is off by less than 5 * 2^-24 (< 4e-7) sum_i |w_i v_i| (weights rounded to
    #    fp32, four products, three sums), plus the position error times the corner values;
    #  * L's knee at t = 0.2 (the derivative jumps from 3 to 2): t in fp32 is a 49-term sum, off by at most 1e-5 t.
    with torch.no_grad():
        eps = 2.0 ** -52
        az = (Hs[:, 2:3, 0].abs() * tx.abs() + Hs[:, 2:3, 1].abs() * ty.abs() + Hs[:, 2:3, 2].abs())
        ax = (Hs[:, 0:1, 0].abs() * tx.abs() + Hs[:, 0:1, 1].abs() * ty.abs() + Hs[:, 0:1, 2].abs())
        ay = (Hs[:, 1:2, 0].abs() * tx.abs() + Hs[:, 1:2, 1].abs() * ty.abs() + Hs[:, 1:2, 2].abs())
        den = (g[..., 2] + 1e-10).abs()
        dg = 8 * eps * torch.maximum(ax + gx.abs() * az, ay + gy.abs() * az) / den
        dg = torch.where(torch.isfinite(dg), dg, torch.full_like(dg, float("inf")))
        ill = dg > 1e-6
        ill = ill & torch.isfinite(gx) & (gx > -2) & (gx < W + 1) & (gy > -2) & (gy < H + 1)
        def near(a, an, img):
            # strict: where every corner is 0 (or the tap is off the map) b' is exactly 0 in fp32 as well, so no decision differs
            C = img.reshape(-1, H * W).shape[0]
            sabs = bilinear_zeros(img.reshape(C, H, W).abs(), gx, gy)               # sum of |w_i v_i|
            return (a - an).abs() < 4e-7 * sabs + dg.clamp(max=1.0) * 2 * sabs
        excl = ill | near(b, bn, base_n).any(0)
        if metallic:
            excl |= near(m[None], mn[None], m_n)[0]
        if roughness:
            excl |= near(r[None], rn[None], r_n)[0]
    out.update(excl_tap=excl, excl_sample=excl_s, tx=tx, ty=ty)
    return out


# ---- an analytic scene: a tilted, bounded plane with a sphere in front, materials anchored in world space ------------------------------
PLANE_N = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
PLANE_D = -0.3
SPHERE_C, SPHERE_R = np.array([0.15, -0.1, 0.25]), 0.45


def _cast(cam, H, W):
    """Per pixel: depth (camera z), world hit point, world normal facing the camera; depth 0 where nothing is hit."""
    from materialrefgs_amd.camera import fov2focal
    fx, fy = fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H)
    R, T = cam.R.double().numpy(), cam.T.double().numpy()
    eye = -R @ T
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirc = np.stack([(xs - 0.5 * W) / fx, (ys - 0.5 * H) / fy, np.ones_like(xs)], -1)
    dirw = dirc @ R.T
    # plane
    t_pl = (PLANE_D - eye @ PLANE_N) / (dirw @ PLANE_N)
    hit_pl = eye + t_pl[..., None] * dirw
    ok_pl = (t_pl > 0) & (np.abs(hit_pl[..., 0]) < 1.2) & (np.abs(hit_pl[..., 1]) < 1.2)
    # sphere
    oc = eye - SPHERE_C
    bq = (dirw * oc).sum(-1)
    aq = (dirw * dirw).sum(-1)
    disc = bq * bq - aq * ((oc * oc).sum() - SPHERE_R ** 2)
    t_sp = (-bq - np.sqrt(np.maximum(disc, 0))) / aq
    ok_sp = (disc > 0) & (t_sp > 0)
    t = np.where(ok_sp & (~ok_pl | (t_sp < t_pl)), t_sp, np.where(ok_pl, t_pl, 0.0))
    hit = eye + t[..., None] * dirw
    nrm = np.where((ok_sp & (~ok_pl | (t_sp < t_pl)))[..., None], (hit - SPHERE_C) / SPHERE_R, PLANE_N[None, None] * np.ones_like(hit))
    nrm = np.where(((nrm * dirw).sum(-1) > 0)[..., None], -nrm, nrm)
    fg = (t > 0).astype(np.float64)
    return t, hit, nrm, fg


def analytic_pair(H, W, az=(30.0, 37.0), noise=0.002, seed=0):
    """Two views: dict per view with depth, normal [3,H,W], distance, base [3,H,W], metal, rough, fg (float32 CPU) and the camera."""
    rng = np.random.default_rng(seed)
    out = []
    for a in az:
        from materialrefgs_amd.camera import look_at_camera
        cam = look_at_camera(a, 25.0, 4.0, 0.7, H, W)
        t, hit, nrm, fg = _cast(cam, H, W)
        Wm = cam.world_view_transform.double().numpy()
        n_c = nrm @ Wm[:3, :3]
        X_c = hit @ Wm[:3, :3] + Wm[3, :3]
        dist = np.abs((n_c * X_c).sum(-1)) * fg
        base = np.stack([0.5 + 0.4 * np.sin(3 * hit[..., 0]), 0.5 + 0.4 * np.cos(2 * hit[..., 1]), 0.5 + 0.3 * np.sin(4 * hit[..., 2])]) * fg
        metal = (0.5 + 0.45 * np.sin(5 * hit[..., 0] + 2 * hit[..., 1])) * fg
        rough = (0.5 + 0.45 * np.cos(4 * hit[..., 1] - 3 * hit[..., 2])) * fg
        depth = t * (1 + noise * rng.standard_normal(t.shape)) * fg
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        out.append(SimpleNamespace(cam=cam, depth=f(depth), normal=f(nrm.transpose(2, 0, 1)), distance=f(dist), base=f(base), metal=f(metal),
                                   rough=f(rough), fg=f(fg)))
    return out
