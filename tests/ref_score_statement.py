"""Float64 torch statement of the multi-view reflection score (calc_ref_score, train_refreal.py:782-1001) and the analytic inputs of its
tests.  Built from the geometry, the plane homographies and the zero-padded bilinear tap of tests/multiview_statement.py; it runs in
chunks of pixels, so the [3, pixels, taps] tensors of a neighbour never exist whole.

For pixel p of view v with neighbours n_1..n_K (all H x W), patch half-width h, P = (2h+1)^2 taps:
  valid_n(p)  the reprojection check of the warp loss (multiview_statement.geometry) with e < th;
  a[c,t]      photograph of v at the integer texel p + o_t, zero outside the image;
  s_n[c,t]    photograph of n at H_n (p + o_t, 1), dehomogenised with + 1e-10, bilinear, zeros, align_corners, non-finite -> 0;
  cnt(p)      number of valid neighbours;
  score(p) =  [cnt > 0] (1/P) sum_t sum_c (sum_{n valid} |s_n[c,t] - a[c,t]|) / (cnt + 1e-8).
"""
from types import SimpleNamespace

import numpy as np
import torch

import multiview_statement as ms
from multiview_statement import bilinear_zeros, geometry, homographies

LIGHT = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


def intrinsics(cam):
    """(Fx, Fy, Cx, Cy) rounded to float32, as the C ABI carries them."""
    from materialrefgs_amd.camera import fov2focal
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


def photograph(view, H, W):
    """[3,H,W] float32: the analytic scene's base colour plus a view-dependent lobe (a mirror-direction highlight), zero off the object."""
    cam = view.cam
    _t, hit, nrm, fg = ms._cast(cam, H, W)
    eye = -(cam.R.double().numpy() @ cam.T.double().numpy())
    v = eye - hit
    v /= np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)            # (off the object hit = eye; masked by fg below)
    r = 2.0 * (nrm * v).sum(-1, keepdims=True) * nrm - v
    lobe = np.maximum((r * LIGHT).sum(-1), 0.0) ** 6
    img = np.clip(0.75 * view.base.double().numpy() + 0.5 * lobe[None], 0.0, 1.0) * fg[None]
    return torch.tensor(img, dtype=torch.float32)


def analytic_views(H, W, az=(30.0, 37.0, 24.0, 41.0)):
    """The views of multiview_statement.analytic_pair at these azimuths, each with its photograph (`image`) and a name."""
    views = ms.analytic_pair(H, W, az=az)
    for i, v in enumerate(views):
        v.image = photograph(v, H, W)
        v.name = f"view{i}"
    return views


def blind_view(H, W, az=210.0):
    """A camera at the orbit position of azimuth `az` that looks away from the scene: it sees nothing, every map is zero."""
    from materialrefgs_amd.camera import look_at_camera
    el, dist = 25.0, 4.0
    a, e = np.radians(az), np.radians(el)
    eye = dist * np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    cam = look_at_camera(az + 180.0, -el, dist, 0.7, H, W, target=tuple(2.0 * eye))
    assert ms._cast(cam, H, W)[3].sum() == 0
    z = torch.zeros(H, W)
    return SimpleNamespace(cam=cam, depth=z, normal=torch.zeros(3, H, W), distance=z, base=torch.zeros(3, H, W), image=torch.zeros(3, H, W),
                           name="blind")


def _z_in_neighbour(D_v, cam_v, cam_n, intr_v):
    """Camera-space z in n of every pixel of v back-projected through D_v (the quantity the check compares with 0.1)."""
    H, W = D_v.shape
    dt, dev = D_v.dtype, D_v.device
    Wv, Rv, Tv = cam_v
    Wn = cam_n[0]
    fx, fy, cx, cy = intr_v
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev), indexing="ij")
    pts = (torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(xs)], -1) * D_v[..., None]).reshape(-1, 3)
    X = (pts - Tv) @ Rv.transpose(0, 1)
    return (X @ Wn[:3, :3] + Wn[3, :3])[:, 2].reshape(H, W)


def ref_score(view, neighbours, *, th=1.0, patch_half=4, chunk=4096, margin=1e-6, dtype=torch.float64, device=None, diagnostics=True):
    """view / neighbours: objects with cam, depth [H,W], normal [3,H,W], distance [H,W] (the view only) and image [3,H,W].
    Returns a SimpleNamespace: score [H,W], count [H,W] int64, valid [K,H,W] bool and, with `diagnostics`, ambiguous [H,W] bool (a
    decision quantity of some neighbour within `margin` of its threshold: e against th, u against 0 and W, v against 0 and H, z against
    0.1) and anchor_outside / nbr_outside: whether any anchor tap / any neighbour tap of a valid (pixel, neighbour) falls outside the image.
    `dtype` / `device`: the arithmetic of the whole evaluation (float64 on the CPU is the statement; tools time the float32 form)."""
    cast = lambda t: t.to(device=device, dtype=dtype)
    D_v, N_v, dist_v, img_v = cast(view.depth), cast(view.normal), cast(view.distance), cast(view.image)
    H, W = D_v.shape
    dev = D_v.device
    cam_v, intr_v = ms.camera_record(view.cam, dtype, dev), intrinsics(view.cam)
    K, h = len(neighbours), patch_half
    P = (2 * h + 1) ** 2
    off = torch.arange(-h, h + 1, device=dev)
    oy, ox = torch.meshgrid(off, off, indexing="ij")
    ox, oy = ox.reshape(1, -1), oy.reshape(1, -1)
    valid = torch.zeros(K, H, W, dtype=torch.bool, device=dev)
    ambiguous = torch.zeros(H, W, dtype=torch.bool, device=dev)
    total = torch.zeros(H * W, dtype=dtype, device=dev)
    nbr_outside = False
    pix = torch.arange(H * W, device=dev)
    for k, n in enumerate(neighbours):
        if (n.cam.image_height, n.cam.image_width) != (H, W):
            raise ValueError("ref_score: all views must have the same image size")
        cam_n, intr_n = ms.camera_record(n.cam, dtype, dev), intrinsics(n.cam)
        e, ok, _w, u = geometry(D_v, cast(n.depth), cam_v, cam_n, intr_v, intr_n, th)
        if diagnostics:
            z = _z_in_neighbour(D_v, cam_v, cam_n, intr_v)
            near = lambda q, t: (q - t).abs() < margin
            ambiguous |= near(e, th) | near(u[..., 0], 0.0) | near(u[..., 0], float(W)) | near(u[..., 1], 0.0) | \
                near(u[..., 1], float(H)) | near(z, 0.1)
        valid[k] = ok
        sel = pix[ok.reshape(-1)]
        img_n = cast(n.image)
        for s0 in range(0, sel.numel(), chunk):
            s = sel[s0:s0 + chunk]
            Hs = homographies(N_v, dist_v, cam_v, cam_n, intr_v, intr_n, s)
            tx, ty = (s % W)[:, None] + ox, (s // W)[:, None] + oy
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            homo = torch.stack([tx.to(dtype), ty.to(dtype), torch.ones_like(tx, dtype=dtype)], -1)
            g = torch.einsum("sij,spj->spi", Hs, homo)
            gx, gy = g[..., 0] / (g[..., 2] + 1e-10), g[..., 1] / (g[..., 2] + 1e-10)
            smp = bilinear_zeros(img_n, gx, gy)                                     # [3,S,P]
            idx = ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)
            anchor = img_v.reshape(3, -1)[:, idx] * inside[None]
            total[s] += (smp - anchor).abs().sum(0).sum(-1)
            if diagnostics:
                nbr_outside |= bool((~(torch.isfinite(gx) & (gx >= 0) & (gx <= W - 1) & (gy >= 0) & (gy <= H - 1))).any())
    count = valid.sum(0)
    score = torch.where(count > 0, total.reshape(H, W) / (count.to(dtype) + 1e-8) / P, torch.zeros(H, W, dtype=dtype, device=dev))
    xs, ys = (pix % W).reshape(H, W), (pix // W).reshape(H, W)
    rim = (xs < h) | (xs >= W - h) | (ys < h) | (ys >= H - h)
    return SimpleNamespace(score=score, count=count, valid=valid, ambiguous=ambiguous, anchor_outside=bool((rim & (count > 0)).any()),
                           nbr_outside=nbr_outside)


class Cam:
    """What materialrefgs_amd.refscore reads of a scene/cameras.py camera, around a MiniCam."""

    def __init__(self, mini, name, image=None):
        self.image_width, self.image_height, self.image_name = mini.image_width, mini.image_height, name
        self.FoVx, self.FoVy = mini.FoVx, mini.FoVy
        self.world_view_transform, self.R, self.T, self.camera_center = mini.world_view_transform, mini.R, mini.T, mini.camera_center
        self.Fx, self.Fy, self.Cx, self.Cy = intrinsics(mini)
        self.original_image = image
