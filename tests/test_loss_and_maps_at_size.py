"""The image-space kernels at production sizes and at ragged ones, against float64 (-m gpu).

A. The fused loss (csrc/mrgs_loss.hip: loss_fwd_kernel, loss_finalize_kernel, loss_bwd_kernel) against
   oracle/loss_oracle.calculate_loss_torch on the CPU: 800^2, 1600^2 and 779 x 1037 with training-like images (gt on the 1/255 grid,
   a flat background, saturated pixels, img == gt on a tenth of the pixels) in both normal modes with the distortion term; images
   below the 11 x 11 window and the 32 x 32 tile with C = 1..4 and lambda_dssim 0, 0.2, 1; 1024 and 1025 partial rows for the
   finalize loop; the C ABI's workspace bound and argument checks; run-to-run identity; a gt that requires grad.
B. The maps kernel (csrc/mrgs_maps.hip: surfel_maps_fwd_kernel / surfel_maps_bwd_kernel with its 32 x 8 tiles and LDS halos)
   against compute_2dgs_normal_and_regularizations_reference in float64 on the CPU, from 1 x 1 to 1600^2, random upstream on
   every output.
C. The compositing kernel (surfel_composite_*) at 1600^2 and 779 x 1037.

Bars are those of tests/test_losses.py and tests/test_shading.py, except surf_normal's value at sizes where the finite differences
cancel in fp32 (see _kappa).  Lines starting with REPORT give the largest errors seen (pytest -s).
"""
import ctypes
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import loss_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAM = dict(lambda_normal=0.05, lambda_dist=100.0)          # tests/golden/reference_loss.npz's settings
UP = 0.37                                                  # upstream scale of every loss backward here
U32 = 2.0 ** -24


def _rel(a, b, floor=1e-30):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def _report(*parts):
    print("REPORT", *parts, flush=True)


# ---------------------------------------------------------------- A. fused loss
def _loss_inputs(C, H, W, seed):
    """Training-like inputs on the CPU: gt on the 1/255 grid with smooth structure, a flat background rectangle where img == gt is one
    constant colour, saturated 0 / 1 pixels, img == gt exactly on ~10 % of the other pixels; unit normals with surf == rend on ~10 %."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(7 * xx + 3 * yy)[None] * torch.cos(5 * yy + torch.arange(C)[:, None, None])
    gt = torch.round((base + 0.2 * torch.rand(C, H, W, generator=g) - 0.1).clamp(0, 1) * 255) / 255
    r = torch.rand(H, W, generator=g)
    gt[:, r < 0.03] = 0.0
    gt[:, r > 0.97] = 1.0
    img = (gt + 0.05 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    eq = torch.rand(H, W, generator=g) < 0.1
    img[:, eq] = gt[:, eq]
    if H >= 16 and W >= 16:
        y0, y1, x0, x1 = H // 5, H // 5 + H // 4, W // 6, W // 6 + W // 3
        colour = torch.tensor([57.0, 140.0, 203.0, 96.0])[:C, None, None] / 255
        gt[:, y0:y1, x0:x1] = colour
        img[:, y0:y1, x0:x1] = colour
    rn = F.normalize(torch.randn(3, H, W, generator=g), dim=0)
    sn = F.normalize(rn + 0.3 * torch.randn(3, H, W, generator=g), dim=0)
    same = torch.rand(H, W, generator=g) < 0.1
    sn[:, same] = rn[:, same]
    dist = torch.rand(1, H, W, generator=g) * 1e-3
    weight = torch.rand(H, W, generator=g) ** 2
    return dict(img=img, gt=gt, rn=rn, sn=sn, dist=dist, weight=weight)


def _run_loss(d, lam_dssim, mode, dist=True):
    """fused_loss on the device and (loss * UP).backward(): (terms [16] on the CPU, gradients dict on the CPU)."""
    from materialrefgs_amd import losses
    t = {k: v.to(DEV) for k, v in d.items()}
    img = t["img"].clone().requires_grad_(True)
    rn, sn, ds = (t[k].clone().requires_grad_(True) for k in ("rn", "sn", "dist"))
    normal = mode in ("w", "cos")
    loss, terms = losses.fused_loss(img, t["gt"], rn if normal else None, sn if normal else None, ds if dist else None,
                                    t["weight"] if mode == "w" else None, lambda_dssim=lam_dssim,
                                    lambda_normal=LAM["lambda_normal"] if normal else 0.0, lambda_dist=LAM["lambda_dist"] if dist else 0.0)
    (loss * UP).backward()
    grads = {"image": img.grad, "rend_normal": rn.grad, "surf_normal": sn.grad, "rend_dist": ds.grad}
    return float(loss.detach()), terms.cpu(), {k: (v.cpu() if v is not None else None) for k, v in grads.items()}


def _check_loss(d, lam_dssim, mode, tag, dist=True, ssim_pair=None, seam=False):
    """One configuration against the float64 checker with the bars of tests/test_losses.py; returns the checker's SSIM pair for reuse."""
    C = d["img"].shape[0]
    normal = mode in ("w", "cos")
    loss, terms, g = _run_loss(d, lam_dssim, mode, dist)
    kw = dict(lambda_dssim=lam_dssim, lambda_normal=LAM["lambda_normal"] if normal else 0.0, lambda_dist=LAM["lambda_dist"] if dist else 0.0)
    args = (d["img"], d["gt"], d["rn"] if normal else None, d["sn"] if normal else None, d["dist"] if dist else None,
            d["weight"] if mode == "w" else None)
    tr, gr = loss_oracle.calculate_loss_torch(*args, ssim_pair=ssim_pair, **kw)
    ref_loss = float(tr["loss"])
    assert abs(loss - ref_loss) < 2e-6 * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
    got = terms[1:7].double().numpy()
    want = np.array([float(tr[k]) for k in ("Ll1", "ssim", "loss0", "normal", "dist", "psnr")])
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.all(got[~fin] == want[~fin]), (tag, got, want)   # psnr = inf: img == gt
    np.testing.assert_allclose(got[fin], want[fin], rtol=5e-6, atol=1e-6, err_msg=tag)
    np.testing.assert_allclose(terms[7:7 + C].double().numpy(), tr["mse"].numpy(), rtol=5e-6, atol=1e-12, err_msg=tag)
    assert torch.all(terms[7 + C:] == 0), tag
    # relative to the largest element, or to 1 / (C H W) (one pixel's L1 derivative) where every element is near zero: identical
    # images, whose float64 gradient is rounding noise
    e_img = _rel(g["image"] / UP, gr["image"], floor=1.0 / d["img"].numel())
    assert e_img < 2e-4, (tag, "image gradient", e_img)
    rows = {"loss": abs(loss - ref_loss) / max(1.0, abs(ref_loss)), "terms": float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-6))),
            "g_img": e_img}
    if normal:
        for k in ("rend_normal", "surf_normal"):
            rows["g_" + k] = _rel(g[k] / UP, gr[k])
            assert rows["g_" + k] < 1e-6, (tag, k, rows)
    else:
        assert g["rend_normal"] is None and g["surf_normal"] is None, tag
    if dist:
        rows["g_dist"] = _rel(g["rend_dist"] / UP, gr["rend_dist"])
        assert rows["g_dist"] < 1e-6, (tag, rows)
    if seam:
        # per-pixel error of the image gradient near the 32-pixel tile seams of loss_fwd_kernel / loss_bwd_kernel and inside the tiles,
        # both at least 16 pixels from the image border: the seams may not be worse than twice the tiles' inside (99.9th percentiles)
        err = ((g["image"] / UP).double() - gr["image"]).abs().amax(0)
        H, W = err.shape
        ys, xs = torch.arange(H) % 32, torch.arange(W) % 32
        near_y, near_x = (ys < 5) | (ys >= 27), (xs < 5) | (xs >= 27)
        near = near_y[:, None] | near_x[None, :]
        inner = torch.zeros(H, W, dtype=torch.bool)
        inner[16:H - 16, 16:W - 16] = True
        q_seam = float(torch.quantile(err[near & inner][::3].float(), 0.999))
        q_in = float(torch.quantile(err[~near & inner][::2].float(), 0.999))
        rows["seam_p999"], rows["inside_p999"] = q_seam, q_in
        assert q_seam <= 2.0 * q_in, (tag, q_seam, q_in)
    _report(tag, " ".join(f"{k}={v:.3g}" for k, v in rows.items()))
    return (tr["ssim_map"], gr["ssim"])


@pytest.mark.parametrize("H,W", [(800, 800), (1600, 1600), (779, 1037)])
def test_loss_at_production_sizes(H, W):
    """C = 3, lambda_dssim 0.2, both normal modes with the distortion term, (loss * 0.37).backward(); the SSIM part of the checker is
    evaluated once per size (it does not depend on the normal mode)."""
    d = _loss_inputs(3, H, W, seed=H + W)
    assert (d["img"] == d["gt"]).double().mean() > 0.1 and (d["gt"] == 0).any() and (d["gt"] == 1).any()
    pair = _check_loss(d, 0.2, "w", f"loss {H}x{W} weighted", seam=True)
    _check_loss(d, 0.2, "cos", f"loss {H}x{W} cosine", ssim_pair=pair)


RAGGED = [(1, 1), (1, 37), (37, 1), (5, 5), (10, 11), (11, 10), (31, 33), (32, 32), (33, 33), (64, 65)]


@pytest.mark.parametrize("H,W", RAGGED)
def test_loss_at_ragged_shapes(H, W):
    """Every C = 1..4 and lambda_dssim 0, 0.2, 1 (the l1_loss and ssim wrappers' settings included) on images below the window and the
    tile; the normal mode and the distortion term alternate.  For C >= 2 the last channel has img == gt: its PSNR is inf in both."""
    for C in (1, 2, 3, 4):
        d = _loss_inputs(C, H, W, seed=100 * C + H * 7 + W)
        if C >= 2:
            d["img"][-1] = d["gt"][-1]
        for i, lam in enumerate((0.0, 0.2, 1.0)):
            mode = ("w", "cos", "none")[(C + i) % 3]
            _check_loss(d, lam, mode, f"loss {H}x{W} C={C} dssim={lam} {mode}", dist=(C + i) % 2 == 0)


@pytest.mark.parametrize("H,W,parts", [(1024, 1024, 1024), (800, 1312, 1025)])
def test_loss_finalize_at_1024_and_1025_partial_rows(H, W, parts):
    """C = 1: the finalize kernel's outer loop (4 x 256 rows a step) ends exactly on its first step, or takes one more row."""
    assert ((W + 31) // 32) * ((H + 31) // 32) == parts
    d = _loss_inputs(1, H, W, seed=parts)
    _check_loss(d, 0.2, "w", f"loss {H}x{W} C=1 ({parts} partial rows)")


def test_l1_and_ssim_wrappers_at_size():
    """losses.l1_loss and losses.ssim (lambda_dssim 0 and 1) at 779 x 1037 against the checker, upstream scale 0.37."""
    from materialrefgs_amd import losses
    d = _loss_inputs(3, 779, 1037, seed=5)
    img, gt = d["img"].to(DEV).requires_grad_(True), d["gt"].to(DEV)
    l1 = losses.l1_loss(img, gt)
    (l1 * UP).backward()
    t1, g1 = loss_oracle.calculate_loss_torch(d["img"], d["gt"], lambda_dssim=0.0)
    assert abs(float(l1) - float(t1["Ll1"])) < 2e-6 * max(1.0, float(t1["Ll1"]))
    assert _rel(img.grad.cpu() / UP, g1["image"]) < 1e-6
    img.grad = None
    s = losses.ssim(img, gt)
    (s * UP).backward()
    ts, gs = loss_oracle.calculate_loss_torch(d["img"], d["gt"], lambda_dssim=1.0)
    assert abs(float(s) - float(ts["ssim"])) < 2e-6
    e = _rel(img.grad.cpu() / UP, -gs["image"])
    assert e < 2e-4, e
    _report("ssim wrapper 779x1037 g_img", f"{e:.3g}")


def test_loss_runs_are_bit_identical_at_1600():
    d = _loss_inputs(3, 1600, 1600, seed=9)
    runs = [_run_loss(d, 0.2, "w") for _ in range(2)]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k


@pytest.mark.parametrize("fn", ["fused_loss", "l1_loss", "ssim"])
def test_gt_that_requires_grad_is_refused(fn):
    """The backward forms no gradient for the second image: a gt that requires grad raises instead of getting a silent None."""
    from materialrefgs_amd import losses
    f = getattr(losses, fn)
    img, gt = torch.rand(3, 40, 40, device=DEV, requires_grad=True), torch.rand(3, 40, 40, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="requires grad"):
        f(img, gt)
    out = f(img, gt.detach())
    (out[0] if isinstance(out, tuple) else out).backward()
    assert img.grad is not None and gt.grad is None
    with torch.no_grad():                                      # no graph: nothing to refuse
        f(img, gt)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("H,W", [(800, 800), (1600, 1600), (779, 1037)])
def test_loss_abi_workspace_bound_and_argument_checks(H, W):
    """mrgs_loss_forward / _backward through ctypes: a workspace of exactly mrgs_loss_ws_bytes followed by a guard of random bytes that
    neither call touches; terms past the last channel's mse are zero; one byte less is MRGS_E_WORKSPACE; bad shapes and pointers a mode
    needs are MRGS_E_BAD_ARG, before anything runs.  The results equal those of losses.fused_loss."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    BAD, WS = 1, _lib.MRGS_E_WORKSPACE
    C = 3
    d = {k: v.to(DEV).contiguous() for k, v in _loss_inputs(C, H, W, seed=H * W).items()}
    need = L.mrgs_loss_ws_bytes(H, W, C)
    nb = ((W + 31) // 32) * ((H + 31) // 32) * C
    assert need == ((3 * C * H * W + 3) // 4 * 4 + nb * 8) * 4
    assert L.mrgs_loss_ws_bytes(0, W, C) == 0 and L.mrgs_loss_ws_bytes(H, W, 0) == 0
    G = 1 << 16
    buf = torch.randint(0, 256, (need + G,), dtype=torch.uint8, device=DEV)
    guard = buf[need:].clone()
    terms = torch.full((16,), float("nan"), device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    st = _lib.stream_ptr(DEV)
    cfg = _lib.MrgsLossConfig(H, W, C, 0.2, LAM["lambda_normal"], LAM["lambda_dist"])
    ins = [_p(d[k]) for k in ("img", "gt", "rn", "sn", "dist", "weight")]
    fwd = lambda c, ins_, n: L.mrgs_loss_forward(ctypes.byref(c), *ins_, _p(buf), n, _p(terms), _p(loss), st)   # noqa: E731
    assert fwd(cfg, ins, need - 1) == WS
    for h, w, c in ((H, W, 0), (H, W, 5), (0, W, C), (H, 0, C)):
        assert fwd(_lib.MrgsLossConfig(h, w, c, 0.2, LAM["lambda_normal"], LAM["lambda_dist"]), ins, need + G) == BAD, (h, w, c)
    for miss in (2, 3, 4):                                     # rend_normal, surf_normal, rend_dist
        assert fwd(cfg, [None if i == miss else p for i, p in enumerate(ins)], need) == BAD, miss
    torch.cuda.synchronize()
    assert torch.isnan(terms).all() and torch.equal(buf[need:], guard)           # refused calls wrote nothing
    assert fwd(cfg, ins, need) == 0
    g_img, g_rn, g_sn, g_d = torch.empty_like(d["img"]), torch.empty_like(d["rn"]), torch.empty_like(d["sn"]), torch.empty_like(d["dist"])
    gl = torch.full((1,), UP, device=DEV)
    bins = [_p(d[k]) for k in ("img", "gt", "rn", "sn", "weight")]
    bwd = lambda outs: L.mrgs_loss_backward(ctypes.byref(cfg), *bins, _p(buf), _p(gl), *outs, st)   # noqa: E731
    outs = [_p(g_img), _p(g_rn), _p(g_sn), _p(g_d)]
    for miss in range(4):                                      # g_image, g_rend_normal, g_surf_normal, g_rend_dist
        assert bwd([None if i == miss else p for i, p in enumerate(outs)]) == BAD, miss
    assert bwd(outs) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[need:], guard), "the loss kernels wrote past mrgs_loss_ws_bytes"
    assert torch.all(terms[7 + C:] == 0) and torch.isfinite(terms[:7 + C]).all()
    _, t_ref, g_ref = _run_loss({k: v.cpu() for k, v in d.items()}, 0.2, "w")
    assert torch.equal(terms.cpu(), t_ref) and float(loss) == float(t_ref[0])
    for a, k in ((g_img, "image"), (g_rn, "rend_normal"), (g_sn, "surf_normal"), (g_d, "rend_dist")):
        assert torch.equal(a.cpu(), g_ref[k]), k


# ---------------------------------------------------------------- B. maps kernel
def _maps_inputs(H, W, seed, cam):
    """allmap [7,H,W] and the "pgsr" plane distance [1,H,W] on the CPU: a smooth surface 3.1..3.9 deep with 2 % noise, camera-facing
    view normals scaled by alpha, holes (alpha = depth = 0: scattered and one disc) and ~2 % tiny alphas (1e-3 .. 1e-8)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    am = torch.rand(7, H, W, generator=g)
    am[1] = am[1] * 0.9 + 0.05
    tiny = torch.rand(H, W, generator=g) < 0.02
    am[1][tiny] = 10.0 ** (-3.0 - 5.0 * torch.rand(int(tiny.sum()), generator=g))
    depth = 3.5 + 0.4 * torch.sin(3 * xx + 1) * torch.cos(2 * yy) + 0.02 * torch.rand(H, W, generator=g)
    am[0] = am[1] * depth
    am[5] = depth + 0.01 * torch.rand(H, W, generator=g)
    nv = F.normalize(torch.stack([0.3 * torch.randn(H, W, generator=g), 0.3 * torch.randn(H, W, generator=g), -torch.ones(H, W)]), dim=0)
    am[2:5] = nv * am[1]
    am[6] = torch.rand(H, W, generator=g) * 1e-2
    hole = (torch.rand(H, W, generator=g) < 0.05) | (((xx - 0.3) ** 2 + (yy + 0.2) ** 2) < 0.05)
    am[:, hole] = 0.0
    # plane distance such that the unbiased depth is `depth` (up to 1 % noise): rd = depth * -(n . ray)
    fx, fy = W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5))   # renderer.pgsr_unbiased_depth's ray
    rx, ry = (torch.arange(W) - 0.5 * (W - 1)) / fx, (torch.arange(H) - 0.5 * (H - 1)) / fy
    ndr = am[2] * rx[None] + am[3] * ry[:, None] + am[4]
    rd = (-ndr * depth * (1 + 0.01 * torch.rand(H, W, generator=g)))[None]
    return am, rd


def _kappa(points, H, W, origin_norm):
    """Conditioning of the normalised cross product at every centre, from the float64 points [H,W,3]: |p| (|p| plus the camera's
    distance from the origin, the size of what fp32 rounds) x (|dx| + |dy|) / |dx x dy|; 0 where the product is exactly zero or the
    pixel is on the border.  The fp32 surf_normal of a centre is off by about U32 x kappa (the literal fp32 reference: <= 1.2)."""
    k = torch.zeros(H, W, dtype=torch.float64)
    if H < 3 or W < 3:
        return k
    dx = points[2:, 1:-1] - points[:-2, 1:-1]
    dy = points[1:-1, 2:] - points[1:-1, :-2]
    n = torch.cross(dx, dy, dim=-1).norm(dim=-1)
    P = F.max_pool2d(points.norm(dim=-1)[None, None], 3, 1, 1)[0, 0, 1:-1, 1:-1] + origin_norm
    kk = P * (dx.norm(dim=-1) + dy.norm(dim=-1)) / n
    kk[(dx.norm(dim=-1) == 0) | (dy.norm(dim=-1) == 0)] = 0.0
    kk[~torch.isfinite(kk)] = float("inf")
    k[1:-1, 1:-1] = kk
    return k


KAPPA_MAX = 1e5          # centres beyond: excluded (|dx x dy| at fp32 rounding level), at most 4e-4 of the pixels


def _check_maps(H, W, flavour, twin, tag, seed=3):
    from materialrefgs_amd.renderer import compute_2dgs_normal_and_regularizations, pgsr_unbiased_depth
    from materialrefgs_amd.synthetic import orbit_camera
    from oracle.glue_oracle import compute_2dgs_normal_and_regularizations_reference as reference, depths_to_points
    pgsr = flavour == "pgsr"
    pipe = SimpleNamespace(depth_ratio=0.0 if pgsr else float(flavour))
    cam = orbit_camera(3, H, W)
    am, rd = _maps_inputs(H, W, seed + H * 131 + W, cam)
    g = torch.Generator().manual_seed(seed)

    def ref_outputs(dt):
        c = cam._replace(world_view_transform=cam.world_view_transform.to(dt), full_proj_transform=cam.full_proj_transform.to(dt))
        a = am.to(dt).requires_grad_(True)
        r_ = rd.to(dt).requires_grad_(True)
        full = torch.cat([a, pgsr_unbiased_depth(a, r_, c)]) if pgsr else a
        ref = reference(full, c, pipe)
        nm = ref["render_normal"].permute(1, 2, 0) / ref["render_alpha"].permute(1, 2, 0).clamp_min(1e-6)
        outs = [ref["render_normal"], ref["surf_depth"], ref["surf_normal"], nm, ref["render_alpha"], ref["render_dist"]]
        if twin:
            outs.append(ref["render_alpha"])
        return outs, a, r_, c

    outs_c, am_c, rd_c, cam_c = ref_outputs(torch.float64)
    ups = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs_c]
    am_g = am.to(DEV).requires_grad_(True)
    rd_g = rd.to(DEV).requires_grad_(True) if pgsr else None
    out = compute_2dgs_normal_and_regularizations(am_g, cam.to(DEV), pipe, return_normal_map=True, rend_distance=rd_g, twin_alpha=twin)
    outs_g = [out["render_normal"], out["surf_depth"], out["surf_normal"], out["normal_map"], out["render_alpha"], out["render_dist"]]
    if twin:
        outs_g.append(out["render_alpha_twin"])
    # conditioning of surf_normal (float64 side)
    pts = depths_to_points(cam_c, outs_c[1].detach()).reshape(H, W, 3)
    kappa = _kappa(pts, H, W, float(cam_c.world_view_transform.inverse()[3, :3].norm()))
    excl = kappa > KAPPA_MAX
    frac = float(excl.double().mean())
    assert frac <= 4e-4, (tag, frac)
    rows = {"excluded": frac}
    names = ("render_normal", "surf_depth", "surf_normal", "normal_map", "render_alpha", "render_dist", "render_alpha_twin")
    for a, b, name in zip(outs_g, outs_c, names):
        a, b = a.detach().cpu().double(), b.detach()
        assert a.shape == b.shape, (tag, name)
        scale = max(1.0, float(b.abs().max()))
        if name == "surf_normal":
            # the existing bar, widened per centre to the first-order fp32 error of the normalised cross product (4 U32 kappa)
            e = (a - b).abs().amax(0)
            tol = 2e-5 * scale + 4 * U32 * kappa
            ok = (e <= tol) | excl
            rows["surf_normal"] = float(e[~excl].max())
            rows["surf_normal/tol"] = float((e / tol)[~excl].max())
            assert bool(ok.all()), (tag, name, rows)
        else:
            rows[name] = float((a - b).abs().max()) / scale
            assert rows[name] <= 2e-5, (tag, name, rows)
    if H < 3 or W < 3:
        assert torch.all(out["surf_normal"] == 0), tag
    torch.autograd.backward(outs_g, [u.float().to(DEV) for u in ups])
    torch.autograd.backward(outs_c, ups)
    ga = [am_g.grad.detach().cpu().double()] + ([rd_g.grad.detach().cpu().double()] if pgsr else [])
    gb = [am_c.grad] + ([rd_c.grad] if pgsr else [])
    # gradient pixels fed by an excluded centre: the centre and its four neighbours
    near = F.max_pool2d(excl[None, None].double(), 3, 1, 1)[0, 0] > 0 if H >= 3 and W >= 3 else torch.zeros(H, W, dtype=torch.bool)
    regular = (am[1] >= 0.05) & ~near                         # pixels whose gradients are not dominated by 1 / alpha^2

    def err_of(x, b, mask):
        return float((x - b)[mask].abs().max() / b[mask].abs().max()) if bool(mask.any()) and float(b[mask].abs().max()) > 0 else 0.0

    for j, (a, b) in enumerate(zip(ga, gb)):
        fin = torch.isfinite(b)
        assert torch.isfinite(a).all(), (tag, j)
        m_all = fin & ~near
        checks = [("g_all" if j == 0 else "g_rd", m_all)]
        if j == 0:
            checks += [(f"g_ch{c}_regular", m_all & regular[None] & (torch.arange(7)[:, None, None] == c)) for c in range(7)]
        else:
            checks += [("g_rd_regular", m_all & regular[None])]
        for key, m in checks:
            rows[key] = err_of(a, b, m)
            assert rows[key] <= 2e-4, (tag, key, rows)
    if H < 3 or W < 3:
        # no interior pixel: an upstream on surf_normal alone reaches nothing
        am2 = am.to(DEV).requires_grad_(True)
        rd2 = rd.to(DEV).requires_grad_(True) if pgsr else None
        o2 = compute_2dgs_normal_and_regularizations(am2, cam.to(DEV), pipe, rend_distance=rd2)
        (o2["surf_normal"] * torch.randn(o2["surf_normal"].shape, generator=g).to(DEV)).sum().backward()
        assert torch.all(am2.grad == 0) and (rd2 is None or torch.all(rd2.grad == 0)), tag
    _report(tag, " ".join(f"{k}={v:.3g}" for k, v in rows.items()))


@pytest.mark.parametrize("H,W,flavour,twin", [(800, 800, 0.3, True), (1600, 1600, 0.0, False), (1600, 1600, "pgsr", True),
                                               (779, 1037, 1.0, True), (779, 1037, "pgsr", False)])
def test_maps_at_production_sizes(H, W, flavour, twin):
    _check_maps(H, W, flavour, twin, f"maps {H}x{W} {flavour} twin={twin}")


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 3), (1, 40), (40, 1), (8, 32), (9, 33), (7, 31), (257, 129)])
def test_maps_at_ragged_shapes(H, W):
    """Narrower than the 32 x 8 tile, no interior pixel (H or W < 3), one interior pixel, one pixel past a tile: every flavour."""
    for i, flavour in enumerate((0.0, 0.3, 1.0, "pgsr")):
        _check_maps(H, W, flavour, i % 2 == 0, f"maps {H}x{W} {flavour} twin={i % 2 == 0}", seed=i)


# ---------------------------------------------------------------- C. compositing
@pytest.mark.parametrize("H,W", [(1600, 1600), (779, 1037)])
@pytest.mark.parametrize("srgb", [False, True])
def test_composite_at_size(H, W, srgb):
    """_SurfelComposite against the float64 torch expression of test_fused_composite_matches_the_reference_ops, random upstream on
    both outputs."""
    from materialrefgs_amd.gs_utils import linear_to_srgb
    from materialrefgs_amd.renderer import _SurfelComposite
    g = torch.Generator().manual_seed(H + W + srgb)
    base, spec = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g) * 0.5
    refl, alpha, bg = torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g), torch.tensor([0.1, 0.5, 0.9])
    dark = torch.rand(H, W, generator=g) < 0.05                              # the linear branch of the sRGB curve
    base[:, dark] *= 1e-3
    spec[:, dark] *= 1e-3
    tc = [t.double().requires_grad_(True) for t in (base, refl, spec, alpha)]
    tg = [t.to(DEV).requires_grad_(True) for t in (base, refl, spec, alpha)]
    diffuse_c = (1 - tc[1]) * tc[0]
    fin = diffuse_c + tc[2]
    if srgb:
        fin = linear_to_srgb(fin)
    render_c = fin + bg.double()[:, None, None] * (1 - tc[3])
    render_g, diffuse_g = _SurfelComposite.apply(tg[0], tg[1], tg[2], tg[3], bg.to(DEV), srgb)
    e_r = float((render_g.detach().cpu().double() - render_c.detach()).abs().max())
    e_d = float((diffuse_g.detach().cpu().double() - diffuse_c.detach()).abs().max())
    assert e_r <= 2e-6 and e_d <= 2e-6, (e_r, e_d)
    u1, u2 = torch.randn(3, H, W, generator=g, dtype=torch.float64), torch.randn(3, H, W, generator=g, dtype=torch.float64)
    torch.autograd.backward([render_c, diffuse_c], [u1, u2])
    torch.autograd.backward([render_g, diffuse_g], [u1.float().to(DEV), u2.float().to(DEV)])
    rows = {"render": e_r, "diffuse": e_d}
    for a, b, n in zip(tg, tc, ("base", "refl", "spec", "alpha")):
        rows["g_" + n] = float((a.grad.detach().cpu().double() - b.grad).abs().max()) / max(1.0, float(b.grad.abs().max()))
        assert rows["g_" + n] <= 2e-5, (n, rows)
    _report(f"composite {H}x{W} srgb={srgb}", " ".join(f"{k}={v:.3g}" for k, v in rows.items()))
