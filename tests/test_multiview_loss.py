"""materialrefgs_amd.multiview (csrc/mrgs_multiview.hip) against the float64 statement of tests/multiview_statement.py.

CPU: the statement's geometry on an analytic two-view scene (consistent depth -> e ~ 0, the plane homography lands where the depth
reprojection does), the C ABI's argument checks and the Python wrappers' errors.  GPU (-m gpu): the native op against the statement with
the native draw on the analytic scene and on render_surfel("pgsr") maps of the synthetic shell at 800^2, 1600^2 and 779x1037; the sampler;
no host read; the edge cases; run-to-run identity of the forward; an end-to-end step whose leaf gradients add up.
Bars: scalars 1e-5 relative, the weight map 1e-5, every texel of every gradient map within 1e-4 of the map's largest element, except
the texels touched by a tap or sample the statement marks as within its derived delta of a decision an fp32 evaluation can take
differently (tests/multiview_statement.py: a sign of |b - b'| / |m - M| / |r - min|, an ill-conditioned projective division, L's
knee); those are counted and must stay at or below 5e-3 of the map's touched texels (64 on the small scenes).  Measured: every other
texel within 6e-7 of the map's largest element; 4.3e-3 of the touched neighbour texels excluded at 800^2, 2.2e-3 at 779x1037.
"""
import ctypes
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiview_statement as ms  # noqa: E402
from materialrefgs_amd.camera import look_at_camera, fov2focal  # noqa: E402


from multiview_statement import analytic_pair  # noqa: E402


def _intr(cam):
    """Fx, Fy, Cx, Cy rounded to float32: the reference multiplies float32 tensors by them, so they enter its arithmetic at float32."""
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


def _stmt_inputs(v, n, dev, dtype=torch.float64):
    f = lambda t: t.to(dev, dtype)
    return dict(D_v=f(v.depth), D_n=f(n.depth), N_v=f(v.normal), dist_v=f(v.distance), base_v=f(v.base), m_v=f(v.metal), r_v=f(v.rough),
                base_n=f(n.base), m_n=f(n.metal), r_n=f(n.rough), fg=f(v.fg), cam_v=ms.camera_record(v.cam, dtype, dev),
                cam_n=ms.camera_record(n.cam, dtype, dev), intr_v=_intr(v.cam), intr_n=_intr(n.cam))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_statement_geometry_on_the_analytic_scene():
    """Exact depths: the reprojection error vanishes where both views see the same surface, and the plane homography of a sample sends
    its centre where the depth reprojection does (the homography convention of the statement is the geometric one)."""
    v, n = analytic_pair(48, 64, noise=0.0)
    inp = _stmt_inputs(v, n, "cpu")
    e, valid, w, u = ms.geometry(inp["D_v"], inp["D_n"], inp["cam_v"], inp["cam_n"], inp["intr_v"], inp["intr_n"])
    assert int(valid.sum()) > 0.4 * 48 * 64
    assert float(e[valid].median()) < 1e-3
    assert torch.allclose(w[valid], torch.exp(-e[valid]))
    samples = torch.nonzero(valid.reshape(-1))[:, 0][::7]
    Hs = ms.homographies(inp["N_v"], inp["dist_v"], inp["cam_v"], inp["cam_n"], inp["intr_v"], inp["intr_n"], samples)
    xs, ys = (samples % 64).double(), (samples // 64).double()
    g = torch.einsum("sij,sj->si", Hs, torch.stack([xs, ys, torch.ones_like(xs)], -1))
    g = g[:, :2] / g[:, 2:]
    err = (g - u.reshape(-1, 2)[samples]).norm(dim=-1)
    assert float(err.median()) < 1e-2, float(err.median())


def test_statement_terms_and_gradients_are_finite():
    v, n = analytic_pair(32, 40)
    inp = _stmt_inputs(v, n, "cpu")
    for k in ("D_v", "D_n", "base_v", "m_v", "r_v", "base_n", "m_n", "r_n"):
        inp[k].requires_grad_(True)
    e, valid, _w, _u = ms.geometry(inp["D_v"], inp["D_n"], inp["cam_v"], inp["cam_n"], inp["intr_v"], inp["intr_n"])
    samples = torch.nonzero(valid.reshape(-1))[:, 0]
    o = ms.warp_loss(**inp, keep=None, samples=samples, geo_w=0.03, base_w=0.015, metal_w=0.025, rough_w=0.025)
    tot = o["geo"] + o["base"] + o["metal"] + o["rough"]
    tot.backward()
    assert torch.isfinite(tot)
    for k in ("D_v", "D_n", "base_n", "m_n", "r_n"):
        assert torch.isfinite(inp[k].grad).all() and float(inp[k].grad.abs().max()) > 0, k
    for k in ("base_v", "m_v", "r_v"):                # sampled under no_grad by the reference (train_refnerf.py:510-559)
        assert inp[k].grad is None, k


def _cfg(**kw):
    from materialrefgs_amd import _lib
    c = _lib.MrgsWarpConfig(48, 64, 1000, 3, -1, _lib.MRGS_WARP_MATERIAL, 1, 2, 50.0, 50.0, 32.0, 24.0, 50.0, 50.0, 32.0, 24.0, 1.0, 0.03, 0.015,
                            0.025, 0.025)
    for k, val in kw.items():
        setattr(c, k, val)
    return c


def test_warp_abi_argument_checks_without_gpu():
    """Every contract violation is MRGS_E_BAD_ARG (or _WORKSPACE) before anything is launched."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    assert L.mrgs_warp_loss_ws_bytes(48, 64, 1000, 3) > 48 * 64 * 5 + 1000 * 88
    assert L.mrgs_warp_loss_ws_bytes(48, 64, 1000, 4) == 0
    assert L.mrgs_warp_loss_ws_bytes(0, 64, 1000, 3) == 0
    assert L.mrgs_warp_loss_ws_bytes(48, 64, 0, 1) == 0
    p = ctypes.c_void_p(0x1000)                       # never dereferenced: every call below is refused
    maps = _lib.MrgsWarpMaps(*([p] * 11 + [None, p, p]))
    big = 1 << 30

    def fwd(cfg, m=maps, ws_bytes=big):
        return L.mrgs_warp_loss_forward(ctypes.byref(cfg), ctypes.byref(m), None, p, ws_bytes, p, p, p, None)

    def bwd(cfg, m=maps):
        return L.mrgs_warp_loss_backward(ctypes.byref(cfg), ctypes.byref(m), p, p, p, *([None] * 8), None)

    bad = _cfg()
    bad.struct_size -= 4
    assert fwd(bad) == 1 and bwd(bad) == 1
    for kw in (dict(patch_half=0), dict(patch_half=4), dict(sample_num=0), dict(H=0), dict(n_given=1001), dict(n_given=-2),
               dict(flags=_lib.MRGS_WARP_METALLIC), dict(flags=16), dict(fx_v=0.0), dict(fy_n=-1.0), dict(cx_v=float("nan"))):
        assert fwd(_cfg(**kw)) == 1, kw
        assert bwd(_cfg(**kw)) == 1, kw
    assert fwd(_cfg(n_given=5)) == 1                  # given samples without the list
    m2 = _lib.MrgsWarpMaps(*([p] * 11 + [None, p, p]))
    m2.fg_v = None
    assert fwd(_cfg(), m2) == 1                       # the material terms need the foreground mask
    m3 = _lib.MrgsWarpMaps(*([p] * 11 + [None, p, p]))
    m3.metal_n = None
    assert fwd(_cfg(flags=_lib.MRGS_WARP_MATERIAL | _lib.MRGS_WARP_METALLIC), m3) == 1
    m4 = _lib.MrgsWarpMaps(*([p] * 11 + [None, p, None]))
    assert fwd(_cfg(flags=0), m4) == 1                # cameras are always needed
    need = L.mrgs_warp_loss_ws_bytes(48, 64, 1000, 3)
    assert fwd(_cfg(), ws_bytes=need - 1) == 5


def _cpu_pkg(v):
    return {"surf_depth": v.depth[None], "rend_normal": v.normal, "rend_distance": v.distance[None], "diffuse_map": v.base,
            "refl_strength_map": v.metal[None], "roughness_map": v.rough[None]}


def test_wrapper_errors():
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(16, 20)
    with pytest.raises(RuntimeError, match="device tensors"):
        mv.warp_consistency_loss(v.cam, _cpu_pkg(v), n.cam, _cpu_pkg(n), v.fg, iteration=20000, seed=1)
    opt = SimpleNamespace(use_virtul_cam=True, wo_use_geo_occ_aware=False, edge_aware_in_warp=False, directional_rghmtl_warp_alignment=True)
    cam = SimpleNamespace(ncc_scale=1.0, nearest_id=[0], image_name="a")
    args = (None, opt, None, None, None, None, _cpu_pkg(v), None, None, None, {}, 20000, None, None)
    with pytest.raises(NotImplementedError, match="use_virtul_cam"):
        mv.calc_warp_loss(cam, *args)
    opt.use_virtul_cam = False
    opt.wo_use_geo_occ_aware = True
    with pytest.raises(NotImplementedError, match="wo_use_geo_occ_aware"):
        mv.calc_warp_loss(cam, *args)
    opt.wo_use_geo_occ_aware = False
    with pytest.raises(NotImplementedError, match="ncc_scale"):
        mv.calc_warp_loss(SimpleNamespace(ncc_scale=2.0, nearest_id=[0], image_name="a"), *args)
    opt.directional_rghmtl_warp_alignment = False
    with pytest.raises(NotImplementedError, match="directional_rghmtl_warp_alignment"):
        mv.calc_warp_loss_refreal(cam, *args, without_ncc=True)
    with pytest.raises(NotImplementedError, match="without_ncc"):     # train_refreal.py's NCC term is not built
        mv.calc_warp_loss_refreal(cam, *args)
    # refnerf sets the switch itself (train_refnerf.py:648): the same arguments reach the device-tensor check instead
    with pytest.raises(RuntimeError, match="device tensors"):
        mv.calc_warp_loss(cam, *args)
    assert mv.basecolor_weight(8000, "refreal") == 4.0 and mv.basecolor_weight(16000, "refreal") == pytest.approx(2.75)
    assert mv.basecolor_weight(30000, "refreal") == 1.5 and mv.basecolor_weight(30000, "refnerf") == 0.1
    assert mv.mtlrgh_weight(15000, "refreal") == 1.0 and mv.mtlrgh_weight(30000, "refnerf") == 0.5


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _dev_pkg(v, dev, grad=False):
    pkg = {k: t.to(dev).clone() for k, t in _cpu_pkg(v).items()}
    if grad:
        for k in ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map"):
            pkg[k].requires_grad_(True)
    return pkg


GRAD_KEYS = (("surf_depth", "D"), ("diffuse_map", "base"), ("refl_strength_map", "m"), ("roughness_map", "r"))
KW = dict(geo_weight=0.03, ncc_weight=0.15, metallic_weight=0.05, roughness_weight=0.05)


def _native(vc, vp, nc, npk, fg, keep=None, iteration=30000, seed=7, schedule="refreal", **kw):
    from materialrefgs_amd import multiview as mv
    dev = vp["surf_depth"].device
    smp = torch.full((kw.get("sample_num", 102400),), -1, dtype=torch.int32, device=dev)
    args = dict(KW, **kw)
    r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, keep, iteration=iteration, seed=seed, out_samples=smp if "samples" not in kw else None,
                                 schedule=schedule, **args)
    return r, smp


def _statement_for(vc, vp, nc, npk, fg, keep, samples, iteration=30000, schedule="refreal", patch_size=3, use_metallic_warp=True,
                   use_roughness_warp=True, **_):
    from materialrefgs_amd import multiview as mv
    dev = vp["surf_depth"].device
    H, W = vp["surf_depth"].shape[-2:]
    f = lambda t: t.detach().to(torch.float64).reshape(-1, H, W).squeeze(0).clone().requires_grad_(True)
    leaves = {"D_v": f(vp["surf_depth"]), "D_n": f(npk["surf_depth"]), "base_v": f(vp["diffuse_map"]), "m_v": f(vp["refl_strength_map"]),
              "r_v": f(vp["roughness_map"]), "base_n": f(npk["diffuse_map"]), "m_n": f(npk["refl_strength_map"]), "r_n": f(npk["roughness_map"])}
    a, b = mv.basecolor_weight(iteration, schedule), mv.mtlrgh_weight(iteration, schedule)
    o = ms.warp_loss(**leaves, N_v=vp["rend_normal"].detach().double(), dist_v=vp["rend_distance"].detach().double().reshape(H, W),
                     fg=fg.double().reshape(H, W), keep=keep, cam_v=ms.camera_record(vc, device=dev), cam_n=ms.camera_record(nc, device=dev),
                     intr_v=_intr(vc), intr_n=_intr(nc), samples=samples, patch_half=patch_size, geo_w=KW["geo_weight"],
                     base_w=a * KW["ncc_weight"], metal_w=b * KW["metallic_weight"], rough_w=b * KW["roughness_weight"],
                     material=iteration > 10000, metallic=use_metallic_warp, roughness=use_roughness_warp)
    return o, leaves


def _compare(vc, vp, nc, npk, fg, keep=None, grads=True, **kw):
    """Native op vs statement with the native draw: scalars, weight map, every gradient map (random upstream on the four terms)."""
    (geo, base, metal, rough, weight, nv), smp = _native(vc, vp, nc, npk, fg, keep, **kw)
    n_sel = min(int(nv), kw.get("sample_num", 102400)) if kw.get("iteration", 30000) > 10000 else 0
    samples = smp[:n_sel].long()
    assert bool((samples >= 0).all())
    o, leaves = _statement_for(vc, vp, nc, npk, fg, keep, samples, **kw)
    assert int(nv) == o["n_valid"]
    assert float((weight.double() - o["weight"]).abs().max()) < 1e-5
    errs = {}
    for name, mine, ref in (("geo", geo, o["geo"]), ("base", base, o["base"]), ("metal", metal, o["metal"]), ("rough", rough, o["rough"])):
        r = float(ref.detach())
        if math.isnan(r):
            assert math.isnan(float(mine)), name
            continue
        errs[name] = abs(float(mine) - r) / max(abs(r), 1e-30)
        assert errs[name] < 1e-5 or abs(float(mine) - r) < 1e-12, (name, float(mine), r)
    if not grads:
        return errs, o
    gen = torch.Generator().manual_seed(3)
    up = torch.rand(4, generator=gen).double() + 0.5
    dev = weight.device
    terms = [geo, base, metal, rough]
    live = [i for i in range(4) if terms[i].requires_grad and math.isfinite(float(terms[i]))]
    torch.autograd.backward([terms[i] for i in live], [up[i].float().to(dev) for i in live])
    live_ref = [i for i in live if o[("geo", "base", "metal", "rough")[i]].requires_grad]
    if live_ref:
        torch.autograd.backward([o[("geo", "base", "metal", "rough")[i]] for i in live_ref], [up[i].to(dev) for i in live_ref])
    pairs = (("surf_depth", "D_v", vp), ("surf_depth", "D_n", npk), ("diffuse_map", "base_v", vp), ("refl_strength_map", "m_v", vp),
             ("roughness_map", "r_v", vp), ("diffuse_map", "base_n", npk), ("refl_strength_map", "m_n", npk), ("roughness_map", "r_n", npk))
    for key, lk, pkg in pairs:
        g = pkg[key].grad
        gr = leaves[lk].grad
        if gr is None or float(gr.abs().max()) == 0:
            assert g is None or float(g.abs().max()) == 0, lk
            continue
        d = (g.double().reshape(gr.shape) - gr).abs()
        scale = float(gr.abs().max())
        H, W = gr.shape[-2:]
        excl = torch.zeros(H, W, dtype=torch.bool, device=gr.device)
        if lk not in ("D_v", "D_n") and o["excl_tap"] is not None:
            et = o["excl_tap"] | o["excl_sample"][:, None]
            if lk.endswith("_v"):
                tx, ty = o["tx"][et], o["ty"][et]
                ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                excl.view(-1)[(ty[ok] * W + tx[ok])] = True
            else:
                G = o["g"][et]
                ok = torch.isfinite(G).all(-1) & (G[:, 0] > -2) & (G[:, 0] < W + 1) & (G[:, 1] > -2) & (G[:, 1] < H + 1)
                x0, y0 = G[ok, 0].floor().long(), G[ok, 1].floor().long()
                for dx in (0, 1):
                    for dy in (0, 1):
                        xx, yy = x0 + dx, y0 + dy
                        inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                        excl.view(-1)[yy[inb] * W + xx[inb]] = True
        touched_map = (gr != 0).reshape(-1, H, W).any(0)
        touched = int(touched_map.sum())
        n_excl = int((excl & touched_map).sum())
        bad = (d.reshape(-1, H, W) > 1e-4 * scale).any(0) & ~excl
        errs[lk] = (float(d.reshape(-1, H, W).amax(0)[~excl].max()) / scale, n_excl, touched)
        assert int(bad.sum()) == 0, (lk, errs[lk], int(bad.sum()))
        # measured: 4.3e-3 of the touched neighbour texels at 800^2, 2.2e-3 at 779x1037, up to 49 texels on the small analytic scenes
        assert n_excl <= max(64, 5e-3 * touched), (lk, errs[lk])
    return errs, o


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,k", [(48, 64, 100000), (48, 64, 300), (61, 83, 700)])
def test_analytic_scene_against_statement(gpu_device, H, W, k):
    v, n = analytic_pair(H, W)
    dev = gpu_device
    vc, nc = v.cam.to(dev), n.cam.to(dev)
    errs, o = _compare(vc, _dev_pkg(v, dev, True), nc, _dev_pkg(n, dev, True), v.fg.to(dev), sample_num=k)
    assert o["n_valid"] > 0.3 * H * W
    print(H, W, k, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("iteration,schedule", [(30000, "refnerf"), (15000, "refreal"), (8000, "refreal")])
def test_schedules_and_keep_mask(gpu_device, iteration, schedule):
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    keep = torch.rand(48, 64, generator=torch.Generator().manual_seed(1)).to(dev) > 0.3
    _compare(v.cam.to(dev), _dev_pkg(v, dev, True), n.cam.to(dev), _dev_pkg(n, dev, True), v.fg.to(dev), keep, iteration=iteration,
             schedule=schedule, sample_num=500)


@pytest.mark.gpu
@pytest.mark.parametrize("patch_size", [1, 2])
def test_small_patches(gpu_device, patch_size):
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    _compare(v.cam.to(dev), _dev_pkg(v, dev, True), n.cam.to(dev), _dev_pkg(n, dev, True), v.fg.to(dev), patch_size=patch_size, sample_num=800)


@pytest.mark.gpu
@pytest.mark.parametrize("m,r", [(False, True), (True, False), (False, False)])
def test_terms_switched_off(gpu_device, m, r):
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    (geo, base, metal, rough, _w, _n), _ = _native(v.cam.to(dev), vp, n.cam.to(dev), npk, v.fg.to(dev), use_metallic_warp=m,
                                                   use_roughness_warp=r, sample_num=500)
    assert (float(metal) != 0) == m and (float(rough) != 0) == r
    _compare(v.cam.to(dev), _dev_pkg(v, dev, True), n.cam.to(dev), _dev_pkg(n, dev, True), v.fg.to(dev), use_metallic_warp=m,
             use_roughness_warp=r, sample_num=500)


@pytest.mark.gpu
def test_given_samples_replay(gpu_device):
    """A caller-supplied draw (how the reference's np.random.choice is replayed), in a random order."""
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    _e, valid, _w, _u = ms.geometry(*[t.to(dev, torch.float64) for t in (v.depth, n.depth)], ms.camera_record(v.cam, device=dev),
                                     ms.camera_record(n.cam, device=dev), _intr(v.cam), _intr(n.cam))
    idx = torch.nonzero(valid.reshape(-1))[:, 0]
    pick = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(4))[:400].to(dev)]
    r = mv.warp_consistency_loss(v.cam.to(dev), vp, n.cam.to(dev), npk, v.fg.to(dev), iteration=30000, seed=0, samples=pick.int(),
                                 sample_num=400, schedule="refreal", **KW)
    o, _ = _statement_for(v.cam.to(dev), vp, n.cam.to(dev), npk, v.fg.to(dev), None, pick)
    for mine, ref in zip(r[:4], (o["geo"], o["base"], o["metal"], o["rough"])):
        assert abs(float(mine) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-12


@pytest.mark.gpu
def test_sampler(gpu_device):
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    vp, npk, fg = _dev_pkg(v, dev), _dev_pkg(n, dev), v.fg.to(dev)
    vc, nc = v.cam.to(dev), n.cam.to(dev)

    def draw(seed, k):
        smp = torch.full((k,), -1, dtype=torch.int32, device=dev)
        r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=30000, seed=seed, sample_num=k, out_samples=smp)
        return smp, r[4], int(r[5])

    smp, weight, nv = draw(1, 500)
    valid = (weight > 0).reshape(-1)
    assert nv == int(valid.sum()) > 500
    s = smp.long()
    assert bool((s >= 0).all()) and torch.unique(s).numel() == 500 and bool(valid[s].all())
    assert bool((s[1:] > s[:-1]).all())                                   # ascending pixel order
    assert torch.equal(draw(1, 500)[0], smp)
    assert not torch.equal(draw(2, 500)[0], smp)
    allv, _, _ = draw(3, nv + 10)
    assert torch.equal(allv[:nv].long(), torch.nonzero(valid)[:, 0])
    # inclusion frequencies over many seeds: chi-square against the uniform k / n_valid
    k, seeds = 200, 400
    counts = torch.zeros(48 * 64, dtype=torch.float64, device=dev)
    for sd in range(seeds):
        counts.index_add_(0, draw(1000 + sd, k)[0].long(), torch.ones(k, dtype=torch.float64, device=dev))
    c = counts[valid]
    p = k / nv
    expect = seeds * p
    chi2 = float(((c - expect) ** 2 / (expect * (1 - p))).sum())
    dof = nv - 1
    assert abs(chi2 - dof) < 5 * math.sqrt(2 * dof), (chi2, dof)


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    vp, npk, fg = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True), v.fg.to(dev)
    vc, nc = v.cam.to(dev), n.cam.to(dev)
    keep = torch.ones(48, 64, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, keep, iteration=30000, seed=5, sample_num=1000, schedule="refreal", **KW)
        (r[0] + r[1] + r[2] + r[3]).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(npk["diffuse_map"].grad.abs().max()) > 0 and float(npk["surf_depth"].grad.abs().max()) > 0


@pytest.mark.gpu
def test_edge_cases(gpu_device):
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(48, 64)
    dev = gpu_device
    vc, nc = v.cam.to(dev), n.cam.to(dev)
    # no valid pixel (the neighbour sees nothing at those depths): zeros and zero gradients
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    with torch.no_grad():
        npk["surf_depth"].zero_()
    r = mv.warp_consistency_loss(vc, vp, nc, npk, v.fg.to(dev), iteration=30000, seed=1, schedule="refreal", **KW)
    assert int(r[5]) == 0 and all(float(t) == 0 for t in r[:4]) and float(r[4].abs().max()) == 0
    sum(r[:4]).backward()
    for k in ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map"):
        for pkg in (vp, npk):
            assert pkg[k].grad is None or float(pkg[k].grad.abs().max()) == 0, k
    # an empty keep set: metallic and roughness are NaN as in the reference, the gradients stay finite
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    r = mv.warp_consistency_loss(vc, vp, nc, npk, v.fg.to(dev) * 0.5, iteration=30000, seed=1, sample_num=500, **KW)
    assert math.isnan(float(r[2])) and math.isnan(float(r[3])) and float(r[1]) > 0
    (r[0] + r[1]).backward()
    assert bool(torch.isfinite(npk["diffuse_map"].grad).all()) and float(npk["diffuse_map"].grad.abs().max()) > 0
    _compare(vc, _dev_pkg(v, dev, True), nc, _dev_pkg(n, dev, True), v.fg.to(dev) * 0.5, sample_num=500)
    # rend_distance = 0: every neighbour tap samples zero, no NaN anywhere
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    vp["rend_distance"] = torch.zeros_like(vp["rend_distance"])
    r = mv.warp_consistency_loss(vc, vp, nc, npk, v.fg.to(dev), iteration=30000, seed=1, sample_num=500, schedule="refreal", **KW)
    sum(r[:4]).backward()
    for k in ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map"):
        for pkg in (vp, npk):
            assert pkg[k].grad is None or bool(torch.isfinite(pkg[k].grad).all()), k
    assert float(npk["diffuse_map"].grad.abs().max()) == 0
    _compare(vc, vp | {k: vp[k].detach().clone().requires_grad_(True) for k in ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map")},
             nc, _dev_pkg(n, dev, True), v.fg.to(dev), sample_num=500)
    # iteration <= 10000: only the geometric term
    vp, npk = _dev_pkg(v, dev, True), _dev_pkg(n, dev, True)
    r = mv.warp_consistency_loss(vc, vp, nc, npk, v.fg.to(dev), iteration=10000, seed=1, schedule="refreal", **KW)
    assert float(r[0]) > 0 and float(r[1]) == 0 and float(r[2]) == 0 and float(r[3]) == 0
    _compare(vc, _dev_pkg(v, dev, True), nc, _dev_pkg(n, dev, True), v.fg.to(dev), iteration=10000)


@pytest.mark.gpu
def test_forward_is_bitwise_repeatable(gpu_device):
    from materialrefgs_amd import multiview as mv
    v, n = analytic_pair(61, 83)
    dev = gpu_device
    vp, npk, fg = _dev_pkg(v, dev), _dev_pkg(n, dev), v.fg.to(dev)
    runs = [mv.warp_consistency_loss(v.cam.to(dev), vp, n.cam.to(dev), npk, fg, iteration=30000, seed=9, sample_num=1500,
                                     schedule="refreal", **KW) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)


# ---- at size: render_surfel("pgsr") maps of the synthetic shell ------------------------------------------------------------------------
PIPE = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)


def _render_pair(dev, H, W, P=300_000, grad=False):
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    pc, env, leaves = make_surfel_model(P, max(H, W), dev)
    cams = [orbit_camera(v, H, W, n_views=96).to(dev) for v in (0, 1)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    env.build_mips()
    ctx = torch.enable_grad() if grad else torch.no_grad()
    with ctx:
        pk = [render_surfel(c, pc, PIPE, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr") for c in cams]
    return cams, pk, (pc, env, leaves, bg)


def _leafify(pkg):
    out = dict(pkg)
    for k in ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map"):
        out[k] = pkg[k].detach().clone().requires_grad_(True)
    for k in ("rend_normal", "rend_distance", "rend_alpha"):
        out[k] = pkg[k].detach()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(800, 800), (1600, 1600), (779, 1037)])
def test_at_size_against_float64(gpu_device, H, W):
    dev = gpu_device
    cams, pk, _ = _render_pair(dev, H, W)
    vp, npk = _leafify(pk[0]), _leafify(pk[1])
    fg = (vp["rend_alpha"] > 0.5).float().reshape(H, W)
    errs, o = _compare(cams[0], vp, cams[1], npk, fg, sample_num=102400)
    assert o["n_valid"] > 102400 // 4, o["n_valid"]
    print(H, W, o["n_valid"], errs)


@pytest.mark.gpu
def test_end_to_end_leaf_gradients_add_up(gpu_device):
    """image loss + warp loss on render_surfel("pgsr") maps: the leaf gradients of one backward equal the sum of the two losses' separate
    backward passes (the material maps have a second reader: _SplitChannels / the fused epilogue must not alias their gradients)."""
    from materialrefgs_amd import multiview as mv
    from materialrefgs_amd.losses import fused_loss
    from materialrefgs_amd.renderer import render_surfel
    dev = gpu_device
    H = W = 128
    cams, _pk, (pc, env, leaves, bg) = _render_pair(dev, H, W, P=20000)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).to(dev)

    def step(which):
        for t in leaves:
            t.grad = None
        env.build_mips()
        pk = [render_surfel(c, pc, PIPE, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr") for c in cams]
        fg = (pk[0]["rend_alpha"].detach() > 0.5).float().reshape(H, W)
        r = mv.warp_consistency_loss(cams[0], pk[0], cams[1], pk[1], fg, iteration=30000, seed=3, sample_num=4000, schedule="refreal", **KW)
        warp = r[0] + r[1] + r[2] + r[3]
        img = fused_loss(pk[0]["render"], gt)[0]
        loss = {"both": img + warp, "img": img, "warp": warp}[which]
        loss.backward()
        return [None if t.grad is None else t.grad.clone() for t in leaves], float(warp)

    both, wv = step("both")
    assert math.isfinite(wv) and wv > 0
    img, _ = step("img")
    warp, _ = step("warp")
    img2, _ = step("img")                      # run-to-run spread of each backward alone (float atomics: the summation order varies)
    warp2, _ = step("warp")
    touched = 0
    for b, i, w, i2, w2 in zip(both, img, warp, img2, warp2):
        if b is None:
            continue
        z = lambda t: 0 if t is None else t
        s = z(i) + z(w)
        scale = max(float(b.abs().max()), 1e-30)
        spread = float((z(i) - z(i2)).abs().max() if i is not None else 0) + float((z(w) - z(w2)).abs().max() if w is not None else 0)
        # measured: 1.2e-6 of the largest element, run-to-run spread 1.3e-7: the rasterizer's fp32 backward applied to the summed
        # upstream is not bit-linear; the bar is 1e-5 and the spread is asserted to stay far below it
        assert float((b - s).abs().max()) <= 1e-5 * scale + 1e-12, (float((b - s).abs().max()) / scale, spread / scale)
        assert spread <= 1e-6 * scale + 1e-12, spread / scale
        touched += int(w is not None and float(w.abs().max()) > 0)
    assert touched > 0
