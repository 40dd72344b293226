"""The grey-image patch NCC term of the multi-view loss (csrc/mrgs_multiview.hip: warp_ncc_fwd / _finalize / _bwd, behind
materialrefgs_amd.multiview.warp_consistency_loss(grey_v=, grey_n=) and calc_warp_loss_refreal) against the float64 statement of
tests/multiview_ncc_statement.py and against tests/golden/reference_ncc.npz, the reference's own train_refreal.py functions run in
float64 by tests/golden/gen_reference_ncc_vectors.py.

CPU: the statement against every fixture case (scalar 1e-10 relative, gradients 1e-6 of the map's maximum: the fixture is float32 -- the
bars of test_multiview_reference.py); the C ABI's argument checks; the conditions on the analytic inputs; the wrapper's image lookup.
GPU (-m gpu): the native term against the statement with the native draw on the analytic scene at 48x64 / 61x83 and at 800^2, 1600^2 and
779x1037 with N = 102 400; the drop-in against the fixture; repeatability, no host read, the empty cases, the image border, the draw;
one render_surfel("pgsr") pair end to end.
Bars (those of the sibling terms): the scalar 1e-5 relative, the ref_weight map 1e-5, the counts exact, every texel of both gradient maps
within 1e-4 of the map's largest element, none excluded.  use_s may differ from float64 only on the statement's ambiguous set A
(delta = 1e-5, at most max(4, 1e-4 samples) samples); the statement is evaluated with the kernel's decisions on A.  Every at-size case
must use at least 10 % of its samples.
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
import multiview_ncc_statement as mn  # noqa: E402
from materialrefgs_amd.camera import MiniCam, fov2focal  # noqa: E402

Z0 = np.load(os.path.join(ROOT, "tests", "golden", "reference_warp.npz"))
Z = np.load(os.path.join(ROOT, "tests", "golden", "reference_ncc.npz"))
CASES = sorted({k[: -len("_meta")] for k in Z.files if k.endswith("_meta")})
KW = dict(geo_weight=0.03, ncc_weight=0.15, metallic_weight=0.05, roughness_weight=0.05)
DELTA = 1e-5


def _intr(cam):
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def _cam(s, i, dev):
    c = torch.from_numpy(Z0[f"{s}_{i}_cam"])
    H, W = Z0[f"{s}_{i}_depth"].shape
    f = lambda t: t.to(torch.float32).to(dev)
    return MiniCam(H, W, float(c[-2]), float(c[-1]), 0.01, 100.0, f(c[:16].reshape(4, 4)), f(torch.eye(4)), f(torch.zeros(3)),
                   f(c[16:25].reshape(3, 3)), f(c[25:28]))


def _case(name, dev, dtype):
    it, k, metal_scale, dscale, patch = Z[f"{name}_meta"]
    s = str(Z[f"{name}_scene"])
    f = lambda key, z=Z0: torch.from_numpy(z[key]).to(dev, dtype)
    H, W = Z0[f"{s}_0_depth"].shape
    pk = []
    for i in (0, 1):
        pk.append({"surf_depth": f(f"{s}_{i}_depth")[None] * (dscale if i == 1 else 1.0), "rend_normal": f(f"{s}_{i}_normal"),
                   "rend_distance": f(f"{s}_{i}_distance")[None], "diffuse_map": f(f"{s}_{i}_base"),
                   "refl_strength_map": f(f"{s}_{i}_metal")[None] * metal_scale, "roughness_map": f(f"{s}_{i}_rough")[None]})
    for key in ("rend_normal", "rend_distance"):
        pk[0][key] = pk[0][key].clone().requires_grad_(True)
    keep = torch.from_numpy(np.unpackbits(Z[f"{name}_keep"])[: H * W].reshape(H, W)).to(dev).bool()
    return SimpleNamespace(it=int(it), k=int(k), patch=int(patch), pk=pk, cams=[_cam(s, i, dev) for i in (0, 1)], fg=f(f"{s}_0_fg"),
                           grey=[f(f"{s}_{i}_grey", Z) for i in (0, 1)], keep=keep, H=H, W=W)


def _samples(c, name):
    dev = c.fg.device
    H, W = c.H, c.W
    d = lambda t: t.detach().double().reshape(H, W)
    _e, valid, w, _u = ms.geometry(d(c.pk[0]["surf_depth"]), d(c.pk[1]["surf_depth"]), ms.camera_record(c.cams[0], device=dev),
                                    ms.camera_record(c.cams[1], device=dev), _intr(c.cams[0]), _intr(c.cams[1]))
    vidx = torch.nonzero(valid.reshape(-1))[:, 0]
    samples = vidx[torch.from_numpy(Z[f"{name}_drawn"]).to(dev).long()] if f"{name}_drawn" in Z.files else vidx
    return samples, w


def _statement(c, name):
    dev = c.fg.device
    H, W = c.H, c.W
    samples, w = _samples(c, name)
    d = lambda t: t.detach().double().reshape(-1, H, W).squeeze(0)
    N, D = d(c.pk[0]["rend_normal"]).requires_grad_(True), d(c.pk[0]["rend_distance"]).requires_grad_(True)
    o = mn.ncc_loss(N, D, d(c.grey[0]), d(c.grey[1]), d(c.pk[0]["refl_strength_map"]), d(c.pk[1]["refl_strength_map"]), w,
                    ms.camera_record(c.cams[0], device=dev), ms.camera_record(c.cams[1], device=dev), _intr(c.cams[0]), _intr(c.cams[1]),
                    samples, patch_half=c.patch, ncc_w=0.15)
    return o, N, D, samples


def test_fixture_cases():
    """The cases the fixture has to hold: NCC with and without the material terms, a ragged size, most samples through the gate, nothing
    used, no valid pixel, and the small patches."""
    meta = {n: Z[f"{n}_meta"] for n in CASES}
    assert any(m[0] <= 10000 and not math.isnan(float(Z[f"{n}_ncc"])) for n, m in meta.items())
    assert any(m[0] > 10000 and not math.isnan(float(Z[f"{n}_ncc"])) for n, m in meta.items())
    assert any(str(Z[f"{n}_scene"]) == "B" for n in CASES)
    assert any(m[2] < 1 and int((Z[f"{n}_refw"] > 0).sum()) > 0.25 * m[1] for n, m in meta.items())
    assert any(math.isnan(float(Z[f"{n}_ncc"])) and m[3] == 1 for n, m in meta.items())
    assert any(math.isnan(float(Z[f"{n}_ncc"])) and m[3] == 0 for n, m in meta.items())
    assert {1, 2} <= {int(m[4]) for m in meta.values()}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "reference_ncc.npz")) <= \
        os.path.getsize(os.path.join(ROOT, "tests", "golden", "reference_warp.npz"))


@pytest.mark.parametrize("name", CASES)
def test_statement_matches_reference(name):
    """The float64 statement against the reference's own get_consistency_loss2 / lncc / visual_refweight: scalar, both gradient maps, the
    ref_weight map."""
    c = _case(name, "cpu", torch.float64)
    o, N, D, _ = _statement(c, name)
    ref = float(Z[f"{name}_ncc"])
    if math.isnan(ref):                                 # None in the reference: no valid pixel, or no sample used
        assert o["n_used"] == 0 and float(o["ncc"].detach()) == 0.0
    else:
        assert o["n_used"] > 0
        assert abs(float(o["ncc"].detach()) - ref) <= 1e-10 * abs(ref), (float(o["ncc"].detach()), ref)
        o["ncc"].backward()
    for leaf, key in ((N, "g_normal"), (D, "g_distance")):
        gref = Z[f"{name}_{key}"].astype(np.float64)
        g = np.zeros_like(gref) if leaf.grad is None else leaf.grad.numpy().reshape(gref.shape)
        scale = max(np.abs(gref).max(), 1e-30)
        assert np.abs(g - gref).max() <= 1e-6 * scale, (name, key, np.abs(g - gref).max() / scale)     # fixture stored as float32
    rw = Z[f"{name}_refw"]
    assert np.array_equal(o["ref_weight"].numpy() > 0, rw > 0)
    assert np.abs(o["ref_weight"].numpy() - rw).max() <= 1e-6


def test_analytic_inputs_meet_the_conditions():
    """The small analytic cases: used samples and an empty ambiguous set (the at-size cases assert the same on the device)."""
    for (H, W), used in (((48, 64), 192), ((61, 83), None)):
        v, n = ms.analytic_pair(H, W)
        gv, gn = mn.grey_pair(H, W)
        d = lambda t: t.double()
        cv, cn = ms.camera_record(v.cam), ms.camera_record(n.cam)
        _e, valid, w, _u = ms.geometry(d(v.depth), d(n.depth), cv, cn, _intr(v.cam), _intr(n.cam))
        idx = torch.nonzero(valid.reshape(-1))[:, 0]
        o = mn.ncc_loss(d(v.normal), d(v.distance), d(gv), d(gn), d(v.metal), d(n.metal), w, cv, cn, _intr(v.cam), _intr(n.cam), idx)
        assert o["n_used"] >= 0.1 * idx.numel() and int(o["ambiguous"].sum()) == 0 and int(o["ambiguous_w"].sum()) == 0
        if used is not None:
            assert (idx.numel(), o["n_used"]) == (1315, used)


def _cfg(**kw):
    from materialrefgs_amd import _lib
    c = _lib.MrgsWarpConfig(48, 64, 1000, 3, -1, _lib.MRGS_WARP_GEO, 1, 2, 50.0, 50.0, 32.0, 24.0, 50.0, 50.0, 32.0, 24.0, 1.0, 0.03, 0.015,
                            0.025, 0.025)
    for k, val in kw.items():
        setattr(c, k, val)
    return c


def test_ncc_abi_argument_checks_without_gpu():
    """The three entry points exist, ws_bytes is 0 for shapes the calls refuse, and every contract violation is MRGS_E_BAD_ARG (1) or
    MRGS_E_WORKSPACE (5) before anything is launched (no pointer below is ever dereferenced)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    need = L.mrgs_warp_ncc_ws_bytes(48, 64, 1000, 3)
    assert need > 48 * 64 * 4 + 1000 * (4 + 8 + 16 + 1)
    for bad in ((48, 64, 1000, 4), (48, 64, 1000, 0), (0, 64, 1000, 3), (48, -1, 1000, 3), (48, 64, 0, 1), (1 << 15, 1 << 15, 10, 1)):
        assert L.mrgs_warp_ncc_ws_bytes(*bad) == 0, bad
    hdr = open(os.path.join(ROOT, "include", "mrgs.h")).read()
    for sym in ("mrgs_warp_ncc_ws_bytes", "mrgs_warp_ncc_forward", "mrgs_warp_ncc_backward"):
        assert sym in hdr
    assert L.mrgs_abi_version() == 10                   # entry points only: the revision stays
    p = ctypes.c_void_p(0x1000)
    full = lambda: _lib.MrgsWarpMaps(*([p] * 11 + [None, p, p]))
    big = 1 << 30

    def fwd(cfg, m=None, ws_bytes=big, warp_ws_bytes=big, grey_v=p, grey_n=p, weight=p, warp_ws=p, ws=p, samples=None, w=0.15, term=p,
            counts=p, refw=p):
        m = full() if m is None else m
        return L.mrgs_warp_ncc_forward(ctypes.byref(cfg), ctypes.byref(m), grey_v, grey_n, weight, warp_ws, warp_ws_bytes, samples, ws,
                                       ws_bytes, w, term, counts, refw, None, None, None)

    def bwd(cfg, warp_ws=p, ws=p, w=0.15, g=p):
        return L.mrgs_warp_ncc_backward(ctypes.byref(cfg), warp_ws, ws, w, g, p, p, None)

    bad = _cfg()
    bad.struct_size -= 4
    assert fwd(bad) == 1 and bwd(bad) == 1
    for kw in (dict(patch_half=0), dict(patch_half=4), dict(sample_num=0), dict(H=0), dict(n_given=1001), dict(n_given=-2),
               dict(flags=_lib.MRGS_WARP_METALLIC), dict(flags=16), dict(fx_v=0.0), dict(fy_n=-1.0), dict(cx_v=float("nan"))):
        assert fwd(_cfg(**kw)) == 1, kw
        assert bwd(_cfg(**kw)) == 1, kw
    assert L.mrgs_warp_ncc_forward(ctypes.byref(_cfg()), None, p, p, p, p, big, None, p, big, 0.15, p, p, p, None, None, None) == 1
    for field in ("cam_v", "cam_n", "normal_v", "distance_v", "metal_v", "metal_n"):     # needed whatever the flags
        m = full()
        setattr(m, field, None)
        assert fwd(_cfg(), m) == 1, field
    for arg in ("grey_v", "grey_n", "weight", "warp_ws", "ws", "term", "counts", "refw"):
        assert fwd(_cfg(), **{arg: None}) == 1, arg
    assert fwd(_cfg(n_given=5)) == 1                    # given samples, no material call that took them, and no list
    assert fwd(_cfg(), w=float("nan")) == 1 and bwd(_cfg(), w=float("nan")) == 1
    assert fwd(_cfg(), ws_bytes=need - 1) == 5
    assert fwd(_cfg(), warp_ws_bytes=L.mrgs_warp_loss_ws_bytes(48, 64, 1000, 3) - 1) == 5
    for arg in ("warp_ws", "ws", "g"):
        assert bwd(_cfg(), **{arg: None}) == 1, arg


def test_wrapper_finds_the_grey_image():
    """calc_warp_loss_refreal takes the grey image as the reference does; with one it passes the gate the image-less cameras of
    test_multiview_loss.py::test_wrapper_errors stop at, and reaches the device-tensor check."""
    from materialrefgs_amd import multiview as mv
    g = torch.rand(1, 4, 5)
    rgb = torch.rand(3, 4, 5)
    assert mv._grey_image(SimpleNamespace(get_image=lambda: (rgb, g), original_image_gray=None)) is g
    assert mv._grey_image(SimpleNamespace(original_image_gray=g, original_image=rgb)) is g
    lum = mv._grey_image(SimpleNamespace(original_image=rgb))
    assert tuple(lum.shape) == (1, 4, 5) and torch.allclose(lum[0], 0.299 * rgb[0] + 0.587 * rgb[1] + 0.114 * rgb[2])
    assert mv._grey_image(SimpleNamespace()) is None
    v, n = ms.analytic_pair(16, 20)
    pkg = {"surf_depth": v.depth[None], "rend_normal": v.normal, "rend_distance": v.distance[None], "diffuse_map": v.base,
           "refl_strength_map": v.metal[None], "roughness_map": v.rough[None]}
    opt = SimpleNamespace(use_virtul_cam=False, wo_use_geo_occ_aware=False, edge_aware_in_warp=False, directional_rghmtl_warp_alignment=True)
    cam = SimpleNamespace(ncc_scale=1.0, nearest_id=[0], image_name="a", original_image_gray=torch.rand(1, 16, 20))
    args = (None, opt, None, None, None, None, pkg, None, None, None, {}, 8000, None, None)
    with pytest.raises(RuntimeError, match="device tensors"):
        mv.calc_warp_loss_refreal(cam, *args)
    with pytest.raises(NotImplementedError, match="ncc_scale"):           # still out of scope
        mv.calc_warp_loss_refreal(SimpleNamespace(ncc_scale=2.0, nearest_id=[0], image_name="a", original_image_gray=g), *args)
    with pytest.raises(NotImplementedError, match="without_ncc"):
        mv.calc_warp_loss_refreal(SimpleNamespace(ncc_scale=1.0, nearest_id=[0], image_name="a"), *args)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _pkg(v, dev, metal_scale=1.0):
    pk = {"surf_depth": v.depth[None], "rend_normal": v.normal, "rend_distance": v.distance[None], "diffuse_map": v.base,
          "refl_strength_map": v.metal[None] * metal_scale, "roughness_map": v.rough[None]}
    pk = {k: t.to(dev).clone() for k, t in pk.items()}
    for k in ("rend_normal", "rend_distance"):
        pk[k].requires_grad_(True)
    return pk


def _native(vc, vp, nc, npk, fg, gv, gn, **kw):
    from materialrefgs_amd import multiview as mv
    dev = gv.device
    k = kw.get("sample_num", 102400)
    smp = torch.full((k,), -1, dtype=torch.int32, device=dev) if "samples" not in kw else None
    detail = {}
    r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, None, seed=kw.pop("seed", 7), out_samples=smp, schedule="refreal", grey_v=gv, grey_n=gn,
                                 ncc_detail=detail, **dict(KW, **kw))
    assert len(r) == 8
    return r, smp, detail


def _stmt(vc, vp, nc, npk, gv, gn, samples, patch_size=3, use_override=None, **_):
    dev = gv.device
    H, W = gv.shape[-2:]
    d = lambda t: t.detach().double().reshape(-1, H, W).squeeze(0)
    cv, cn = ms.camera_record(vc, device=dev), ms.camera_record(nc, device=dev)
    _e, valid, w, _u = ms.geometry(d(vp["surf_depth"]), d(npk["surf_depth"]), cv, cn, _intr(vc), _intr(nc))
    N, D = d(vp["rend_normal"]).requires_grad_(True), d(vp["rend_distance"]).requires_grad_(True)
    o = mn.ncc_loss(N, D, d(gv), d(gn), d(vp["refl_strength_map"]), d(npk["refl_strength_map"]), w, cv, cn, _intr(vc), _intr(nc), samples,
                    patch_half=patch_size, ncc_w=KW["ncc_weight"], delta=DELTA, use_override=use_override)
    return o, N, D, int(valid.sum())


def _compare(vc, vp, nc, npk, fg, gv, gn, min_used=0.0, **kw):
    """Native NCC vs the statement on the native draw (or the given samples): counts, per-sample decisions, scalar, ref_weight map, both
    gradient maps under a random upstream.  Returns the measured figures."""
    (r, smp, det) = _native(vc, vp, nc, npk, fg, gv, gn, **kw)
    ncc, refw = r[6], r[7]
    dev = gv.device
    H, W = gv.shape[-2:]
    n_s, n_used = (int(x) for x in det["counts"])
    samples = kw["samples"].long() if "samples" in kw else smp[:n_s].long()
    assert samples.numel() == n_s and bool((samples >= 0).all())
    kwargs = {k: v for k, v in kw.items() if k == "patch_size"}
    o, _N, _D, nv = _stmt(vc, vp, nc, npk, gv, gn, samples, **kwargs)
    assert int(r[5]) == nv
    if "samples" not in kw:
        assert n_s == min(nv, kw.get("sample_num", 102400))
    use = det["use_s"][:n_s].bool()
    A = o["ambiguous"]
    assert int(A.sum()) <= max(4, 1e-4 * n_s), int(A.sum())
    assert int(o["ambiguous_w"].sum()) <= max(4, 1e-4 * n_s), int(o["ambiguous_w"].sum())
    assert bool((use == o["use_s"])[~A].all()), int((use != o["use_s"])[~A].sum())
    assert not bool(det["use_s"][n_s:].any())
    # the statement with the kernel's decisions on A (one flipped sample moves the mean's denominator for every texel)
    o, N, D, _ = _stmt(vc, vp, nc, npk, gv, gn, samples, use_override=use, **kwargs)
    assert o["n_used"] == n_used
    assert n_used >= min_used * n_s, (n_used, n_s)
    figs = dict(samples=n_s, used=n_used, ambiguous=int(A.sum()))
    figs["ncc_s"] = float((det["ncc_s"][:n_s].double() - o["ncc_s"]).abs().max()) if n_s else 0.0
    assert figs["ncc_s"] <= 1e-5, figs
    ref = float(o["ncc"].detach())
    figs["scalar"] = abs(float(ncc) - ref) / max(abs(ref), 1e-30)
    assert figs["scalar"] < 1e-5 or abs(float(ncc) - ref) < 1e-12, (float(ncc), ref)
    # ref_weight: 1e-5; a sample within delta of m = 0.2 may sit on either side of the 0.9 cut
    dm = (refw.double() - o["ref_weight"]).abs().reshape(-1)
    loose = torch.zeros(H * W, dtype=torch.bool, device=dev)
    loose[samples[o["ambiguous_w"]]] = True
    figs["ref_weight"] = float(dm[~loose].max())
    assert figs["ref_weight"] <= 1e-5, figs
    assert bool(((dm[loose] <= 1e-5) | (refw.reshape(-1)[loose] == 0) | ((refw.reshape(-1)[loose] - 0.9).abs() <= 1e-5)).all())
    up = 0.5 + float(torch.rand(1, generator=torch.Generator().manual_seed(3)))
    for k in ("rend_normal", "rend_distance"):
        vp[k].grad = None
    (ncc * up).backward()
    if o["ncc"].requires_grad and o["n_used"] > 0:
        (o["ncc"] * up).backward()
    for key, leaf in (("rend_normal", N), ("rend_distance", D)):
        g = vp[key].grad
        assert g is not None and bool(torch.isfinite(g).all())
        gr = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        scale = float(gr.abs().max())
        if scale == 0:
            assert float(g.abs().max()) == 0, key
            continue
        figs[key] = float((g.double().reshape(gr.shape) - gr).abs().max()) / scale
        assert figs[key] <= 1e-4, (key, figs)
    return figs


def _analytic(H, W, dev, metal_scale=1.0):
    v, n = ms.analytic_pair(H, W)
    gv, gn = (g.to(dev) for g in mn.grey_pair(H, W))
    return v.cam.to(dev), _pkg(v, dev, metal_scale), n.cam.to(dev), _pkg(n, dev, metal_scale), v.fg.to(dev), gv, gn


@pytest.mark.gpu
@pytest.mark.parametrize("iteration", [8000, 15000])
@pytest.mark.parametrize("H,W,k", [(48, 64, 100000), (48, 64, 300), (61, 83, 100000), (61, 83, 700)])
def test_analytic_scene_against_statement(gpu_device, H, W, k, iteration):
    figs = _compare(*_analytic(H, W, gpu_device), iteration=iteration, sample_num=k, min_used=0.05)
    print(H, W, k, iteration, figs)


@pytest.mark.gpu
@pytest.mark.parametrize("iteration", [8000, 15000])
@pytest.mark.parametrize("patch_size", [1, 2, 3])
def test_patch_sizes(gpu_device, patch_size, iteration):
    figs = _compare(*_analytic(48, 64, gpu_device, 0.5), iteration=iteration, sample_num=800, patch_size=patch_size, min_used=0.05)
    print(patch_size, iteration, figs)


@pytest.mark.gpu
@pytest.mark.parametrize("iteration", [8000, 15000])
def test_given_samples(gpu_device, iteration):
    """A caller-supplied draw in a random order, with and without the material call that would have taken it."""
    dev = gpu_device
    a = _analytic(48, 64, dev, 0.5)
    d = lambda t: t.detach().double().reshape(48, 64)
    _e, valid, _w, _u = ms.geometry(d(a[1]["surf_depth"]), d(a[3]["surf_depth"]), ms.camera_record(a[0], device=dev),
                                     ms.camera_record(a[2], device=dev), _intr(a[0]), _intr(a[2]))
    idx = torch.nonzero(valid.reshape(-1))[:, 0]
    pick = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(4))[:400].to(dev)]
    figs = _compare(*a, iteration=iteration, sample_num=400, samples=pick.int(), min_used=0.05)
    print(iteration, figs)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(800, 800), (1600, 1600), (779, 1037)])
def test_at_size_against_float64(gpu_device, H, W):
    figs = _compare(*_analytic(H, W, gpu_device), iteration=8000, sample_num=102400, min_used=0.10)
    assert figs["samples"] == 102400
    print(H, W, figs)


@pytest.mark.gpu
def test_at_size_with_the_material_terms(gpu_device):
    """800^2 at iteration 15 000: the draw and the homographies come from the material call."""
    figs = _compare(*_analytic(800, 800, gpu_device), iteration=15000, sample_num=102400, min_used=0.10)
    assert figs["samples"] == 102400
    print(figs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_drop_in_replays_reference(gpu_device, name):
    """calc_warp_loss_refreal with cameras that carry grey images and the recorded draw, against the reference's own numbers."""
    from materialrefgs_amd import multiview as mv
    dev = gpu_device
    c = _case(name, dev, torch.float32)
    H, W = c.H, c.W
    samples, _w = _samples(_case(name, dev, torch.float64), name)
    opt = SimpleNamespace(edge_aware_in_warp=True, use_virtul_cam=False, multi_view_patch_size=c.patch, multi_view_sample_num=c.k,
                          multi_view_pixel_noise_th=1.0, multi_view_ncc_weight=0.15, multi_view_geo_weight=0.03, metallic_warp_weight=0.05,
                          roughness_warp_weight=0.05, wo_use_geo_occ_aware=False, directional_rghmtl_warp_alignment=True, srgb=False)
    rgb = c.grey[0][None].expand(3, -1, -1)
    cam0 = SimpleNamespace(**c.cams[0]._asdict(), image_name="view0", nearest_id=[0], ncc_scale=1.0, get_image=lambda: (rgb, c.grey[0][None]))
    cam1 = SimpleNamespace(**c.cams[1]._asdict(), image_name="view1", original_image_gray=c.grey[1][None])
    scene = SimpleNamespace(getTrainCameras=lambda: [cam1])
    render = lambda cam, *a, **k: c.pk[1]
    edges = lambda normal, dilate_size: (~c.keep).float()
    args = (cam0, scene, opt, None, None, None, render, c.pk[0], None, None, None, {"view0": c.fg}, c.it, None, None)
    kw = dict(use_metallic_warp=True, use_roughness_warp=True, edges_fn=edges, samples=samples.int())

    def grads(which):
        for k in ("rend_normal", "rend_distance"):
            c.pk[0][k].grad = None
        r = mv.calc_warp_loss_refreal(*args, **kw)
        terms = [t for t in (r[0], r[1], r[2], r[3], r[4]) if t is not None and math.isfinite(float(t))]
        (sum(terms) if which == "all" else r[1]).backward()
        return r, [None if c.pk[0][k].grad is None else c.pk[0][k].grad.clone() for k in ("rend_normal", "rend_distance")]

    r, g_all = grads("all")
    assert len(r) == 8 and r[7] is None
    assert isinstance(r[1], torch.Tensor) and r[1].dim() == 0 and r[1].device == c.fg.device
    assert tuple(r[6].shape) == (H, W) and r[6].device == c.fg.device
    rw = torch.from_numpy(Z[f"{name}_refw"]).to(dev)
    assert torch.equal(r[6] > 0, rw > 0) and float((r[6] - rw).abs().max()) <= 1e-6
    ref = float(Z[f"{name}_ncc"])
    if math.isnan(ref):
        assert float(r[1]) == 0.0                       # None in the reference
    else:
        assert abs(float(r[1]) - ref) <= 1e-5 * abs(ref), (float(r[1]), ref)
    tref = Z[f"{name}_terms"]                           # the other terms of the same call are the reference's too
    for mine, t in zip((r[0], r[2]), tref[:2]):         # (geo and base colour)
        if not math.isnan(t) and mine is not None and math.isfinite(float(mine)):
            assert abs(float(mine) - t) <= 1e-5 * abs(t), (float(mine), t)
    _r, g_ncc = grads("ncc")
    for ga, gn_, key in zip(g_all, g_ncc, ("g_normal", "g_distance")):
        assert ga is not None and gn_ is not None and torch.equal(ga, gn_)          # only the NCC node reaches these two maps
        gref = torch.from_numpy(Z[f"{name}_{key}"]).to(dev).double()
        scale = float(gref.abs().max())
        if scale == 0:
            assert float(ga.abs().max()) == 0
        else:
            assert float((ga.double().reshape(gref.shape) - gref).abs().max()) <= 1e-4 * scale


@pytest.mark.gpu
def test_forward_and_backward_are_bitwise_repeatable(gpu_device):
    from materialrefgs_amd import multiview as mv
    dev = gpu_device
    vc, vp, nc, npk, fg, gv, gn = _analytic(61, 83, dev, 0.5)
    runs = []
    for _ in range(3):
        for k in ("rend_normal", "rend_distance"):
            vp[k].grad = None
        det = {}
        r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=15000, seed=9, sample_num=1500, schedule="refreal", grey_v=gv,
                                     grey_n=gn, ncc_detail=det, **KW)
        r[6].backward()
        runs.append([r[6].detach(), r[7], det["ncc_s"], det["use_s"], det["counts"], vp["rend_normal"].grad.clone(),
                     vp["rend_distance"].grad.clone()])
    assert int(runs[0][4][1]) > 0 and float(runs[0][5].abs().max()) > 0
    for run in runs[1:]:
        for a, b in zip(run, runs[0]):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    from materialrefgs_amd import multiview as mv
    dev = gpu_device
    vc, vp, nc, npk, fg, gv, gn = _analytic(48, 64, dev, 0.5)
    gv3, gn3 = gv[None].clone(), gn[None].clone()       # [1,H,W] as the cameras hold them
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in (8000, 15000):
            r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=it, seed=5, sample_num=1000, schedule="refreal", grey_v=gv3,
                                         grey_n=gn3, **KW)
            (r[0] + r[6]).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(vp["rend_normal"].grad.abs().max()) > 0 and float(vp["rend_distance"].grad.abs().max()) > 0


@pytest.mark.gpu
def test_empty_cases(gpu_device):
    from materialrefgs_amd import multiview as mv
    dev = gpu_device

    def run(a, **kw):
        vc, vp, nc, npk, fg, gv, gn = a
        det = {}
        r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=kw.pop("iteration", 8000), seed=1, sample_num=500, schedule="refreal",
                                     grey_v=kw.pop("gv", gv), grey_n=kw.pop("gn", gn), ncc_detail=det, **KW)
        (r[0] + r[6]).backward()
        return r, det, vp

    # no valid pixel
    a = _analytic(48, 64, dev)
    with torch.no_grad():
        a[3]["surf_depth"].zero_()
    for it in (8000, 15000):
        r, det, vp = run(a, iteration=it)
        assert int(r[5]) == 0 and float(r[6]) == 0 and float(r[7].abs().max()) == 0 and det["counts"].tolist() == [0, 0]
        assert float(vp["rend_normal"].grad.abs().max()) == 0 and float(vp["rend_distance"].grad.abs().max()) == 0
    # nothing used: every sample fails the metal gate
    r, det, vp = run(_analytic(48, 64, dev, 8.0), iteration=15000)
    assert det["counts"].tolist()[0] == 500 and det["counts"].tolist()[1] == 0 and float(r[6]) == 0 and float(r[7].abs().max()) == 0
    assert float(vp["rend_normal"].grad.abs().max()) == 0 and float(vp["rend_distance"].grad.abs().max()) == 0
    # grey images of constant value: ncc_s = 1 and nothing used, though the metal gate is open.  The samples are the valid pixels more
    # than a patch away from the edges of both images: a patch that reaches outside an image reads zeros there and is not constant.
    from materialrefgs_amd import multiview as mv
    vc, vp, nc, npk, fg, gv, gn = _analytic(48, 64, dev, 0.1)
    d = lambda t: t.detach().double().reshape(48, 64)
    _e, valid, _w, u = ms.geometry(d(vp["surf_depth"]), d(npk["surf_depth"]), ms.camera_record(vc, device=dev),
                                    ms.camera_record(nc, device=dev), _intr(vc), _intr(nc))
    s = torch.nonzero(valid.reshape(-1))[:, 0]
    sx, sy, us = s % 64, s // 64, u.reshape(-1, 2)[s]
    s = s[(sx >= 3) & (sx < 61) & (sy >= 3) & (sy < 45) & (us[:, 0] > 6) & (us[:, 0] < 57) & (us[:, 1] > 6) & (us[:, 1] < 41)][::2][:500]
    assert s.numel() > 200
    det = {}
    r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=8000, seed=1, sample_num=500, schedule="refreal", samples=s.int(),
                                 grey_v=torch.full_like(gv, 0.37), grey_n=torch.full_like(gn, 0.62), ncc_detail=det, **KW)
    (r[0] + r[6]).backward()
    assert det["counts"].tolist() == [s.numel(), 0] and float(r[6]) == 0
    assert float((det["ncc_s"][: s.numel()] - 1).abs().max()) == 0 and not bool(det["use_s"].any())
    assert float(vp["rend_normal"].grad.abs().max()) == 0 and float(vp["rend_distance"].grad.abs().max()) == 0
    assert float(r[7].max()) > 0.9                      # the ref_weight map does not depend on the grey images


@pytest.mark.gpu
def test_samples_at_the_image_border(gpu_device):
    """Samples on the image's edges and corners: the view's taps outside read zero.  The scene is given a surface everywhere (a plane
    behind the analytic one) so that the homography of a border sample is finite, and a texture that is not zero at the border."""
    dev = gpu_device
    H, W = 48, 64
    vc, vp, nc, npk, fg, _gv, _gn = _analytic(H, W, dev, 0.3)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(W, device=dev).float(), indexing="ij")
    fill = 0.5 + 0.3 * torch.sin(0.9 * xs + 0.7 * ys)
    gv, gn = torch.where(_gv > 0, _gv, fill), torch.where(_gn > 0, _gn, fill)
    with torch.no_grad():
        bgn = torch.tensor([0.0, 0.0, 1.0], device=dev) @ vc.world_view_transform[:3, :3].T       # faces the view's camera
        hole = fg.reshape(H, W) < 0.5
        vp["rend_normal"].copy_(torch.where(hole[None], -bgn[:, None, None].expand(3, H, W), vp["rend_normal"]))
        vp["rend_distance"].copy_(torch.where(hole[None], torch.full_like(vp["rend_distance"], 5.0), vp["rend_distance"]))
    border = [0, W - 1, (H - 1) * W, H * W - 1, W // 2, (H // 2) * W, (H // 2) * W + W - 1, (H - 1) * W + W // 2, W + 1, 2 * W + 2]
    d = lambda t: t.detach().double().reshape(H, W)
    _e, valid, _w, _u = ms.geometry(d(vp["surf_depth"]), d(npk["surf_depth"]), ms.camera_record(vc, device=dev),
                                     ms.camera_record(nc, device=dev), _intr(vc), _intr(nc))
    inner = torch.nonzero(valid.reshape(-1))[:, 0][::9][:200]
    pick = torch.cat([torch.tensor(border, device=dev), inner]).unique()
    for it in (8000, 15000):
        figs = _compare(vc, vp, nc, npk, fg, gv, gn, iteration=it, sample_num=400, samples=pick.int())
        print(it, figs)


@pytest.mark.gpu
def test_the_draw_does_not_depend_on_the_material_terms(gpu_device):
    """Iteration 8000 (the NCC call draws) and 15 000 (the material call draws): the same samples for the same seed and valid set."""
    dev = gpu_device
    a = _analytic(61, 83, dev)
    draws = []
    for it in (8000, 15000, 8000):
        (r, smp, det) = _native(*a, iteration=it, sample_num=700, seed=11)
        assert int(det["counts"][0]) == 700
        draws.append(smp.clone())
    assert torch.equal(draws[0], draws[1]) and torch.equal(draws[0], draws[2])
    assert bool((draws[0][1:] > draws[0][:-1]).all())
    (r, smp, det) = _native(*a, iteration=8000, sample_num=700, seed=12)
    assert not torch.equal(smp, draws[0])


@pytest.mark.gpu
def test_end_to_end_gradient_reaches_the_surfels(gpu_device):
    """One render_surfel("pgsr") pair: the NCC term's gradient goes through rend_normal / rend_distance into the surfel parameters."""
    from materialrefgs_amd import multiview as mv
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    H = W = 128
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    pc, env, leaves = make_surfel_model(20000, H, dev)
    cams = [orbit_camera(v, H, W, n_views=96).to(dev) for v in (0, 1)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    env.build_mips()
    pk = [render_surfel(c, pc, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr") for c in cams]
    assert pk[0]["rend_normal"].requires_grad and pk[0]["rend_distance"].requires_grad
    lum = lambda img: (0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2]).detach()
    grey = [lum(p["render"]) for p in pk]
    # the gate is on the metal maps, which carry no gradient from this term: scaled so that samples pass it
    pv, pn = dict(pk[0]), dict(pk[1])
    for p in (pv, pn):
        p["refl_strength_map"] = p["refl_strength_map"].detach() * 0.05
    fg = (pk[0]["rend_alpha"].detach() > 0.5).float().reshape(H, W)
    det = {}
    r = mv.warp_consistency_loss(cams[0], pv, cams[1], pn, fg, iteration=8000, seed=3, sample_num=4000, schedule="refreal", grey_v=grey[0],
                                 grey_n=grey[1], ncc_detail=det, **KW)
    assert int(det["counts"][1]) > 0 and float(r[6]) > 0
    r[6].backward()
    touched = 0
    for t in leaves:
        if t.grad is not None:
            assert bool(torch.isfinite(t.grad).all())
            touched += int(float(t.grad.abs().max()) > 0)
    assert touched > 0
