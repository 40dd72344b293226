"""The multi-view reflection score (materialrefgs_amd.refscore over mrgs_ref_score, csrc/mrgs_multiview.hip).

CPU: the float64 statement (tests/ref_score_statement.py) against what the reference's own calc_ref_score computed on four analytic
views (tests/golden/reference_ref_score.npz, written by tests/golden/gen_reference_ref_score_vectors.py), get_multi_view_neighbor
against the reference's lists, the conditions of the inputs the GPU tests use, the C ABI's argument checks and the wrapper's errors.
GPU (-m gpu): the native call against the statement at three sizes and with the small patches, calc_ref_score replaying the fixture,
run-to-run identity, no host read, the edge cases and one end-to-end pass into priors.ref_score_loss.

Bars: every count equal and every score texel within 1e-5 of the map's largest element (the project's bar for forward terms,
test_multiview_loss.py), outside the pixels the statement marks ambiguous: a decision quantity of some neighbour (e against the noise
bound, u against 0 and W, v against 0 and H, z against 0.1) within 1e-6 of its threshold.  The analytic inputs have none.
"""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ref_score_statement as rs

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_ref_score.npz")
AZ4 = (30.0, 37.0, 24.0, 41.0)
TH = 1.0
BAR = 1e-5


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(FIXTURE)
    from materialrefgs_amd.camera import MiniCam
    views = []
    for i in range(4):
        rec = z[f"{i}_cam"]
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
        H, W = z[f"{i}_depth"].shape
        cam = MiniCam(H, W, float(rec[31]), float(rec[32]), 0.01, 100.0, f32(rec[:16].reshape(4, 4)), torch.eye(4), f32(rec[28:31]),
                      f32(rec[16:25].reshape(3, 3)), f32(rec[25:28]))
        views.append(SimpleNamespace(cam=cam, name=f"view{i}", depth=torch.tensor(z[f"{i}_depth"]), normal=torch.tensor(z[f"{i}_normal"]),
                                     distance=torch.tensor(z[f"{i}_distance"]), image=torch.tensor(z[f"{i}_image"]),
                                     score=torch.tensor(z[f"{i}_score"])))
    lists = [[int(j) for j in row if j >= 0] for row in z["neighbours"]]
    return views, lists, float(z["th"])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(view, neighbours) of the named input; computed once."""
    if name == "40x52":
        v = rs.analytic_views(40, 52, AZ4)
        return v[0], [v[2], v[1], v[3]]
    if name == "61x83":                                   # neither side a multiple of the 8 x 8 block
        v = rs.analytic_views(61, 83, AZ4)
        return v[0], [v[2], v[1], v[3]]
    if name == "96x136":                                  # K = 6: four near views, the azimuth opposite, the view itself (e = 0)
        v = rs.analytic_views(96, 136, AZ4 + (33.0, 210.0))
        return v[0], [v[1], v[2], v[3], v[4], v[5], v[0]]
    if name == "dist0":                                   # rend_distance exactly 0 on a lattice of pixels, valid ones among them
        v, n = _case("40x52")
        ys, xs = torch.meshgrid(torch.arange(40), torch.arange(52), indexing="ij")
        d = torch.where((xs + 2 * ys) % 5 == 0, torch.zeros_like(v.distance), v.distance)
        return SimpleNamespace(cam=v.cam, name=v.name, depth=v.depth, normal=v.normal, distance=d, image=v.image), n
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _statement(name, patch_half=4):
    view, nbrs = _case(name)
    return rs.ref_score(view, nbrs, th=TH, patch_half=patch_half)


CASES = ("40x52", "61x83", "96x136")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_statement_equals_the_reference():
    """1e-12 absolute: float64 reordering of at most 243 K terms of order 1 (observed 1e-15)."""
    views, lists, th = _fixture()
    for i, v in enumerate(views):
        o = rs.ref_score(v, [views[j] for j in lists[i]], th=th, patch_half=4)
        err = float((o.score - v.score).abs().max())
        print(f"view{i}: |statement - reference| max {err:.2e}, reference max {float(v.score.max()):.3f}")
        assert float(v.score.max()) > 0.3
        assert err <= 1e-12, (i, err)


def test_neighbour_lists_equal_the_reference():
    from materialrefgs_amd import refscore
    views, lists, _th = _fixture()
    cams = [rs.Cam(v.cam, v.name) for v in views]
    got = refscore.get_multi_view_neighbor(SimpleNamespace(getTrainCameras=lambda: cams))
    assert lists == [[2, 1, 3], [0, 2], [0, 1], [0, 2]]                       # (the carried minimum: two after the first camera)
    for i, v in enumerate(views):
        assert got[v.name] == [(j, views[j].name) for j in lists[i]], (i, got[v.name])


@pytest.mark.parametrize("name", CASES + ("dist0",))
def test_input_conditions(name):
    """What makes the GPU comparison meaningful, on every analytic input it uses."""
    view, nbrs = _case(name)
    o = _statement(name)
    K, npix = len(nbrs), o.count.numel()
    n_amb = int(o.ambiguous.sum())
    hist = [int((o.count == c).sum()) for c in range(K + 1)]
    print(f"{name}: ambiguous {n_amb}, count histogram {hist}, per neighbour {[int(x.sum()) for x in o.valid]}, max {float(o.score.max()):.3f}")
    assert n_amb <= max(8, 0.005 * npix)
    assert sum(hist[1:]) >= 0.3 * npix
    assert hist[0] > 0 and sum(hist[1:K]) > 0 and hist[K] > 0
    assert o.anchor_outside and o.nbr_outside
    assert bool(torch.isfinite(o.score).all())
    if name == "96x136":
        assert int(o.valid[5].sum()) == int((o.count > 0).sum()) and int(o.valid[5].sum()) > 0      # the view itself: valid wherever anything is
    if name == "dist0":
        assert int(((view.distance == 0) & (o.count > 0)).sum()) > 50


def _abi_cfg(**kw):
    from materialrefgs_amd import _lib
    c = _lib.MrgsRefScoreConfig(48, 64, 4, 3, 50.0, 50.0, 32.0, 24.0, 1.0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_abi_argument_checks():
    """Every contract violation is MRGS_E_BAD_ARG before a device is touched (the status code include/mrgs.h has for an invalid argument)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p(0x1000)                            # never dereferenced: every call below is refused
    ptrs = [P] * 8                                         # depth, normal, distance, image, cam, neighbours, score, count

    def call(cfg, p=ptrs):
        return L.mrgs_ref_score(ctypes.byref(cfg) if cfg is not None else None, *p, None)
    assert _lib.MRGS_E_BAD_ARG == 1 and _lib.MRGS_ABI_VERSION == 10 and L.mrgs_abi_version() == 10
    assert call(None) == 1
    for kw in (dict(struct_size=36), dict(struct_size=0), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 15), dict(patch_half=0),
               dict(patch_half=5), dict(n_neighbours=-1), dict(fx_v=0.0), dict(fy_v=-1.0), dict(cx_v=float("nan")),
               dict(pixel_noise_th=float("nan"))):
        assert call(_abi_cfg(**kw)) == 1, kw
    for i in (0, 1, 2, 3, 4, 5, 6):                        # every pointer but count
        p = list(ptrs)
        p[i] = None
        assert call(_abi_cfg(), p) == 1, i
    p = list(ptrs)
    p[5] = p[6] = None
    assert call(_abi_cfg(n_neighbours=0), p) == 1          # K = 0 needs no table, but an output


def test_wrapper_errors():
    from materialrefgs_amd import refscore
    v, nbrs = _case("40x52")
    cam = rs.Cam(v.cam, "v", v.image)
    pkg = {"surf_depth": v.depth[None], "rend_normal": v.normal, "rend_distance": v.distance[None]}
    nb = [(rs.Cam(n.cam, n.name), n.depth[None], n.image) for n in nbrs]
    with pytest.raises(RuntimeError, match="device tensor"):
        refscore.reflection_score(cam, pkg, nb, pixel_noise_th=1.0)
    with pytest.raises(ValueError, match="patch_size 5"):
        refscore.reflection_score(cam, pkg, nb, pixel_noise_th=1.0, patch_size=5)
    with pytest.raises(ValueError, match="rend_distance"):
        refscore.reflection_score(cam, {k: pkg[k] for k in ("surf_depth", "rend_normal")}, nb, pixel_noise_th=1.0)
    other = rs.analytic_views(32, 52, AZ4[:2])[1]
    with pytest.raises(ValueError, match="same image size"):
        refscore.reflection_score(cam, pkg, [(rs.Cam(other.cam, "o"), other.depth[None], other.image)], pixel_noise_th=1.0)
    with pytest.raises(ValueError, match="photograph of neighbour 0"):
        refscore.reflection_score(cam, pkg, [(nb[0][0], nb[0][1], nb[0][2][:, :32])], pixel_noise_th=1.0)
    with pytest.raises(ValueError, match="no photograph"):
        refscore.reflection_score(rs.Cam(v.cam, "v"), pkg, nb, pixel_noise_th=1.0)
    with pytest.raises(ValueError, match="shape="):
        refscore.ref_score_mask(torch.zeros(12), 0.1)
    m = refscore.ref_score_mask(torch.tensor([[0.0, 0.2], [0.3, 0.05]]), 0.1, fg_mask=torch.tensor([1.0, 1.0, 0.0, 1.0]))
    assert m.shape == (1, 2, 2) and m.dtype == torch.bool and m.reshape(-1).tolist() == [False, True, False, False]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _native(dev, view, nbrs, patch_half=4, return_count=True):
    from materialrefgs_amd import refscore
    cam = rs.Cam(view.cam, view.name, view.image.to(dev))
    pkg = {"surf_depth": view.depth[None].to(dev), "rend_normal": view.normal.to(dev), "rend_distance": view.distance[None].to(dev)}
    nb = [(rs.Cam(n.cam, n.name), n.depth[None].to(dev), n.image.to(dev)) for n in nbrs]
    return refscore.reflection_score(cam, pkg, nb, pixel_noise_th=TH, patch_size=patch_half, return_count=return_count)


def _compare(label, score, count, o):
    keep = ~o.ambiguous
    top = float(o.score.max())
    err = float(((score.detach().cpu().double() - o.score).abs() * keep).max())
    n_cnt = int(((count.cpu().long() != o.count) & keep).sum())
    print(f"{label}: score max {top:.4f}, worst texel {err:.2e} ({err / top:.2e} of the max, bar {BAR:.0e}), counts that differ {n_cnt}, "
          f"ambiguous pixels left out {int(o.ambiguous.sum())}")
    assert n_cnt == 0
    assert err <= BAR * top, (label, err, top)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_native_against_the_statement(gpu_device, name):
    view, nbrs = _case(name)
    score, count = _native(gpu_device, view, nbrs)
    _compare(name, score, count, _statement(name))


@pytest.mark.gpu
@pytest.mark.parametrize("patch_half", (1, 2, 3))
def test_small_patches(gpu_device, patch_half):
    view, nbrs = _case("40x52")
    score, count = _native(gpu_device, view, nbrs, patch_half)
    _compare(f"patch_size {patch_half}", score, count, _statement("40x52", patch_half))


@pytest.mark.gpu
def test_calc_ref_score_replays_the_fixture(gpu_device):
    """The drop-in over a stub scene whose render returns the fixture's maps: the reference's scores of all four views, through the
    drop-in's own neighbour lists."""
    from materialrefgs_amd import refscore
    dev = gpu_device
    views, lists, th = _fixture()
    cams = [rs.Cam(v.cam, v.name, v.image.to(dev)) for v in views]
    pkgs = {v.name: {"surf_depth": v.depth[None].to(dev), "rend_normal": v.normal.to(dev), "rend_distance": v.distance[None].to(dev)} for v in views}
    calls = []

    def render(cam, gaussians, pipe, bg, srgb=False, opt=None):
        calls.append(cam.image_name)
        return pkgs[cam.image_name]
    scene = SimpleNamespace(getTrainCameras=lambda: list(cams))
    opt = SimpleNamespace(srgb=False, multi_view_pixel_noise_th=th)
    out = refscore.calc_ref_score(scene, opt, None, None, None, None, None, None, None, 0, None, render=render)
    assert calls == [v.name for v in views] and sorted(out) == sorted(calls)
    for i, v in enumerate(views):
        amb = rs.ref_score(v, [views[j] for j in lists[i]], th=th).ambiguous
        got = out[v.name]
        assert got.shape == (40 * 52,) and got.device.type == "cuda"
        top = float(v.score.max())
        err = float(((got.cpu().double().reshape(40, 52) - v.score).abs() * ~amb).max())
        print(f"{v.name}: worst texel {err:.2e} ({err / top:.2e} of the max {top:.3f})")
        assert err <= BAR * top, (i, err, top)


@pytest.mark.gpu
def test_repeatable(gpu_device):
    view, nbrs = _case("96x136")
    a = _native(gpu_device, view, nbrs)
    b = _native(gpu_device, view, nbrs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(a[0].max()) > 0.1 and int(a[1].max()) == 6


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    """Once the cameras' records are cached, a call makes no synchronising call (the way test_prior_terms.py::test_no_host_read checks)."""
    from materialrefgs_amd import refscore
    dev = gpu_device
    view, nbrs = _case("40x52")
    cam = rs.Cam(view.cam, view.name, view.image.to(dev))
    pkg = {"surf_depth": view.depth[None].to(dev), "rend_normal": view.normal.to(dev), "rend_distance": view.distance[None].to(dev)}
    nb = [(rs.Cam(n.cam, n.name), n.depth[None].to(dev), n.image.to(dev)) for n in nbrs]
    first = refscore.reflection_score(cam, pkg, nb, pixel_noise_th=TH, return_count=True)      # (the library is loaded, the records cached)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = refscore.reflection_score(cam, pkg, nb, pixel_noise_th=TH, return_count=True)
        mask = refscore.ref_score_mask(again[0], 0.1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and bool(mask.any())


@pytest.mark.gpu
def test_edge_cases(gpu_device):
    dev = gpu_device
    view, nbrs = _case("40x52")
    flat = SimpleNamespace(cam=view.cam, name=view.name, depth=torch.zeros_like(view.depth), normal=view.normal, distance=view.distance,
                           image=view.image)
    score, count = _native(dev, flat, nbrs)                       # an all-zero surf_depth: no neighbour is valid anywhere
    assert int(count.abs().sum()) == 0 and float(score.abs().sum()) == 0.0
    score, count = _native(dev, view, [])                         # K = 0
    assert score.shape == (40, 52) and int(count.abs().sum()) == 0 and float(score.abs().sum()) == 0.0
    blind = rs.blind_view(40, 52)                                 # a neighbour that sees nothing is valid nowhere: the others' result
    score, count = _native(dev, view, [nbrs[0], blind, nbrs[1], nbrs[2]])
    _compare("with a blind neighbour", score, count, _statement("40x52"))
    v0, n0 = _case("dist0")                                       # rend_distance 0: those homographies are not finite, the taps sample zero
    score, count = _native(dev, v0, n0)
    assert bool(torch.isfinite(score).all())
    _compare("rend_distance 0", score, count, _statement("dist0"))


class _SceneCam:
    """A MiniCam with the name and the photograph a scene camera carries."""

    def __init__(self, mini, name):
        self._mini, self.image_name, self.original_image = mini, name, None

    def __getattr__(self, k):
        return getattr(self._mini, k)


@pytest.mark.gpu
def test_end_to_end(gpu_device):
    """Four orbit cameras on the synthetic surfel model, the photographs being the renders themselves: calc_ref_score with its own render
    and neighbour lists, then ref_score_mask into priors.ref_score_loss and its backward."""
    from materialrefgs_amd import priors, refscore
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    dev = gpu_device
    H = W = 64
    pc, env, leaves = make_surfel_model(3000, 64, dev, seed=1, radius_px=5.0, env_res=64, env_min=16)
    env.build_mips()
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    opt = SimpleNamespace(indirect=False, srgb=False, multi_view_pixel_noise_th=1.0)
    bg = torch.zeros(3, device=dev)
    cams = [_SceneCam(orbit_camera(v, H, W, n_views=36).to(dev), f"cam{v}") for v in range(4)]
    alphas = {}
    for c in cams:
        with torch.no_grad():
            pk = render_surfel(c, pc, pipe, bg, srgb=False, opt=opt, flag="pgsr")
        c.original_image, alphas[c.image_name] = pk["render"].detach().clone(), pk["rend_alpha"].detach().reshape(-1)
    scene = SimpleNamespace(getTrainCameras=lambda: list(cams))
    lists = refscore.get_multi_view_neighbor(scene)
    assert all(len(lists[c.image_name]) >= 1 for c in cams), lists
    out = refscore.calc_ref_score(scene, opt, pc, None, pipe, None, None, None, None, 0, bg)
    for c in cams:
        s = out[c.image_name]
        assert s.shape == (H * W,) and bool(torch.isfinite(s).all())
        assert float(s[alphas[c.image_name] == 0].abs().sum()) == 0.0
    assert max(float(out[c.image_name].max()) for c in cams) > 0
    s0 = out["cam0"]
    mask = refscore.ref_score_mask(s0, float(s0[s0 > 0].median()), shape=(H, W))
    assert mask.shape == (1, H, W) and 0 < int(mask.sum()) < H * W
    pk = render_surfel(cams[0], pc, pipe, bg, srgb=False, opt=opt, flag="pgsr")
    loss = priors.ref_score_loss(pk["refl_strength_map"], pk["roughness_map"], mask, 0.05)
    loss.backward()
    assert bool(torch.isfinite(loss)) and any(t.grad is not None and float(t.grad.abs().max()) > 0 for t in leaves)
