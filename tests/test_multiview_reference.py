"""tests/golden/reference_warp.npz -- the reference's own calc_warp_loss (train_refnerf.py and train_refreal.py, run in float64 by
tests/golden/gen_reference_warp_vectors.py) on the analytic two-view scene -- against the float64 statement of
tests/multiview_statement.py (CPU) and against the native op through both drop-ins with the recorded draw replayed (-m gpu).
Cases: sample_num above and below n_valid, a ragged 29x37 scene, refnerf at 30 000, refreal at 15 000 and 8 000, an empty keep set
(NaN terms) and no valid pixel (the reference returns None; the drop-ins 0)."""
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
from materialrefgs_amd.camera import MiniCam, fov2focal  # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "reference_warp.npz"))
CASES = sorted({k[: -len("_meta")] for k in Z.files if k.endswith("_meta")})
MAPS = ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map")
UP = (0.7, 1.3, 0.9, 1.1)                      # the generator's upstream weights of geo, base, metallic, roughness


def _cam(s, i, dev):
    c = torch.from_numpy(Z[f"{s}_{i}_cam"])
    H, W = Z[f"{s}_{i}_depth"].shape
    f = lambda t: t.to(torch.float32).to(dev)
    return MiniCam(H, W, float(c[-2]), float(c[-1]), 0.01, 100.0, f(c[:16].reshape(4, 4)), f(torch.eye(4)), f(torch.zeros(3)),
                   f(c[16:25].reshape(3, 3)), f(c[25:28]))


def _intr(cam):
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


def _case(name, dev, dtype):
    it, k, fg_scale, dscale, dist_scale, refreal = Z[f"{name}_meta"]
    s = str(Z[f"{name}_scene"])
    f = lambda key: torch.from_numpy(Z[key]).to(dev, dtype)
    pk = []
    for i in (0, 1):
        p = {"surf_depth": f(f"{s}_{i}_depth")[None] * (dscale if i == 1 else 1.0), "rend_normal": f(f"{s}_{i}_normal"),
             "rend_distance": f(f"{s}_{i}_distance")[None] * dist_scale, "diffuse_map": f(f"{s}_{i}_base"),
             "refl_strength_map": f(f"{s}_{i}_metal")[None], "roughness_map": f(f"{s}_{i}_rough")[None]}
        for m in MAPS:
            p[m] = p[m].clone().requires_grad_(True)
        pk.append(p)
    cams = [_cam(s, i, dev) for i in (0, 1)]
    fg = f(f"{s}_0_fg") * fg_scale
    keep = torch.from_numpy(Z[f"{name}_keep"]).to(dev).bool()
    return SimpleNamespace(it=int(it), k=int(k), refreal=bool(refreal), pk=pk, cams=cams, fg=fg, keep=keep)


def _statement(c, name):
    dev = c.fg.device
    H, W = c.fg.shape
    a = 0.1 if not c.refreal else (4.0 if c.it < 12000 else 4.0 - (c.it - 12000) / 8000 * 2.5 if c.it <= 20000 else 1.5)
    b = 1.0 if c.refreal else 0.5
    e, valid, w, _u = ms.geometry(c.pk[0]["surf_depth"].detach().reshape(H, W), c.pk[1]["surf_depth"].detach().reshape(H, W),
                                   ms.camera_record(c.cams[0], device=dev), ms.camera_record(c.cams[1], device=dev), _intr(c.cams[0]),
                                   _intr(c.cams[1]))
    vidx = torch.nonzero(valid.reshape(-1))[:, 0]
    samples = vidx[torch.from_numpy(Z[f"{name}_drawn"]).to(dev).long()] if f"{name}_drawn" in Z.files else vidx
    leaves = [c.pk[i][m].detach().to(torch.float64).clone().requires_grad_(True) for i in (0, 1) for m in MAPS]
    sq = lambda t: t.reshape(-1, H, W).squeeze(0)
    o = ms.warp_loss(sq(leaves[0]), sq(leaves[4]), c.pk[0]["rend_normal"].detach().double(), sq(c.pk[0]["rend_distance"].detach().double()),
                     sq(leaves[1]), sq(leaves[2]), sq(leaves[3]), sq(leaves[5]), sq(leaves[6]), sq(leaves[7]), c.fg.double(), c.keep,
                     ms.camera_record(c.cams[0], device=dev), ms.camera_record(c.cams[1], device=dev), _intr(c.cams[0]), _intr(c.cams[1]),
                     samples, geo_w=0.03, base_w=a * 0.15, metal_w=b * 0.05, rough_w=b * 0.05, material=c.it > 10000)
    return o, leaves, samples


@pytest.mark.parametrize("name", CASES)
def test_statement_matches_reference(name):
    """Scalars, weight map, valid mask and every gradient map of the float64 statement against the reference's own function."""
    c = _case(name, "cpu", torch.float64)
    o, leaves, _ = _statement(c, name)
    present = Z[f"{name}_present"]
    ref = Z[f"{name}_terms"]
    mine = [o["geo"], o["base"], o["metal"], o["rough"]]
    assert np.array_equal(o["weight"].numpy(), Z[f"{name}_weight"]) or np.abs(o["weight"].numpy() - Z[f"{name}_weight"]).max() < 1e-12
    assert np.array_equal(o["valid"].numpy(), Z[f"{name}_weight"] > 0)
    live = []
    for i in range(4):
        if not present[i]:
            continue                                  # None in the reference (refnerf's geo, iteration <= 10000, no valid pixel)
        if math.isnan(ref[i]):
            assert math.isnan(float(mine[i].detach())), (name, i)
            continue
        assert abs(float(mine[i].detach()) - ref[i]) <= 1e-10 * abs(ref[i]), (name, i, float(mine[i].detach()), ref[i])
        live.append(i)
    if live:
        torch.autograd.backward([mine[i] for i in live], [torch.tensor(UP[i], dtype=torch.float64) for i in live])
    for j, (who, m) in enumerate([(w, m) for w in ("v", "n") for m in MAPS]):
        gref = Z[f"{name}_g_{who}_{m}"].astype(np.float64)
        g = np.zeros_like(gref) if leaves[j].grad is None else leaves[j].grad.numpy().reshape(gref.shape)
        scale = max(np.abs(gref).max(), 1e-30)
        assert np.abs(g - gref).max() <= 1e-6 * scale, (name, who, m, np.abs(g - gref).max() / scale)   # fixture stored as float32


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_drop_ins_replay_reference(gpu_device, name):
    """The native op through calc_warp_loss (refnerf) / calc_warp_loss_refreal, with the recorded draw, against the fixture."""
    from materialrefgs_amd import multiview as mv
    dev = gpu_device
    c = _case(name, dev, torch.float32)
    H, W = c.fg.shape
    o, _leaves, samples = _statement(_case(name, dev, torch.float64), name)
    opt = SimpleNamespace(edge_aware_in_warp=True, use_virtul_cam=False, multi_view_patch_size=3, multi_view_sample_num=c.k,
                          multi_view_pixel_noise_th=1.0, multi_view_ncc_weight=0.15, multi_view_geo_weight=0.03, metallic_warp_weight=0.05,
                          roughness_warp_weight=0.05, wo_use_geo_occ_aware=False, directional_rghmtl_warp_alignment=True, srgb=False)
    cam0 = SimpleNamespace(**c.cams[0]._asdict(), image_name="view0", nearest_id=[0], ncc_scale=1.0)
    rendered = []
    render = lambda cam, *a, **k: (rendered.append(cam), c.pk[1])[1]
    scene = SimpleNamespace(getTrainCameras=lambda: [c.cams[1]])
    edges = lambda normal, dilate_size: (~c.keep).float()
    args = (cam0, scene, opt, None, None, None, render, c.pk[0], None, None, None, {"view0": c.fg}, c.it, None, None)
    kw = dict(use_metallic_warp=True, use_roughness_warp=True, edges_fn=edges, samples=samples.int())
    if c.refreal:
        with pytest.raises(NotImplementedError, match="without_ncc"):
            mv.calc_warp_loss_refreal(*args, **kw)
        r = mv.calc_warp_loss_refreal(*args, without_ncc=True, **kw)
        assert r[1] is None and tuple(r[6].shape) == (H, W) and r[6].device.type == "cpu" and r[7] is None
    else:
        r = mv.calc_warp_loss(*args, **kw)
        assert r[0] is None and r[1] is None and r[6] is None and r[7] is None
    assert len(rendered) == 1 and rendered[0] is c.cams[1]
    terms = [r[0], r[2], r[3], r[4]]
    present, ref = Z[f"{name}_present"], Z[f"{name}_terms"]
    assert float((r[5].double() - torch.from_numpy(Z[f"{name}_weight"]).to(dev)).abs().max()) < 1e-5
    live = []
    for i in range(4):
        if not present[i]:
            # None in the reference: None here too, except a term the reference drops for want of a valid pixel (0 here)
            assert terms[i] is None or float(terms[i]) == 0.0, (name, i)
            continue
        if math.isnan(ref[i]):
            assert math.isnan(float(terms[i])), (name, i)
            continue
        assert abs(float(terms[i]) - ref[i]) <= 1e-5 * abs(ref[i]), (name, i, float(terms[i]), ref[i])
        live.append(i)
    if not live:
        return
    torch.autograd.backward([terms[i] for i in live], [torch.tensor(UP[i], device=dev) for i in live])
    for j, (who, m) in enumerate([(w, m) for w in ("v", "n") for m in MAPS]):
        gref = torch.from_numpy(Z[f"{name}_g_{who}_{m}"]).to(dev).double()
        p = c.pk[0 if who == "v" else 1][m]
        g = torch.zeros_like(gref) if p.grad is None else p.grad.double().reshape(gref.shape)
        scale = float(gref.abs().max())
        if scale == 0:
            assert float(g.abs().max()) == 0, (name, who, m)
            continue
        excl = torch.zeros(H, W, dtype=torch.bool, device=dev)
        if m != "surf_depth" and o["excl_tap"] is not None:
            et = o["excl_tap"] | o["excl_sample"][:, None]
            if who == "v":
                tx, ty = o["tx"][et], o["ty"][et]
                ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                excl.view(-1)[ty[ok] * W + tx[ok]] = True
            else:
                G = o["g"][et]
                ok = torch.isfinite(G).all(-1) & (G[:, 0] > -2) & (G[:, 0] < W + 1) & (G[:, 1] > -2) & (G[:, 1] < H + 1)
                for dx in (0, 1):
                    for dy in (0, 1):
                        xx, yy = G[ok, 0].floor().long() + dx, G[ok, 1].floor().long() + dy
                        inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                        excl.view(-1)[yy[inb] * W + xx[inb]] = True
        d = (g - gref).abs().reshape(-1, H, W).amax(0)
        touched = (gref != 0).reshape(-1, H, W).any(0)
        assert int(((d > 1e-4 * scale) & ~excl).sum()) == 0, (name, who, m, float(d[~excl].max()) / scale)
        assert int((excl & touched).sum()) <= max(64, 5e-3 * int(touched.sum())), (name, who, m, int((excl & touched).sum()))
