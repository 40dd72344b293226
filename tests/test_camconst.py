"""materialrefgs_amd._camconst: every launch constant the host path derives from a camera, against the expressions the call sites used
to carry (written out here), and the one staleness rule of its one per-camera cache."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from materialrefgs_amd import _camconst as cc
from materialrefgs_amd.camera import look_at_camera

H, W = 48, 64
CPU = torch.device("cpu")


def _k(fx=500.0, fy=500.0, cx=32.0, cy=24.0):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def _mini():
    return look_at_camera(30.0, 20.0, 4.0, 0.8, H, W)


def _bare():
    """numpy R, T and HWK only (the camera of the staleness test)."""
    return SimpleNamespace(R=np.eye(3, dtype=np.float32), T=np.array([0.0, 0.0, 3.0], dtype=np.float32), HWK=(H, W, _k()))


def _off_centre():
    """Fx / Fy / Cx / Cy that are not what the field of view and the image centre give; a float64 pose."""
    c = look_at_camera(-70.0, 35.0, 3.0, 0.9, H, W)
    return SimpleNamespace(image_height=H, image_width=W, FoVx=c.FoVx, FoVy=c.FoVy, Fx=71.25, Fy=69.5, Cx=30.125, Cy=25.75,
                           R=c.R.double().numpy(), T=c.T.double().numpy(), world_view_transform=c.world_view_transform,
                           HWK=(H, W, _k(71.25, 69.5, 30.125, 25.75)))


def _flat32(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float32).reshape(-1)


def test_values_are_the_call_sites_expressions():
    for cam in (_mini(), _off_centre()):
        fx = getattr(cam, "Fx", None)
        fy = getattr(cam, "Fy", None)
        if fx is None:
            fx = W / (2.0 * math.tan(cam.FoVx * 0.5))
        if fy is None:
            fy = H / (2.0 * math.tan(cam.FoVy * 0.5))
        assert cc.focal(cam) == (float(fx), float(fy), float(getattr(cam, "Cx", 0.5 * W)), float(getattr(cam, "Cy", 0.5 * H)))
        assert cc.fov_focal(cam) == (W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5)))
    assert cc.focal(_off_centre()) == (71.25, 69.5, 30.125, 25.75) and cc.fov_focal(_off_centre())[0] != 71.25
    for cam in (_mini(), _bare(), _off_centre()):
        c = cc.consts(cam, CPU)
        kinv = tuple(np.linalg.inv(np.asarray(cam.HWK[2], dtype=np.float32)).astype(np.float32).reshape(-1).tolist())
        assert cc.kinv(cam.HWK[2]) == kinv and c.Kinv == kinv
        for got, src in ((c.R, cam.R), (c.T, cam.T)):
            want = torch.as_tensor(src, dtype=torch.float32, device=CPU).contiguous()
            assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape and torch.equal(got, want)
        R = cam.R
        R = R.detach().to("cpu", torch.float32).numpy() if torch.is_tensor(R) else np.asarray(R, dtype=np.float32)
        assert c.rt_host == tuple(float(x) for x in R.T.reshape(-1))
        assert c.r_host == tuple(_flat32(cam.R).tolist()) and c.t_host == tuple(_flat32(cam.T).tolist())
        assert len(c.r_host) == 9 and len(c.t_host) == 3
    for cam in (_mini(), _off_centre()):
        c = cc.consts(cam, CPU)
        parts = [torch.as_tensor(t).reshape(-1).to(torch.float32) for t in (cam.world_view_transform, cam.R, cam.T)]
        assert c.record.dtype == torch.float32 and c.record.shape == (28,) and torch.equal(c.record, torch.cat(parts))
        assert c.record_host == tuple(torch.cat([_flat32(t) for t in (cam.world_view_transform, cam.R, cam.T)]).tolist())


def test_camera_constants_follow_an_in_place_pose_change():
    """K^-1 / R / T are cached per camera object; a pose refined in place (same object, same arrays) or new intrinsics must not be served
    from the cache."""
    K = np.array([[500.0, 0, 32], [0, 500.0, 24], [0, 0, 1]], dtype=np.float32)
    cam = SimpleNamespace(R=np.eye(3, dtype=np.float32), T=np.array([0.0, 0.0, 3.0], dtype=np.float32), HWK=(48, 64, K))
    dev = torch.device("cpu")
    camera_consts = lambda cam, dev: (cc.consts(cam, dev).Kinv, cc.consts(cam, dev).R, cc.consts(cam, dev).T)   # noqa: E731
    k0, r0, t0 = camera_consts(cam, dev)
    k1, r1, t1 = camera_consts(cam, dev)
    assert r1 is r0 and t1 is t0 and k1 == k0                      # unchanged camera: the cached tensors
    cam.T[2] = 5.0                                                 # in place
    _, _, t2 = camera_consts(cam, dev)
    assert float(t2[2]) == 5.0
    cam.R[:] = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], dtype=np.float32)
    _, r3, _ = camera_consts(cam, dev)
    assert float(r3[0, 1]) == 1.0 and float(r3[0, 0]) == 0.0
    K[0, 0] = 250.0
    k4, _, _ = camera_consts(cam, dev)
    assert abs(k4[0] - 1.0 / 250.0) < 1e-9


def test_records_follow_an_in_place_write_to_the_view_matrix():
    cam = _mini()
    c0 = cc.consts(cam, CPU)
    rec0, host0 = c0.record.clone(), c0.record_host
    assert cc.consts(cam, CPU) is c0 and cc.consts(cam, CPU).record is c0.record
    cam.world_view_transform[3, 0] += 0.5
    c1 = cc.consts(cam, CPU)
    want = float(cam.world_view_transform[3, 0])
    assert c1 is not c0 and float(c1.record[12]) == want and c1.record_host[12] == want
    assert float(rec0[12]) != want and host0[12] != want
    assert torch.equal(c1.record[:12], rec0[:12]) and c1.record_host[13:] == host0[13:]


def test_a_missing_source_only_matters_to_the_field_that_needs_it():
    m = _mini()
    no_hwk = SimpleNamespace(R=m.R, T=m.T, world_view_transform=m.world_view_transform)
    c = cc.consts(no_hwk, CPU)
    assert c.record.shape == (28,) and len(c.record_host) == 28 and len(c.r_host) == 9
    with pytest.raises(AttributeError):
        c.Kinv
    c = cc.consts(_bare(), CPU)                                    # no world_view_transform
    assert len(c.Kinv) == 9 and c.R.shape == (3, 3) and c.T.shape == (3,) and len(c.rt_host) == 9
    for field in ("record", "record_host"):
        with pytest.raises(AttributeError):
            getattr(c, field)
    only_r = cc.consts(SimpleNamespace(R=np.arange(9.0).reshape(3, 3)), CPU)
    assert only_r.rt_host == (0.0, 3.0, 6.0, 1.0, 4.0, 7.0, 2.0, 5.0, 8.0)
    with pytest.raises(AttributeError):
        only_r.T


def test_every_accessor_shares_one_entry_per_camera():
    """What the renderer, the priors, refscore, multiview, ballquery and the contact sheet read of n cameras leaves n entries."""
    from materialrefgs_amd import refscore, visualize
    cams = [look_at_camera(40.0 * i, 15.0, 4.0, 0.8, H, W) for i in range(5)]
    cc._CAMERAS.clear()
    for _ in range(2):
        for cam in cams:
            c = cc.consts(cam, CPU)
            (c.Kinv, c.R, c.T), c.rt_host                                                        # renderer, shading, priors
            refscore._cam_record(cam, CPU, "record_host"), refscore._cam_record(cam, CPU, "record")
            cc.consts(cam, CPU).record                                                           # multiview
            cc.consts(cam, CPU).r_host, cc.consts(cam, CPU).t_host                               # ballquery
            visualize.view_rotation(cam, CPU), visualize.view_rotation(cam)
    assert len(cc._CAMERAS) == len(cams)
    assert all(cc.consts(cam, CPU).cam is cam for cam in cams)


@pytest.mark.gpu
def test_device_record_and_pose_make_no_host_read(gpu_device):
    """A cold cache and a camera whose pose tensors and view matrix live on the device: `record`, `R` and `T` under sync-debug "error"."""
    host = _mini()
    cam = host.to(gpu_device)
    cc._CAMERAS.clear()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        c = cc.consts(cam, gpu_device)
        record, R, T = c.record, c.R, c.T
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = torch.cat([_flat32(t) for t in (host.world_view_transform, host.R, host.T)])
    assert record.dtype == torch.float32 and record.device == gpu_device and torch.equal(record.cpu(), want)
    assert torch.equal(R.cpu(), host.R) and torch.equal(T.cpu(), host.T)
    assert c.record_host == tuple(want.tolist())                   # the one host read, outside the mode
