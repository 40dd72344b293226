"""csrc/mrgs_image.hip behind materialrefgs_amd.viewstore: the PIL-exact 8-bit resize, the Blender compositing table and the per-iteration
decode.  Every comparison is exact: the resize against Pillow's recorded outputs (tests/golden/pil_resize.npz) and the numpy statement
(tests/scene_statement.py), the compositing against the reference's float64 expression over all 65 536 (colour, alpha) pairs, the decode
against torch CPU ops written as the reference writes them.  No test needs Pillow."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_statement as ss  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pil_resize.npz"))
SIZES = [tuple(int(v) for v in row) for row in GOLD["sizes"]]
BAD_ARG = 1


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("k", range(len(SIZES)))
def test_statement_is_the_pillow_fixture(k):
    h, w, H, W = SIZES[k]
    for kind in ("random", "mask"):
        for mode in ("L", "RGB"):
            a, want = GOLD[f"{k}_{kind}_{mode}_in"], GOLD[f"{k}_{kind}_{mode}_out"]
            assert a.shape[:2] == (h, w) and want.shape[:2] == (H, W)
            assert np.array_equal(ss.resize_u8(a, H, W), want), (k, kind, mode)


def test_statement_is_live_pillow():
    """Where Pillow imports; elsewhere the recorded outputs above stand for it."""
    try:
        from PIL import Image
    except ImportError:
        return
    rng = np.random.default_rng(7)
    for (h, w, H, W) in SIZES + [(31, 45, 77, 5)]:
        for shape, mode in (((h, w), "L"), ((h, w, 3), "RGB")):
            a = rng.integers(0, 256, shape, dtype=np.uint8)
            assert np.array_equal(ss.resize_u8(a, H, W), np.array(Image.fromarray(a, mode).resize((W, H))))
    rgba = rng.integers(0, 256, (20, 24, 4), dtype=np.uint8)               # RGBA as the reference resizes it: four L images
    im = Image.fromarray(rgba, "RGBA")
    split = np.stack([np.array(c.resize((11, 9))) for c in im.split()], axis=-1)
    assert np.array_equal(ss.resize_u8(rgba, 9, 11), split)


def test_host_tables_are_the_statement():
    from materialrefgs_amd import viewstore as vs
    for i, o in [(37, 18), (50, 16), (24, 48), (33, 1), (48, 47), (200, 3), (257, 128), (1600, 800), (800, 1600), (1, 7)]:
        k1, b1, c1 = ss.coefficients(i, o)
        k2, b2, c2 = vs.resize_table(i, o)
        assert k1 == k2 and np.array_equal(b1, b2) and np.array_equal(c1, c2), (i, o)
        assert (b2[:, 0] >= 0).all() and (b2[:, 0] + b2[:, 1] <= i).all() and (b2[:, 1] <= k2).all()      # what the kernel trusts
    for white in (True, False):
        want = ss.composite_reference(ss.all_pairs_rgba(), white)
        assert np.array_equal(vs.composite_table(white), want[:, :, 0]) and np.array_equal(want[:, :, 0], want[:, :, 2])
    n = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    assert torch.equal(torch.from_numpy(vs.normal_table()), ss.decode_normal(n)[:, 0])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)                                             # never dereferenced
    good = dict(channels=3, in_h=8, in_w=8, out_h=4, out_w=4, ksize_x=9, ksize_y=9, flags=0, stride_c=1, stride_y=24, stride_x=3)

    def resize(src=p, dst=p, bx=p, kx=p, by=p, ky=p, ws=p, ws_bytes=1 << 20, size=None, **kw):
        cfg = _lib.MrgsResizeConfig(*dict(good, **kw).values())
        if size is not None:
            cfg.struct_size = size
        return L.mrgs_image_resize_u8(ctypes.byref(cfg), src, bx, kx, by, ky, ws, ws_bytes, dst, None)
    assert L.mrgs_image_resize_u8(None, p, p, p, p, p, p, 0, p, None) == BAD_ARG
    for kw in (dict(size=8), dict(flags=1), dict(channels=0), dict(channels=5), dict(in_h=0), dict(out_w=0), dict(out_h=(1 << 24) + 1),
               dict(stride_x=0), dict(stride_y=-1), dict(stride_c=-1), dict(src=None), dict(dst=None), dict(bx=None), dict(ky=None),
               dict(ksize_x=0), dict(ws=None)):
        assert resize(**kw) == BAD_ARG, kw
    assert resize(ws_bytes=3 * 8 * 4 - 1) == _lib.MRGS_E_WORKSPACE
    assert L.mrgs_image_resize_ws_bytes(3, 8, 8, 4, 4) == 3 * 8 * 4 and L.mrgs_image_resize_ws_bytes(3, 8, 8, 8, 4) == 0
    assert L.mrgs_image_resize_ws_bytes(0, 8, 8, 4, 4) == 0
    assert L.mrgs_image_composite_u8(-1, p, p, p, None) == BAD_ARG
    assert L.mrgs_image_composite_u8(4, None, p, p, None) == BAD_ARG
    assert L.mrgs_image_composite_u8(4, ctypes.c_void_p(0x1002), p, p, None) == BAD_ARG
    assert L.mrgs_image_composite_u8(0, None, None, None, None) == 0

    def dec(size=None, **kw):
        f = dict(H=4, W=4, Hg=4, Wg=4, rgb=0x1000, alpha=None, grey_rgb=None, normal=None, mask=None, score=None, normal_table=None, gt=0x1000,
                 alpha_out=None, grey=None, normal_out=None, mask_out=None, score_out=None, flags=0)
        f.update(kw)
        v = _lib.MrgsViewDecode(*f.values())
        if size is not None:
            v.struct_size = size
        return L.mrgs_view_decode(ctypes.byref(v), None)
    assert L.mrgs_view_decode(None, None) == BAD_ARG
    for kw in (dict(size=16), dict(flags=1), dict(H=0), dict(W=-3), dict(gt=None), dict(rgb=None), dict(alpha_out=0x1000), dict(mask_out=0x1000),
               dict(score_out=0x1000), dict(normal_out=0x1000, normal=0x1000), dict(grey=0x1000), dict(grey=0x1000, grey_rgb=0x1000, Hg=0),
               dict(gt=0x1002)):
        assert dec(**kw) == BAD_ARG, kw


def test_wrappers_refuse_host_tensors():
    from materialrefgs_amd import viewstore as vs
    with pytest.raises(RuntimeError, match="device tensor"):
        vs.resize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), 2, 2)
    with pytest.raises(RuntimeError, match="device tensor"):
        vs.decode(rgb=torch.zeros(3, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        vs.ViewStore("cpu")


# ---------------------------------------------------------------- GPU
def _gpu_resize(a, H, W, dev):
    from materialrefgs_amd import viewstore as vs
    src = torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[:, :, None])).to(dev)
    out = vs.resize_u8(src, H, W).permute(1, 2, 0).cpu()
    return out if a.ndim == 3 else out[:, :, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SIZES)))
def test_resize_is_pillow(gpu_device, k):
    h, w, H, W = SIZES[k]
    for kind in ("random", "mask"):
        for mode in ("L", "RGB"):                                           # 1 and 3 channels against Pillow's recorded bytes
            got = _gpu_resize(GOLD[f"{k}_{kind}_{mode}_in"], H, W, gpu_device)
            assert torch.equal(got, torch.from_numpy(GOLD[f"{k}_{kind}_{mode}_out"])), (kind, mode)
    rng = np.random.default_rng(100 + k)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba[:, :, 1] = checker                                                 # the largest overshoot of the negative lobes
    rgba[:, :, 2] = 255                                                     # clamp and rounding ends
    rgba[:, :, 3] = 0
    assert torch.equal(_gpu_resize(rgba, H, W, gpu_device), torch.from_numpy(ss.resize_u8(rgba, H, W)))


@pytest.mark.gpu
def test_resize_of_planes_equals_resize_of_pixels(gpu_device):
    from materialrefgs_amd import viewstore as vs
    a = torch.from_numpy(GOLD["0_random_RGB_in"]).to(gpu_device)
    planes = a.permute(2, 0, 1).contiguous()
    for (H, W) in ((14, 18), (29, 18), (14, 37), (29, 37)):
        assert torch.equal(vs.resize_u8(planes, H, W, planar=True), vs.resize_u8(a, H, W))
    assert torch.equal(vs.resize_u8(a, 29, 37), planes)


@pytest.mark.gpu
@pytest.mark.parametrize("white", (True, False))
def test_compositing_over_every_pair(gpu_device, white):
    from materialrefgs_amd import viewstore as vs
    rgba = ss.all_pairs_rgba()
    rgba[:, :, 1] = rgba[::-1, :, 0]                                        # three different colours per pixel
    rgba[:, :, 2] = np.roll(rgba[:, :, 0], 77, axis=0)
    got = vs.composite_u8(torch.from_numpy(rgba).to(gpu_device), white).permute(1, 2, 0).cpu()
    assert torch.equal(got, torch.from_numpy(ss.composite_reference(rgba, white)))


def _planes(rng, H, W, Hg, Wg):
    def ramp(shape, shift):                                                 # every byte value when there is room, then random
        n = int(np.prod(shape))
        flat = rng.integers(0, 256, n, dtype=np.uint8)
        flat[:min(n, 256)] = ((np.arange(256) + shift) % 256).astype(np.uint8)[:min(n, 256)]
        return rng.permutation(flat).reshape(shape)
    return dict(rgb=ramp((3, H, W), 0), alpha=ramp((H, W), 3), grey_rgb=ramp((3, Hg, Wg), 5), normal=ramp((H, W, 3), 7), mask=ramp((H, W), 11),
                score=ramp((H, W), 13))


def _decode_statement(p):
    gt = ss.decode_image(p["rgb"].transpose(1, 2, 0))
    return dict(gt=gt, alpha=ss.decode_image(p["alpha"]), grey=ss.decode_grey(ss.decode_image(p["grey_rgb"].transpose(1, 2, 0))),
                normal=ss.decode_normal(p["normal"]), mask=ss.decode_mask(p["mask"]), score=ss.decode_score(p["score"]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((13, 7, 26, 14), (32, 40, 16, 20), (1, 1, 3, 1), (20, 24, 20, 24)))
def test_decode(gpu_device, shape):
    from materialrefgs_amd import viewstore as vs
    H, W, Hg, Wg = shape
    p = _planes(np.random.default_rng(H * 100 + W), H, W, Hg, Wg)
    if H * W >= 256:
        assert all(len(np.unique(v)) == 256 for v in p.values())
    want = _decode_statement(p)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for k, v in p.items()}
    got = vs.decode(**dev)
    assert set(got) == set(vs.OUTPUTS)
    for k in vs.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k]), k
    for absent in vs.OUTPUTS:                                               # each optional output absent in turn
        some = vs.decode(**dev, want=[k for k in vs.OUTPUTS if k != absent])
        assert absent not in some and len(some) == 5
        for k, t in some.items():
            assert torch.equal(t.cpu(), want[k]), (absent, k)
    for only in vs.OUTPUTS:
        assert torch.equal(vs.decode(**dev, want=[only])[only].cpu(), want[only]), only
    same = vs.decode(rgb=dev["rgb"], want=("gt", "grey"))                   # the grey image from the image's own planes
    assert torch.equal(same["grey"].cpu(), ss.decode_grey(want["gt"]))


@pytest.mark.gpu
def test_store_add_and_fetch(gpu_device):
    from materialrefgs_amd import viewstore as vs
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (20, 24, 4), dtype=np.uint8)
    store = vs.ViewStore(gpu_device)
    store.add("blender", rgba, size=(10, 12), grey_size=(20, 24), white_background=True)
    store.add("colmap", rgba, size=(10, 12))
    store.add_prior("blender", normal=rgba[:10, :12, :3], mask=rgba[:10, :12, 3], score=rgba[:10, :12, 0])
    rgb = ss.composite_reference(rgba, True)
    a = store.fetch("blender")
    assert set(a) == {"gt", "grey", "normal", "mask", "score"}              # composited: no alpha plane
    assert torch.equal(a["gt"].cpu(), ss.decode_image(ss.resize_u8(rgb, 10, 12)))
    assert torch.equal(a["grey"].cpu(), ss.decode_grey(ss.decode_image(rgb)))           # 20x24 -> 20x24: the source itself
    assert torch.equal(a["mask"].cpu(), ss.decode_mask(rgba[:10, :12, 3]))
    b = store.fetch("colmap")
    small = ss.resize_u8(rgba, 10, 12)
    assert set(b) == {"gt", "alpha", "grey"}
    assert torch.equal(b["gt"].cpu(), ss.decode_image(small[:, :, :3])) and torch.equal(b["alpha"].cpu(), ss.decode_image(small[:, :, 3]))
    assert torch.equal(b["grey"].cpu(), ss.decode_grey(ss.decode_image(small[:, :, :3])))
    again = store.fetch("colmap")
    assert all(torch.equal(again[k], b[k]) and again[k].data_ptr() != b[k].data_ptr() for k in b)
    assert store.nbytes == 3 * 120 + 3 * 480 + 120 * 5 + 4 * 120
