"""The edge mask of the multi-view loss (materialrefgs_amd.edges, csrc/mrgs_edges.hip; the definition is stated in include/mrgs.h).
Without a GPU: known answers that pin the rules of the numpy statement (tests/edges_statement.py).  With one (-m gpu): the native mask
and class map against the statement, bit for bit -- the operation is integer, so there is no tolerance anywhere in this file."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edges_statement as es  # noqa: E402


def _tile():
    """The width and height of the classify tile, read from the kernel file (its EDGE_TILE constant)."""
    src = open(os.path.join(ROOT, "materialrefgs_amd", "csrc", "mrgs_edges.hip")).read()
    return int(re.search(r"constexpr int EDGE_TILE = (\d+);", src).group(1))


T = _tile()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def noise_image(H, W, seed=0, signed=False, sigma=0.04):
    """fp32 noise 0.5 + 0.04 N(0, 1) per channel: gradients around the default thresholds, so that strong, promoted and dropped
    candidates all occur (full-range noise would make every candidate strong and a 7 x 7 dilation fill the image).  `signed`: the same
    noise scaled into [-1, 1] as a normal map is; its negative values exercise the wrap, which makes nearly every candidate strong."""
    x = (0.5 + sigma * np.random.default_rng(seed).standard_normal((3, H, W))).astype(np.float32)
    return (2.0 * (x - 0.5)).astype(np.float32) if signed else x


def step_image(H, W, row=None, col=None):
    img = np.zeros((3, H, W), dtype=np.float32)
    if col is not None:
        img[:, :, col:] = 1.0
    if row is not None:
        img[:, row:, :] = 1.0
    return img


def disk_image(seeded):
    """300 x 300, 10 / 255 inside the disk of radius 120 around (150, 150): one ring of weak candidates; `seeded` adds a 4 x 4 block of
    1.0 on its top, the only strong pixels."""
    yy, xx = np.mgrid[0:300, 0:300]
    g = np.where((yy - 150) ** 2 + (xx - 150) ** 2 <= 120 ** 2, np.float32(10.0 / 255.0), np.float32(0.0)).astype(np.float32)
    if seeded:
        g[28:32, 148:152] = 1.0
    return np.stack([g, g, g])


def _classes_of(img, t1=0.0, t2=80.0):
    return es.classes(es.grey(es.quantise(img)), t1, t2)


# ---- CPU: the rules -------------------------------------------------------------------------------------------------------------------
def test_vertical_step_puts_the_tie_on_the_left_pixel():
    cls = _classes_of(step_image(9, 12, col=6))
    want = np.zeros((9, 12), dtype=bool)
    want[:, 5] = True
    assert np.array_equal(cls > 0, want)


def test_horizontal_step_puts_the_tie_on_the_top_pixel():
    cls = _classes_of(step_image(9, 12, row=5))
    want = np.zeros((9, 12), dtype=bool)
    want[4, :] = True
    assert np.array_equal(cls > 0, want)


def test_quantise_wraps_and_zeroes():
    q = es.quantise(np.array([-0.5, 1.0, np.nan, np.inf, -np.inf, 1e30, 0.0], dtype=np.float32))
    assert q.tolist() == [129, 255, 0, 0, 0, 0, 0]
    assert es.grey(np.array([[[255]], [[255]], [[255]]])).tolist() == [[255]]


def test_swapped_thresholds():
    img = noise_image(40, 50, seed=3, sigma=0.1)
    a, ca = es.edge_mask(img, 4, 150.0, 50.0)
    b, cb = es.edge_mask(img, 4, 50.0, 150.0)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    assert (ca == 1).any() and (ca == 2).any()


@pytest.mark.parametrize("d", [1, 2, 4, 7])
def test_dilate_window_and_clipping(d):
    H, W, a = 15, 17, d // 2
    for (y, x) in [(7, 8), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        e = np.zeros((H, W), dtype=bool)
        e[y, x] = True
        # out[v, u] is set where (y, x) lies in the window of (v, u): v + oy = y with oy in [-a, d-1-a], so v in [y-(d-1-a), y+a]
        want = np.zeros((H, W), dtype=bool)
        want[max(0, y - (d - 1 - a)):min(H, y + a + 1), max(0, x - (d - 1 - a)):min(W, x + a + 1)] = True
        assert np.array_equal(es.dilate(e, d), want), (d, y, x)
    mid = np.zeros((H, W), dtype=bool)
    mid[7, 8] = True
    assert int(es.dilate(mid, d).sum()) == d * d


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (2, 3)])
def test_tiny_images(H, W):
    img = np.full((3, H, W), 0.3, dtype=np.float32)
    cls = _classes_of(img)
    assert cls.shape == (H, W) and not cls.any()
    for d in (1, 2, 4, 7):
        assert not es.dilate(np.zeros((H, W), dtype=bool), d).any()
        assert es.dilate(np.ones((H, W), dtype=bool), d).all()
    mask, _ = es.edge_mask(img, 7)
    assert not mask.any()


def test_abi_argument_checks_without_gpu():
    """Every refusal of mrgs_edge_mask comes before the first HIP call, so it can be asked for without a device."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    assert L.mrgs_edges_ws_bytes(0, 5) == 0 and L.mrgs_edges_ws_bytes(5, -1) == 0 and L.mrgs_edges_ws_bytes(65536, 32768) == 0
    need = L.mrgs_edges_ws_bytes(100, 260)
    assert need >= 100 * 260 * 6
    one = ctypes.c_void_p(256)                           # a non-NULL address that is never dereferenced: the call returns first
    call = lambda H=100, W=260, d=7, t1=0.0, t2=80.0, img=one, out=one, ws=one, n=need: L.mrgs_edge_mask(img, H, W, d, t1, t2, 0, out, None, ws,
                                                                                                         n, None)
    assert call(H=0) == _lib.MRGS_E_BAD_ARG and call(W=-3) == _lib.MRGS_E_BAD_ARG
    assert call(d=0) == _lib.MRGS_E_BAD_ARG and call(d=32) == _lib.MRGS_E_BAD_ARG
    assert call(t1=float("nan")) == _lib.MRGS_E_BAD_ARG and call(t2=float("nan")) == _lib.MRGS_E_BAD_ARG
    assert call(img=None) == _lib.MRGS_E_BAD_ARG and call(out=None) == _lib.MRGS_E_BAD_ARG and call(ws=None) == _lib.MRGS_E_BAD_ARG
    assert call(H=65536, W=32768) == _lib.MRGS_E_UNSUPPORTED
    assert call(n=need - 1) == _lib.MRGS_E_WORKSPACE


def test_python_wrapper_refuses_what_it_cannot_serve():
    from materialrefgs_amd import edges
    with pytest.raises(RuntimeError, match="device tensor"):
        edges.edge_mask(torch.zeros(3, 8, 8))
    with pytest.raises(TypeError, match="float32"):
        edges.edge_mask(torch.zeros(3, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        edges.edge_mask(torch.zeros(1, 8, 8))
    with pytest.raises(RuntimeError, match="device tensor"):
        edges.dilated_edges_imgs(torch.zeros(3, 8, 8))


# ---- GPU: bit for bit against the statement ---------------------------------------------------------------------------------------------
def _check(dev, img, d=7, t1=0.0, t2=80.0, invert=False, classes=True):
    from materialrefgs_amd import edges
    want_mask, want_cls = es.edge_mask(img, d, t1, t2, invert)
    r = edges.edge_mask(torch.from_numpy(img).to(dev), d, t1, t2, invert=invert, classes=classes)
    mask, cls = r if classes else (r, None)
    assert mask.dtype is torch.bool and tuple(mask.shape) == img.shape[1:] and mask.device.type == "cuda"
    assert torch.equal(mask.cpu(), torch.from_numpy(want_mask)), (img.shape, d, t1, t2, invert)
    if classes:
        assert cls.dtype is torch.uint8
        assert torch.equal(cls.cpu(), torch.from_numpy(want_cls)), (img.shape, d, t1, t2)
    return want_mask, want_cls


# 1 x 1 ... 3 x 3, then one below, at and above the classify tile (T, read from the kernel file above) in each dimension, then several tiles
SIZES = [(1, 1), (1, 7), (2, 3), (3, 3)] + [(h, w) for h in (T - 1, T, T + 1) for w in (T - 1, T, T + 1)] + [(100, 260)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("signed", [False, True])
def test_noise_against_statement(gpu_device, H, W, signed):
    img = noise_image(H, W, seed=H * 1000 + W, signed=signed)
    _mask, cls = _check(gpu_device, img, d=4)
    _check(gpu_device, img, d=7, invert=True, classes=False)
    if (H, W) == (100, 260) and not signed:
        edge = es.hysteresis(cls)
        n = float(H * W)
        strong, promoted, dropped = (cls == 2).sum() / n, ((cls == 1) & edge).sum() / n, ((cls == 1) & ~edge).sum() / n
        assert strong >= 0.01 and promoted >= 0.01 and dropped >= 0.01, (strong, promoted, dropped)
    if signed and H * W > 100:
        assert (img < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("t1,t2", [(0.0, 80.0), (50.0, 150.0), (150.0, 50.0), (80.0, 80.0)])
@pytest.mark.parametrize("d", [1, 2, 4, 7])
def test_parameters(gpu_device, t1, t2, d):
    img = noise_image(100, 260, seed=11)
    _check(gpu_device, img, d, t1, t2, invert=False, classes=True)
    _check(gpu_device, img, d, t1, t2, invert=True, classes=False)


@pytest.mark.gpu
def test_largest_window_and_steps(gpu_device):
    _check(gpu_device, noise_image(70, 45, seed=5, sigma=0.1), d=31, t1=100.0, t2=200.0)
    _check(gpu_device, step_image(9, 12, col=6), d=2)
    _check(gpu_device, step_image(9, 12, row=5), d=2)
    special = noise_image(20, 30, seed=2)
    special[0, 3, 4], special[1, 5, 6], special[2, 7, 8], special[0, 9, 9] = np.nan, np.inf, -np.inf, 3e9
    _check(gpu_device, special, d=4)


@pytest.mark.gpu
def test_one_long_component_is_carried_across_tiles(gpu_device):
    """A ring of ~800 weak candidates that spans 240 pixels both ways: without a strong pixel nothing is an edge; with strong pixels in a
    6 x 6 box on its top the whole ring is -- the labels have to travel across many tiles."""
    plain, seeded = disk_image(False), disk_image(True)
    cls0 = _classes_of(plain)
    labels, n = es.components(cls0)
    ys, xs = np.nonzero(cls0)
    assert n == 1 and int((cls0 > 0).sum()) == 792 and not (cls0 == 2).any()
    assert ys.max() - ys.min() >= 200 and xs.max() - xs.min() >= 200
    cls1 = _classes_of(seeded)
    labels, n = es.components(cls1)
    ys, xs = np.nonzero(cls1)
    sy, sx = np.nonzero(cls1 == 2)
    assert n == 1 and int((cls1 > 0).sum()) == 798
    assert ys.max() - ys.min() >= 200 and xs.max() - xs.min() >= 200
    assert len(sy) > 0 and sy.min() >= 27 and sy.max() <= 31 and sx.min() >= 147 and sx.max() <= 152
    assert int(es.hysteresis(cls1).sum()) == 798
    m0, _ = _check(gpu_device, plain, d=1)
    assert not m0.any()
    m1, _ = _check(gpu_device, seeded, d=1)
    assert int(m1.sum()) == 798
    _check(gpu_device, seeded, d=7, invert=True)


@pytest.mark.gpu
def test_errors(gpu_device):
    from materialrefgs_amd import _lib, edges
    dev = gpu_device
    L = _lib.lib()
    H, W = 40, 50
    img = torch.from_numpy(noise_image(H, W)).to(dev)
    need = L.mrgs_edges_ws_bytes(H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((H, W), 7, dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr(dev)
    call = lambda d=7, n=need: L.mrgs_edge_mask(img.data_ptr(), H, W, d, 0.0, 80.0, 0, out.data_ptr(), None, ws.data_ptr(), n, st)
    assert call(n=need - 1) == _lib.MRGS_E_WORKSPACE
    assert call(d=0) == _lib.MRGS_E_BAD_ARG and call(d=32) == _lib.MRGS_E_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all())                        # a refused call leaves `out` untouched
    assert call() == _lib.MRGS_OK
    assert torch.equal(out.cpu().bool(), torch.from_numpy(es.edge_mask(img.cpu().numpy(), 7)[0]))
    with pytest.raises(RuntimeError, match="device tensor"):
        edges.edge_mask(img.cpu())
    with pytest.raises(TypeError, match="float32"):
        edges.edge_mask(img.half())
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        edges.edge_mask(img[:1])
    # a view that is not contiguous is made so
    wide = torch.from_numpy(noise_image(H, 2 * W, seed=4)).to(dev)
    assert torch.equal(edges.edge_mask(wide[:, :, ::2]).cpu(), torch.from_numpy(es.edge_mask(wide[:, :, ::2].cpu().numpy(), 4)[0]))


@pytest.mark.gpu
def test_dilated_edges_imgs_keeps_the_reference_convention(gpu_device):
    from materialrefgs_amd import edges
    img = noise_image(61, 83, seed=9, signed=True)
    r = edges.dilated_edges_imgs(torch.from_numpy(img).to(gpu_device), dilate_size=7)
    assert r.dtype is torch.float64 and r.device.type == "cuda" and tuple(r.shape) == (61, 83)
    assert torch.equal(r.cpu(), torch.from_numpy(es.edge_mask(img, 7)[0].astype(np.float64)))
    r4 = edges.dilated_edges_imgs(torch.from_numpy(img).to(gpu_device))
    assert torch.equal(r4.cpu(), torch.from_numpy(es.edge_mask(img, 4)[0].astype(np.float64)))


@pytest.mark.gpu
def test_call_is_legal_inside_a_stream_capture(gpu_device):
    """mrgs_edge_mask allocates nothing, reads nothing back and does not synchronise: it can be captured, and the replay (a chain of four
    kernels, no parallel branch) computes the mask of whatever the input buffer then holds."""
    from materialrefgs_amd import edges
    dev = gpu_device
    first, second = noise_image(50, 70, seed=1), noise_image(50, 70, seed=2, signed=True)
    buf = torch.from_numpy(first).to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        edges.edge_mask(buf, 7, invert=True)             # loads the code object outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask, cls = edges.edge_mask(buf, 7, invert=True, classes=True)
    buf.copy_(torch.from_numpy(second).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    want_mask, want_cls = es.edge_mask(second, 7, invert=True)
    assert torch.equal(mask.cpu(), torch.from_numpy(want_mask)) and torch.equal(cls.cpu(), torch.from_numpy(want_cls))


# ---- the drop-ins ---------------------------------------------------------------------------------------------------------------------
def faceted(normal, block=12, amount=0.25, seed=0):
    """`normal` [3,H,W] with one random offset per block x block cell, renormalised: edges along the cell borders all over the object, so
    that the mask decides about samples the loss uses (the smooth sphere of the analytic scene has edges on its silhouette only)."""
    rng = np.random.default_rng(seed)
    _, H, W = normal.shape
    cells = rng.standard_normal((3, (H + block - 1) // block, (W + block - 1) // block))
    n = normal.astype(np.float64) + amount * np.repeat(np.repeat(cells, block, axis=1), block, axis=2)[:, :H, :W]
    return (n / np.linalg.norm(n, axis=0, keepdims=True)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("refreal", [False, True])
def test_drop_in_computes_its_own_mask(gpu_device, refreal):
    """calc_warp_loss / calc_warp_loss_refreal with opt.edge_aware_in_warp and no edges_fn: the same tuple, element by element, as with
    the statement handed in as edges_fn.  Two analytic cameras (the scene of the multi-view tests), a fixed draw."""
    from materialrefgs_amd import multiview as mv
    from multiview_statement import analytic_pair
    import test_multiview_loss as tml
    dev = gpu_device
    H, W = 48, 64
    v, n = analytic_pair(H, W)
    normal = faceted(v.normal.numpy())
    keep_stmt = es.edge_mask(normal, 7, invert=True)[0]
    assert 0.05 < keep_stmt.mean() < 0.95, keep_stmt.mean()
    npk = tml._dev_pkg(n, dev)
    fg = {"view0": v.fg.to(dev)}
    cam0 = SimpleNamespace(**v.cam.to(dev)._asdict(), image_name="view0", nearest_id=[0], ncc_scale=1.0)
    scene = SimpleNamespace(getTrainCameras=lambda: [n.cam.to(dev)])
    samples = torch.arange(0, H * W, 3, dtype=torch.int32)
    seen = []

    def statement_fn(img, dilate_size):
        seen.append(dilate_size)
        return torch.from_numpy(es.edge_mask(img.detach().cpu().numpy(), dilate_size)[0].astype(np.float64))

    def run(edges_fn):
        opt = SimpleNamespace(edge_aware_in_warp=True, use_virtul_cam=False, multi_view_patch_size=3, multi_view_sample_num=samples.numel(),
                              multi_view_pixel_noise_th=1.0, multi_view_ncc_weight=0.15, multi_view_geo_weight=0.03, metallic_warp_weight=0.05,
                              roughness_warp_weight=0.05, wo_use_geo_occ_aware=False, directional_rghmtl_warp_alignment=True, srgb=False)
        vp = tml._dev_pkg(v, dev)
        vp["rend_normal"] = torch.from_numpy(normal).to(dev)
        args = (cam0, scene, opt, None, None, None, lambda cam, *a, **k: npk, vp, None, None, None, fg, 30000, None, None)
        kw = dict(use_metallic_warp=True, use_roughness_warp=True, edges_fn=edges_fn, samples=samples)
        return mv.calc_warp_loss_refreal(*args, without_ncc=True, **kw) if refreal else mv.calc_warp_loss(*args, **kw)

    native, given = run(None), run(statement_fn)
    assert seen == [7]
    assert len(native) == len(given) == 8
    live = 0
    for a, b in zip(native, given):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
            live += 1
    assert live >= (6 if refreal else 4)
    # the mask matters here: it gates the metallic and roughness terms (not the base colour's), and without it they differ
    plain = run(lambda img, dilate_size: torch.zeros(H, W))
    assert torch.equal(plain[2], native[2]) and not torch.equal(plain[3], native[3]) and not torch.equal(plain[4], native[4])
