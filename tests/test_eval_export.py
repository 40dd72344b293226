"""8-bit export of a view's maps (csrc/mrgs_eval.hip: mrgs_export_rgb8 behind materialrefgs_amd.evaluate.to_rgb8) and the PNG writer.
Exact equality everywhere: UNIT / NORMAL against torch's own mul(255).add(0.5).clamp(0, 255).to(uint8) on the CPU in float32 (what
torchvision.utils.save_image runs), DEPTH levels against the reference's numpy statement (tests/golden/reference_eval.npz) and the float32
numpy statement of tests/eval_statement.py, bytes against the table."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_statement as es  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_eval.npz"))
SHAPES = ((5, 7), (33, 64), (1, 1))                                   # planes not 16-byte aligned and rows of 21 bytes; several chunks; one pixel


def _torch_unit(x):
    return x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)          # torchvision.utils.save_image, float32 on the CPU


def _edge_values():
    """Every k / 255 and (k +- 0.5) / 255 with their two float32 neighbours, negatives, values above 1, +-inf -- no NaN."""
    k = np.arange(256, dtype=np.float64)
    base = np.concatenate([k / 255, (k + 0.5) / 255, (k - 0.5) / 255]).astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf)),
                           np.array([-1.0, -1e-3, -1e-30, -0.0, 1.0 + 1e-6, 1.5, 2.0, 300.0, 1e30, np.inf, -np.inf], dtype=np.float32)])
    return vals.astype(np.float32)


def _fill(shape, values, seed):
    """A float32 tensor of `shape` that holds every one of `values` when it has room, the rest drawn from them."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    flat = values[rng.integers(0, len(values), n)]
    if n >= len(values):
        flat[rng.permutation(n)[: len(values)]] = values
    return torch.from_numpy(flat.reshape(shape).copy())


def read_png(path):
    """(H, W, bytes [H,W,3]) of an 8-bit RGB non-interlaced PNG whose rows all use filter type 0."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, tag = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return H, W, rows[:, 1:].reshape(H, W, 3)


# ---------------------------------------------------------------- CPU
def test_table_is_the_formula():
    from materialrefgs_amd import evaluate as ev
    t = ev.jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert np.array_equal(t, es.jet_table())
    assert tuple(t[0]) == (0, 0, 128) and tuple(t[255]) == (128, 0, 0)


def test_statement_levels_are_the_reference_levels():
    for tag in "abcd":
        assert np.array_equal(es.depth_levels(GOLD[f"{tag}_depth"][0]), GOLD[f"{tag}_depth_levels"])
        assert GOLD[f"{tag}_depth_levels"].min() == 0 and GOLD[f"{tag}_depth_levels"].max() == 255


def test_statement_bytes_are_torchs():
    x = torch.from_numpy(_edge_values())
    assert np.array_equal(es.unit_bytes(x.numpy()), _torch_unit(x).numpy())
    assert np.array_equal(es.normal_bytes(x.numpy()), _torch_unit(x * 0.5 + 0.5).numpy())


@pytest.mark.parametrize("shape", ((5, 7), (33, 64)))
def test_write_png_round_trip(shape, tmp_path):
    from materialrefgs_amd import evaluate as ev
    H, W = shape
    a = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    ev.write_png(path, a)
    h, w, back = read_png(path)
    assert (h, w) == (H, W) and np.array_equal(back, a)
    ev.write_png(path, torch.from_numpy(a), level=1)
    assert np.array_equal(read_png(path)[2], a)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), a)
    with pytest.raises(ValueError):
        ev.write_png(path, a.astype(np.float32))


def test_export_bad_arguments_are_refused_before_any_launch():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    BAD_ARG, WORKSPACE = 1, 5
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ws_need = L.mrgs_export_ws_bytes()

    def call(H=5, W=7, maps=((p, 3, 0),), n=None, ws=p, ws_bytes=ws_need, out=p, flags=0, size=None):
        table = (_lib.MrgsExportMap * max(1, len(maps)))(*[_lib.MrgsExportMap(*m) for m in maps])
        cfg = _lib.MrgsExportConfig(H, W, len(maps) if n is None else n, flags)
        if size is not None:
            cfg.struct_size = size
        return L.mrgs_export_rgb8(ctypes.byref(cfg), table, ws, ws_bytes, out, None)
    assert call(H=0) == BAD_ARG and call(W=0) == BAD_ARG and call(flags=2) == BAD_ARG and call(size=16) == BAD_ARG
    assert call(maps=()) == BAD_ARG and call(maps=((p, 3, 0),) * 17) == BAD_ARG                       # 17 maps refused
    assert call(maps=((None, 3, 0),)) == BAD_ARG and call(maps=((p, 2, 0),)) == BAD_ARG and call(maps=((p, 3, 3),)) == BAD_ARG
    assert call(maps=((p, 3, 2),)) == BAD_ARG                                                       # DEPTH takes one channel
    assert call(out=None) == BAD_ARG and call(out=p + 1) == BAD_ARG
    assert call(maps=((p, 1, 2),), ws=None) == BAD_ARG and call(maps=((p, 1, 2),), ws_bytes=ws_need - 1) == WORKSPACE
    assert L.mrgs_eval_jet_table(None) == BAD_ARG


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_unit_and_normal_bytes_are_torchs(shape, gpu_device):
    from materialrefgs_amd import evaluate as ev
    H, W = shape
    vals = _edge_values()
    x3, x1 = _fill((3, H, W), vals, 1), _fill((1, H, W), vals, 2)
    n3, n1 = _fill((3, H, W), vals * 2 - 1, 3), _fill((1, H, W), np.concatenate([vals * 2 - 1, vals]), 4)
    out = ev.to_rgb8([(x3.to(gpu_device), "unit"), (x1.to(gpu_device), ev.UNIT), (n3.to(gpu_device), "normal"), (n1.to(gpu_device), ev.NORMAL)])
    assert out.shape == (4, H, W, 3) and out.dtype == torch.uint8 and out.is_cuda
    out = out.cpu()
    assert torch.equal(out[0], _torch_unit(x3).permute(1, 2, 0))
    assert torch.equal(out[1], _torch_unit(x1).repeat(3, 1, 1).permute(1, 2, 0))                    # eval.py:63-64
    assert torch.equal(out[2], _torch_unit(n3 * 0.5 + 0.5).permute(1, 2, 0))                        # eval.py:56
    assert torch.equal(out[3], _torch_unit(n1 * 0.5 + 0.5).repeat(3, 1, 1).permute(1, 2, 0))
    assert np.array_equal(out.numpy(), es.to_rgb8([(x3, "unit"), (x1, "unit"), (n3, "normal"), (n1, "normal")]))


@pytest.mark.gpu
def test_every_edge_value_and_nan(gpu_device):
    """All edge values in one map (a shape with room for them: 48 x 50 = 2400 pixels per plane, three chunks with a partial last one), and
    NaN apart from the torch comparison: byte 0 in UNIT and NORMAL, level 0 in DEPTH."""
    from materialrefgs_amd import evaluate as ev
    vals = _edge_values()
    H, W = 48, 50
    assert H * W >= len(vals)
    x = _fill((3, H, W), vals, 5)
    assert np.isin(vals, x.numpy()).all()
    out = ev.to_rgb8([(x.to(gpu_device), "unit"), ((x * 2 - 1).to(gpu_device), "normal")]).cpu()
    assert torch.equal(out[0], _torch_unit(x).permute(1, 2, 0))
    assert torch.equal(out[1], _torch_unit((x * 2 - 1) * 0.5 + 0.5).permute(1, 2, 0))
    nan = torch.full((1, 5, 7), float("nan"))
    d = torch.linspace(1, 2, 35).reshape(1, 5, 7).clone()
    d[0, 2, 3] = float("nan")
    out = ev.to_rgb8([(nan.to(gpu_device), "unit"), (nan.to(gpu_device), "normal"), (d.to(gpu_device), "depth")]).cpu().numpy()
    assert (out[0] == 0).all() and (out[1] == 0).all()
    table = ev.jet_table()
    assert tuple(out[2, 2, 3]) == tuple(table[0]) and tuple(out[2, 0, 0]) == tuple(table[0]) and tuple(out[2, 4, 6]) == tuple(table[255])
    assert np.array_equal(out[2], table[es.depth_levels(d[0].numpy())])


@pytest.mark.gpu
def test_sixteen_maps_in_one_call_and_seventeen_refused(gpu_device):
    from materialrefgs_amd import evaluate as ev
    H, W = 5, 7
    g = torch.Generator().manual_seed(3)
    maps = []
    for k in range(16):
        t = torch.rand(3 if k % 2 else 1, H, W, generator=g) * 1.6 - 0.3
        maps.append((t, ("unit", "normal", "depth")[k % 3] if t.shape[0] == 1 else ("unit", "normal")[k % 2]))
    assert sum(m == "depth" for _, m in maps) >= 2                     # more than one DEPTH map: each has its own minimum and maximum
    out = ev.to_rgb8([(t.to(gpu_device), m) for t, m in maps]).cpu().numpy()
    assert np.array_equal(out, es.to_rgb8([(t.numpy(), m) for t, m in maps]))
    with pytest.raises(ValueError, match="1..16"):
        ev.to_rgb8([(maps[0][0].to(gpu_device), "unit")] * 17)
    with pytest.raises(ValueError):
        ev.to_rgb8([(maps[0][0].to(gpu_device), "jet")])


@pytest.mark.gpu
def test_depth_levels_and_bytes(gpu_device):
    from materialrefgs_amd import evaluate as ev
    table = ev.jet_table()
    for tag in "abcd":                                                 # the fixture's maps: levels equal the reference's on every pixel
        d = torch.from_numpy(GOLD[f"{tag}_depth"])
        out = ev.to_rgb8([(d.to(gpu_device), "depth")])[0].cpu().numpy()
        assert np.array_equal(out, table[GOLD[f"{tag}_depth_levels"]])
        assert np.array_equal(out, table[es.depth_levels(d[0].numpy())])
    g = torch.Generator().manual_seed(9)
    const = torch.full((1, 33, 64), 3.25)                              # constant: 0 / 1e-20, all level 0
    ties = torch.rand(1, 33, 64, generator=g)
    ties[0, :4] = ties.min()                                           # ties at the minimum and at the maximum
    ties[0, -3:, ::2] = ties.max()
    two = (torch.rand(1, 5, 7, generator=g) > 0.5).float() * 4.0 - 1.0  # two values
    big = torch.rand(1, 300, 1000, generator=g) * 9.0 + 0.5            # more chunks than partial rows of the min/max launch (293 > 256)
    big[0, 299, 999], big[0, 0, 0] = 20.0, 0.25                        # the extremes in the first and the last chunk
    for d in (const, ties, two, big, -big):
        out = ev.to_rgb8([(d.to(gpu_device), "depth")])[0].cpu().numpy()
        levels = es.depth_levels(d[0].numpy())
        assert np.array_equal(out, table[levels])
    assert (es.depth_levels(const[0].numpy()) == 0).all()
    assert set(np.unique(es.depth_levels(two[0].numpy()))) == {0, 255}
    vis = ev.visualize_depth(ties.to(gpu_device))                      # the float form scripts call by name: [3,H,W], table bytes / 255
    assert vis.shape == (3, 33, 64) and vis.dtype == torch.float32
    want = torch.from_numpy(table[es.depth_levels(ties[0].numpy())])
    # `/ 255.` on the device, where the reference divides too (image_utils.py:78: .float().cuda() ... / 255.)
    assert torch.equal(vis, want.to(gpu_device).permute(2, 0, 1).float() / 255.0)
    assert torch.equal((vis.cpu() * 255.0).round().to(torch.uint8), want.permute(2, 0, 1))
    assert torch.equal(ev.visualize_depth(ties[0].to(gpu_device)), vis)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((5, 7), (33, 64)))
def test_save_image_writes_the_unit_bytes(shape, gpu_device, tmp_path):
    from materialrefgs_amd import evaluate as ev
    H, W = shape
    x = torch.rand(3, H, W, generator=torch.Generator().manual_seed(H)) * 1.2 - 0.1
    ev.save_image(x.to(gpu_device), str(tmp_path / "x.png"))
    assert np.array_equal(read_png(str(tmp_path / "x.png"))[2], _torch_unit(x).permute(1, 2, 0).numpy())
    ev.save_image(x[None, :1].to(gpu_device), str(tmp_path / "y.png"))
    assert np.array_equal(read_png(str(tmp_path / "y.png"))[2], _torch_unit(x[:1]).repeat(3, 1, 1).permute(1, 2, 0).numpy())
