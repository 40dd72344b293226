"""materialrefgs_amd.scene against the reference's own results (tests/golden/reference_scene.npz, written by
tests/golden/gen_reference_scene_vectors.py from the reference's readers, loadCam, Camera and Scene.__init__ on a small generated dataset
whose files travel in the same archive).  Integers and bytes are compared with array_equal, float32 tensors with torch.equal -- but for
full_proj_transform and camera_center, which the reference forms in float32 arithmetic whose bits belong to the routine that ran: those two
are compared under bounds derived from the formats (_check_float32_routines).

Restated here because they cannot be driven through the reference where the fixture is made (no cv2, no plyfile): the image_msk branch of
loadCam (`cv2.imread(path) != 0`: three channels in B, G, R order) and the points3D.bin -> .ply conversion of readColmapSceneInfo."""
import json
import os
import random
import struct
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_statement as ss  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_scene.npz"))
CASES = [(int(r), bool(w), float(n)) for r, w, n in GOLD["cases"]]
ARGS = dict(images=None, eval=True, relight=False, multi_view_num=3, multi_view_max_angle=40, multi_view_min_dis=0.01, multi_view_max_dis=3.0)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The generated datasets (blender, colmap, colmap_txt) as files."""
    root = tmp_path_factory.mktemp("scene_data")
    for key in GOLD.files:
        if key.startswith("file:"):
            path = root / key[5:]
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(GOLD[key].tobytes())
    return str(root)


def _check_infos(tag, infos):
    assert [c.image_name for c in infos] == list(GOLD[f"{tag}_names"]) and [c.uid for c in infos] == list(GOLD[f"{tag}_uid"])
    for f in ("R", "T", "K"):
        assert np.array_equal(np.stack([getattr(c, f) for c in infos]), GOLD[f"{tag}_{f}"]), (tag, f)
    assert np.array_equal(np.array([[c.FovX, c.FovY] for c in infos]), GOLD[f"{tag}_fov"])
    assert np.array_equal(np.array([[c.width, c.height] for c in infos]), GOLD[f"{tag}_wh"])


def _blender_infos(tree, white):
    from materialrefgs_amd import scene as sc
    path = os.path.join(tree, "blender")
    return sc.readCamerasFromTransforms(path, "transforms_train.json", white) + sc.readCamerasFromTransforms(path, "transforms_test.json", white)


U = 2.0 ** -24                                                          # unit roundoff of float32


def _check_float32_routines(wvt, proj, full, center, ref_full, ref_center, tag):
    """full_proj_transform and camera_center are the two members the reference forms in float32 ARITHMETIC (a 4 x 4 bmm and an inverse,
    on the GPU in a real run, on this container's CPU where the fixture was made), so their last bits belong to whichever routine ran and
    there is nothing to be bit-equal to.  The library rounds the float64 product / inverse once.  Bounds, per entry, from the formats:
      product   a 4-term float32 dot product is within gamma_4 sum|a||b| of the exact one (gamma_4 = 4u / (1 - 4u) < 4.01 u), the
                library's value within u |value| <= u sum|a||b|:                       |ours - reference| <= 5.01 u (|A||B|)_ij
      inverse   an inverse X^ computed from an LU factorisation with partial pivoting satisfies |X^ - X| <= c_n u |X||L^||U^||X| with
                |L^||U^| <= n rho |A| elementwise in the worst case and growth rho = 1 here (the pivots of [R t; 0 1] are bounded by its
                entries); with c_n = 2n and n = 4 that is 32 u (|X||A||X|)_ij, plus u |X|_ij for the library's one rounding."""
    A, B = wvt.double().abs(), proj.double().abs()
    assert bool(((full.double() - ref_full.double()).abs() <= 5.01 * U * (A @ B)).all()), (tag, "full_proj_transform")
    X = torch.linalg.inv(wvt.double()).abs()
    bound = (32 * U * (X @ A @ X) + U * X)[3, :3]
    assert bool(((center.double() - ref_center.double()).abs() <= bound).all()), (tag, "camera_center")
    assert float(bound.max()) < 2e-4                                     # the bound is a statement about rounding, not a loose tolerance
    assert torch.equal(full, (wvt.double() @ proj.double()).float()), (tag, "full_proj_transform is the float64 product rounded once")


def _check_camera(tag, cam):
    for f in ("world_view_transform", "projection_matrix", "R", "T"):     # float64 host arithmetic and one cast: the reference's bits
        got = getattr(cam, f).cpu()
        assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(GOLD[f"{tag}_{f}"])), (tag, f)
    assert cam.full_proj_transform.dtype == torch.float32 and cam.camera_center.dtype == torch.float32
    _check_float32_routines(cam.world_view_transform.cpu(), cam.projection_matrix.cpu(), cam.full_proj_transform.cpu(), cam.camera_center.cpu(),
                            torch.from_numpy(GOLD[f"{tag}_full_proj_transform"]), torch.from_numpy(GOLD[f"{tag}_camera_center"]), tag)
    assert torch.equal(cam.get_k().cpu(), torch.from_numpy(GOLD[f"{tag}_k"])) and torch.equal(cam.get_inv_k().cpu(), torch.from_numpy(GOLD[f"{tag}_inv_k"]))
    assert torch.equal(cam.get_k(2.0).cpu(), torch.from_numpy(GOLD[f"{tag}_k2"])) and torch.equal(cam.get_inv_k(2.0).cpu(), torch.from_numpy(GOLD[f"{tag}_inv_k2"]))
    assert torch.equal(cam.get_rays().cpu(), torch.from_numpy(GOLD[f"{tag}_rays"]))
    assert np.array_equal(np.asarray(cam.HWK[2], dtype=np.float64), GOLD[f"{tag}_hwk_K"])
    assert np.array_equal(np.array([cam.image_height, cam.image_width, cam.HWK[0], cam.HWK[1], cam.Fx, cam.Fy, cam.Cx, cam.Cy], dtype=np.float64),
                          GOLD[f"{tag}_scalars"])
    intr, extr = cam.get_calib_matrix_nerf()
    assert torch.equal(intr, cam.get_k().cpu()) and torch.equal(extr.cpu(), cam.world_view_transform.cpu().T)


def _host_camera(sc, info, resolution, ncc, uid):
    """The Camera loadCam builds, without its photograph: everything but the store."""
    h, w = info.image.shape[:2]
    (rw, rh), scale = sc.target_resolution(w, h, resolution, 1.0)
    K = info.K.copy()
    K[:2] = K[:2] / scale
    return sc.Camera(info.uid, info.R, info.T, info.FovX, info.FovY, None, None, info.image_name, uid, data_device="cpu", HWK=(rh, rw, K), ncc_scale=ncc)


# ---------------------------------------------------------------- CPU: readers
@pytest.mark.parametrize("white", (True, False))
def test_blender_reader(tree, white):
    from materialrefgs_amd import scene as sc
    tag = "blender_white" if white else "blender_black"
    infos = _blender_infos(tree, white)
    _check_infos(tag, infos)
    for k, c in enumerate(infos):
        assert c.image.dtype == np.uint8 and c.image.shape == (20, 24, 4) and c.mode == ("RGBA->white" if white else "RGBA->black")
        assert np.array_equal(sc.composited(c), GOLD[f"{tag}_image_{k}"])           # the RGB image the reference's CameraInfo holds
        assert np.array_equal(ss.composite_reference(c.image, white), GOLD[f"{tag}_image_{k}"])
    norm = sc.getNerfppNorm(infos)
    assert np.array_equal(np.concatenate([norm["translate"], [norm["radius"]]]), GOLD[f"{tag}_norm"])
    assert [sc.camera_to_JSON(k, c) for k, c in enumerate(infos)] == json.loads(str(GOLD[f"{tag}_json"]))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_resolution_rules_and_camera_matrices(tree, case):
    """loadCam's resolution and K (utils/camera_utils.py:43-66) and every matrix of Camera, per case; the photographs through the numpy
    statement of the resize, which ties the statement the kernels are tested against to the reference's own tensors."""
    from materialrefgs_amd import scene as sc
    resolution, white, ncc = CASES[case]
    for k, info in enumerate(_blender_infos(tree, white)):
        tag = f"case{case}_cam{k}"
        cam = _host_camera(sc, info, resolution, ncc, k)
        _check_camera(tag, cam)
        rgb = sc.composited(info)
        H, W = cam.image_height, cam.image_width
        image = ss.decode_image(ss.resize_u8(rgb, H, W))
        assert torch.equal(image, torch.from_numpy(GOLD[f"{tag}_image"]))
        src = image if ncc == 1.0 else ss.decode_image(ss.resize_u8(rgb, int(H / ncc), int(W / ncc)))
        assert torch.equal(ss.decode_grey(src), torch.from_numpy(GOLD[f"{tag}_grey"]))
        assert f"{tag}_alpha" not in GOLD.files
    assert sc.target_resolution(1601, 1201, 2, 1.0) == ((800, 600), 2.0) and sc.target_resolution(1601, 1201, -1, 2.0) == ((800, 600), 2.0)
    assert sc.target_resolution(1601, 1201, 500, 1.0)[0] == (500, 375) and sc.target_resolution(1603, 1201, 4, 1.0)[0] == (401, 300)


def test_a_camera_built_from_tensors_keeps_them():
    from materialrefgs_amd import scene as sc
    g = torch.Generator().manual_seed(0)
    image, alpha = torch.rand(3, 6, 8, generator=g) * 1.4 - 0.2, torch.rand(1, 6, 8, generator=g)
    cam = sc.Camera(1, np.eye(3), np.array([0.0, 0.0, 3.0]), 0.7, 0.6, image, alpha, "v", 0, data_device="cpu")
    assert torch.equal(cam.original_image, image.clamp(0.0, 1.0)) and cam.gt_alpha_mask.data_ptr() == alpha.data_ptr()
    assert torch.equal(cam.original_image_gray, ss.decode_grey(image.clamp(0.0, 1.0))) and (cam.image_height, cam.image_width) == (6, 8)
    assert not hasattr(cam, "HWK") and cam.nearest_id == [] and cam.refl_mask is None and cam.colmap_id == 1 and cam.znear == 0.01
    a, b = cam.get_image()
    assert torch.equal(a, cam.original_image) and torch.equal(b, cam.original_image_gray)
    grey = torch.rand(1, 3, 4, generator=g)
    assert sc.Camera(1, np.eye(3), np.zeros(3), 0.7, 0.6, image, None, "v", 0, data_device="cpu", gray_image=grey).original_image_gray is grey
    with pytest.raises(ValueError, match="not both"):
        sc.Camera(1, np.eye(3), np.zeros(3), 0.7, 0.6, image, None, "v", 0, store=object(), store_key="k")


def _colmap_json(d):
    return {str(k): [v.id, list(map(float, v.qvec)), list(map(float, v.tvec)), v.camera_id, v.name, v.xys.tolist(), v.point3D_ids.tolist()]
            for k, v in d.items()}


def test_colmap_readers(tree):
    from materialrefgs_amd import scene as sc
    sp, tp = os.path.join(tree, "colmap", "sparse", "0"), os.path.join(tree, "colmap_txt", "sparse", "0")
    intr = sc.read_intrinsics_binary(os.path.join(sp, "cameras.bin"))
    assert {str(k): [v.id, v.model, int(v.width), int(v.height), list(map(float, v.params))] for k, v in intr.items()} == json.loads(str(GOLD["colmap_intr"]))
    assert _colmap_json(sc.read_extrinsics_binary(os.path.join(sp, "images.bin"))) == json.loads(str(GOLD["colmap_extr"]))
    assert _colmap_json(sc.read_extrinsics_text(os.path.join(tp, "images.txt"))) == json.loads(str(GOLD["colmap_txt_extr"]))
    assert list(sc.read_intrinsics_text(os.path.join(tp, "cameras.txt"))) == [1]
    for got in (sc.read_points3D_binary(os.path.join(sp, "points3D.bin")), sc.read_points3D_text(os.path.join(tp, "points3D.txt"))):
        for a, key in zip(got, ("xyz", "rgb", "err")):
            assert a.dtype == np.float64 and np.array_equal(a, GOLD[f"colmap_points_{key}"])


def test_colmap_scene_info(tree, tmp_path, monkeypatch):
    from materialrefgs_amd import scene as sc
    monkeypatch.chdir(tmp_path)
    path = os.path.join(tree, "colmap")
    for tag, ev in (("colmap_eval", True), ("colmap_all", False)):
        info = sc.readColmapSceneInfo(path, None, ev, llffhold=2)
        _check_infos(f"{tag}_train", info.train_cameras)
        if ev:
            _check_infos(f"{tag}_test", info.test_cameras)
            assert len(info.test_cameras) == 3 and len(info.train_cameras) == 2
        else:
            assert info.test_cameras == []
        norm = info.nerf_normalization
        assert np.array_equal(np.concatenate([norm["translate"], [norm["radius"]]]), GOLD[f"{tag}_norm"])
        assert os.path.relpath(info.ply_path, tree) == str(GOLD[f"{tag}_ply_path"]) and info.point_cloud.points.shape == (40, 3)
        for k, c in enumerate(info.train_cameras):
            assert np.array_equal(c.image, GOLD[f"{tag}_train_image_{k}"]) and c.mode == ("RGBA" if c.image.shape[2] == 4 else "RGB")
        assert [sc.camera_to_JSON(k, c) for k, c in enumerate(info.train_cameras)] == json.loads(str(GOLD[f"{tag}_train_json"]))
    assert not os.path.exists(tmp_path / "transforms")                   # the reference's write into the current directory is not copied
    modes = set()
    for resolution in (1, 2):                                            # loadCam on the five views, one of them with an alpha mask
        for k, c in enumerate(info.train_cameras):
            tag = f"colmap_r{resolution}_cam{k}"
            cam = _host_camera(sc, c, resolution, 1.0, k)
            _check_camera(tag, cam)
            small = ss.resize_u8(c.image, cam.image_height, cam.image_width)
            assert torch.equal(ss.decode_image(small[:, :, :3]), torch.from_numpy(GOLD[f"{tag}_image"]))
            assert torch.equal(ss.decode_grey(ss.decode_image(small[:, :, :3])), torch.from_numpy(GOLD[f"{tag}_grey"]))
            assert (c.mode == "RGBA") == (f"{tag}_alpha" in GOLD.files)
            if c.mode == "RGBA":
                assert torch.equal(ss.decode_image(small[:, :, 3]), torch.from_numpy(GOLD[f"{tag}_alpha"]))
            modes.add(c.mode)
    assert modes == {"RGB", "RGBA"}
    _check_infos("colmap_txt_train", sc.readColmapSceneInfo(os.path.join(tree, "colmap_txt"), None, False).train_cameras)
    sc.save_transformer_matrix(info.train_cameras, str(tmp_path / "elsewhere"))
    assert len(json.load(open(tmp_path / "elsewhere" / "transformers.json"))["frames"]) == 5


def test_colmap_point_cloud_conversion(tree, tmp_path):
    """Restated (plyfile is not where the fixture is made): without points3D.ply the binary points are converted once, a points_spc.ply
    is preferred, and a missing .bin falls back to the text file."""
    import shutil
    from materialrefgs_amd import scene as sc
    for source in ("colmap", "colmap_txt"):
        work = tmp_path / source
        shutil.copytree(os.path.join(tree, source), work)
        os.remove(work / "sparse" / "0" / "points3D.ply")
        info = sc.readColmapSceneInfo(str(work), None, False)
        assert info.ply_path == str(work / "sparse/0/points3D.ply") and os.path.exists(info.ply_path)
        pcd = info.point_cloud
        assert np.array_equal(pcd.points, GOLD["colmap_points_xyz"].astype(np.float32)) and pcd.points.dtype == np.float32
        assert np.array_equal(pcd.colors, GOLD["colmap_points_rgb"] / 255.0) and not pcd.normals.any()
    shutil.copy(os.path.join(tree, "blender", "points3d.ply"), work / "sparse" / "0" / "points_spc.ply")
    info = sc.readColmapSceneInfo(str(work), None, False)
    assert info.ply_path.endswith("points_spc.ply") and info.point_cloud.points.shape == (40, 3)


def test_neighbour_lists(tree):
    """The neighbour block of Scene.__init__ on cameras in the reference's shuffled order."""
    from materialrefgs_amd import scene as sc
    infos = _blender_infos(tree, True)
    order = [int(i) for i in GOLD["scene_info_index"]]
    random.seed(0)
    shuffled = list(range(6))
    random.shuffle(shuffled)
    assert shuffled == order                                             # the seeded shuffle of the reference's run
    resolution, _, ncc = CASES[1]
    cams = [_host_camera(sc, infos[i], resolution, ncc, k) for k, i in enumerate(order)]
    assert float((torch.stack([c.camera_center for c in cams]) - torch.from_numpy(GOLD["scene_centers"])).abs().max()) < 2e-4   # _check_float32_routines
    got = sc.nearest_views(cams, ARGS["multi_view_num"], ARGS["multi_view_max_angle"], ARGS["multi_view_min_dis"], ARGS["multi_view_max_dis"])
    assert [[int(i) for i in row] for row in got] == json.loads(str(GOLD["scene_nearest_id"]))
    assert sc.nearest_views(cams, 1, 40, 0.01, 3.0) == [row[:1] for row in got]
    assert all(row == [] for row in sc.nearest_views(cams, 3, 40, 0.01, 0.02))


def test_refl_mask_is_cv2_imread_not_zero(tmp_path):
    from materialrefgs_amd import evaluate, scene as sc
    rng = np.random.default_rng(1)
    rgb = (rng.integers(0, 3, (5, 7, 3)) * 100).astype(np.uint8)
    evaluate.write_png(str(tmp_path / "m.png"), rgb)
    m = sc.read_refl_mask(str(tmp_path / "m.png"))
    assert m.dtype == torch.float32 and torch.equal(m, torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1].transpose(2, 0, 1)) != 0).float())


def test_search_for_max_iteration(tmp_path):
    from materialrefgs_amd import scene as sc
    for n in (7000, 30000, 900):
        (tmp_path / f"iteration_{n}").mkdir()
    assert sc.searchForMaxIteration(str(tmp_path)) == 30000
    assert set(sc.sceneLoadTypeCallbacks) == {"Colmap", "Blender"}


# ---------------------------------------------------------------- CPU: files
def _png(path, rows, W, H, colour, depth=8, interlace=0, extra=b""):
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    raw = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace)) + extra + \
        chunk(b"IDAT", zlib.compress(rows)) + chunk(b"IEND", b"")
    open(path, "wb").write(raw)


def _filter_row(kind, cur, prev, bpp):
    """PNG's forward filters on one row (lists of ints)."""
    out = []
    for i, x in enumerate(cur):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        if kind == 4:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
        else:
            pred = (0, a, b, (a + b) >> 1)[kind]
        out.append((x - pred) & 255)
    return out


@pytest.mark.parametrize("colour,bpp", ((0, 1), (4, 2), (2, 3), (6, 4)))
def test_read_png_filters_and_colour_types(tmp_path, colour, bpp):
    from materialrefgs_amd import io
    rng = np.random.default_rng(colour)
    H, W = 11, 9
    img = rng.integers(0, 256, (H, W, bpp), dtype=np.uint8)
    img[3], img[4, :, :] = 255, 0
    flat = img.reshape(H, W * bpp).tolist()
    rows = b""
    for y in range(H):
        kind = y % 5                                                     # every filter type, with and without a row above
        rows += bytes([kind] + _filter_row(kind, flat[y], flat[y - 1] if y else [0] * (W * bpp), bpp))
    path = str(tmp_path / "f.png")
    _png(path, rows, W, H, colour)
    got = io.read_png(path)
    assert got.dtype == np.uint8 and np.array_equal(got, img if bpp > 1 else img[:, :, 0])
    a, mode = io.read_image(path)
    assert mode == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[bpp] and np.array_equal(a, got)       # Pillow's decode where Pillow imports
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(path)), got)


def test_read_png_round_trip_and_refusals(tmp_path):
    from materialrefgs_amd import evaluate, io
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    evaluate.write_png(path, img)
    assert np.array_equal(io.read_png(path), img)
    rows = bytes(1 + 4 * 3) * 4
    _png(str(tmp_path / "p.png"), bytes(5) * 4, 4, 4, 3, extra=b"")
    with pytest.raises(ValueError, match="palette"):
        io.read_png(str(tmp_path / "p.png"))
    _png(str(tmp_path / "d.png"), bytes(1 + 4 * 6) * 4, 4, 4, 2, depth=16)
    with pytest.raises(ValueError, match="8-bit"):
        io.read_png(str(tmp_path / "d.png"))
    _png(str(tmp_path / "i.png"), rows, 4, 4, 2, interlace=1)
    with pytest.raises(ValueError, match="interlaced"):
        io.read_png(str(tmp_path / "i.png"))
    open(tmp_path / "n.png", "wb").write(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        io.read_png(str(tmp_path / "n.png"))
    raw = bytearray(open(path, "rb").read())
    raw[60] ^= 1
    open(tmp_path / "c.png", "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="damaged"):
        io.read_png(str(tmp_path / "c.png"))


def test_jpeg_without_pillow_says_so(tmp_path, monkeypatch):
    from materialrefgs_amd import io
    monkeypatch.setitem(sys.modules, "PIL", None)                        # `from PIL import Image` raises ImportError
    open(tmp_path / "a.jpg", "wb").write(b"\xff\xd8\xff")
    with pytest.raises(RuntimeError, match="without Pillow"):
        io.read_image(str(tmp_path / "a.jpg"))
    from materialrefgs_amd import evaluate
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    evaluate.write_png(str(tmp_path / "a.png"), img)
    a, mode = io.read_image(str(tmp_path / "a.png"))                     # PNG files are still read
    assert mode == "RGB" and np.array_equal(a, img)


def test_store_and_fetch_ply(tmp_path):
    from materialrefgs_amd import io
    rng = np.random.default_rng(2)
    xyz, rgb = rng.normal(size=(9, 3)), rng.random((9, 3)) * 255
    path = str(tmp_path / "p.ply")
    io.storePly(path, xyz, rgb)
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
              "property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode()
    assert raw.startswith(header) and len(raw) == len(header) + 9 * 27
    pcd = io.fetchPly(path)
    assert pcd.points.dtype == np.float32 and np.array_equal(pcd.points, xyz.astype(np.float32))
    assert pcd.colors.dtype == np.float64 and np.array_equal(pcd.colors, np.floor(rgb) / 255.0) and not pcd.normals.any()
    io.storePly(path, xyz, rgb.astype(np.uint8))
    assert np.array_equal(io.fetchPly(path).colors, np.floor(rgb) / 255.0)
    # a file without colours or normals: the reference's random initialisation, colours first
    bare = str(tmp_path / "bare.ply")
    open(bare, "wb").write(b"ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\nend_header\n" +
                           xyz.astype("<f4").tobytes())
    np.random.seed(4)
    pcd = io.fetchPly(bare)
    np.random.seed(4)
    colors, normals = np.random.rand(9, 3) / 255.0, np.random.rand(9, 3)
    assert np.array_equal(pcd.points, xyz.astype(np.float32)) and np.array_equal(pcd.colors, colors)
    assert np.array_equal(pcd.normals, normals / np.linalg.norm(normals, axis=-1, keepdims=True))
    with pytest.raises(ValueError, match="shape"):
        io.storePly(path, xyz, rgb[:4])


def test_random_cloud_of_a_blender_scene(tree, tmp_path):
    import shutil
    from materialrefgs_amd import scene as sc
    work = tmp_path / "blender"
    shutil.copytree(os.path.join(tree, "blender"), work)
    os.remove(work / "points3d.ply")
    np.random.seed(0)
    info = sc.readNerfSyntheticInfo(str(work), True, eval=True)
    assert len(info.train_cameras) == 4 and len(info.test_cameras) == 2 and os.path.exists(work / "points3d.ply")
    pcd = info.point_cloud
    assert pcd.points.shape == (100000, 3) and float(np.abs(pcd.points).max()) <= 1.3 and np.unique(pcd.colors * 255).tolist() == [127.0]
    np.random.seed(0)
    assert np.array_equal(pcd.points, (np.random.random((100000, 3)) * 2.6 - 1.3).astype(np.float32))
    assert len(sc.readNerfSyntheticInfo(str(work), True, eval=False).train_cameras) == 6


# ---------------------------------------------------------------- CPU: load_normal_prior
class _Recorder:
    """Stands for a ViewStore: records what load_normal_prior hands over."""

    def __init__(self):
        self.priors, self.images = [], []

    def add_prior(self, name, **kw):
        self.priors.append((name, {k: v.shape for k, v in kw.items()}))

    def add(self, name, image, **kw):
        self.images.append((name, image.shape))


def _prior_tree(root, source_name, mask_files):
    from materialrefgs_amd import evaluate
    rgb = np.full((4, 6, 3), 200, dtype=np.uint8)
    src = root / source_name
    for folder, names in ((root / "m3d" / "scanA_train" / "normal", ("r_0", "r_1")), (root / "m3d" / "scanA" / "normal", ("r_0",)),
                          (root / "idarb" / "scanA" / "mtl", ("r_0",)), (root / "idarb" / "scanA" / "rgh", ("r_0",)),
                          (root / "idarb" / "scanA" / "albeldo", ("r_0",)), (root / "score", ("r_0", "r_1", "r_2"))):
        folder.mkdir(parents=True, exist_ok=True)
        for n in names:
            evaluate.write_png(str(folder / f"{n}.png"), rgb)
    for rel in mask_files:
        (src / rel).parent.mkdir(parents=True, exist_ok=True)
        evaluate.write_png(str(src / rel), rgb)
    args = SimpleNamespace(idarb_path=str(root / "idarb"), metric3d_path=str(root / "m3d"), geowizard_path=str(root / "gw"),
                           ref_score_path=str(root / "score"))
    return SimpleNamespace(source_path=str(src)), args


def test_load_normal_prior_names(tmp_path):
    from materialrefgs_amd import scene as sc
    dataset, args = _prior_tree(tmp_path, "refnerf_car", ("train/r_0.png", "train/r_1.png", "train/r_0_normal.png", "train/r_10_alpha.png"))
    rec = _Recorder()
    mask, normal, mtl, rgh, albedo, score = sc.load_normal_prior(dataset, "scanA", 1, "GeoWizard", args, store=rec)
    assert list(mask) == ["r_0", "r_1"]                                  # the r_<n>.png filter of the refnerf folders
    assert list(normal) == ["r_0", "r_1"] and list(score) == ["r_0", "r_1", "r_2"] and list(albedo) == ["r_0"]
    assert mtl == {} and rgh == {}                                       # as in the reference: its resize call raises inside a bare except
    assert ("r_0" in mask) and ("r_7" not in mask) and len(score) == 3
    assert (("prior", "r_0"), {"normal": (4, 6, 3)}) in rec.priors and (("prior", "r_1"), {"mask": (4, 6)}) in rec.priors
    assert (("prior", "r_2"), {"score": (4, 6)}) in rec.priors and rec.images == [(("albedo", "r_0"), (4, 6, 3))]
    with pytest.raises(KeyError):
        mask["r_7"]
    # a "ball" scene keeps the *_alpha files and drops the suffix from the key
    dataset, args = _prior_tree(tmp_path / "b", "refnerf_ball", ("train/r_0.png", "train/r_0_alpha.png", "train/r_3_alpha.png"))
    mask = sc.load_normal_prior(dataset, "scanA", -1, "GeoWizard", args, store=_Recorder())[0]      # r < 0 means 1
    assert list(mask) == ["r_0", "r_3"]
    # DTU scans read images/, the refreal flavour reads the IDArb mask folder and the Metric3D folder without the _train suffix
    dataset, args = _prior_tree(tmp_path / "c", "dtu_scan24", ("images/0001.png", "images/0002.png"))
    mask, normal = sc.load_normal_prior(dataset, "scanA", 1, "GeoWizard", args, store=_Recorder())[:2]
    assert list(mask) == ["0001", "0002"] and list(normal) == ["r_0", "r_1"]
    dataset, args = _prior_tree(tmp_path / "d", "refreal_sedan", ())
    from materialrefgs_amd import evaluate
    (tmp_path / "d" / "idarb" / "scanA" / "mask").mkdir(parents=True)
    evaluate.write_png(str(tmp_path / "d" / "idarb" / "scanA" / "mask" / "frame_1.png"), np.zeros((4, 6, 3), dtype=np.uint8))
    mask, normal = sc.load_normal_prior(dataset, "scanA", 1, "GeoWizard", args, store=_Recorder(), script="refreal")[:2]
    assert list(mask) == ["frame_1"] and list(normal) == ["r_0"]
    for r in (2, 4):
        with pytest.raises(NotImplementedError, match="r = 1"):
            sc.load_normal_prior(dataset, "scanA", r, "GeoWizard", args, store=_Recorder())
    with pytest.raises(ValueError, match="no mask folder"):
        sc.load_normal_prior(SimpleNamespace(source_path=str(tmp_path / "elsewhere")), "scanA", 1, "GeoWizard", args, store=_Recorder())


# ---------------------------------------------------------------- GPU
def _scene(tree, tmp_path, dev, case, gaussians=None, source="blender", **kw):
    from materialrefgs_amd import scene as sc
    resolution, white, ncc = CASES[case]
    args = SimpleNamespace(resolution=resolution, ncc_scale=ncc, white_background=white, source_path=os.path.join(tree, source),
                           model_path=str(tmp_path / "model"), data_device="cuda", envmap_max_res=32, envmap_min_roughness=0.08,
                           envmap_max_roughness=0.5, **dict(ARGS, eval=False))
    made = {}
    if gaussians is None:
        gaussians = SimpleNamespace(create_from_pcd=lambda pcd, extent, a, device=None: made.update(pcd=pcd, extent=extent, device=device))
    random.seed(0)
    return sc.Scene(args, gaussians, device=dev, **kw), made


@pytest.mark.gpu
def test_scene_end_to_end(tree, tmp_path, gpu_device):
    scene, made = _scene(tree, tmp_path, gpu_device, 1)
    cams = scene.getTrainCameras()
    order = [int(i) for i in GOLD["scene_info_index"]]
    assert [c.image_name for c in cams] == list(GOLD["scene_order"]) and [c.uid for c in cams] == list(range(6)) and scene.getTestCameras() == []
    nearest = json.loads(str(GOLD["scene_nearest_id"]))
    for j, cam in enumerate(cams):
        tag = f"case1_cam{order[j]}"
        _check_camera(tag, cam)
        image, grey = cam.original_image, cam.original_image_gray
        assert image.is_cuda and image.dtype == torch.float32 and cam.world_view_transform.is_cuda and image.cuda() is image
        assert torch.equal(image.cpu(), torch.from_numpy(GOLD[f"{tag}_image"])) and torch.equal(grey.cpu(), torch.from_numpy(GOLD[f"{tag}_grey"]))
        assert grey.shape == (1, 20, 24) and image.shape == (3, 10, 12) and cam.gt_alpha_mask is None and cam.ncc_scale == 0.5
        a, b = cam.get_image()
        assert torch.equal(a, image) and torch.equal(b, grey) and torch.equal(cam.original_image, image) and a.data_ptr() != image.data_ptr()
        assert [int(i) for i in cam.nearest_id] == nearest[j] and cam.nearest_names == json.loads(str(GOLD["scene_nearest_names"]))[j]
    assert float(scene.cameras_extent) == float(GOLD["scene_extent"]) and made["extent"] == scene.cameras_extent
    assert made["pcd"].points.shape == (40, 3) and made["device"] == scene.view_store.device          # create_from_pcd ran
    model = tmp_path / "model"
    assert open(model / "multi_view.json").read() == str(GOLD["scene_multi_view_json"])
    assert json.load(open(model / "cameras.json")) == json.loads(str(GOLD["scene_cameras_json"]))
    assert open(model / "input.ply", "rb").read() == GOLD["file:blender/points3d.ply"].tobytes()
    assert scene.view_store.nbytes == 6 * 3 * (10 * 12 + 20 * 24) and scene.world_view_transforms.shape == (6, 4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("case", (0, 2, 3))
def test_load_cam_on_the_device(tree, gpu_device, case):
    from materialrefgs_amd import scene as sc
    from materialrefgs_amd.viewstore import ViewStore
    resolution, white, ncc = CASES[case]
    args = SimpleNamespace(resolution=resolution, ncc_scale=ncc, data_device="cuda")
    store = ViewStore(gpu_device)
    cams = sc.cameraList_from_camInfos(_blender_infos(tree, white), 1.0, args, store=store, tag="t")
    for k, cam in enumerate(cams):
        tag = f"case{case}_cam{k}"
        _check_camera(tag, cam)
        assert torch.equal(cam.original_image.cpu(), torch.from_numpy(GOLD[f"{tag}_image"]))
        assert torch.equal(cam.original_image_gray.cpu(), torch.from_numpy(GOLD[f"{tag}_grey"]))


@pytest.mark.gpu
def test_colmap_views_with_an_alpha_mask(tree, gpu_device, tmp_path, monkeypatch):
    from materialrefgs_amd import scene as sc
    from materialrefgs_amd.viewstore import ViewStore
    monkeypatch.chdir(tmp_path)
    infos = sc.readColmapSceneInfo(os.path.join(tree, "colmap"), None, False).train_cameras
    for resolution in (1, 2):
        cams = sc.cameraList_from_camInfos(infos, 1.0, SimpleNamespace(resolution=resolution, ncc_scale=1.0, data_device="cuda"), store=ViewStore(gpu_device))
        for k, cam in enumerate(cams):
            tag = f"colmap_r{resolution}_cam{k}"
            _check_camera(tag, cam)
            assert torch.equal(cam.original_image.cpu(), torch.from_numpy(GOLD[f"{tag}_image"]))
            assert torch.equal(cam.original_image_gray.cpu(), torch.from_numpy(GOLD[f"{tag}_grey"]))
            if f"{tag}_alpha" in GOLD.files:
                assert torch.equal(cam.gt_alpha_mask.cpu(), torch.from_numpy(GOLD[f"{tag}_alpha"]))
            else:
                assert cam.gt_alpha_mask is None


@pytest.mark.gpu
def test_prior_maps_through_the_store(tmp_path, gpu_device):
    from materialrefgs_amd import evaluate, scene as sc
    from materialrefgs_amd.viewstore import ViewStore
    dataset, args = _prior_tree(tmp_path, "refnerf_car", ("train/r_0.png",))
    rng = np.random.default_rng(9)
    maps = {k: rng.integers(0, 256, (7, 13, 3), dtype=np.uint8) for k in ("normal", "mask", "score", "albedo")}
    evaluate.write_png(str(tmp_path / "m3d" / "scanA_train" / "normal" / "r_0.png"), maps["normal"])
    evaluate.write_png(str(tmp_path / "refnerf_car" / "train" / "r_0.png"), maps["mask"])
    evaluate.write_png(str(tmp_path / "score" / "r_0.png"), maps["score"])
    evaluate.write_png(str(tmp_path / "idarb" / "scanA" / "albeldo" / "r_0.png"), maps["albedo"])
    mask, normal, mtl, rgh, albedo, score = sc.load_normal_prior(dataset, "scanA", 1, "GeoWizard", args, store=ViewStore(gpu_device))
    assert torch.equal(normal["r_0"].cpu(), ss.decode_normal(maps["normal"])) and normal["r_0"].is_cuda
    assert torch.equal(mask["r_0"].cpu(), ss.decode_mask(maps["mask"][:, :, 2])) and mask["r_0"].shape == (7 * 13, 1)
    assert torch.equal(score["r_0"].cpu(), ss.decode_score(maps["score"][:, :, 2])) and score["r_0"].dtype == torch.bool
    assert torch.equal(albedo["r_0"].cpu(), ss.decode_image(maps["albedo"]))
    from materialrefgs_amd import priors
    moved = priors.to_device(mask, gpu_device)
    assert torch.equal(moved["r_0"], mask["r_0"])


@pytest.mark.gpu
def test_a_scene_camera_serves_render_and_loss(tree, tmp_path, gpu_device):
    """The Camera surface is complete for the callers this library ships: one render_initial + calculate_loss step on a Scene camera."""
    from materialrefgs_amd import losses
    from materialrefgs_amd.model import GaussianModel
    from materialrefgs_amd.renderer import render_initial
    torch.manual_seed(0)
    gm = GaussianModel(3)
    scene, _ = _scene(tree, tmp_path, gpu_device, 0, gaussians=gm)
    assert gm._xyz.shape == (40, 3) and gm._xyz.is_cuda                  # create_from_pcd ran on the scene's cloud
    cam = scene.getTrainCameras()[1]
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    pkg = render_initial(cam, gm, pipe, torch.zeros(3, device=gpu_device), srgb=False, opt=SimpleNamespace(indirect=False))
    assert pkg["render"].shape == (3, cam.image_height, cam.image_width) == cam.original_image.shape
    opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.05, normal_loss_start=0, lambda_dist=100.0, dist_loss_start=100,
                          lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                          use_perceptual_loss=False)
    loss, tb = losses.calculate_loss(cam, gm, pkg, opt, 1, None, None)
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss) > 0 and bool(torch.isfinite(gm._xyz.grad).all()) and float(gm._features_dc.grad.abs().sum()) > 0
