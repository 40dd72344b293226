"""Generates tests/golden/reference_scene.npz by IMPORTING the reference's scene/ and utils/ modules in the build container and running
its own readCamerasFromTransforms, getNerfppNorm, loadCam / process_image / PILtoTorch, Camera (all matrices, get_k, get_inv_k, get_rays),
camera_to_JSON, the colmap_loader readers, readColmapSceneInfo and Scene.__init__ (cameras.json, the seeded shuffle, the neighbour block
and multi_view.json) on a small generated dataset.  Only the dataset's files and the recorded results are committed.

What the generator changes around the reference, none of it arithmetic:
  * modules this image lacks and the path never calls (cv2, plyfile, simple_knn, the rasterizers, ...) are registered as placeholders;
    scene.gaussian_model is a placeholder that carries BasicPointCloud, so that scene/__init__.py imports;
  * there is no GPU here: `.cuda()` returns the tensor itself and `device='cuda'` is dropped, so the reference's matrix product and
    inverse run on the CPU;
  * both datasets carry their point cloud as a PLY file, so the reference never reaches storePly (plyfile); its fetchPly fails on the
    placeholder inside the reference's own try / except and the cloud comes back None.
  * this image's Pillow (12) refuses the int8 array readCamerasFromTransforms hands to `Image.fromarray(..., "RGB")`; the Pillow the
    reference was written for took that array's bytes as they are, so here fromarray is given the same bytes viewed as uint8;
Not driven through the reference: the image_msk branch of loadCam (cv2.imread) and the bin -> ply conversion (plyfile); the tests restate
those.  read_points3D_binary / _text themselves are run here.

The Blender set: 6 views (4 train, 2 test) of 24 x 20 RGBA PNG files on an orbit.  The COLMAP set: sparse/0 written with struct, 5 images
of 24 x 20 for cameras declared 48 x 40 (real_im_scale 0.5), one PINHOLE and one SIMPLE_PINHOLE camera; a text twin with PINHOLE cameras only
(the reference's text reader asserts that).

    python tests/golden/gen_reference_scene_vectors.py      # needs /root/reference and Pillow (both absent on the GPU box)
"""
import io as _pyio
import json
import math
import os
import random
import struct
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from materialrefgs_amd.io import storePly  # noqa: E402  (writes the datasets' point clouds; not under test here)

REF = "/root/reference"
sys.path.insert(0, REF)
for name in ("cv2", "plyfile", "simple_knn", "simple_knn._C", "kornia", "kornia.filters", "lpips", "open3d", "trimesh", "nvdiffrast", "nvdiffrast.torch",
             "diff_surfel_rasterization", "diff_surfel_tracing", "cubemapencoder", "imageio", "imageio.v2", "scene.gaussian_model"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None


class BasicPointCloud(tuple):
    pass


sys.modules["scene.gaussian_model"].BasicPointCloud = BasicPointCloud
sys.modules["scene.gaussian_model"].GaussianModel = object
torch.Tensor.cuda = lambda self, *a, **k: self
_tensor = torch.tensor
torch.tensor = lambda *a, **k: _tensor(*a, **{n: v for n, v in k.items() if not (n == "device" and str(v).startswith("cuda"))})

_fromarray = Image.fromarray
Image.fromarray = lambda obj, mode=None: _fromarray(obj.view(np.uint8) if getattr(obj, "dtype", None) == np.int8 else obj, mode)

from scene import Scene, colmap_loader, dataset_readers  # noqa: E402
from utils import camera_utils  # noqa: E402

W, H = 24, 20
CASES = ((1, True, 1.0), (2, True, 0.5), (-1, False, 1.0), (10, False, 0.5), (2, False, 1.0), (1, True, 0.5))     # resolution, white, ncc_scale
ARGS = dict(data_device="cpu", images=None, eval=True, relight=False, multi_view_num=3, multi_view_max_angle=40, multi_view_min_dis=0.01,
            multi_view_max_dis=3.0)
out, files = {}, {}


def png_bytes(a, mode):
    buf = _pyio.BytesIO()
    Image.fromarray(a, mode).save(buf, format="PNG")
    return buf.getvalue()


def photograph(rng, k):
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([(xx * 9 + yy * 5 + 40 * k) % 256, (xx * 3 + yy * 11 + 17 * k) % 256, (xx * yy + 29 * k) % 256], axis=-1).astype(np.int64)
    rgb = np.clip(rgb + rng.integers(-20, 21, rgb.shape), 0, 255)
    alpha = np.clip(255 - 14 * np.hypot(xx - W / 2 + k, yy - H / 2) + rng.integers(-30, 31, (H, W)), 0, 255)
    alpha[:3, :5], alpha[-3:, -5:] = 0, 255
    return np.concatenate([rgb, alpha[..., None]], axis=-1).astype(np.uint8)


def orbit_c2w(az_deg, el_deg, radius):
    """A Blender camera-to-world matrix (x right, y up, z back) looking at the origin."""
    az, el = math.radians(az_deg), math.radians(el_deg)
    eye = radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    back = eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, 0.0, 1.0]), back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, eye
    return m


def write_tree(root):
    for rel, data in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)


def build_datasets():
    rng = np.random.default_rng(61)
    poses = [(0, 20, 4.0), (12, 22, 4.0), (25, 18, 4.2), (70, 30, 4.0), (8, 25, 9.0), (31, 15, 4.1)]       # far in angle: 3, far away: 4
    for split, ids in (("train", (0, 1, 2, 3)), ("test", (4, 5))):
        frames = []
        for n, k in enumerate(ids):
            files[f"blender/{split}/r_{n}.png"] = png_bytes(photograph(rng, k), "RGBA")
            frames.append({"file_path": f"./{split}/r_{n}", "transform_matrix": orbit_c2w(*poses[k]).tolist()})
        files[f"blender/transforms_{split}.json"] = json.dumps({"camera_angle_x": 0.6911112070083618, "frames": frames}, indent=1).encode()
    cloud = rng.normal(size=(40, 3)) * 0.4
    tmp = tempfile.mkdtemp()
    storePly(os.path.join(tmp, "p.ply"), cloud, rng.integers(0, 256, (40, 3)).astype(np.float64))
    ply = open(os.path.join(tmp, "p.ply"), "rb").read()
    files["blender/points3d.ply"] = ply
    # COLMAP: cameras 1 (PINHOLE) and 2 (SIMPLE_PINHOLE) declared at 48 x 40, five images
    cams = {1: (1, (60.0, 58.0, 24.5, 19.0)), 2: (0, (55.0, 23.0, 20.5))}
    blob = struct.pack("<Q", len(cams))
    for cid, (model, params) in cams.items():
        blob += struct.pack("<iiQQ", cid, model, 48, 40) + struct.pack("<" + "d" * len(params), *params)
    files["colmap/sparse/0/cameras.bin"] = blob
    blob, text = struct.pack("<Q", 5), ""
    for n in range(5):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        t = rng.normal(size=3) * 2
        name = f"img_{4 - n}.png"                                          # file order is not name order: the reader sorts by name
        pts = [(float(rng.random() * 48), float(rng.random() * 40), int(rng.integers(-1, 40))) for _ in range(n + 1)]
        blob += struct.pack("<idddddddi", 10 + n, *q, *t, 1 + n % 2) + name.encode() + b"\x00" + struct.pack("<Q", len(pts))
        for p in pts:
            blob += struct.pack("<ddq", *p)
        text += f"{10 + n} {' '.join(repr(float(v)) for v in q)} {' '.join(repr(float(v)) for v in t)} 1 {name}\n"
        text += " ".join(f"{p[0]!r} {p[1]!r} {p[2]}" for p in pts) + "\n"
        im = photograph(rng, n)
        files[f"colmap/images/{name}"] = png_bytes(im if n == 2 else im[:, :, :3], "RGBA" if n == 2 else "RGB")   # one view with an alpha mask
        files[f"colmap_txt/images/{name}"] = files[f"colmap/images/{name}"]
    files["colmap/sparse/0/images.bin"] = blob
    files["colmap_txt/sparse/0/images.txt"] = ("# Image list with two lines of data per image\n" + text).encode()
    files["colmap_txt/sparse/0/cameras.txt"] = b"# Camera list\n1 PINHOLE 48 40 60.0 58.0 24.5 19.0\n"
    blob, text = struct.pack("<Q", 7), "# 3D point list\n"
    for n in range(7):
        xyz, rgb, err = rng.normal(size=3), rng.integers(0, 256, 3), float(rng.random())
        track = [(int(rng.integers(0, 5)), int(rng.integers(0, 9))) for _ in range(n % 3 + 1)]
        blob += struct.pack("<QdddBBBd", n + 1, *xyz, *[int(v) for v in rgb], err) + struct.pack("<Q", len(track))
        for tr in track:
            blob += struct.pack("<ii", *tr)
        text += f"{n + 1} {' '.join(repr(float(v)) for v in xyz)} {' '.join(str(int(v)) for v in rgb)} {err!r} " + \
            " ".join(f"{a} {b}" for a, b in track) + "\n"
    files["colmap/sparse/0/points3D.bin"] = blob
    files["colmap_txt/sparse/0/points3D.txt"] = text.encode()
    files["colmap/sparse/0/points3D.ply"] = ply
    files["colmap_txt/sparse/0/points3D.ply"] = ply


def record_info(tag, infos):
    out[f"{tag}_names"] = np.array([c.image_name for c in infos])
    out[f"{tag}_uid"] = np.array([c.uid for c in infos])
    for f in ("R", "T", "K"):
        out[f"{tag}_{f}"] = np.stack([np.asarray(getattr(c, f), dtype=np.float64) for c in infos])
    out[f"{tag}_fov"] = np.array([[c.FovX, c.FovY] for c in infos], dtype=np.float64)
    out[f"{tag}_wh"] = np.array([[c.width, c.height] for c in infos])
    for k, c in enumerate(infos):
        out[f"{tag}_image_{k}"] = np.array(c.image)
    out[f"{tag}_json"] = np.array(json.dumps([camera_utils.camera_to_JSON(k, c) for k, c in enumerate(infos)]))


def record_camera(tag, cam):
    out[f"{tag}_image"] = cam.original_image.numpy()
    out[f"{tag}_grey"] = cam.original_image_gray.numpy()
    if cam.gt_alpha_mask is not None:
        out[f"{tag}_alpha"] = cam.gt_alpha_mask.numpy()
    for f in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center", "R", "T"):
        out[f"{tag}_{f}"] = getattr(cam, f).numpy()
    out[f"{tag}_k"], out[f"{tag}_inv_k"] = cam.get_k().numpy(), cam.get_inv_k().numpy()
    out[f"{tag}_k2"], out[f"{tag}_inv_k2"] = cam.get_k(2.0).numpy(), cam.get_inv_k(2.0).numpy()
    out[f"{tag}_rays"] = cam.get_rays().numpy()
    out[f"{tag}_hwk_K"] = np.asarray(cam.HWK[2], dtype=np.float64)
    out[f"{tag}_scalars"] = np.array([cam.image_height, cam.image_width, cam.HWK[0], cam.HWK[1], cam.Fx, cam.Fy, cam.Cx, cam.Cy], dtype=np.float64)


def main():
    build_datasets()
    root = tempfile.mkdtemp()
    write_tree(root)
    os.chdir(root)                                                          # the reference writes ./transforms/transformers.json on a COLMAP load
    for rel, data in files.items():
        out["file:" + rel] = np.frombuffer(data, dtype=np.uint8)
    blender = os.path.join(root, "blender")
    for white in (True, False):
        wtag = "white" if white else "black"
        infos = dataset_readers.readCamerasFromTransforms(blender, "transforms_train.json", white) + \
            dataset_readers.readCamerasFromTransforms(blender, "transforms_test.json", white)
        record_info(f"blender_{wtag}", infos)
        norm = dataset_readers.getNerfppNorm(infos)
        out[f"blender_{wtag}_norm"] = np.concatenate([norm["translate"], [norm["radius"]]])
        for case, (resolution, w, ncc) in enumerate(CASES):
            if w != white:
                continue
            args = SimpleNamespace(resolution=resolution, ncc_scale=ncc, **ARGS)
            for k, c in enumerate(infos):
                record_camera(f"case{case}_cam{k}", camera_utils.loadCam(args, k, c, 1.0))
    out["cases"] = np.array(CASES, dtype=np.float64)
    # COLMAP: the readers, then the scene info with the hold-out split
    sp = os.path.join(root, "colmap", "sparse", "0")
    intr, extr = colmap_loader.read_intrinsics_binary(os.path.join(sp, "cameras.bin")), colmap_loader.read_extrinsics_binary(os.path.join(sp, "images.bin"))
    out["colmap_intr"] = np.array(json.dumps({str(k): [v.id, v.model, int(v.width), int(v.height), list(map(float, v.params))] for k, v in intr.items()}))
    out["colmap_extr"] = np.array(json.dumps({str(k): [v.id, list(map(float, v.qvec)), list(map(float, v.tvec)), v.camera_id, v.name,
                                                       v.xys.tolist(), v.point3D_ids.tolist()] for k, v in extr.items()}))
    xyz, rgb, err = colmap_loader.read_points3D_binary(os.path.join(sp, "points3D.bin"))
    out["colmap_points_xyz"], out["colmap_points_rgb"], out["colmap_points_err"] = xyz, rgb, err
    tp = os.path.join(root, "colmap_txt", "sparse", "0")
    xyz_t, rgb_t, err_t = colmap_loader.read_points3D_text(os.path.join(tp, "points3D.txt"))
    assert np.array_equal(xyz, xyz_t) and np.array_equal(rgb, rgb_t) and np.array_equal(err, err_t)
    extr_t = colmap_loader.read_extrinsics_text(os.path.join(tp, "images.txt"))
    out["colmap_txt_extr"] = np.array(json.dumps({str(k): [v.id, list(map(float, v.qvec)), list(map(float, v.tvec)), v.camera_id, v.name,
                                                           v.xys.tolist(), v.point3D_ids.tolist()] for k, v in extr_t.items()}))
    for tag, ev in (("colmap_eval", True), ("colmap_all", False)):
        info = dataset_readers.readColmapSceneInfo(os.path.join(root, "colmap"), None, ev, llffhold=2)
        assert info.point_cloud is None                                     # plyfile is a placeholder here
        record_info(f"{tag}_train", info.train_cameras)
        if info.test_cameras:
            record_info(f"{tag}_test", info.test_cameras)
        out[f"{tag}_norm"] = np.concatenate([info.nerf_normalization["translate"], [info.nerf_normalization["radius"]]])
        out[f"{tag}_ply_path"] = np.array(os.path.relpath(info.ply_path, root))
        if not ev:
            for resolution in (1, 2):
                args = SimpleNamespace(resolution=resolution, ncc_scale=1.0, **ARGS)
                for k, c in enumerate(info.train_cameras):
                    record_camera(f"colmap_r{resolution}_cam{k}", camera_utils.loadCam(args, k, c, 1.0))
    info = dataset_readers.readColmapSceneInfo(os.path.join(root, "colmap_txt"), None, False)
    record_info("colmap_txt_train", info.train_cameras)
    # Scene.__init__ on the Blender set: cameras.json, the seeded shuffle, the neighbour lists and multi_view.json
    model_path = os.path.join(root, "model")
    os.makedirs(model_path)
    made = {}
    gaussians = SimpleNamespace(create_from_pcd=lambda pcd, extent, a: made.update(extent=extent, pcd=pcd))
    resolution, white, ncc = CASES[1]                                       # the scene's cameras are those of case 1, in the shuffled order
    args = SimpleNamespace(resolution=resolution, ncc_scale=ncc, white_background=white, source_path=blender, model_path=model_path,
                           **dict(ARGS, eval=False))
    random.seed(0)
    scene = Scene(args, gaussians, shuffle=True)
    cams = scene.getTrainCameras()
    out["scene_order"] = np.array([c.image_name for c in cams])
    out["scene_uid"] = np.array([c.uid for c in cams])
    R_all = out["blender_white_R"].astype(np.float32).reshape(-1, 9)         # on an orbit around the origin T is (0, 0, radius) for every view
    out["scene_info_index"] = np.array([int(np.flatnonzero((R_all == c.R.numpy().reshape(9)).all(axis=1))[0]) for c in cams])
    assert sorted(out["scene_info_index"]) == list(range(6))
    for j, c in enumerate(cams):
        assert np.array_equal(c.original_image.numpy(), out[f"case1_cam{out['scene_info_index'][j]}_image"])
    out["scene_centers"] = np.stack([c.camera_center.numpy() for c in cams])
    out["scene_nearest_id"] = np.array(json.dumps([[int(i) for i in c.nearest_id] for c in cams]))
    out["scene_nearest_names"] = np.array(json.dumps([list(c.nearest_names) for c in cams]))
    out["scene_extent"] = np.array(scene.cameras_extent, dtype=np.float64)
    assert made["extent"] == scene.cameras_extent and len(scene.getTestCameras()) == 0
    out["scene_multi_view_json"] = np.array(open(os.path.join(model_path, "multi_view.json")).read())
    out["scene_cameras_json"] = np.array(open(os.path.join(model_path, "cameras.json")).read())
    assert open(os.path.join(model_path, "input.ply"), "rb").read() == files["blender/points3d.ply"]
    lens = [len(c.nearest_id) for c in cams]
    print("neighbours per view:", lens, out["scene_nearest_id"])
    assert min(lens) == 0 and max(lens) == 3 and 1 in lens, lens           # the thresholds and the cap both bite
    dst = os.path.join(HERE, "reference_scene.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, len(out), "arrays", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
