"""Opening a dataset, behind the reference's names: the readers of scene/dataset_readers.py and scene/colmap_loader.py, `loadCam` and
its companions of utils/camera_utils.py, `Camera` (scene/cameras.py:17-115), `Scene` (scene/__init__.py) and `load_normal_prior`
(train_refnerf.py:70-200).  Everything here is host code except where a photograph lives: a `Camera` made by `loadCam` keeps no fp32
image; its `original_image`, `original_image_gray`, `gt_alpha_mask` and `get_image()` are decoded from the 8-bit planes of a
`viewstore.ViewStore` on the device, bit-equal to what the reference holds on the host and uploads every iteration.

Differences from the reference (INTEGRATION.md, section "Scene"):
  * `CameraInfo.image` is a host uint8 array (with `CameraInfo.mode`), not a PIL image.  Files are decoded by Pillow when it imports,
    otherwise PNG files by `io.read_png`; JPEG without Pillow raises.
  * `readColmapCameras` does not call `save_transformer_matrix` (:165), which writes `transforms/transformers.json` into the CURRENT
    directory of whoever opens a scene; the function exists and takes the folder to write into.
  * the matrices of a `Camera` are computed on the host and then moved to `data_device`.  world_view_transform and projection_matrix
    are the reference's bits (float64 arithmetic, one cast); full_proj_transform and camera_center, which the reference forms in float32
    on the GPU, are the float64 product / inverse of those float32 matrices rounded once, so they do not depend on a device's or a CPU's
    float32 routines.  With data_device="cpu" nothing touches a GPU (the photographs then need tensors, not a store).
  * `load_normal_prior` serves r = 1 only: the prior maps go through `cv2.resize`, whose 8-bit bilinear is not pinned here.
    `mtl_images` and `rgh_images` come back empty, as they do in the reference: its `cv2.resize(mtl, (w+0.5*r)//r, (h+0.5*r)//r)`
    passes a float where the size tuple belongs and raises inside a bare `except: pass` on the first file.
"""
import glob
import json
import os
import random
import re
import struct
import sys
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import io as _io
from .camera import focal2fov, fov2focal, get_projection_matrix, get_projection_matrix_correct, get_world2view2
from .gs_utils import SH2RGB
from .io import BasicPointCloud, fetchPly, storePly  # noqa: F401  (the reference's dataset_readers exports them)
from .viewstore import ViewStore


class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray
    T: np.ndarray
    K: np.ndarray
    FovY: float
    FovX: float
    image: np.ndarray          # uint8 [H,W,C] (the reference: a PIL image)
    image_path: str
    image_name: str
    width: int
    height: int
    mode: str = "RGB"


class SceneInfo(NamedTuple):
    point_cloud: BasicPointCloud
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str


def getNerfppNorm(cam_info):
    def get_center_and_diag(cam_centers):
        cam_centers = np.hstack(cam_centers)
        avg_cam_center = np.mean(cam_centers, axis=1, keepdims=True)
        center = avg_cam_center
        dist = np.linalg.norm(cam_centers - center, axis=0, keepdims=True)
        diagonal = np.max(dist)
        return center.flatten(), diagonal

    cam_centers = []
    for cam in cam_info:
        W2C = get_world2view2(cam.R, cam.T)
        C2W = np.linalg.inv(W2C)
        cam_centers.append(C2W[:3, 3:4])
    center, diagonal = get_center_and_diag(cam_centers)
    radius = diagonal * 1.1
    translate = -center
    return {"translate": translate, "radius": radius}


def save_transformer_matrix(cam_infos, folder):
    """dataset_readers.py:70-95 into `folder` (the reference writes into ./transforms of the current directory on every COLMAP load;
    readColmapCameras here does not call it)."""
    os.makedirs(folder, exist_ok=True)
    frames = []
    for cam_info in cam_infos:
        w2c = np.zeros((4, 4))
        w2c[3, 3] = 1.
        w2c[:3, 3] = cam_info.T
        w2c[:3, :3] = np.transpose(cam_info.R)
        c2w = np.linalg.inv(w2c)
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": cam_info.image_name, "transform_matrix": c2w.tolist()})
    with open(os.path.join(folder, "transformers.json"), "w") as f:
        f.write(json.dumps({"frames": frames}, indent=1))


# ---- COLMAP files (scene/colmap_loader.py) ------------------------------------------------------------------------------------------------
class ColmapCamera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray


class ColmapImage(NamedTuple):
    id: int
    qvec: np.ndarray
    tvec: np.ndarray
    camera_id: int
    name: str
    xys: np.ndarray
    point3D_ids: np.ndarray


# model id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


def qvec2rotmat(qvec):
    return np.array([
        [1 - 2 * qvec[2]**2 - 2 * qvec[3]**2, 2 * qvec[1] * qvec[2] - 2 * qvec[0] * qvec[3], 2 * qvec[3] * qvec[1] + 2 * qvec[0] * qvec[2]],
        [2 * qvec[1] * qvec[2] + 2 * qvec[0] * qvec[3], 1 - 2 * qvec[1]**2 - 2 * qvec[3]**2, 2 * qvec[2] * qvec[3] - 2 * qvec[0] * qvec[1]],
        [2 * qvec[3] * qvec[1] - 2 * qvec[0] * qvec[2], 2 * qvec[2] * qvec[3] + 2 * qvec[0] * qvec[1], 1 - 2 * qvec[1]**2 - 2 * qvec[2]**2]])


def _unpack(fid, fmt):
    fmt = "<" + fmt
    data = fid.read(struct.calcsize(fmt))
    return struct.unpack(fmt, data)


def _data_lines(path):
    with open(path, "r") as fid:
        for line in fid:
            line = line.strip()
            if len(line) > 0 and line[0] != "#":
                yield line


def read_points3D_text(path):
    rows = [line.split() for line in _data_lines(path)]
    xyzs, rgbs, errors = np.empty((len(rows), 3)), np.empty((len(rows), 3)), np.empty((len(rows), 1))
    for k, elems in enumerate(rows):
        xyzs[k] = tuple(map(float, elems[1:4]))
        rgbs[k] = tuple(map(int, elems[4:7]))
        errors[k] = float(elems[7])
    return xyzs, rgbs, errors


def read_points3D_binary(path_to_model_file):
    with open(path_to_model_file, "rb") as fid:
        num_points = _unpack(fid, "Q")[0]
        xyzs, rgbs, errors = np.empty((num_points, 3)), np.empty((num_points, 3)), np.empty((num_points, 1))
        for p_id in range(num_points):
            props = _unpack(fid, "QdddBBBd")
            xyzs[p_id], rgbs[p_id], errors[p_id] = props[1:4], props[4:7], props[7]
            track_length = _unpack(fid, "Q")[0]
            fid.read(8 * track_length)
    return xyzs, rgbs, errors


def read_intrinsics_text(path):
    cameras = {}
    for line in _data_lines(path):
        elems = line.split()
        camera_id, model = int(elems[0]), elems[1]
        assert model == "PINHOLE", "While the loader support other types, the rest of the code assumes PINHOLE"
        cameras[camera_id] = ColmapCamera(id=camera_id, model=model, width=int(elems[2]), height=int(elems[3]),
                                          params=np.array(tuple(map(float, elems[4:]))))
    return cameras


def read_intrinsics_binary(path_to_model_file):
    cameras = {}
    with open(path_to_model_file, "rb") as fid:
        num_cameras = _unpack(fid, "Q")[0]
        for _ in range(num_cameras):
            camera_id, model_id, width, height = _unpack(fid, "iiQQ")
            model_name, num_params = CAMERA_MODELS[model_id]
            params = _unpack(fid, "d" * num_params)
            cameras[camera_id] = ColmapCamera(id=camera_id, model=model_name, width=width, height=height, params=np.array(params))
        assert len(cameras) == num_cameras
    return cameras


def read_extrinsics_binary(path_to_model_file):
    images = {}
    with open(path_to_model_file, "rb") as fid:
        num_reg_images = _unpack(fid, "Q")[0]
        for _ in range(num_reg_images):
            props = _unpack(fid, "idddddddi")
            image_id, qvec, tvec, camera_id = props[0], np.array(props[1:5]), np.array(props[5:8]), props[8]
            name = b""
            ch = fid.read(1)
            while ch != b"\x00":
                if not ch:
                    raise ValueError(f"{path_to_model_file}: unterminated image name")
                name += ch
                ch = fid.read(1)
            num_points2D = _unpack(fid, "Q")[0]
            x_y_id_s = _unpack(fid, "ddq" * num_points2D)
            xys = np.column_stack([tuple(map(float, x_y_id_s[0::3])), tuple(map(float, x_y_id_s[1::3]))])
            point3D_ids = np.array(tuple(map(int, x_y_id_s[2::3])))
            images[image_id] = ColmapImage(id=image_id, qvec=qvec, tvec=tvec, camera_id=camera_id, name=name.decode("utf-8"), xys=xys,
                                           point3D_ids=point3D_ids)
    return images


def read_extrinsics_text(path):
    images = {}
    with open(path, "r") as fid:
        while True:
            line = fid.readline()
            if not line:
                break
            line = line.strip()
            if len(line) > 0 and line[0] != "#":
                elems = line.split()
                image_id = int(elems[0])
                qvec, tvec = np.array(tuple(map(float, elems[1:5]))), np.array(tuple(map(float, elems[5:8])))
                camera_id, image_name = int(elems[8]), elems[9]
                elems = fid.readline().split()
                xys = np.column_stack([tuple(map(float, elems[0::3])), tuple(map(float, elems[1::3]))])
                point3D_ids = np.array(tuple(map(int, elems[2::3])))
                images[image_id] = ColmapImage(id=image_id, qvec=qvec, tvec=tvec, camera_id=camera_id, name=image_name, xys=xys,
                                               point3D_ids=point3D_ids)
    return images


# ---- readers (scene/dataset_readers.py) -----------------------------------------------------------------------------------------------------
def readColmapCameras(cam_extrinsics, cam_intrinsics, images_folder):
    cam_infos = []
    for idx, key in enumerate(cam_extrinsics):
        sys.stdout.write('\r')
        sys.stdout.write("Reading camera {}/{}".format(idx + 1, len(cam_extrinsics)))
        sys.stdout.flush()
        extr = cam_extrinsics[key]
        intr = cam_intrinsics[extr.camera_id]
        height, width = intr.height, intr.width
        uid = intr.id
        R = np.transpose(qvec2rotmat(extr.qvec))
        T = np.array(extr.tvec)
        if intr.model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL"):
            focal_length_x = intr.params[0]
            FovY = focal2fov(focal_length_x, height)
            FovX = focal2fov(focal_length_x, width)
            K = np.array([[focal_length_x, 0, intr.params[1]], [0, focal_length_x, intr.params[2]], [0, 0, 1]])
        elif intr.model == "PINHOLE":
            focal_length_x, focal_length_y = intr.params[0], intr.params[1]
            FovY = focal2fov(focal_length_y, height)
            FovX = focal2fov(focal_length_x, width)
            K = np.array([[focal_length_x, 0, intr.params[2]], [0, focal_length_y, intr.params[3]], [0, 0, 1]])
        else:
            assert False, "Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!"
        image_path = os.path.join(images_folder, os.path.basename(extr.name))
        image_name = os.path.basename(image_path).split(".")[0]
        image, mode = _io.read_image(image_path.replace('.JPG', '.jpg') if not ("mip360" in image_path) else image_path)
        real_im_scale = image.shape[1] / width
        K[:2] *= real_im_scale
        cam_infos.append(CameraInfo(uid=uid, R=R, T=T, K=K, FovY=FovY, FovX=FovX, image=image, image_path=image_path, image_name=image_name,
                                    width=width, height=height, mode=mode))
    sys.stdout.write('\n')
    return cam_infos


def readColmapSceneInfo(path, images, eval, llffhold=8):
    try:
        cam_extrinsics = read_extrinsics_binary(os.path.join(path, "sparse/0", "images.bin"))
        cam_intrinsics = read_intrinsics_binary(os.path.join(path, "sparse/0", "cameras.bin"))
    except Exception:
        cam_extrinsics = read_extrinsics_text(os.path.join(path, "sparse/0", "images.txt"))
        cam_intrinsics = read_intrinsics_text(os.path.join(path, "sparse/0", "cameras.txt"))
    reading_dir = "images" if images is None else images
    cam_infos_unsorted = readColmapCameras(cam_extrinsics=cam_extrinsics, cam_intrinsics=cam_intrinsics,
                                           images_folder=os.path.join(path, reading_dir))
    cam_infos = sorted(cam_infos_unsorted.copy(), key=lambda x: x.image_name)
    if eval:
        train_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold != 0]
        test_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold == 0]
    else:
        train_cam_infos = cam_infos
        test_cam_infos = []
    nerf_normalization = getNerfppNorm(train_cam_infos)
    ply_path = os.path.join(path, "sparse/0/points3D.ply")
    spc_ply_path = os.path.join(path, "sparse/0/points_spc.ply")
    if os.path.exists(spc_ply_path):
        ply_path = spc_ply_path
    bin_path = os.path.join(path, "sparse/0/points3D.bin")
    txt_path = os.path.join(path, "sparse/0/points3D.txt")
    if not os.path.exists(ply_path):
        print("Converting point3d.bin to .ply, will happen only the first time you open the scene.")
        try:
            xyz, rgb, _ = read_points3D_binary(bin_path)
        except Exception:
            xyz, rgb, _ = read_points3D_text(txt_path)
        storePly(ply_path, xyz, rgb)
    try:
        pcd = fetchPly(ply_path)
    except Exception:
        pcd = None
    return SceneInfo(point_cloud=pcd, train_cameras=train_cam_infos, test_cameras=test_cam_infos, nerf_normalization=nerf_normalization,
                     ply_path=ply_path)


def readCamerasFromTransforms(path, transformsfile, white_background, extension=".png"):
    """:249-300.  The photograph stays RGBA in `CameraInfo.image` with mode "RGBA->white" / "RGBA->black": the compositing onto the
    background runs on the device when the view enters a store (viewstore.composite_u8), where it gives the bytes of the reference's
    float64 expression; `composited` evaluates the same table on the host."""
    cam_infos = []
    with open(os.path.join(path, transformsfile)) as json_file:
        contents = json.load(json_file)
        fovx = contents["camera_angle_x"]
        frames = contents["frames"]
        for idx, frame in enumerate(frames):
            cam_name = os.path.join(path, frame["file_path"] + extension)
            c2w = np.array(frame["transform_matrix"])
            c2w[:3, 1:3] *= -1                                  # OpenGL / Blender axes (Y up, Z back) -> COLMAP (Y down, Z forward)
            w2c = np.linalg.inv(c2w)
            R = np.transpose(w2c[:3, :3])                       # stored transposed, as the rasterizer reads it
            T = w2c[:3, 3]
            image_path = os.path.join(path, cam_name)
            image_name = Path(cam_name).stem
            image, mode = _io.read_image(image_path)
            im_data = _to_rgba(image, mode)
            W, H = im_data.shape[1], im_data.shape[0]
            fo = fov2focal(fovx, W)
            K = np.array([[fo, 0, W / 2], [0, fo, H / 2], [0, 0, 1]])
            fovy = focal2fov(fov2focal(fovx, W), H)
            cam_infos.append(CameraInfo(uid=idx, R=R, T=T, K=K, FovY=fovy, FovX=fovx, image=im_data, image_path=image_path,
                                        image_name=image_name, width=W, height=H, mode="RGBA->white" if white_background else "RGBA->black"))
    return cam_infos


def _to_rgba(image, mode):
    """`image.convert("RGBA")` for the four modes read_image returns."""
    a = image if image.ndim == 3 else image[:, :, None]
    opaque = np.full(a.shape[:2] + (1,), 255, dtype=np.uint8)
    if mode == "RGBA":
        return np.ascontiguousarray(a)
    if mode == "RGB":
        return np.concatenate([a, opaque], axis=2)
    if mode == "L":
        return np.concatenate([a, a, a, opaque], axis=2)
    if mode == "LA":
        return np.concatenate([a[:, :, :1]] * 3 + [a[:, :, 1:]], axis=2)
    raise ValueError(f"materialrefgs_amd.scene: unknown image mode {mode!r}")


def composited(cam_info):
    """The RGB bytes the reference's CameraInfo.image holds for a Blender view (host; the store does the same on the device)."""
    from .viewstore import composite_table
    if not cam_info.mode.startswith("RGBA->"):
        return cam_info.image
    table = composite_table(cam_info.mode == "RGBA->white")
    return table[cam_info.image[:, :, :3], cam_info.image[:, :, 3:4]]


def readNerfSyntheticInfo(path, white_background, eval, extension=".png"):
    print("Reading Training Transforms")
    train_cam_infos = readCamerasFromTransforms(path, "transforms_train.json", white_background, extension)
    print("Reading Test Transforms")
    test_cam_infos = readCamerasFromTransforms(path, "transforms_test.json", white_background, extension)
    if not eval:
        train_cam_infos.extend(test_cam_infos)
        test_cam_infos = []
    nerf_normalization = getNerfppNorm(train_cam_infos)
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        num_pts = 100_000                                       # no COLMAP data: random points inside the bounds of the Blender scenes
        print(f"Generating random point cloud ({num_pts})...")
        xyz = np.random.random((num_pts, 3)) * 2.6 - 1.3
        shs = np.random.random((num_pts, 3)) / 255.0
        storePly(ply_path, xyz, SH2RGB(shs) * 255)
    try:
        pcd = fetchPly(ply_path)
    except Exception:
        pcd = None
    return SceneInfo(point_cloud=pcd, train_cameras=train_cam_infos, test_cameras=test_cam_infos, nerf_normalization=nerf_normalization,
                     ply_path=ply_path)


sceneLoadTypeCallbacks = {"Colmap": readColmapSceneInfo, "Blender": readNerfSyntheticInfo}


def searchForMaxIteration(folder):
    return max(int(fname.split("_")[-1]) for fname in os.listdir(folder))


# ---- Camera (scene/cameras.py:17-115) -------------------------------------------------------------------------------------------------------
class Camera:
    """The reference's Camera.  Built by `loadCam` it reads its photograph from a ViewStore (`store`, `store_key`): `original_image`
    [3,H,W], `original_image_gray` [1,Hg,Wg] and `gt_alpha_mask` [1,H,W] (None without an alpha channel) are decoded on access into
    fresh device tensors, `get_image()` decodes image and grey in one launch.  Built from tensors (`image`, `gt_alpha_mask`,
    `gray_image`) it keeps them as given, as the reference does."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid, trans=np.array([0.0, 0.0, 0.0]), scale=1.0,
                 data_device="cuda", HWK=None, gt_refl_mask=None, gray_image=None, ncc_scale=1.0, store=None, store_key=None):
        self.uid = uid
        self.nearest_id = []
        self.nearest_names = []
        self.colmap_id = colmap_id
        self.R = R
        self.T = T
        self.FoVx = FoVx
        self.FoVy = FoVy
        self.image_name = image_name
        self.refl_mask = gt_refl_mask
        self.ncc_scale = ncc_scale
        try:
            self.data_device = torch.device(data_device)
        except Exception as e:
            print(e)
            print(f"[Warning] Custom device {data_device} failed, fallback to default cuda device")
            self.data_device = torch.device("cuda")
        self._store, self._store_key = store, store_key
        self._image = self._alpha = self._grey = None
        if HWK is not None:
            self.image_width = int(HWK[1])
            self.image_height = int(HWK[0])
        if store is not None:
            if image is not None or gt_alpha_mask is not None or gray_image is not None:
                raise ValueError("materialrefgs_amd.scene: a Camera takes its photograph from a store or from tensors, not both")
            _, self.image_height, self.image_width = store.shape(store_key)
        elif image is not None:
            self._image = image.clamp(0.0, 1.0)
            self.image_width = self._image.shape[2]
            self.image_height = self._image.shape[1]
            if gt_alpha_mask is not None:
                self._alpha = gt_alpha_mask.to(self.data_device)
            self._grey = gray_image if gray_image is not None else \
                (0.299 * self._image[0] + 0.587 * self._image[1] + 0.114 * self._image[2])[None]
        self.Fx = fov2focal(FoVx, self.image_width)
        self.Fy = fov2focal(FoVy, self.image_height)
        self.Cx = 0.5 * self.image_width
        self.Cy = 0.5 * self.image_height
        self.zfar = 100.0
        self.znear = 0.01
        self.trans = trans
        self.scale = scale
        dev = self.data_device
        # host arithmetic, then one copy: the values do not depend on the device's matrix product
        wvt = torch.tensor(get_world2view2(R, T, trans, scale)).transpose(0, 1)
        if HWK is None:
            proj = get_projection_matrix(znear=self.znear, zfar=self.zfar, fovX=self.FoVx, fovY=self.FoVy).transpose(0, 1)
        else:
            self.HWK = HWK
            proj = get_projection_matrix_correct(self.znear, self.zfar, HWK[0], HWK[1], HWK[2]).transpose(0, 1)
        # The reference forms these two in float32 on the GPU (bmm, inverse), so their last bits depend on the device's routines; here the
        # float32 matrices above are multiplied and inverted in float64 and the result is rounded once.
        full = (wvt.double() @ proj.double()).float()
        center = torch.from_numpy(np.linalg.inv(wvt.double().numpy())[3, :3].copy()).float()
        self.world_view_transform = wvt.to(dev)
        self.projection_matrix = proj.to(dev)
        self.full_proj_transform = full.to(dev)
        self.camera_center = center.to(dev)
        self.R = torch.tensor(self.R, dtype=torch.float32, device=dev)
        self.T = torch.tensor(self.T, dtype=torch.float32, device=dev)

    def _fetch(self, *want):
        got = self._store.fetch(self._store_key, want)
        return [got.get(k) for k in want]

    @property
    def original_image(self):
        return self._fetch("gt")[0] if self._store is not None else self._image

    @property
    def original_image_gray(self):
        return self._fetch("grey")[0] if self._store is not None else self._grey

    @property
    def gt_alpha_mask(self):
        if self._store is not None:
            return self._fetch("alpha")[0] if self._store.has(self._store_key, "alpha") else None
        return self._alpha

    def get_image(self):
        if self._store is not None:
            return tuple(self._fetch("gt", "grey"))
        return self._image.to(self.data_device), self._grey.to(self.data_device)

    def get_calib_matrix_nerf(self, scale=1.0):
        intrinsic_matrix = torch.tensor([[self.Fx / scale, 0, self.Cx / scale], [0, self.Fy / scale, self.Cy / scale], [0, 0, 1]]).float()
        extrinsic_matrix = self.world_view_transform.transpose(0, 1).contiguous()
        return intrinsic_matrix, extrinsic_matrix

    def get_rays(self, scale=1.0):
        W, H = int(self.image_width / scale), int(self.image_height / scale)
        ix, iy = torch.meshgrid(torch.arange(W), torch.arange(H), indexing='xy')
        rays_d = torch.stack([(ix - self.Cx / scale) / self.Fx * scale, (iy - self.Cy / scale) / self.Fy * scale, torch.ones_like(ix)], -1).float()
        return rays_d.to(self.data_device)

    def get_k(self, scale=1.0):
        return torch.tensor([[self.Fx / scale, 0, self.Cx / scale], [0, self.Fy / scale, self.Cy / scale], [0, 0, 1]]).to(self.data_device)

    def get_inv_k(self, scale=1.0):
        return torch.tensor([[scale / self.Fx, 0, -self.Cx / self.Fx], [0, scale / self.Fy, -self.Cy / self.Fy], [0, 0, 1]]).to(self.data_device)


# ---- utils/camera_utils.py ------------------------------------------------------------------------------------------------------------------
def target_resolution(orig_w, orig_h, resolution, resolution_scale):
    """utils/camera_utils.py:43-61, literally: ((width, height), scale)."""
    if resolution in [1, 2, 4, 8]:
        res = round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
        scale = float(resolution_scale * resolution)
    else:
        if resolution == -1:
            global_down = 1
        else:
            global_down = orig_w / resolution
        scale = float(global_down) * float(resolution_scale)
        res = (int(orig_w / scale), int(orig_h / scale))
    return res, scale


_DEFAULT_STORES = {}


def default_store(device="cuda"):
    """The store `loadCam` uses when it is given none: one per device for the life of the process."""
    dev = torch.device(device)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
    if dev not in _DEFAULT_STORES:
        _DEFAULT_STORES[dev] = ViewStore(dev)
    return _DEFAULT_STORES[dev]


def read_refl_mask(path):
    """`cv2.imread(path) != 0` (:86) as a float tensor [3,H,W]: three channels in cv2's B, G, R order, an alpha channel dropped, a grey
    file repeated."""
    a, mode = _io.read_image(path)
    rgb = _to_rgba(a, mode)[:, :, :3]
    return torch.tensor(np.ascontiguousarray(rgb[:, :, ::-1]) != 0).permute(2, 0, 1).float()


def loadCam(args, id, cam_info, resolution_scale, store=None, store_key=None):
    """utils/camera_utils.py:40-94.  The photograph goes into `store` (default_store(args.data_device) when None) under `store_key`
    (default (image_name, resolution_scale, id)): upload, compositing for a Blender view, Pillow's resize to the resolution of :43-61
    and, with args.ncc_scale != 1, the second resize of process_image for the grey image."""
    orig_h, orig_w = cam_info.image.shape[:2]
    resolution, scale = target_resolution(orig_w, orig_h, args.resolution, resolution_scale)
    HWK = None
    if cam_info.K is not None:
        K = cam_info.K.copy()
        K[:2] = K[:2] / scale
        HWK = (resolution[1], resolution[0], K)
    if store is None:
        store = default_store(args.data_device)
    if store_key is None:
        store_key = (cam_info.image_name, resolution_scale, id)
    grey_size = None
    if args.ncc_scale != 1.0:
        grey_size = (int(resolution[1] / args.ncc_scale), int(resolution[0] / args.ncc_scale))
    white = {"RGBA->white": True, "RGBA->black": False}.get(cam_info.mode)
    image = cam_info.image if cam_info.image.ndim == 3 else cam_info.image[:, :, None]
    if image.shape[2] not in (3, 4):
        raise ValueError(f"{cam_info.image_path}: a photograph needs three colour channels (process_image reads channels 0, 1, 2), got mode "
                         f"{cam_info.mode}")
    store.add(store_key, image, size=(resolution[1], resolution[0]), grey_size=grey_size, white_background=white)
    refl_path = os.path.join(os.path.dirname(os.path.dirname(cam_info.image_path)), 'image_msk')
    refl_path = os.path.join(refl_path, os.path.basename(cam_info.image_path))
    if not os.path.exists(refl_path):
        refl_path = refl_path.replace('.JPG', '.jpg')
    refl_msk = read_refl_mask(refl_path) if os.path.exists(refl_path) else None
    return Camera(colmap_id=cam_info.uid, R=cam_info.R, T=cam_info.T, FoVx=cam_info.FovX, FoVy=cam_info.FovY, image=None, gt_alpha_mask=None,
                  image_name=cam_info.image_name, uid=id, data_device=store.device, HWK=HWK, gt_refl_mask=refl_msk, gray_image=None,
                  ncc_scale=args.ncc_scale, store=store, store_key=store_key)


def cameraList_from_camInfos(cam_infos, resolution_scale, args, store=None, tag=""):
    return [loadCam(args, id, c, resolution_scale, store=store, store_key=(tag, resolution_scale, id)) for id, c in enumerate(cam_infos)]


def camera_to_JSON(id, camera):
    """:104-124 (takes a CameraInfo)."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = camera.R.transpose()
    Rt[:3, 3] = camera.T
    Rt[3, 3] = 1.0
    W2C = np.linalg.inv(Rt)
    pos = W2C[:3, 3]
    rot = W2C[:3, :3]
    return {'id': id, 'img_name': camera.image_name, 'width': camera.width, 'height': camera.height, 'position': pos.tolist(),
            'rotation': [x.tolist() for x in rot], 'fy': fov2focal(camera.FovY, camera.height), 'fx': fov2focal(camera.FovX, camera.width)}


def gen_virtul_cam(cam, trans_noise=1.0, deg_noise=15.0):
    """:126-155 (numpy's global generator: translation first, then the three angles)."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = cam.R.cpu().numpy().transpose()
    Rt[:3, 3] = cam.T.cpu().numpy()
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    translation_perturbation = np.random.uniform(-trans_noise, trans_noise, 3)
    rotation_perturbation = np.random.uniform(-deg_noise, deg_noise, 3)
    rx, ry, rz = np.deg2rad(rotation_perturbation)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    R_perturbation = Rz @ Ry @ Rx
    C2W[:3, :3] = C2W[:3, :3] @ R_perturbation
    C2W[:3, 3] = C2W[:3, 3] + translation_perturbation
    Rt = np.linalg.inv(C2W)
    return Camera(100000, Rt[:3, :3].transpose(), Rt[:3, 3], cam.FoVx, cam.FoVy, cam.original_image, None, cam.image_name, 100000,
                  HWK=cam.HWK, data_device=cam.data_device)


# ---- Scene (scene/__init__.py) ----------------------------------------------------------------------------------------------------------------
def nearest_views(cameras, multi_view_num, multi_view_max_angle, multi_view_min_dis, multi_view_max_dis):
    """The neighbour block of Scene.__init__ (:82-118) on the host: for every camera the indices of its neighbours, nearest first --
    sorted by distance of the camera centres, then by the angle between the optical axes, and filtered by the three thresholds."""
    camera_centers = torch.stack([c.camera_center.detach().cpu() for c in cameras], dim=0)
    center_rays = []
    for cur_cam in cameras:
        R = cur_cam.R.float().cpu()
        center_ray = torch.tensor([0.0, 0.0, 1.0]).float()
        center_rays.append(center_ray @ R.transpose(-1, -2))
    center_rays = torch.nn.functional.normalize(torch.stack(center_rays, dim=0), dim=-1)
    diss = torch.norm(camera_centers[:, None] - camera_centers[None], dim=-1).numpy()
    tmp = torch.sum(center_rays[:, None] * center_rays[None], dim=-1)
    angles = (torch.arccos(tmp) * 180 / 3.14159).numpy()
    out = []
    for id in range(len(cameras)):
        sorted_indices = np.lexsort((angles[id], diss[id]))
        mask = (angles[id][sorted_indices] < multi_view_max_angle) & (diss[id][sorted_indices] > multi_view_min_dis) & \
            (diss[id][sorted_indices] < multi_view_max_dis)
        sorted_indices = sorted_indices[mask]
        out.append(list(sorted_indices[:min(multi_view_num, len(sorted_indices))]))
    return out


class Scene:
    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0], env_gaussians=None, store=None,
                 device="cuda"):
        """scene/__init__.py:27-139.  `store`: the ViewStore the photographs go into (a new one on `device` when None), kept as
        `self.view_store`."""
        self.model_path = args.model_path
        self.loaded_iter = None
        self.gaussians = gaussians
        self.env_gaussians = env_gaussians
        if load_iteration:
            self.loaded_iter = searchForMaxIteration(os.path.join(self.model_path, "point_cloud")) if load_iteration == -1 else load_iteration
            print("Loading trained model at iteration {}".format(self.loaded_iter))
        self.train_cameras = {}
        self.test_cameras = {}
        if os.path.exists(os.path.join(args.source_path, "sparse")):
            scene_info = sceneLoadTypeCallbacks["Colmap"](args.source_path, args.images, args.eval)
        elif os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
            print("Found transforms_train.json file, assuming Blender data set!")
            scene_info = sceneLoadTypeCallbacks["Blender"](args.source_path, args.white_background, args.eval)
        else:
            assert False, "Could not recognize scene type!"
        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            with open(scene_info.ply_path, 'rb') as src_file, open(os.path.join(self.model_path, "input.ply"), 'wb') as dest_file:
                dest_file.write(src_file.read())
            camlist = []
            if scene_info.test_cameras:
                camlist.extend(scene_info.test_cameras)
            if scene_info.train_cameras:
                camlist.extend(scene_info.train_cameras)
            json_cams = [camera_to_JSON(id, cam) for id, cam in enumerate(camlist)]
            with open(os.path.join(self.model_path, "cameras.json"), 'w') as file:
                json.dump(json_cams, file)
        if shuffle:
            random.shuffle(scene_info.train_cameras)            # multi-res consistent random shuffling
            random.shuffle(scene_info.test_cameras)
        self.cameras_extent = scene_info.nerf_normalization["radius"]
        self.view_store = store if store is not None else ViewStore(device)
        self.multi_view_num = args.multi_view_num
        for resolution_scale in resolution_scales:
            print("Loading Training Cameras")
            self.train_cameras[resolution_scale] = cameraList_from_camInfos(scene_info.train_cameras, resolution_scale, args, self.view_store, "train")
            print("Loading Test Cameras")
            self.test_cameras[resolution_scale] = cameraList_from_camInfos(scene_info.test_cameras, resolution_scale, args, self.view_store, "test")
            print("computing nearest_id")
            cams = self.train_cameras[resolution_scale]
            self.world_view_transforms = torch.stack([c.world_view_transform for c in cams]) if cams else torch.zeros(0, 4, 4)
            nearest = nearest_views(cams, self.multi_view_num, args.multi_view_max_angle, args.multi_view_min_dis, args.multi_view_max_dis) \
                if cams else []
            with open(os.path.join(self.model_path, "multi_view.json"), 'w') as file:
                for cur_cam, ids in zip(cams, nearest):
                    json_d = {'ref_name': cur_cam.image_name, 'nearest_name': []}
                    for index in ids:
                        cur_cam.nearest_id.append(index)
                        cur_cam.nearest_names.append(cams[index].image_name)
                        json_d["nearest_name"].append(cams[index].image_name)
                    file.write(json.dumps(json_d, separators=(',', ':')))
                    file.write('\n')
        if self.loaded_iter:
            folder = os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter))
            if args.relight:
                self.gaussians.load_ply(os.path.join(folder, "point_cloud.ply"), relight=True, args=args)
            else:
                self.gaussians.load_ply(os.path.join(folder, "point_cloud.ply"), args=args)
            env_path = os.path.join(folder, "env_point_cloud.ply")
            if os.path.exists(env_path) and self.env_gaussians is not None:
                from . import env_model
                env_model.load_ply(self.env_gaussians, env_path, device=self.view_store.device)
        else:
            self.gaussians.create_from_pcd(scene_info.point_cloud, self.cameras_extent, args, device=self.view_store.device)

    def save(self, iteration):
        point_cloud_path = os.path.join(self.model_path, "point_cloud/iteration_{}".format(iteration))
        self.gaussians.save_ply(os.path.join(point_cloud_path, "point_cloud.ply"))
        if self.env_gaussians is not None and self.env_gaussians.get_xyz.shape[0] > 0:
            from . import env_model
            env_model.save_ply(self.env_gaussians, os.path.join(point_cloud_path, "env_point_cloud.ply"))

    def get_env_gaussians(self):
        return self.env_gaussians

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]


# ---- the prior maps (train_refnerf.py:54-200) ---------------------------------------------------------------------------------------------------
class StoreView:
    """A read-only mapping image name -> tensor whose values are decoded from a ViewStore on every access (one launch, fresh device
    tensors), standing for one of the dictionaries load_normal_prior returns.  `.cuda()` on a value is a no-op; `priors.to_device` finds
    nothing to move."""

    def __init__(self, store, what, names):
        self._store, self._what, self._names = store, what, dict.fromkeys(names)

    def __getitem__(self, name):
        if name not in self._names:
            raise KeyError(name)
        return self._store.fetch(("prior", name), (self._what,))[self._what]

    def __contains__(self, name):
        return name in self._names

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)

    def keys(self):
        return self._names.keys()

    def values(self):
        return (self[k] for k in self._names)

    def items(self):
        return ((k, self[k]) for k in self._names)

    def get(self, name, default=None):
        return self[name] if name in self._names else default


def load_by_method(method="GeoWizard", scan_id=None, args=None, script="refnerf"):
    """:54-67; the Metric3D folder is `{scan_id}_train` in train_refnerf.py and `{scan_id}` in train_refreal.py / train_glossy.py."""
    if method == "GeoWizard":
        return f"{args.geowizard_path}/dtu_prior/{scan_id}/normal_colored", "*_pred_colored.png", "_pred_colored.png"
    if method == "Metric3D":
        return f"{args.metric3d_path}/{scan_id}{'_train' if script == 'refnerf' else ''}/normal", "*.png", ".png"
    if method == "IDArb":
        return f"{args.idarb_path}/{scan_id}/normal/", "*.png", ".png"
    raise ValueError(f"materialrefgs_amd.scene: unknown prior method {method!r}")


def _last_channel(a):
    return np.ascontiguousarray(a if a.ndim == 2 else a[..., -1])


def load_normal_prior(dataset, scan_id: str, r=1, method="GeoWizard", args=None, store=None, script="refnerf"):
    """train_refnerf.py:70-200 (train_glossy.py's is the same plus its `rgb` mask folder; train_refreal.py's differs in the Metric3D
    folder, `script="refreal"`, and keeps alpha / 255 as the mask where this thresholds at 128 as the other two do).  Returns
    (mask_images, normal_images, mtl_images, rgh_images, albedo_images, ref_score_images): the maps' bytes go into `store` (default:
    default_store()) and each dictionary decodes a value on access -- normal [H W,3] float32((n / 255.) * 2. - 1), mask [H W,1] in {0, 1},
    ref score bool [1,H,W], albedo [3,H,W] = u8 / 255.  mtl_images and rgh_images are EMPTY, as in the reference (module docstring).
    As there, `method` is not consulted: the normals are read from the Metric3D folder.  r != 1 raises NotImplementedError."""
    if r < 0:
        r = 1
    if r != 1:
        raise NotImplementedError("materialrefgs_amd.scene: load_normal_prior serves r = 1 only (the maps at another r go through "
                                  "cv2.resize, whose 8-bit bilinear filter is not reproduced here)")
    store = store if store is not None else default_store()
    prior_rt = args.idarb_path
    prior_rt2, glob_regx, posix = load_by_method(method="Metric3D", scan_id=scan_id, args=args, script=script)

    def glob_data(pattern):
        return sorted(glob.glob(pattern))

    print("Loading Normal Maps...")
    normal_names = []
    for npath in glob_data(os.path.join(prior_rt2, glob_regx)):
        a, mode = _io.read_image(npath)
        img_name = os.path.basename(npath).replace(posix, "")
        if a.ndim != 3 or a.shape[2] < 3:
            raise ValueError(f"{npath}: a normal map needs three channels, got mode {mode}")
        store.add_prior(("prior", img_name), normal=a[..., :3])
        normal_names.append(img_name)
    print("Loading Mask Maps...")
    src = dataset.source_path
    mask_dir = os.path.join(src, "images") if "scan" in src else os.path.join(src, "train") if "refnerf" in src else \
        os.path.join(src, "rgb") if "GlossySynthetic_blender" in src else f"{args.idarb_path}/{scan_id}/mask" if "refreal" in src else None
    print(mask_dir)
    if mask_dir is None:
        raise ValueError(f"materialrefgs_amd.scene: no mask folder is known for {src!r} (the reference's get_mask_dir returns None there and fails)")
    mask_paths = glob_data(os.path.join(mask_dir, "*.png"))
    if "refnerf" in mask_dir and mask_paths:
        pattern = re.compile(r'^r_\d+\.png$')
        mask_paths = [f for f in mask_paths if "alpha" in f] if "ball" in mask_paths[0] else \
            [f for f in mask_paths if pattern.match(os.path.basename(f))]
    mask_names = []
    for mpath in mask_paths:
        a, _ = _io.read_image(mpath)
        img_name = os.path.basename(mpath).replace(".png", "").replace(".jpg", "").replace("_alpha", "")
        store.add_prior(("prior", img_name), mask=_last_channel(a))
        mask_names.append(img_name)
    print("Loading Albeldo Maps...")
    albedo_names = []
    for npath in glob_data(os.path.join(prior_rt, scan_id, "albeldo", "*.png")):
        a, mode = _io.read_image(npath)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"{npath}: albedo maps are read as RGB files, got mode {mode}")
        img_name = os.path.basename(npath)[:-4]
        store.add(("albedo", img_name), a)
        albedo_names.append(img_name)
    print("Loading Ref Score Maps...")
    score_names = []
    for npath in glob_data(f"{args.ref_score_path}/" + "*.png"):
        a, _ = _io.read_image(npath)
        img_name = os.path.basename(npath)[:-4]
        store.add_prior(("prior", img_name), score=_last_channel(a))
        score_names.append(img_name)
    print("Finised Loading Prior Maps!!!")

    class _Albedo(StoreView):
        def __getitem__(self, name):
            if name not in self._names:
                raise KeyError(name)
            return self._store.fetch(("albedo", name), ("gt",))["gt"]
    return (StoreView(store, "mask", mask_names), StoreView(store, "normal", normal_names), {}, {}, _Albedo(store, "gt", albedo_names),
            StoreView(store, "score", score_names))
