"""On-disk formats of a trained model: the point-cloud PLY of GaussianModel.save_ply / load_ply
(scene/gaussian_model.py:462-529, 725-838) and the environment-map `.map` files next to it (`EnvLight.state_dict()` through
torch.save, :520-527).  Plain host I/O in numpy -- the reference goes through the `plyfile` package, which writes exactly this
layout: ASCII header, one `vertex` element, every property `float` (f4), little-endian rows in the attribute order of
`construct_list_of_attributes` (:462-487)."""
import os
from typing import Dict, NamedTuple

import numpy as np
import torch

# tensor name -> (PLY prefix, transposed on disk?)  in the order save_ply concatenates them (:515)
_FIELDS = [("xyz", None), ("normal1", None), ("normal2", None), ("features_dc", "f_dc"), ("features_rest", "f_rest"), ("indirect_dc", "ind_dc"),
           ("indirect_rest", "ind_rest"), ("indirect_asg", "ind_asg"), ("opacity", "opacity"), ("refl_strength", "refl_strength"),
           ("metalness", "metalness"), ("roughness", "roughness"), ("ori_color", "ori_color"), ("diffuse_color", "diffuse_color"),
           ("scaling", "scale"), ("rotation", "rot")]
_SCALAR = {"opacity", "refl_strength", "metalness", "roughness"}
_CHANNEL_MAJOR = {"features_dc", "features_rest", "indirect_dc", "indirect_rest", "indirect_asg"}   # stored as [P, C, K] -> transpose(1, 2).flatten


def attribute_names(shapes: Dict[str, tuple]):
    """construct_list_of_attributes (:462-487) for tensors of the given shapes."""
    names = ["x", "y", "z", "nx", "ny", "nz", "nx2", "ny2", "nz2"]
    for key, prefix in _FIELDS[3:]:
        n = int(np.prod(shapes[key][1:]))
        if key in _SCALAR:
            names.append(prefix)
        else:
            names += [f"{prefix}_{i}" for i in range(n)]
    return names


def _flat(key, t):
    a = t.detach().cpu().float()
    if key in _CHANNEL_MAJOR:
        a = a.transpose(1, 2)
    return a.reshape(a.shape[0], -1).contiguous().numpy()


def _write_vertex_ply(path: str, names, data):
    """One `vertex` element of float properties `names`, rows `data` [P, len(names)], binary little-endian: what plyfile writes."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    data = np.ascontiguousarray(data, dtype="<f4")
    assert data.ndim == 2 and data.shape[1] == len(names)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {data.shape[0]}"] + [f"property float {n}" for n in names] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(data.tobytes())


def save_ply(path: str, tensors: Dict[str, torch.Tensor], env_map=None, env_map_2=None):
    """tensors: GaussianModel layout -- xyz [P,3], normal1/2 [P,3], features_dc [P,1,3], features_rest [P,15,3], indirect_dc [P,1,3],
    indirect_rest [P,15,3], indirect_asg [P,32,5], opacity/refl_strength/metalness/roughness [P,1], ori_color/diffuse_color [P,3],
    scaling [P,2], rotation [P,4] (raw, pre-activation values as the reference stores them)."""
    cols = [_flat(k, tensors[k]) for k, _ in _FIELDS]
    names = attribute_names({k: tuple(tensors[k].shape) for k, _ in _FIELDS})
    _write_vertex_ply(path, names, np.concatenate(cols, axis=1))
    if env_map is not None:
        torch.save(env_map.state_dict(), path.replace(".ply", "1.map"))
    if env_map_2 is not None:
        torch.save(env_map_2.state_dict(), path.replace(".ply", "2.map"))


def read_ply_vertices(path: str):
    """(property names, float32 array [P, n_properties]) of the vertex element of a binary little-endian or ASCII PLY whose vertex
    properties are all 4-byte floats (what save_ply writes)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, count, names, in_vertex = None, None, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
                elif count is None:
                    raise ValueError("the vertex element must come first")
            elif tok[0] == "property" and in_vertex:
                if tok[1] not in ("float", "float32"):
                    raise ValueError(f"unsupported vertex property type {tok[1]}")
                names.append(tok[2])
            elif tok[0] == "end_header":
                break
        if fmt == "binary_little_endian":
            data = np.frombuffer(f.read(count * len(names) * 4), dtype="<f4").reshape(count, len(names))
        elif fmt == "ascii":
            data = np.loadtxt(f, dtype=np.float32, max_rows=count).reshape(count, len(names))
        else:
            raise ValueError(f"unsupported PLY format {fmt}")
    return names, np.array(data, dtype=np.float32)


def save_mesh_ply(path: str, mesh_or_vertices, triangles=None):
    """Triangle mesh as a binary little-endian PLY: `vertex` with float x, y, z and `face` with `list uchar int vertex_indices` -- the layout
    of o3d.io.write_triangle_mesh for a mesh without colours or normals (train_refnerf.py:1468), read back by load_mesh_ply and by the
    reference's load_mesh_from_ply.  Takes a mesh (`.vertices`, `.triangles`) or the two arrays.  A mesh that carries an "rgb" attribute
    group (mesh.TriangleMesh) is written with `uchar red green blue` after x, y, z, round(clip(c, 0, 1) * 255), as
    o3d.io.write_triangle_mesh writes a coloured mesh; without the group the bytes are those of the two arrays."""
    v, t = (mesh_or_vertices.vertices, mesh_or_vertices.triangles) if triangles is None else (mesh_or_vertices, triangles)
    v = np.ascontiguousarray(np.asarray(v), dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(np.asarray(t), dtype="<i4").reshape(-1, 3)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    coloured = triangles is None and "rgb" in (getattr(mesh_or_vertices, "layout", None) or {})
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", "property float x", "property float y", "property float z"]
    rows = v
    if coloured:
        header += ["property uchar red", "property uchar green", "property uchar blue"]
        rows = np.empty(v.shape[0], dtype=[("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
        rows["xyz"] = v
        rows["rgb"] = np.round(np.clip(np.asarray(mesh_or_vertices.vertex_colors, dtype=np.float64).reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
    header += [f"element face {t.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    faces["n"], faces["idx"] = 3, t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())
        f.write(faces.tobytes())


MATERIAL_PLY_PROPERTIES = ("x", "y", "z", "red", "green", "blue", "normal_x", "normal_y", "normal_z", "diffuse_r", "diffuse_g", "diffuse_b",
                           "albedo_r", "albedo_g", "albedo_b", "metallic_0", "roughness_0")
# (attribute group of the mesh, its channels in the file), in file order after x, y, z
_MATERIAL_GROUPS = (("rgb", 3), ("normal", 3), ("diffuse", 3), ("base_color", 3), ("metallic", 1), ("roughness", 1))


def save_material_ply(path: str, mesh):
    """The material mesh of extract_mesh_bouned_with_material (utils/mesh_utils.py:278-306) as a binary little-endian PLY: `vertex` with
    the double properties MATERIAL_PLY_PROPERTIES in that order, `face` with `list uchar int vertex_indices`.  `mesh` carries the groups
    rgb, normal, diffuse, base_color (albedo_*), metallic and roughness (mesh.TriangleMesh.attribute); of a group wider than the file's
    columns the first ones are taken.  Values are the fp32 attributes widened, normals stored as they are: the reference passes them through
    8-bit colour and `* 2 - 1`, this does not quantise."""
    v = np.asarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(np.asarray(mesh.triangles), dtype="<i4").reshape(-1, 3)
    cols = [v]
    for group, width in _MATERIAL_GROUPS:
        a = mesh.attribute(group)
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.shape[0] != v.shape[0] or a.shape[1] < width:
            raise ValueError(f"attribute group {group!r} must be [V,{width}]")
        cols.append(a[:, :width].astype(np.float64))
    data = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f8")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"] + [f"property double {p}" for p in MATERIAL_PLY_PROPERTIES] + \
             [f"element face {t.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    faces = np.empty(t.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    faces["n"], faces["idx"] = 3, t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(data.tobytes())
        f.write(faces.tobytes())


def load_material_ply(path: str):
    """What save_material_ply wrote: dict(vertices float64 [V,3], triangles int32 [T,3], rgb, normal, diffuse, base_color [V,3], metallic,
    roughness [V,1], all float64)."""
    with open(path, "rb") as f:
        head = b""
        while not head.endswith(b"end_header\n"):
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            head += line
        lines = [ln.split() for ln in head.decode("ascii").splitlines()]
        if lines[0] != ["ply"] or ["format", "binary_little_endian", "1.0"] not in lines:
            raise ValueError("not a binary little-endian PLY file")
        elements = [ln for ln in lines if ln and ln[0] == "element"]
        props = [ln[1:] for ln in lines if ln and ln[0] == "property"]
        if [e[1] for e in elements] != ["vertex", "face"] or props[:-1] != [["double", p] for p in MATERIAL_PLY_PROPERTIES] or \
                props[-1] != ["list", "uchar", "int", "vertex_indices"]:
            raise ValueError("not a material PLY: expected the double vertex properties " + " ".join(MATERIAL_PLY_PROPERTIES))
        nv, nf = int(elements[0][2]), int(elements[1][2])
        ncol = len(MATERIAL_PLY_PROPERTIES)
        data = np.frombuffer(f.read(nv * ncol * 8), dtype="<f8").reshape(nv, ncol).astype(np.float64)
        faces = np.frombuffer(f.read(nf * 13), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        if len(faces) != nf or (faces["n"] != 3).any():
            raise ValueError("only triangle faces are read")
    out = dict(vertices=data[:, :3].copy(), triangles=np.ascontiguousarray(faces["idx"], dtype=np.int32))
    at = 3
    for group, width in _MATERIAL_GROUPS:
        out[group] = data[:, at:at + width].copy()
        at += width
    return out


def load_mesh_ply(path: str):
    """(vertices float32 [V,3], triangles int32 [T,3]) of a binary little-endian PLY whose vertex element starts with float x, y, z and
    whose faces are triangles in a `list uchar int` (or uint) property -- what save_mesh_ply writes."""
    sizes = {"float": 4, "float32": 4, "double": 8, "float64": 8, "uchar": 1, "uint8": 1, "char": 1, "int8": 1, "short": 2, "int16": 2,
             "ushort": 2, "uint16": 2, "int": 4, "int32": 4, "uint": 4, "uint32": 4}
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append(tok[1:])
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"unsupported PLY format {fmt}")
        if [e[0] for e in elements[:2]] != ["vertex", "face"]:
            raise ValueError("expected the elements vertex and face, in that order")
        (_, nv, vprops), (_, nf, fprops) = elements[:2]
        if [p[-1] for p in vprops[:3]] != ["x", "y", "z"] or any(p[0] not in ("float", "float32") for p in vprops[:3]) or \
                any(p[0] == "list" for p in vprops):
            raise ValueError("the vertex element must start with float x, y, z and hold no lists")
        row = sum(sizes[p[0]] for p in vprops)
        raw = np.frombuffer(f.read(nv * row), dtype=np.uint8).reshape(nv, row)
        vertices = np.ascontiguousarray(raw[:, :12]).view("<f4").reshape(nv, 3).astype(np.float32)
        if len(fprops) != 1 or fprops[0][0] != "list" or sizes.get(fprops[0][1]) != 1 or fprops[0][2] not in ("int", "int32", "uint", "uint32"):
            raise ValueError("the face element must be one `list uchar int` property")
        faces = np.frombuffer(f.read(nf * 13), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        if len(faces) != nf or (faces["n"] != 3).any():
            raise ValueError("only triangle faces are read")
    return vertices, np.ascontiguousarray(faces["idx"], dtype=np.int32)


def load_ply(path: str, max_sh_degree: int = 3, device="cpu") -> Dict[str, torch.Tensor]:
    """load_ply (:725-838): returns the tensors in the GaussianModel layout (see save_ply)."""
    names, data = read_ply_vertices(path)
    col = {n: i for i, n in enumerate(names)}

    def group(prefix):
        ks = sorted([n for n in names if n.startswith(prefix + "_")], key=lambda x: int(x.split("_")[-1]))
        return data[:, [col[k] for k in ks]]

    def cols(*ks):
        return data[:, [col[k] for k in ks]]

    P = data.shape[0]
    n_rest = 3 * (max_sh_degree + 1) ** 2 - 3
    f_rest, ind_rest = group("f_rest"), group("ind_rest")
    assert f_rest.shape[1] == n_rest and ind_rest.shape[1] == n_rest                  # :762, :775
    out = {
        "xyz": cols("x", "y", "z"), "normal1": cols("nx", "ny", "nz"), "normal2": cols("nx2", "ny2", "nz2"),
        "features_dc": group("f_dc").reshape(P, 3, 1).transpose(0, 2, 1),
        "features_rest": f_rest.reshape(P, 3, -1).transpose(0, 2, 1),
        "indirect_dc": group("ind_dc").reshape(P, 3, 1).transpose(0, 2, 1),
        "indirect_rest": ind_rest.reshape(P, 3, -1).transpose(0, 2, 1),
        "indirect_asg": group("ind_asg").reshape(P, 5, -1).transpose(0, 2, 1),          # :788
        "opacity": cols("opacity"), "refl_strength": cols("refl_strength"), "metalness": cols("metalness"), "roughness": cols("roughness"),
        "ori_color": group("ori_color"), "diffuse_color": group("diffuse_color"), "scaling": group("scale"), "rotation": group("rot"),
    }
    return {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float32, device=device) for k, v in out.items()}


# ---- the environment set (scene/env_gaussian_model.py:198-277) ------------------------------------------------------------------------
_ENV_FIELDS = [("features_dc", "f_dc"), ("features_rest", "f_rest"), ("opacity", "opacity"), ("scaling", "scale"), ("rotation", "rot")]


def env_attribute_names(shapes: Dict[str, tuple]):
    """construct_list_of_attributes of EnvGaussianModel (:198-210): x y z nx ny nz f_dc_* f_rest_* opacity scale_* rot_*."""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    for key, prefix in _ENV_FIELDS:
        names += [prefix] if key in _SCALAR else [f"{prefix}_{i}" for i in range(int(np.prod(shapes[key][1:])))]
    return names


def save_env_ply(path: str, tensors: Dict[str, torch.Tensor]):
    """EnvGaussianModel.save_ply (:212-229).  tensors: xyz [P,3], features_dc [P,1,3], features_rest [P,K,3] (both stored transposed),
    opacity [P,1], scaling [P,2], rotation [P,4], raw values; the normals are zeros."""
    xyz = _flat("xyz", tensors["xyz"])
    cols = [xyz, np.zeros_like(xyz)] + [_flat(k, tensors[k]) for k, _ in _ENV_FIELDS]
    _write_vertex_ply(path, env_attribute_names({k: tuple(tensors[k].shape) for k, _ in _ENV_FIELDS}), np.concatenate(cols, axis=1))


def load_env_ply(path: str, max_sh_degree: int = 3, device="cpu") -> Dict[str, torch.Tensor]:
    """EnvGaussianModel.load_ply (:236-275): the tensors of save_env_ply; the f_rest count is checked as the reference asserts it (:251)."""
    names, data = read_ply_vertices(path)
    col = {n: i for i, n in enumerate(names)}

    def group(prefix):
        ks = sorted([n for n in names if n.startswith(prefix)], key=lambda x: int(x.split("_")[-1]))
        return data[:, [col[k] for k in ks]]

    P = data.shape[0]
    f_rest = group("f_rest_")
    if f_rest.shape[1] != 3 * (max_sh_degree + 1) ** 2 - 3:
        raise ValueError(f"{path}: {f_rest.shape[1]} f_rest properties, sh degree {max_sh_degree} needs {3 * (max_sh_degree + 1) ** 2 - 3}")
    out = {
        "xyz": data[:, [col["x"], col["y"], col["z"]]],
        "features_dc": data[:, [col["f_dc_0"], col["f_dc_1"], col["f_dc_2"]]].reshape(P, 3, 1).transpose(0, 2, 1),
        "features_rest": f_rest.reshape(P, 3, (max_sh_degree + 1) ** 2 - 1).transpose(0, 2, 1),
        "opacity": data[:, [col["opacity"]]], "scaling": group("scale_"), "rotation": group("rot"),
    }
    return {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float32, device=device) for k, v in out.items()}


def load_env_maps(path: str, env_map=None, env_map_2=None):
    """The two `.map` files next to a PLY (:804-812): state dicts of EnvLight (key `base`, [6, res, res, 3])."""
    for env, suffix in ((env_map, "1.map"), (env_map_2, "2.map")):
        p = path.replace(".ply", suffix)
        if env is not None and os.path.exists(p):
            env.load_state_dict(torch.load(p, map_location="cpu"))


# ---- the input point cloud (scene/dataset_readers.py:168-197) ------------------------------------------------------------------------------
class BasicPointCloud(NamedTuple):
    """utils/graphics_utils.py:17-20"""
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}
_POINT_DTYPE = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
_POINT_PLY_NAMES = {"<f4": "float", "u1": "uchar"}


def storePly(path, xyz, rgb):
    """storePly (:182-197): x y z nx ny nz as float, red green blue as uchar, the normals zero, binary little endian -- the header and the
    rows `plyfile` writes for that structured array.  Values are cast as its element assignment casts them (colours truncate)."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError(f"materialrefgs_amd.io: storePly takes xyz and rgb of shape [N,3], got {xyz.shape} and {rgb.shape}")
    elements = np.zeros(xyz.shape[0], dtype=_POINT_DTYPE)
    for k, n in enumerate("xyz"):
        elements[n] = xyz[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        elements[n] = np.asarray(rgb[:, k], dtype=np.float64).astype(np.int64).astype(np.uint8) if rgb.dtype.kind == "f" else rgb[:, k]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}"] + \
             [f"property {_POINT_PLY_NAMES[t]} {n}" for n, t in _POINT_DTYPE] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(elements.tobytes())


def read_ply_points(path):
    """The vertex element of a binary little-endian PLY as a structured array, whatever scalar types its properties have."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, count, fields, element = None, None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                element = tok[1]
                if element == "vertex":
                    count = int(tok[2])
                elif count is None:
                    raise ValueError("the vertex element must come first")
            elif tok[0] == "property" and element == "vertex":
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"unsupported vertex property type {tok[1]}")
                fields.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"unsupported PLY format {fmt}")
        dtype = np.dtype(fields)
        data = np.frombuffer(f.read(count * dtype.itemsize), dtype=dtype)
        if len(data) != count:
            raise ValueError("PLY file is shorter than its header says")
    return data


def fetchPly(path):
    """fetchPly (:168-180): positions as stored, colours / 255.0, normals; a file without colours or normals gets the reference's random
    ones (numpy's global generator, colours first)."""
    vertices = read_ply_points(path)
    positions = np.vstack([vertices['x'], vertices['y'], vertices['z']]).T
    try:
        colors = np.vstack([vertices['red'], vertices['green'], vertices['blue']]).T / 255.0
        normals = np.vstack([vertices['nx'], vertices['ny'], vertices['nz']]).T
    except ValueError:                                   # "no field of name ..."
        print('Load Ply color and normals failed, random init')
        colors = np.random.rand(*positions.shape) / 255.0
        normals = np.random.rand(*positions.shape)
        normals = normals / np.linalg.norm(normals, axis=-1, keepdims=True)
    return BasicPointCloud(points=positions, colors=colors, normals=normals)


# ---- PNG decoding: the counterpart of evaluate.write_png ------------------------------------------------------------------------------------
_PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def _paeth_row(cur, prev, bpp):
    out = bytearray(cur)
    for i in range(len(out)):
        a = out[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        out[i] = (out[i] + (a if pa <= pb and pa <= pc else (b if pb <= pc else c))) & 255
    return out


def _average_row(cur, prev, bpp):
    out = bytearray(cur)
    for i in range(len(out)):
        out[i] = (out[i] + (((out[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
    return out


def read_png(path):
    """uint8 [H,W] (grey) or [H,W,2|3|4] (grey+alpha, RGB, RGBA) of an 8-bit non-interlaced PNG, all five filter types, on the standard
    library's zlib.  Palette, 16-bit and interlaced files raise ValueError.  Checksums are verified."""
    import struct
    import zlib
    raw = open(path, "rb").read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    at, head, idat = 8, None, []
    while at + 12 <= len(raw):
        n, tag = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        if len(data) != n or struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] != zlib.crc32(tag + data) & 0xFFFFFFFF:
            raise ValueError(f"{path}: damaged {tag!r} chunk")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"IEND":
            break
        at += 12 + n
    if head is None:
        raise ValueError(f"{path}: no IHDR chunk")
    W, H, depth, colour, comp, filt, interlace = head
    if colour == 3:
        raise ValueError(f"{path}: palette PNG files are not read (convert to RGB)")
    if depth != 8 or colour not in _PNG_CHANNELS:
        raise ValueError(f"{path}: only 8-bit grey / grey+alpha / RGB / RGBA PNG files are read, got bit depth {depth}, colour type {colour}")
    if interlace != 0:
        raise ValueError(f"{path}: interlaced PNG files are not read")
    if comp != 0 or filt != 0 or W < 1 or H < 1:
        raise ValueError(f"{path}: malformed IHDR")
    bpp = _PNG_CHANNELS[colour]
    stride = W * bpp
    data = zlib.decompress(b"".join(idat))
    if len(data) != H * (1 + stride):
        raise ValueError(f"{path}: {len(data)} bytes of image data, expected {H * (1 + stride)}")
    rows = np.frombuffer(data, dtype=np.uint8).reshape(H, 1 + stride)
    out = np.empty((H, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for y in range(H):
        kind, cur = int(rows[y, 0]), rows[y, 1:]
        if kind == 0:
            out[y] = cur
        elif kind == 1:                                   # Sub: a running sum per channel, modulo 256
            out[y] = np.cumsum(cur.reshape(W, bpp), axis=0, dtype=np.uint8).reshape(stride)
        elif kind == 2:                                   # Up
            out[y] = cur + prev
        elif kind == 3:
            out[y] = np.frombuffer(bytes(_average_row(cur.tobytes(), prev.tobytes(), bpp)), dtype=np.uint8)
        elif kind == 4:
            out[y] = np.frombuffer(bytes(_paeth_row(cur.tobytes(), prev.tobytes(), bpp)), dtype=np.uint8)
        else:
            raise ValueError(f"{path}: unknown filter type {kind} in row {y}")
        prev = out[y]
    return out.reshape(H, W) if bpp == 1 else out.reshape(H, W, bpp)


def read_image(path):
    """(uint8 array [H,W] or [H,W,C], mode "L" / "LA" / "RGB" / "RGBA") of an image file: Pillow's decode when Pillow imports (palette and
    other modes converted as `Image.convert` does: P with transparency and anything with alpha to RGBA, the rest to RGB), otherwise
    read_png for PNG files.  Other formats without Pillow raise."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            if im.mode not in ("L", "LA", "RGB", "RGBA"):
                im = im.convert("RGBA" if (im.mode in ("PA", "RGBa", "La") or "transparency" in im.info) else "RGB")
            return np.array(im), im.mode
    if not str(path).lower().endswith(".png"):
        raise RuntimeError(f"{path}: only PNG files can be decoded without Pillow (JPEG and other formats need `pip install pillow`)")
    a = read_png(path)
    return a, {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[1 if a.ndim == 2 else a.shape[2]]
