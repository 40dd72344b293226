"""Vertex attributes of the mesh step (mrgs_vertex_fuse in csrc/mrgs_mesh.hip; pack_attributes, fuse_vertex_attributes, TriangleMesh and
GaussianExtractor in materialrefgs_amd/mesh.py; the material PLY in io.py) against the float64 statement tests/mesh_attr_statement.py,
which is itself held against the reference's own texturing arithmetic (tests/golden/reference_mesh_colour.npz).

Without a GPU: the statement against the reference's recorded results and its known answers, the argument codes of the new entry point,
the packing, the mesh accessors, both PLY writers.  On the GPU: the kernel within the statement's derived bound and with its exact
weights for every channel count and both start weights, the variants and edge cases, the acceptance branch, the bitwise equalities and the
front end."""
import ctypes
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_attr_statement as mas
import mesh_statement as ms

BAD_ARG, UNSUPPORTED = 1, 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_mesh_colour.npz")
H, W = 40, 48
TRUNC = float(np.float32(0.2))


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------
def test_statement_against_reference():
    """The reference's compute_unbounded_tsdf(..., return_rgb=True) in float64 on three views of two sizes and 257 points near the sphere
    (trunc = 5 * 0.02): on the points whose decisions are not within 1e-4 of a threshold the statement with w0 = 1 returns its rgbs, and
    mesh_statement.fuse its tsdfs, to 1e-12."""
    g = np.load(GOLDEN)
    views = [(g[f"proj_{i}"].astype(np.float64), g[f"depth_{i}"].astype(np.float64), g[f"rgb_{i}"].astype(np.float64)) for i in range(3)]
    assert {v[1].shape for v in views} == {(20, 24), (28, 32)}
    x = g["points"].astype(np.float64)
    trunc = 5 * float(g["voxel_size"])
    st = mas.fuse_attributes(x, trunc, views, 1)
    ts = ms.fuse(x, trunc, [(M, d) for M, d, _ in views], bound=False)
    ok = ~st["excluded"]
    assert len(x) == 257 and ok.mean() > 0.99
    assert np.abs(st["values"] - g["rgbs"])[ok].max() < 1e-12
    assert np.abs(ts["tsdf"] - g["tsdfs"])[ok].max() < 1e-12
    assert (st["w"] > 1).mean() > 0.9 and (g["rgbs"][ok] != 0).any(axis=1).mean() > 0.9      # the input does exercise the rule
    assert set(np.unique(st["w"])) >= {2.0, 3.0}                                               # points seen by one and by two views


def test_statement_known_answers():
    """A constant map: k accepted views give k / (k + 1) times the constant at w0 = 1 and the constant itself at w0 = 0 (0 for k = 0)."""
    views = _fusion_views()
    const = np.array([0.25, -3.0, 7.5])
    cv = [(M, d, np.broadcast_to(const, d.shape + (3,))) for M, d in views]
    x = _vertices()[::7].astype(np.float64)
    one, zero = mas.fuse_attributes(x, TRUNC, cv, 1), mas.fuse_attributes(x, TRUNC, cv, 0)
    k = zero["w"]
    assert (one["w"] == k + 1).all() and k.max() >= 3 and k.min() == 0
    assert np.abs(one["values"] - (k / (k + 1))[:, None] * const).max() < 1e-14
    assert np.abs(zero["values"] - np.where(k[:, None] > 0, const, 0.0)).max() < 1e-14


def test_argument_codes_without_gpu():
    """Every contract violation of mrgs_vertex_fuse is a status code before any HIP call (no GPU here: a call that got as far as a launch
    would return MRGS_E_HIP instead); the ABI version stays 10."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    assert L.mrgs_abi_version() == _lib.MRGS_ABI_VERSION == 10
    assert ctypes.sizeof(_lib.MrgsVertexFuseConfig) == 32 and ctypes.sizeof(_lib.MrgsAttrView) == 88
    buf = (ctypes.c_double * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                              # never dereferenced: every call below is refused first

    def vf(**kw):
        c = _lib.MrgsVertexFuseConfig(2, 5, 8, 1, 0.1, 0.0)
        views, points, out = kw.pop("views", p), kw.pop("points", p), kw.pop("out", p)
        for k, v in kw.items():
            setattr(c, k, v)
        return L.mrgs_vertex_fuse(ctypes.byref(c), views, points, out, None, None)
    assert vf(struct_size=28) == BAD_ARG
    for channels in (0, 3, 5, 20, -4):
        assert vf(channels=channels) == BAD_ARG
    for w0 in (2, -1):
        assert vf(w0=w0) == BAD_ARG
    for trunc in (0.0, -1.0, float("nan")):
        assert vf(trunc=trunc) == BAD_ARG
    assert vf(n_views=-1) == BAD_ARG
    assert vf(n_points=-1) == BAD_ARG
    assert vf(points=None) == BAD_ARG
    assert vf(out=None) == BAD_ARG
    assert vf(views=None) == BAD_ARG
    assert vf(out=p + 4) == BAD_ARG and vf(out=p + 8) == BAD_ARG        # out is stored 16 bytes at a time
    assert vf(n_points=2 ** 39) == UNSUPPORTED                          # beyond one launch's grid, as mrgs_tsdf_fuse
    assert vf(n_points=2 ** 39, channels=5) == BAD_ARG
    assert vf(n_points=0, points=None, out=None, views=None) == 0       # nothing to do
    assert L.mrgs_vertex_fuse(None, p, p, p, None, None) == BAD_ARG


def test_pack_attributes():
    from materialrefgs_amd import mesh
    g = torch.Generator().manual_seed(0)
    rgb, rough, normal = torch.rand(3, 5, 7, generator=g), torch.rand(1, 5, 7, generator=g), torch.rand(3, 5, 7, generator=g)
    packed, layout = mesh.pack_attributes({"rgb": rgb, "roughness": rough, "normal": normal})
    assert packed.shape == (5, 7, 8) and packed.is_contiguous() and packed.dtype == torch.float32
    assert layout == {"rgb": slice(0, 3), "roughness": slice(3, 4), "normal": slice(4, 7)}
    assert torch.equal(packed[..., layout["rgb"]], rgb.permute(1, 2, 0)) and torch.equal(packed[..., 3], rough[0])
    assert torch.equal(packed[..., layout["normal"]], normal.permute(1, 2, 0)) and (packed[..., 7] == 0).all()
    listed = mesh.pack_attributes([rgb, rough])                          # a list: the tensor alone, 4 channels need no padding
    assert torch.is_tensor(listed) and listed.shape == (5, 7, 4) and torch.equal(listed[..., 3], rough[0])
    assert mesh.pack_attributes([torch.rand(16, 2, 2)]).shape == (2, 2, 16)
    with pytest.raises(ValueError, match="at most 16"):
        mesh.pack_attributes([torch.rand(16, 2, 2), rough[:, :2, :2]])
    with pytest.raises(TypeError, match="float32"):
        mesh.pack_attributes([rgb.double()])
    with pytest.raises(TypeError, match="one size"):
        mesh.pack_attributes([rgb, rough[:, :4]])


def test_triangle_mesh_accessors():
    from materialrefgs_amd.mesh import TriangleMesh
    v, t = torch.rand(6, 3), torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)
    plain = TriangleMesh(v, t)                                           # the two-argument form is unchanged
    assert plain.vertex_attributes_device is None and plain.layout is None and plain.vertices.shape == (6, 3)
    with pytest.raises(KeyError, match="rgb"):
        plain.attribute("rgb")
    a = torch.rand(6, 8)
    m = TriangleMesh(v, t, a, {"normal": slice(0, 3), "rgb": slice(3, 6), "metallic": slice(6, 7)})
    assert m.vertex_attributes_device is a
    assert torch.equal(m.attribute("rgb"), a[:, 3:6]) and m.attribute("metallic").shape == (6, 1)
    assert m.attribute("rgb").data_ptr() == a[:, 3:6].data_ptr()        # a view, not a copy
    c = m.vertex_colors
    assert c.dtype == np.float64 and c.shape == (6, 3) and np.array_equal(c, a[:, 3:6].double().numpy()) and m.vertex_colors is c
    with pytest.raises(KeyError, match="roughness"):
        m.attribute("roughness")
    with pytest.raises(ValueError, match="one row per vertex"):
        TriangleMesh(v, t, torch.rand(5, 4))


def _material_mesh(V=101, T=203, seed=0):
    from materialrefgs_amd.mesh import TriangleMesh
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    a = rng.standard_normal((V, 16)).astype(np.float32)
    if V:
        v[0] = [np.float32(1e-45), -0.0, np.float32(3.4e38)]             # a denormal, a signed zero, a huge value: bits must survive
        a[0, :3] = [np.float32(1e-45), -0.0, np.float32(-3.4e38)]
    t = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    layout = {"rgb": slice(0, 3), "normal": slice(3, 6), "diffuse": slice(6, 9), "base_color": slice(9, 12), "metallic": slice(12, 13),
              "roughness": slice(13, 14)}
    return TriangleMesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(a), layout), v, t, a, layout


def test_material_ply_round_trip(tmp_path):
    from materialrefgs_amd import io
    m, v, t, a, layout = _material_mesh()
    path = os.path.join(tmp_path, "sub", "material.ply")
    io.save_material_ply(path, m)
    got = io.load_material_ply(path)
    assert got["vertices"].dtype == np.float64 and got["triangles"].dtype == np.int32
    assert got["vertices"].tobytes() == v.astype(np.float64).tobytes() and got["triangles"].tobytes() == t.tobytes()
    for name, sl in layout.items():
        assert got[name].tobytes() == a[:, sl].astype(np.float64).tobytes(), name      # fp32 widened: the bits survive
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 101"]
    names = "x y z red green blue normal_x normal_y normal_z diffuse_r diffuse_g diffuse_b albedo_r albedo_g albedo_b metallic_0 roughness_0".split()
    assert head[3:20] == [f"property double {n}" for n in names]
    assert head[20:] == ["element face 203", "property list uchar int vertex_indices"]
    assert os.path.getsize(path) == len("\n".join(head)) + len("\nend_header\n") + 101 * 17 * 8 + 203 * 13
    empty, *_ = _material_mesh(0, 0)
    io.save_material_ply(path, empty)
    got = io.load_material_ply(path)
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["roughness"].shape == (0, 1)
    from materialrefgs_amd.mesh import TriangleMesh
    with pytest.raises(KeyError, match="normal"):
        io.save_material_ply(path, TriangleMesh(m.vertices_device, m.triangles_device, m.vertex_attributes_device, {"rgb": slice(0, 3)}))


def test_mesh_ply_with_and_without_colours(tmp_path):
    from materialrefgs_amd import io
    from materialrefgs_amd.mesh import TriangleMesh
    m, v, t, a, layout = _material_mesh(seed=1)
    a[1, :3], a[2, :3], a[3, :3] = [0.0, 1.0, 0.5], [-0.2, 1.7, 0.25], [0.499 / 255, 0.501 / 255, 254.5 / 255]
    coloured, plain = os.path.join(tmp_path, "c.ply"), os.path.join(tmp_path, "p.ply")
    io.save_mesh_ply(coloured, m)
    raw = open(coloured, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode().splitlines() == ["ply", "format binary_little_endian 1.0", "element vertex 101", "property float x", "property float y",
                                          "property float z", "property uchar red", "property uchar green", "property uchar blue",
                                          "element face 203", "property list uchar int vertex_indices"]
    rows = np.frombuffer(body[:101 * 15], dtype=np.uint8).reshape(101, 15)
    assert rows[:, :12].tobytes() == v.tobytes()
    want = np.round(np.clip(a[:, :3].astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(rows[:, 12:], want)
    assert rows[1, 12:].tolist() == [0, 255, 128] and rows[2, 12:].tolist() == [0, 255, 64] and rows[3, 12:].tolist() == [0, 1, 254]
    assert len(body) == 101 * 15 + 203 * 13 and body.endswith(t[-1].tobytes())
    v2, t2 = io.load_mesh_ply(coloured)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()   # the geometry, bit for bit
    # no rgb group: byte for byte the file of the two arrays
    io.save_mesh_ply(plain, v, t)
    ref = open(plain, "rb").read()
    for other in (TriangleMesh(m.vertices_device, m.triangles_device), TriangleMesh(m.vertices_device, m.triangles_device, m.vertex_attributes_device,
                                                                                  {"normal": slice(3, 6)})):
        io.save_mesh_ply(plain, other)
        assert open(plain, "rb").read() == ref


def test_front_end_refuses_host_tensors_and_wrong_types():
    from materialrefgs_amd import mesh
    with pytest.raises(RuntimeError, match="device tensor"):
        mesh.fuse_vertex_attributes(torch.zeros(4, 3), [(torch.eye(4), torch.ones(8, 6), torch.ones(8, 6, 4))], 0.1)
    ex = mesh.GaussianExtractor(SimpleNamespace(), None, None, device="cpu")
    with pytest.raises(ValueError, match="albedo"):
        ex.reconstruction([], attributes=("rgb", "albedo"))
    with pytest.raises(ValueError, match="missing: normal, diffuse, base_color, metallic, roughness"):
        ex.attribute_layout = {"rgb": slice(0, 3)}
        ex.extract_mesh_bouned_with_material()


# ---- the scene of the GPU tests (tests/test_mesh.py's) ------------------------------------------------------------------------------
def _cameras(n, H, W, distance=2.2, fov_deg=40.0, elevations=(0.0,), azimuth0=10.0):
    from materialrefgs_amd.camera import look_at_camera
    return [look_at_camera(azimuth0 + 360.0 * i / n, elevations[i % len(elevations)], distance, math.radians(fov_deg), H, W) for i in range(n)]


@functools.lru_cache(maxsize=None)
def _fusion_views():
    """Six views of 48 x 40 on a circle of radius 2.2, FoV 40 degrees: the 0.5 sphere in front of a wall at view depth 3.1."""
    return tuple((c.full_proj_transform.numpy().astype(np.float32), ms.analytic_depth(c, H, W)) for c in _cameras(6, H, W))


@functools.lru_cache(maxsize=None)
def _vertices():
    """The vertices of the statement's own mesh of that scene (lattice ms.ORG / ms.SPACING / ms.SHAPE, trunc 0.2), rounded to fp32."""
    x, _ = ms.plain_samples(ms.ORG, ms.SPACING, ms.SHAPE)
    field = ms.fuse(x, TRUNC, list(_fusion_views()), bound=False)["tsdf"].astype(np.float32).reshape(ms.SHAPE)
    v = ms.marching_tetrahedra(field, 0.0, ms.ORG, ms.SPACING)["vertices"].astype(np.float32)
    v.setflags(write=False)
    return v


def _maps(i, h, w):
    """fp32 [h,w,17]: sixteen analytic channels and, last, the pattern the tests put into padding channels (non-zero, unlike any channel)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pad = (3.0 + 0.05 * xx - 0.03 * yy + 0.5 * i).astype(np.float32)
    return np.concatenate([mas.analytic_attributes(i, h, w, 16), pad[..., None]], axis=-1)


@functools.lru_cache(maxsize=None)
def _scene(variant):
    """(views as (proj, depth, maps [h,w,17]), depth_trunc) of a variant of the scene."""
    base = list(_fusion_views())
    depth_trunc = None
    if variant == "holed":                                              # the maps of test_fusion_variants: only taps wholly on the sphere count
        holed = []
        for M, d in base:
            d = d.copy()
            d[12:22, 18:30] = 0.0
            holed.append((M, d))
        base, depth_trunc = holed, float(np.float32(3.0))
    elif variant == "two sizes":
        cams = _cameras(4, 28, 32, elevations=(20.0, -35.0), azimuth0=40.0)
        base = base[:3] + [(c.full_proj_transform.numpy().astype(np.float32), ms.analytic_depth(c, 28, 32)) for c in cams] + base[3:]
    else:
        assert variant == "free"
    return tuple((M, d, _maps(i, *d.shape)) for i, (M, d) in enumerate(base)), depth_trunc


@functools.lru_cache(maxsize=None)
def _statement(variant, w0):
    """The statement on all 17 channels of the variant, computed once; a CP-channel run is its first CP - 1 channels and the last."""
    views, depth_trunc = _scene(variant)
    return mas.fuse_attributes(_vertices().astype(np.float64), TRUNC, list(views), w0, depth_trunc=depth_trunc)


def _channels(cp):
    return list(range(cp - 1)) + [16]


def _run(dev, variant, cp, w0, rows=slice(None), weight=True, extra=None):
    from materialrefgs_amd import mesh
    views, depth_trunc = _scene(variant)
    dv = [(torch.from_numpy(M).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(a[..., _channels(cp)])).to(dev))
          for M, d, a in views]
    if extra is not None:
        dv = extra(dv)
    pts = torch.from_numpy(np.array(_vertices()[rows])).to(dev)
    return mesh.fuse_vertex_attributes(pts, dv, TRUNC, depth_trunc=depth_trunc or 0.0, mean=(w0 == 0), return_weight=weight)


def _check(name, got, got_w, st, cp, rows=slice(None), max_excluded=0.01):
    got, got_w = got.double().cpu().numpy(), got_w.double().cpu().numpy()
    ok = ~st["excluded"][rows]
    want, tol, w = st["values"][rows][:, _channels(cp)], st["tol"][rows][:, _channels(cp)], st["w"][rows]
    assert got.shape == want.shape and got_w.shape == w.shape
    frac = st["excluded"].mean()
    diff = np.abs(got - want)[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff > 0, diff / tol[ok], 0.0)
    print(f"[{name}] points {len(got)}  excluded {100 * frac:.3f} %  points by w {np.bincount(w.astype(int)).tolist()}  "
          f"worst |diff| {diff.max(initial=0):.3e}  worst diff/bound {np.nanmax(ratio, initial=0):.3f}  wrong weights {(got_w[ok] != w[ok]).sum()}")
    assert frac <= max_excluded
    assert (got_w[ok] == w[ok]).all()
    assert (diff <= tol[ok]).all()


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w0", (0, 1))
@pytest.mark.parametrize("cp", (4, 8, 12, 16))
def test_fusion_against_statement(gpu_device, cp, w0):
    """The 14 418 vertices of the statement's mesh, six views, trunc 0.2: every vertex whose decisions are not within 1e-4 of a threshold
    carries exactly the statement's w and every channel within the bound mesh_attr_statement.fuse_attributes derives from fp32 rounding
    of the stated operation sequence; at most 1 % of the vertices may be left out.  The last channel of the packed maps holds a pattern of
    its own, as a padding channel might: channels do not mix."""
    st = _statement("free", w0)
    assert len(_vertices()) == 14418
    k = st["w"] - w0
    assert k.min() == 0 and k.max() == 4 and 0 < (k == 0).mean() < 0.01                        # seen by 0 to 4 views; some by none
    out, w = _run(gpu_device, "free", cp, w0)
    _check(f"CP {cp} w0 {w0}", out, w, st, cp)
    none = torch.from_numpy(k == 0).to(gpu_device)
    assert (out[none] == 0).all() and (w[none] == w0).all()                                   # no view: 0, and w0


@pytest.mark.gpu
def test_fusion_variants_and_edges(gpu_device):
    """Texel validity (the holed maps of test_fusion_variants, depth_trunc 3.0: the counts fall against the free run), views of two sizes
    in one table, one point, 257 points (one thread past a workgroup), no view, no point."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    for w0 in (0, 1):
        st, free = _statement("holed", w0), _statement("free", w0)
        assert (st["w"] < free["w"]).mean() > 0.3 and (st["w"] > w0).mean() > 0.05
        _check(f"validity w0 {w0}", *_run(dev, "holed", 8, w0), st, 8)
        _check(f"two sizes w0 {w0}", *_run(dev, "two sizes", 12, w0), _statement("two sizes", w0), 12)
    full, full_w = _run(dev, "free", 16, 1)
    for n in (1, 257):
        out, w = _run(dev, "free", 16, 1, rows=slice(0, n))
        _check(f"n = {n}", out, w, _statement("free", 1), 16, rows=slice(0, n))
        assert torch.equal(out, full[:n]) and torch.equal(w, full_w[:n])
    pts = torch.from_numpy(_vertices()[:300].copy()).to(dev)
    for mean in (False, True):
        out, w = mesh.fuse_vertex_attributes(pts, [], TRUNC, mean=mean, return_weight=True)
        assert out.shape == (300, 4) and (out == 0).all() and (w == (0.0 if mean else 1.0)).all()
    out, w = _run(dev, "free", 8, 1, rows=slice(0, 0))
    assert out.shape == (0, 8) and w.shape == (0,)
    M0, d0, a0 = _scene("free")[0][0]
    M, d, a = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (M0, d0, a0[..., :4]))
    with pytest.raises(TypeError, match="float32"):
        mesh.fuse_vertex_attributes(pts, [(M, d, a.double())], TRUNC)
    with pytest.raises(ValueError, match="4, 8, 12 or 16"):
        mesh.fuse_vertex_attributes(pts, [(M, d, a[..., :3])], TRUNC)
    with pytest.raises(ValueError, match="a view is"):
        mesh.fuse_vertex_attributes(pts, [(M, d, a[:-1])], TRUNC)


@pytest.mark.gpu
def test_attributes_are_read_only_behind_the_acceptance_branch(gpu_device):
    """Two more views whose attribute maps are all NaN: a camera that looks away from the scene (no point passes z > 0) and a view whose
    depth map says 0.1 everywhere, so that every point in its frustum fails sdf > -trunc.  The output is finite and bitwise the run
    without them: a rejected view's attributes never reach the accumulators."""
    from materialrefgs_amd.camera import look_at_camera
    dev = gpu_device
    eye = 2.2 * np.array([math.cos(math.radians(100.0)), math.sin(math.radians(100.0)), 0.0])
    away = look_at_camera(280.0, 0.0, 2.2, math.radians(40.0), H, W, target=tuple(2.0 * eye))      # stands at `eye` on the orbit, its back to the scene
    x = _vertices().astype(np.float64)
    assert ((x @ away.full_proj_transform.double().numpy()[:3] + away.full_proj_transform.double().numpy()[3])[:, 3] < 0).all()
    near = _cameras(1, H, W, azimuth0=55.0)[0]
    clip = x @ near.full_proj_transform.double().numpy()[:3] + near.full_proj_transform.double().numpy()[3]
    assert (np.abs(clip[:, :2] / clip[:, 3:]) < 1).all(axis=1).mean() > 0.5 and (0.1 - clip[:, 3] < -2 * TRUNC).all()     # most points in its frustum, every sdf far below -trunc
    nan = torch.full((H, W, 8), float("nan"), device=dev)

    def extra(dv):
        a = (away.full_proj_transform.to(dev), torch.full((H, W), 3.1, device=dev), nan)
        b = (near.full_proj_transform.to(dev), torch.full((H, W), 0.1, device=dev), nan)
        return dv[:2] + [a] + dv[2:5] + [b] + dv[5:]
    for w0 in (0, 1):
        base, base_w = _run(dev, "free", 8, w0)
        out, w = _run(dev, "free", 8, w0, extra=extra)
        assert torch.isfinite(out).all() and torch.equal(out, base) and torch.equal(w, base_w)


@pytest.mark.gpu
def test_bitwise_equalities(gpu_device):
    """Two calls agree bit for bit; without the weight output the values are the same; and the w of a w0 = 1 run without texel validity is
    tsdf_fuse's weight on the same points, bit for bit: both use the same acceptance arithmetic."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    for variant, cp in (("free", 16), ("two sizes", 4)):
        out, w = _run(dev, variant, cp, 1)
        again, again_w = _run(dev, variant, cp, 1)
        assert torch.equal(out, again) and torch.equal(w, again_w)
        assert torch.equal(_run(dev, variant, cp, 1, weight=False), out)
        views = [(torch.from_numpy(M).to(dev), torch.from_numpy(d).to(dev)) for M, d, _ in _scene(variant)[0]]
        _, fw = mesh.tsdf_fuse(views, TRUNC, points=torch.from_numpy(_vertices().copy()).to(dev), return_weight=True)
        assert torch.equal(w, fw)
        mean, mean_w = _run(dev, variant, cp, 0)
        assert torch.equal(mean_w, w - 1)


# ---- the front end -----------------------------------------------------------------------------------------------------------------
GROUPS = ("rgb", "normal", "diffuse", "base_color", "metallic", "roughness")
SOURCES = {"rgb": ("render", slice(0, 3)), "normal": ("rend_normal", slice(3, 6)), "diffuse": ("diffuse_map", slice(6, 9)),
           "base_color": ("base_color_map", slice(9, 12)), "metallic": ("refl_strength_map", slice(12, 13)), "roughness": ("roughness_map", slice(13, 14))}


class _StubRender:
    """render(viewpoint_camera, pc, pipe=, bg_color=, opt=) -> analytic maps on the device: the depth of the sphere before the wall and
    fourteen smooth channels dealt to the six groups (rend_normal is not of unit length: the extractor normalises it)."""

    def __init__(self, cams):
        self.index = {id(c): i for i, c in enumerate(cams)}

    def __call__(self, cam, pc, pipe=None, bg_color=None, opt=None):
        dev = cam.full_proj_transform.device
        i = self.index[id(cam)]
        host = SimpleNamespace(world_view_transform=cam.world_view_transform.cpu(), FoVx=cam.FoVx, FoVy=cam.FoVy)
        pkg = {"surf_depth": torch.from_numpy(ms.analytic_depth(host, H, W)).to(dev)[None]}
        maps = torch.from_numpy(mas.analytic_attributes(i, H, W, 14)).to(dev).permute(2, 0, 1)
        for key, sl in SOURCES.values():
            pkg[key] = maps[sl].contiguous() - (0.5 if key == "rend_normal" else 0.0)
        return pkg


def _extractor(dev, attributes):
    from materialrefgs_amd import mesh
    cams = [c.to(dev) for c in _cameras(6, H, W)]
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(2000, 3, generator=g)
    gaussians = SimpleNamespace(get_xyz=(0.5 * xyz / xyz.norm(dim=1, keepdim=True)).to(dev))
    render = _StubRender(cams)
    ex = mesh.GaussianExtractor(gaussians, render, SimpleNamespace(), bg_color=[0, 0, 0])
    ex.reconstruction(cams, attributes=attributes)
    return ex, cams, render


BOUNDED = dict(voxel_size=0.06, sdf_trunc=0.24, depth_trunc=2.4)         # a lattice of 41^3; the wall at 3.1 lies beyond depth_trunc


@pytest.mark.gpu
def test_extractor_fuses_attributes_and_leaves_the_geometry_alone(gpu_device):
    """reconstruction(..., attributes=...) keeps one packed tensor per view; both extractions return the geometry of the run without
    attributes bit for bit, with attributes that are bitwise fuse_vertex_attributes on the final vertices with the documented parameters:
    unbounded trunc = 5 voxels, sum / (k + 1), no texel validity; bounded trunc = sdf_trunc, the plain mean, the mode's texel validity."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    ex, cams, render = _extractor(dev, GROUPS)
    bare, _, _ = _extractor(dev, ())
    assert bare.attrmaps == [] and bare.attribute_layout is None
    assert len(ex.attrmaps) == 6 and all(a.is_cuda and a.shape == (H, W, 16) and a.is_contiguous() for a in ex.attrmaps)
    assert ex.attribute_layout == {g: sl for g, (_, sl) in SOURCES.items()}
    pkg = render(cams[2], None)
    for g, (key, sl) in SOURCES.items():
        want = torch.nn.functional.normalize(pkg[key], dim=0) if g == "normal" else pkg[key]
        assert torch.equal(ex.attrmaps[2][..., sl], want.permute(1, 2, 0)), g
    assert (ex.attrmaps[2][..., 14:] == 0).all()
    views = [(c.full_proj_transform, d, a) for c, d, a in zip(cams, ex.depthmaps, ex.attrmaps)]

    m, m0 = ex.extract_mesh_unbounded(40), bare.extract_mesh_unbounded(40)
    assert m0.vertex_attributes_device is None and len(m.triangles) > 1000
    assert torch.equal(m.vertices_device, m0.vertices_device) and torch.equal(m.triangles_device, m0.triangles_device)
    want = mesh.fuse_vertex_attributes(m.vertices_device, views, 5 * (ex.radius * 2 / 40))
    assert torch.equal(m.vertex_attributes_device, want) and m.layout == ex.attribute_layout
    assert m.vertex_colors.shape == (len(m.vertices), 3) and (m.vertex_colors > 0).any()

    b, b0 = ex.extract_mesh_bounded(**BOUNDED), bare.extract_mesh_bounded(**BOUNDED)
    assert ex.last_lattice["shape"] == (41, 41, 41) and len(b.triangles) > 1000
    assert torch.equal(b.vertices_device, b0.vertices_device) and torch.equal(b.triangles_device, b0.triangles_device)
    want = mesh.fuse_vertex_attributes(b.vertices_device, views, BOUNDED["sdf_trunc"], depth_trunc=BOUNDED["depth_trunc"], mean=True)
    assert torch.equal(b.vertex_attributes_device, want)
    n = b.attribute("normal")
    seen = n.norm(dim=1) > 0
    assert seen.float().mean() > 0.5 and (n[seen].norm(dim=1) <= 1 + 1e-5).all()              # a mean of unit vectors


@pytest.mark.gpu
def test_post_process_keeps_attribute_rows_with_their_vertices(gpu_device):
    """Two spheres: post_process_mesh(mesh, 1) drops the small one; the surviving attribute rows are those of the kept-vertex mask, in
    order, as the vertices are.  A mesh without attributes comes back without."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    m = mesh.marching_tetrahedra(torch.from_numpy(ms.known_field("two_spheres")).to(dev), 0.0, ms.ORG.astype(np.float32), ms.SPACING.astype(np.float32))
    V = m.vertices_device.shape[0]
    attrs = torch.from_numpy(np.random.default_rng(3).standard_normal((V, 12)).astype(np.float32)).to(dev)
    layout = {"rgb": slice(0, 3), "normal": slice(3, 6)}
    _, _, kept_v, _ = ms.post_process_mesh(m.vertices, m.triangles.astype(np.int64), 1)
    assert 0 < len(kept_v) < V
    out = mesh.post_process_mesh(mesh.TriangleMesh(m.vertices_device, m.triangles_device, attrs, layout), 1)
    assert out.layout == layout and out.vertex_attributes_device.shape == (len(kept_v), 12)
    assert np.array_equal(out.vertex_attributes_device.cpu().numpy(), attrs.cpu().numpy()[kept_v])
    assert np.array_equal(out.vertices, m.vertices[kept_v])
    plain = mesh.post_process_mesh(m, 1)
    assert plain.vertex_attributes_device is None and plain.layout is None
    assert torch.equal(plain.vertices_device, out.vertices_device) and torch.equal(plain.triangles_device, out.triangles_device)


@pytest.mark.gpu
def test_material_mesh_is_written_and_read_back(gpu_device, tmp_path):
    """extract_mesh_bouned_with_material: one extraction, the largest cluster, a material PLY that load_material_ply reads back equal to
    the returned mesh; with a group missing it raises and names the group."""
    from materialrefgs_amd import io, mesh
    ex, _, _ = _extractor(gpu_device, GROUPS)
    path = os.path.join(tmp_path, "out", "material.ply")
    m = ex.extract_mesh_bouned_with_material(BOUNDED["voxel_size"], BOUNDED["sdf_trunc"], BOUNDED["depth_trunc"], True, save_path=path)
    want = mesh.post_process_mesh(ex.extract_mesh_bounded(**BOUNDED), 1)
    assert len(m.triangles) > 1000 and torch.equal(m.vertices_device, want.vertices_device) and torch.equal(m.triangles_device, want.triangles_device)
    assert torch.equal(m.vertex_attributes_device, want.vertex_attributes_device)
    got = io.load_material_ply(path)
    assert np.array_equal(got["vertices"], m.vertices.astype(np.float64)) and np.array_equal(got["triangles"], m.triangles)
    for g in GROUPS:
        assert np.array_equal(got[g], m.attribute(g).double().cpu().numpy()), g
    few, _, _ = _extractor(gpu_device, ("rgb", "normal", "diffuse", "base_color", "metallic"))
    with pytest.raises(ValueError, match="missing: roughness"):
        few.extract_mesh_bouned_with_material(save_path=path)
