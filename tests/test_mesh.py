"""Mesh extraction (materialrefgs_amd/mesh.py, csrc/mrgs_mesh.hip) against its float64 statement (tests/mesh_statement.py).

Without a GPU: the statement's known answers, the argument checks of every new entry point, the bounding sphere, the mesh PLY.
On the GPU: fusion within the statement's derived bound and with its exact update counts, extraction as exact triangle sets with vertex
positions within the derived tolerance, clusters and the floater rule bit for bit.  The view table of mrgs_tsdf_fuse is unbounded (one
launch serves any number of views), so there is no "one more view than a table holds" case."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mesh_statement as ms

BAD_ARG, WORKSPACE, UNSUPPORTED = 1, 5, 6


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------
def test_statement_known_answers():
    """Sphere, torus and two spheres on the 40 x 36 x 44 lattice: vertex and triangle counts, Euler characteristic, components, every edge
    in exactly two triangles, every directed edge once, no zero-area triangle, outward winding (and the kernel's parity rule for the
    winding agrees with the geometry on every triangle)."""
    assert ms.self_test()


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_argument_validation_without_gpu():
    """Every contract violation of the mesh entry points is a status code before any HIP call (no GPU here: a call that got as far as
    a launch would return MRGS_E_HIP instead)."""
    from materialrefgs_amd import _lib
    from materialrefgs_amd._lib import MrgsMeshConfig, MrgsTsdfConfig
    L = _lib.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)                                      # never dereferenced: every call below is refused first

    def tsdf(**kw):
        c = MrgsTsdfConfig(_lib.MRGS_TSDF_PLAIN, 4, 4, 4, 2, 0, _f3(0, 0, 0), _f3(1, 1, 1), _f3(0, 0, 0), 1.0, 0.1, 0.0, None)
        views, field = kw.pop("views", p), kw.pop("field", p)
        for k, v in kw.items():
            setattr(c, k, v)
        return L.mrgs_tsdf_fuse(ctypes.byref(c), views, field, None, None)
    assert tsdf(struct_size=80) == BAD_ARG
    assert tsdf(mode=3) == BAD_ARG
    assert tsdf(n1=1) == BAD_ARG
    assert tsdf(trunc=0.0) == BAD_ARG
    assert tsdf(trunc=float("nan")) == BAD_ARG
    assert tsdf(n_views=-1) == BAD_ARG
    assert tsdf(field=None) == BAD_ARG
    assert tsdf(views=None) == BAD_ARG
    assert tsdf(mode=_lib.MRGS_TSDF_CONTRACTED, radius=0.0) == BAD_ARG
    assert tsdf(mode=_lib.MRGS_TSDF_POINTS, n_points=5, points=None) == BAD_ARG
    assert tsdf(mode=_lib.MRGS_TSDF_POINTS, n_points=-1, points=p) == BAD_ARG
    assert tsdf(mode=_lib.MRGS_TSDF_POINTS, n_points=2 ** 39, points=p) == UNSUPPORTED                 # beyond one launch's grid
    assert tsdf(mode=_lib.MRGS_TSDF_POINTS, n_points=0, points=None, field=None, views=None) == 0      # nothing to do
    assert L.mrgs_tsdf_fuse(None, p, p, None, None) == BAD_ARG

    def cfg(**kw):
        c = MrgsMeshConfig(40, 36, 44, 16, 0, 0.0, _f3(0, 0, 0), _f3(1, 1, 1), _f3(0, 0, 0), 1.0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    good = cfg()
    need = L.mrgs_mesh_ws_bytes(ctypes.byref(good))
    assert need >= 17 * 36 * 44 * 4                                # one word per point of a slab of 16 cube layers
    assert L.mrgs_mesh_ws_bytes(ctypes.byref(cfg(slab_planes=1))) < need // 4
    totals = (ctypes.c_int64 * 2)(10, 10)
    for bad in (cfg(struct_size=64), cfg(n0=1), cfg(n2=1), cfg(slab_planes=0), cfg(spacing=_f3(1, 0, 1)), cfg(level=float("nan")),
                cfg(contracted=1, radius=0.0)):
        assert L.mrgs_mesh_ws_bytes(ctypes.byref(bad)) == 0
        assert L.mrgs_mesh_count(ctypes.byref(bad), p, p, need, p, None) == BAD_ARG
        assert L.mrgs_mesh_emit(ctypes.byref(bad), p, p, need, totals, p, p, None) == BAD_ARG
    assert L.mrgs_mesh_count(ctypes.byref(cfg(n0=2, n1=20000, n2=20000)), p, p, need, p, None) == UNSUPPORTED      # a slab beyond 2^28 points
    assert L.mrgs_mesh_count(ctypes.byref(good), None, p, need, p, None) == BAD_ARG
    assert L.mrgs_mesh_count(ctypes.byref(good), p, None, need, p, None) == BAD_ARG
    assert L.mrgs_mesh_count(ctypes.byref(good), p, p, need, None, None) == BAD_ARG
    assert L.mrgs_mesh_count(ctypes.byref(good), p, p + 4, need, p, None) == BAD_ARG
    assert L.mrgs_mesh_count(ctypes.byref(good), p, p, need - 1, p, None) == WORKSPACE
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need - 1, totals, p, p, None) == WORKSPACE
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, None, p, p, None) == BAD_ARG
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, totals, None, p, None) == BAD_ARG
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, totals, p, None, None) == BAD_ARG
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, (ctypes.c_int64 * 2)(-1, 0), p, p, None) == BAD_ARG
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, (ctypes.c_int64 * 2)(2 ** 31, 5), p, p, None) == UNSUPPORTED
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, (ctypes.c_int64 * 2)(5, 2 ** 31), p, p, None) == UNSUPPORTED
    assert L.mrgs_mesh_emit(ctypes.byref(good), p, p, need, (ctypes.c_int64 * 2)(0, 0), None, None, None) == 0     # empty mesh: nothing launched

    assert L.mrgs_mesh_clusters(-1, 0, p, p, p, None) == BAD_ARG
    assert L.mrgs_mesh_clusters(5, 5, None, p, p, None) == BAD_ARG
    assert L.mrgs_mesh_clusters(5, 5, p, None, p, None) == BAD_ARG
    assert L.mrgs_mesh_clusters(2 ** 31, 5, p, p, p, None) == UNSUPPORTED
    assert L.mrgs_mesh_clusters(0, 0, None, None, None, None) == 0
    assert L.mrgs_mesh_select(5, 5, p, p, p, 50, None, p, None) == BAD_ARG
    assert L.mrgs_mesh_select(5, 5, p, None, p, 50, p, p, None) == BAD_ARG
    assert L.mrgs_mesh_select(5, 2 ** 31, p, p, p, 50, p, p, None) == UNSUPPORTED
    assert L.mrgs_mesh_select(0, 0, None, None, None, 50, None, None, None) == 0
    assert L.mrgs_mesh_reindex(5, 6, p, p, 5, p, None) == BAD_ARG
    assert L.mrgs_mesh_reindex(5, 4, None, p, 5, p, None) == BAD_ARG
    assert L.mrgs_mesh_reindex(5, 4, p, p, 2 ** 31, p, None) == UNSUPPORTED
    assert L.mrgs_mesh_reindex(5, 4, None, None, 0, None, None) == 0


def test_python_front_end_refuses_host_tensors_and_wrong_types():
    from materialrefgs_amd import mesh
    proj, depth = torch.eye(4), torch.ones(8, 6)
    with pytest.raises(RuntimeError, match="device tensor"):
        mesh.tsdf_fuse([(proj, depth)], 0.1, points=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="device tensor"):
        mesh.marching_tetrahedra(torch.zeros(4, 4, 4), 0.0, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="device tensor"):
        mesh.post_process_mesh(mesh.TriangleMesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="points.*or a lattice"):
        mesh.tsdf_fuse([], 0.1)
    with pytest.raises(ValueError, match="at least 1"):
        mesh.post_process_mesh(None, 0)


def test_ray_tracer_names_the_empty_mesh():
    """A mesh of 8 triangles or fewer (everything removed: the largest cluster was under 50 triangles) is refused in words."""
    from materialrefgs_amd.raytracing import RayTracer
    with pytest.raises(AssertionError, match="more than 8 triangles.*got 0.*post_process_mesh"):
        RayTracer(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))


def _cameras(n, H, W, distance=2.2, fov_deg=40.0, elevations=(0.0,), azimuth0=10.0):
    from materialrefgs_amd.camera import look_at_camera
    return [look_at_camera(azimuth0 + 360.0 * i / n, elevations[i % len(elevations)], distance, math.radians(fov_deg), H, W) for i in range(n)]


def test_estimate_bounding_sphere_against_float64():
    """Twelve look-at cameras at distance 2.2 from (0.1, -0.2, 0.05): the centre is the least-squares point of the optical axes and the
    radius the smallest camera distance.  The cameras carry fp32 matrices (relative error 2^-24 on entries of size <= 2.2, through one
    4 x 4 inversion and a well-conditioned 3 x 3 solve): 1e-5 is two orders above that."""
    from types import SimpleNamespace
    from materialrefgs_amd import mesh
    from materialrefgs_amd.camera import look_at_camera
    target = np.array([0.1, -0.2, 0.05])
    cams = [look_at_camera(30.0 * i, (-25.0, 10.0, 40.0)[i % 3], 2.2, math.radians(40.0), 64, 64, target=tuple(target)) for i in range(12)]
    ex = mesh.GaussianExtractor(SimpleNamespace(), None, None, device="cpu")
    ex.viewpoint_stack = cams
    ex.estimate_bounding_sphere()
    # float64, from the camera centres and forward axes: sum_i (I - d d^T) (c - o_i) = 0
    A, b = np.zeros((3, 3)), np.zeros(3)
    for c in cams:
        o = c.camera_center.double().numpy()
        d = c.R.double().numpy()[:, 2]
        d = d / np.linalg.norm(d)
        m = np.eye(3) - np.outer(d, d)
        A += m
        b += m @ o
    centre = np.linalg.solve(A, b)
    assert np.abs(centre - target).max() < 1e-5
    assert np.abs(ex.center.double().numpy() - centre).max() < 1e-5
    radius = min(np.linalg.norm(c.camera_center.double().numpy() - centre) for c in cams)
    assert abs(ex.radius - radius) < 1e-5 and abs(ex.radius - 2.2) < 1e-5


def test_mesh_ply_round_trip(tmp_path):
    from materialrefgs_amd import io
    rng = np.random.default_rng(0)
    v = rng.standard_normal((1001, 3)).astype(np.float32)
    v[0] = [np.float32(1e-45), -0.0, np.float32(3.4e38)]           # a denormal, a signed zero, a huge value: bits must survive
    t = rng.integers(0, 1001, (1999, 3)).astype(np.int32)
    path = os.path.join(tmp_path, "sub", "mesh.ply")
    io.save_mesh_ply(path, v, t)
    v2, t2 = io.load_mesh_ply(path)
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    head = open(path, "rb").read(200).split(b"end_header\n")[0].decode()
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head and "element face 1999" in head
    from materialrefgs_amd.mesh import TriangleMesh
    m = TriangleMesh(torch.from_numpy(v), torch.from_numpy(t))
    io.save_mesh_ply(path, m)
    assert open(path, "rb").read().endswith(t[-1].tobytes())
    io.save_mesh_ply(path, v[:0], t[:0])
    v3, t3 = io.load_mesh_ply(path)
    assert v3.shape == (0, 3) and t3.shape == (0, 3)


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fusion_views():
    """Six views of 48 x 40 on a circle of radius 2.2, FoV 40 degrees: the 0.5 sphere in front of a wall at view depth 3.1."""
    H, W = 40, 48
    cams = _cameras(6, H, W)
    return [(c.full_proj_transform.numpy().astype(np.float32), ms.analytic_depth(c, H, W)) for c in cams]


def _device_views(views, dev):
    return [(torch.from_numpy(M).to(dev), torch.from_numpy(d).to(dev)) for M, d in views]


def _check_fusion(name, got, got_w, st, max_excluded=0.01):
    got, got_w = got.double().cpu().numpy().ravel(), got_w.double().cpu().numpy().ravel()
    ok = ~st["excluded"]
    frac = 1.0 - ok.mean()
    diff = np.abs(got - st["tsdf"])[ok]
    tol = st["tol"][ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff > 0, diff / tol, 0.0)
    updated = (st["w"] > 1).mean()
    print(f"[{name}] samples {len(got)}  excluded {100 * frac:.3f} %  updated {100 * updated:.1f} %  views/sample {st['w'].mean() - 1:.2f}  "
          f"worst |diff| {diff.max():.3e}  worst diff/bound {np.nanmax(ratio):.3f}  wrong counts {(got_w[ok] != st['w'][ok]).sum()}")
    assert frac <= max_excluded
    assert (got_w[ok] == st["w"][ok]).all()
    assert (diff <= tol).all()


@pytest.mark.gpu
def test_fusion_plain_lattice(gpu_device, fusion_views):
    """The 40 x 36 x 44 lattice, trunc 0.2, six views.  Every sample whose decisions are not within 1e-4 of a threshold carries exactly
    the statement's update count and a value within the bound mesh_statement.fuse derives from fp32 rounding of the stated operation
    sequence (its docstring: rounding of the sample position, of z, of the tap position times the local texel differences, of d, averaged
    as the rule averages); at most 1 % of the samples may be left out."""
    from materialrefgs_amd import mesh
    org, sp = ms.ORG.astype(np.float32), ms.SPACING.astype(np.float32)
    trunc = np.float32(0.2)
    field, w = mesh.tsdf_fuse(_device_views(fusion_views, gpu_device), trunc, shape=ms.SHAPE, origin=org, spacing=sp, return_weight=True)
    x, pos_err = ms.plain_samples(org, sp, ms.SHAPE)
    st = ms.fuse(x, float(trunc), fusion_views, pos_err=pos_err)
    assert field.shape == ms.SHAPE
    _check_fusion("plain", field, w, st)
    assert (st["w"] > 1).mean() > 0.5 and st["tsdf"].min() < 0                # the input does exercise the rule: most samples updated, a surface inside
    # no debug output: the same field
    assert torch.equal(mesh.tsdf_fuse(_device_views(fusion_views, gpu_device), trunc, shape=ms.SHAPE, origin=org, spacing=sp), field)


@pytest.mark.gpu
def test_fusion_variants(gpu_device, fusion_views):
    """Contracted lattice with samples beyond the unit ball, an explicit point list, the bounded mode's texel validity, views of two
    sizes, and no view at all."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    views = _device_views(fusion_views, dev)
    # (a) contracted, N = 40, R = 1.4: |s| > 1 and the scaled trunc occur; the trunc factor 1 / (2 - min(|s|, 1.9)) amplifies the three
    # roundings of |s| by at most 1.9 / 0.1, so trunc is off by less than 64 * 2^-24 relative
    N, R = 40, np.float32(1.4)
    centre, radius = np.array([0.05, -0.02, 0.03], np.float32), np.float32(0.9)
    step = np.float32(2.0 * float(R) / (N - 1))
    voxel = np.float32(0.05)
    field, w = mesh.tsdf_fuse(views, 5 * float(voxel), shape=(N, N, N), origin=-R, spacing=step, contraction=(centre, radius), return_weight=True)
    s = -float(R) + float(step) * ms.lattice_index((N, N, N))
    mag = np.linalg.norm(s, axis=-1)
    trunc = np.full(len(s), float(np.float32(5 * float(voxel))))
    trunc[mag > 1] *= 1.0 / (2.0 - np.minimum(mag[mag > 1], 1.9))
    x = centre.astype(np.float64) + float(radius) * ms.uncontract(s)
    rel = (12.0 + 4.0 / np.maximum(np.abs(2.0 - mag), 1e-3)) * ms.EPS
    pos_err = rel[:, None] * np.abs(x - centre) + ms.EPS * np.abs(x)
    assert (mag > 1).mean() > 0.3
    with np.errstate(invalid="ignore", over="ignore"):
        st = ms.fuse(x, trunc, fusion_views, pos_err=pos_err, trunc_rel_err=64 * ms.EPS)
    _check_fusion("contracted", field, w, st)
    assert ((st["w"] > 1) & (mag > 1)).any()

    # (c) 1000 explicit points
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.8, 0.8, (1000, 3)).astype(np.float32)
    field, w = mesh.tsdf_fuse(views, 0.2, points=torch.from_numpy(pts).to(dev), return_weight=True)
    st = ms.fuse(pts.astype(np.float64), float(np.float32(0.2)), fusion_views)
    _check_fusion("points", field, w, st)

    # (b) texel validity: a zeroed rectangle in every map and a depth_trunc below the wall, so only taps wholly on the sphere count
    holed = []
    for M, d in fusion_views:
        d = d.copy()
        d[12:22, 18:30] = 0.0
        holed.append((M, d))
    org, sp = ms.ORG.astype(np.float32), ms.SPACING.astype(np.float32)
    field, w = mesh.tsdf_fuse(_device_views(holed, dev), 0.2, shape=ms.SHAPE, origin=org, spacing=sp, depth_trunc=3.0, return_weight=True)
    x, pos_err = ms.plain_samples(org, sp, ms.SHAPE)
    st = ms.fuse(x, float(np.float32(0.2)), holed, depth_trunc=float(np.float32(3.0)), pos_err=pos_err)
    free = ms.fuse(x, float(np.float32(0.2)), fusion_views, pos_err=pos_err)
    _check_fusion("validity", field, w, st)      # the cell choice is one more decision per view (fuse's docstring)
    assert (st["w"] < free["w"]).mean() > 0.3 and (st["w"] > 1).mean() > 0.05

    # views of two sizes in one table
    cams = _cameras(4, 28, 32, elevations=(20.0, -35.0), azimuth0=40.0)
    mixed = fusion_views[:3] + [(c.full_proj_transform.numpy().astype(np.float32), ms.analytic_depth(c, 28, 32)) for c in cams] + fusion_views[3:]
    field, w = mesh.tsdf_fuse(_device_views(mixed, dev), 0.2, shape=ms.SHAPE, origin=org, spacing=sp, return_weight=True)
    st = ms.fuse(x, float(np.float32(0.2)), mixed, pos_err=pos_err)
    _check_fusion("two sizes", field, w, st)

    # no view: the field is all 1
    field, w = mesh.tsdf_fuse([], 0.2, shape=(5, 4, 3), origin=0.0, spacing=1.0, return_weight=True, device=dev)
    assert (field == 1).all() and (w == 1).all() and field.shape == (5, 4, 3)

    with pytest.raises(TypeError, match="float32"):
        mesh.tsdf_fuse([(views[0][0], views[0][1].double())], 0.2, points=torch.zeros(4, 3, device=dev))


def _canon(tk):
    """Triangles as key triples rotated to start at their smallest key (the winding survives), sorted."""
    tk = np.asarray(tk)
    r = np.argmin(tk, axis=1)
    rot = np.stack([np.take_along_axis(tk, ((r + i) % 3)[:, None], axis=1)[:, 0] for i in range(3)], axis=1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


def _check_extraction(name, F, dev, slab_planes=None, origin=None, spacing=None):
    from materialrefgs_amd import mesh
    origin = ms.ORG.astype(np.float32) if origin is None else origin
    spacing = ms.SPACING.astype(np.float32) if spacing is None else spacing
    m = mesh.marching_tetrahedra(torch.from_numpy(F).to(dev), 0.0, origin, spacing, slab_planes=slab_planes)
    st = ms.marching_tetrahedra(F, 0.0, origin, spacing)
    v, t = m.vertices, m.triangles
    print(f"[{name}] V {len(v)} T {len(t)} (statement {len(st['vertices'])} {len(st['triangles'])})")
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == (len(st["vertices"]), 3) and t.shape == (len(st["triangles"]), 3)
    if len(t):
        assert t.min() >= 0 and t.max() < len(v)
        # vertex i is the i-th vertex by (owning lattice point, direction code): the order include/mrgs.h states; so keys[i] is its key
        got = _canon(st["keys"][t])
        assert np.array_equal(got, _canon(st["tkeys"]))              # the same triangle set, the same windings
        err = np.abs(v.astype(np.float64) - st["vertices"])
        tol = ms.vertex_tolerance(st)
        print(f"[{name}] worst vertex error / tolerance {np.max(err / tol):.3f}")
        assert (err <= tol).all()
    return m, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ms.KNOWN))
def test_extraction_known_fields(gpu_device, name):
    """The triangle set equals the statement's as triples of edge keys, windings included; V and T are equal; every vertex lies within
    mesh_statement.vertex_tolerance of the statement's (4 ulp of the larger end-point coordinate plus the edge's extent times 2^-22
    |F_a| / |F_b - F_a|: derivation in its docstring)."""
    m, st = _check_extraction(name, ms.known_field(name), gpu_device)
    assert (len(m.vertices), len(m.triangles)) == ms.KNOWN[name][1:3]


@pytest.mark.gpu
def test_extraction_edge_cases(gpu_device):
    """No crossing (an empty mesh), an axis of 2 points, a sphere that leaves the lattice (an open mesh: its boundary edges lie in exactly
    one triangle), and slabs of 16 and of 1 cube layers on the 40-plane axis (two and 38 slab boundaries crossed)."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    F = ms.known_field("sphere")
    m, _ = _check_extraction("no crossing", np.abs(F) + np.float32(0.1), dev)
    assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3)
    for axis in range(3):
        sl = [slice(None)] * 3
        sl[axis] = slice(18, 20)
        _check_extraction(f"axis {axis} of 2", np.ascontiguousarray(F[tuple(sl)]), dev)
    shifted = ms.field_sphere(ms.lattice_points(np.array([-0.79, -0.71, -0.87]), np.full(3, 0.04)), centre=(0.55, 0.1, -0.6)).astype(np.float32)
    m, st = _check_extraction("open", shifted, dev)
    und, directed = ms.edge_census(m.triangles.astype(np.int64))
    assert set(np.unique(und)) == {1, 2} and (directed == 1).all()
    base = mesh.marching_tetrahedra(torch.from_numpy(F).to(dev), 0.0, ms.ORG.astype(np.float32), ms.SPACING.astype(np.float32))
    for slab in (16, 1, 39, 1000):
        m, _ = _check_extraction(f"slab {slab}", F, dev, slab_planes=slab)
        assert np.array_equal(m.vertices, base.vertices) and np.array_equal(m.triangles, base.triangles)
    for name, Fx in (("torus slab 16", ms.known_field("torus")), ("open slab 16", shifted)):
        _check_extraction(name, Fx, dev, slab_planes=16)


@pytest.mark.gpu
def test_extraction_more_than_1024_blocks_in_one_slab(gpu_device):
    """66 x 64 x 64 points in a single slab are 1056 blocks of 256: the one-workgroup scan takes 1024 block sums a step, so the blocks of
    the last two planes get their offsets from a second step that needs the first one's totals.  The sphere leaves the lattice through
    those planes, so they own vertices and triangles."""
    shape, origin, spacing = (66, 64, 64), np.array([-0.651, -0.633, -0.627], np.float32), np.full(3, 0.02, np.float32)
    F = ms.field_sphere(ms.lattice_points(origin.astype(np.float64), spacing.astype(np.float64), shape), centre=(0.2, 0.05, -0.03)).astype(np.float32)
    _m, st = _check_extraction("66 x 64 x 64", F, gpu_device, origin=origin, spacing=spacing)
    beyond = 1024 * 256 * 8                                             # keys are lattice index * 8 + direction code
    assert (st["keys"] >= beyond).sum() > 100 and (st["tkeys"].min(axis=1) >= beyond).sum() > 100


@pytest.mark.gpu
def test_clusters_and_post_process(gpu_device):
    """Two spheres (radii 0.25 and 0.13) plus a blob of fewer than 50 triangles: cluster_to_keep = 1 keeps the large sphere, 2 keeps both
    spheres and drops the blob (the floor of 50), 1000 clamps to the three clusters and still drops the blob.  Survivors keep their order,
    no unreferenced vertex remains, every index is below V; labels equal scipy's components up to renaming."""
    from materialrefgs_amd import mesh
    dev = gpu_device
    p = ms.lattice_points(np.array([-0.79, -0.71, -0.87]), np.full(3, 0.04))
    blob = ms.field_sphere(p, centre=(-0.79 + 0.04 * 20 + 0.004, -0.71 + 0.04 * 30 - 0.003, -0.87 + 0.04 * 36 + 0.002), r=0.025)
    F = np.minimum(ms.field_two_spheres(p), blob).astype(np.float32)
    m, st = _check_extraction("two spheres and a blob", F, dev)
    v, t = m.vertices, m.triangles.astype(np.int64)
    ref_labels, ref_counts = ms.components(len(v), t)
    sizes = np.sort(ref_counts)
    assert len(sizes) == 3 and sizes[0] < 50 <= sizes[1] < sizes[2]
    labels, counts = mesh.cluster_triangles(m)
    labels, counts = labels.cpu().numpy(), counts.cpu().numpy()
    pairs = np.unique(np.stack([labels, ref_labels], axis=1), axis=0)
    assert len(pairs) == 3 and len(np.unique(pairs[:, 0])) == 3 and len(np.unique(pairs[:, 1])) == 3
    for lab, ref in pairs:
        assert lab == np.nonzero(ref_labels == ref)[0].min()        # a label is its component's smallest vertex index
        assert counts[lab] == ref_counts[ref]
    assert counts.sum() == len(t) and (counts > 0).sum() == 3
    for k, n_left in ((1, sizes[2]), (2, sizes[1] + sizes[2]), (1000, sizes[1] + sizes[2])):
        out = mesh.post_process_mesh(m, k)
        ev, et, _, _ = ms.post_process_mesh(v, t, k)
        assert len(out.triangles) == n_left == len(et)
        assert out.vertices.tobytes() == ev.tobytes()               # the surviving rows, in their order
        assert np.array_equal(out.triangles, et)
        assert out.triangles.max() < len(out.vertices) and len(np.unique(out.triangles)) == len(out.vertices)
    # the largest cluster under 50 triangles: everything goes, and the ray tracer says why it cannot take the result
    only_blob = mesh.marching_tetrahedra(torch.from_numpy(blob.astype(np.float32)).to(dev), 0.0, ms.ORG.astype(np.float32), ms.SPACING.astype(np.float32))
    assert 0 < len(only_blob.triangles) < 50
    empty = mesh.post_process_mesh(only_blob, 1)
    assert empty.vertices.shape == (0, 3) and empty.triangles.shape == (0, 3)
    from materialrefgs_amd.raytracing import RayTracer
    with pytest.raises(AssertionError, match="more than 8 triangles"):
        RayTracer(empty.vertices, empty.triangles)
