"""The mesh step of the training loop end to end (train_refnerf.py:1459-1472 after the import swap of INTEGRATION.md section 4c):
GaussianExtractor.reconstruction over twelve cameras with a stub `render` that returns the analytic depth of a sphere, TSDF fusion, mesh
extraction, post_process_mesh, RayTracer.  Every piece has its exact test in tests/test_mesh.py; this one is about the pieces meeting:
the mesh is the sphere as well as the float64 statement's own mesh of the same depth maps is, and the ray tracer built from it answers
rays with the sphere's distances."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_statement as ms

pytestmark = pytest.mark.gpu

H = W = 64
RADIUS = 0.5
DISTANCE, FOV = 1.4, math.radians(50.0)      # the sphere fills the view; the bounded lattice (side 2 x distance) stays at 71^3


def _cameras(dev):
    from materialrefgs_amd.camera import look_at_camera
    return [look_at_camera(30.0 * i, (-65.0, -20.0, 20.0, 65.0)[i % 4], DISTANCE, FOV, H, W).to(dev) for i in range(12)]


class _StubRender:
    """render(viewpoint_camera, pc, pipe=, bg_color=, opt=) -> the keys GaussianExtractor and the training loop read; surf_depth is the
    analytic depth of the sphere, 0 where a ray misses it (nothing was rendered there)."""

    def __init__(self):
        self.calls = 0

    def __call__(self, cam, pc, pipe=None, bg_color=None, opt=None):
        self.calls += 1
        assert not torch.is_grad_enabled()
        dev = cam.full_proj_transform.device
        depth = torch.from_numpy(ms.analytic_depth(SimpleNamespace(world_view_transform=cam.world_view_transform.cpu(), FoVx=cam.FoVx, FoVy=cam.FoVy),
                                                H, W, RADIUS, background=0.0)).to(dev)[None]
        zeros = torch.zeros(3, H, W, device=dev)
        return {"render": zeros, "rend_alpha": (depth > 0).float(), "rend_normal": zeros, "surf_normal": zeros, "surf_depth": depth}


def _ray_hits(vertices, triangles, o, d):
    """float64 distance of the first hit of each ray with the mesh (inf for none): Moeller-Trumbore over all pairs."""
    v0, v1, v2 = (vertices[triangles[:, k]] for k in range(3))
    e1, e2 = v1 - v0, v2 - v0
    best = np.full(len(o), np.inf)
    for i in range(len(o)):
        pv = np.cross(d[i], e2)
        det = (e1 * pv).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o[i] - v0
            u = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            v = (qv @ d[i]) * inv
            t = (e2 * qv).sum(1) * inv
        hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        if hit.any():
            best[i] = t[hit].min()
    return best


def _statement_mesh(views, lat):
    """The statement's own mesh of the same maps on the lattice the extractor used (its fp32 parameters), largest cluster only."""
    shape = lat["shape"]
    if lat["contraction"] is None:
        x, _ = ms.plain_samples(lat["origin"], np.full(3, lat["spacing"]), shape)
        st = ms.fuse(x, float(lat["trunc"]), views, depth_trunc=float(lat["depth_trunc"]), bound=False)
        mt = ms.marching_tetrahedra(st["tsdf"].reshape(shape), 0.0, lat["origin"], np.full(3, lat["spacing"]))
    else:
        centre, radius = lat["contraction"]
        s = float(lat["origin"]) + float(lat["spacing"]) * ms.lattice_index(shape)
        mag = np.linalg.norm(s, axis=-1)
        trunc = np.full(len(s), float(lat["trunc"]))
        trunc[mag > 1] *= 1.0 / (2.0 - np.minimum(mag[mag > 1], 1.9))
        x = centre.astype(np.float64) + float(radius) * ms.uncontract(s)
        st = ms.fuse(x, trunc, views, bound=False)
        mt = ms.marching_tetrahedra(st["tsdf"].reshape(shape), 0.0, np.full(3, float(lat["origin"])), np.full(3, float(lat["spacing"])),
                                    contraction=(centre.astype(np.float64), float(radius)))
    v, t, kept_v, _ = ms.post_process_mesh(mt["vertices"], mt["triangles"], 1)
    tol = ms.vertex_tolerance(mt)[kept_v].max()
    if lat["contraction"] is not None:       # inside the unit ball the map is centre + radius * v: the lattice tolerance scales, two more roundings
        tol = tol * float(lat["contraction"][1]) + 4 * 2.0 ** -23 * np.abs(v).max()
    return v, t, tol


def _check_sphere(name, mesh_out, stmt, cams, dev):
    """Vertex radii deviate from 0.5 by no more than the statement's own mesh deviates plus the vertex tolerance of
    mesh_statement.vertex_tolerance.  256 rays from the camera centres towards points within 0.3 of the sphere's centre hit at the
    analytic distance within what the statement's mesh deviates for the same rays (its flat triangles sag below the sphere by about
    edge^2 / 8r), plus 1.25 times the vertex tolerance (the rays meet the surface at cos >= 0.8) and 8 ulp of the ray length for the
    tracer's fp32 arithmetic.  Rays that pass the sphere report depth 10."""
    from materialrefgs_amd.raytracing import RayTracer
    sv, stri, tol = stmt
    v, t = mesh_out.vertices, mesh_out.triangles
    dev_stmt = np.abs(np.linalg.norm(sv, axis=1) - RADIUS).max()
    dev_gpu = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - RADIUS).max()
    print(f"[{name}] V {len(v)} T {len(t)} (statement {len(sv)} {len(stri)})  radial deviation {dev_gpu:.6e} (statement {dev_stmt:.6e}, tolerance {tol:.2e})")
    assert len(t) > 1000
    assert dev_gpu <= dev_stmt + tol
    rng = np.random.default_rng(5)
    centres = np.stack([c.camera_center.double().cpu().numpy() for c in cams])
    o = centres[np.arange(256) % len(cams)]
    aim = rng.standard_normal((256, 3))
    aim *= (0.3 * rng.uniform(0, 1, (256, 1)) ** (1 / 3)) / np.linalg.norm(aim, axis=1, keepdims=True)
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    od = (o * d).sum(1)
    analytic = -od - np.sqrt(od * od - ((o * o).sum(1) - RADIUS * RADIUS))
    dev_rays = np.abs(_ray_hits(sv, stri, o, d) - analytic).max()
    tracer = RayTracer(v, t)
    o32, d32 = torch.from_numpy(o.astype(np.float32)).to(dev), torch.from_numpy(d.astype(np.float32)).to(dev)
    _, _, depth = tracer.trace(o32, d32)
    err = np.abs(depth.double().cpu().numpy() - analytic).max()
    bound = dev_rays + 1.25 * tol + 8 * 2.0 ** -23 * (DISTANCE + RADIUS)
    print(f"[{name}] rays: worst |depth - analytic| {err:.6e}  (statement's mesh {dev_rays:.6e}, bound {bound:.6e})")
    assert err <= bound
    # rays past the sphere: aimed at points 0.8 from the centre, perpendicular to the line of sight
    side = np.cross(o, rng.standard_normal((256, 3)))
    side *= 0.8 / np.linalg.norm(side, axis=1, keepdims=True)
    dm = side - o
    dm /= np.linalg.norm(dm, axis=1, keepdims=True)
    _, _, miss = tracer.trace(o32, torch.from_numpy(dm.astype(np.float32)).to(dev))
    assert (miss == 10).all()


def test_extract_a_sphere_and_trace_it(gpu_device):
    from materialrefgs_amd import mesh
    dev = gpu_device
    cams = _cameras(dev)
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(5000, 3, generator=g)
    gaussians = SimpleNamespace(get_xyz=(RADIUS * xyz / xyz.norm(dim=1, keepdim=True)).to(dev))
    render = _StubRender()
    ex = mesh.GaussianExtractor(gaussians, render, SimpleNamespace(), bg_color=[0, 0, 0])
    ex.reconstruction(cams)
    assert render.calls == 12 and len(ex.depthmaps) == 12 and all(d.is_cuda and d.shape == (1, H, W) for d in ex.depthmaps)
    assert abs(ex.radius - DISTANCE) < 1e-5 and ex.center.abs().max() < 1e-5
    views = [(c.full_proj_transform.cpu().numpy(), d[0].cpu().numpy()) for c, d in zip(cams, ex.depthmaps)]

    raw = ex.extract_mesh_bounded(voxel_size=0.04, sdf_trunc=0.2, depth_trunc=2 * ex.radius)
    lattice = ex.last_lattice
    bounded = mesh.post_process_mesh(raw, 1)
    assert len(bounded.triangles) < len(raw.triangles)              # the shell behind the truncation band is a cluster of its own, and goes
    _check_sphere("bounded", bounded, _statement_mesh(views, lattice), cams, dev)

    raw_u = ex.extract_mesh_unbounded(resolution=64)
    lattice_u = ex.last_lattice
    assert lattice_u["contraction"] is not None and lattice_u["shape"] == (64, 64, 64)
    _check_sphere("unbounded", mesh.post_process_mesh(raw_u, 1), _statement_mesh(views, lattice_u), cams, dev)

    # a second reconstruction after clean(): the same mesh, nothing carried over
    ex.clean()
    assert ex.depthmaps == [] and ex.viewpoint_stack == []
    ex.reconstruction(cams)
    again = mesh.post_process_mesh(ex.extract_mesh_bounded(voxel_size=0.04, sdf_trunc=0.2, depth_trunc=2 * ex.radius), 1)
    assert torch.equal(again.vertices_device, bounded.vertices_device) and torch.equal(again.triangles_device, bounded.triangles_device)
    assert render.calls == 24
