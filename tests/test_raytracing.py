"""Mesh ray queries: host-built hierarchy (CPU checks) and GPU traversal vs the brute-force oracle.

The bar is EXACT, for the closest-hit query (depth and position bit for bit) and for the fused visibility (every pixel, none left
out), for three reasons:
  * csrc/mrgs_bvh.hip is compiled with -ffp-contract=off: no multiply-add is fused, every float32 operation is the one written;
  * its sqrtf and / are the correctly rounded ones, so numpy float32 reproduces each intermediate (oracle/trace_oracle.py for the
    triangle test, tests/visibility_statement.py for the mirror-ray set-up);
  * the hierarchy only prunes, and conservatively (padded boxes, widened slab test): the answer is the brute-force minimum over all
    triangles, whatever the tree looks like.
An allowance of "a few silhouette pixels" belongs only where the other side builds its rays with different arithmetic (the torch
sequence kept in test_fused_visibility_matches_traced_mirror_rays, the float64 checkers of tests/test_render_e2e.py).

The deepest supported walk (test_trace_deepest_supported_walk: 4**10 + 1 triangles, every box entered by each of 64 rays) was measured
on an MI355X on 2026-10-21: 0.50 s for the first launch, 0.43 s for the second.
"""
import ctypes
import functools
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import trace_oracle  # noqa: E402
import visibility_statement as vs  # noqa: E402


from materialrefgs_amd.synthetic import sphere_mesh  # noqa: E402


def _constant(name):
    with open(os.path.join(ROOT, "materialrefgs_amd", "csrc", "mrgs_bvh.hip")) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


BVH_LEAF, BVH_STACK = _constant("BVH_LEAF"), _constant("BVH_STACK")
BVH_EMPTY = 0x7FFFFFFF
BVH_LEVELS = (BVH_STACK - 1) // 3                  # inner levels the LDS stack has room for: three pushes per level


def scene(seed=0, n_lat=16, n_lon=24):
    """Bumpy unit sphere + a big ground quad grid + a small inner sphere: hits, misses, grazing rays, occlusion."""
    v1, t1 = sphere_mesh(n_lat, n_lon, 1.0, 0.03, seed)
    v2, t2 = sphere_mesh(6, 8, 0.3, 0.0, seed + 1)
    v2 = v2 + np.array([1.8, 0.2, 0.1], dtype=np.float32)
    g = np.linspace(-3, 3, 9).astype(np.float32)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    v3 = np.stack([gx, gy, np.full_like(gx, -1.2)], -1).reshape(-1, 3)
    t3 = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = i * 9 + j, i * 9 + j + 1, (i + 1) * 9 + j, (i + 1) * 9 + j + 1
            t3 += [(a, c, b), (b, c, d)]                        # normal +z
    t3 = np.asarray(t3, dtype=np.int32)
    v = np.concatenate([v1, v2, v3]).astype(np.float32)
    t = np.concatenate([t1, t2 + len(v1), t3 + len(v1) + len(v2)]).astype(np.int32)
    return v, t


def rays(n, seed=0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)).astype(np.float32)
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 4.0, size=(n, 1))).astype(np.float32)
    target = rng.normal(size=(n, 3)).astype(np.float32) * 0.8
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    # special rays: axis-parallel (zero direction components), origins on the surface, rays from inside (back faces only)
    o[:8] = np.array([[3, 0, 0], [0, 3, 0], [0, 0, 3], [-3, 0, 0], [0.5, 0.5, 3], [0, 0, 0], [0, 0, 0], [0.1, 0.1, -1.2]], dtype=np.float32)
    d[:8] = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [0, 0, -1], [0, 0, 1], [-1, 0, 0], [0, 0, -1]], dtype=np.float32)
    return o, d


def _lib():
    from materialrefgs_amd import _lib as L
    return L


def _build(v, t):
    L = _lib()
    lib = L.lib()
    nbytes = lib.mrgs_bvh_bytes(len(t))
    blob = np.zeros(nbytes, dtype=np.uint8)
    rc = lib.mrgs_bvh_build(ctypes.c_void_p(v.ctypes.data), len(v), ctypes.c_void_p(t.ctypes.data), len(t),
                            ctypes.c_void_p(blob.ctypes.data), nbytes)
    return rc, blob


def _views(blob, n):
    cap = n // 3 + 2
    align = lambda x: (x + 255) // 256 * 256   # noqa: E731
    tris_off = align(cap * 128)
    perm_off = align(tris_off + n * 48)
    nodes = blob[:cap * 128].view(np.float32).reshape(cap, 32)
    codes = blob[:cap * 128].view(np.int32).reshape(cap, 32)[:, 24:28]
    rec = blob[tris_off:tris_off + n * 48].view(np.float32).reshape(n, 12)
    perm = blob[perm_off:perm_off + n * 4].view(np.int32)
    return nodes, codes, rec, perm


# ---------------------------------------------------------------- CPU: the host-side build
@pytest.mark.parametrize("n_lat,n_lon", [(3, 4), (16, 24), (40, 60)])
def test_bvh_build_partitions_every_triangle_and_boxes_enclose(n_lat, n_lon):
    v, t = scene(1, n_lat, n_lon)
    rc, blob = _build(v, t)
    assert rc == 0
    n = len(t)
    nodes, codes, rec, perm = _views(blob, n)
    assert sorted(perm.tolist()) == list(range(n))                      # a permutation: every triangle exactly once
    a = v[t[perm, 0]]
    np.testing.assert_array_equal(rec[:, 0:3], a)
    np.testing.assert_array_equal(rec[:, 3:6], v[t[perm, 1]] - a)
    np.testing.assert_array_equal(rec[:, 6:9], v[t[perm, 2]] - a)
    seen = np.zeros(n, dtype=np.int32)
    max_depth = 0

    def walk(node, lo, hi, depth):
        nonlocal max_depth
        max_depth = max(max_depth, depth)
        for c in range(4):
            code = int(codes[node, c])
            if code == 0x7FFFFFFF:
                continue
            clo = nodes[node, [0 + c, 4 + c, 8 + c]]
            chi = nodes[node, [12 + c, 16 + c, 20 + c]]
            assert np.all(clo >= lo - 1e-4) and np.all(chi <= hi + 1e-4)          # nested (up to the padding)
            if code < 0:
                first, cnt = (~code) >> 3, ((~code) & 7) + 1
                assert cnt <= 4
                seen[first:first + cnt] += 1
                tv = v[t[perm[first:first + cnt]]].reshape(-1, 3)
                assert np.all(tv >= clo) and np.all(tv <= chi)                    # leaf box encloses its triangles
            else:
                walk(code, clo, chi, depth + 1)

    walk(0, np.full(3, -np.inf), np.full(3, np.inf), 1)
    assert np.all(seen == 1)
    assert 3 * max_depth + 1 <= 32


def test_bvh_build_rejects_bad_input():
    v, t = scene(0, 3, 4)
    L = _lib()
    lib = L.lib()
    bad = t.copy()
    bad[5, 1] = len(v)                                                   # vertex index out of range
    rc, _ = _build(v, bad)
    assert rc == 1
    blob = np.zeros(64, dtype=np.uint8)
    rc = lib.mrgs_bvh_build(ctypes.c_void_p(v.ctypes.data), len(v), ctypes.c_void_p(t.ctypes.data), len(t),
                            ctypes.c_void_p(blob.ctypes.data), 64)
    assert rc == L.MRGS_E_WORKSPACE
    assert lib.mrgs_bvh_bytes(0) == 0


def test_trace_oracle_known_answers():
    """One triangle in the plane z = 0, normal +z: hit from above, back face from below, miss outside, t >= 10 dropped."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    t = np.array([[0, 1, 2]], dtype=np.int32)
    o = np.array([[0.25, 0.25, 2], [0.25, 0.25, -2], [2, 2, 2], [0.25, 0.25, 11], [0.25, 0.25, 0.0]], dtype=np.float32)
    d = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1]], dtype=np.float32)
    pos, nrm, depth, ids = trace_oracle.trace(v, t, o, d)
    np.testing.assert_array_equal(depth, np.array([2, 10, 10, 10, 0], dtype=np.float32))
    np.testing.assert_array_equal(ids, [0, -1, -1, -1, 0])
    np.testing.assert_array_equal(nrm[0], [0, 0, 1])
    np.testing.assert_array_equal(nrm[1], [0, 0, 0])
    np.testing.assert_array_equal(pos[0], [0.25, 0.25, 0])
    np.testing.assert_array_equal(pos[1], [0.25, 0.25, 8])               # a miss still advances by MAX_DIST (bvh.cu:706-708)


def _inner_levels(codes):
    """Number of inner levels of a built hierarchy (the root is level 1), walked level by level from the child codes."""
    frontier, levels = np.zeros(1, dtype=np.int64), 0
    while frontier.size:
        levels += 1
        ch = codes[frontier].reshape(-1)
        frontier = ch[(ch >= 0) & (ch != BVH_EMPTY)].astype(np.int64)
    return levels


def test_bvh_build_stack_bound_both_sides():
    """The LDS traversal stack holds BVH_STACK entries and a walk pushes up to three per inner level, so the build accepts
    3 * levels + 1 <= BVH_STACK.  With BVH_LEAF triangles per leaf and four children per node the largest accepted mesh has
    BVH_LEAF ** (BVH_LEVELS + 1) triangles (4 194 304 with the shipped constants, measured), one more is MRGS_E_UNSUPPORTED.
    The triangles are index triples into six vertices: all that counts here is their number."""
    assert BVH_LEAF == 4                                                 # the boundary below is that of a 4-ary tree with 4-triangle leaves
    L = _lib()
    lib = L.lib()
    n_max = BVH_LEAF ** (BVH_LEVELS + 1)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [0.5, 0.2, 1], [0.1, 0.9, 0.3]], dtype=np.float32)
    rng = np.random.default_rng(0)
    t = np.ascontiguousarray(np.argsort(rng.random((n_max + 1, 6)), axis=1)[:, :3].astype(np.int32))   # three distinct vertices each
    nbytes = lib.mrgs_bvh_bytes(n_max + 1)
    blob = np.zeros(nbytes, dtype=np.uint8)

    def build(n):
        return lib.mrgs_bvh_build(ctypes.c_void_p(v.ctypes.data), len(v), ctypes.c_void_p(t.ctypes.data), n,
                                  ctypes.c_void_p(blob.ctypes.data), nbytes)
    assert build(n_max + 1) == L.MRGS_E_UNSUPPORTED
    assert build(n_max) == L.MRGS_OK
    _, codes, _, perm = _views(blob, n_max)
    assert _inner_levels(codes) == BVH_LEVELS                            # the deepest inner node sits exactly at the bound
    assert np.array_equal(np.sort(perm), np.arange(n_max, dtype=np.int32))


# ---------------------------------------------------------------- CPU: the visibility statement and the inputs of the GPU cases
VIS_SIZES = ((120, 160), (7, 31), (9, 33), (41, 67))                    # full tiles; a partial tile; one pixel past a tile each way; ragged


@functools.lru_cache(maxsize=None)
def _vis_mesh():
    return scene(3, 24, 36)


def _vis_camera(H, W):
    from materialrefgs_amd.synthetic import orbit_camera
    cam = orbit_camera(2, H, W)
    K = np.asarray(cam.HWK[2], dtype=np.float32)
    return cam, K, cam.R.float().numpy(), cam.T.float().numpy()


@functools.lru_cache(maxsize=None)
def _vis_case(H, W):
    """Inputs of one visibility case, numpy float32 on the CPU, and the statement's answer for them: (normal [H,W,3], alpha [H,W],
    surf_depth [H,W], statement [H,W], blocked share of the traced pixels).  The surface is the first hit of the pixel rays against the
    mesh itself (brute force), the depth just in front of it, the normal the face normal plus noise, alpha 0 on a fifth.  On top of
    that five groups of pixels, spread over the image by a multiplicative hash of the pixel index: negative alpha; a zero normal (the
    mirror direction degenerates to the view ray); surf_depth 0 (origin at the camera); a grazing normal, n . w = 1e-4; a surface point
    behind the camera-facing mesh (depth x 1.05)."""
    v, t = _vis_mesh()
    _, K, R, T = _vis_camera(H, W)
    Kinv = vs.kinv_f32(K)
    ro, c = vs.camera_rays(H, W, Kinv, R, T)
    _, nrm, t_hit, _ = trace_oracle.trace(v, t, np.broadcast_to(ro, (H * W, 3)), c.reshape(-1, 3))      # t runs along the un-normalised ray
    rng = np.random.default_rng(11 + H * W)
    hit = t_hit < 10
    sd = (np.where(hit, t_hit, np.float32(3.0)) * np.float32(0.999)).astype(np.float32)
    rnd = rng.standard_normal((H * W, 3)).astype(np.float32)
    n = np.where(hit[:, None], nrm, rnd / np.linalg.norm(rnd, axis=1, keepdims=True))
    n = n + np.float32(0.2) * rng.standard_normal((H * W, 3)).astype(np.float32)
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    alpha = ((rng.random(H * W) > 0.2) * rng.random(H * W)).astype(np.float32)
    group = (np.arange(H * W) * 7919) % 13
    alpha[group == 0] = -0.5
    alpha[(group >= 1) & (group <= 4) & (alpha <= 0)] = 0.5             # the groups below are traced
    n[group == 1] = 0.0
    sd[group == 2] = 0.0
    w = -c.reshape(-1, 3) / np.linalg.norm(c.reshape(-1, 3), axis=1, keepdims=True)
    side = np.cross(w, np.array([0.3, -0.5, 0.8], dtype=np.float32))
    graze = side / np.linalg.norm(side, axis=1, keepdims=True) + np.float32(1e-4) * w
    n[group == 3] = graze[group == 3].astype(np.float32)
    sd[group == 4] = (sd[group == 4] * np.float32(1.05)).astype(np.float32)
    normal, alpha, sd = n.reshape(H, W, 3).astype(np.float32), alpha.reshape(H, W), sd.reshape(H, W)
    stmt = vs.visibility(v, t, H, W, Kinv, R, T, normal, alpha, sd)
    traced = alpha > 0
    assert (alpha == 0).any() and (alpha < 0).any() and bool((stmt[~traced] == 1).all())
    blocked = float((stmt[traced] == 0).mean())
    for a in (normal, alpha, sd, stmt):
        a.setflags(write=False)
    return normal, alpha, sd, stmt, blocked


@functools.lru_cache(maxsize=None)
def _vis_case_one_pixel(want_blocked):
    """The 1 x 1 image: its single mirror ray starts 3 units along the pixel ray; the normal is the first of a fixed random sequence
    for which the statement reports the wanted outcome."""
    v, t = _vis_mesh()
    _, K, R, T = _vis_camera(1, 1)
    rng = np.random.default_rng(5)
    for _ in range(64):
        n = rng.standard_normal(3).astype(np.float32)
        normal = (n / np.linalg.norm(n)).astype(np.float32).reshape(1, 1, 3)
        alpha, sd = np.full((1, 1), 0.7, dtype=np.float32), np.full((1, 1), 3.0, dtype=np.float32)
        stmt = vs.visibility(v, t, 1, 1, vs.kinv_f32(K), R, T, normal, alpha, sd)
        if bool(stmt[0, 0] == 0) == want_blocked:
            return normal, alpha, sd, stmt, float(stmt[0, 0] == 0)
    raise AssertionError("no normal with the wanted outcome")


def test_visibility_cases_exercise_both_outcomes():
    """What the GPU cases assume of their inputs, checked without a GPU: both outcomes at every size, and the special groups present."""
    for H, W in VIS_SIZES[1:]:
        normal, alpha, sd, stmt, blocked = _vis_case(H, W)
        assert 0.02 < blocked < 0.98, (H, W, blocked)
        assert (sd == 0).any() and (np.abs(normal).sum(-1) == 0).any()
    assert _vis_case_one_pixel(True)[3][0, 0] == 0 and _vis_case_one_pixel(False)[3][0, 0] == 1


def test_visibility_statement_is_the_reference_sequence_up_to_rounding():
    """tests/visibility_statement.py (the kernel's float32 operations) against the reference's sequence (utils/refl_utils.py:379-391)
    in float64 on the 120 x 160 case: directions within 1e-6, origins within 1e-6 of the largest coordinate, and every pixel whose
    visibility differs is a near-tie in float64 -- for each triangle that one side accepts and the other does not, one of the
    quantities the triangle test compares with a threshold (u, v, 1 - u - v, dn, t - 10) lies within 1e-4 of it."""
    H, W = VIS_SIZES[0]
    v, t = _vis_mesh()
    _, K, R, T = _vis_camera(H, W)
    normal, alpha, sd, stmt, blocked = _vis_case(H, W)
    assert 0.02 < blocked < 0.98, blocked
    o32, d32, traced = vs.mirror_rays(H, W, vs.kinv_f32(K), R, T, normal, alpha, sd)
    o64, d64 = vs.reference_rays_f64(H, W, K, R, T, normal, sd)
    d_err = float(np.abs(d32[traced] - d64[traced]).max())
    o_err = float(np.abs(o32[traced] - o64[traced]).max())
    o_scale = float(np.abs(o64[traced]).max())
    print(f"directions differ by {d_err:.3e}, origins by {o_err:.3e} at a largest coordinate of {o_scale:.3f}")
    assert d_err <= 1e-6, d_err
    assert o_err <= 1e-6 * o_scale, (o_err, o_scale)
    # the float64 triangle test on the float64 rays, brute force; the float32 side is the statement
    pix = np.argwhere(traced)
    O, D, o32t, d32t = o64[traced], d64[traced], o32[traced], d32[traced]
    free32 = stmt[traced] == 1
    n_diff = 0
    for s in range(0, len(O), 512):
        slack, tt = vs.triangle_slack_f64(v, t, O[s:s + 512], D[s:s + 512])
        acc = (slack[..., :3] >= 0).all(-1) & (slack[..., 0] <= 1) & (slack[..., 3] > 0) & (slack[..., 4] > 0) & (tt >= 0)
        free64 = ~acc.any(1)
        for k in np.nonzero(free64 != free32[s:s + 512])[0]:
            n_diff += 1
            where = tuple(pix[s + k])
            if free64[k]:                   # float32 blocked: the triangle it reports is rejected in float64, but by a hair only
                _, _, _, j = trace_oracle.trace(v, t, o32t[s + k:s + k + 1], d32t[s + k:s + k + 1])
                assert j[0] >= 0
                worst = min(float(slack[k, j[0]].min()), float(tt[k, j[0]]))
                assert -1e-4 <= worst < 0, (where, int(j[0]), slack[k, j[0]].tolist(), float(tt[k, j[0]]))
            else:                           # float64 blocked: every triangle it accepts sits within 1e-4 of one of its thresholds
                for j in np.nonzero(acc[k])[0]:
                    assert float(slack[k, j].min()) <= 1e-4, (where, int(j), slack[k, j].tolist())
    print(f"float32 and float64 visibility differ at {n_diff} of {len(O)} traced pixels, every one a near-tie")


# ---------------------------------------------------------------- GPU: traversal vs brute force
def _compare_with_oracle(v, t, o, d, pos, nrm, depth, ids):
    """Depth and position bit-equal; ids equal or an exact tie proven by hit_time; normals equal where the ids agree."""
    rpos, rnrm, rdepth, rids = trace_oracle.trace(v, t, o, d)
    np.testing.assert_array_equal(depth, rdepth)                         # bit-exact closest distance
    np.testing.assert_array_equal(pos, rpos)
    same = ids == rids
    if not same.all():                                                   # only exact ties may pick another triangle
        idx = np.nonzero(~same)[0]
        tt = trace_oracle.hit_time(v, t, o[idx], d[idx], ids[idx])
        np.testing.assert_array_equal(tt, rdepth[idx])
    np.testing.assert_array_equal(nrm[same], rnrm[same])
    return depth, ids


def _check_against_oracle(v, t, o, d, inplace=False):
    from materialrefgs_amd.raytracing import RayTracer
    rt = RayTracer(v, t)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    pos, nrm, depth, ids = rt.trace(to.clone(), td.clone(), inplace=inplace, return_faceids=True)
    pos, nrm, depth, ids = pos.cpu().numpy(), nrm.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()
    return _compare_with_oracle(v, t, o, d, pos, nrm, depth, ids)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_trace_matches_brute_force(inplace):
    v, t = scene(0)
    o, d = rays(6000, 1)
    depth, ids = _check_against_oracle(v, t, o, d, inplace)
    assert (depth < 10).mean() > 0.3 and (depth >= 10).mean() > 0.02     # the case has both hits and misses
    assert depth[5] >= 10 and depth[6] >= 10                             # rays from inside the sphere: back faces only


@pytest.mark.gpu
def test_trace_reflection_rays_from_the_surface():
    """The way the shading pass uses it (utils/refl_utils.py:381-391): origins on the mesh, mirrored view directions."""
    v, t = scene(2, 24, 36)
    rng = np.random.default_rng(5)
    f = rng.integers(0, len(t), size=4000)
    w = rng.dirichlet([1, 1, 1], size=4000).astype(np.float32)
    p = (v[t[f, 0]] * w[:, :1] + v[t[f, 1]] * w[:, 1:2] + v[t[f, 2]] * w[:, 2:]).astype(np.float32)
    n = np.cross(v[t[f, 1]] - v[t[f, 0]], v[t[f, 2]] - v[t[f, 0]])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    cam = np.array([0, -4, 1.5], dtype=np.float32)
    wo = cam - p
    wo = wo / np.linalg.norm(wo, axis=1, keepdims=True)
    r = (2 * n * (n * wo).sum(1, keepdims=True) - wo).astype(np.float32)
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
    _check_against_oracle(v, t, p, r)


@pytest.mark.gpu
def test_trace_large_mesh_properties():
    """~1 M triangles, 640 000 rays (the C4 mesh size, C2 image size): identities that need no oracle."""
    from materialrefgs_amd.raytracing import RayTracer
    v, t = sphere_mesh(700, 720, 1.0, 0.0)
    assert len(t) > 1_000_000
    rt = RayTracer(v, t)
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.nn.functional.normalize(torch.randn(640_000, 3, device="cuda", generator=g), dim=-1)
    o = -3.0 * d                                                          # towards the centre from radius 3
    pos, nrm, depth, ids = rt.trace(o, d, return_faceids=True)
    polar = d[:, 2].abs() > 0.9995                                        # the open caps at the poles
    hit = depth < 10
    missed = (~hit) & (~polar)
    assert float(missed.float().mean()) < 1e-3                            # the reference's edge test is not watertight: a few rays slip through
    # a sample of rays (all of the slipped ones first) against the brute-force oracle at full mesh size
    pick = torch.cat([torch.nonzero(missed)[:16, 0], torch.arange(0, 640_000, 13_337, device="cuda")]).cpu().numpy()
    _, _, rdepth, rids = trace_oracle.trace(v, t, o[pick].cpu().numpy(), d[pick].cpu().numpy(), chunk=8)
    np.testing.assert_array_equal(depth[pick].cpu().numpy(), rdepth)
    assert float((depth[hit] - 2.0).abs().max()) < 2e-3                   # unit sphere seen from radius 3 (faceted)
    assert float((pos[hit].norm(dim=-1) - 1.0).abs().max()) < 2e-3
    assert float((nrm[hit] * (-d[hit])).sum(-1).min()) > 0.99             # outward normals face the ray origin
    tv = torch.from_numpy(v).cuda()[torch.from_numpy(t).cuda()[ids[hit].long()].long()]        # [n,3,3]
    nn = torch.linalg.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    assert float(((pos[hit] - tv[:, 0]) * torch.nn.functional.normalize(nn, dim=-1)).sum(-1).abs().max()) < 1e-4   # hit lies in its triangle's plane
    # rays leaving the sphere from inside see only back faces: all miss
    _, _, depth2 = rt.trace(torch.zeros_like(d), d)
    assert bool((depth2 >= 10).all())


def _camera_rays_unnormalized(H, W, K, R, T):
    """sample_camera_rays_unnormalize (utils/refl_utils.py:75-93) restated with torch fp32 ops for the test."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = torch.tensor(np.dot(xy1, np.linalg.inv(K.astype(np.float32)).T)).to(R.device)
    Rt = R.T
    rays_o = (-Rt.T @ T.unsqueeze(-1)).flatten()
    pixel_world = (pixel_camera - T[None, None]).reshape(-1, 3) @ Rt
    return (pixel_world - rays_o[None]).reshape(H, W, 3), rays_o


@pytest.mark.gpu
def test_fused_visibility_matches_traced_mirror_rays():
    """mrgs_bvh_visibility on maps made on the device: exactly the statement (tests/visibility_statement.py) at every pixel, and beside it
    the reference's sequence (utils/refl_utils.py:379-391) executed with torch ops + RayTracer.trace, whose rays round differently."""
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.synthetic import orbit_camera
    H, W = 120, 160
    v, t = scene(3, 24, 36)
    rt = RayTracer(v, t)
    cam = orbit_camera(2, H, W).to("cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    rays_cam, rays_o = _camera_rays_unnormalized(H, W, np.asarray(cam.HWK[2]), cam.R.float(), cam.T.float())
    # surface points = first hit of the pixel rays against the mesh itself; z-depth = t (rays_cam has unit camera-space z)
    _, nrm, t_hit = rt.trace(rays_o.expand(H * W, 3).contiguous(), rays_cam.reshape(-1, 3).contiguous())
    # the tracer wants unit directions for distances, but t is a parameter along rays_cam here, which is what surf_depth multiplies
    hit = (t_hit < 10).view(H, W)
    surf_depth = torch.where(hit, t_hit.view(H, W), torch.full((H, W), 3.0, device="cuda")).view(1, H, W) * 0.999   # just in front of the surface
    normal = torch.where(hit[..., None], nrm.view(H, W, 3), torch.nn.functional.normalize(torch.randn(H, W, 3, device="cuda", generator=g), dim=-1))
    normal = torch.nn.functional.normalize(normal + 0.2 * torch.randn(H, W, 3, device="cuda", generator=g), dim=-1)
    alpha = (torch.rand(H, W, 1, device="cuda", generator=g) > 0.2).float() * torch.rand(H, W, 1, device="cuda", generator=g)
    vis = rt.visibility(cam.HWK, cam.R, cam.T, normal, alpha, surf_depth)
    # reference sequence
    mask = (alpha > 0)[..., 0]
    w_o = torch.nn.functional.normalize(-rays_cam, dim=-1)
    refl = torch.nn.functional.normalize(2 * normal * (w_o * normal).sum(-1, keepdim=True) - w_o, dim=-1)
    inter = rays_o + surf_depth.permute(1, 2, 0) * rays_cam
    _, _, depth = rt.trace(inter[mask], refl[mask])
    ref = torch.ones_like(alpha)
    ref[mask] = (depth >= 10).float().unsqueeze(-1)
    assert vis.shape == (H, W, 1)
    assert bool((vis[~mask] == 1).all())
    # the kernel's own operations restated in numpy float32 on exactly these maps: every pixel, no allowance
    stmt = vs.visibility(v, t, H, W, vs.kinv_f32(np.asarray(cam.HWK[2])), cam.R.float().cpu().numpy(), cam.T.float().cpu().numpy(),
                         normal.cpu().numpy(), alpha.cpu().numpy(), surf_depth.cpu().numpy())
    assert torch.equal(vis.cpu()[..., 0], torch.from_numpy(stmt))
    mism = float((vis != ref).float().mean())
    assert mism < 2e-3, mism                                            # torch builds these rays with other roundings: silhouettes only
    blocked = float((ref[mask] == 0).float().mean())
    assert 0.02 < blocked < 0.98, blocked                               # the case exercises both outcomes


@pytest.mark.gpu
def test_render_surfel_indirect_branch():
    """opt.indirect with a mesh tracer: reference keys, visibility in {0,1}, blend formula, gradients to the indirect SH."""
    from types import SimpleNamespace
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.renderer import SurfelModel, render_surfel
    from materialrefgs_amd.shading import EnvLight
    from materialrefgs_amd.synthetic import make_shell_scene, orbit_camera
    dev = "cuda"
    P, H, W = 3000, 96, 128
    sc = make_shell_scene(P, S=0, seed=1, radius_px=6.0, image_size=128).to(dev)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)   # noqa: E731
    env = EnvLight(device=dev, trainable=True)
    with torch.no_grad():
        env.base.copy_(rnd(6, 128, 128, 3))
    env.build_mips()
    inv_sig = lambda x: torch.log(x / (1 - x))   # noqa: E731
    pc = SurfelModel(sc.means3D.clone(), torch.log(sc.scales), sc.rotations.clone(), inv_sig(sc.opacities.clamp(1e-4, 1 - 1e-4)),
                     sc.shs[:, :1].clone(), sc.shs[:, 1:].clone(), refl_strength=rnd(P, 1), roughness=rnd(P, 1), ori_color=rnd(P, 3),
                     indirect_dc=rnd(P, 1, 3).abs() * 0.5, indirect_rest=rnd(P, 15, 3) * 0.01, envmap=env)
    for p_ in pc.parameters():
        p_.requires_grad_(True)
    # the shell scene lives on the unit sphere: a slightly larger inward-facing... the tracer culls back faces, so use an
    # outward-facing sphere of radius 0.9 plus a blocker sphere off to the side
    v1, t1 = sphere_mesh(24, 36, 0.9)
    v2, t2 = sphere_mesh(12, 16, 0.8)
    v2 = v2 + np.array([0.0, 2.2, 0.0], dtype=np.float32)
    pc.ray_tracer = RayTracer(np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)]))
    cam = orbit_camera(1, H, W).to(dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    out = render_surfel(cam, pc, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=True))
    for k in ("render", "specular_map", "visibility", "indirect_light", "direct_light", "indirect_color", "specular_weight", "surf_depth"):
        assert k in out, k
    vis = out["visibility"]
    assert vis.shape == (1, H, W) and bool(((vis == 0) | (vis == 1)).all())
    assert 0.0 < float((vis == 0).float().mean()) < 1.0
    alpha = out["rend_alpha"]
    light = out["direct_light"] * vis + (1 - vis) * out["indirect_light"]
    want = light * alpha * out["specular_weight"].permute(2, 0, 1)
    assert torch.allclose(out["specular_map"], want, atol=1e-6)
    out["render"].mean().backward()
    assert pc._indirect_dc.grad is not None and float(pc._indirect_dc.grad.abs().sum()) > 0
    assert env.base.grad is not None and torch.isfinite(env.base.grad).all()


@pytest.mark.gpu
def test_indirect_blend_kernel_matches_torch_ops():
    """mrgs_indirect_blend_* against the reference's expressions (utils/refl_utils.py:393-401) evaluated with torch autograd."""
    from materialrefgs_amd.shading import _IndirectBlend
    H, W = 37, 53
    g = torch.Generator(device="cuda").manual_seed(4)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g)   # noqa: E731
    direct, weight = r(3, H, W).requires_grad_(True), r(H, W, 3).requires_grad_(True)
    feat = r(8, H, W).requires_grad_(True)
    alpha_chw = r(1, H, W).requires_grad_(True)
    vis = (r(H, W, 1) > 0.4).float()
    indirect, alpha = feat[5:8].permute(1, 2, 0), alpha_chw.permute(1, 2, 0)            # strided views, as render_surfel passes them
    spec, ic = _IndirectBlend.apply(direct, weight, indirect, alpha, vis)
    light = direct.permute(1, 2, 0) * vis + (1 - vis) * indirect
    spec_ref = (light * alpha * weight).permute(2, 0, 1)
    ic_ref = ((1 - vis) * indirect * alpha * weight).permute(2, 0, 1)
    torch.testing.assert_close(spec, spec_ref, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(ic, ic_ref, rtol=1e-6, atol=1e-7)
    gs, gi = r(3, H, W), r(3, H, W)
    got = torch.autograd.grad([spec, ic], [direct, weight, feat, alpha_chw], [gs, gi])
    want = torch.autograd.grad([spec_ref, ic_ref], [direct, weight, feat, alpha_chw], [gs, gi])
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_trace_tiny_and_degenerate_meshes():
    """Nine triangles (the reference's minimum is > 8) incl. zero-area and duplicated ones, rays parallel to faces, zero rays."""
    from materialrefgs_amd.raytracing import RayTracer
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5], [2, 2, 2]], dtype=np.float32)
    t = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [8, 8, 8], [9, 9, 1], [0, 2, 1]], dtype=np.int32)
    o, d = rays(500, 3)
    o[:4] = np.array([[0.25, 0.25, 3], [0.25, 0.25, -3], [-1, 0.5, 0.0], [0.5, 0.5, 0.5]], dtype=np.float32)
    d[:4] = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [0, 0, 1]], dtype=np.float32)        # ray 2 runs inside the plane z = 0
    _check_against_oracle(v, t, o * 0.7, d)
    rt = RayTracer(v, t)
    pos, nrm, depth = rt.trace(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"))
    assert pos.shape == (0, 3) and depth.shape == (0,)
    with pytest.raises(AssertionError):
        RayTracer(v, t[:8])


# ---------------------------------------------------------------- GPU: the fused visibility, exact, every pixel
def _normal_layouts(n):
    """normal [H,W,3] on the device, three ways: contiguous; the permuted view of a [3,H,W] tensor (stride_c = H W); channels 1..3 of
    an [H,W,5] tensor whose other channels hold values a wrong stride would pick up."""
    H, W, _ = n.shape
    wide = torch.full((H, W, 5), 7.0, device=n.device)
    wide[..., 1:4] = n
    return {"hwc": n.contiguous(), "chw": n.permute(2, 0, 1).contiguous().permute(1, 2, 0), "slice": wide[..., 1:4]}


def _alpha_layouts(a):
    """alpha [H,W] on the device as [H,W,1] contiguous, as the permuted view of [1,H,W] (what render_surfel passes), 2-D, and as
    channel 1 of an [H,W,2] tensor: the only one of the four whose stride_w is not 1."""
    wide = torch.full((a.shape[0], a.shape[1], 2), -3.0, device=a.device)
    wide[..., 1] = a
    return {"hw1": a.unsqueeze(-1).contiguous(), "1hw": a.unsqueeze(0).contiguous().permute(1, 2, 0), "hw": a.contiguous(),
            "slice": wide[..., 1:2]}


@functools.lru_cache(maxsize=None)
def _vis_tracer():
    from materialrefgs_amd.raytracing import RayTracer
    return RayTracer(*_vis_mesh())


def _assert_visibility_is_the_statement(H, W, case):
    from materialrefgs_amd.synthetic import orbit_camera
    normal, alpha, sd, stmt, _ = case
    rt = _vis_tracer()
    cam = orbit_camera(2, H, W).to("cuda")
    want = torch.tensor(stmt)                                             # (copies: the cached case is read-only)
    n_dev, a_dev = torch.tensor(normal).cuda(), torch.tensor(alpha).cuda()
    sd_dev = torch.tensor(sd).cuda().view(1, H, W)
    for kn, n_ in _normal_layouts(n_dev).items():
        for ka, a_ in _alpha_layouts(a_dev).items():
            vis = rt.visibility(cam.HWK, cam.R, cam.T, n_, a_, sd_dev)
            assert vis.shape == (H, W, 1)
            got = vis.cpu()[..., 0]
            assert torch.equal(got, want), (kn, ka, torch.nonzero(got != want)[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", VIS_SIZES)
def test_fused_visibility_is_exact_at_every_pixel(H, W):
    """mrgs_bvh_visibility against tests/visibility_statement.py: equal at every pixel, for every layout of the normal and alpha maps,
    at sizes with full, partial and ragged 8 x 32 tiles, on inputs that hold alpha <= 0, zero and grazing normals, a zero depth and
    surface points behind the mesh (_vis_case)."""
    case = _vis_case(H, W)
    assert 0.02 < case[4] < 0.98, case[4]                                # the case exercises both outcomes
    _assert_visibility_is_the_statement(H, W, case)


@pytest.mark.gpu
@pytest.mark.parametrize("want_blocked", [True, False])
def test_fused_visibility_of_a_single_pixel(want_blocked):
    """A 1 x 1 image: one lane of one workgroup, once blocked and once free."""
    case = _vis_case_one_pixel(want_blocked)
    assert bool(case[3][0, 0] == 0) == want_blocked
    _assert_visibility_is_the_statement(1, 1, case)


# ---------------------------------------------------------------- GPU: small and awkward trees through the C ABI
def _trace_abi(v, t, o, d, inplace=False):
    """mrgs_bvh_build + mrgs_bvh_trace by ctypes (RayTracer refuses <= 8 triangles; the library does not): numpy results."""
    L = _lib()
    rc, blob = _build(v, t)
    assert rc == L.MRGS_OK, rc
    dev = torch.device("cuda")
    blob_dev = torch.from_numpy(blob).to(dev)
    to, td = torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    n = to.shape[0]
    pos, nrm = (to, td) if inplace else (torch.empty_like(to), torch.empty_like(td))
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    with L.guard(dev):
        L.check(L.lib().mrgs_bvh_trace(p(blob_dev), len(t), n, p(to), p(td), p(pos), p(nrm), p(depth), p(ids), L.stream_ptr(dev)))
    return pos.cpu().numpy(), nrm.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()


def _check_abi_against_oracle(v, t, o, d, inplace=False):
    pos, nrm, depth, ids = _trace_abi(v, t, o, d, inplace)
    return _compare_with_oracle(v, t, o, d, pos, nrm, depth, ids)


CUBE_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5], [2, 2, 2]], dtype=np.float32)
CUBE_T = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [8, 8, 8], [9, 9, 1], [0, 2, 1]], dtype=np.int32)


def _small_mesh(n):
    """The first n of 65 triangles: the nine of the tiny cube case (with its zero-area and duplicated ones), then random ones."""
    rng = np.random.default_rng(21)
    extra = rng.uniform(-0.5, 1.5, size=(65 - len(CUBE_T), 3, 3)).astype(np.float32)
    v = np.concatenate([CUBE_V, extra.reshape(-1, 3)])
    t = np.concatenate([CUBE_T, len(CUBE_V) + np.arange(3 * len(extra), dtype=np.int32).reshape(-1, 3)])
    return v, np.ascontiguousarray(t[:n])


def _awkward_rays(n=257):
    """n rays at the unit cube; the first 24 are special: signed zeros in the direction, directions of length 0.25 and 3, origins on
    a triangle's plane and on a vertex, zero directions (indices 20..23)."""
    o, d = rays(n, 3)
    o = (o * np.float32(0.7)).astype(np.float32)
    nz = np.float32(-0.0)
    so = np.array([[0.25, 0.25, 3], [0.25, 0.25, 3], [0.25, 0.25, -3], [0.25, 0.25, -3], [3, 0.3, 0.4], [-3, 0.3, 0.4],      # signed zeros
                   [0.25, 0.25, 3], [0.25, 0.25, -3], [0.3, -2, 0.5], [0.3, -2, 0.5],                                     # lengths 0.25 and 3
                   [0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0], [0.6, 0, 0.3],                                      # on a plane
                   [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1],                                      # on a vertex
                   [0.5, 0.5, 0.5], [0.25, 0.25, 0], [1, 0, 0], [5, 5, 5]], dtype=np.float32)                             # zero direction
    sd = np.array([[0, nz, -1], [nz, 0, -1], [nz, nz, 1], [0, 0, 1], [-1, nz, 0], [1, nz, nz],
                   [0, 0, -0.25], [0, 0, 3], [0, 0.25, 0], [0, 3, 0],
                   [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, 1, 0],
                   [0, 0, 1], [-0.6, 0.48, 0.64], [0, 1, 0], [0, 0, 1], [0.577, 0.577, 0.577], [-0.577, -0.577, -0.577],
                   [0, 0, 0], [0, nz, 0], [nz, nz, nz], [0, 0, 0]], dtype=np.float32)
    k = min(n, len(so))
    o[:k], d[:k] = so[:k], sd[:k]
    if n > 40:
        d[24:32] = (d[24:32] * np.float32(0.25)).astype(np.float32)
        d[32:40] = (d[32:40] * np.float32(3.0)).astype(np.float32)
    return o, d


ZERO_RAYS = slice(20, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1.0], ids=["origin", "far"])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 9, 16, 17, 64, 65])
def test_trace_small_trees_through_the_c_abi(n, shift):
    """1..8 triangles (a forced inner root with empty slots) and the leaf / inner boundaries around 16 and 64, with 1, 255, 256 and
    257 rays that include signed zeros, non-unit and zero directions and origins on planes and vertices; `far` translates mesh and
    rays to coordinates of order 1e3."""
    v, t = _small_mesh(n)
    o, d = _awkward_rays(257)
    off = (np.float32(shift) * np.array([1000, -2000, 1500], dtype=np.float32)).astype(np.float32)
    v, o = (v + off).astype(np.float32), (o + off).astype(np.float32)
    for count in (257, 256, 255, 1):
        _check_abi_against_oracle(v, t, o[:count], d[:count], inplace=count == 255)
    pos, nrm, depth, ids = _trace_abi(v, t, o, d)
    assert bool((depth[ZERO_RAYS] == 10).all()) and bool((ids[ZERO_RAYS] == -1).all())          # a zero direction misses ...
    want = (o[ZERO_RAYS] + np.float32(10) * d[ZERO_RAYS]).astype(np.float32)
    assert pos[ZERO_RAYS].tobytes() == want.tobytes()                                            # ... and stays where it is, bit for bit
    assert not np.any(nrm[ZERO_RAYS])
    if n >= 9 and shift == 0:
        assert (depth < 10).any() and (depth >= 10).any()


@pytest.mark.gpu
def test_trace_mesh_of_repeated_triangles():
    """1 000 copies of three distinct triangles: every centroid ties with 999 others, so the median split falls back on the index
    order; every hit is an exact tie between copies, which the id check accepts only with proof."""
    v = CUBE_V
    t = np.ascontiguousarray(np.tile(CUBE_T[[0, 2, 4]], (1000, 1)))
    o, d = _awkward_rays(257)
    depth, ids = _check_abi_against_oracle(v, t, o, d)
    assert (depth < 10).any() and (depth >= 10).any()


# ---------------------------------------------------------------- GPU: the deepest supported walk
def _slab_hit(lo, hi, o, d, mint=np.float32(10.0)):
    """bvh_traverse's box test for rays o, d [N,3] against one box, float32 as written there."""
    with np.errstate(all="ignore"):
        iv = np.float32(1.0) / d
        a, b = (lo[None] - o) * iv, (hi[None] - o) * iv
        t_in = np.fmax(np.fmax(np.fmin(a[:, 0], b[:, 0]), np.fmin(a[:, 1], b[:, 1])), np.fmax(np.fmin(a[:, 2], b[:, 2]), np.float32(0)))
        t_out = np.fmin(np.fmin(np.fmax(a[:, 0], b[:, 0]), np.fmax(a[:, 1], b[:, 1])), np.fmax(a[:, 2], b[:, 2]))
        return (t_in <= t_out * np.float32(1.00001) + np.float32(1e-30)) & (t_in * np.float32(0.99999) < mint), t_in


def _first_descent_fill(nodes, codes, o, d):
    """Stack entries of ray (o, d) when its walk reaches its first leaf: bvh_traverse's child order (the sorting network on t_in,
    ties keep the slot order) followed from the root."""
    cur, fill = 0, 0
    while cur >= 0:
        dist, code = [], [int(c) for c in codes[cur]]
        for c in range(4):
            h, t_in = _slab_hit(nodes[cur, [0 + c, 4 + c, 8 + c]], nodes[cur, [12 + c, 16 + c, 20 + c]], o[None], d[None])
            dist.append(float(t_in[0]) if (h[0] and code[c] != BVH_EMPTY) else np.inf)
        for i, j in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
            if dist[j] < dist[i]:
                dist[i], dist[j], code[i], code[j] = dist[j], dist[i], code[j], code[i]
        assert dist[0] < np.inf
        fill += sum(1 for c in (1, 2, 3) if dist[c] < np.inf)
        cur = code[0]
    return fill


def _deep_mesh(staggered):
    """BVH_LEAF ** BVH_LEVELS + 1 triangles (one root-to-leaf path has BVH_LEVELS inner levels, as in the largest mesh the build
    accepts): copies of eight large tilted triangles that face away from rays travelling in -z, plus one that faces them, farther
    along the rays than all the others, stored in the middle of the index range.  `staggered`: copies of the first of them alone,
    copy i lifted by i * 2**-20 in z, so that every split is along z in index order, the larger (deeper) last quarter of every node
    is the one the rays enter first, and the walk descends the deepest path first with three siblings pushed at every level."""
    n = BVH_LEAF ** BVH_LEVELS + 1
    rng = np.random.default_rng(3)
    base = np.zeros((9, 3, 3), dtype=np.float32)
    for k in range(8):                                                    # (A, B, C): n_z = -64, away from the rays
        j = rng.uniform(-0.3, 0.3, size=(3, 2))
        base[k] = [[-4 + j[0, 0], -4 + j[0, 1], rng.uniform(0.0, 0.1)], [0 + j[1, 0], 4 + j[1, 1], rng.uniform(2.9, 3.0)],
                   [4 + j[2, 0], -4 + j[2, 1], rng.uniform(0.4, 0.6)]]
    base[8] = [[-4, -4, -1.5], [4, -4, -1.5], [0, 4, 2.0]]               # (A, C, B): faces +z, below the others over the ray patch
    if not staggered:
        kind = (np.arange(n) % 8).astype(np.int64)
        kind[n // 2] = 8
        v = base.reshape(-1, 3)
        t = (3 * kind[:, None] + np.arange(3)[None]).astype(np.int32)
    else:
        lift = np.arange(n, dtype=np.float32) * np.float32(2.0 ** -20)
        lift[n - 2:] = 1.5                                                # two copies on top of everything ...
        v = np.broadcast_to(base[0], (n, 3, 3)).copy()
        v[..., 2] += lift[:, None]
        base[8] = [[-4, -4, 3.9], [4, -4, 3.9], [0, 4, -0.3]]            # ... and the facing triangle's centroid right below theirs:
        v[n // 2] = base[8]                                               # it is one of the three leaves pushed at the deepest node
        v = v.reshape(-1, 3)
        t = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, 8), np.linspace(-0.5, 0.5, 8), indexing="ij")
    o = np.stack([gx.ravel(), gy.ravel(), np.full(64, 5.0)], -1).astype(np.float32)
    d = np.stack([0.02 * gy.ravel() + 0.003, -0.02 * gx.ravel() + 0.001, np.full(64, -1.0)], -1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(t), base, o, d


@pytest.mark.gpu
@pytest.mark.parametrize("staggered", [False, True], ids=["copies", "staggered"])
def test_trace_deepest_supported_walk(staggered):
    """One wave of 64 rays through a mesh of 4**10 + 1 triangles in which every ray enters every box: the walk with the longest stack
    the build lets through.  All triangles but one face away from the rays, so nothing is accepted before the one facing triangle is
    met and no box is pruned after it (it lies below every box's top): about 350 000 node visits and a million triangle tests per
    lane.  The host confirms that every ray passes through the intersection of all boxes, and the stack fill of the first descent.

    `copies` is the mesh of exact copies of eight triangles: boxes of equal children tie, ties keep the slot order, and the deeper
    last child is visited last, so the stack reaches 3 * 9 = 27 entries.  `staggered` lifts copy i of one triangle by i * 2**-20:
    the deepest path is walked first and the stack holds 3 * 10 = 30 entries, the most the build accepts; the facing triangle sits in
    one of the three leaves pushed last, so a walk that loses or overwrites an entry above 27 loses the hit.  A second launch writes
    positions and normals over the rays and must give the same bits.

    Measured on an MI355X, 2026-10-21: 0.50 s for the first launch and 0.43 s for the second, the same for both meshes; the whole
    test takes 1.1 s."""
    L = _lib()
    v, t, base, o, d = _deep_mesh(staggered)
    n = len(t)
    assert n == BVH_LEAF ** BVH_LEVELS + 1
    rc, blob = _build(v, t)
    assert rc == L.MRGS_OK, rc
    nodes, codes, _, perm = _views(blob, n)
    assert _inner_levels(codes) == BVH_LEVELS
    if staggered:                                                          # the facing triangle is one of the three leaves pushed on top of
        assert n - int(np.nonzero(perm == n // 2)[0][0]) in (3, 4, 5)      # the full stack: the deepest node holds the last five, 1 + 1 + 1 + 2
    used = np.zeros(len(codes), dtype=bool)
    used[0] = True
    used[codes[(codes >= 0) & (codes != BVH_EMPTY)]] = True
    real = (codes != BVH_EMPTY) & used[:, None]                            # child slots of the nodes the build wrote
    lo = np.stack([nodes[:, 0:4][real].max(), nodes[:, 4:8][real].max(), nodes[:, 8:12][real].max()]).astype(np.float32)
    hi = np.stack([nodes[:, 12:16][real].min(), nodes[:, 16:20][real].min(), nodes[:, 20:24][real].min()]).astype(np.float32)
    assert bool((lo < hi).all()), (lo, hi)                                 # all boxes share a volume ...
    inside, _ = _slab_hit(lo, hi, o, d)
    assert bool(inside.all())                                              # ... every ray passes through, so it enters every box (the slab test is monotone)
    fills = {_first_descent_fill(nodes, codes, o[r], d[r]) for r in (0, 21, 63)}
    assert fills == {3 * BVH_LEVELS if staggered else 3 * (BVH_LEVELS - 1)}, fills
    # expected: the facing triangle, at the distance the brute force finds among the nine distinct triangles
    _, _, rdepth, rids = trace_oracle.trace(base.reshape(-1, 3), np.arange(27).reshape(9, 3), o, d)
    assert bool((rids == 8).all()) and bool((rdepth < 10).all())
    dev = torch.device("cuda")
    blob_dev = torch.from_numpy(blob).to(dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    results = []
    for inplace in (False, True):
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        pos, nrm = (to, td) if inplace else (torch.empty_like(to), torch.empty_like(td))
        depth = torch.empty(64, dtype=torch.float32, device=dev)
        ids = torch.empty(64, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with L.guard(dev):
            L.check(L.lib().mrgs_bvh_trace(p(blob_dev), n, 64, p(to), p(td), p(pos), p(nrm), p(depth), p(ids), L.stream_ptr(dev)))
        torch.cuda.synchronize()
        print(f"deepest walk ({'staggered' if staggered else 'copies'}, inplace={inplace}): {time.perf_counter() - t0:.3f} s")
        results.append((pos.cpu().numpy(), nrm.cpu().numpy(), depth.cpu().numpy(), ids.cpu().numpy()))
    pos, nrm, depth, ids = results[0]
    assert bool((ids == n // 2).all()), ids
    np.testing.assert_array_equal(depth, rdepth)
    np.testing.assert_array_equal(pos, (o + rdepth[:, None] * d).astype(np.float32))
    for a, b in zip(results[0], results[1]):
        assert a.tobytes() == b.tobytes()
