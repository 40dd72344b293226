"""TEST INFRASTRUCTURE ONLY -- the statement of mrgs_bvh_visibility (csrc/mrgs_bvh.hip, bvh_visibility_kernel) in numpy float32.

`mirror_rays` restates the kernel's ray set-up operation by operation, in the kernel's order and association: the file is compiled
with -ffp-contract=off (no multiply-add is fused) and its sqrtf and / are the correctly rounded ones, so every intermediate is the
float32 value numpy computes and the rays are the kernel's bit for bit.  `visibility` then asks the brute-force triangle test of
oracle/trace_oracle.py whether any front-facing triangle is hit at 0 <= t < 10.  Any-hit and closest-hit agree on that question, and
the hierarchy only prunes -- conservatively: padded boxes, widened slab test -- so equality with this statement, for every pixel, is
the kernel's specification and not an approximation of it.

`reference_rays_f64` is the sequence of the reference (utils/refl_utils.py:75-98 and :379-391) in float64, and `triangle_slack_f64`
the triangle test's quantities in float64: what tests/test_raytracing.py uses to show that only rounding separates the two.
"""
import numpy as np

from oracle import trace_oracle

f32 = np.float32
MAX_DIST = 10.0


def kinv_f32(K):
    """The inverse RayTracer.visibility hands to the kernel."""
    return np.linalg.inv(np.asarray(K, dtype=np.float32)).astype(np.float32)


def _row(M, r, x, y, z):
    return (M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z


def camera_rays(H, W, Kinv, R, T):
    """(rays_o [3], rays_cam [H,W,3]): the un-normalised pixel rays as the kernel forms them."""
    Kinv, R, T = (np.asarray(a, dtype=np.float32) for a in (Kinv, R, T))
    Kinv, R, T = Kinv.reshape(3, 3), R.reshape(3, 3), T.reshape(3)
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    pcx = (Kinv[0, 0] * fx + Kinv[0, 1] * fy) + Kinv[0, 2]
    pcy = (Kinv[1, 0] * fx + Kinv[1, 1] * fy) + Kinv[1, 2]
    pcz = (Kinv[2, 0] * fx + Kinv[2, 1] * fy) + Kinv[2, 2]
    qx, qy, qz = pcx - T[0], pcy - T[1], pcz - T[2]
    ro = np.stack([-_row(R, r, T[0], T[1], T[2]) for r in range(3)]).astype(np.float32)
    c = np.stack([_row(R, r, qx, qy, qz) - ro[r] for r in range(3)], axis=-1)
    assert c.dtype == np.float32 and ro.dtype == np.float32
    return ro, c


def _unit(x, y, z):
    """v / max(|v|, 1e-20), fmaxf semantics (a NaN length gives 1e-20)."""
    length = np.fmax(np.sqrt((x * x + y * y) + z * z), f32(1e-20))
    return x / length, y / length, z / length


def mirror_rays(H, W, Kinv, R, T, normal, alpha, surf_depth):
    """(origins [H,W,3], directions [H,W,3], traced [H,W] bool) of bvh_visibility_kernel; normal [H,W,3], alpha [H,W] or [H,W,1],
    surf_depth [H,W] or [1,H,W], all float32."""
    n = np.asarray(normal, dtype=np.float32).reshape(H, W, 3)
    a = np.asarray(alpha, dtype=np.float32).reshape(H, W)
    sd = np.asarray(surf_depth, dtype=np.float32).reshape(H, W)
    ro, c = camera_rays(H, W, Kinv, R, T)
    with np.errstate(all="ignore"):
        cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
        wx, wy, wz = _unit(-cx, -cy, -cz)
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        ndv = (wx * nx + wy * ny) + wz * nz
        rx, ry, rz = (f32(2) * nx) * ndv - wx, (f32(2) * ny) * ndv - wy, (f32(2) * nz) * ndv - wz
        rx, ry, rz = _unit(rx, ry, rz)
        origins = np.stack([ro[0] + sd * cx, ro[1] + sd * cy, ro[2] + sd * cz], axis=-1)
    directions = np.stack([rx, ry, rz], axis=-1)
    assert origins.dtype == np.float32 and directions.dtype == np.float32
    return origins, directions, a > 0


def visibility(vertices, triangles, H, W, Kinv, R, T, normal, alpha, surf_depth):
    """[H,W] float32: 1 where the pixel is not traced or its mirror ray is free for 10 units, 0 where a triangle blocks it."""
    o, d, traced = mirror_rays(H, W, Kinv, R, T, normal, alpha, surf_depth)
    vis = np.ones((H, W), dtype=np.float32)
    if traced.any():
        _, _, depth, _ = trace_oracle.trace(vertices, triangles, o[traced], d[traced])
        vis[traced] = (depth >= f32(MAX_DIST)).astype(np.float32)
    return vis


# ---------------------------------------------------------------- float64: the reference's sequence
def reference_rays_f64(H, W, K, R, T, normal, surf_depth):
    """(origins, directions) [H,W,3] float64: sample_camera_rays_unnormalize (utils/refl_utils.py:75-93), safe_normalize and
    reflection (:95-98) and the intersection point of get_specular_color_surfel (:379-386), all in float64 from the float32 inputs."""
    K, R, T = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (K, R, T))
    n = np.asarray(normal, dtype=np.float32).astype(np.float64).reshape(H, W, 3)
    sd = np.asarray(surf_depth, dtype=np.float32).astype(np.float64).reshape(H, W, 1)
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = xy1 @ np.linalg.inv(K).T
    Rt = R.T
    rays_o = -(Rt.T @ T)
    rays_cam = ((pixel_camera - T).reshape(-1, 3) @ Rt - rays_o).reshape(H, W, 3)
    safe = lambda x: x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-20)   # noqa: E731
    w_o = safe(-rays_cam)
    refl = safe(2 * n * (w_o * n).sum(-1, keepdims=True) - w_o)
    return rays_o + sd * rays_cam, refl


def triangle_slack_f64(vertices, triangles, rays_o, rays_d):
    """[N,T,5] float64 for N rays against T triangles: (u, v, 1 - u - v, -dn, 10 - t), the quantities Triangle::ray_intersect and the
    closest-hit loop compare with 0, and t [N,T] itself.  A triangle is accepted where all five are >= 0 (-dn > 0) and t >= 0."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    a, e1, e2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    n = np.cross(e1, e2)
    o, d = np.asarray(rays_o, dtype=np.float64)[:, None, :], np.asarray(rays_d, dtype=np.float64)[:, None, :]
    r = o - a[None]
    dn = (d * n[None]).sum(-1)
    q = np.cross(r, np.broadcast_to(d, r.shape))
    with np.errstate(all="ignore"):
        inv = 1.0 / dn
        u = inv * -(q * e2[None]).sum(-1)
        w = inv * (q * e1[None]).sum(-1)
        tt = inv * -(n[None] * r).sum(-1)
    return np.stack([u, w, 1.0 - u - w, -dn, MAX_DIST - tt], axis=-1), tt
