"""TEST INFRASTRUCTURE ONLY -- the statement of RayTracer.secondary_indirect_color / shade (raytracing_brdf/raytracer.py:218-297) in
torch, in whatever dtype its inputs have (float64 = the truth leg, float32 = the literal reading), with autograd for the gradients.

Texture fetches come from oracle/shading_oracle.py (`env_lookup`, `lut_fetch`), the stand-ins the reference fixtures are generated with.
Three readings are fixed here as the product fixes them:
  * every ray uses its own FG pair; `first_row_fg=True` reproduces the reference's text (`fg[0]` of the reshaped fetch, :259-263), which
    weights every hit ray with the pair of the FIRST hit ray -- used only to pin this statement to the reference's recorded output;
  * the normal table arrives decoded;
  * the weights are the xy-projected areas of barycentric_interpolation (:209-216) in its literal form; a projected area of exactly 0
    writes 0.
"""
import numpy as np
import torch

from oracle import shading_oracle as so

MISS_DEPTH = 10.0


def area(v1, v2, v3):
    """barycentric_interpolation's `area`, :210-213."""
    return 0.5 * torch.abs(v1[..., 0] * (v2[..., 1] - v3[..., 1]) + v2[..., 0] * (v3[..., 1] - v1[..., 1]) +
                           v3[..., 0] * (v1[..., 1] - v2[..., 1]))


def gather(pos, ids, vertices, triangles, tables):
    """The interpolated rows of every table in `tables` (a dict of [V,c]) at `pos` on the triangles `ids` (all valid), the weights
    [N,3] and the projected area of the triangle [N].  A triangle of projected area 0 gives zeros."""
    vid = triangles[ids.long()].long()
    vp = vertices[vid]
    a, b, c = vp[:, 0], vp[:, 1], vp[:, 2]
    den = area(a, b, c)
    ok = den > 0
    safe = torch.where(ok, den, torch.ones_like(den))
    w = torch.stack([area(pos, b, c), area(pos, c, a), area(pos, a, b)], dim=-1)
    out = {}
    for k, t in tables.items():
        v = (w.unsqueeze(-1) * t[vid]).sum(dim=1) / safe.unsqueeze(-1)
        out[k] = torch.where(ok.unsqueeze(-1), v, torch.zeros_like(v))
    return out, w, den


def secondary_indirect_color(pos, view, ids, depth, vertices, triangles, tables, base, spec, lut, min_roughness=0.08, max_roughness=0.5,
                             first_row_fg=False, active=None):
    """[N,3].  tables: diffuse, albedo, normal (decoded) [V,3], metallic, roughness [V,1]; base [6,R,R,3]; spec: the prefiltered chain."""
    N = pos.shape[0]
    out = torch.zeros((N, 3), dtype=base.dtype)
    act = torch.ones(N, dtype=torch.bool) if active is None else active.bool()
    miss = (depth >= MISS_DEPTH) & act
    hit = (depth < MISS_DEPTH) & act
    if bool(miss.any()):
        out[miss] = so.env_lookup([base], -view[miss])
    if bool(hit.any()):
        g, _, den = gather(pos[hit], ids[hit], vertices, triangles, tables)
        v = view[hit]
        n, m, r = g["normal"], g["metallic"], g["roughness"]
        ndv = torch.sum(v * n, dim=-1, keepdim=True)
        l = 2 * n * ndv - v
        l = l / torch.clamp(torch.linalg.norm(l, dim=-1, keepdim=True), min=1e-20)
        fg = so.lut_fetch(lut, torch.cat([ndv, r], -1).clamp(0, 1))
        if first_row_fg:
            fg = fg[0:1].expand_as(fg)
        light = so.env_lookup(spec, l, roughness=r[:, 0], min_roughness=min_roughness, max_roughness=max_roughness)
        col = (1 - m) * g["diffuse"] + ((0.04 * (1 - m) + g["albedo"] * m) * fg[:, 0:1] + fg[:, 1:2]) * light
        out[hit] = torch.where((den > 0).unsqueeze(-1), col, torch.zeros_like(col))
    return out


def incident(rays_n, rays_v):
    """reflection(rays_v, rays_n) (utils/refl_utils.py:95-98), not normalised (raytracer.py:284-285 drops safe_normalize's result)."""
    return 2 * rays_n * torch.sum(rays_v * rays_n, dim=-1, keepdim=True) - rays_v


def ambiguous(pos, ids, depth, vertices, triangles, tables, lut_res, n_levels, min_roughness=0.08, max_roughness=0.5):
    """bool [N]: hit rays at which the gradient of the statement is not continuous, or whose weights are ill-conditioned."""
    N = pos.shape[0]
    flag = torch.zeros(N, dtype=torch.bool)
    hit = depth < MISS_DEPTH
    if not bool(hit.any()):
        return flag
    vid = triangles[ids[hit].long()].long()
    vp = vertices[vid].double()
    g, _, den = gather(pos[hit].double(), ids[hit], vertices.double(), triangles, {"roughness": tables["roughness"].double()})
    r = g["roughness"][:, 0]
    fy = r.clamp(0, 1) * lut_res - 0.5
    bad = (fy - torch.round(fy)).abs() < 1e-4
    lev = so.get_mip(r, n_levels, min_roughness, max_roughness).clamp(0, n_levels - 1)
    bad |= (lev - torch.round(lev)).abs() < 1e-4
    for edge in (0.0, 1.0, min_roughness, max_roughness):
        bad |= (r - edge).abs() < 1e-5
    true_area = 0.5 * torch.linalg.norm(torch.cross(vp[:, 1] - vp[:, 0], vp[:, 2] - vp[:, 0], dim=-1), dim=-1)
    bad |= den < 1e-6 * true_area
    flag[hit] = bad
    return flag


# ---- the test scene ------------------------------------------------------------------------------------------------------------------
def sheet(z0, seed, face_down, n=9):
    """A height field on an n x n lattice over [-1,1]^2 at z0 +- 0.05: (vertices [n n,3], triangles [2 (n-1)^2,3])."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-1.0, 1.0, n)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    Z = z0 + rng.uniform(-0.05, 0.05, size=X.shape)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: i * n + j   # noqa: E731
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            p00, p10, p01, p11 = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            tris += [(p00, p10, p11), (p00, p11, p01)]                       # counter-clockwise in xy: the normal points up
    t = np.asarray(tris, dtype=np.int32)
    if face_down:
        t = t[:, [0, 2, 1]]
    return v, t


def scene(seed=0, n_rays=4099, wall=False):
    """Two sheets (a floor at z = -1 facing up, a ceiling at z = 1 facing down: the tracer accepts front faces only), random material
    tables, and surface points on -1.3 ... 1.3 at z ~ 0 with perturbed unit normals and view directions -- about a third of the mirror
    rays meet the ceiling, the rest leave.  wall=True adds one vertical wall (two triangles of projected area 0, facing -x) at x = 0.5."""
    g = torch.Generator().manual_seed(seed)
    v0, t0 = sheet(-1.0, 100 + seed, face_down=False)
    v1, t1 = sheet(1.0, 200 + seed, face_down=True)
    vs, ts = [v0, v1], [t0, t1 + len(v0)]
    if wall:
        nv = len(v0) + len(v1)
        vs.append(np.array([[0.5, -0.9, -0.8], [0.5, 0.9, -0.8], [0.5, 0.9, 0.8], [0.5, -0.9, 0.8]], dtype=np.float32))
        ts.append(np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32) + nv)       # normal (-1, 0, 0)
    vertices, triangles = torch.from_numpy(np.concatenate(vs)), torch.from_numpy(np.concatenate(ts))
    V = vertices.shape[0]
    rnd = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    normal = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.35 * torch.randn(V, 3, generator=g), dim=-1)
    normal[:len(v0)] *= -1.0                                                   # the floor's normals point up
    tables = {"diffuse": rnd(V, 3), "albedo": rnd(V, 3), "metallic": rnd(V, 1), "roughness": 0.03 + 0.94 * rnd(V, 1), "normal": normal}
    pos = torch.cat([rnd(n_rays, 2) * 2.6 - 1.3, 0.05 * torch.randn(n_rays, 1, generator=g)], dim=-1)
    up = torch.tensor([0.0, 0.0, 1.0])
    rays_n = torch.nn.functional.normalize(up + 0.25 * torch.randn(n_rays, 3, generator=g), dim=-1)
    rays_v = torch.nn.functional.normalize(up + 0.45 * torch.randn(n_rays, 3, generator=g), dim=-1)
    return {"vertices": vertices, "triangles": triangles, "tables": tables, "surface_pos": pos, "rays_n": rays_n, "rays_v": rays_v}


def environment(seed=0, res=(32, 16, 8)):
    """(base, spec): a random un-filtered level and a random chain (the kernel takes them as independent inputs)."""
    g = torch.Generator().manual_seed(1000 + seed)
    base = torch.randn(6, res[0], res[0], 3, generator=g)
    spec = [torch.randn(6, r, r, 3, generator=g) for r in res]
    return base, spec


def trace_cpu(sc, rays_o, rays_d):
    """oracle/trace_oracle.py on the scene: (hit_pos, face_normals, depth, ids int32) as fp32 torch tensors."""
    from oracle import trace_oracle as to
    pos, nrm, dpt, ids = to.trace(sc["vertices"].numpy(), sc["triangles"].numpy(), rays_o.numpy(), rays_d.numpy())
    return torch.from_numpy(pos), torch.from_numpy(nrm), torch.from_numpy(dpt), torch.from_numpy(ids.astype(np.int32))


def to64(x):
    if isinstance(x, dict):
        return {k: to64(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to64(v) for v in x]
    return x.double() if x.dtype.is_floating_point else x
