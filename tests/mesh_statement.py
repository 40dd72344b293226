"""The mesh extraction step restated in float64 numpy: the contract of include/mrgs.h's mesh section, written for reading, not for speed.

  fuse                  the TSDF rule of compute_unbounded_tsdf / compute_sdf_perframe (utils/mesh_utils.py:322-373) with the update
                        count, the samples whose decisions sit within `margin` of a threshold, and a per-sample bound on what fp32
                        rounding of the stated operation sequence can move (derivation: `fuse`'s docstring)
  marching_tetrahedra   six Kuhn tetrahedra per cube, vertices keyed by (owning lattice point, edge kind), windings decided by geometry
  components / post_process_mesh   connected components through shared vertex indices (scipy.sparse.csgraph) and the floater rule
  self_test             the three known answers of the issue's table

Inputs that are fp32 on the device (camera matrices, depth maps, fields, origins, spacings) are passed as fp32 values converted to
float64, so the statement computes the exact function of the same numbers.
"""
import itertools

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph

EPS = 2.0 ** -24          # unit roundoff of fp32

# ---- samples ---------------------------------------------------------------------------------------------------------------------


def lattice_index(shape):
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)            # C order: the last axis is the fastest


def plain_samples(origin, spacing, shape):
    """x = origin + spacing * (i, j, k).  pos_err: fp32 forms the product (eps |s i|) and the sum (eps |x|)."""
    origin, spacing = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    idx = lattice_index(shape)
    x = origin + spacing * idx
    return x, EPS * (np.abs(spacing * idx) + np.abs(x))


def uncontract(y):
    mag = np.linalg.norm(y, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag < 1, y, y / ((2 - mag) * mag))


def contract(x):
    mag = np.linalg.norm(x, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag < 1, x, (2 - 1 / mag) * (x / mag))


def contracted_samples(R, N, center, radius, voxel):
    """s = linspace(-R, R, N) per axis (one lattice), x = center + radius * uncontract(s), trunc = 5 voxel, times 1 / (2 - min(|s|, 1.9))
    where |s| > 1.  pos_err: s carries 2 eps |s| per axis; the norm, the factor 1 / ((2 - m) m) and the scaling add about 8 roundings, and
    the factor's sensitivity to m grows as 1 / (2 - m): bounded by (12 + 4 / |2 - m|) eps |x - center| + eps |x| per axis."""
    step = 2.0 * R / (N - 1)
    s = -R + step * lattice_index((N, N, N))
    mag = np.linalg.norm(s, axis=-1)
    trunc = np.full(len(s), 5.0 * voxel)
    out = mag > 1
    trunc[out] *= 1.0 / (2.0 - np.minimum(mag[out], 1.9))
    x = np.asarray(center, np.float64) + radius * uncontract(s)
    rel = (12.0 + 4.0 / np.maximum(np.abs(2.0 - mag), 1e-3)) * EPS
    pos_err = rel[:, None] * np.abs(x - np.asarray(center, np.float64)) + EPS * np.abs(x)
    return x, trunc, pos_err


# ---- fusion ----------------------------------------------------------------------------------------------------------------------
def _gather(depth, yy, xx):
    H, W = depth.shape
    return depth[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]


def fuse(x, trunc, views, depth_trunc=None, pos_err=None, trunc_rel_err=0.0, margin=1e-4, bound=True):
    """views: list of (full_proj_transform [4,4], depth [H,W]).  Returns dict(tsdf, w, excluded, tol).

    The bound `tol` on |fp32 result - this result|, per sample, follows the operation sequence of the contract.  With e = 2^-24:
      clip_j = sum_i x_i M_ij + M_3j     four terms: |d clip_j| <= sum_i pos_err_i |M_ij| + 4 e (sum_i |x_i M_ij| + |M_3j|)   =: E_j
      z = clip_w                         dz = E_w
      ndc = clip_xy / z                  d ndc <= (E_xy + |ndc| E_w) / |z| + e |ndc|
      p = (ndc + 1) / 2 * (S - 1)        dp <= (S - 1) / 2 * (d ndc + 2 e (|ndc| + 1))           (S = W for x, H for y)
      d = bilinear tap                   dd <= dp_x Gx + dp_y Gy + 6 e max|texel|: the tap is continuous and piecewise bilinear, so a
                                         position error moves it by at most the largest texel difference per texel of position; Gx, Gy are
                                         the largest horizontal / vertical differences in the 4 x 4 neighbourhood of the cell (the fp32 tap
                                         may fall in the next cell); 6 e covers the weights, the four products and the three sums
      sdf = d - z                        dsdf <= dd + dz + e |sdf|
      r = sdf / trunc                    dr <= dsdf / trunc + (2 e + trunc_rel_err) |r|;  t = clamp(r) is exact 1 or -1 when |r| - dr >= 1
      tsdf' = (tsdf w + t) / (w + 1)     err' <= (err w + dt) / (w + 1) + 3 e            (|tsdf|, |t| <= 1; product, sum, quotient)
    -- the per-view terms are averaged exactly as the rule averages the values.
    A sample is `excluded` when, in any view, |ndc_x| - 1, |ndc_y| - 1 or z lies within `margin` of 0, or the view passes those and
    (sdf + trunc) / trunc does; with depth_trunc (texel validity: the choice of the cell is a decision there) also when a tap position lies
    within `margin` of a texel centre.  bound=False skips the bound (tol is None): the values alone cost a third."""
    x = np.asarray(x, np.float64)
    n = len(x)
    trunc = np.broadcast_to(np.asarray(trunc, np.float64), (n,))
    pos_err = np.zeros_like(x) if pos_err is None else pos_err
    tsdf, w, err = np.ones(n), np.ones(n), np.zeros(n)
    excluded = np.zeros(n, bool)
    for M, depth in views:
        M, depth = np.asarray(M, np.float64), np.asarray(depth, np.float64)
        H, W = depth.shape
        clip = x @ M[:3] + M[3]
        z = clip[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            ndc = clip[:, :2] / z[:, None]
        mask = (ndc[:, 0] > -1) & (ndc[:, 0] < 1) & (ndc[:, 1] > -1) & (ndc[:, 1] < 1) & (z > 0)
        near = (np.abs(np.abs(ndc[:, 0]) - 1) < margin) | (np.abs(np.abs(ndc[:, 1]) - 1) < margin) | (np.abs(z) < margin)
        size = np.array([W - 1, H - 1], np.float64)
        nd = np.where(mask[:, None], ndc, 0.0)
        p = np.clip((nd + 1) * 0.5 * size, 0, size)
        f = np.floor(p)
        x0, y0 = f[:, 0].astype(np.int64), f[:, 1].astype(np.int64)
        tx, ty = p[:, 0] - f[:, 0], p[:, 1] - f[:, 1]
        d00, d01, d10, d11 = _gather(depth, y0, x0), _gather(depth, y0, x0 + 1), _gather(depth, y0 + 1, x0), _gather(depth, y0 + 1, x0 + 1)
        d = d00 * ((1 - tx) * (1 - ty)) + d01 * (tx * (1 - ty)) + d10 * ((1 - tx) * ty) + d11 * (tx * ty)
        if depth_trunc is not None:
            lo, hi = np.minimum.reduce([d00, d01, d10, d11]), np.maximum.reduce([d00, d01, d10, d11])
            near |= mask & ((np.abs(p - np.round(p)) < margin).any(axis=1))
            mask = mask & (lo > 0) & (hi <= depth_trunc)
        sdf = d - z
        q = (sdf + trunc) / trunc
        excluded |= near | (mask & (np.abs(q) < margin))
        mask = mask & (sdf > -trunc)
        r = sdf / trunc
        t = np.clip(r, -1, 1)
        if bound:
            E = pos_err @ np.abs(M[:3]) + 4 * EPS * (np.abs(x) @ np.abs(M[:3]) + np.abs(M[3]))
            with np.errstate(divide="ignore", invalid="ignore"):
                dndc = (E[:, :2] + np.abs(ndc) * E[:, 3:4]) / np.abs(z)[:, None] + EPS * np.abs(ndc)
            dp = 0.5 * size * (np.where(mask[:, None], dndc, 0.0) + 2 * EPS * (np.abs(nd) + 1))
            Gx, Gy, dmax = np.zeros(n), np.zeros(n), np.zeros(n)
            for a in range(-1, 3):
                for b in range(-1, 3):
                    c = _gather(depth, y0 + a, x0 + b)
                    dmax = np.maximum(dmax, np.abs(c))
                    if b < 2:
                        Gx = np.maximum(Gx, np.abs(_gather(depth, y0 + a, x0 + b + 1) - c))
                    if a < 2:
                        Gy = np.maximum(Gy, np.abs(_gather(depth, y0 + a + 1, x0 + b) - c))
            dsdf = dp[:, 0] * Gx + dp[:, 1] * Gy + 6 * EPS * dmax + E[:, 3] + EPS * np.abs(sdf)
            dr = dsdf / trunc + (2 * EPS + trunc_rel_err) * np.abs(r)
            dt = np.where(np.abs(r) - dr >= 1, 0.0, dr)
            err = np.where(mask, (err * w + dt) / (w + 1) + 3 * EPS, err)
        tsdf = np.where(mask, (tsdf * w + t) / (w + 1), tsdf)
        w = np.where(mask, w + 1, w)
    return dict(tsdf=tsdf, w=w, excluded=excluded, tol=err if bound else None)


# ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
def _code_offset(c):
    return np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1])


KUHN = []                                     # (corner codes of the four vertices, sign of the axis permutation)
for perm in itertools.permutations(range(3)):
    bits = [4 >> a for a in perm]
    sign = round(float(np.linalg.det(np.eye(3)[list(perm)])))
    KUHN.append(((0, bits[0], bits[0] | bits[1], 7), sign))


def predicted_flip(sign, ins):
    """The parity rule the kernel uses for the triangle orders produced below (`ins`: bit m = vertex m of the tetrahedron is inside);
    self_test checks it against the geometric winding."""
    inside = [m for m in range(4) if (ins >> m) & 1]
    if len(inside) == 2:
        return (sign > 0) != (inside[1] - inside[0] != 2)
    lone = inside[0] if len(inside) == 1 else [m for m in range(4) if not (ins >> m) & 1][0]
    positive = ((sign > 0) == (lone % 2 == 0)) == (len(inside) == 1)
    return not positive


def marching_tetrahedra(F, level, origin, spacing, contraction=None, return_flips=False):
    """F [n0,n1,n2] (fp32 values).  Returns dict(vertices [V,3] float64, triangles [T,3] int64 indices into the key-sorted vertices,
    keys [V] = lattice_linear_index * 8 + direction code, tkeys [T,3] the same triangles as vertex keys, frac [V] = |F_a - level| / |F_b - F_a|,
    ends [V,2,3] the two lattice end points).  contraction = (center, radius): vertices are formed as stated, then mapped by
    center + radius * uncontract(.) and clipped to +-32."""
    F = np.asarray(F, np.float64)
    origin, spacing = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    n0, n1, n2 = F.shape
    inside = F < level
    lin = np.arange(F.size).reshape(F.shape)
    idx3 = lattice_index(F.shape)
    keys, pos, frac, ends = [], [], [], []
    for c in range(1, 8):
        dx, dy, dz = _code_offset(c)
        lo = (slice(0, n0 - dx), slice(0, n1 - dy), slice(0, n2 - dz))
        hi = (slice(dx, n0), slice(dy, n1), slice(dz, n2))
        cross = inside[lo] != inside[hi]
        owner = lin[lo][cross]
        Fa, Fb = F[lo][cross], F[hi][cross]
        t = (level - Fa) / (Fb - Fa)
        pa = origin + spacing * idx3[owner]
        pb = origin + spacing * (idx3[owner] + _code_offset(c))
        keys.append(owner * 8 + c)
        pos.append(pa + t[:, None] * (pb - pa))
        frac.append(np.abs(Fa - level) / np.abs(Fb - Fa))
        ends.append(np.stack([pa, pb], axis=1))
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    order = np.argsort(keys)
    keys = keys[order]
    pos, frac, ends = np.concatenate(pos)[order], np.concatenate(frac)[order], np.concatenate(ends)[order]
    lattice_pos = pos.copy()

    cube = (slice(0, n0 - 1), slice(0, n1 - 1), slice(0, n2 - 1))
    base = lin[cube]
    strides = np.array([n1 * n2, n2, 1])

    def corner(c):
        d = _code_offset(c)
        return inside[d[0]:n0 - 1 + d[0], d[1]:n1 - 1 + d[1], d[2]:n2 - 1 + d[2]]

    tkeys, flips_pred, tets = [], [], []
    for codes, sign in KUHN:
        ins = sum(corner(c).astype(np.int64) << m for m, c in enumerate(codes))
        for pattern in range(1, 15):
            sel = base[ins == pattern]
            if sel.size == 0:
                continue
            ii = [m for m in range(4) if (pattern >> m) & 1]
            oo = [m for m in range(4) if not (pattern >> m) & 1]

            def edge(m, n):
                a, b = min(m, n), max(m, n)
                return (sel + int(_code_offset(codes[a]) @ strides)) * 8 + (codes[b] ^ codes[a])
            if len(ii) == 2:
                (a, b), (c, d) = ii, oo
                tris = [(edge(a, c), edge(a, d), edge(b, d)), (edge(a, c), edge(b, d), edge(b, c))]
            else:
                lone = ii[0] if len(ii) == 1 else oo[0]
                others = [m for m in range(4) if m != lone]
                tris = [tuple(edge(lone, o) for o in others)]
            for tri in tris:
                tkeys.append(np.stack(tri, axis=1))
                flips_pred.append(np.full(sel.size, predicted_flip(sign, pattern)))
                # centroid of the outside corners minus centroid of the inside corners: along it the interpolant grows
                cin = np.mean([_code_offset(codes[m]) for m in ii], axis=0)
                cout = np.mean([_code_offset(codes[m]) for m in oo], axis=0)
                tets.append(np.broadcast_to((cout - cin) * spacing, (sel.size, 3)))
    if tkeys:
        tkeys, flips_pred, tets = np.concatenate(tkeys), np.concatenate(flips_pred), np.concatenate(tets)
        tri = np.searchsorted(keys, tkeys)
        assert (keys[tri] == tkeys).all()
        p = lattice_pos[tri]
        normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        flip = (normal * tets).sum(axis=1) < 0            # the normal points from inside to outside
        tri[flip] = tri[flip][:, [0, 2, 1]]
        tkeys[flip] = tkeys[flip][:, [0, 2, 1]]
    else:
        tkeys, tri, flip, flips_pred = np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros(0, bool), np.zeros(0, bool)
    if contraction is not None:
        center, radius = contraction
        pos = np.clip(np.asarray(center, np.float64) + radius * uncontract(pos), -32.0, 32.0)
    out = dict(vertices=pos, triangles=tri, keys=keys, tkeys=tkeys, frac=frac, ends=ends, lattice_vertices=lattice_pos)
    if return_flips:
        out["flip"], out["flip_predicted"] = flip, flips_pred
    return out


def vertex_tolerance(mt):
    """|fp32 vertex - statement vertex| per coordinate, for vertices formed as p_a + t (p_b - p_a), t = (level - F_a) / (F_b - F_a), from the
    same fp32 F: the two differences and the quotient each round once, so t is off by at most 3 * 2^-24 t <= 2^-22 |F_a - level| /
    |F_b - F_a| relative to the edge (times the spacing, bounded by the edge's extent on that axis); p_a, p_b (product and sum: 2 roundings
    each), their difference, the product with t and the final sum stay within 4 ulp of the larger end point's coordinate
    (ulp(c) <= 2^-23 |c|)."""
    ends = mt["ends"]
    big = np.abs(ends).max(axis=1)
    extent = np.abs(ends[:, 1] - ends[:, 0])
    return 4 * 2.0 ** -23 * big + extent * 2.0 ** -22 * mt["frac"][:, None]


def edge_census(tri):
    """(undirected edge -> count, directed edge -> count) as arrays of counts."""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    V = int(tri.max()) + 1 if tri.size else 1
    directed = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)[1]
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * V + np.maximum(e[:, 0], e[:, 1]), return_counts=True)[1]
    return und, directed


def components(n_vertices, tri):
    """labels [V] of the connected components through shared vertex indices, and triangles per label."""
    tri = np.asarray(tri)
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]]]) if len(tri) else np.zeros((0, 2), np.int64)
    g = scipy.sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n_vertices, n_vertices))
    ncomp, labels = scipy.sparse.csgraph.connected_components(g, directed=False)
    counts = np.bincount(labels[tri[:, 0]], minlength=ncomp) if len(tri) else np.zeros(ncomp, np.int64)
    return labels, counts


def post_process_mesh(vertices, tri, cluster_to_keep=1000):
    """post_process_mesh (utils/mesh_utils.py:30-51) with cluster_to_keep clamped to the number of clusters: (vertices, triangles, kept
    vertex ids, kept triangle ids), survivors in their original order."""
    labels, counts = components(len(vertices), tri)
    has = counts[counts > 0]
    k = min(cluster_to_keep, len(has))
    n = np.sort(has)[-k] if k > 0 else 0
    n = max(int(n), 50)
    keep_t = counts[labels[tri[:, 0]]] >= n if len(tri) else np.zeros(0, bool)
    keep_v = counts[labels] >= n
    remap = np.cumsum(keep_v) - 1
    return vertices[keep_v], remap[tri[keep_t]], np.nonzero(keep_v)[0], np.nonzero(keep_t)[0]


# ---- the depth maps of the GPU tests ------------------------------------------------------------------------------------------------
def analytic_depth(cam, H, W, radius=0.5, background=3.1):
    """fp32 view depth of the sphere |x| = radius seen through the centres of the H x W pixels (align_corners: pixel (u, v) is
    ndc (2u / (W-1) - 1, 2v / (H-1) - 1)), `background` elsewhere."""
    wvt = cam.world_view_transform.double().numpy()
    c = wvt[3, :3]                                                 # the world origin in view space
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([(2 * u / (W - 1) - 1) * np.tan(0.5 * cam.FoVx), (2 * v / (H - 1) - 1) * np.tan(0.5 * cam.FoVy), np.ones((H, W))], axis=-1)
    dd, dc = (d * d).sum(-1), d @ c
    disc = dc * dc - dd * (c @ c - radius * radius)
    s = (dc - np.sqrt(np.maximum(disc, 0))) / dd
    return np.where(disc > 0, s, background).astype(np.float32)


# ---- the fields of the self-test and of the GPU tests ------------------------------------------------------------------------------
ORG = np.array([-0.79, -0.71, -0.87], np.float32).astype(np.float64)
SPACING = np.full(3, np.float32(0.04), np.float64)
SHAPE = (40, 36, 44)


def lattice_points(origin=ORG, spacing=SPACING, shape=SHAPE):
    return (origin + spacing * lattice_index(shape)).reshape(*shape, 3)


def field_sphere(p, centre=(0.0, 0.0, 0.0), r=0.5):
    return np.linalg.norm(p - np.asarray(centre), axis=-1) - r


def field_torus(p):
    return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 2] ** 2) - 0.45) ** 2 + p[..., 1] ** 2) - 0.17


def field_two_spheres(p):
    return np.minimum(field_sphere(p, (0.3, 0.0, 0.0), 0.25), field_sphere(p, (-0.35, -0.1, -0.2), 0.13))


KNOWN = {"sphere": (field_sphere, 8840, 17676, 2, 1), "torus": (field_torus, 8208, 16416, 0, 1),
         "two_spheres": (field_two_spheres, 2740, 5472, 4, 2)}


def known_field(name):
    """The field on the float64 lattice (-0.79, -0.71, -0.87) + 0.04 (i, j, k), cast to fp32 (a cast keeps every sign)."""
    return KNOWN[name][0](lattice_points(np.array([-0.79, -0.71, -0.87]), np.full(3, 0.04))).astype(np.float32)


def self_test():
    for name, (fn, V, T, chi, ncomp) in KNOWN.items():
        F = known_field(name)
        assert np.abs(F).min() > 0, name                                # no lattice point on the surface: no zero-area triangle
        mt = marching_tetrahedra(F, 0.0, ORG, SPACING, return_flips=True)
        v, t = mt["vertices"], mt["triangles"]
        assert (len(v), len(t)) == (V, T), (name, len(v), len(t))
        und, directed = edge_census(t)
        assert (und == 2).all() and (directed == 1).all(), name
        assert len(v) - len(und) + len(t) == chi, name
        assert components(len(v), t)[1].size == ncomp, name
        area = np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)
        assert (area > 0).all(), name
        assert (mt["flip"] == mt["flip_predicted"]).all(), name        # the parity rule agrees with the geometry
        # outward: the signed volume is positive
        vol = np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6
        assert vol > 0, name
    return True
