"""What materialrefgs_amd.ballquery and the pooling of materialrefgs_amd.refscore compute, stated without any search structure (no reference
code here): chunked numpy float32 brute force.  numpy's float32 arithmetic rounds after every operation -- it never fuses a product into a
sum -- so these values are the un-fused fp32 form bit for bit, which is what csrc/mrgs_ballquery.hip is pinned to.

  d(q, k)  = (dx dx + dy dy) + dz dz, dx = fl(q.x - p_k.x), ...; r = float32(radius), r2 = fl(r r); a hit is d < r2, strictly (a
             comparison with a NaN is false).
  ball_query: per query the first nsample hits in ascending index order, padded with the first of them; no hit: zeros.
  furthest_point_sample: idx[0] = 0, temp = 1e10; per pick the points with float32 (x x + y y) + z z > 1e-3 (compared in double) take
             temp = fmin(temp, d(p_old, p_k)); the pick is the eligible point of largest temp, ties to the lowest index, 0 without one.
  pooling:   pooled[j] = fmax over score[row of ball_query(points, points)]; with a mask the masked-out rows take no part and keep their
             score, and a masked-in row without a hit keeps its own.
  points:    in float64, ((x - Cx) / Fx z, (y - Cy) / Fy z, z), then (p - T) @ R^T.
"""
import numpy as np

F32 = np.float32
PAIRS_PER_CHUNK = 1 << 22


def dist2(q, p):
    """[M,3] x [N,3] float32 -> [M,N] float32."""
    q, p = np.asarray(q, dtype=F32), np.asarray(p, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[:, None, k] - p[None, :, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def radius2(radius):
    r = F32(radius)
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(r * r)


def _rows(r2, nsample, xyz, new_xyz):
    """One batch: (idx int32 [M,nsample], number of hits int64 [M])."""
    N, M = len(xyz), len(new_xyz)
    idx = np.zeros((M, nsample), dtype=np.int32)
    hits = np.zeros(M, dtype=np.int64)
    if N == 0:
        return idx, hits
    step = max(1, PAIRS_PER_CHUNK // N)
    slots = np.arange(nsample)[None, :]
    for a in range(0, M, step):
        with np.errstate(invalid="ignore"):
            hit = dist2(new_xyz[a:a + step], xyz) < r2
        order = np.cumsum(hit, axis=1)
        rows, cols = np.nonzero(hit & (order <= nsample))
        part = np.zeros((hit.shape[0], nsample), dtype=np.int32)
        part[rows, order[rows, cols] - 1] = cols
        total = order[:, -1]
        pad = slots >= np.minimum(total, nsample)[:, None]
        part[pad] = np.broadcast_to(part[:, :1], part.shape)[pad]
        idx[a:a + step], hits[a:a + step] = part, total
    return idx, hits


def ball_query(radius, nsample, xyz, new_xyz, return_hits=False):
    """xyz [B,N,3], new_xyz [B,M,3] -> int32 [B,M,nsample] (and the number of hits of every query, int64 [B,M])."""
    xyz, new_xyz = np.asarray(xyz, dtype=F32), np.asarray(new_xyz, dtype=F32)
    r2 = radius2(radius)
    out = [_rows(r2, nsample, x, q) for x, q in zip(xyz, new_xyz)]
    idx = np.stack([o[0] for o in out]) if out else np.zeros((0, new_xyz.shape[1], nsample), np.int32)
    hits = np.stack([o[1] for o in out]) if out else np.zeros((0, new_xyz.shape[1]), np.int64)
    return (idx, hits) if return_hits else idx


def row_kinds(hits, nsample):
    """Shares of the queries without a hit, with 1 .. nsample-1 hits (nsample = 1: exactly one), and with nsample or more."""
    hits = np.asarray(hits).reshape(-1)
    if nsample == 1:
        return float(np.mean(hits == 0)), float(np.mean(hits == 1)), float(np.mean(hits > 1))
    return float(np.mean(hits == 0)), float(np.mean((hits > 0) & (hits < nsample))), float(np.mean(hits >= nsample))


def furthest_point_sample(xyz, npoint, return_span=False):
    """xyz [B,N,3] -> int32 [B,npoint] (and float32 [B]: |p[idx[0]] - p[idx[1]]|, 0 with fewer than two picks)."""
    xyz = np.asarray(xyz, dtype=F32)
    B, N, _ = xyz.shape
    idx = np.zeros((B, npoint), dtype=np.int32)
    span = np.zeros(B, dtype=F32)
    for b in range(B):
        p = xyz[b]
        with np.errstate(invalid="ignore", over="ignore"):
            mag = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
            eligible = mag.astype(np.float64) > 1e-3
        temp = np.full(N, 1e10, dtype=F32)
        for j in range(1, npoint):
            d = dist2(p[idx[b, j - 1]][None], p)[0]
            temp[eligible] = np.fmin(temp[eligible], d[eligible])
            if eligible.any():
                cand = np.where(eligible, temp, F32(-1.0))
                idx[b, j] = int(np.argmax(cand))                       # argmax returns the first of equal maxima: the lowest index
        if npoint >= 2:
            with np.errstate(invalid="ignore"):
                span[b] = np.sqrt(dist2(p[idx[b, 0]][None], p[idx[b, 1]][None])[0, 0])
    return (idx, span) if return_span else idx


def max_pool(points, score, r, nsample, valid=None):
    """points [N,3], score [N], r the float32 radius, valid [N] bool or None -> pooled float32 [N]."""
    points, score = np.array(points, dtype=F32), np.asarray(score, dtype=F32)
    if valid is not None:
        valid = np.asarray(valid).astype(bool)
        points[~valid, 0] = np.nan                                       # never hits, is never hit
    idx, hits = ball_query(r, nsample, points[None], points[None], return_hits=True)
    pooled = np.fmax.reduce(score[idx[0]], axis=1)
    if valid is not None:
        pooled = np.where(hits[0] == 0, score, pooled)
    return pooled.astype(F32)


def fps_radius(points, ratio):
    """float32: |p[f0] - p[f1]| * float32(ratio) with f = furthest_point_sample(points, 2)."""
    _idx, span = furthest_point_sample(np.asarray(points, dtype=F32)[None], 2, return_span=True)
    with np.errstate(invalid="ignore"):
        return F32(span[0] * F32(ratio))


def points64(cams, depths, focal):
    """float64 [V*H*W, 3]; cams carry R [3,3], T [3], image_height, image_width; focal(cam) -> (Fx, Fy, Cx, Cy); depths [V][H*W]."""
    out = []
    for cam, depth in zip(cams, depths):
        H, W = int(cam.image_height), int(cam.image_width)
        fx, fy, cx, cy = focal(cam)
        z = np.asarray(depth, dtype=np.float64).reshape(H, W)
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        p = np.stack([(x - cx) / fx * z, (y - cy) / fy * z, z], axis=-1).reshape(-1, 3)
        R, T = np.asarray(cam.R, dtype=np.float64), np.asarray(cam.T, dtype=np.float64)
        out.append((p - T) @ R.T)
    return np.concatenate(out, axis=0)
