"""What materialrefgs_amd.knn.distCUDA2 computes, stated twice without any search structure (no reference code here):

statement32: the float32 brute force of the definition -- per pair d = (dx dx + dy dy) + dz dz with dx = q.x - p.x in float32, un-fused
(numpy never contracts), the pair (i, i) replaced by FLT_MAX ("other" is decided by index), the three smallest b0 <= b1 <= b2 per row
(missing ones FLT_MAX) and ((b0 + b1) + b2) / 3 with an IEEE quotient.  The HIP kernels must equal it bit for bit.
truth64: the same quantity from scipy's k-d tree on the float32 inputs widened to float64."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def statement32(points, chunk=512):
    p = np.ascontiguousarray(points, dtype=np.float32)
    P = p.shape[0]
    out = np.empty(P, dtype=np.float32)
    with np.errstate(over="ignore"):
        for s in range(0, P, chunk):
            q = p[s:s + chunk]
            n = q.shape[0]
            dx, dy, dz = (q[:, None, k] - p[None, :, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            d[np.arange(n), np.arange(s, s + n)] = FLT_MAX          # the self column
            if P < 3:
                d = np.concatenate([d, np.full((n, 3 - P), FLT_MAX, dtype=np.float32)], axis=1)
            b = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
            out[s:s + n] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3)
    return out


def truth64(points):
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, dtype=np.float32).astype(np.float64)
    d, _ = cKDTree(p).query(p, k=4, workers=4)
    return (d[:, 1:] ** 2).sum(axis=1) / 3.0      # column 0 is one zero: the point itself or a duplicate of it
