"""Statement-side helpers of tests/test_envmap_seams.py: the cell probes, the roughness cycle, and where a set of directions fetches
(border / vertex classes, the rows too close to a decision for a per-row gradient).  Everything here is float64 on the CPU and goes
through oracle/shading_oracle.py; nothing here touches a kernel."""
import numpy as np
import torch

from oracle import shading_oracle as so

F64 = torch.float64
CELL_MARGIN = 1e-3          # texels: a tap coordinate closer than this to an integer may floor the other way in fp32
FACE_MARGIN = 1e-4          # (|major| - |second|) / |major| below this: fp32 may select the other face
KNOT_MARGIN = 1e-4          # levels: the mip level closer than this to an integer (or the roughness on a clamp) is "on a knot"
VERTEX_OFFSETS = ((0.25, 0.6), (0.7, 0.35), (0.45, 0.8), (0.85, 0.15), (0.3, 0.55), (0.6, 0.9))    # in half texels, u never equal to v


def cell_probes(res, n_along=16):
    """Directions well inside the border and vertex CELLS of a res^2 level (and of every coarser level of a chain below it): on each
    face, for each of the four sides, u or v a quarter texel inside the border (+-(1 - 0.5 / res)) and the other coordinate spread over
    +-0.9 (n_along positions, jittered so that none sits on a texel centre of a level); for each of the four corners, both coordinates
    inside the last half texel (VERTEX_OFFSETS).  [6 * (4 n_along + 4 * 6), 3] float64, through so.cube_to_dir."""
    rng = np.random.default_rng(1000 + res)
    us, vs, faces = [], [], []
    for s in range(6):
        for side in range(4):
            t = np.linspace(-0.9, 0.9, n_along) + rng.uniform(-0.02, 0.02, n_along)
            a = np.full(n_along, (1 - 0.5 / res) * (1 if side & 1 else -1))
            u, v = (a, t) if side < 2 else (t, a)
            us.append(u); vs.append(v); faces.append(np.full(n_along, s))
        for su in (-1, 1):
            for sv in (-1, 1):
                o = np.array(VERTEX_OFFSETS)
                us.append(su * (1 - o[:, 0] / res)); vs.append(sv * (1 - o[:, 1] / res)); faces.append(np.full(len(o), s))
    u, v, face = (torch.tensor(np.concatenate(x)) for x in (us, vs, faces))
    d = torch.zeros(u.shape[0], 3, dtype=F64)
    for s in range(6):
        m = face == s
        d[m] = so.cube_to_dir(s, u[m].to(F64), v[m].to(F64))
    return d


def level_roughness(level, n, lo=0.08, hi=0.5):
    """Inverse of so.get_mip on its two linear pieces (n >= 2; level in [0, n - 1])."""
    if n > 2 and level <= n - 2:
        return lo + level / (n - 2) * (hi - lo)
    return hi + (level - (n - 2)) * (1.0 - hi)


def roughness_cycle(n, lo=0.08, hi=0.5):
    """The roughness values a chain of n levels is probed with, as float32: below min_roughness, every integer level, every half level,
    max_roughness, 1, above 1.  A single level (n = 1) is fetched without roughness."""
    if n == 1:
        return None
    r = [0.02] + [level_roughness(float(l), n, lo, hi) for l in range(n)] + [level_roughness(l + 0.5, n, lo, hi) for l in range(n - 1)]
    return np.unique(np.array(r + [hi, 1.0, 1.3], np.float32))


def probe_rows(res_list, n_along=16):
    """Every cell probe of the finest level with every roughness of the cycle: dirs [N,3] float32, roughness [N] float32 or None."""
    d = cell_probes(res_list[0], n_along).to(torch.float32)
    cyc = roughness_cycle(len(res_list))
    if cyc is None:
        return d, None
    r = torch.tensor(cyc)
    return d.repeat_interleave(len(r), dim=0), r.repeat(d.shape[0])


def level_shares(rough, n, lo=0.08, hi=0.5):
    """share[l, row] of level l in a fetch (float64): (1 - f) at l0 and f at l1, as so.env_lookup blends; and the rows on a knot (the
    level within KNOT_MARGIN of an integer or the roughness on one of get_mip's clamps), whose roughness gradient is one-sided."""
    if rough is None:
        return None, None
    rough = rough.to(F64)
    level = so.get_mip(rough, n, lo, hi)
    lc = torch.clamp(level, 0, n - 1)
    share = torch.stack([torch.clamp(1 - (lc - l).abs(), min=0) for l in range(n)])
    knot = (rough > lo) & (rough < 1.0) & ((lc - torch.round(lc)).abs() < KNOT_MARGIN)          # (a clamped roughness has slope zero)
    for k in (lo, hi, 1.0):
        knot |= (rough - k).abs() < 1e-6
    return share, knot


def classify(res_list, dirs, rough, lo=0.08, hi=0.5):
    """Where the rows fetch, from the float64 statement on the rows' own (float32) values.  Returns dict:
      keep [N] bool:  the row's per-row gradients can be compared (no tap coordinate of a used level within CELL_MARGIN of an integer,
                      face_gap >= FACE_MARGIN);
      knot [N] bool:  roughness on a knot (left out of g_roughness only);
      classes:        {(level index, 'e', face, side) | (level index, 'v', face, corner): [N] bool}, over the rows that use the level;
                      side 0..3 = x0 < 0, x0 + 1 >= res, y0 < 0, y0 + 1 >= res; corner = 2 * (x side) + (y side)."""
    dirs = dirs.to(F64)
    n = len(res_list)
    share, knot = level_shares(rough, n, lo, hi)
    N = dirs.shape[0]
    if share is None:
        share, knot = torch.ones(1, N, dtype=F64), torch.zeros(N, dtype=torch.bool)
    a = dirs.abs().topk(2, dim=1).values
    keep = (a[:, 0] - a[:, 1]) / a[:, 0] >= FACE_MARGIN
    classes = {}
    dist = lambda x: (x - torch.round(x)).abs()
    for li in range(share.shape[0]):
        res = res_list[li]
        used = share[li] > 0
        _, _, fx, fy, face = so.bilinear_taps(res, dirs)
        keep &= ~used | (torch.minimum(dist(fx), dist(fy)) >= CELL_MARGIN)
        x0, y0 = torch.floor(fx).long(), torch.floor(fy).long()
        sx = torch.where(x0 < 0, 0, torch.where(x0 + 1 >= res, 1, -1))
        sy = torch.where(y0 < 0, 0, torch.where(y0 + 1 >= res, 1, -1))
        for f in range(6):
            on = used & (face == f)
            for s in (0, 1):
                if res >= 2:
                    classes[(li, "e", f, s)] = on & (sx == s) & (sy < 0)
                    classes[(li, "e", f, 2 + s)] = on & (sy == s) & (sx < 0)
                for t in (0, 1):
                    classes[(li, "v", f, 2 * s + t)] = on & (sx == s) & (sy == t)
    return dict(keep=keep, knot=knot, classes=classes)


def coverage(cls, rows=None):
    """(share of rows left out, smallest class count among the kept rows, the class that has it)."""
    keep = cls["keep"] if rows is None else cls["keep"] & rows
    counts = {k: int((m & keep).sum()) for k, m in cls["classes"].items()}
    worst = min(counts, key=counts.get)
    return float((~cls["keep"]).double().mean()), counts[worst], worst
