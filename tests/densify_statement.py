"""Float64 torch statement of GaussianModel.densify_and_prune (scene/gaussian_model.py:975-1057) as the literal three-stage sequence --
clone and cat, split with cat and prune, final prune -- with boolean indexing on the CPU, and of the two per-iteration statistics lines
(:1059-1061 and the max_radii2D line of the training loops).  The GPU tests compare materialrefgs_amd.densify against it.

Conventions (include/mrgs.h): the split's standard normals are an argument, `noise` [P, N, 2] indexed by SOURCE row (child k of row i
uses noise[i, k]); every tensor is carried in float64, so copied rows stay exact images of their float32 sources.  Two bookkeeping
columns travel with the rows like parameters: `row` (the source row) and `kind` (0 original, 1 clone, 2 + k child k).
"""
from types import SimpleNamespace

import torch

SPATIAL = ("xyz", "scaling", "rotation", "opacity")


def build_rotation(q):
    """utils/general_utils.py build_rotation: rows (w, x, y, z), normalised here."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros(q.shape[0], 3, 3, dtype=q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _rel(q, thr):
    return float(((q - thr).abs() / abs(thr)).min()) if q.numel() else float("inf")


class _State:
    """The model's per-gaussian tensors and their Adam moments (None before the first step)."""

    def __init__(self, params, moments):
        P = params["xyz"].shape[0]
        self.t = {k: v.detach().cpu().double() for k, v in params.items()}
        self.t["row"] = torch.arange(P, dtype=torch.float64).reshape(P, 1)
        self.t["kind"] = torch.zeros(P, 1, dtype=torch.float64)
        self.m = None if moments is None else {k: tuple(x.detach().cpu().double() for x in mv) for k, mv in moments.items()}

    scale = property(lambda s: torch.exp(s.t["scaling"]))

    def cat(self, ext):                                         # cat_tensors_to_optimizer: zero moments for the new rows
        for k in self.t:
            if self.m is not None and k in self.m:
                self.m[k] = tuple(torch.cat((x, torch.zeros_like(ext[k])), dim=0) for x in self.m[k])
            self.t[k] = torch.cat((self.t[k], ext[k]), dim=0)

    def prune(self, mask):                                      # prune_points
        keep = ~mask
        for k in self.t:
            self.t[k] = self.t[k][keep]
            if self.m is not None and k in self.m:
                self.m[k] = tuple(x[keep] for x in self.m[k])


def densify_and_prune(params, moments, accum, denom, percent_dense, max_grad, min_opacity, extent, max_screen_size, noise, N=2):
    """params: name -> [P, ...] (must hold xyz [P,3], scaling [P,2], rotation [P,4], opacity [P,1]); moments: name -> (exp_avg, exp_avg_sq)
    or None.  Returns the resulting tensors / moments, the decision masks over the source rows, the three counts, the bookkeeping
    columns and `margin`: the smallest relative distance of any decision quantity (g, max(s), a child's max(s), o) from its threshold."""
    assert max_grad > 0
    st = _State(params, moments)
    P = st.t["xyz"].shape[0]
    noise = noise.detach().cpu().double().reshape(P, N, 2)
    t = percent_dense * extent
    grads = accum.detach().cpu().double().reshape(P, 1) / denom.detach().cpu().double().reshape(P, 1)
    grads[grads.isnan()] = 0.0
    margins = [_rel(grads[torch.isfinite(grads)], max_grad), _rel(st.scale.max(dim=1).values, t)]

    # stage 1: clone and cat
    clone = (torch.norm(grads, dim=-1) >= max_grad) & (st.scale.max(dim=1).values <= t)
    ext = {k: v[clone] for k, v in st.t.items()}
    ext["kind"] = torch.ones_like(ext["kind"])
    st.cat(ext)

    # stage 2: split with cat and prune (the clones carry g = 0)
    n = st.t["xyz"].shape[0]
    padded = torch.zeros(n, dtype=torch.float64)
    padded[:P] = grads.squeeze(-1)
    split = (padded >= max_grad) & (st.scale.max(dim=1).values > t)
    rows = st.t["row"][split].squeeze(-1).long()
    stds = st.scale[split].repeat(N, 1)
    z = torch.cat([noise[rows, k] for k in range(N)], dim=0)
    samples = torch.cat([stds * z, torch.zeros_like(stds[:, :1])], dim=-1)
    rots = build_rotation(st.t["rotation"][split]).repeat(N, 1, 1)
    offset = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1)
    ext = {k: v[split].repeat(N, *([1] * (v.dim() - 1))) for k, v in st.t.items()}
    ext["xyz"] = offset + st.t["xyz"][split].repeat(N, 1)
    ext["scaling"] = torch.log(st.scale[split].repeat(N, 1) / (0.8 * N))
    ext["kind"] = torch.cat([torch.full((int(split.sum()), 1), 2.0 + k, dtype=torch.float64) for k in range(N)], dim=0)
    n_new = ext["xyz"].shape[0]
    st.cat(ext)
    st.prune(torch.cat((split, torch.zeros(n_new, dtype=torch.bool))))
    offset_norm = torch.cat((torch.zeros(st.t["xyz"].shape[0] - n_new), offset.abs().max(dim=1).values if n_new else torch.zeros(0)))

    # stage 3: the final prune over every row now present (max_radii2D has been zeroed by the two postfixes above)
    opac = torch.sigmoid(st.t["opacity"])
    margins.append(_rel(opac, min_opacity))
    prune = (opac < min_opacity).squeeze(-1)
    if max_screen_size:
        max_radii2D = torch.zeros(st.t["xyz"].shape[0], dtype=torch.float64)
        big_vs = max_radii2D > max_screen_size
        big_ws = st.scale.max(dim=1).values > 0.1 * extent
        margins.append(_rel(st.scale.max(dim=1).values, 0.1 * extent))
        prune = prune | big_vs | big_ws
    st.prune(prune)
    offset_norm = offset_norm[~prune]

    kind = st.t.pop("kind").squeeze(-1).long()
    row = st.t.pop("row").squeeze(-1).long()
    n_keep, n_clone = int((kind == 0).sum()), int((kind == 1).sum())
    n_child = int((kind == 2).sum())
    assert all(int((kind == 2 + k).sum()) == n_child for k in range(N))
    rows_out = st.t["xyz"].shape[0]
    return SimpleNamespace(tensors=st.t, moments=st.m, clone=clone, split=split[:P], counts=(n_keep, n_clone, n_child), row=row, kind=kind,
                           offset_norm=offset_norm, margin=min(margins),
                           stats=(torch.zeros(rows_out, 1, dtype=torch.float64), torch.zeros(rows_out, 1, dtype=torch.float64),
                                  torch.zeros(rows_out, dtype=torch.float64)))


def add_densification_stats(accum, denom, max_radii2D, grad, update_filter, radii=None):
    """Returns the three vectors after the two lines of the loop (float64 copies; max_radii2D untouched when radii is None)."""
    accum, denom = accum.detach().cpu().double().clone(), denom.detach().cpu().double().clone()
    max_radii2D = None if max_radii2D is None else max_radii2D.detach().cpu().double().clone()
    f = update_filter.detach().cpu().bool()
    g = grad.detach().cpu().double()
    if radii is not None:
        max_radii2D[f] = torch.max(max_radii2D[f], radii.detach().cpu().double()[f])
    accum[f] += torch.norm(g[f], dim=-1, keepdim=True)
    denom[f] += 1
    return accum, denom, max_radii2D


# ---- the counter generator of the split offsets (include/mrgs.h): Philox4x32-10, key = seed, counter = (row, child) --------------------
def philox_normals(seed, rows, k):
    """(u0 numerators, u1 numerators, z [n,2] float64) for source rows `rows` (numpy int array) and child index k."""
    import numpy as np
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    mask = np.uint64(0xFFFFFFFF)
    rows = np.asarray(rows, dtype=np.uint64)
    c = [rows & mask, rows >> np.uint64(32), np.full_like(rows, k), np.zeros_like(rows)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    n0 = (c[0] >> np.uint64(8)) + np.uint64(1)
    n1 = (c[1] >> np.uint64(8)) + np.uint64(1)
    u0, u1 = n0.astype(np.float64) * 2.0 ** -24, n1.astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u0))
    return n0, n1, np.stack([r * np.cos(2 * np.pi * u1), r * np.sin(2 * np.pi * u1)], axis=-1)
