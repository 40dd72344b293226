"""Torch statement on the CPU of EnvGaussianModel.densify_and_prune (scene/env_gaussian_model.py:384-597) as the literal six-stage chain
-- clone and cat, split in 2 with cat and prune, opacity prune, quantile-of-weights prune with split in 5, top-k visibility cap, reset --
with boolean indexing, and of add_densification_stats (:600-603).  The GPU tests compare materialrefgs_amd.env_model against it.

Conventions (include/mrgs.h): the standard normals are arguments, `noise` [P, 2, 2] for stage 2 (child k of source row i uses noise[i, k])
and `noise4` [P, 4, 5, 2] for stage 4 (child j of slot sigma of source row i uses noise4[i, sigma, j]; sigma = 0 original, 1 clone, 2 + k
stage-2 child k).  Parameters, moments and the scale / opacity / gradient decisions are carried in float64, so copied rows stay exact
images of their float32 sources.  The WEIGHT path (xyz_weight_accum, the three maxima, the products, weight / denom, the quantile, the
top-k set) and the RADIUS path (max_radii2D and its ratios) are carried in float32 with one torch op per rounded operation: they are
compared exactly, without a margin.  Bookkeeping columns travel with the rows like parameters: `row` (source row), `slot` (sigma), `gen`
(splits behind the row: 0, 1 or 2), `child4` (stage-4 child index, -1 otherwise) and `xyz_bound` (the bound of the centre, see split)."""
from types import SimpleNamespace

import numpy as np
import torch

from densify_statement import build_rotation

F32 = torch.float32
ULP16 = 16 * 2.0 ** -24                   # tests/test_densify.py: one generation of a child's centre, relative to |parent| + |offset|
SCALING_REL = 1e-6                        # ... of a child's raw scaling, relative to max(|value|, 1)
BOOK = ("row", "slot", "gen", "child4", "xyz_bound")


def _rel(q, thr):
    q = q.double()
    return float(((q - thr).abs() / abs(thr)).min()) if q.numel() else float("inf")


def quantile_rule(v, qf=0.1):
    """The 0.1 quantile of the float32 vector v, every operation rounded to float32 on its own (include/mrgs.h)."""
    v = v.reshape(-1).to(F32)
    n = v.numel()
    s = torch.sort(v).values
    rank = torch.tensor(qf, dtype=F32) * torch.tensor(float(n - 1), dtype=F32)
    lo, hi = torch.floor(rank), torch.ceil(rank)
    f = rank - lo
    v_lo, v_hi = s[int(lo)], s[int(hi)]
    diff = v_hi - v_lo
    if float(f) < 0.5:
        return v_lo + f * diff
    return v_hi - diff * (torch.tensor(1.0, dtype=F32) - f)


class _State:
    def __init__(self, params, moments, accum, denom, radii, weight):
        P = params["xyz"].shape[0]
        self.t = {k: v.detach().cpu().double() for k, v in params.items()}
        self.t["row"] = torch.arange(P, dtype=torch.float64).reshape(P, 1)
        for k in ("slot", "gen", "xyz_bound"):
            self.t[k] = torch.zeros(P, 1, dtype=torch.float64)
        self.t["child4"] = torch.full((P, 1), -1.0, dtype=torch.float64)
        self.m = None if moments is None else {k: tuple(x.detach().cpu().double() for x in mv) for k, mv in moments.items()}
        self.a = accum.detach().cpu().double().reshape(P, 1)
        self.d = denom.detach().cpu().to(F32).reshape(P, 1)
        self.r = radii.detach().cpu().to(F32).reshape(P)
        self.w = weight.detach().cpu().to(F32).reshape(P, 1)

    n = property(lambda s: s.t["xyz"].shape[0])
    scale = property(lambda s: torch.exp(s.t["scaling"]))
    smax = property(lambda s: s.scale.max(dim=1).values)

    def grads(self):
        g = self.a / self.d.double()
        g[g.isnan()] = 0.0
        return g

    def wavg(self):
        avg = self.w / self.d
        avg[avg.isnan()] = 0.0
        return avg

    def cat(self, ext):                                         # cat_tensors_to_optimizer: zero moments for the new rows
        for k in self.t:
            if self.m is not None and k in self.m:
                self.m[k] = tuple(torch.cat((x, torch.zeros_like(ext[k])), dim=0) for x in self.m[k])
            self.t[k] = torch.cat((self.t[k], ext[k]), dim=0)

    def densify_stats(self, mask, split, ratio):               # :384-392
        self.a = torch.cat([self.a, self.a[mask].repeat(split, 1) * ratio], dim=0)
        new_w = self.w[mask].repeat(split, 1) * self.w.max()
        self.d = torch.cat([self.d, self.d[mask].repeat(split, 1)], dim=0)
        self.r = torch.cat([self.r, self.r[mask].repeat(split) * torch.tensor(ratio, dtype=F32)], dim=0)
        self.w = torch.cat([self.w, new_w], dim=0)

    def prune(self, mask):                                      # prune_points
        keep = ~mask
        for k in self.t:
            self.t[k] = self.t[k][keep]
            if self.m is not None and k in self.m:
                self.m[k] = tuple(x[keep] for x in self.m[k])
        self.a, self.d, self.r, self.w = self.a[keep], self.d[keep], self.r[keep], self.w[keep]

    def split(self, mask, N, div, z, stage4):
        """Replace the rows of `mask` by N children each (child-major), z [n_split, N, 2]."""
        n_split = int(mask.sum())
        stds = self.scale[mask].repeat(N, 1)
        zz = torch.cat([z[:, k] for k in range(N)], dim=0)
        samples = torch.cat([stds * zz, torch.zeros_like(stds[:, :1])], dim=-1)
        rots = build_rotation(self.t["rotation"][mask]).repeat(N, 1, 1)
        offset = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1)
        ext = {k: v[mask].repeat(N, *([1] * (v.dim() - 1))) for k, v in self.t.items()}
        parent = self.t["xyz"][mask].repeat(N, 1)
        ext["xyz"] = offset + parent
        ext["scaling"] = torch.log(self.scale[mask].repeat(N, 1) / div)
        # the centre's bound: a generation costs 16 roundings of |parent| + |offset|; a second generation also carries its source's
        # scaling bound through the offset
        omax = offset.abs().max(dim=1, keepdim=True).values
        ext["xyz_bound"] = ext["xyz_bound"] + ULP16 * (parent.abs().max(dim=1, keepdim=True).values + omax) + ext["gen"] * SCALING_REL * omax
        ext["gen"] = ext["gen"] + 1.0
        idx = torch.cat([torch.full((n_split, 1), float(k), dtype=torch.float64) for k in range(N)], dim=0)
        if stage4:
            ext["child4"] = idx
        else:
            ext["slot"] = 2.0 + idx
        self.cat(ext)
        self.densify_stats(mask, N, 1.0 / div)
        self.prune(torch.cat((mask, torch.zeros(N * n_split, dtype=torch.bool))))


def densify_and_prune(params, moments, accum, denom, max_radii2D, weight_accum, percent_dense, max_grad, min_opacity, extent,
                      max_screen_size, noise, noise4, max_gs=2e6, max_gs_threshold=0.9):
    """params: name -> [P, ...] (xyz [P,3], scaling [P,2], rotation [P,4], opacity [P,1] among them); moments: name -> (exp_avg, exp_avg_sq)
    or None.  Returns the resulting tensors / moments, the bookkeeping columns, what each stage did, q / W0 / W1 / W4 (float32) and
    `margin`: the smallest relative distance of g, max(s) of every generation, o and the radius (against max_screen_size) from their
    thresholds."""
    assert max_grad > 0
    st = _State(params, moments, accum, denom, max_radii2D, weight_accum)
    P = st.n
    noise = noise.detach().cpu().double().reshape(P, 2, 2)
    noise4 = noise4.detach().cpu().double().reshape(P, 4, 5, 2)
    t = percent_dense * extent
    info = SimpleNamespace(q=None, W0=None, W1=None, W4=None, n_clone=0, n_split=0, n_stage3=0, n_pruned4=0, n_split4=0, n_pruned5=0,
                           wavg4=None, low=None)
    g = st.grads()
    margins = [_rel(g[torch.isfinite(g)], max_grad), _rel(st.smax, t)]

    # stage 1: clone (densify_and_clone :456-470)
    clone = (torch.norm(g, dim=-1) >= max_grad) & (st.smax <= t)
    ext = {k: v[clone] for k, v in st.t.items()}
    ext["slot"] = torch.ones_like(ext["slot"])
    info.W0 = st.w.max() if P else None
    st.cat(ext)
    st.densify_stats(clone, 1, 1.0)
    info.n_clone = int(clone.sum())

    # stage 2: split in 2 (densify_and_split :398-432); the clones carry their sources' accum / denom, but max(s) <= t
    g = st.grads()
    split = (st.smax > t) & (g >= max_grad).squeeze(-1)
    info.n_split = int(split.sum())
    if info.n_split > 0:
        info.W1 = st.w.max()
        st.split(split, 2, 0.8 * 2, noise[st.t["row"][split].squeeze(-1).long()], stage4=False)

    # stage 3: opacity (prune_min_opacity_and_gradients :484-511, min_gradient None)
    opac = torch.sigmoid(st.t["opacity"])
    margins.append(_rel(opac, min_opacity))
    st.prune((opac < min_opacity).squeeze(-1))
    info.n_stage3 = st.n

    # stage 4: scene / screen with the quantile of the weights (prune_max_scene_and_screen :513-558)
    if st.n > 0:
        weights = st.wavg()
        info.q = quantile_rule(weights)
        big = st.smax > extent * 0.1
        margins.append(_rel(st.smax, extent * 0.1))
        if max_screen_size is not None:
            big = big | (st.r > max_screen_size)
            margins.append(_rel(st.r, max_screen_size))
        low = (weights < info.q).squeeze(-1)
        info.wavg4, info.low = weights.squeeze(-1).clone(), low.clone()
        prune_mask = big & low
        split_mask = (big & ~low)[~prune_mask]
        info.n_pruned4, info.n_split4 = int(prune_mask.sum()), int(split_mask.sum())
        if info.n_pruned4 > 0:
            st.prune(prune_mask)
        if info.n_split4 > 0:
            info.W4 = st.w.max()
            rows, slots = st.t["row"][split_mask].squeeze(-1).long(), st.t["slot"][split_mask].squeeze(-1).long()
            st.split(split_mask, 5, 0.5 * 5, noise4[rows, slots], stage4=True)
            margins.append(_rel(st.smax, extent * 0.1))            # (no later decision reads it; kept for the margin's definition)

    # stage 5: the visibility cap (prune_visibility :560-573); ties: the earlier row goes first
    n_after = int(max_gs * max_gs_threshold)
    n_prune = st.n - n_after
    info.wavg5 = st.wavg().squeeze(-1).clone()
    if n_prune > 0:
        order = torch.sort(info.wavg5, stable=True).indices
        mask = torch.zeros(st.n, dtype=torch.bool)
        mask[order[:n_prune]] = True
        info.cut = info.wavg5[order[n_prune - 1]]
        st.prune(mask)
        info.n_pruned5 = n_prune

    # stage 6: reset
    book = {k: st.t.pop(k).squeeze(-1) for k in BOOK}
    rows_out = st.n
    return SimpleNamespace(tensors=st.t, moments=st.m, clone=clone, row=book["row"].long(), slot=book["slot"].long(), gen=book["gen"].long(),
                           child4=book["child4"].long(), xyz_bound=book["xyz_bound"], rows=rows_out, margin=min(margins), info=info,
                           stats=(torch.zeros(rows_out, 1), torch.zeros(rows_out, 1), torch.zeros(rows_out, 1), torch.zeros(rows_out)))


def segments(ref):
    """Rows per output segment (kept slot sigma: sigma; stage-4 child j of slot sigma: 4 + 4 j + sigma) and that the order is segment-major
    with ascending source rows inside a segment."""
    seg = torch.where(ref.child4 < 0, ref.slot, 4 + 4 * ref.child4 + ref.slot)
    key = seg * (1 << 40) + ref.row
    assert bool((key[1:] > key[:-1]).all())
    return tuple(int((seg == s).sum()) for s in range(24))


def add_densification_stats(accum, denom, weight_accum, grad, update_filter, weight_accumulate=None):
    """The three vectors after the call (float64 copies; weight_accum untouched when weight_accumulate is None)."""
    accum, denom, weight_accum = (x.detach().cpu().double().clone() for x in (accum, denom, weight_accum))
    f = update_filter.detach().cpu().bool()
    g = grad.detach().cpu().double()
    accum[f] += torch.norm(g[f], dim=-1, keepdim=True)
    denom[f] += 1
    if weight_accumulate is not None:
        weight_accum[f] += weight_accumulate.detach().cpu().double().reshape(-1, 1)[f]
    return accum, denom, weight_accum


# ---- the counter generator (include/mrgs.h): Philox4x32-10, key = seed, counter = (row lo, row hi, child, c3) ----------------------------
def philox_words(seed, c0, c1, c2, c3):
    """The four output words for arrays (or scalars) of 32-bit counter words."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    mask = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def philox_normals(seed, rows, child, c3=0):
    """z [n, 2] float64 for source rows `rows`: stage 2 uses (child k, c3 = 0), stage 4 (child j, c3 = 1 + sigma)."""
    rows = np.asarray(rows, dtype=np.uint64)
    c = philox_words(seed, rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), np.uint64(child), np.uint64(c3))
    u0 = ((c[0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u1 = ((c[1] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u0))
    return np.stack([r * np.cos(2 * np.pi * u1), r * np.sin(2 * np.pi * u1)], axis=-1)
