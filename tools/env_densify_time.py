"""Times one EnvGaussianModel.densify_and_prune call and one add_densification_stats call (materialrefgs_amd/env_model.py on
csrc/mrgs_env_densify.hip; allocation of the outputs and the optimizer surgery included) at P = 300 000 and 1 000 000 rows carrying the
six groups of training_setup with both Adam moments, beside the literal torch chain on the same GPU in the same run: the reference's
statements in fp32 -- clone, split in 2, opacity prune, quantile prune with split in 5, top-k cap, reset; every cat and boolean prune over
all parameters, moments and the four statistics vectors -- with its .item() reads, and its three boolean-mask statistics lines.
The inputs are drawn from bands in which every stage fires and no decision sits on a threshold (as tests/test_env_densify.py), so both
forms must end with the same number of rows: asserted.  max_gs is set so that the cap removes ~5 % of the rows that reach it.
A densify call changes its model, so every repetition gets a fresh copy outside the timed window; the window is a host clock between two
device synchronisations (the call contains a host read by design), the two forms alternate, the first pair is the warm-up, the minimum
and every run are printed.  Per-kernel times:  rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/env_densify_time.py 300000
Developer tool; prints two lines per size."""
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd.env_model import EnvGaussianModel  # noqa: E402
from materialrefgs_amd.gs_utils import build_rotation  # noqa: E402

GROUPS = {"xyz": ("_xyz", (3,)), "f_dc": ("_features_dc", (1, 3)), "f_rest": ("_features_rest", (15, 3)), "opacity": ("_opacity", (1,)),
          "scaling": ("_scaling", (2,)), "rotation": ("_rotation", (4,))}
PERCENT_DENSE, EXTENT, MAX_GRAD, MIN_OPACITY, SCREEN = 0.01, 5.0, 5e-5, 0.05, 20
OPT = SimpleNamespace(position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
                      features_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3)


def source_tensors(P, dev):
    g = torch.Generator(device=dev).manual_seed(P)
    u = lambda *sh: torch.rand(*sh, generator=g, device=dev)
    pick = lambda probs: torch.multinomial(torch.tensor(probs, device=dev), P, replacement=True, generator=g)
    t = {n: torch.randn((P,) + sh, generator=g, device=dev) for n, (_a, sh) in GROUPS.items()}
    gc, sc = pick([0.45, 0.20, 0.35]), pick([0.50, 0.25, 0.15, 0.10])
    zero = torch.zeros(P, device=dev)
    gval = torch.where(gc == 0, zero, torch.where(gc == 1, 0.2 + 0.4 * u(P), 1.5 + 2.5 * u(P))) * MAX_GRAD
    denom = torch.randint(1, 6, (P,), generator=g, device=dev).float()
    denom = torch.where((gc == 0) & (u(P) < 0.1), zero, denom)                            # a few rows never seen
    lo, hi = torch.tensor([0.3, 2.0, 12.0, 30.0], device=dev)[sc], torch.tensor([0.7, 4.0, 15.0, 38.0], device=dev)[sc]
    smax = (lo + (hi - lo) * u(P)) * PERCENT_DENSE * EXTENT
    other, first = smax * (0.1 + 0.85 * u(P)), u(P) < 0.5
    t["scaling"] = torch.log(torch.stack([torch.where(first, smax, other), torch.where(first, other, smax)], dim=1))
    t["opacity"] = torch.where(u(P, 1) < 0.1, torch.full((P, 1), -4.0, device=dev), 0.5 + 2.0 * u(P, 1))
    mom = {n: (torch.randn(v.shape, generator=g, device=dev), torch.rand(v.shape, generator=g, device=dev)) for n, v in t.items()}
    stats = {"xyz_gradient_accum": (gval * denom).reshape(P, 1), "denom": denom.reshape(P, 1),
             "max_radii2D": torch.where(u(P) < 0.15, 60.0 + torch.floor(41.0 * u(P)), torch.floor(6.0 * u(P))),
             "xyz_weight_accum": (denom * (0.02 + 2.0 * u(P))).reshape(P, 1)}
    frame = SimpleNamespace(grad=torch.randn(P, 3, generator=g, device=dev) * 1e-3, vis=u(P) < 0.5, weight=u(P, 1))
    return t, mom, stats, frame


def fresh_model(t, mom, stats, max_gs):
    m = EnvGaussianModel(3)
    for n, (attr, _sh) in GROUPS.items():
        setattr(m, attr, torch.nn.Parameter(t[n].clone()))
    m.spatial_lr_scale = 1.0
    m.training_setup(OPT)
    m.max_gs = max_gs
    for gr in m.optimizer.param_groups:
        m.optimizer.state[gr["params"][0]] = {"step": torch.tensor(1.0), "exp_avg": mom[gr["name"]][0].clone(), "exp_avg_sq": mom[gr["name"]][1].clone()}
    for k, v in stats.items():
        setattr(m, k, v.clone())
    return m


def torch_form(t, mom, stats, max_gs):
    """The six stages on dictionaries of tensors, fp32 on the device, with the reference's host reads; returns the row count."""
    t, mom = dict(t), dict(mom)
    a, d, r, w = (stats[k].clone() for k in ("xyz_gradient_accum", "denom", "max_radii2D", "xyz_weight_accum"))
    lim = PERCENT_DENSE * EXTENT

    def cat(ext):
        for n in t:
            mom[n] = tuple(torch.cat((x, torch.zeros_like(ext[n])), dim=0) for x in mom[n])
            t[n] = torch.cat((t[n], ext[n]), dim=0)

    def densify_stats(mask, split, ratio):
        nonlocal a, d, r, w
        a = torch.cat([a, a[mask].repeat(split, 1) * ratio], dim=0)
        new_w = w[mask].repeat(split, 1) * w.max()
        d = torch.cat([d, d[mask].repeat(split, 1)], dim=0)
        r = torch.cat([r, r[mask].repeat(split) * ratio], dim=0)
        w = torch.cat([w, new_w], dim=0)

    def prune(mask):
        nonlocal a, d, r, w
        keep = ~mask
        for n in t:
            t[n] = t[n][keep]
            mom[n] = tuple(x[keep] for x in mom[n])
        a, d, r, w = a[keep], d[keep], r[keep], w[keep]

    def avg(x):
        v = x / d
        v[v.isnan()] = 0.0
        return v

    def split(mask, N, div):
        stds = torch.exp(t["scaling"][mask]).repeat(N, 1)
        stds = torch.cat([stds, torch.zeros_like(stds[:, :1])], dim=-1)
        samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
        rots = build_rotation(t["rotation"][mask]).repeat(N, 1, 1)
        ext = {n: v[mask].repeat(N, *([1] * (v.dim() - 1))) for n, v in t.items()}
        ext["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][mask].repeat(N, 1)
        ext["scaling"] = torch.log(torch.exp(t["scaling"][mask]).repeat(N, 1) / div)
        n_split = mask.sum().item()
        if n_split > 0:
            cat(ext)
            densify_stats(mask, N, 1.0 / div)
            prune(torch.cat((mask, torch.zeros(N * n_split, device=mask.device, dtype=torch.bool))))

    smax = lambda: torch.exp(t["scaling"]).max(dim=1).values
    sel = (torch.norm(avg(a), dim=-1) >= MAX_GRAD) & (smax() <= lim)
    cat({n: v[sel] for n, v in t.items()})
    densify_stats(sel, 1, 1.0)
    split((smax() > lim) & (avg(a) >= MAX_GRAD).squeeze(-1), 2, 0.8 * 2)
    faint = (torch.sigmoid(t["opacity"]) < MIN_OPACITY).squeeze(-1)
    if faint.sum().item() > 0:
        prune(faint)
    big = r > SCREEN
    big.sum().item()
    scene = smax() > EXTENT * 0.1
    scene.sum().item()
    weights = avg(w)
    low = (weights < torch.quantile(weights, 0.1)).squeeze(-1)
    low.sum().item()
    big = big | scene
    prune_mask = big & low
    split_mask = (big & ~low)[~prune_mask]
    n_prune, n_split = prune_mask.sum().item(), split_mask.sum().item()
    if n_prune > 0:
        prune(prune_mask)
    if n_split > 0:
        split(split_mask, 5, 0.5 * 5)
    n_cut = t["xyz"].shape[0] - int(max_gs * 0.9)
    if n_cut > 0:
        _, idx = torch.topk(avg(w)[..., 0], n_cut, largest=False)
        mask = torch.zeros(t["xyz"].shape[0], dtype=torch.bool, device=idx.device)
        mask[idx] = True
        prune(mask)
    n = t["xyz"].shape[0]
    a, d, w, r = torch.zeros(n, 1, device=d.device), torch.zeros(n, 1, device=d.device), torch.zeros(n, 1, device=d.device), torch.zeros(n, device=d.device)
    return n


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [300_000, 1_000_000]
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    for P in sizes:
        t, mom, stats, frame = source_tensors(P, dev)
        free = fresh_model(t, mom, stats, 2e6 * 100).densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SCREEN, seed=0)
        max_gs = (int(0.95 * free.rows) + 0.5) / 0.9
        nat, tor, counts, rows_t = [], [], None, None
        for rep in range(6):                                            # alternating; the first pair is the warm-up
            m = fresh_model(t, mom, stats, max_gs)
            ms, counts = host_ms(lambda: m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, SCREEN, seed=rep))
            nat.append(ms)
            del m
            ms, rows_t = host_ms(lambda: torch_form(t, mom, stats, max_gs))
            tor.append(ms)
        assert counts.rows == rows_t == int(0.95 * free.rows), (counts.rows, rows_t, free.rows)
        assert min(counts.n_clone, counts.n_split, counts.n_pruned4, counts.n_split4, counts.n_pruned5) > 0 and counts.n_stage3 < P + counts.n_clone + counts.n_split
        nat, tor = nat[1:], tor[1:]
        print(f"P {P}: densify_and_prune {min(nat):.3f} ms (runs {fmt(nat)}) -> {counts.rows} rows: cloned {counts.n_clone}, split in 2 {counts.n_split}, "
              f"stage 4 pruned {counts.n_pruned4} / split in 5 {counts.n_split4}, capped {counts.n_pruned5}; torch chain {min(tor):.3f} ms "
              f"(runs {fmt(tor)}), ratio {min(tor) / min(nat):.1f}x", flush=True)
        m = fresh_model(t, mom, stats, max_gs)
        a2, d2, w2 = (stats[k].clone() for k in ("xyz_gradient_accum", "denom", "xyz_weight_accum"))

        def native_stats():
            for _ in range(20):
                m.add_densification_stats(frame.grad, frame.vis, frame.weight)

        def torch_stats():
            for _ in range(20):
                a2[frame.vis] += torch.norm(frame.grad[frame.vis], dim=-1, keepdim=True)
                d2[frame.vis] += 1
                w2[frame.vis] += frame.weight[frame.vis]
        ns, ts = [], []
        for rep in range(6):
            ns.append(host_ms(native_stats)[0] / 20)
            ts.append(host_ms(torch_stats)[0] / 20)
        ns, ts = ns[1:], ts[1:]
        assert torch.equal(m.denom, d2)
        print(f"P {P}: add_densification_stats {min(ns):.4f} ms a call (runs {fmt(ns)}); torch form (three boolean-mask lines) "
              f"{min(ts):.4f} ms (runs {fmt(ts)}), ratio {min(ts) / min(ns):.1f}x", flush=True)


if __name__ == "__main__":
    main()
