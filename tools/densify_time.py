"""Times one materialrefgs_amd.densify.densify_and_prune call and one add_densification_stats call (libmrgs.so:
csrc/mrgs_densify.hip, allocation of the outputs and the optimizer surgery included) at P = 300 000 and 1 000 000 on the bench scene
(synthetic.make_surfel_model) carrying the sixteen per-gaussian groups of GaussianModel.training_setup with both Adam moments, beside
the torch form of the same step -- the reference's three stages (clone + cat, split + cat + prune, final prune) and its two statistics
lines, in fp32 on the same GPU in the same run.  The thresholds are quantiles of the inputs: ~20 % of the rows cloned, ~10 % split,
~10 % pruned, half of the rows visible.  A densify call changes its model, so every repetition gets a fresh copy outside the timed window;
the window is a host clock between two device synchronisations (the call contains a host read by design), the minimum of several
repetitions and all of them printed.  The torch form waits for the host ~50 times a call, so the comparison is one-sided: for the record.
Per-kernel times:  rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/densify_time.py 300000
Developer tool; prints two lines per size."""
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import densify  # noqa: E402
from materialrefgs_amd.synthetic import make_surfel_model  # noqa: E402

EXTRA = {"diffuse_color": (3,), "normal1": (3,), "normal2": (3,), "metalness": (1,), "ind_asg": (32, 5)}     # groups the bench model lacks
ORDER = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "refl_strength", "ori_color", "diffuse_color", "roughness", "metalness",
         "normal1", "normal2", "ind_dc", "ind_rest", "ind_asg")
PERCENT_DENSE, N = 0.01, 2


def source_tensors(P, dev):
    pc, _env, _ = make_surfel_model(P, 512, dev, seed=0, env_res=16, env_min=8)
    g = torch.Generator(device=dev).manual_seed(1)
    t = {}
    for n in ORDER:
        t[n] = (torch.randn((P,) + EXTRA[n], generator=g, device=dev) if n in EXTRA else getattr(pc, densify.group_attr(n)).detach().clone())
    mom = {n: (torch.randn(v.shape, generator=g, device=dev), torch.rand(v.shape, generator=g, device=dev)) for n, v in t.items()}
    accum, denom = torch.rand(P, 1, generator=g, device=dev), torch.ones(P, 1, device=dev)
    smax = torch.exp(t["scaling"]).max(dim=1).values
    th = SimpleNamespace(max_grad=0.7, extent=float(torch.quantile(smax, 0.65)) / PERCENT_DENSE,
                         min_opacity=float(torch.quantile(torch.sigmoid(t["opacity"]), 0.10)))
    grad = torch.randn(P, 3, generator=g, device=dev) * 1e-3
    vis = torch.rand(P, generator=g, device=dev) < 0.5
    radii = torch.randint(0, 60, (P,), generator=g, dtype=torch.int32, device=dev)
    return t, mom, accum, denom, th, grad, vis, radii


def fresh_model(t, mom, accum, denom):
    groups = [{"params": [torch.nn.Parameter(t[n].clone())], "lr": 0.01, "name": n} for n in ORDER]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    m = SimpleNamespace(optimizer=opt, percent_dense=PERCENT_DENSE, xyz_gradient_accum=accum.clone(), denom=denom.clone(),
                        max_radii2D=torch.zeros(accum.shape[0], device=accum.device))
    for gr in groups:
        p = gr["params"][0]
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": mom[gr["name"]][0].clone(), "exp_avg_sq": mom[gr["name"]][1].clone()}
        setattr(m, densify.group_attr(gr["name"]), p)
    return m


def build_rotation(q):
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def torch_form(t, mom, accum, denom, th, max_screen_size=20):
    """The three stages on dictionaries of tensors (moments: zeros for new rows), fp32 on the device; returns the row count."""
    t, mom = dict(t), dict(mom)

    def cat(ext):
        for n in t:
            mom[n] = tuple(torch.cat((x, torch.zeros_like(ext[n])), dim=0) for x in mom[n])
            t[n] = torch.cat((t[n], ext[n]), dim=0)

    def prune(mask):
        keep = ~mask
        for n in t:
            t[n] = t[n][keep]
            mom[n] = tuple(x[keep] for x in mom[n])
    P = t["xyz"].shape[0]
    lim = PERCENT_DENSE * th.extent
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    sel = (torch.norm(grads, dim=-1) >= th.max_grad) & (torch.exp(t["scaling"]).max(dim=1).values <= lim)
    cat({n: v[sel] for n, v in t.items()})
    padded = torch.zeros(t["xyz"].shape[0], device=grads.device)
    padded[:P] = grads.squeeze()
    sel = (padded >= th.max_grad) & (torch.exp(t["scaling"]).max(dim=1).values > lim)
    stds = torch.exp(t["scaling"][sel]).repeat(N, 1)
    stds = torch.cat([stds, torch.zeros_like(stds[:, :1])], dim=-1)
    samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
    rots = build_rotation(t["rotation"][sel]).repeat(N, 1, 1)
    ext = {n: v[sel].repeat(N, *([1] * (v.dim() - 1))) for n, v in t.items()}
    ext["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(N, 1)
    ext["scaling"] = torch.log(torch.exp(t["scaling"][sel]).repeat(N, 1) / (0.8 * N))
    cat(ext)
    prune(torch.cat((sel, torch.zeros(N * int(sel.sum()), device=sel.device, dtype=torch.bool))))
    mask = (torch.sigmoid(t["opacity"]) < th.min_opacity).squeeze()
    if max_screen_size:
        mask = mask | (torch.exp(t["scaling"]).max(dim=1).values > 0.1 * th.extent)
    prune(mask)
    return t["xyz"].shape[0]


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
        t, mom, accum, denom, th, grad, vis, radii = source_tensors(P, dev)
        nat, tor, counts, rows_t = [], [], None, None
        for rep in range(6):                                            # alternating; the first pair is the warm-up
            m = fresh_model(t, mom, accum, denom)
            ms, counts = host_ms(lambda: densify.densify_and_prune(m, th.max_grad, th.min_opacity, th.extent, 20, seed=rep))
            nat.append(ms)
            del m
            ms, rows_t = host_ms(lambda: torch_form(t, mom, accum, denom, th))
            tor.append(ms)
        rows = counts[0] + counts[1] + N * counts[2]
        assert rows == rows_t, (rows, rows_t)
        nat, tor = nat[1:], tor[1:]
        print(f"P {P}: densify_and_prune {min(nat):.3f} ms (runs {fmt(nat)}) -> {rows} rows: kept {counts[0]}, clones {counts[1]}, "
              f"split rows {counts[2]}; torch form {min(tor):.3f} ms (runs {fmt(tor)}), ratio {min(tor) / min(nat):.1f}x", flush=True)
        a1, d1, r1 = accum.clone(), denom.clone(), torch.zeros(P, device=dev)
        a2, d2, r2 = accum.clone(), denom.clone(), torch.zeros(P, device=dev)

        def native_stats():
            for _ in range(20):
                densify.add_densification_stats((a1, d1, r1), grad, vis, radii)

        def torch_stats():
            for _ in range(20):
                r2[vis] = torch.max(r2[vis], radii[vis])
                a2[vis] += torch.norm(grad[vis], dim=-1, keepdim=True)
                d2[vis] += 1
        ns, ts = [], []
        for rep in range(6):
            ns.append(host_ms(native_stats)[0] / 20)
            ts.append(host_ms(torch_stats)[0] / 20)
        ns, ts = ns[1:], ts[1:]
        print(f"P {P}: add_densification_stats {min(ns):.4f} ms a call (runs {fmt(ns)}); torch form (two lines, four boolean-index syncs) "
              f"{min(ts):.4f} ms (runs {fmt(ts)}), ratio {min(ts) / min(ns):.1f}x", flush=True)


if __name__ == "__main__":
    main()
