"""Times GaussianModel.normal_propagation_step and GaussianModel.opacity_reset_step (materialrefgs_amd/model.py on
csrc/mrgs_model_reset.hip; allocation of the outputs and the optimizer surgery included) at P = 300 000 and 1 000 000 rows with both Adam
moments present, beside the fp32 torch chain of the same statements on the same GPU in the same run: reset_opacity1 + dist_color +
reset_scale, and reset_opacity0 + reset_refl, each followed by its replace_tensor_to_optimizer (two zeros_like and a new Parameter per
group), with an exclusive mask.  Every repetition gets a fresh model outside the timed window; the window is a host clock between two
device synchronisations around a batch of 10 calls, the two forms alternate, the first pair is the warm-up, the minimum and every run are
printed.  Both forms must move the same rows: asserted.  Bytes a row: 16 per fp32 element of a written group (value read and written, two moments
written) plus the mask inputs an item selects.  The window holds the host side of the call (allocation, optimizer surgery) as well as the
kernel, so no bandwidth is derived from it; the kernel's own time comes from a trace:
    rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/reset_time.py 300000
Developer tool; prints two lines per size."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import checkpoint  # noqa: E402
from materialrefgs_amd.model import GaussianModel  # noqa: E402

GROUPS = {"xyz": ("_xyz", (3,)), "f_dc": ("_features_dc", (1, 3)), "f_rest": ("_features_rest", (15, 3)), "opacity": ("_opacity", (1,)),
          "scaling": ("_scaling", (2,)), "rotation": ("_rotation", (4,)), "refl_strength": ("_refl_strength", (1,)), "ori_color": ("_ori_color", (3,)),
          "diffuse_color": ("_diffuse_color", (3,)), "roughness": ("_roughness", (1,)), "metalness": ("_metalness", (1,)), "normal1": ("_normal1", (3,)),
          "normal2": ("_normal2", (3,)), "ind_dc": ("_indirect_dc", (1, 3)), "ind_rest": ("_indirect_rest", (15, 3)), "ind_asg": ("_indirect_asg", (32, 5))}
TOUCHED = ("opacity", "f_dc", "scaling", "refl_strength", "roughness")
BATCH = 10
REFL_THR, ROUGH_THR, ENLARGE = 0.02, 0.1, 1.5


def source_tensors(P, dev):
    g = torch.Generator(device=dev).manual_seed(P)
    t = {n: torch.randn((P,) + GROUPS[n][1], generator=g, device=dev) * 2.0 for n in TOUCHED}
    t["refl_strength"] = t["refl_strength"] - 3.0                      # sigmoid around 0.05: both sides of 0.02 and of 0.1 occur
    t["roughness"] = t["roughness"] - 2.0
    mom = {n: (torch.randn(v.shape, generator=g, device=dev), torch.rand(v.shape, generator=g, device=dev)) for n, v in t.items()}
    return t, mom, torch.rand(P, generator=g, device=dev) < 0.25


def fresh_model(t, mom, P, dev):
    m = GaussianModel(3)
    for n, (attr, sh) in GROUPS.items():
        v = t[n].clone() if n in t else torch.zeros((P if n == "xyz" else 1,) + sh, device=dev)         # untouched groups: one-row placeholders
        setattr(m, attr, torch.nn.Parameter(v))
    m.spatial_lr_scale = 1.0
    m.training_setup(checkpoint.default_training_args())
    for gr in m.optimizer.param_groups:
        if gr["name"] in t:
            m.optimizer.state[gr["params"][0]] = {"step": torch.tensor(1.0), "exp_avg": mom[gr["name"]][0].clone(), "exp_avg_sq": mom[gr["name"]][1].clone()}
    return m


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def replace(state, name, tensor):
    """replace_tensor_to_optimizer on a dictionary: two zeroed moments and a new Parameter"""
    state[name] = (torch.nn.Parameter(tensor.requires_grad_(True)), torch.zeros_like(tensor), torch.zeros_like(tensor))


def torch_normal_propagation(state, excl):
    opacity, f_dc, scaling = state["opacity"][0].detach(), state["f_dc"][0].detach(), state["scaling"][0].detach()
    refl, rough = torch.sigmoid(state["refl_strength"][0].detach()), torch.sigmoid(state["roughness"][0].detach())
    old = torch.sigmoid(opacity)
    keep = torch.logical_or((old > 0.9).flatten(), excl)
    new = torch.ones_like(old) * inverse_sigmoid(torch.tensor([0.9], device=old.device))
    new[keep] = opacity[keep]
    replace(state, "opacity", new)
    keep = torch.logical_or(refl.flatten() > REFL_THR, excl)
    dcc = f_dc.clone()
    dist = dcc + (torch.rand_like(dcc) * 0.4 * 2 - 0.4)
    dist[keep] = dcc[keep]
    replace(state, "f_dc", dist)
    keep = torch.logical_or(torch.logical_or(refl.flatten() < REFL_THR, rough.flatten() > ROUGH_THR), excl)
    scales = torch.exp(scaling)
    new = torch.log(scales * (torch.ones_like(scales) * ENLARGE))
    new[keep] = scaling[keep]
    replace(state, "scaling", new)


def torch_opacity_reset(state, excl):
    opacity, refl_raw = state["opacity"][0].detach(), state["refl_strength"][0].detach()
    o = torch.sigmoid(opacity)
    replace(state, "opacity", inverse_sigmoid(torch.min(o, torch.ones_like(o) * 0.01)))
    r = torch.sigmoid(refl_raw)
    new = inverse_sigmoid(torch.max(r, torch.ones_like(r) * 0.1))
    new[excl] = refl_raw[excl]
    replace(state, "refl_strength", new)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [300_000, 1_000_000]
    fmt = lambda xs: ", ".join(f"{x:.4f}" for x in xs)
    for P in sizes:
        t, mom, excl = source_tensors(P, dev)
        steps = (("normal_propagation_step", lambda m: m.normal_propagation_step(exclusive_msk=excl, seed=1), torch_normal_propagation, ("opacity", "f_dc", "scaling"), 6 * 16 + 15),
                 ("opacity_reset_step", lambda m: m.opacity_reset_step(exclusive_msk=excl), torch_opacity_reset, ("opacity", "refl_strength"), 2 * 16 + 1))
        for name, native, chain, written, row_bytes in steps:
            nat, tor = [], []
            for rep in range(6):                                        # alternating; the first pair is the warm-up
                m = fresh_model(t, mom, P, dev)
                nat.append(host_ms(lambda: [native(m) for _ in range(BATCH)])[0] / BATCH)
                state = {n: (torch.nn.Parameter(t[n].clone()), mom[n][0].clone(), mom[n][1].clone()) for n in t}
                tor.append(host_ms(lambda: [chain(state, excl) for _ in range(BATCH)])[0] / BATCH)
            m, state = fresh_model(t, mom, P, dev), {n: (torch.nn.Parameter(t[n].clone()), mom[n][0].clone(), mom[n][1].clone()) for n in t}
            native(m)
            chain(state, excl)
            for n in written:                                           # the same rows change in both forms (where the torch form's
                sane = (t[n].abs() < 6.0).flatten(1).all(1)             # logit(sigmoid(v)) round trip still returns v to 1e-3)
                moved = lambda new: ((new.detach() - t[n]).abs() > 1e-3).flatten(1).any(1)[sane]
                assert torch.equal(moved(getattr(m, GROUPS[n][0])), moved(state[n][0])), (name, n)
            nat, tor = nat[1:], tor[1:]
            print(f"P {P}: {name} {min(nat):.4f} ms a call (runs {fmt(nat)}), {row_bytes} B a row = {row_bytes * P * 1e-6:.1f} MB through the kernel; "
                  f"torch chain {min(tor):.4f} ms (runs {fmt(tor)})", flush=True)


if __name__ == "__main__":
    main()
