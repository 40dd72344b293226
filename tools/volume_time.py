"""Times the per-gaussian stage of render_volume -- shading.volume_features on csrc/mrgs_volume.hip -- forward + backward at P = 300 000 and
1 000 000 rows of the shell scene with an environment 128 -> 16, both flavours ("2dgs", "pgsr"), beside the chain of torch ops it
replaces (renderer._NATIVE_VOLUME off: the getters, get_normal, the view vectors, the unused degree-3 SH evaluation, the FG lookup, two
EnvLight lookups, the split-sum weight and the concatenations), in the same process on the same GPU; then whole render_volume forward +
backward at 800 x 800 both ways.  The mip levels and the diffuse map are leaves here (build_mips is not part of the stage); both forms
write gradients for the seven raw tensors and every level.  The window is a host clock between two device synchronisations around a
batch of calls, the two forms alternate, the first pair is the warm-up, the minimum and every run are printed.  Before anything is
timed both forms are compared with the float64 statement (tests/volume_statement.py, evaluated on the device) by the rule of
tests/test_volume_features.py: per tensor err(native) <= 1.5 err(torch chain) + 1e-6, asserted.  The kernels' own times come from a trace:
    rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/volume_time.py 300000
Developer tool; prints one line per size, flavour and measurement."""
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_statement as vs  # noqa: E402
from materialrefgs_amd import renderer, shading  # noqa: E402
from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera  # noqa: E402

BATCH, REPS = 5, 6
RAW = ("_xyz", "_scaling", "_rotation", "_opacity", "_refl_strength", "_roughness", "_ori_color")
MARGIN = 1e-4


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def model(P, dev):
    pc, env, _ = make_surfel_model(P, 800, dev, seed=1, env_res=128, env_min=16)
    pc.env_map_2 = env
    env.build_mips()
    levels = [m.detach().clone().requires_grad_(True) for m in env.specular]
    diffuse = env.diffuse.detach().clone().requires_grad_(True)
    env._specular, env._diffuse = levels, diffuse
    return pc, env, [diffuse] + levels


def upstreams(P, C, dev):
    g = torch.Generator(device=dev).manual_seed(77)
    return [torch.randn(P, w, generator=g, device=dev) for w in (1, 2, 4, 3, C, 3)]


def stage(pc, env, cam, flag, native, up, leaves):
    if native:
        *outs, xyz = shading.volume_features(pc, cam, env, flag=flag, pass_xyz=True)
    else:
        outs, xyz = vs.torch_chain(pc, cam, flag, dead_sh=True), pc._xyz
    return outs, torch.autograd.grad(list(outs) + [xyz], leaves, up, allow_unused=True)


def agree(pc, env, cam, flag, up, chain):
    """the rule of tests/test_volume_features.py, with the float64 statement evaluated on the device"""
    dev = pc._xyz.device
    raw64 = [getattr(pc, n).detach().double().requires_grad_(True) for n in RAW]
    chain64 = [t.detach().double().requires_grad_(True) for t in chain]
    lut = shading.load_fg_lut(dev).double()
    campos = cam.camera_center.double()
    Rt = cam.R.double().T
    rays_o = (-Rt.T @ cam.T.double().unsqueeze(-1)).flatten()
    vm = cam.world_view_transform.double() if flag != "2dgs" else None
    ref = vs.volume_statement(raw64, campos, rays_o, lut, chain64[1:], chain64[0], viewmatrix=vm)
    g_ref = torch.autograd.grad(list(ref) + [raw64[0]], raw64 + chain64, [u.double() for u in up], allow_unused=True)
    keep = vs.decision_margin(raw64, campos, rays_o, lut, [t.detach() for t in chain64[1:]], chain64[0].detach()) >= MARGIN
    leaves = [getattr(pc, n) for n in RAW] + chain
    legs = [stage(pc, env, cam, flag, native, up, leaves) for native in (True, False)]
    names = ["opacity", "scales", "rotations", "colors_precomp", "features"] + ["d" + n for n in RAW] + ["d_diffuse"] + [f"d_level{i}" for i in range(len(chain) - 1)]
    worst = 0.0
    for i, (n, r) in enumerate(zip(names, list(ref) + list(g_ref))):
        if r is None:
            continue
        a, b = [(leg[0][i] if i < 5 else leg[1][i - 5]) for leg in legs]
        rows = keep if n in ("d_xyz", "d_rotation", "d_roughness") else slice(None)
        scale = max(float(r.abs().max()), 1e-30)
        ea, eb = [float((t.detach().double() - r.detach())[rows].abs().max()) / scale for t in (a, b)]
        assert ea <= 1.5 * eb + 1e-6, (flag, n, ea, eb)
        worst = max(worst, ea)
    return worst, float((~keep).double().mean())


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [300_000, 1_000_000]
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    cam = orbit_camera(1, 800, 800).to(dev)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, use_asg=False, compute_cov3D_python=False)
    bg = torch.zeros(3, device=dev)
    for P in sizes:
        pc, env, chain = model(P, dev)
        leaves = [getattr(pc, n) for n in RAW] + chain
        for flag in ("2dgs", "pgsr"):
            up = upstreams(P, 11 if flag == "2dgs" else 12, dev)
            worst, low = agree(pc, env, cam, flag, up, chain)
            nat, tor = [], []
            for _ in range(REPS):                                      # alternating; the first pair is the warm-up
                nat.append(host_ms(lambda: [stage(pc, env, cam, flag, True, up, leaves) for _ in range(BATCH)]) / BATCH)
                tor.append(host_ms(lambda: [stage(pc, env, cam, flag, False, up, leaves) for _ in range(BATCH)]) / BATCH)
            nat, tor = nat[1:], tor[1:]
            assert all(a < b for a, b in zip(nat, tor)), (P, flag, nat, tor)
            print(f"P {P} {flag}: stage fwd+bwd native {min(nat):.3f} ms (runs {fmt(nat)}), torch chain {min(tor):.3f} ms (runs {fmt(tor)}), "
                  f"ratio {min(tor) / min(nat):.1f}; worst native error {worst:.1e}, rows under the margin {100 * low:.2f} %", flush=True)

            def view(native):
                renderer._NATIVE_VOLUME = native
                out = renderer.render_volume(cam, pc, pipe, bg, opt=SimpleNamespace(indirect=False), flag=flag)
                torch.autograd.grad(out["render"].sum() + out["rend_normal"].sum(), leaves, allow_unused=True)
            nat, tor = [], []
            try:
                for _ in range(REPS):
                    nat.append(host_ms(lambda: [view(True) for _ in range(BATCH)]) / BATCH)
                    tor.append(host_ms(lambda: [view(False) for _ in range(BATCH)]) / BATCH)
            finally:
                renderer._NATIVE_VOLUME = True
            nat, tor = nat[1:], tor[1:]
            print(f"P {P} {flag}: render_volume 800x800 fwd+bwd native {min(nat):.3f} ms (runs {fmt(nat)}), torch chain {min(tor):.3f} ms "
                  f"(runs {fmt(tor)})", flush=True)
            assert min(nat) <= min(tor), (P, flag, nat, tor)


if __name__ == "__main__":
    main()
