"""Times the multi-view consistency loss (libmrgs.so, materialrefgs_amd.multiview) forward+backward at 800^2 and 1600^2 with
N = 102 400 samples, alternating with an fp32 torch form of the same statement (tests/multiview_statement.py) in the same process;
device events after warm-up.  Inputs: render_surfel("pgsr") maps of the synthetic shell from two orbit cameras.  Per-kernel times:
    rocprofv3 --kernel-trace --stats -d OUT -o w -- python tools/warp_time.py
Developer tool; prints one line per size."""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiview_statement as ms  # noqa: E402
from materialrefgs_amd import multiview as mv  # noqa: E402
from materialrefgs_amd.renderer import render_surfel  # noqa: E402
from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera  # noqa: E402

PIPE = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
KW = dict(geo_weight=0.03, ncc_weight=0.15, metallic_weight=0.05, roughness_weight=0.05)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    dev = torch.device("cuda:0")
    for H in (800, 1600):
        W = H
        pc, env, _ = make_surfel_model(300_000, H, dev)
        cams = [orbit_camera(v, H, W, n_views=96).to(dev) for v in (0, 1)]
        env.build_mips()
        with torch.no_grad():
            pk = [render_surfel(c, pc, PIPE, torch.zeros(3, device=dev), srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr")
                  for c in cams]
        fg = (pk[0]["rend_alpha"] > 0.5).float().reshape(H, W)
        leaf = lambda p: {**p, **{k: p[k].detach().clone().requires_grad_(True) for k in ("surf_depth", "diffuse_map", "refl_strength_map",
                                                                                          "roughness_map")}}
        vp, npk = leaf(pk[0]), leaf(pk[1])
        smp = torch.empty(102400, dtype=torch.int32, device=dev)

        def native():
            r = mv.warp_consistency_loss(cams[0], vp, cams[1], npk, fg, iteration=30000, seed=3, out_samples=smp, schedule="refreal", **KW)
            (r[0] + r[1] + r[2] + r[3]).backward()

        native()
        torch.cuda.synchronize()
        nv = int(mv.warp_consistency_loss(cams[0], vp, cams[1], npk, fg, iteration=30000, seed=3, out_samples=smp, **KW)[5])
        samples = smp[:min(nv, 102400)].long()
        f = lambda t: t.detach().reshape(-1, H, W).squeeze(0).clone().requires_grad_(True)
        leaves = [f(vp["surf_depth"]), f(npk["surf_depth"]), f(npk["diffuse_map"]), f(npk["refl_strength_map"]), f(npk["roughness_map"])]
        intr = lambda c: (W / (2 * torch.tan(torch.tensor(c.FoVx / 2)).item()), H / (2 * torch.tan(torch.tensor(c.FoVy / 2)).item()), W / 2, H / 2)

        def torch_form():
            o = ms.warp_loss(leaves[0], leaves[1], vp["rend_normal"].detach(), vp["rend_distance"].detach().reshape(H, W),
                             vp["diffuse_map"].detach(), vp["refl_strength_map"].detach().reshape(H, W), vp["roughness_map"].detach().reshape(H, W),
                             leaves[2], leaves[3], leaves[4], fg, None, ms.camera_record(cams[0], torch.float32, dev),
                             ms.camera_record(cams[1], torch.float32, dev), intr(cams[0]), intr(cams[1]), samples, geo_w=0.03, base_w=0.225,
                             metal_w=0.05, rough_w=0.05)
            (o["geo"] + o["base"] + o["metal"] + o["rough"]).backward()

        torch_form()
        torch.cuda.synchronize()
        tn, tt = [], []
        for _ in range(3):
            tn.append(timed(native, 20))
            tt.append(timed(torch_form, 3))
        print(f"{H}x{W}: n_valid {nv}, samples {samples.numel()}: native fwd+bwd {min(tn):.3f} ms, fp32 torch form {min(tt):.3f} ms "
              f"(runs {', '.join(f'{x:.3f}' for x in tn)} / {', '.join(f'{x:.3f}' for x in tt)})", flush=True)


if __name__ == "__main__":
    main()
