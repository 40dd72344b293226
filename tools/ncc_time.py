"""Times the grey-image NCC term of the multi-view loss (libmrgs.so: warp_ncc_fwd / _finalize / _bwd behind
materialrefgs_amd.multiview.warp_consistency_loss(grey_v=, grey_n=)) forward+backward at 800^2 and 1600^2 with N = 102 400 samples,
alternating in one process with an fp32 torch form of the same term (tests/multiview_ncc_statement.py in float32, on the same draw) and
with the existing call without the new node; device events after warm-up, the minimum and all repeats printed.  Inputs: the analytic
two-view scene and grey texture of the tests.  Two iterations: 15 000 (the material call draws, the NCC node reuses its draw and
homographies) and 8 000 (no material terms: the NCC node runs the sampler itself).  Per-kernel times:
    rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/ncc_time.py
Developer tool; prints one line per size and iteration."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multiview_statement as ms  # noqa: E402
import multiview_ncc_statement as mn  # noqa: E402
from materialrefgs_amd import multiview as mv  # noqa: E402
from materialrefgs_amd.camera import fov2focal  # noqa: E402

KW = dict(geo_weight=0.03, ncc_weight=0.15, metallic_weight=0.05, roughness_weight=0.05)
GRAD = ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map", "rend_normal", "rend_distance")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def intr(cam):
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [800, 1600]
    for H in sizes:
        W = H
        v, n = ms.analytic_pair(H, W)
        gv, gn = (g.to(dev) for g in mn.grey_pair(H, W))
        pkg = lambda x: {k: t.to(dev).clone().requires_grad_(k in GRAD) for k, t in
                         {"surf_depth": x.depth[None], "rend_normal": x.normal, "rend_distance": x.distance[None], "diffuse_map": x.base,
                          "refl_strength_map": x.metal[None], "roughness_map": x.rough[None]}.items()}
        vp, npk, fg = pkg(v), pkg(n), v.fg.to(dev)
        vc, nc = v.cam.to(dev), n.cam.to(dev)
        smp = torch.empty(102400, dtype=torch.int32, device=dev)
        for it in (15000, 8000):
            def without():
                r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=it, seed=3, out_samples=smp, schedule="refreal", **KW)
                (r[0] + r[1] + r[2] + r[3]).backward()

            def with_ncc():
                r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=it, seed=3, out_samples=smp, schedule="refreal", grey_v=gv,
                                             grey_n=gn, **KW)
                (r[0] + r[1] + r[2] + r[3] + r[6]).backward()

            det = {}
            r = mv.warp_consistency_loss(vc, vp, nc, npk, fg, iteration=it, seed=3, out_samples=smp, schedule="refreal", grey_v=gv, grey_n=gn,
                                         ncc_detail=det, **KW)
            ns, nu = (int(x) for x in det["counts"])
            samples = smp[:ns].long()
            weight = r[4]
            cv, cn = ms.camera_record(vc, torch.float32, dev), ms.camera_record(nc, torch.float32, dev)
            N = vp["rend_normal"].detach().clone().requires_grad_(True)
            D = vp["rend_distance"].detach().reshape(H, W).clone().requires_grad_(True)
            mvd, mnd = vp["refl_strength_map"].detach().reshape(H, W), npk["refl_strength_map"].detach().reshape(H, W)

            def torch_form():
                o = mn.ncc_loss(N, D, gv, gn, mvd, mnd, weight, cv, cn, intr(vc), intr(nc), samples)
                o["ncc"].backward()

            for f in (without, with_ncc, torch_form):
                f()
            torch.cuda.synchronize()
            ta, tb, tt = [], [], []
            for _ in range(5):
                ta.append(timed(without, 50))
                tb.append(timed(with_ncc, 50))
                tt.append(timed(torch_form, 5))
            fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
            print(f"{H}x{W} it {it}: samples {ns}, used {nu}: call without NCC {min(ta):.3f} ms, with {min(tb):.3f} ms, NCC node fwd+bwd "
                  f"{min(tb) - min(ta):.3f} ms, fp32 torch form of the term {min(tt):.3f} ms, ratio {min(tt) / (min(tb) - min(ta)):.1f}x "
                  f"(runs {fmt(ta)} / {fmt(tb)} / {fmt(tt)})", flush=True)


if __name__ == "__main__":
    main()
