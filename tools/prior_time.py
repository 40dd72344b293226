"""Times the per-pixel prior terms (libmrgs.so: prior_terms_fwd / _finalize / _bwd behind materialrefgs_amd.priors.view_prior_terms)
forward+backward with all three groups (normal prior with a mask, mask entropy, ref score) at 800^2 and 1600^2, alternating in one
process with the literal fp32 torch form of the same terms on the device (tests/prior_statement.py in float32: what a user of the training
scripts executes, with the prior images already on the device); device events after warm-up over 5 x 500 native and 5 x 50 torch calls, the minimum and all repeats printed.  Also
prints the host time of one native forward+backward (wall clock over the same calls, the queue drained once at the end) and, per
direction, the algorithmic bytes against the kernel time the events imply.  Inputs: the analytic maps of the tests.  Per-kernel times:
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/prior_time.py
Developer tool; prints one line per size."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prior_statement as ps  # noqa: E402
from materialrefgs_amd import priors  # noqa: E402

LEAVES = ("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")


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
    sizes = [int(a) for a in sys.argv[1:]] or [800, 1600]
    for H in sizes:
        W = H
        inp = {k: v.to(dev) for k, v in ps.analytic_inputs(H, W).items()}
        x = {k: inp[k].clone().requires_grad_(True) for k in LEAVES}
        leaves = [x[k] for k in LEAVES]
        cam = SimpleNamespace(R=inp["R"].cpu().numpy(), T=np.zeros(3, dtype=np.float32), HWK=(H, W, np.eye(3, dtype=np.float32)), image_name="v")

        def native():
            t = priors.view_prior_terms(cam, surf_normal=x["surf_normal"], rend_normal=x["rend_normal"], normal_prior=inp["prior"],
                                        normal_mask=inp["mask"], rend_alpha=x["rend_alpha"], alpha_mask=inp["mask"], refl_strength_map=x["refl"],
                                        roughness_map=x["rough"], ref_score_image=inp["score"])
            return torch.autograd.grad(0.01 * (t.l1_surf + t.cos_surf + t.l1_rend + t.cos_rend) + 0.01 * t.mask_entropy + 0.1 * t.ref_sum, leaves)

        def torch_form():
            o = ps.prior_terms(R=inp["R"], surf_normal=x["surf_normal"], rend_normal=x["rend_normal"], prior=inp["prior"], mask=inp["mask"],
                               rend_alpha=x["rend_alpha"], alpha_mask=inp["mask"], refl=x["refl"], rough=x["rough"], score=inp["score"], terms_only=True)
            return torch.autograd.grad(0.01 * (o["l1_surf"] + o["cos_surf"] + o["l1_rend"] + o["cos_rend"]) + 0.01 * o["mask_entropy"] +
                                       0.1 * o["ref_metallic"] + 0.1 * o["ref_roughness"] + 0.1 * o["ref_metallic_bg"] +
                                       .5 * 0.1 * o["ref_roughness_bg"], leaves)

        for f in (native, torch_form):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        tn, tt = [], []
        for _ in range(5):
            tn.append(timed(native, 500))
            tt.append(timed(torch_form, 50))
        t0 = time.perf_counter()
        for _ in range(200):
            native()
        host = (time.perf_counter() - t0) / 200 * 1e3
        torch.cuda.synchronize()
        fmt = lambda xs: ", ".join(f"{v:.3f}" for v in xs)
        mb = H * W / 1e6
        print(f"{H}x{W}: native fwd+bwd {min(tn):.3f} ms (host {host:.3f} ms per call; fwd reads {53 * mb:.1f} MB, bwd reads {53 * mb:.1f} MB and "
              f"writes {36 * mb:.1f} MB), fp32 torch form {min(tt):.3f} ms, ratio {min(tt) / min(tn):.1f}x (runs {fmt(tn)} / {fmt(tt)})", flush=True)


if __name__ == "__main__":
    main()
