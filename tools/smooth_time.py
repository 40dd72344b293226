"""Times the Sobel smoothness terms (libmrgs.so: smooth_terms_fwd / _finalize / _bwd behind materialrefgs_amd.smoothness) forward+backward at
800^2 and 1600^2: (a) the albedo term of train_refreal.py:1261, smooth_loss(base_color_map * ref_score_image), and (b) both edge-aware terms
of calculate_loss (rend_normal and surf_depth against the ground-truth image) in one call, each alternating in one process with the fp32
torch form of the same statements on the device (tests/smooth_statement.py in float32: the torch ops `losses.smooth_loss` and
`losses.first_order_edge_aware_loss` were before the native node, with the score already on the device); device events after warm-up
over 5 x 500 native and 5 x 50 torch calls, the minimum and all repeats printed.  Also prints the host time of one native forward+backward
(wall clock over the same calls, the queue drained once at the end: a native time close to it is bound by the host, not by the kernels)
and the algorithmic bytes of each direction.  Inputs: the maps of the tests.  Per-kernel times, in a run of its own (--profile: one
short batch of each, so that the trace stays small):
    rocprofv3 --kernel-trace --stats -d OUT -o s -- python tools/smooth_time.py --profile
Developer tool; prints two lines per size."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_statement as ss  # noqa: E402
from materialrefgs_amd import smoothness as sm  # noqa: E402


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
    profile = "--profile" in sys.argv[1:]
    sizes = [int(a) for a in sys.argv[1:] if a != "--profile"] or [800, 1600]
    batches, n_native, n_torch = (1, 50, 5) if profile else (5, 500, 50)
    for H in sizes:
        W = H
        inp = {k: v.to(dev) for k, v in ss.inputs(H, W).items()}
        albedo, normal, depth = (inp[k].clone().requires_grad_(True) for k in ("albedo", "normal", "depth"))
        img, score = inp["img"], inp["score"]
        mb = 4 * H * W / 1e6                                          # one fp32 plane

        def albedo_native():
            return torch.autograd.grad(sm.albedo_smooth_loss(albedo, score), [albedo])

        def albedo_torch():
            return torch.autograd.grad(ss.smooth_loss(albedo * score), [albedo])

        def edge_native():
            tn, td = sm.view_smooth_terms(img, (sm.SmoothItem(normal, None, True), sm.SmoothItem(depth, None, True)))
            return torch.autograd.grad(0.01 * tn + 0.01 * td, [normal, depth])

        def edge_torch():
            return torch.autograd.grad(0.01 * ss.first_order_edge_aware_loss(normal, img) + 0.01 * ss.first_order_edge_aware_loss(depth, img),
                                       [normal, depth])

        # (a) reads three planes and the byte mask each way and writes three; (b) reads 3 + 1 planes and the image's three each way, writes four
        for what, native, torch_form, planes in (("albedo term", albedo_native, albedo_torch, (3.25, 3.25, 3)),
                                                  ("two edge-aware terms, one call", edge_native, edge_torch, (7, 7, 4))):
            for f, n in ((native, n_native), (torch_form, n_torch)):      # warm-up: a batch of each, the host's first calls are its slowest
                for _ in range(n):
                    f()
            torch.cuda.synchronize()
            tn, tt = [], []
            for _ in range(batches):
                tn.append(timed(native, n_native))
                tt.append(timed(torch_form, n_torch))
            t0 = time.perf_counter()
            for _ in range(200):
                native()
            host = (time.perf_counter() - t0) / 200 * 1e3
            torch.cuda.synchronize()
            fmt = lambda xs: ", ".join(f"{v:.3f}" for v in xs)
            print(f"{H}x{W} {what}: native fwd+bwd {min(tn):.3f} ms (host {host:.3f} ms per call; fwd reads {planes[0] * mb:.1f} MB, bwd reads "
                  f"{planes[1] * mb:.1f} MB and writes {planes[2] * mb:.1f} MB), fp32 torch form {min(tt):.3f} ms, ratio {min(tt) / min(tn):.1f}x "
                  f"(runs {fmt(tn)} / {fmt(tt)})", flush=True)


if __name__ == "__main__":
    main()
