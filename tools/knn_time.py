"""Times materialrefgs_amd.knn.distCUDA2 (libmrgs.so: every launch of csrc/mrgs_knn.hip, workspace allocation included) at
P = 100 000, 300 000, 1 000 000 and 4 000 000 on the bench's sphere-shell centres (materialrefgs_amd/synthetic.py) and on a uniform cube;
device events after warm-up, the minimum of several batches and all of them printed.  At P = 100 000 an fp32 torch form of the same
quantity (chunked cdist + topk: the only thing a ROCm user could run before) is timed on the same GPU in the same run.  Per-kernel times:
    rocprofv3 --kernel-trace --stats -d OUT -o n -- python tools/knn_time.py
Developer tool; prints one line per size and cloud."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd.knn import distCUDA2  # noqa: E402
from materialrefgs_amd.synthetic import shell_centres  # noqa: E402

TORCH_FORM_P = 100_000


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_form(x, chunk=4096):
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    rows = torch.arange(chunk, device=x.device)
    for s in range(0, x.shape[0], chunk):
        d = torch.cdist(x[s:s + chunk], x, compute_mode="donot_use_mm_for_euclid_dist")
        n = d.shape[0]
        d[rows[:n], rows[:n] + s] = float("inf")
        out[s:s + n] = d.topk(3, dim=1, largest=False).values.square().mean(dim=1)
    return out


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [100_000, 300_000, 1_000_000, 4_000_000]
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    for P in sizes:
        clouds = {"shell": shell_centres(P, seed=0), "cube": np.random.default_rng(0).random((P, 3)).astype(np.float32)}
        for name, pts in clouds.items():
            x = torch.from_numpy(pts).to(dev)
            call = lambda: distCUDA2(x)
            ref = call()
            torch.cuda.synchronize()
            reps = 20 if P <= 1_000_000 else 5
            t = [timed(call, reps) for _ in range(5)]
            line = f"P {P} {name}: distCUDA2 {min(t):.3f} ms, {1e6 * min(t) / P:.3f} ns per point (runs {fmt(t)})"
            if P == TORCH_FORM_P:
                other = torch_form(x)
                torch.cuda.synchronize()
                rel = float(((other - ref).abs() / ref).max())
                tt = [timed(lambda: torch_form(x), 2) for _ in range(3)]
                line += f"; fp32 torch form (cdist + topk, chunks of 4096) {min(tt):.3f} ms, ratio {min(tt) / min(t):.0f}x, worst relative difference {rel:.1e}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
