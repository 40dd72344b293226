"""Times the edge mask of the multi-view loss (libmrgs.so: edge_classify / edge_link / edge_flag / edge_dilate behind
materialrefgs_amd.edges.edge_mask, dilate_size = 7, inverted: the call of multiview._drop_in) at 800^2 and 1600^2 on the rend_normal of one
view of the bench scene (synthetic.make_surfel_model through render_surfel), alternating in one process with the floor of what the
reference's path costs on the same machine: an edges_fn that only does its two transfers -- `img.detach().cpu()`, then a [H,W] float64
host tensor `.to(device)` -- and no CPU work at all.  cv2 is not installed, so the CPU time of cvtColor + Canny + dilate that the
reference pays on top of that floor is NOT measured here.
Device events around batches of calls after warm-up, the minimum of 5 batches and all batches printed; also the candidate and strong
fractions of the image (the link step's work), the edge and kept fractions, and the algorithmic bytes of the four launches.  Per-kernel times:
    rocprofv3 --kernel-trace --stats -f csv -d OUT -o e -- python tools/edges_time.py
Developer tool; prints one line per size."""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import edges  # noqa: E402
from materialrefgs_amd.camera import look_at_camera  # noqa: E402
from materialrefgs_amd.synthetic import CAM_DISTANCE, FOV, make_surfel_model  # noqa: E402

P_SURFELS = 300_000
PIPE = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    from materialrefgs_amd.renderer import render_surfel
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [800, 1600]
    for size in sizes:
        H = W = size
        pc, env, _ = make_surfel_model(P_SURFELS, size, dev, seed=0)
        env.build_mips()
        with torch.no_grad():
            pk = render_surfel(look_at_camera(17.0, 30.0, CAM_DISTANCE, FOV, H, W).to(dev), pc, PIPE, torch.zeros(3, device=dev), srgb=False,
                               opt=SimpleNamespace(indirect=False), flag="pgsr")
        normal = pk["rend_normal"].detach().clone()
        del pc, env, pk
        host_mask = torch.zeros(H, W, dtype=torch.float64)

        native = lambda: edges.edge_mask(normal, dilate_size=7, invert=True)

        def transfers_only():
            normal.detach().cpu()                        # the reference's download (a stream synchronisation) ...
            return host_mask.to(dev)                     # ... and its upload; cvtColor, Canny and dilate between them cost nothing here

        keep, cls = edges.edge_mask(normal, dilate_size=7, invert=True, classes=True)
        edge = ~edges.edge_mask(normal, dilate_size=1, invert=True)
        n = float(H * W)
        cand, strong = int((cls > 0).sum()) / n, int((cls == 2).sum()) / n
        for f in (native, transfers_only):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        tn, tt = [], []
        for _ in range(5):
            tn.append(timed(native, 500))
            tt.append(timed(transfers_only, 50))
        fmt = lambda xs: ", ".join(f"{x:.4f}" for x in xs)
        # classify reads 12 B and writes 6 B (class, parent, flag) a pixel; link and flag read the class byte; dilate reads it and writes 1 B
        bytes_alg = H * W * (12 + 6 + 1 + 1 + 2)
        print(f"{H}x{W}: candidates {cand:.4f} of the pixels, strong {strong:.4f}, edges {int(edge.sum()) / n:.4f}, kept after the 7x7 dilation "
              f"{int(keep.sum()) / n:.4f}; native edge_mask {min(tn) * 1e3:.1f} us per call (4 launches, algorithmic bytes {bytes_alg / 1e6:.1f} MB: "
              f"{bytes_alg / (min(tn) * 1e-3) / 1e9:.0f} GB/s), the reference's two transfers alone {min(tt) * 1e3:.1f} us, ratio "
              f"{min(tt) / min(tn):.1f}x; cv2's CPU time not measured (cv2 is not installed) (runs in ms {fmt(tn)} / {fmt(tt)})", flush=True)


if __name__ == "__main__":
    main()
