"""Times the multi-view reflection score (libmrgs.so: ref_score_fwd behind materialrefgs_amd.refscore.reflection_score) for one view of the
bench scene (the synthetic surfel model, render_surfel("pgsr") at 800^2, the photographs being the renders) against K = 8 and K = 20
neighbouring views, alternating in one process with the fp32 torch form of the same statement (tests/ref_score_statement.py in float32
on the device, evaluated in chunks of pixels: the reference's literal form holds a [3,H,W,81] tensor per neighbour and does not fit).
Device events after warm-up, the minimum of 5 batches and all batches printed; from the counts, the achieved taps per second (one tap
= one patch position of one valid (pixel, neighbour) pair: a homography product, four texels of three channels) and the algorithmic
bytes (every map read once, the outputs written once).  Per-kernel times:
    rocprofv3 --kernel-trace --stats -f csv -d OUT -o r -- python tools/ref_score_time.py
Developer tool; prints one line per K."""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_score_statement as rs  # noqa: E402
from materialrefgs_amd import refscore  # noqa: E402
from materialrefgs_amd.camera import look_at_camera  # noqa: E402
from materialrefgs_amd.synthetic import CAM_DISTANCE, FOV, make_surfel_model  # noqa: E402

P_SURFELS, TH = 300_000, 1.0
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
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 800
    ks = [int(a) for a in sys.argv[2:]] or [8, 20]
    H = W = size
    pc, env, _ = make_surfel_model(P_SURFELS, size, dev, seed=0)
    env.build_mips()
    bg = torch.zeros(3, device=dev)
    # the view at azimuth 17 degrees, neighbours alternating on both sides in steps of 1.5 degrees (all inside the reference's 0.1 .. 1.5 baseline)
    offsets = [0.0] + [s * 1.5 * (i // 2 + 1) for i, s in zip(range(max(ks)), [1, -1] * max(ks))]
    views = []
    with torch.no_grad():
        for i, off in enumerate(offsets):
            mini = look_at_camera(17.0 + off, 30.0, CAM_DISTANCE, FOV, H, W)
            pk = render_surfel(mini.to(dev), pc, PIPE, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr")
            views.append(SimpleNamespace(cam=mini, name=f"v{i}", depth=pk["surf_depth"].reshape(H, W).clone(), normal=pk["rend_normal"].clone(),
                                         distance=pk["rend_distance"].reshape(H, W).clone(), image=pk["render"].clamp(0, 1).clone()))
    v = views[0]
    cam_v = rs.Cam(v.cam, v.name, v.image)
    pkg = {"surf_depth": v.depth[None], "rend_normal": v.normal, "rend_distance": v.distance[None]}
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    for K in ks:
        nbrs = views[1:K + 1]
        nb = [(rs.Cam(n.cam, n.name), n.depth[None], n.image) for n in nbrs]
        native = lambda: refscore.reflection_score(cam_v, pkg, nb, pixel_noise_th=TH, return_count=True)
        torch_form = lambda: rs.ref_score(v, nbrs, th=TH, patch_half=4, chunk=32768, dtype=torch.float32, device=dev, diagnostics=False)
        score, count = native()
        o = torch_form()
        torch.cuda.synchronize()
        pairs = int(count.sum())
        same = int((count.long() == o.count).sum())
        diff = float((score - o.score).abs().max())
        tn, tt = [], []
        for _ in range(5):
            tn.append(timed(native, 5))
            tt.append(timed(torch_form, 1))
        taps = pairs * 81
        bytes_alg = H * W * 4 * (8 + 4 * K + 2)
        print(f"{H}x{W} K {K}: valid pairs {pairs} ({pairs / (H * W * K):.2f} of all), pixels with a neighbour {int((count > 0).sum()) / (H * W):.2f}; "
              f"native {min(tn):.3f} ms per view, fp32 torch form {min(tt):.1f} ms, ratio {min(tt) / min(tn):.1f}x; "
              f"{taps / (min(tn) * 1e-3) / 1e9:.2f} G taps/s, algorithmic bytes {bytes_alg / 1e6:.1f} MB ({bytes_alg / (min(tn) * 1e-3) / 1e9:.1f} GB/s); "
              f"native against the torch form: counts equal on {same / (H * W):.4f} of the pixels, max score difference {diff:.2e} "
              f"(map max {float(o.score.max()):.3f}) (runs {fmt(tn)} / {fmt(tt)})", flush=True)


if __name__ == "__main__":
    main()
