"""Times the post-render part of one evaluated view (materialrefgs_amd.evaluate on csrc/mrgs_eval.hip) at 800^2 and 1600^2: the metrics
(image_metrics into a row of a device table), the 8-bit export of the ten maps of eval.py:27 (to_rgb8, one call) and the copy of the bytes
to the host (one non-blocking copy into a pinned buffer) -- beside the fp32 torch chain of the reference's statements on the same GPU:
eval.py:44-52 (two clamps, ssim's five depthwise 11x11 convolutions, psnr, three .item() reads) and, per map, eval.py:56-65 with
torchvision.utils.save_image's mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8) (a blocking copy each).  For the
depth map the chain uses the DEVICE-SIDE EQUIVALENT of visualize_depth (min, max, the fp32 level, a table lookup, / 255) without its numpy /
cv2 round trip, which would only make the chain slower.  LPIPS and the PNG compression are the same work both ways and are left out.

Batches alternate in one process (native, chain, native, ...), wall clock per batch with a device synchronise closing it (the chain's host
stops are part of what it costs), all repeats printed.  Then ONE kernel-trace run of its own: a child process under
    rocprofv3 --kernel-trace --stats -d OUT -o e -- python tools/eval_time.py --profile
(one short native batch per size) whose per-kernel lines are printed.  --no-trace skips it.  Developer tool."""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_statement as es  # noqa: E402
from materialrefgs_amd import evaluate as ev  # noqa: E402

MAPS = (("render", 3, "unit"), ("gt", 3, "unit"), ("rend_normal", 3, "normal"), ("surf_normal", 3, "normal"), ("surf_depth", 1, "depth"),
        ("diffuse_map", 3, "unit"), ("specular_map", 3, "unit"), ("base_color_map", 3, "unit"), ("roughness_map", 1, "unit"),
        ("refl_strength_map", 1, "unit"))


def inputs(H, W, dev):
    g = torch.Generator().manual_seed(H)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    smooth = torch.stack([0.5 + 0.6 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.6 * torch.cos(5 * yy), 0.2 + 1.1 * xx * yy])
    out = {}
    for name, c, mode in MAPS:
        t = smooth[:c] + 0.05 * torch.randn(c, H, W, generator=g)
        out[name] = (t * 2 - 1 if mode == "normal" else t * 4 + 1 if mode == "depth" else t).to(dev)
    return out


def torch_chain(m, window, table):
    """The reference's statements, fp32 on the device."""
    render_color = torch.clamp(m["render"], 0.0, 1.0)[None]                                   # eval.py:44-47
    gt = torch.clamp(m["gt"], 0.0, 1.0)[None]
    conv = lambda x: torch.nn.functional.conv2d(x, window, padding=5, groups=3)
    mu1, mu2 = conv(render_color), conv(gt)                                                   # loss_utils.py:98-110
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(render_color * render_color) - mu1_sq, conv(gt * gt) - mu2_sq, conv(render_color * gt) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    numbers = [ssim_map.mean().item()]                                                        # eval.py:50
    mse = (((render_color - gt) ** 2).reshape(1, -1)).mean(1, keepdim=True)
    numbers.append((20 * torch.log10(1.0 / torch.sqrt(mse))).item())                          # :51
    numbers.append((render_color - gt).abs().mean().item())                                   # the third read (:52 reads the LPIPS value)
    d = m["surf_depth"][0]                                                                    # image_utils.py:75-79 on the device
    level = (((d - d.min()) / (1e-20 + d.max() - d.min())) * 255).clip(0, 255).to(torch.uint8)
    depth_c = table[level.long()].permute(2, 0, 1).float() / 255.0
    to_save = [render_color, gt, m["rend_normal"] * 0.5 + 0.5, m["surf_normal"] * 0.5 + 0.5, depth_c, m["diffuse_map"], m["specular_map"],
               m["base_color_map"], m["roughness_map"], m["refl_strength_map"]]
    host = []
    for item in to_save:                                                                      # eval.py:60-65
        if len(item.shape) > 3:
            item = item.squeeze(0)
        if item.shape[0] == 1:
            item = item.repeat(3, 1, 1)
        host.append(item.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8))
    return numbers, host


def batch(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def kernel_trace(sizes):
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "e", "--", sys.executable, os.path.abspath(__file__), "--profile"] + \
              [str(s) for s in sizes]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print(f"kernel trace: no statistics (rocprofv3 exit {r.returncode})\n{r.stdout[-600:]}")
            return
        print("kernel trace (one run; calls, mean / min / max us):")
        for row in csv.DictReader(open(files[0])):
            for name in ("eval_metrics_kernel", "eval_finalize_kernel", "export_minmax_kernel", "export_rgb8_kernel"):
                if name not in row["Name"]:
                    continue
                print(f"  {name}: {row['Calls']} calls, {float(row['AverageNs']) / 1e3:.1f} / {float(row['MinNs']) / 1e3:.1f} / {float(row['MaxNs']) / 1e3:.1f}")


def main():
    dev = torch.device("cuda:0")
    args = sys.argv[1:]
    profile, trace = "--profile" in args, "--no-trace" not in args
    sizes = [int(a) for a in args if not a.startswith("--")] or [800, 1600]
    batches, n_native, n_torch = (1, 20, 0) if profile else (5, 100, 20)
    window = es.window_2d(torch.float32)[None, None].expand(3, 1, 11, 11).contiguous().to(dev)
    table = torch.from_numpy(ev.jet_table()).to(dev)
    for H in sizes:
        W = H
        m = inputs(H, W, dev)
        rows = torch.zeros((4, 8), device=dev)
        pinned = torch.empty((len(MAPS), H, W, 3), dtype=torch.uint8, pin_memory=True)
        pairs = [(m[name], mode) for name, _c, mode in MAPS]

        def native():
            ev.image_metrics(m["render"], m["gt"], out=rows[1])
            pinned.copy_(ev.to_rgb8(pairs), non_blocking=True)

        def chain():
            return torch_chain(m, window, table)
        native()
        torch.cuda.synchronize()
        if profile:
            batch(native, n_native)
            continue
        numbers, host = chain()
        got = rows[1].cpu()
        same = sum(int(torch.equal(a, b)) for a, b in zip(host, pinned))
        print(f"{H}x{W} check: ssim {float(got[1]):.6f} / chain {numbers[0]:.6f}, psnr {float(got[0]):.4f} / {numbers[1]:.4f}, l1 {float(got[2]):.6f} / "
              f"{numbers[2]:.6f}; {same} of {len(MAPS)} maps byte-equal to the chain's", flush=True)
        for f, n in ((native, n_native), (chain, n_torch)):
            batch(f, n)
        tn, tt = [], []
        for _ in range(batches):
            tn.append(batch(native, n_native))
            tt.append(batch(chain, n_torch))
        read = 4 * sum(c for _n, c, _m in MAPS) * H * W / 1e6
        fmt = lambda xs: ", ".join(f"{v:.3f}" for v in xs)
        print(f"{H}x{W} metrics + export of {len(MAPS)} maps + copy: native {min(tn):.3f} ms per view (metrics read {24 * H * W / 1e6:.1f} MB; export reads "
              f"{read:.1f} MB and writes {3 * len(MAPS) * H * W / 1e6:.1f} MB, copied once), fp32 torch chain {min(tt):.3f} ms, ratio {min(tt) / min(tn):.1f}x; "
              f"native faster in {sum(a < b for a, b in zip(tn, tt))} of {batches} alternated pairs (runs {fmt(tn)} / {fmt(tt)})", flush=True)
    if not profile and trace:
        kernel_trace(sizes)


if __name__ == "__main__":
    main()
