"""Times the training contact sheet (materialrefgs_amd.visualize on csrc/mrgs_sheet.hip) at 800^2 with 12 and with 19 cells and at
1600 x 1200 with 12 cells, per call:
  * the native `contact_sheet` alone (the bytes stay on the device), and with its one non-blocking copy into a pinned buffer;
  * `save_training_vis` with a TrainingVisualizer: the time until the call returns and the time until the file exists under its final name
    (the copy, zlib at level 1 on the worker thread, the rename);
  * beside them the fp32 torch form of the reference's statements on the same GPU (train_refreal.py:1518-1606 and save_image's byte
    conversion): the list with a(x), the three colour-map helpers WITH their .cpu() round trips (utils/image_utils.py:65-93; this library's jet
    table indexed in numpy where cv2.applyColorMap stood), torch.stack, make_grid restated from torchvision's source, F.interpolate, and
    mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).
The PNG encoder is left out of both "sheet" figures.  cv2's and torchvision's own CPU time cannot be measured here (neither is installed): the
torch form's host work is numpy's only.

Batches alternate in one process (native, torch form, native, ...), wall clock per batch with a device synchronise closing it, all repeats
printed.  Then ONE kernel-trace run of its own: a child process under
    rocprofv3 --kernel-trace --stats -d OUT -o v -- python tools/vis_time.py --profile
whose per-kernel lines are printed.  --no-trace skips it.  Developer tool."""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sheet_statement as ss  # noqa: E402
from materialrefgs_amd import evaluate as ev  # noqa: E402
from materialrefgs_amd import visualize as vz  # noqa: E402

CONFIGS = ((800, 800, 12), (800, 800, 19), (1200, 1600, 12))


def inputs(H, W, n, dev):
    """A render_pkg, a camera and the optional maps of a sheet of n cells (12: the surfel stage's list; 19: + rend_distance, d_mask,
    ref_weight, base_color_loss_map and the three light maps)."""
    g = torch.Generator().manual_seed(H + n)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    smooth = torch.stack([0.5 + 0.6 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.6 * torch.cos(5 * yy), 0.2 + 1.1 * xx * yy])
    img = lambda c: (smooth[:c] + 0.05 * torch.randn(c, H, W, generator=g)).to(dev)
    nrm = lambda: torch.nn.functional.normalize(torch.randn(3, H, W, generator=g) + smooth, dim=0).to(dev)
    pkg = {"render": img(3), "base_color_map": img(3), "diffuse_map": img(3), "specular_map": img(3), "refl_strength_map": img(1),
           "roughness_map": img(1), "rend_alpha": img(1), "surf_depth": img(1) * 4 + 1, "rend_normal": nrm(), "surf_normal": nrm()}
    extras = dict(d_mask=None, ref_weight=None, base_color_loss_map=None)
    if n == 19:
        pkg.update({"rend_distance": img(1) * 2, "visibility": img(1), "direct_light": img(3), "indirect_light": img(3)})
        extras = dict(d_mask=(torch.rand(H * W, generator=g) > 0.5).to(dev), ref_weight=img(1), base_color_loss_map=(img(1)[0] ** 2))
    q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((3, 3)))
    cam = SimpleNamespace(original_image=img(3), R=q.astype(np.float32))
    return cam, pkg, extras


# ---- the reference's statements, fp32 on the device -----------------------------------------------------------------------------------------
def _jet(levels_u8, table_np, dev):
    depth_c = table_np[levels_u8]                                       # cv2.applyColorMap(..., COLORMAP_JET)[..., ::-1]
    return torch.from_numpy(depth_c).float().to(dev).permute(2, 0, 1) / 255.


def ref_visualize_depth(depth, table_np, norm=True):
    dev = depth.device
    depth = depth.detach().cpu().squeeze().numpy()
    if norm:
        depth = (depth - depth.min()) / (1e-20 + depth.max() - depth.min())
    return _jet((depth * 255).clip(0, 255).astype(np.uint8), table_np, dev)


def ref_visualize_depth2(depth, table_np):
    dev = depth.device
    depth = depth.detach().cpu().squeeze().numpy()
    std = depth.std()
    depth = depth.clip(0, 6 * std)
    depth = (depth - depth.min()) / (1e-20 + depth.max() - depth.min())
    return _jet((depth * 255).clip(0, 255).astype(np.uint8), table_np, dev)


def ref_visualize_d_mask(d_mask, H, W, table_np):
    return _jet((d_mask.float() * 255).detach().cpu().numpy().astype(np.uint8).reshape(H, W), table_np, d_mask.device)


def torch_sheet(cam, pkg, extras, table_np):
    """:1518-1606 and save_image's conversion; returns the host bytes [Ho,Wo,3]."""
    error_map = torch.abs(cam.original_image - pkg["render"])
    rot = torch.from_numpy(cam.R).T.float().to(error_map.device)

    def a(x):
        sz = x.shape
        x = (rot @ x.reshape(3, -1)).reshape(*sz)[[2, 1, 0], ...]
        return 0.5 * x + 0.5
    lst = [cam.original_image, pkg["render"], pkg["base_color_map"], pkg["diffuse_map"], pkg["specular_map"], pkg["refl_strength_map"].repeat(3, 1, 1),
           pkg["roughness_map"].repeat(3, 1, 1), pkg["rend_alpha"].repeat(3, 1, 1), ref_visualize_depth(pkg["surf_depth"], table_np),
           a(pkg["rend_normal"]), a(pkg["surf_normal"]), error_map]
    if "rend_distance" in pkg:
        lst.append(ref_visualize_depth(pkg["rend_distance"], table_np))
    if extras["d_mask"] is not None:
        lst.append(ref_visualize_d_mask(extras["d_mask"], pkg["rend_normal"].shape[1], pkg["rend_normal"].shape[2], table_np))
    if extras["ref_weight"] is not None:
        lst.append(ref_visualize_depth(extras["ref_weight"], table_np, norm=False))
    if extras["base_color_loss_map"] is not None:
        lst.append(ref_visualize_depth2(extras["base_color_loss_map"], table_np))
    if "visibility" in pkg:
        lst += [pkg["visibility"].repeat(3, 1, 1), pkg["direct_light"], pkg["indirect_light"]]
    grid = torch.stack(lst, dim=0)
    grid = ss.make_grid(grid, nrow=4)
    scale = grid.shape[-2] / 2400
    grid = F.interpolate(grid[None], (int(grid.shape[-2] / scale), int(grid.shape[-1] / scale)))[0]
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)


def batch(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def kernel_trace():
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "v", "--", sys.executable, os.path.abspath(__file__), "--profile"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print(f"kernel trace: no statistics (rocprofv3 exit {r.returncode})\n{r.stdout[-600:]}")
            return
        print("kernel trace (one run over the three configurations; calls, mean / min / max us):")
        for row in csv.DictReader(open(files[0])):
            for name in ("sheet_stats_kernel", "sheet_rgb8_kernel"):
                if name in row["Name"]:
                    print(f"  {name}: {row['Calls']} calls, {float(row['AverageNs']) / 1e3:.1f} / {float(row['MinNs']) / 1e3:.1f} / {float(row['MaxNs']) / 1e3:.1f}")


def main():
    dev = torch.device("cuda:0")
    args = sys.argv[1:]
    profile, trace = "--profile" in args, "--no-trace" not in args
    batches, n_native, n_torch, n_save = (1, 10, 0, 0) if profile else (5, 20, 5, 4)
    table_np = ev.jet_table()
    opt = SimpleNamespace(volume_render_until_iter=0, init_until_iter=0, indirect=False, srgb=False)
    env = {"env1": torch.rand(64, 128, 3, device=dev), "env2": torch.rand(64, 128, 3, device=dev)}
    gaussians = SimpleNamespace(render_env_map=lambda: env, render_env_map_2=lambda: env)
    fmt = lambda xs: ", ".join(f"{v:.2f}" for v in xs)
    for H, W, n in CONFIGS:
        cam, pkg, extras = inputs(H, W, n, dev)
        cells = [c for _, c in vz.training_cells(cam, pkg, opt, 400, False, **extras)]
        assert len(cells) == n
        rot = vz.view_rotation(cam)
        Hg, Wg, Ho, Wo = vz.sheet_layout(n, H, W)
        pinned = torch.empty((Ho, Wo, 3), dtype=torch.uint8, pin_memory=True)

        def native():
            return vz.contact_sheet(cells, rot=rot)

        def native_copy():
            pinned.copy_(vz.contact_sheet(cells, rot=rot), non_blocking=True)

        def chain():
            return torch_sheet(cam, pkg, extras, table_np)
        native_copy()
        torch.cuda.synchronize()
        if profile:
            batch(native, n_native)
            continue
        host = chain()
        diff = int((host.numpy() != pinned.numpy()).sum())
        print(f"{H}x{W}, {n} cells -> {Ho}x{Wo} ({3 * Ho * Wo / 1e6:.1f} MB): {diff} of {host.numel()} bytes differ from the torch form's "
              f"(normal_view / depth2 bytes may, by one)", flush=True)
        for f, k in ((native, n_native), (native_copy, n_native), (chain, n_torch)):
            batch(f, max(1, k // 2))
        ta, tn, tt = [], [], []
        for _ in range(batches):
            ta.append(batch(native, n_native))
            tn.append(batch(native_copy, n_native))
            tt.append(batch(chain, n_torch))
        print(f"  contact_sheet alone {min(ta):.3f} ms (runs {fmt(ta)}); with the copy to a pinned buffer {min(tn):.3f} ms (runs {fmt(tn)}); fp32 torch "
              f"form {min(tt):.2f} ms (runs {fmt(tt)}), ratio {min(tt) / min(tn):.1f}x; native faster in {sum(x < y for x, y in zip(tn, tt))} of {batches} "
              f"alternated pairs", flush=True)
        with tempfile.TemporaryDirectory() as folder:
            vis = vz.TrainingVisualizer(folder)
            t_ret, t_file = [], []
            for i in range(n_save):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                path = vis.save(cam, gaussians, None, None, None, opt, i, False, extras["d_mask"], extras["ref_weight"], extras["base_color_loss_map"], pkg)[0]
                t1 = time.perf_counter()
                while not os.path.exists(path):
                    time.sleep(0.001)
                t_ret.append((t1 - t0) * 1e3)
                t_file.append((time.perf_counter() - t0) * 1e3)
            vis.close()
            size = os.path.getsize(path) / 1e6
        print(f"  save_training_vis with a TrainingVisualizer (and its 64x128 env sheet): returns after {min(t_ret):.2f} ms (runs {fmt(t_ret)}; the first "
              f"allocates the pinned ring), the file ({size:.1f} MB at zlib level 1) exists after {min(t_file):.0f} ms (runs {fmt(t_file)})", flush=True)
    if not profile and trace:
        kernel_trace()


if __name__ == "__main__":
    main()
