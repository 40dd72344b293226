"""Times the mesh step of the training loop (materialrefgs_amd/mesh.py, csrc/mrgs_mesh.hip) on the bench's scene: 120 views of the
300 000-surfel shell at 800 x 800 rendered once through render_surfel (GaussianExtractor.reconstruction: the depth maps stay on the
device), then on plain lattices of 256^3 and 512^3 points over the cube [-1.25, 1.25]^3, truncation five voxels:
  fusion          mrgs_tsdf_fuse, one launch over all views
  count + emit    marching tetrahedra (the 16-byte host read of V and T lies inside the window), with V and T
  clusters        mrgs_mesh_clusters (hooking, pointer jumping, per-label counts); post_process_mesh as a whole beside it
  texturing       mrgs_vertex_fuse (fuse_vertex_attributes) on the vertices of that lattice's mesh, all 120 views, CP = 4 and CP = 16
                  channels; the attribute maps are uniform noise made on the device (the kernel's traffic does not depend on their
                  values).  Beside each, in the same run: the fp32 torch form of the same rule, the grid_sample loop of
                  compute_unbounded_tsdf(..., return_rgb=True) (utils/mesh_utils.py:352-368) with the maps already on the device
                  (channel-first, as grid_sample takes them) -- the best a ROCm user has without this kernel -- and the largest
                  difference of the two results over the vertices on which both count the same views.
Beside the fusion at 256^3: the fp32 torch form of the same rule, the reference's own loop (compute_unbounded_tsdf /
compute_sdf_perframe, utils/mesh_utils.py:322-373) restated, in the same run, and the largest difference of the two fields.
Each figure is the time between two device events around a batch of 4 calls, divided by 4, after a warm-up call: the minimum of 5
batches, all of them printed.  The window holds the whole Python call, not the kernels alone: torch's allocations of the outputs and
the workspace, for the fusion the host read of the 120 projection matrices and the copy of the view table to the device, for count +
emit the 16-byte host read of V and T, for post_process_mesh the read of the label counts and two compaction counts.  The cluster
kernels take well under a millisecond, so their figure is mostly launches and the allocator; per-kernel times want
rocprofv3 --kernel-trace --stats in a run of its own.  Records, not bars: neither the reference's stack (Open3D, skimage, trimesh on
host copies) nor an earlier revision of this library has anything to compare with.  Developer tool; arguments: lattice sizes (default 256 512)."""
import math
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import mesh  # noqa: E402
from materialrefgs_amd.camera import look_at_camera  # noqa: E402
from materialrefgs_amd.synthetic import CAM_DISTANCE, FOV, make_surfel_model  # noqa: E402

P, SIZE, N_VIEWS, HALF = 300_000, 800, 120, 1.25


def event_ms(fn, batches=5, calls=4):
    fn()                                                            # warm-up: code objects, allocator
    out, times = None, []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return times, out


def torch_fuse(views, points, trunc):
    """compute_unbounded_tsdf without contraction and colours, fp32 on the device."""
    tsdfs, weights = torch.ones_like(points[:, 0]), torch.ones_like(points[:, 0])
    for proj, depth in views:
        new_points = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1) @ proj
        z = new_points[..., -1:]
        pix = new_points[..., :2] / new_points[..., -1:]
        mask = ((pix > -1.0) & (pix < 1.0) & (z > 0)).all(dim=-1)
        sampled = torch.nn.functional.grid_sample(depth[None], pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(-1, 1)
        sdf = (sampled - z).flatten()
        mask = mask & (sdf > -trunc)
        sdf = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[mask]
        w = weights[mask]
        tsdfs[mask] = (tsdfs[mask] * w + sdf) / (w + 1)
        weights[mask] = w + 1
    return tsdfs


def torch_texture(views, points, trunc):
    """compute_unbounded_tsdf(..., return_rgb=True) without contraction, fp32 on the device; views are (proj, depth [1,H,W], maps [C,H,W])."""
    tsdfs, weights = torch.ones_like(points[:, 0]), torch.ones_like(points[:, 0])
    rgbs = torch.zeros((points.shape[0], views[0][2].shape[0]), device=points.device)
    for proj, depth, amap in views:
        new_points = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1) @ proj
        z = new_points[..., -1:]
        pix = new_points[..., :2] / new_points[..., -1:]
        mask = ((pix > -1.0) & (pix < 1.0) & (z > 0)).all(dim=-1)
        sampled = torch.nn.functional.grid_sample(depth[None], pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(-1, 1)
        rgb = torch.nn.functional.grid_sample(amap[None], pix[None, None], mode="bilinear", padding_mode="border", align_corners=True).reshape(amap.shape[0], -1).T
        sdf = (sampled - z).flatten()
        mask = mask & (sdf > -trunc)
        sdf = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[mask]
        w = weights[mask]
        wp = w + 1
        tsdfs[mask] = (tsdfs[mask] * w + sdf) / wp
        rgbs[mask] = (rgbs[mask] * w[:, None] + rgb[mask]) / wp[:, None]
        weights[mask] = wp
    return rgbs, weights


def time_texturing(n, m, cams, depthmaps, trunc, fmt):
    dev = m.vertices_device.device
    V = m.vertices_device.shape[0]
    for cp in (4, 16):
        gen = torch.Generator(device=dev).manual_seed(cp)
        packed = [torch.rand(SIZE, SIZE, cp, device=dev, generator=gen) for _ in cams]
        views = [(c.full_proj_transform, d, a) for c, d, a in zip(cams, depthmaps, packed)]
        t_k, (out, w) = event_ms(lambda: mesh.fuse_vertex_attributes(m.vertices_device, views, trunc, return_weight=True))
        pairs = float((w - 1).sum())
        print(f"lattice {n}^3: texturing V {V}, CP {cp}: {min(t_k):.3f} ms (batches {fmt(t_k)}); {pairs / V:.1f} accepted views per vertex, "
              f"{pairs * 16 * (cp + 1) / 2 ** 30:.2f} GiB of taps, maps {len(cams) * SIZE * SIZE * cp * 4 / 2 ** 30:.2f} GiB", flush=True)
        first = [(c.full_proj_transform, d, a.permute(2, 0, 1).contiguous()) for c, d, a in zip(cams, depthmaps, packed)]
        t_t, (ref, ref_w) = event_ms(lambda: torch_texture(first, m.vertices_device, trunc))
        same = ref_w == w
        print(f"lattice {n}^3: torch form of the texturing, CP {cp}: {min(t_t):.3f} ms (batches {fmt(t_t)}), ratio {min(t_t) / min(t_k):.1f}x; "
              f"{int((~same).sum())} of {V} vertices count other views (a decision at a threshold), the others differ by at most "
              f"{float((ref - out)[same].abs().max()):.3e}", flush=True)
        del packed, views, first, out, w, ref, ref_w
        torch.cuda.empty_cache()


def main():
    from materialrefgs_amd.renderer import render_surfel
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [256, 512]
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    pc, env, _ = make_surfel_model(P, SIZE, dev, seed=0)
    env.build_mips()
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    cams = [look_at_camera(3.0 * i + 17.0, (-40.0, -10.0, 20.0, 50.0)[i % 4], CAM_DISTANCE, FOV, SIZE, SIZE).to(dev) for i in range(N_VIEWS)]
    render = lambda cam, model, pipe, bg_color, opt=None: render_surfel(cam, model, pipe, bg_color, srgb=False, opt=opt, wo_render_img=True)
    ex = mesh.GaussianExtractor(pc, render, pipe)
    ex.reconstruction(cams, opt=SimpleNamespace(indirect=False))
    views = [(c.full_proj_transform, d) for c, d in zip(cams, ex.depthmaps)]
    print(f"{N_VIEWS} views of {SIZE} x {SIZE}, P {P}; depth maps {sum(d.numel() for d in ex.depthmaps) * 4 / 2 ** 20:.0f} MiB on the device", flush=True)
    for n in sizes:
        spacing = 2 * HALF / (n - 1)
        trunc = 5 * spacing
        lattice = dict(shape=(n, n, n), origin=-HALF, spacing=spacing)
        t_fuse, field = event_ms(lambda: mesh.tsdf_fuse(views, trunc, **lattice))
        print(f"lattice {n}^3: fusion {min(t_fuse):.3f} ms (batches {fmt(t_fuse)}), {4 * n ** 3 / 2 ** 20:.0f} MiB written", flush=True)
        if n == 256:
            ax = torch.linspace(-HALF, HALF, n, device=dev)
            pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
            t_torch, ref = event_ms(lambda: torch_fuse(views, pts, trunc))
            diff = (ref - field.reshape(-1)).abs()
            print(f"lattice {n}^3: torch form of the fusion {min(t_torch):.3f} ms (batches {fmt(t_torch)}), ratio {min(t_torch) / min(t_fuse):.1f}x; "
                  f"{int((diff > 1e-3).sum())} of {n ** 3} samples differ by more than 1e-3 (a decision at a threshold), the others by at most "
                  f"{float(diff[diff <= 1e-3].max()):.3e}",
                  flush=True)
            del pts, ref, diff
        t_mt, m = event_ms(lambda: mesh.marching_tetrahedra(field, 0.0, -HALF, spacing))
        V, T = m.vertices_device.shape[0], m.triangles_device.shape[0]
        print(f"lattice {n}^3: count + emit {min(t_mt):.3f} ms (batches {fmt(t_mt)}): V {V}, T {T}", flush=True)
        t_cl, _ = event_ms(lambda: mesh.cluster_triangles(m))
        t_pp, kept = event_ms(lambda: mesh.post_process_mesh(m, 50))
        print(f"lattice {n}^3: clusters {min(t_cl):.3f} ms (batches {fmt(t_cl)}); post_process_mesh(50) {min(t_pp):.3f} ms (batches {fmt(t_pp)}) "
              f"-> V {kept.vertices_device.shape[0]}, T {kept.triangles_device.shape[0]}", flush=True)
        del field, kept
        time_texturing(n, m, cams, ex.depthmaps, trunc, fmt)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
