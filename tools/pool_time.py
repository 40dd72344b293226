"""Times pointnet2_ops' ball_query (materialrefgs_amd.ballquery on csrc/mrgs_ballquery.hip) and the fused 3D max-pooling of the reflection
score (refscore.ref_scores_max_pooling) on clouds lifted from rendered depth maps of the bench scene (the synthetic surfel model,
render_surfel("pgsr"), views every 18 degrees of the orbit).

  1. ball_query(r, 49, cloud, cloud) on the image-ordered cloud of 4 views and on a random permutation of it, at 200^2 and 400^2 a view
     (160 000 and 640 000 points), r = 0.1 and 0.01 of the scene extent; at 200^2 beside a chunked fp32 torch brute force (cdist chunks,
     the first 49 hits by a masked top-k, padding) -- the largest size at which that quadratic form finishes in about a second.
  2. ref_scores_max_pooling over 20 views at 800^2 (12.8 M points; points kernel + walk, workspace allocation included), ratios 0.1 and
     0.01; the brute force does not fit there (1.6e14 pairs) and is timed at 4 views of 200^2 instead, beside the native call there.

Native and torch batches alternate in one process, a synchronise around each batch, device events, the minimum and all batches
printed (five native batches, the torch form beside the first three).  Before anything is timed, the walk's result is compared with
the statement (the fp32 brute force of tests/pool_statement.py, evaluated on the device one operation at a time) on a subsample of the
queries of the very clouds that are timed, and the peak of the allocator during a pooled call is printed beside the size of the
[points, 49] index tensor it never builds.  Per-kernel times:
    rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/pool_time.py
Developer tool."""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import refscore  # noqa: E402
from materialrefgs_amd.ballquery import ball_query, points_from_depth  # noqa: E402
from materialrefgs_amd.camera import look_at_camera  # noqa: E402
from materialrefgs_amd.synthetic import CAM_DISTANCE, FOV, make_surfel_model  # noqa: E402

P_SURFELS, NSAMPLE = 300_000, 49
EXTENT = 1.1 * CAM_DISTANCE          # scene.cameras_extent of an orbit: 1.1 times the largest distance of a camera from their centre
PIPE = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)


def timed(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def views(n_views, size, dev):
    """(cameras with image_name, depth maps [size,size]) of the bench scene."""
    from materialrefgs_amd.renderer import render_surfel
    pc, env, _ = make_surfel_model(P_SURFELS, size, dev, seed=0)
    env.build_mips()
    bg = torch.zeros(3, device=dev)
    cams, depths = [], []
    with torch.no_grad():
        for i in range(n_views):
            mini = look_at_camera(17.0 + 18.0 * i, 30.0, CAM_DISTANCE, FOV, size, size)
            pk = render_surfel(mini.to(dev), pc, PIPE, bg, srgb=False, opt=SimpleNamespace(indirect=False), flag="pgsr")
            cams.append(SimpleNamespace(image_name=f"v{i:02d}", image_height=size, image_width=size, FoVx=mini.FoVx, FoVy=mini.FoVy, R=mini.R, T=mini.T))
            depths.append(pk["surf_depth"].reshape(size, size).clone())
    return cams, depths


def first_hits(q, x, r, nsample):
    """The statement's rows for the queries q against the cloud x, on the device, every operation rounded on its own: (keys [Q,nsample]
    with N for a missing hit, ascending)."""
    N = x.shape[0]
    ar = torch.arange(N, device=x.device, dtype=torch.int32)
    r2 = torch.tensor(r, dtype=torch.float32, device=x.device)
    r2 = r2 * r2
    rows = []
    for s in range(0, q.shape[0], 8):
        d = [(q[s:s + 8, None, k] - x[None, :, k]) for k in range(3)]
        dist = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        key = torch.where(dist < r2, ar[None, :], torch.full((), N, dtype=torch.int32, device=x.device))
        rows.append(key.topk(min(nsample, N), dim=1, largest=False).values)
    return torch.cat(rows)


def rows_from_keys(keys, N):
    first = torch.where(keys[:, :1] == N, torch.zeros_like(keys[:, :1]), keys[:, :1])
    return torch.where(keys == N, first, keys)


def torch_ball_query(x, r, nsample, chunk=2048):
    """The brute force a ROCm user could run: cdist chunks, the first nsample hits by a masked top-k, padded."""
    N = x.shape[0]
    ar = torch.arange(N, device=x.device, dtype=torch.int32)
    out = torch.empty((N, nsample), dtype=torch.int32, device=x.device)
    for s in range(0, N, chunk):
        d = torch.cdist(x[s:s + chunk], x, compute_mode="donot_use_mm_for_euclid_dist")
        key = torch.where(d < r, ar[None, :], torch.full((), N, dtype=torch.int32, device=x.device))
        out[s:s + chunk] = rows_from_keys(key.topk(nsample, dim=1, largest=False).values, N)
    return out


def check_rows(x, r, got, n_check, what):
    sel = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1))[:n_check].to(x.device)
    want = rows_from_keys(first_hits(x[sel], x, r, NSAMPLE), x.shape[0])
    same = bool(torch.equal(got[sel], want))
    hits = (first_hits(x[sel], x, r, NSAMPLE) < x.shape[0]).sum(dim=1)
    print(f"  {what}: {n_check} sampled rows equal the statement: {same}; of them {int((hits >= NSAMPLE).sum())} saturated, {int((hits == 0).sum())} empty",
          flush=True)
    if not same:
        raise SystemExit("the walk differs from the statement")


def main():
    dev = torch.device("cuda:0")
    fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)
    # ---- 1. ball_query ----
    for size in (200, 400):
        cams, depths = views(4, size, dev)
        cloud = points_from_depth(cams, depths)
        perm = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(0)).to(dev)
        for ratio in (0.1, 0.01):
            r = EXTENT * ratio
            for name, x in (("image order", cloud), ("permuted", cloud[perm].contiguous())):
                call = lambda: ball_query(r, NSAMPLE, x[None], x[None])
                got = call()[0]
                check_rows(x, r, got, 256, f"{size}^2 x 4 {name} r {r:.4f}")
                with_torch = size == 200
                tn, tt = [], []
                for batch in range(5):
                    tn.append(timed(call, 5))
                    if with_torch and batch < 3:
                        tt.append(timed(lambda: torch_ball_query(x, r, NSAMPLE), 1))
                line = f"ball_query N = M = {x.shape[0]} ({name}), nsample {NSAMPLE}, r {r:.4f}: native {min(tn):.3f} ms (runs {fmt(tn)})"
                if with_torch:
                    line += f"; torch brute force {min(tt):.1f} ms (runs {fmt(tt)}), ratio {min(tt) / min(tn):.0f}x"
                print(line, flush=True)
    # ---- 2. the fused pooling ----
    for n_views, size, with_torch in ((4, 200, True), (20, 800, False)):
        cams, depths = views(n_views, size, dev)
        gen = torch.Generator().manual_seed(3)
        scores = [torch.rand(size, size, generator=gen).to(dev) for _ in cams]
        N = n_views * size * size
        for ratio in (0.1, 0.01):
            call = lambda: refscore.ref_scores_max_pooling(scores, cams, EXTENT, ratio, NSAMPLE, depth_images=depths)
            out = call()
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            out = call()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev) - before
            pooled = torch.cat([out[c.image_name].reshape(-1) for c in cams])
            x, score = points_from_depth(cams, depths), torch.cat([s.reshape(-1) for s in scores])
            r = EXTENT * ratio
            sel = torch.randperm(N, generator=torch.Generator().manual_seed(2))[:64 if N > 10 ** 6 else 256].to(dev)
            keys = first_hits(x[sel], x, r, NSAMPLE)
            vals = torch.where(keys == N, torch.full((), float("-inf"), device=dev), score[keys.clamp(max=N - 1).long()]).max(dim=1).values
            want = torch.where(keys[:, 0] == N, score[0], vals)
            same = bool(torch.equal(pooled[sel], want))
            print(f"  pooling {n_views} x {size}^2 ratio {ratio}: {len(sel)} sampled pixels equal the statement: {same}; peak allocation of the call "
                  f"{peak / 1e6:.1f} MB, a [points, {NSAMPLE}] int32 tensor would be {N * NSAMPLE * 4 / 1e6:.1f} MB", flush=True)
            if not same:
                raise SystemExit("the pooling differs from the statement")

            def torch_form():
                idx = torch_ball_query(x, r, NSAMPLE)
                return score[idx.long()].max(dim=1).values
            tn, tt = [], []
            for batch in range(5):
                tn.append(timed(call, 3))
                if with_torch and batch < 3:
                    tt.append(timed(torch_form, 1))
            line = f"ref_scores_max_pooling {n_views} views x {size}^2 = {N} points, ratio {ratio} (r {r:.4f}): native {min(tn):.3f} ms (runs {fmt(tn)})"
            if with_torch:
                line += f"; torch brute force (ball query + gather + max, points given) {min(tt):.1f} ms (runs {fmt(tt)}), ratio {min(tt) / min(tn):.0f}x"
            print(line, flush=True)


if __name__ == "__main__":
    main()
