"""refscore.ref_scores_max_pooling / ref_scores_max_pooling_wiht_mask and ballquery.points_from_depth (libmrgs.so: csrc/mrgs_ballquery.hip)
against their statements (tests/pool_statement.py).

The scene: 3 views of synthetic.orbit_camera at 24 x 32, depth and score maps from a seeded generator, the depth with some zeros and one NaN
pixel.  The points compare with the float64 statement within 2e-7 relative + 2e-7 of the largest coordinate.  The allowance for the fp32
rounding of a three-term product ((x - Cx) / Fx z: three roundings, 1.8e-7 relative), one subtraction and a 3 x 3 rotation (five
roundings on terms no larger than the largest coordinate plus |T|) is 2e-6 relative + 1e-6 of the largest coordinate; the run shows a
worst error of 2.4e-7 absolute = 7.2e-8 of the largest coordinate (3.338; MI355X, 2026-10-20), and the bar is tightened to three times
that.  The pooled maps compare BIT FOR BIT with the statement evaluated on the points the module
itself produced: every decision (d < r2) is then taken on identical numbers."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pool_statement as ps

V, H, W = 3, 24, 32
EXTENT = 1.0
RATIOS = (0.5, 0.1)               # of EXTENT: a ball that holds more than 49 points for most pixels, and one that does not
FPS_RATIOS = (0.1, 0.02)          # of the distance between the two sampled points


def _cams():
    from materialrefgs_amd.synthetic import orbit_camera
    out = []
    for v in range(V):
        c = orbit_camera(v, H, W)
        out.append(SimpleNamespace(image_name=f"view_{v:03d}", image_height=H, image_width=W, FoVx=c.FoVx, FoVy=c.FoVy, R=c.R, T=c.T))
    return out


@functools.lru_cache(maxsize=None)
def _maps():
    rng = np.random.default_rng(20)
    depth = rng.uniform(3.0, 4.0, size=(V, H, W)).astype(np.float32)
    depth[rng.random((V, H, W)) < 0.05] = 0.0
    depth[0, 0, 0] = 3.5                                   # point 0 (the zero row's target, the sampler's first pick) is an ordinary point
    depth[1, 5, 7] = np.nan
    score = rng.random((V, H, W)).astype(np.float32)
    mask = rng.random((V, H, W)) > 0.4
    return depth, score, mask


def _focal(cam):
    from materialrefgs_amd._camconst import focal
    return focal(cam)


_STATE = {}


def _scene(dev):
    """Device maps and the module's own points (host copy), built once."""
    if "scene" not in _STATE:
        from materialrefgs_amd.ballquery import points_from_depth
        depth, score, mask = _maps()
        cams = _cams()
        d = [torch.from_numpy(depth[v].copy()).to(dev) for v in range(V)]
        s = [torch.from_numpy(score[v].copy()).to(dev) for v in range(V)]
        m = [torch.from_numpy(mask[v].copy()).to(dev) for v in range(V)]
        pts = points_from_depth(cams, d)
        _STATE["scene"] = SimpleNamespace(cams=cams, depth=d, score=s, mask=m, points=pts, points_host=pts.cpu().numpy())
    return _STATE["scene"]


def _stack(pooled, cams):
    return torch.stack([pooled[c.image_name] for c in cams]).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- refusals (no GPU needed) -----------------------------------------------------------------------------------------------------------
def test_refusals():
    from materialrefgs_amd.refscore import ref_scores_max_pooling, ref_scores_max_pooling_wiht_mask
    from materialrefgs_amd.ballquery import points_from_depth
    cams = _cams()
    maps = [torch.zeros(H, W) for _ in cams]
    with pytest.raises(TypeError, match="depth_images"):
        ref_scores_max_pooling(maps, cams, 1.0)
    with pytest.raises(TypeError, match="depth_images"):
        ref_scores_max_pooling_wiht_mask(maps, maps, cams, 1.0)
    with pytest.raises(NotImplementedError, match="Only ball query"):
        ref_scores_max_pooling(maps, cams, 1.0, backend="knn", depth_images=maps)
    with pytest.raises(NotImplementedError, match="Only ball query"):
        ref_scores_max_pooling_wiht_mask(maps, maps, cams, 1.0, 0.1, 49, "knn", depth_images=maps)
    with pytest.raises(ValueError, match="2 ref_score_images for 3 cameras"):
        ref_scores_max_pooling(maps[:2], cams, 1.0, depth_images=maps)
    with pytest.raises(ValueError, match="elements"):
        ref_scores_max_pooling(maps, cams, 1.0, depth_images=[torch.zeros(H, W + 1) for _ in cams])
    with pytest.raises(ValueError, match="no entry"):
        ref_scores_max_pooling({"other": maps[0]}, cams, 1.0, depth_images=maps)
    with pytest.raises(ValueError, match="one image size"):
        ref_scores_max_pooling(maps, cams[:2] + [SimpleNamespace(**{**vars(cams[2]), "image_width": W + 2})], 1.0, depth_images=maps)
    with pytest.raises(RuntimeError, match="device tensor"):                  # CPU tensors: there is no fallback
        ref_scores_max_pooling(maps, cams, 1.0, depth_images=maps)
    with pytest.raises(RuntimeError, match="device tensor"):
        ref_scores_max_pooling_wiht_mask(maps, maps, cams, 1.0, depth_images=maps)
    with pytest.raises(RuntimeError, match="device tensor"):
        points_from_depth(cams, maps)


def test_statement_of_the_pooling_on_a_hand_case():
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5, 5, 5], [np.nan, 0, 0]], np.float32)
    score = np.array([1, 5, 3, 2, 9], np.float32)
    # r = 0.15: point 0 sees {0, 1}, 1 sees {0, 1, 2}, 2 sees {1, 2}, 3 itself; the NaN row sees nothing and takes score[0]
    assert ps.max_pool(pts, score, np.float32(0.15), 49, None).tolist() == [5, 5, 5, 2, 1]
    assert ps.max_pool(pts, score, np.float32(0.15), 1, None).tolist() == [1, 1, 5, 2, 1]          # the first hit only
    valid = np.array([1, 0, 1, 1, 1], bool)
    assert ps.max_pool(pts, score, np.float32(0.15), 49, valid).tolist() == [1, 5, 3, 2, 9]        # without point 1 nobody has a neighbour


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_points_from_depth_against_float64(gpu_device):
    sc = _scene(gpu_device)
    want = ps.points64(sc.cams, [d for d in _maps()[0]], _focal)
    got = sc.points_host.astype(np.float64)
    assert got.shape == (V * H * W, 3) and sc.points.dtype == torch.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)) and int(np.isnan(want).any(axis=1).sum()) == 1
    ok = ~np.isnan(want)
    top = float(np.abs(want[ok]).max())
    err = np.abs(got[ok] - want[ok])
    print(f"points_from_depth: worst |error| {err.max():.3e} = {err.max() / top:.3e} of the largest coordinate {top:.3f}")
    assert np.all(err <= 2e-7 * np.abs(want[ok]) + 2e-7 * top)
    # image order: point i H W + y W + x; a zero depth lands on its camera's centre, -T @ R^T
    centre = -(sc.cams[2].T.double() @ sc.cams[2].R.double().T).numpy()
    zero = np.flatnonzero(_maps()[0][2].reshape(-1) == 0)
    assert len(zero) > 5 and np.allclose(got[2 * H * W + zero], centre[None], atol=1e-5)


def _want(sc, r, n_samples, masked):
    depth, score, mask = _maps()
    valid = mask.reshape(-1) if masked else None
    return ps.max_pool(sc.points_host, score.reshape(-1), r, n_samples, valid).reshape(V, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("n_samples", (1, 49))
def test_pooling_equals_the_statement_bit_for_bit(gpu_device, n_samples, ratio, masked):
    from materialrefgs_amd.refscore import ref_scores_max_pooling, ref_scores_max_pooling_wiht_mask
    sc = _scene(gpu_device)
    if masked:
        out = ref_scores_max_pooling_wiht_mask(sc.score, sc.mask, sc.cams, EXTENT, ratio, n_samples, depth_images=sc.depth)
    else:
        out = ref_scores_max_pooling(sc.score, sc.cams, EXTENT, ratio, n_samples, depth_images=sc.depth)
    assert list(out) == [c.image_name for c in sc.cams]
    for t in out.values():
        assert t.shape == (H, W) and t.dtype == torch.float32 and t.device.type == "cuda" and t.requires_grad is False
    got = _stack(out, sc.cams)
    want = _want(sc, np.float32(EXTENT * ratio), n_samples, masked)
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    score, mask = _maps()[1], _maps()[2]
    if masked:
        assert np.array_equal(_bits(got[~mask]), _bits(score[~mask]))              # unmasked pixels keep their score bit for bit
    assert (got != score).mean() > (0.05 if n_samples == 49 else 0.02)             # and the pooling did change others
    if n_samples == 49 and not masked:
        # the condition on the inputs: the large ball saturates most rows, the small one hardly any
        hits = ps.ball_query(np.float32(EXTENT * ratio), 49, sc.points_host[None], sc.points_host[None], return_hits=True)[1]
        share = float(np.mean(hits >= 49))
        assert share > 0.5 if ratio == RATIOS[0] else share < 0.05, share


@pytest.mark.gpu
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("ratio", FPS_RATIOS)
def test_pooling_with_the_sampled_radius(gpu_device, ratio, masked):
    """calc_depth_points_radius: |p[f0] - p[f1]| * ratio with f = furthest_point_sample(points, 2), never read by the host."""
    from materialrefgs_amd.refscore import ref_scores_max_pooling, ref_scores_max_pooling_wiht_mask
    sc = _scene(gpu_device)
    r = ps.fps_radius(sc.points_host, ratio)
    assert 0.05 < float(r) < 2.0, r
    if masked:
        out = ref_scores_max_pooling_wiht_mask(sc.score, sc.mask, sc.cams, 123.0, ratio, 49, 'ball query', True, depth_images=sc.depth)
    else:
        out = ref_scores_max_pooling(sc.score, sc.cams, 123.0, ratio, 49, 'ball query', True, depth_images=sc.depth)
    got, want = _stack(out, sc.cams), _want(sc, r, 49, masked)
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.gpu
def test_input_forms(gpu_device):
    """By position and by image_name; [H*W], [H,W] and [1,H,W]; a device scene_extend."""
    from materialrefgs_amd.refscore import ref_scores_max_pooling, ref_scores_max_pooling_wiht_mask
    sc = _scene(gpu_device)
    names = [c.image_name for c in sc.cams]
    base = _stack(ref_scores_max_pooling(sc.score, sc.cams, EXTENT, RATIOS[1], depth_images=sc.depth), sc.cams)
    by_name = ref_scores_max_pooling({n: s.reshape(-1) for n, s in zip(reversed(names), reversed(sc.score))}, sc.cams, EXTENT, RATIOS[1],
                                     depth_images={n: d[None] for n, d in zip(names, sc.depth)})
    assert np.array_equal(_bits(_stack(by_name, sc.cams)), _bits(base))
    on_device = ref_scores_max_pooling(sc.score, sc.cams, torch.tensor(EXTENT, device=gpu_device), RATIOS[1], depth_images=sc.depth)
    assert np.array_equal(_bits(_stack(on_device, sc.cams)), _bits(base))
    masked = _stack(ref_scores_max_pooling_wiht_mask(sc.score, sc.mask, sc.cams, EXTENT, RATIOS[1], depth_images=sc.depth), sc.cams)
    other = ref_scores_max_pooling_wiht_mask(tuple(sc.score), {n: m.to(torch.float32).reshape(1, H, W) for n, m in zip(names, sc.mask)}, sc.cams,
                                             EXTENT, RATIOS[1], depth_images=sc.depth)
    assert np.array_equal(_bits(_stack(other, sc.cams)), _bits(masked))
    assert not np.array_equal(_bits(masked), _bits(base))


@pytest.mark.gpu
def test_no_host_synchronisation_and_no_index_tensor(gpu_device):
    """torch.cuda.set_sync_debug_mode("error") around both functions, with and without calc_depth_points_radius (the cameras' R and T
    are host tensors); the peak of the allocator stays below the [points, n_samples] int32 tensor the reference materialises."""
    from materialrefgs_amd.refscore import ref_scores_max_pooling, ref_scores_max_pooling_wiht_mask
    sc = _scene(gpu_device)
    want = {calc: ref_scores_max_pooling(sc.score, sc.cams, EXTENT, 0.1, 49, 'ball query', calc, depth_images=sc.depth) for calc in (False, True)}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu_device)
    torch.cuda.reset_peak_memory_stats(gpu_device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = {calc: ref_scores_max_pooling(sc.score, sc.cams, EXTENT, 0.1, 49, 'ball query', calc, depth_images=sc.depth) for calc in (False, True)}
        for calc in (False, True):
            ref_scores_max_pooling_wiht_mask(sc.score, sc.mask, sc.cams, EXTENT, 0.1, 49, 'ball query', calc, depth_images=sc.depth)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    peak = torch.cuda.max_memory_allocated(gpu_device) - before
    for calc in (False, True):
        assert np.array_equal(_bits(_stack(got[calc], sc.cams)), _bits(_stack(want[calc], sc.cams)))
    print(f"peak allocation of the pooling calls: {peak} bytes; [points, 49] int32 would be {V * H * W * 49 * 4}")
    assert peak < V * H * W * 49 * 4
