"""materialrefgs_amd.ballquery (libmrgs.so: csrc/mrgs_ballquery.hip) behind the `pointnet2_ops.pointnet2_utils` shim: ball_query and
furthest_point_sample.  Both have exact definitions (tests/pool_statement.py), so every GPU case compares with torch.equal against the
float32 brute force: no tolerance, no excluded rows.

The random clouds are built so that a pruning walk meets every kind of row: for every random GPU case and each of its two radii the
statement must show at least 5 % of the queries without a hit, 5 % partly filled (0 < hits < nsample; with nsample = 1, where no row can
be partly filled, exactly one hit) and 5 % saturated (hits >= nsample; with nsample = 1 more than one hit).  That is a condition on the
inputs and is asserted on the CPU (test_random_cases_show_every_kind_of_row).  The lone point (N = M = 1) has one row and therefore one
kind per radius; it is listed for the walk's sake and left out of that condition only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pool_statement as ps

BAD_ARG, HIP, WORKSPACE = 1, 4, 5


# ---- the clouds -----------------------------------------------------------------------------------------------------------------------
def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def radial_cloud(N, M, seed, shell=(0.03, 1.0)):
    """Candidates at log-uniform distances 1e-3 .. 1 from the origin (density falls with the cube of the distance: every radius finds crowded
    and empty places); queries: 20 % within 1e-3 of the origin, 15 % at distance 50, the rest at log-uniform distances inside `shell`."""
    rng = np.random.default_rng(seed)
    xyz = _directions(rng, N) * 10.0 ** rng.uniform(-3.0, 0.0, size=(N, 1))
    kind = rng.random(M)
    rho = np.where(kind < 0.2, 1e-3 * rng.random(M), np.where(kind < 0.35, 50.0, 10.0 ** rng.uniform(*np.log10(shell), size=M)))
    return xyz.astype(np.float32), (_directions(rng, M) * rho[:, None]).astype(np.float32)


def image_cloud(H=64, W=80, seed=5):
    """An image-ordered cloud: pixel (x, y) lifted by a depth that runs from 0.5 to 20 across the columns (so the spacing of neighbours
    does too), 7 % of the pixels without a depth (NaN)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 0.5 * 40.0 ** (x / (W - 1.0)) * (1.0 + 0.01 * rng.standard_normal((H, W)))
    z[rng.random((H, W)) < 0.07] = np.nan
    f = 80.0
    return np.stack([(x - 0.5 * W) / f * z, (y - 0.5 * H) / f * z, z], axis=-1).reshape(-1, 3).astype(np.float32)


def _case(name):
    """name -> (xyz [B,N,3], new_xyz [B,M,3], nsample, (radius, radius))."""
    if name == "n1":
        return np.array([[[0.3, -0.2, 0.1]]], np.float32), np.array([[[0.35, -0.2, 0.1]]], np.float32), 7, (0.1, 0.01)
    if name in ("n63", "n64", "n65"):
        N = int(name[1:])
        xyz, q = radial_cloud(N, N, seed=N)
        return xyz[None], q[None], 7, (0.15, 0.05)
    if name == "n4097":
        xyz, q = radial_cloud(4097, 4097, seed=4097)
        return xyz[None], q[None], 49, (0.3, 0.05)
    if name.startswith("nsample"):
        xyz, q = radial_cloud(1500, 700, seed=15, shell=(0.1, 1.0))
        return xyz[None], q[None], int(name[7:]), (0.1, 0.05)
    if name == "big":
        xyz, q = radial_cloud(270_000, 300, seed=27, shell=(0.05, 1.0))
        return xyz[None], q[None], 49, (0.05, 0.01)
    if name == "batch2":
        a, b = radial_cloud(1000, 600, seed=1), radial_cloud(1000, 600, seed=2)
        return np.stack([a[0], b[0] * 0.5]), np.stack([a[1], b[1] * 0.5]), 7, (0.15, 0.05)
    if name in ("image", "image_permuted"):
        xyz = image_cloud()
        if name == "image_permuted":
            xyz = xyz[np.random.default_rng(9).permutation(len(xyz))]
        return xyz[None], xyz[None], 49, (0.5, 0.2)
    raise KeyError(name)


RANDOM_CASES = ("n63", "n64", "n65", "n4097", "nsample1", "nsample7", "nsample49", "nsample64", "nsample65", "big", "batch2", "image",
                "image_permuted")
ALL_CASES = ("n1",) + RANDOM_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    xyz, q, nsample, radii = _case(name)
    xyz.setflags(write=False)
    q.setflags(write=False)
    return xyz, q, nsample, radii


@functools.lru_cache(maxsize=None)
def case_statement(name, which):
    """(idx, hits) of the case at its radius number `which`: computed once, shared by the CPU condition and the GPU comparison."""
    xyz, q, nsample, radii = case(name)
    idx, hits = ps.ball_query(radii[which], nsample, xyz, q, return_hits=True)
    idx.setflags(write=False)
    return idx, hits


# hand cases: (xyz, queries, radius, nsample, expected rows)
HAND = {
    "duplicate_hits_at_distance_0": ([[1, 2, 3], [1, 2, 3]], [[1, 2, 3]], 0.1, 3, [[0, 1, 0]]),
    "exactly_r2_misses": ([[0.5, 0, 0], [0.25, 0, 0]], [[0, 0, 0]], 0.5, 2, [[1, 1]]),
    "radius_0_gives_zero_rows": ([[7, 7, 7], [1, 2, 3], [1, 2, 3]], [[1, 2, 3]], 0.0, 2, [[0, 0]]),
    "nan_row_never_hits_and_is_never_hit": ([[np.nan, 0, 0], [0, 0, 0]], [[0, 0, 0], [np.nan, 0, 0], [0, np.nan, 0]], 1.0, 2, [[1, 1], [0, 0], [0, 0]]),
    "inf_row_never_hits": ([[np.inf, 0, 0], [0, 0, 0]], [[np.inf, 0, 0], [0, 0, 0]], 1.0, 2, [[0, 0], [1, 1]]),
    "padding_repeats_h0": ([[9, 9, 9], [8, 8, 8], [0, 0, 0.1], [7, 7, 7], [0, 0.1, 0]], [[0, 0, 0]], 0.5, 4, [[2, 4, 2, 2]]),
    "no_hit_is_zeros": ([[5, 5, 5], [6, 6, 6]], [[0, 0, 0]], 1.0, 3, [[0, 0, 0]]),
    "query_not_among_its_own_first_hits": ([[1, 1, 1]] * 5, [[1, 1, 1]] * 5, 0.1, 2, [[0, 1]] * 5),
}


def _hand(name):
    xyz, q, r, ns, want = HAND[name]
    return np.array([xyz], np.float32), np.array([q], np.float32), r, ns, np.array([want], np.int32)


# ---- without a GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_statement_on_hand_cases(name):
    xyz, q, r, ns, want = _hand(name)
    assert np.array_equal(ps.ball_query(r, ns, xyz, q), want)


def test_statement_exact_rim_is_exact():
    """(0.5, 0, 0) against the origin at r = 0.5: d = 0.25 = r2 exactly, a miss; one float below the rim is a hit."""
    assert ps.dist2(np.zeros((1, 3)), np.array([[0.5, 0, 0]]))[0, 0] == ps.radius2(0.5) == np.float32(0.25)
    inside = np.nextafter(np.float32(0.5), np.float32(0))
    idx, hits = ps.ball_query(0.5, 1, np.array([[[0.5, 0, 0], [inside, 0, 0]]], np.float32), np.zeros((1, 1, 3), np.float32), return_hits=True)
    assert hits[0, 0] == 1 and idx[0, 0, 0] == 1


def test_fps_statement_on_hand_cases():
    tie = np.array([[[1, 0, 0], [3, 0, 0], [-1, 0, 0]]], np.float32)            # both others at squared distance 4: the lower index
    assert ps.furthest_point_sample(tie, 3).tolist() == [[0, 1, 2]]
    small = np.array([[[1, 0, 0], [0.03, 0, 0], [0, 0.02, 0.02], [1.5, 0, 0]]], np.float32)     # two points inside the magnitude ball
    assert ps.furthest_point_sample(small, 4).tolist() == [[0, 3, 0, 0]]
    assert ps.furthest_point_sample(np.zeros((1, 4, 3), np.float32) + 0.001, 3).tolist() == [[0, 0, 0]]         # no eligible point
    idx, span = ps.furthest_point_sample(np.array([[[0, 0, 0], [3, 4, 0], [1, 1, 1]]], np.float32), 2, return_span=True)
    assert idx.tolist() == [[0, 1]] and span[0] == np.float32(5.0)


@pytest.mark.parametrize("name", RANDOM_CASES)
def test_random_cases_show_every_kind_of_row(name):
    _xyz, _q, nsample, radii = case(name)
    for which, r in enumerate(radii):
        kinds = ps.row_kinds(case_statement(name, which)[1], nsample)
        print(f"{name}: r = {r}: no hit {kinds[0]:.3f}, partly {kinds[1]:.3f}, saturated {kinds[2]:.3f}")
        assert min(kinds) >= 0.05, (name, r, kinds)


def test_pointnet2_ops_shim_resolves_to_the_hip_implementation():
    """utils/ref_score_utils.py:1, the import line that cannot resolve on ROCm."""
    from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample
    import pointnet2_ops  # noqa: F401
    from materialrefgs_amd import ballquery
    assert ball_query is ballquery.ball_query and furthest_point_sample is ballquery.furthest_point_sample


def test_wrappers_reject_before_the_library_is_touched(monkeypatch):
    from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample
    from materialrefgs_amd import _lib

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    x = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        ball_query(0.1, 4, x, x)                                               # CPU tensors: there is no fallback
    with pytest.raises(RuntimeError, match="CUDA"):
        furthest_point_sample(x, 2)
    with pytest.raises(ValueError, match=r"\(B, N, 3\)"):
        ball_query(0.1, 4, torch.zeros(8, 3), x)
    with pytest.raises(TypeError, match="float32"):
        furthest_point_sample(x.double(), 2)
    with pytest.raises(TypeError, match="tensor"):
        ball_query(0.1, 4, x.numpy(), x)


def _c():
    from materialrefgs_amd import _lib
    return _lib, _lib.lib()


def test_workspace_size():
    _lib, L = _c()
    size = L.mrgs_ball_query_ws_bytes
    sizes = [int(size(1, N)) for N in (1, 64, 10 ** 5, 64 * 10 ** 6)]
    assert 0 < sizes[0] <= sizes[1] < sizes[2] < sizes[3], sizes
    assert 16 * 64 * 10 ** 6 <= sizes[-1] <= 17 * 64 * 10 ** 6 + (1 << 20)     # the packed rows and 33 bytes per 64 points
    assert int(size(3, 1000)) >= 3 * 16 * 1000
    for B, N in ((-1, 10), (65536, 10), (1, -1), (1, 1 << 31)):
        assert size(B, N) == 0


def test_entry_points_check_their_arguments_before_any_launch():
    """Contract violations are reported before any HIP call is made: the pointers below are never dereferenced."""
    _lib, L = _c()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    need = int(L.mrgs_ball_query_ws_bytes(1, 100))
    bq = lambda r=0.1, ns=4, xyz=p, q=p, B=1, N=100, M=50, idx=p, ws=p, n=need: L.mrgs_ball_query(r, ns, xyz, q, B, N, M, idx, ws, n, None)
    assert bq(B=0, xyz=None, q=None, idx=None, ws=None, n=0) == 0 and bq(M=0) == 0          # empty: nothing to launch
    for kw in (dict(ns=0), dict(ns=-3), dict(B=-1), dict(B=65536), dict(N=-1), dict(N=1 << 31), dict(M=-1), dict(M=1 << 31), dict(xyz=None),
               dict(q=None), dict(idx=None), dict(ws=None), dict(ws=odd)):
        assert bq(**kw) == BAD_ARG, kw
    assert bq(n=need - 1) == WORKSPACE and bq(n=0) == WORKSPACE
    pool = lambda r=0.1, rd=None, ns=49, pts=p, sc=p, valid=None, B=1, N=100, out=p, ws=p, n=need: L.mrgs_ball_max_pool(r, rd, ns, pts, sc, valid, B, N,
                                                                                                                   out, ws, n, None)
    assert pool(N=0, pts=None, sc=None, out=None, ws=None, n=0) == 0 and pool(B=0) == 0
    for kw in (dict(ns=0), dict(B=-1), dict(B=65536), dict(N=-1), dict(N=1 << 31), dict(pts=None), dict(sc=None), dict(out=None), dict(ws=None),
               dict(ws=odd)):
        assert pool(**kw) == BAD_ARG, kw
    assert pool(n=need - 1) == WORKSPACE
    fps = lambda xyz=p, B=1, N=100, np_=2, idx=p, span=None, ws=p, n=need: L.mrgs_furthest_point_sample(xyz, B, N, np_, idx, span, ws, n, None)
    assert fps(np_=0, xyz=None, idx=None, ws=None, n=0) == 0 and fps(B=0) == 0
    for kw in (dict(np_=-1), dict(B=-1), dict(N=-1), dict(N=0), dict(N=1 << 31), dict(xyz=None), dict(idx=None), dict(ws=None), dict(ws=odd)):
        assert fps(**kw) == BAD_ARG, kw
    assert fps(n=need - 1) == WORKSPACE
    dp = lambda views=p, V=3, H=24, W=32, pts=p: L.mrgs_depth_points(views, V, H, W, pts, None)
    assert dp(V=0, views=None, pts=None) == 0 and dp(H=0) == 0 and dp(W=0) == 0
    for kw in (dict(V=-1), dict(V=65536), dict(H=-1), dict(W=-1), dict(V=4, H=1 << 15, W=1 << 14), dict(views=None), dict(pts=None)):
        assert dp(**kw) == BAD_ARG, kw
    assert ctypes.sizeof(_lib.MrgsDepthView) == 8 + 16 * 4


@pytest.mark.skipif(torch.cuda.device_count() != 0, reason="host addresses as arguments: only for a machine without a device")
def test_without_a_device_a_well_formed_call_names_the_file():
    _lib, L = _c()
    buf = (ctypes.c_float * 65536)()
    p = (ctypes.addressof(buf) + 63) & ~63
    need = int(L.mrgs_ball_query_ws_bytes(1, 64))
    assert need <= 65536 * 4 - 64
    calls = (lambda: L.mrgs_ball_query(0.1, 4, p, p, 1, 64, 64, p, p, need, None),
             lambda: L.mrgs_ball_max_pool(0.1, None, 4, p, p, None, 1, 64, p, p, need, None),
             lambda: L.mrgs_furthest_point_sample(p, 1, 64, 2, p, None, p, need, None),
             lambda: L.mrgs_depth_points(p, 1, 4, 4, p, None))
    for call in calls:
        assert call() == _lib.MRGS_E_HIP
        text = L.mrgs_last_hip_error()
        assert text and b" at mrgs_ballquery.hip:" in text, text


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)              # (a copy: the cached clouds are read-only)


def _run(radius, nsample, xyz, q, dev):
    from pointnet2_ops.pointnet2_utils import ball_query
    out = ball_query(radius, nsample, _dev(xyz, dev), _dev(q, dev))
    assert out.shape == (xyz.shape[0], q.shape[1], nsample) and out.dtype == torch.int32 and out.device.type == "cuda"
    assert out.requires_grad is False
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", ALL_CASES)
def test_ball_query_equals_the_statement(gpu_device, name, which):
    """A lone point, a partial leaf, a full leaf, a leaf + 1, a top box + 1; every nsample; 270 000 candidates (more than 64 top boxes)
    against 300 queries; two batches with different clouds; the same cloud image-ordered and permuted: two radii each."""
    xyz, q, nsample, radii = case(name)
    got = _run(radii[which], nsample, xyz, q, gpu_device)
    want = torch.from_numpy(np.array(case_statement(name, which)[0])).to(gpu_device)
    assert torch.equal(got, want), int((got != want).any(dim=-1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_ball_query_hand_cases(gpu_device, name):
    xyz, q, r, ns, want = _hand(name)
    assert torch.equal(_run(r, ns, xyz, q, gpu_device), torch.from_numpy(want).to(gpu_device))


@pytest.mark.gpu
def test_ball_query_empty_inputs(gpu_device):
    from pointnet2_ops.pointnet2_utils import ball_query
    pts = torch.rand(1, 10, 3, device=gpu_device)
    none = torch.zeros(1, 0, 3, device=gpu_device)
    assert ball_query(0.5, 3, pts, none).shape == (1, 0, 3)
    assert torch.equal(ball_query(0.5, 3, none, pts), torch.zeros(1, 10, 3, dtype=torch.int32, device=gpu_device))     # no candidate: zero rows


def _fps_cloud(N, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(1, N, 3)) * 0.5).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("npoint", (1, 2, 5))
@pytest.mark.parametrize("N", (1, 65, 4097))
def test_furthest_point_sample_equals_the_statement(gpu_device, N, npoint):
    from pointnet2_ops.pointnet2_utils import furthest_point_sample
    xyz = _fps_cloud(N, seed=N)
    got = furthest_point_sample(_dev(xyz, gpu_device), npoint)
    assert got.shape == (1, npoint) and got.dtype == torch.int32
    assert torch.equal(got.cpu(), torch.from_numpy(ps.furthest_point_sample(xyz, npoint)))


@pytest.mark.gpu
def test_furthest_point_sample_magnitude_ball_tie_nothing_eligible_batches_and_span(gpu_device):
    from materialrefgs_amd.ballquery import furthest_point_sample
    rng = np.random.default_rng(3)
    inside = (rng.normal(size=(1, 600, 3)) * 0.01).astype(np.float32)                      # |p|^2 <= 1e-3 for nearly all of them
    outside = _fps_cloud(600, seed=4)
    mixed = np.concatenate([inside, outside], axis=1)[:, rng.permutation(1200)]
    tie = np.array([[[1, 0, 0], [3, 0, 0], [-1, 0, 0]]], np.float32)
    nothing = (rng.random((1, 300, 3)) * 0.01).astype(np.float32)
    for cloud, npoint in ((mixed, 6), (tie, 3), (nothing, 4), (np.concatenate([mixed, mixed[:, ::-1]]), 5)):
        want_idx, want_span = ps.furthest_point_sample(cloud, npoint, return_span=True)
        idx, span = furthest_point_sample(_dev(cloud, gpu_device), npoint, return_span=True)
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), (idx, want_idx)
        assert torch.equal(span.cpu().view(torch.int32), torch.from_numpy(want_span).view(torch.int32))
    mag = (mixed[0] ** 2).sum(axis=1)
    picks = ps.furthest_point_sample(mixed, 6)[0, 1:]
    assert (mag[picks] > 1e-3).all() and (mag <= 1e-3).sum() > 500                            # the ball's points exist and are never picked
    assert ps.furthest_point_sample(tie, 3).tolist() == [[0, 1, 2]] and not ps.furthest_point_sample(nothing, 4).any()


@pytest.mark.gpu
def test_two_runs_are_bitwise_identical_and_the_inputs_unchanged(gpu_device):
    from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample
    xyz, q, nsample, radii = case("n4097")
    x, y = _dev(xyz, gpu_device), _dev(q, gpu_device)
    keep_x, keep_y = x.clone(), y.clone()
    a, b = ball_query(radii[0], nsample, x, y), ball_query(radii[0], nsample, x, y)
    assert torch.equal(a, b) and torch.equal(x, keep_x) and torch.equal(y, keep_y)
    f, g = furthest_point_sample(x, 5), furthest_point_sample(x, 5)
    assert torch.equal(f, g) and torch.equal(x, keep_x)


@pytest.mark.gpu
def test_no_host_synchronisation(gpu_device):
    """torch.cuda.set_sync_debug_mode("error") around ball_query and the sampler (the pooling: tests/test_ref_score_pooling.py)."""
    from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample
    xyz, q, nsample, radii = case("nsample7")
    x, y = _dev(xyz, gpu_device), _dev(q, gpu_device)
    ball_query(radii[0], nsample, x, y)                       # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ball_query(radii[0], nsample, x, y)
        picks = furthest_point_sample(x, 3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got.cpu(), torch.from_numpy(np.array(case_statement("nsample7", 0)[0])))
    assert torch.equal(picks.cpu(), torch.from_numpy(ps.furthest_point_sample(xyz, 3)))
