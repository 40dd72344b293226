"""materialrefgs_amd.knn.distCUDA2 (libmrgs.so: csrc/mrgs_knn.hip) behind the `simple_knn._C` shim: the mean squared distance to the three
nearest other points.  The value has an exact definition (tests/knn_statement.py), so the GPU cases compare BIT FOR BIT with its float32
brute force; the two sizes a brute force cannot serve compare with scipy's k-d tree in float64 within 1e-6 relative per element.

Where 1e-6 comes from: each fp32 difference is within 2^-24 relative, each squared distance within about 5 * 2^-24 after its three products
and two sums, the mean of three positives adds three roundings: <= 8 * 2^-24 = 4.8e-7; a neighbour swapped by an fp32 near-tie has a true
distance inside the same band.  1e-6 is that bound with a factor two."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from knn_statement import FLT_MAX, statement32, truth64

BAD_ARG, WORKSPACE = 1, 5


def cube(P, seed=0):
    return np.random.default_rng(seed).random((P, 3)).astype(np.float32)


def shell(P, seed=0):
    from materialrefgs_amd.synthetic import shell_centres
    return shell_centres(P, seed=seed)


def _clouds(P):
    """The clouds that break a pruning search, each of about P points (seeded)."""
    rng = np.random.default_rng(7)
    half = P // 2
    g = np.arange(20, dtype=np.float32)
    base = rng.random((half, 3))
    return {
        "cube": rng.random((P, 3)),
        "shell": shell(P, seed=2),
        "constant_z": np.c_[rng.random((P, 2)), np.full(P, 0.25)],                     # one zero extent
        "line_x": np.c_[rng.random(P), np.full(P, -1.5), np.full(P, 3.0)],            # two zero extents
        "identical": np.tile(np.array([[0.3, -0.7, 2.0]]), (min(P, 3000), 1)),        # three zero extents, every distance 0
        "twice": np.r_[base, base][rng.permutation(2 * half)],                        # every point present twice
        "lattice": np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3),   # ties everywhere
        # the whole small cluster shares one Morton cell; its neighbours must not be rejected by the far cluster's boxes
        "two_clusters": np.r_[rng.normal(0.0, 1e-4, (half, 3)), 100.0 + rng.normal(0.0, 1.0, (half, 3))],
        "shifted": 1000.0 + rng.random((P, 3)),                                       # differences of large coordinates
    }


CLOUD_NAMES = ("cube", "shell", "constant_z", "line_x", "identical", "twice", "lattice", "two_clusters", "shifted")
GPU_CLOUD_P = 6000        # two clusters of 3 000 (the lattice is 20^3 at any P): all but the 3 000 identical points span more than one box of 64 leaves (4 096 points)


@functools.lru_cache(maxsize=None)
def cloud(name, P):
    a = np.ascontiguousarray(_clouds(P)[name], dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cloud_statement(name, P):
    a = statement32(cloud(name, P))
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------

def test_simple_knn_shim_resolves_to_the_hip_implementation():
    """The reference's first import line that failed: scene/gaussian_model.py:11, env_gaussian_model.py:20."""
    from simple_knn._C import distCUDA2
    from materialrefgs_amd import knn
    assert distCUDA2 is knn.distCUDA2 and knn.mean_dist2 is knn.distCUDA2


def test_workspace_size_grows_with_P_and_stays_under_the_cap():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    sizes = [int(L.mrgs_knn_ws_bytes(P)) for P in (0, 1, 64, 10 ** 6, 2 * 10 ** 7)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for P, s in zip((0, 1, 64, 10 ** 6, 2 * 10 ** 7), sizes):
        assert 0 < s <= 64 * P + (1 << 20), (P, s)
    assert sizes[3] >= 36 * 10 ** 6           # two key / value pairs, the float4 rows, the sort's status words


def test_status_codes_without_gpu():
    """Contract violations are reported before any HIP call is made."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)               # never dereferenced: every call below is refused or has nothing to do
    call = L.mrgs_knn_mean_dist2
    need = int(L.mrgs_knn_ws_bytes(100))
    assert call(None, 0, None, None, 0, None) == 0                          # P = 0: nothing to launch
    assert call(p, -1, p, p, need, None) == BAD_ARG
    assert call(p, 1 << 31, p, p, 1 << 40, None) == BAD_ARG
    assert call(None, 100, p, p, need, None) == BAD_ARG
    assert call(p, 100, None, p, need, None) == BAD_ARG
    assert call(p, 100, p, None, need, None) == BAD_ARG
    assert call(p, 100, p, ctypes.c_void_p(0x1004), need, None) == BAD_ARG   # the workspace holds float4 rows
    assert call(p, 100, p, p, need - 1, None) == WORKSPACE
    assert call(p, 100, p, p, 0, None) == WORKSPACE


def test_wrapper_rejects_before_the_library_is_touched(monkeypatch):
    from materialrefgs_amd import _lib, knn

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    with pytest.raises(RuntimeError, match="CUDA"):
        knn.distCUDA2(torch.zeros(8, 3))                                    # a CPU tensor: there is no fallback
    with pytest.raises(ValueError, match="num_points, 3"):
        knn.distCUDA2(torch.zeros(8, 4))
    with pytest.raises(TypeError, match="float32"):
        knn.distCUDA2(torch.zeros(8, 3, dtype=torch.float64))


@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_statement32_is_within_1e6_of_float64(name):
    pts = cloud(name, 5000)
    a, b = statement32(pts).astype(np.float64), truth64(pts)
    worst = float(np.max(np.abs(a - b) / np.where(b > 0, b, 1.0)))
    print(f"{name}: P = {len(pts)}, worst relative difference {worst:.3e}")
    assert np.all(np.abs(a - b) <= 1e-6 * b)


def test_statement32_with_too_few_neighbours():
    for P in (1, 2):
        assert np.all(np.isposinf(statement32(cube(P))))
    three = statement32(cube(3))
    assert np.all(np.isfinite(three)) and np.all(three > 1.1e38)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

def run(pts, dev):
    from simple_knn._C import distCUDA2
    x = torch.from_numpy(np.array(pts, dtype=np.float32)).to(dev)              # (a copy: the cached clouds are read-only)
    out = distCUDA2(x)
    assert out.shape == (len(pts),) and out.dtype == torch.float32 and out.device == x.device
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097])
def test_edges_of_every_grouping_bit_for_bit(gpu_device, P):
    """Too few neighbours, the wave / leaf boundary, the boundary of the second level."""
    pts = cube(P, seed=P)
    got, want = run(pts, gpu_device), statement32(pts)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


@pytest.mark.gpu
def test_empty_cloud_returns_an_empty_tensor(gpu_device):
    assert run(np.zeros((0, 3), dtype=np.float32), gpu_device).shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUD_NAMES)
def test_clouds_that_break_a_pruning_search_bit_for_bit(gpu_device, name):
    pts = cloud(name, GPU_CLOUD_P)
    got, want = run(pts, gpu_device), cloud_statement(name, GPU_CLOUD_P)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


@functools.lru_cache(maxsize=None)
def shell_300k():
    a = shell(300_000, seed=0)
    a.setflags(write=False)
    return a


@pytest.mark.gpu
def test_shell_300k_against_float64_permuted_and_repeated(gpu_device):
    from simple_knn._C import distCUDA2
    pts = shell_300k()
    x = torch.from_numpy(pts.copy()).to(gpu_device)
    keep = x.clone()
    a = distCUDA2(x)
    b = distCUDA2(x)
    assert torch.equal(x, keep)                                             # the input is unchanged
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))            # two calls: bit-equal
    perm = torch.from_numpy(np.random.default_rng(1).permutation(len(pts))).to(gpu_device)
    c = distCUDA2(x[perm])
    assert torch.equal(c.view(torch.int32), a[perm].view(torch.int32))      # rows permuted: the same values, permuted
    got, want = a.cpu().numpy().astype(np.float64), truth64(pts)
    print(f"shell 300k: worst relative difference {float(np.max(np.abs(got - want) / want)):.3e}")
    assert np.all(np.abs(got - want) <= 1e-6 * want)
    # the reference's use of it (scene/gaussian_model.py:367-368)
    scales = torch.log(torch.sqrt(torch.clamp_min(a, 1e-7)))
    assert bool(torch.isfinite(scales).all())


@pytest.mark.gpu
def test_cube_1000003_against_float64(gpu_device):
    pts = cube(1_000_003, seed=11)
    got, want = run(pts, gpu_device).astype(np.float64), truth64(pts)
    print(f"cube 1000003: worst relative difference {float(np.max(np.abs(got - want) / want)):.3e}")
    assert np.all(np.abs(got - want) <= 1e-6 * want)


@pytest.mark.gpu
def test_surface_views_grad_and_streams(gpu_device):
    from simple_knn._C import distCUDA2
    pts = cloud("cube", GPU_CLOUD_P)
    want = bits(cloud_statement("cube", GPU_CLOUD_P))
    big = torch.zeros(len(pts), 4, device=gpu_device)
    big[:, :3] = torch.from_numpy(pts.copy()).to(gpu_device)
    view = big[:, :3]
    assert not view.is_contiguous()
    assert np.array_equal(bits(distCUDA2(view).cpu().numpy()), want)        # a non-contiguous view gives the contiguous result
    x = view.contiguous().requires_grad_(True)
    out = distCUDA2(x)
    assert out.requires_grad is False and out.grad_fn is None
    assert out.shape == (len(pts),) and out.dtype == torch.float32 and out.device == x.device
    assert np.array_equal(bits(out.cpu().numpy()), want)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        r = distCUDA2(x.detach())
        doubled = r * 2.0                                                   # later work on the same stream sees the finished result
    side.synchronize()
    assert np.array_equal(bits(r.cpu().numpy()), want)
    assert torch.equal(doubled, out * 2.0)
