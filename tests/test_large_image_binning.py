"""The rasterizer's binning on either side of the tile-count boundary (mrgs_bin_supported: 16 384 tiles = 2048 x 2048 px) and, above
it, on the radix path of mrgs_sort.hip at the sizes that select every instance of its radix passes and send the scan's look-back over
more than one window.  Everything goes through test_gpu_parity.compare_all against the C oracle: num_rendered, tiles_touched,
point_list, ranges and n_contrib bit for bit, the maps at its usual bars, no pixel allowance.

Every case asserts the class it was written for from P and the pair count it rendered, so that a change of the scene generator cannot
move it to another instance unnoticed (helpers.SORT_ITEMS restates sort_items() of mrgs_sort.hip)."""
import pytest

from helpers import BIN_MAX_TILES, scan_workgroups, sort_items
from materialrefgs_amd.synthetic import make_shell_scene, orbit_camera
from test_gpu_parity import compare_all

pytestmark = pytest.mark.gpu


def _tiles(H, W):
    return ((H + 15) // 16) * ((W + 15) // 16)


def _scene(P, H, W, rpx):
    return make_shell_scene(P, S=0, seed=5, radius_px=rpx, image_size=max(H, W))


def test_last_image_size_on_the_tile_path(gpu_device):
    """Exactly 16 384 tiles: the largest image the slice histograms hold, where tile_emit_kernel carves the most LDS it ever does
    (64 KB of cursors + 88 KB of per-wave staging)."""
    H = W = 2048
    assert _tiles(H, W) == BIN_MAX_TILES
    hr = compare_all(_scene(3000, H, W, 30.0), orbit_camera(2, H, W), gpu_device, check_grads=False)
    assert hr.num_rendered > 3000


# P, H, W, radius_px | instance of the pair sort (R keys), instance of the depth sort (P keys), workgroups of the scan (P elements)
RADIX_CASES = [
    (135_000, 2050, 2064, 4.0, 8, 8, 66),      # ragged image; the scan's last workgroups look back over a second window
    (60_000, 2064, 2064, 12.0, 8, 4, 30),      # 16 641 tiles: 15 tile-key bits, the second pass has 7 live bits
    (150_000, 2064, 2064, 12.0, 16, 8, 74),
    (800_000, 2064, 2064, 1.5, 16, 16, 391),   # seven look-back windows in the scan
]


def _assert_radix_class(hr, P, H, W, pair_items, depth_items, scan_wgs):
    assert _tiles(H, W) > BIN_MAX_TILES                                   # the radix path, not the tile path
    assert sort_items(P) == depth_items, (P, sort_items(P))
    assert scan_workgroups(P) == scan_wgs, scan_workgroups(P)
    assert sort_items(hr.num_rendered) == pair_items, (hr.num_rendered, sort_items(hr.num_rendered))


@pytest.mark.parametrize("P,H,W,rpx,pair_items,depth_items,scan_wgs", RADIX_CASES)
def test_radix_path_instances_against_the_oracle(gpu_device, P, H, W, rpx, pair_items, depth_items, scan_wgs):
    hr = compare_all(_scene(P, H, W, rpx), orbit_camera(2, H, W), gpu_device, check_grads=False)
    _assert_radix_class(hr, P, H, W, pair_items, depth_items, scan_wgs)


def test_radix_path_with_a_third_of_the_surfels_culled(gpu_device):
    """Zero tiles_touched entries through the scan and duplicate_kernel: every third surfel far outside the frustum."""
    P, H, W = 150_000, 2064, 2064
    scene = _scene(P, H, W, 12.0)
    means = scene.means3D.clone()
    means[::3] *= 40.0
    hr = compare_all(scene._replace(means3D=means), orbit_camera(2, H, W), gpu_device, check_grads=False)
    _assert_radix_class(hr, P, H, W, 8, 8, 74)
    culled = int((hr.export("tiles_touched") == 0).sum())
    assert culled > P // 4, culled       # (a few of the displaced ones stay in the frustum)
