"""The one-sweep radix sort and the one-kernel scan of mrgs_sort.hip on their own, bit for bit against numpy.

Through the debug entries mrgs_debug_radix_sort_pairs / mrgs_debug_scan_tiles (include/mrgs.h), thin wrappers over the functions the
rasterizer's radix path, the surfel BVH build and the k-NN call.  References:
  * sort: with m = (keys >> bit_lo) & ((1 << (bit_hi - bit_lo)) - 1) the permutation is np.argsort(m, kind="stable"); the values are
    arange(n), so `vals` IS the permutation the kernels applied and an unstable pass shows; the keys travel whole (keys_out == keys_in[vals]);
  * scan: np.cumsum in uint64 over tiles_touched[order], shifted to exclusive.
Counts sit on the edges of a wave run (64), a workgroup tile (1024 keys at 4 per thread; 2048 scan elements), the look-back windows
(8 tiles in the sort, 64 in the scan) and the thresholds between the three radix instances (helpers.SORT_ITEMS).
Nothing here tries to make a look-back wait."""

import numpy as np
import pytest
import torch

from helpers import SORT_ITEMS, scan_workgroups, sort_items

OK, BAD_ARG, WORKSPACE = 0, 1, 5

# ---- counts -------------------------------------------------------------------------------------------------------------------------
SMALL_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
# one below, on and one above each threshold of sort_items() (mrgs_sort.hip; the table is helpers.SORT_ITEMS), and 2^20 + 7
LARGE_COUNTS = [upto + d for upto, _items in SORT_ITEMS if upto is not None for d in (-1, 0, 1)] + [1_048_583]
assert LARGE_COUNTS == [131_071, 131_072, 131_073, 786_431, 786_432, 786_433, 1_048_583]
assert [sort_items(n) for n in LARGE_COUNTS] == [4, 4, 8, 8, 8, 16, 16]

BIT_RANGES = [(0, 32),   # rasterizer depth sort
              (0, 30),   # k-NN
              (0, 24),   # BVH
              (0, 16),   # two full passes
              (0, 15),   # last pass has 7 live bits (the tile ids of 16 641 tiles)
              (0, 9),    # last pass has 1 live bit
              (0, 8),    # one pass
              (0, 1)]    # one bit
LARGE_BIT_RANGES = [(0, 32), (0, 15), (0, 30)]

PATTERN_COUNTS = [5000, 200_000, 1_048_583]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _dev_u32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(dev)


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _workspace(nbytes, dev):
    """Filled with a pattern: the wrappers, not the caller, clear what the primitives need zero."""
    return torch.full((max(int(nbytes), 8),), 0xA5, dtype=torch.uint8, device=dev)


def run_sort(dev, keys, bit_lo, bit_hi, count=None):
    """(status, keys_out, vals_out); `count`: a device-resident element count, len(keys) is then the capacity."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    n = len(keys)
    k, v = _dev_u32(keys, dev), _dev_u32(np.arange(n), dev)
    ws = _workspace(L.mrgs_debug_sort_ws_bytes(n), dev)
    c = None if count is None else _dev_u32([count], dev)
    rc = L.mrgs_debug_radix_sort_pairs(k.data_ptr(), v.data_ptr(), n, None if c is None else c.data_ptr(), bit_lo, bit_hi, ws.data_ptr(),
                                       ws.numel(), _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, _host_u32(k), _host_u32(v)


def expected_permutation(keys, bit_lo, bit_hi):
    m = (keys.astype(np.uint64) >> np.uint64(bit_lo)) & np.uint64((1 << (bit_hi - bit_lo)) - 1)
    return np.argsort(m, kind="stable").astype(np.uint32)


def check_sort(dev, keys, bit_lo, bit_hi, what=""):
    keys = np.ascontiguousarray(keys, np.uint32)
    rc, k_out, v_out = run_sort(dev, keys, bit_lo, bit_hi)
    assert rc == OK, (what, rc)
    perm = expected_permutation(keys, bit_lo, bit_hi)
    bad = np.flatnonzero(v_out != perm)
    assert bad.size == 0, (what, f"n = {len(keys)}, bits [{bit_lo}, {bit_hi}): {bad.size} values off the stable permutation, first at {bad[:4]}")
    assert np.array_equal(k_out, keys[v_out]), (what, "keys did not travel with their values")


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


# ---- the sort: counts x bit ranges --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_COUNTS)
def test_sort_small_counts_over_every_bit_range(gpu_device, n):
    """Uniform 32-bit keys: bits outside the range are set at random and must neither order nor change."""
    keys = _uniform(n, n)
    for lo, hi in BIT_RANGES:
        check_sort(gpu_device, keys, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", LARGE_BIT_RANGES)
@pytest.mark.parametrize("n", LARGE_COUNTS)
def test_sort_counts_around_the_instance_thresholds(gpu_device, n, lo, hi):
    check_sort(gpu_device, _uniform(n, n + hi), lo, hi, what=f"radix_onesweep_kernel<{sort_items(n)}>")


# ---- the sort: key patterns ---------------------------------------------------------------------------------------------------------
BASE = np.uint32(0x40A1B2C3)          # no byte zero, none 0xFF


def _pattern(name, n):
    rng = np.random.default_rng(n + len(name))
    if name == "uniform":
        return _uniform(n, 1)
    if name == "all_equal":                       # every pass takes the copy shortcut
        return np.full(n, BASE, np.uint32)
    if name.startswith("one_byte_"):              # three passes shortcut, the pass of byte b does not
        b = int(name[-1])
        byte = rng.integers(0, 256, n, dtype=np.uint32)
        return (BASE & ~np.uint32(0xFF << (8 * b))) | (byte << np.uint32(8 * b))
    if name == "all_equal_but_one":               # digit totals n - 1 and 1 in every pass: no shortcut, and the odd key crosses the array
        k = np.full(n, BASE, np.uint32)
        k[(2 * n) // 3] = np.uint32(0x1F5E4D3C)   # differs in all four bytes, sorts first
        return k
    if name == "two_keys_runs":                   # runs of 1 500: equal keys cross every workgroup tile, no run is tile aligned
        return np.where((np.arange(n) // 1500) % 2 == 0, np.uint32(0xC0FFEE11), np.uint32(0x0BADF00D)).astype(np.uint32)
    if name == "two_keys_halves":                 # the larger key first: both halves move as blocks
        return np.where(np.arange(n) < n // 2, np.uint32(0xC0FFEE11), np.uint32(0x0BADF00D)).astype(np.uint32)
    if name == "sorted":
        return np.sort(_uniform(n, 2))
    if name == "reversed":
        return np.sort(_uniform(n, 3))[::-1].copy()
    if name == "three_values":
        return rng.choice(np.array([0x00000001, 0x80000000, 0x7F00FF00], np.uint32), n)
    if name == "float_depths":                    # the rasterizer's keys: positive float bits from a narrow range, the high byte constant
        k = rng.uniform(2.0, 3.9, n).astype(np.float32).view(np.uint32)
        assert np.unique(k >> 24).size == 1
        return k
    if name == "with_all_ones":                   # the value the kernel pads its invalid lanes with, as a real key: first, last, scattered
        k = _uniform(n, 4)
        k[rng.integers(0, n, max(n // 50, 1))] = 0xFFFFFFFF
        k[0] = k[n - 1] = 0xFFFFFFFF
        return k
    raise KeyError(name)


PATTERNS = ["uniform", "all_equal", "one_byte_0", "one_byte_1", "one_byte_2", "one_byte_3", "all_equal_but_one", "two_keys_runs",
            "two_keys_halves", "sorted", "reversed", "three_values", "float_depths", "with_all_ones"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", PATTERN_COUNTS)
def test_sort_key_patterns(gpu_device, n, name):
    check_sort(gpu_device, _pattern(name, n), 0, 32, what=name)


# ---- the sort: element count on the device ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(0, 32), (0, 24)])      # an even and an odd number of passes: result in place / copied back
@pytest.mark.parametrize("n", [4097, 200_000])
def test_sort_with_a_device_resident_count(gpu_device, n, lo, hi):
    """n is a capacity, the count c is read on the device (mrgs_count): the first c outputs are the stable sort of the first c inputs.
    c > n means "nothing to do": only the status is specified."""
    keys = _uniform(n, 7 * n)
    for c in (0, 1, n // 2, n - 1, n):
        rc, k_out, v_out = run_sort(gpu_device, keys, lo, hi, count=c)
        assert rc == OK, (c, rc)
        perm = expected_permutation(keys[:c], lo, hi)
        assert np.array_equal(v_out[:c], perm), (c, int((v_out[:c] != perm).sum()))
        assert np.array_equal(k_out[:c], keys[:c][perm]), c
    for c in (n + 1, 2 * n, 0xFFFFFFFF):
        assert run_sort(gpu_device, keys, lo, hi, count=c)[0] == OK, c


# ---- the scan -----------------------------------------------------------------------------------------------------------------------
# 131 073: 65 workgroups, the last looks back over a second window of 64; 264 197: 130 workgroups, a third
SCAN_COUNTS = [1, 2047, 2048, 2049, 131_071, 131_072, 131_073, 133_121, 264_197, 300_000, 1_000_003]
assert [scan_workgroups(n) for n in (131_072, 131_073, 264_197)] == [64, 65, 130]
SCAN_VALUES = ["zero", "one", "random_identity", "random", "all_in_first", "all_in_last", "under_2_30", "over_2_32", "over_2_33"]


# totals just above 2^32 and above 2^33 (the look-back words carry 62 bits), in equal terms
OVER = {"over_2_32": (1 << 32) + 1000, "over_2_33": (1 << 33) + (1 << 31)}


def _reachable(name, n):
    """Any 2 048 consecutive terms must sum below 2^32 (the contract of the scan: a workgroup's own sum is 32-bit), so the totals above
    2^32 need more than one workgroup: from n = 2 049 and n = 5 121 on."""
    return name not in OVER or 2048 * (OVER[name] // n + 1) < 1 << 32


def _scan_values(name, n, order):
    """tiles_touched such that tiles_touched[order] is the named sequence."""
    rng = np.random.default_rng(n)
    if name == "zero":
        seq = np.zeros(n, np.uint32)
    elif name == "one":
        seq = np.ones(n, np.uint32)
    elif name in ("random", "random_identity"):     # a third zero: culled surfels
        seq = rng.integers(1, 401, n).astype(np.uint32)
        seq[rng.random(n) < 1 / 3] = 0
    elif name in ("all_in_first", "all_in_last"):
        seq = np.zeros(n, np.uint32)
        seq[0 if name == "all_in_first" else n - 1] = 123_456_789
    elif name == "under_2_30":                      # total 2^30 - 1: the largest pair count the rasterizer accepts
        seq = np.full(n, ((1 << 30) - 1) // n, np.uint32)
        seq[rng.integers(0, n)] += ((1 << 30) - 1) % n
        assert int(seq.sum(dtype=np.uint64)) == (1 << 30) - 1
    else:
        seq = np.full(n, OVER[name] // n + 1, np.uint32)
    v = np.empty(n, np.uint32)
    v[order] = seq
    return v


SCAN_CASES = [(n, name) for n in SCAN_COUNTS for name in SCAN_VALUES if _reachable(name, n)]
assert (2049, "over_2_32") in SCAN_CASES and (2048, "over_2_32") not in SCAN_CASES and (131_071, "over_2_33") in SCAN_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("n,name", SCAN_CASES)
def test_scan_against_cumsum(gpu_device, n, name):
    from materialrefgs_amd import _lib
    L = _lib.lib()
    dev = gpu_device
    order = np.arange(n) if name == "random_identity" else np.random.default_rng(n + 1).permutation(n)
    v = _scan_values(name, n, order)
    inc = np.cumsum(v[order], dtype=np.uint64)
    excl, total = inc - v[order], int(inc[-1])
    tt, od = _dev_u32(v, dev), _dev_u32(order, dev)
    offsets = torch.full((n,), -1, dtype=torch.int32, device=dev)
    tot = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ws = _workspace(L.mrgs_debug_scan_ws_bytes(n), dev)
    rc = L.mrgs_debug_scan_tiles(tt.data_ptr(), od.data_ptr(), n, offsets.data_ptr(), tot.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == OK, rc
    got_total = int(_host_u32(tot)[0])
    if total > 0xFFFFFFFF:
        assert got_total == 0xFFFFFFFF, hex(got_total)       # saturated; the offsets are not specified
        return
    assert got_total == total, (got_total, total)
    got = _host_u32(offsets)
    bad = np.flatnonzero(got != excl.astype(np.uint32))
    assert bad.size == 0, (f"{bad.size} offsets wrong, first at {bad[:4]} (workgroup {bad[0] // 2048} of {scan_workgroups(n)})")


# ---- without a GPU: arguments and workspace sizes -----------------------------------------------------------------------------------
def test_debug_sort_and_scan_reject_bad_arguments_before_any_launch():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    p = 0x10000                         # never dereferenced: every call below returns before its first HIP call
    big = 1 << 40
    sort = L.mrgs_debug_radix_sort_pairs
    assert sort(None, p, 10, None, 0, 32, p, big, None) == BAD_ARG
    assert sort(p, None, 10, None, 0, 32, p, big, None) == BAD_ARG
    assert sort(p, p, 10, None, 0, 32, None, big, None) == BAD_ARG
    assert sort(p, p, -1, None, 0, 32, p, big, None) == BAD_ARG
    assert sort(p, p, 10, None, 0, 33, p, big, None) == BAD_ARG
    assert sort(p, p, 10, None, 8, 8, p, big, None) == BAD_ARG
    assert sort(p, p, 10, None, 9, 8, p, big, None) == BAD_ARG
    assert sort(p, p, 10, None, -1, 8, p, big, None) == BAD_ARG
    assert sort(p, p, 0, None, 8, 8, p, big, None) == OK             # nothing to sort: the bit range is not looked at
    for n in (1, 1024, 1025, 200_000):
        need = L.mrgs_debug_sort_ws_bytes(n)
        assert need >= 8 * n                                         # the alternate keys and values at least
        assert sort(p, p, n, None, 0, 32, p, need - 1, None) == WORKSPACE
        assert sort(p, p, n, p, 0, 32, p, 0, None) == WORKSPACE
    scan = L.mrgs_debug_scan_tiles
    for k in range(6):
        args = [p, p, 10, p, p, p, big, None]
        if k < 5:
            args[(0, 1, 3, 4, 5)[k]] = None                          # each pointer in turn
        else:
            args[2] = -1
        assert scan(*args) == BAD_ARG, k
    for n in (1, 2048, 2049, 300_000):
        need = L.mrgs_debug_scan_ws_bytes(n)
        assert need >= 8 * scan_workgroups(n)                        # a 64-bit status word per workgroup at least
        assert scan(p, p, n, p, p, p, need - 1, None) == WORKSPACE


def test_debug_workspace_sizes_do_not_decrease_with_n():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    ns = sorted(set([0, 1, 2, 63, 64, 65] + [c + d for c in (1024, 2048, 4096, 131_072, 786_432, 1 << 20, 1 << 24) for d in (-1, 0, 1)]
                    + list(range(0, 20_000, 997))))
    for query in (L.mrgs_debug_sort_ws_bytes, L.mrgs_debug_scan_ws_bytes):
        sizes = [query(n) for n in ns]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), query.__name__
