"""The cubemapencoder fetch against the geometry of a cube, with no restatement in between: each check is written once as a function
of an `encode(dirs, cubemap, fail, interp, seamless, go=None)` callable and runs on the numpy restatement (CPU) and on the HIP kernels
(GPU).  What they pin is what the kernel's 6 x 4 kEdge table and the restatement's edge_table transcribe by hand: which texel lies
across each of the twelve edges and at each of the eight vertices, the fourth weight a vertex sample folds into the other three, and
the sign flips of the direction gradient.  `eps` is the unit roundoff of the implementation under test (2^-24 / 2^-53)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import cubemap_encoder_oracle as co
from helpers import rel_err
from test_cubemap_encoder import _dirs

MODES = ((0, 0), (1, 0), (1, 1))          # (interp, seamless): nearest, bilinear, seamless bilinear
DELTA = 2.0 ** -18                        # probe offset from an edge: 1 - DELTA is exact in fp32
# texel seed of the seam maps: chosen on the CPU with the restatement so that the plain (seamless = 0) fetch jumps by more than 0.5
# somewhere along EVERY one of the twelve edges at every L >= 2 run here (smallest per-edge jump: 1.40 at L = 2, 2.49 .. 2.68 above)
SEAM_TEXEL_SEED = 0
SEAM_LEVELS = (1, 2, 4, 8, 33)


def oracle_encode(dirs, cm, fail, interp, seamless, go=None):
    return co.encode(dirs, cm, fail, interp, seamless, go)


def hip_encode(device):
    from materialrefgs_amd.cubemap_encoder import cubemap_encode

    def encode(dirs, cm, fail, interp, seamless, go=None):
        t = lambda a: torch.tensor(np.asarray(a, np.float32), device=device, requires_grad=go is not None)
        td, tc, tf = t(dirs), t(cm), t(fail)
        out = cubemap_encode(td, tc, tf, interp, seamless)
        if go is None:
            return out.detach().cpu().numpy()
        out.backward(torch.tensor(np.asarray(go, np.float32), device=device))
        return tuple(a.detach().cpu().numpy() for a in (out, td.grad, tc.grad, tf.grad))
    return encode


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_texel_centres(encode, eps):
    """A direction through a texel's centre fetches that texel, on all six faces and in every mode: exactly in nearest mode, within
    16 L eps M in the bilinear ones (the centre's rounding moves kx, ky by at most ~4 L eps, the patch slope is at most 2 M per unit
    weight; the bound doubles the product)."""
    C = 2
    for L in (1, 2, 3, 4, 7):
        rng = np.random.default_rng(100 + L)
        cm = rng.normal(size=(6, C, L, L)).astype(np.float32)
        M = float(np.abs(cm).max())
        want = cm.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64)
        d = co.texel_centre_dirs(L)
        for interp, seamless in MODES:
            got = np.asarray(encode(d, cm, np.zeros(C), interp, seamless), np.float64)
            err = float(np.abs(got - want).max())
            print(f"texel centres L={L} mode=({interp},{seamless}): max err {err:.3e}, bound {16 * L * eps * M:.3e}")
            if interp == 0:
                assert np.array_equal(got, want), (L, err)
            else:
                assert err <= 16 * L * eps * M, (L, interp, seamless, err)


def edge_probe_pairs():
    """The twelve edges: ((a, b, sa, sb), d1 [41,3], d2 [41,3]) -- d1 just inside the face sa*e_a, d2 just inside the face sb*e_b, at
    the same 41 positions along the edge."""
    t = np.linspace(-0.97, 0.97, 41).astype(np.float32).astype(np.float64)
    for (a, b), sa, sb in itertools.product(((0, 1), (0, 2), (1, 2)), (1.0, -1.0), (1.0, -1.0)):
        c = 3 - a - b
        d1, d2 = np.zeros((41, 3)), np.zeros((41, 3))
        d1[:, a], d1[:, b], d1[:, c] = sa, sb * (1 - DELTA), t
        d2[:, a], d2[:, b], d2[:, c] = sa * (1 - DELTA), sb, t
        yield (a, b, sa, sb), d1, d2


def vertex_probe_triples():
    """The eight vertices: (s, d [3,3]) -- s * (1 - DELTA) with component k put back to s_k: one probe just inside each of the three
    faces that meet at the vertex s."""
    for s in itertools.product((1.0, -1.0), repeat=3):
        s = np.array(s)
        d = np.tile(s * (1 - DELTA), (3, 1))
        d[np.arange(3), np.arange(3)] = s
        yield s, d


def seam_map(L, C=4):
    return np.random.default_rng(SEAM_TEXEL_SEED).normal(size=(6, C, L, L)).astype(np.float32)


def plain_edge_jumps(encode, L):
    """Largest difference of the plain bilinear fetch between the two sides of each edge, over the 41 positions: [12]."""
    cm = seam_map(L)
    fail = np.zeros(cm.shape[1])
    return np.array([np.abs(np.asarray(encode(d1, cm, fail, 1, 0), np.float64) - np.asarray(encode(d2, cm, fail, 1, 0), np.float64)).max()
                     for _, d1, d2 in edge_probe_pairs()])


def check_seam_continuity(encode):
    """The seamless fetch is continuous across all twelve edges and at all eight vertices: two probes DELTA inside the two (three)
    faces agree within 8 L DELTA M (each probe lies within 2 DELTA of the common point in u and in v; the fetch moves at most L M per
    unit uv per axis).  Control: the plain fetch jumps by more than 0.5 on every edge, i.e. the probes do straddle and a wrong table
    entry would show."""
    for L in SEAM_LEVELS:
        cm = seam_map(L)
        fail = np.zeros(cm.shape[1])
        M = float(np.abs(cm).max())
        bound = 8 * L * DELTA * M
        worst = 0.0
        for key, d1, d2 in edge_probe_pairs():
            a, b = (np.asarray(encode(d, cm, fail, 1, 1), np.float64) for d in (d1, d2))
            diff = float(np.abs(a - b).max())
            worst = max(worst, diff)
            assert diff <= bound, ("edge", L, key, diff, bound)
        for s, d in vertex_probe_triples():
            o = np.asarray(encode(d, cm, fail, 1, 1), np.float64)
            diff = float(max(np.abs(o[:, i] - o[:, j]).max() for i, j in ((0, 1), (0, 2), (1, 2))))
            worst = max(worst, diff)
            assert diff <= bound, ("vertex", L, tuple(s), diff, bound)
        line = f"seams L={L}: worst seamless difference {worst:.3e}, bound {bound:.3e}"
        if L >= 2:
            jumps = plain_edge_jumps(encode, L)
            line += f"; smallest plain jump over the 12 edges {jumps.min():.3f}"
            assert (jumps > 0.5).all(), (L, jumps)
        print(line)


def probe_dirs(L):
    """512 directions: the 21 specials of _dirs (edges, vertices, axes, the zero vector, the diagonals) and 491 random ones."""
    return _dirs(491, 11, L)


def _assert_tangential(g_in, d, eps, tag):
    terms = np.asarray(g_in, np.float64) * d.astype(np.float64)
    radial, size = np.abs(terms.sum(1)), np.abs(terms).sum(1)
    print(f"tangent {tag}: worst radial / size {np.max(radial / np.maximum(size, 1e-300)):.3e} (bound {32 * eps:.3e}), max |g| {np.abs(g_in).max():.3g}")
    assert (radial <= 32 * eps * size).all(), (tag, int(np.argmax(radial - 32 * eps * size)))


def check_weights_and_tangent(encode, eps, sums_channels_in_uv):
    """(a) The fetch weights of a sample sum to one, so sum_texels grad_cubemap[:, c] + grad_fail[c] = sum_n go[c, n] within
    (B + 8) eps sum_n |go[c, n]| (B additions per texel at worst, plus the weights' own roundings): catches a vertex sample's folded
    fourth weight.  (b) The fetch depends on the direction only, not on its length: the direction gradient is tangential,
    |sum_k g_k d_k| <= 32 eps sum_k |g_k d_k| per sample, in the bilinear modes.  The bound is that of ONE application of the
    (u, v) -> (x, y, z) backward: its three products cancel to a few roundings of their own size.  It holds for the gradient of one
    channel in any implementation, and for all channels together where the channel slopes are summed in uv first and the backward
    applied once, as the HIP kernel does (`sums_channels_in_uv`).  The restatement applies it per channel and adds in xyz: channels
    that cancel there leave roundings of the per-channel size, which the [B, 3] result no longer shows."""
    C = 3
    for L in (1, 2, 5):
        rng = np.random.default_rng(200 + L)
        cm = rng.normal(size=(6, C, L, L)).astype(np.float32)
        fail = rng.normal(size=C).astype(np.float32)
        d = probe_dirs(L)
        B = len(d)
        assert B == 512
        go = rng.normal(size=(C, B)).astype(np.float32)
        for interp, seamless in MODES:
            _, g_in, g_cm, g_fail = (np.asarray(a, np.float64) for a in encode(d, cm, fail, interp, seamless, go))
            got = g_cm.sum(axis=(0, 2, 3)) + g_fail
            want = go.astype(np.float64).sum(1)
            bound = (B + 8) * eps * np.abs(go.astype(np.float64)).sum(1)
            print(f"weights L={L} mode=({interp},{seamless}): |sum error| {np.abs(got - want).max():.3e}, bound {bound.min():.3e}")
            assert (np.abs(got - want) <= bound).all(), (L, interp, seamless, got - want, bound)
            if interp == 0:
                assert np.abs(g_in).max() == 0.0
                continue
            if sums_channels_in_uv:
                _assert_tangential(g_in, d, eps, f"L={L} seamless={seamless} all channels")
            for c in range(C):
                one = np.zeros_like(go)
                one[c] = go[c]
                g_c = np.asarray(encode(d, cm, fail, interp, seamless, one)[1], np.float64)
                _assert_tangential(g_c, d, eps, f"L={L} seamless={seamless} channel {c}")
                if L > 1 or seamless:                      # (L = 1, plain: the four clamped taps are one texel, the slope is zero)
                    assert np.abs(g_c).max() > 1.0         # the property is not met by an all-zero gradient


def _cells(d, L):
    """(face, floor(pu - .5), floor(pv - .5)) of each direction -- the bilinear cell it samples in -- and whether it sits at least
    1e-3 of a texel inside that cell (so that fp32 and fp64 agree on it).  Geometry only: no edge table involved."""
    face, _ = co.compute_uv(np.asarray(d, np.float64))
    pu, pv = co.pixel_coords(d, L)
    fx, fy = np.floor(pu - 0.5), np.floor(pv - 0.5)
    inside = np.minimum.reduce([pu - 0.5 - fx, fx + 1 - (pu - 0.5), pv - 0.5 - fy, fy + 1 - (pv - 0.5)]) > 1e-3
    return np.stack([face, fx, fy], 1), inside


def check_gradient_is_the_slope(encode, eps):
    """The direction gradient is the slope of the implementation's OWN forward.  Moving one of the two minor components of d (the
    major one fixed) moves u or v linearly, and inside one bilinear cell the fetch is linear in each of them: the central difference
    over two points of the same cell IS the derivative, with no truncation error, at any step.  Steps of 1/128 .. 1/256 texel (powers
    of two), samples kept where d - h, d, d + h share the cell.  With the tangent check (which fixes the major component's gradient
    from the other two) this pins the whole gradient, sign flips of the edge and vertex cells included.
    Bound: a fetched value carries at most V = 16 (L + 1) eps M of rounding (kx, ky move by <= 4 L eps, slope <= 2 M, two axes: the
    texel-centre bound; plus 16 eps M for the blend itself), so the difference quotient of sum_c go_c out_c carries at most
    2 V sum_c |go_c| / (2 h); the bound is twice that, the gradient's own rounding being far smaller."""
    C = 3
    for L in (1, 2, 5):
        rng = np.random.default_rng(400 + L)
        cm = rng.normal(size=(6, C, L, L)).astype(np.float32)
        fail = np.zeros(C, np.float32)
        M = float(np.abs(cm).max())
        d = probe_dirs(L)
        d = d[np.any(d != 0, axis=1)]
        go = rng.normal(size=(C, len(d))).astype(np.float32)
        go1 = np.abs(go.astype(np.float64)).sum(0)
        major = np.argmax(np.abs(d), axis=1)
        rows = np.arange(len(d))
        h = (2.0 ** np.floor(np.log2(np.abs(d[rows, major]).astype(np.float64) / (64 * L)))).astype(np.float32)
        cell, inside = _cells(d, L)
        for seamless in (0, 1):
            g_in = np.asarray(encode(d, cm, fail, 1, seamless, go)[1], np.float64)
            phi = lambda x: (go.astype(np.float64) * np.asarray(encode(x, cm, fail, 1, seamless), np.float64)).sum(0)
            kept = 0
            seen = {"u<0": 0, "v<0": 0, "u>=L": 0, "v>=L": 0, "vertex": 0}
            for which in (1, 2):
                j = (major + which) % 3
                dp, dm = d.copy(), d.copy()
                dp[rows, j] += h
                dm[rows, j] -= h
                step = dp[rows, j].astype(np.float64) - dm[rows, j].astype(np.float64)
                (cp, ip), (cq, iq) = _cells(dp, L), _cells(dm, L)
                keep = inside & ip & iq & (cp == cell).all(1) & (cq == cell).all(1)
                fd = (phi(dp) - phi(dm)) / step
                tol = 2 * 2 * 16 * (L + 1) * eps * M * go1 / step
                err = np.abs(fd - g_in[rows, j])
                print(f"slope L={L} seamless={seamless} minor {which}: kept {int(keep.sum())}/{len(d)}, worst err / bound "
                      f"{np.max(err[keep] / tol[keep]):.3f}, median bound / |g| {np.median(tol[keep] / np.maximum(np.abs(g_in[rows, j][keep]), 1e-30)):.2e}")
                assert (err[keep] <= tol[keep]).all(), (L, seamless, which, int(np.argmax(np.where(keep, err / tol, 0))))
                kept += int(keep.sum())
                lo_u, lo_v, hi_u, hi_v = cell[:, 1] < 0, cell[:, 2] < 0, cell[:, 1] >= L - 1, cell[:, 2] >= L - 1
                for name, m in (("u<0", lo_u), ("v<0", lo_v), ("u>=L", hi_u), ("v>=L", hi_v), ("vertex", (lo_u | hi_u) & (lo_v | hi_v))):
                    seen[name] += int((m & keep).sum())
            assert kept > len(d) and min(seen.values()) >= 4, (L, seamless, kept, seen)     # more than half, every border class


def check_scale_invariance(encode, cubemap_rel):
    """encode(s d) = encode(d) and s grad_inputs(s d) = grad_inputs(d) bit for bit for s = 2^k: every operation of the direction ->
    (face, u, v) map and of its backward is exact under a power-of-two scale.  grad_cubemap agrees to `cubemap_rel` (atomics
    reorder)."""
    L, C = 5, 3
    rng = np.random.default_rng(300)
    cm = rng.normal(size=(6, C, L, L)).astype(np.float32)
    fail = rng.normal(size=C).astype(np.float32)
    d = probe_dirs(L)
    go = rng.normal(size=(C, len(d))).astype(np.float32)
    for interp, seamless in MODES:
        out, g_in, g_cm, g_fail = encode(d, cm, fail, interp, seamless, go)
        for k in (-20, -1, 1, 20):
            s = np.float32(2.0 ** k)
            out_s, g_in_s, g_cm_s, g_fail_s = encode(d * s, cm, fail, interp, seamless, go)
            assert np.array_equal(out_s, out), (interp, seamless, k, float(np.abs(out_s - out).max()))
            assert np.array_equal(g_in_s * s, g_in), (interp, seamless, k, float(np.abs(g_in_s * s - g_in).max()))
            assert rel_err(g_cm_s, g_cm) <= cubemap_rel and rel_err(g_fail_s, g_fail) <= cubemap_rel, (interp, seamless, k)


# ---- on the restatement (CPU) ---------------------------------------------------------------------------------------------------------
def test_oracle_texel_centres_all_faces():
    check_texel_centres(oracle_encode, 2.0 ** -53)


def test_oracle_seams_all_edges_and_vertices():
    check_seam_continuity(oracle_encode)


def test_oracle_weights_sum_to_one_and_gradient_is_tangential():
    check_weights_and_tangent(oracle_encode, 2.0 ** -53, False)


def test_oracle_gradient_is_the_slope_of_its_forward():
    check_gradient_is_the_slope(oracle_encode, 2.0 ** -53)


def test_oracle_scale_invariance():
    check_scale_invariance(oracle_encode, 0.0)


# ---- on the HIP kernels (GPU) -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_texel_centres_all_faces(gpu_device):
    check_texel_centres(hip_encode(gpu_device), 2.0 ** -24)


@pytest.mark.gpu
def test_hip_seams_all_edges_and_vertices(gpu_device):
    check_seam_continuity(hip_encode(gpu_device))


@pytest.mark.gpu
def test_hip_weights_sum_to_one_and_gradient_is_tangential(gpu_device):
    check_weights_and_tangent(hip_encode(gpu_device), 2.0 ** -24, True)


@pytest.mark.gpu
def test_hip_gradient_is_the_slope_of_its_forward(gpu_device):
    check_gradient_is_the_slope(hip_encode(gpu_device), 2.0 ** -24)


@pytest.mark.gpu
def test_hip_scale_invariance(gpu_device):
    check_scale_invariance(hip_encode(gpu_device), 1e-6)
