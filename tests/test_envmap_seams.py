"""The environment-map fetch (csrc/mrgs_envmap.h; restated as oracle/shading_oracle.py) at every seam, every level and through every
caller.  Kernel and statement transcribe the same re-projection trick (wrap_tap / _wrap with the 1/4096 pull), so a comparison of the
two cannot see a mistake they share at a seam.  Part 1 therefore pins the STATEMENT by the geometry of a cube alone, in float64 on the
CPU: texel centres, continuity across the twelve edges and at the eight vertices (probes of tests/test_cubemap_seams.py: plain xyz
directions, no face convention), weights that sum to one, a tangential direction gradient that is the slope of the forward -- and three
deliberate mistakes in the statement that those checks must catch.  Parts 2-4 then hold the kernels to the pinned statement on CELL
probes (tests/envmap_probes.py): directions well inside every border and vertex cell of every level, where random directions
practically never land.  `eps` is the unit roundoff of the implementation under test (2^-53 / 2^-24)."""
import functools

import numpy as np
import pytest
import torch

import envmap_probes as ep
import volume_statement as vs
from oracle import shading_oracle as so
from test_cubemap_seams import DELTA, edge_probe_pairs, vertex_probe_triples

F64 = torch.float64
EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24
CENTRE_LEVELS = (1, 2, 3, 4, 7)
SEAM_LEVELS = (1, 2, 4, 8, 33, 128)


def seam_texels(L):
    return np.random.default_rng(0).normal(size=(6, L, L, 3))


def centre_dirs(L):
    """cube_to_dir of every texel centre, in texel order (face, y, x): [6 L L, 3] float64."""
    lin = (torch.arange(L, dtype=F64) * 2 + 1) / L - 1
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    return torch.cat([so.cube_to_dir(s, gx, gy).reshape(-1, 3) for s in range(6)], 0)


# ---- the two implementations as one callable: fetch(tex [6,L,L,3], dirs [N,3], go [N,3] or None) ----------------------------------
def statement_fetch(tex, dirs, go=None):
    """so.cube_fetch in float64 (no sigmoid): out [N,3], or (out, g_dirs, g_tex) with the upstream gradient go."""
    t = torch.as_tensor(np.asarray(tex), dtype=F64).clone().requires_grad_(go is not None)
    d = torch.as_tensor(np.asarray(dirs), dtype=F64).clone().requires_grad_(go is not None)
    out = so.cube_fetch(t, d)
    if go is None:
        return out.detach().numpy()
    out.backward(torch.as_tensor(np.asarray(go), dtype=F64))
    return out.detach().numpy(), d.grad.numpy(), t.grad.numpy()


def clamped_fetch(tex, dirs, go=None):
    """The control: the same bilinear fetch with every tap clamped to the direction's own face."""
    t, d = torch.as_tensor(np.asarray(tex), dtype=F64), torch.as_tensor(np.asarray(dirs), dtype=F64)
    L = t.shape[1]
    face, u, v = so.dir_to_face_uv(d)
    fx, fy = (u * 0.5 + 0.5) * L - 0.5, (v * 0.5 + 0.5) * L - 0.5
    x0, y0 = torch.floor(fx), torch.floor(fy)
    wx, wy = (fx - x0).unsqueeze(-1), (fy - y0).unsqueeze(-1)
    xa, xb = x0.long().clamp(0, L - 1), (x0.long() + 1).clamp(0, L - 1)
    ya, yb = y0.long().clamp(0, L - 1), (y0.long() + 1).clamp(0, L - 1)
    out = (1 - wy) * ((1 - wx) * t[face, ya, xa] + wx * t[face, ya, xb]) + wy * ((1 - wx) * t[face, yb, xa] + wx * t[face, yb, xb])
    return out.numpy()


def hip_fetch(device):
    """shading._EnvLookup on one level without roughness: sigmoid(fetch), fp32 (no filter is built, so any L goes)."""
    from materialrefgs_amd.shading import _EnvLookup

    def fetch(tex, dirs, go=None):
        t = torch.tensor(np.asarray(tex, np.float32), device=device, requires_grad=go is not None)
        d = torch.tensor(np.asarray(dirs, np.float32), device=device, requires_grad=go is not None)
        out = _EnvLookup.apply(d, None, 0.08, 0.5, t)
        if go is None:
            return out.detach().cpu().numpy()
        out.backward(torch.tensor(np.asarray(go, np.float32), device=device))
        return out.detach().cpu().numpy(), d.grad.cpu().numpy(), t.grad.cpu().numpy()
    return fetch


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# ---- the geometry checks --------------------------------------------------------------------------------------------------------------
def check_texel_centres(fetch, eps, link, link_err):
    """A direction through a texel's centre fetches that texel, on all six faces: within 16 L eps M (the centre's rounding moves fx, fy
    by at most ~4 L eps, the patch slope is at most 2 M per unit weight; the bound doubles the product) -- the bound of
    test_cubemap_seams.  Through the kernels' sigmoid (slope <= 1/4, so the same bound holds for the fetch's part) `link_err` adds the
    sigmoid's own rounding: v_exp_f32 and v_rcp_f32 at 1 ulp each, the product x log2(e) and the sum 1 + e half an ulp each, on a value
    below one: 8 eps covers twice their sum."""
    for L in CENTRE_LEVELS:
        tex = np.random.default_rng(100 + L).normal(size=(6, L, L, 3)).astype(np.float32)
        M = float(np.abs(tex).max())
        want = link(tex.reshape(-1, 3).astype(np.float64))
        d = centre_dirs(L).numpy()
        bound = 16 * L * eps * M + link_err
        for scale in (1.0, 3.7):                  # un-normalised directions address the same texel
            err = float(np.abs(np.asarray(fetch(tex, d * scale), np.float64) - want).max())
            print(f"texel centres L={L} scale={scale}: max err {err:.3e}, bound {bound:.3e}")
            assert err <= bound, ("texel centre", L, scale, err, bound)


def seam_differences(fetch, L):
    """Largest difference between the probes on the two (three) sides of each of the 12 edges [12] and 8 vertices [8]."""
    tex = seam_texels(L)
    edges = []
    for _, d1, d2 in edge_probe_pairs():
        a, b = (np.asarray(fetch(tex, d), np.float64) for d in (d1, d2))
        edges.append(np.abs(a - b).max())
    verts = []
    for _, d in vertex_probe_triples():
        o = np.asarray(fetch(tex, d), np.float64)
        verts.append(max(np.abs(o[i] - o[j]).max() for i, j in ((0, 1), (0, 2), (1, 2))))
    return np.array(edges), np.array(verts)


def check_seam_continuity(fetch):
    """The fetch is continuous across all twelve edges and at all eight vertices: two probes DELTA inside the two (three) faces agree
    within 8 L DELTA M (each probe lies within 2 DELTA of the common point in u and in v; the fetch moves at most L M per unit uv per
    axis).  A sigmoid behind the fetch has slope <= 1/4: the same bound holds."""
    for L in SEAM_LEVELS:
        M = float(np.abs(seam_texels(L)).max())
        bound = 8 * L * DELTA * M
        edges, verts = seam_differences(fetch, L)
        worst = max(edges.max(), verts.max())
        print(f"seams L={L}: worst difference {worst:.3e}, bound {bound:.3e}, worst / bound {worst / bound:.3f}")
        assert (edges <= bound).all(), ("seam edge", L, edges, bound)
        assert (verts <= bound).all(), ("seam vertex", L, verts, bound)


def geometry_dirs(L):
    """The cell probes of level L (all 24 border strips, all 24 vertex cells) and 200 random directions, as float32 values."""
    rnd = torch.nn.functional.normalize(torch.randn(200, 3, generator=torch.Generator().manual_seed(300 + L), dtype=F64), dim=1)
    return torch.cat([ep.cell_probes(L, 8), rnd]).to(torch.float32).numpy().astype(np.float64)


def assert_tangential(g_dirs, d, eps, tag):
    """|sum_k g_k d_k| <= 32 eps sum_k |g_k d_k| per sample: ONE application of the (u, v) -> (x, y, z) backward, whose three products
    cancel to a few roundings of their own size (check_weights_and_tangent of test_cubemap_seams)."""
    terms = np.asarray(g_dirs, np.float64) * d
    radial, size = np.abs(terms.sum(1)), np.abs(terms).sum(1)
    print(f"tangent {tag}: worst radial / size {np.max(radial / np.maximum(size, 1e-300)):.3e} (bound {32 * eps:.3e}), max |g| {np.abs(g_dirs).max():.3g}")
    assert (radial <= 32 * eps * size).all(), (tag, int(np.argmax(radial - 32 * eps * size)))
    assert np.abs(g_dirs).max() > 1e-2, tag                      # the property is not met by an all-zero gradient


def check_weights_and_tangent(fetch, eps, zero_map):
    """(a) The tap weights of a sample sum to one: sum_texels g_tex[..., c] = k sum_n go[n, c] within (B + 8) eps k sum_n |go[n, c]| (B
    additions per texel at worst, plus the weights' own roundings); k = 1 for the bare fetch.  Through the kernels' sigmoid the map is
    all zero (`zero_map`): sigmoid_fast(0) is exactly 1/2, y (1 - y) exactly 1/4 = k.  Catches a vertex sample's weights that are not
    renormalised.  (b) The fetch depends on the direction only, not on its length: the direction gradient is tangential (on a random
    map)."""
    for L in (1, 2, 5, 16):
        rng = np.random.default_rng(200 + L)
        tex = rng.normal(size=(6, L, L, 3)).astype(np.float32)
        d = geometry_dirs(L)
        B = len(d)
        cls = ep.classify([L], torch.tensor(d), None)
        assert min(int(m.sum()) for k, m in cls["classes"].items() if k[1] == "v") >= 4          # samples in all 24 vertex cells
        go = rng.normal(size=(B, 3)).astype(np.float32).astype(np.float64)
        k = 0.25 if zero_map else 1.0
        _, _, g_tex = fetch(np.zeros_like(tex) if zero_map else tex, d, go)
        got, want = np.asarray(g_tex, np.float64).sum(axis=(0, 1, 2)), k * go.sum(0)
        bound = (B + 8) * eps * k * np.abs(go).sum(0)
        print(f"weights L={L}: |sum error| {np.abs(got - want).max():.3e}, bound {bound.min():.3e}")
        assert (np.abs(got - want) <= bound).all(), ("weight sum", L, got - want, bound)
        _, g_dirs, _ = fetch(tex, d, go)
        assert_tangential(g_dirs, d, eps, f"L={L}")


def _raw_taps(L, d, taps=None):
    """The un-normalised bilinear weights [4, N] of so.bilinear_taps' own taps (the missing vertex tap at zero), from the cell
    coordinates the statement returns: the vertex rule of the header is stated on these."""
    idx, w, fx, fy, _ = (taps or so.bilinear_taps)(L, d)
    x0, y0 = torch.floor(fx), torch.floor(fy)
    wx, wy = fx - x0, fy - y0
    ox, oy = [x0 < 0, x0 + 1 >= L] * 2, [y0 < 0, y0 < 0, y0 + 1 >= L, y0 + 1 >= L]
    raw = torch.stack([(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy])
    corner = torch.stack([ox[k] & oy[k] for k in range(4)])
    return torch.stack(idx), torch.where(corner, torch.zeros_like(raw), raw), corner.any(0), torch.stack([x0, y0, fx - x0, fy - y0], 1)


def check_gradient_is_the_slope(fetch, eps):
    """The direction gradient is the slope of the implementation's OWN forward.  Moving one of the two minor components of d (the major
    one fixed) moves u or v linearly, and inside one bilinear cell the fetch is linear in each of them: the central difference over two
    points of the same cell IS the derivative, with no truncation error (check_gradient_is_the_slope of test_cubemap_seams, whose step
    and bound these are: a fetched value carries at most V = 16 (L + 1) eps M of rounding, the quotient of sum_c go_c out_c at most
    2 V sum_c |go_c| / step; the bound is twice that).  With the tangent check this pins the whole gradient.
    In VERTEX cells the rule is another by design -- "renormalisation held constant" -- and what is asserted is what the header states:
    the gradient equals `norm` times the slope of the un-normalised three-tap sum, which IS bilinear in the cell.  How far that is from
    the true slope of the forward is printed: the size of the deviation is on record, not asserted.
    For the bare fetch only: behind the kernels' sigmoid the forward is no longer linear in the cell, and their slope is compared with
    this statement's in part 2b."""
    for L in (1, 2, 5, 16):
        rng = np.random.default_rng(400 + L)
        tex = rng.normal(size=(6, L, L, 3)).astype(np.float32).astype(np.float64)
        M = float(np.abs(tex).max())
        d = geometry_dirs(L)
        N = len(d)
        go = rng.normal(size=(N, 3)).astype(np.float32).astype(np.float64)
        go1 = np.abs(go).sum(1)
        rows = np.arange(N)
        major = np.argmax(np.abs(d), axis=1)
        h = 2.0 ** np.floor(np.log2(np.abs(d[rows, major]) / (64 * L)))
        _, g_dirs, _ = fetch(tex, d, go)
        td = torch.tensor(d)
        idx, raw, vertex, cell = _raw_taps(L, td)
        vertex, norm = vertex.numpy(), (1.0 / raw.sum(0)).numpy()
        flat = torch.tensor(tex).reshape(-1, 3)
        phi = lambda x: (go * np.asarray(fetch(tex, x), np.float64)).sum(1)

        def unnormalised(x):         # sum_c go_c (three-tap sum without the renormalisation), on the taps of x's own cell
            i, r, _, _ = _raw_taps(L, torch.tensor(x))
            return (torch.tensor(go) * sum(r[k].unsqueeze(-1) * flat[i[k]] for k in range(4))).sum(1).numpy()
        seen = {"edge": 0, "vertex": 0, "inner": 0}
        worst_dev = 0.0
        for which in (1, 2):
            j = (major + which) % 3
            dp, dm = d.copy(), d.copy()
            dp[rows, j] += h
            dm[rows, j] -= h
            step = dp[rows, j] - dm[rows, j]
            cp, cq = _raw_taps(L, torch.tensor(dp))[3], _raw_taps(L, torch.tensor(dm))[3]
            inside = lambda c: (torch.minimum(c[:, 2:], 1 - c[:, 2:]).min(1).values > 1e-3).numpy()
            same = (cp[:, :2] == cell[:, :2]).all(1).numpy() & (cq[:, :2] == cell[:, :2]).all(1).numpy()
            fp, fq = (np.abs(x).argmax(1) == major for x in (dp, dm))
            keep = inside(cell) & inside(cp) & inside(cq) & same & fp & fq
            tol = 2 * 2 * 16 * (L + 1) * eps * M * go1 / step
            fd_true = (phi(dp) - phi(dm)) / step
            fd_rule = norm * (unnormalised(dp) - unnormalised(dm)) / step
            err = np.abs(np.where(vertex, fd_rule, fd_true) - g_dirs[rows, j])
            border = (cell[:, 0] < 0) | (cell[:, 0] + 1 >= L) | (cell[:, 1] < 0) | (cell[:, 1] + 1 >= L)
            border = border.numpy()
            seen["vertex"] += int((keep & vertex).sum())
            seen["edge"] += int((keep & border & ~vertex).sum())
            seen["inner"] += int((keep & ~border).sum())
            if (keep & vertex).any():
                dev = np.abs(fd_true - g_dirs[rows, j])[keep & vertex] / np.maximum(np.abs(fd_true[keep & vertex]), 1e-300)
                worst_dev = max(worst_dev, float(np.median(dev)))
            print(f"slope L={L} minor {which}: kept {int(keep.sum())}/{N}, worst err / bound {np.max(err[keep] / tol[keep]):.3f}")
            assert (err[keep] <= tol[keep]).all(), (L, which, int(np.argmax(np.where(keep, err / tol, 0))))
        print(f"slope L={L}: rows checked {seen}; in vertex cells the held-constant gradient is a median {worst_dev:.3f} of the true "
              f"slope away from it (relative)")
        assert seen["vertex"] >= 48 and (L == 1 or seen["edge"] >= 48), (L, seen)


# ---- 1. the statement, by geometry alone (CPU, float64) --------------------------------------------------------------------------------
def test_statement_texel_centres_all_faces():
    check_texel_centres(statement_fetch, EPS64, lambda x: x, 0.0)


def test_statement_seams_all_edges_and_vertices():
    check_seam_continuity(statement_fetch)
    for L in SEAM_LEVELS:                      # the control: the probes do straddle, a tap taken from the wrong place would show
        edges, _ = seam_differences(clamped_fetch, L)
        print(f"seams L={L}: smallest clamp-to-face jump over the 12 edges {edges.min():.3f}")
        assert (edges > 0.5).all(), (L, edges)


def test_statement_weights_sum_to_one_and_gradient_is_tangential():
    check_weights_and_tangent(statement_fetch, EPS64, zero_map=False)


def test_statement_gradient_is_the_slope_of_its_forward():
    check_gradient_is_the_slope(statement_fetch, EPS64)


def _fails(check, tag):
    """The check fails, and on the assertion that carries `tag` in its message: another assertion of the same check (coverage,
    tangency) firing first does not count as the mistake caught."""
    try:
        check()
    except AssertionError as e:
        return tag in str(e)
    return False


def test_geometry_checks_catch_three_mistakes_in_the_statement(monkeypatch):
    """The checks bite: each of three deliberate mistakes in the statement (never a code path of the repository) fails the checks
    named beside it, and the unpatched statement passes them again afterwards."""
    centres = lambda: check_texel_centres(statement_fetch, EPS64, lambda x: x, 0.0)
    seams = lambda: check_seam_continuity(statement_fetch)
    weights = lambda: check_weights_and_tangent(statement_fetch, EPS64, zero_map=False)
    taps, face_uv = so.bilinear_taps, so.dir_to_face_uv

    def not_renormalised(res, dirs):             # a. the vertex weights keep their bilinear values: they sum to less than one
        idx, w, fx, fy, face = taps(res, dirs)
        _, raw, vertex, _ = _raw_taps(res, dirs, taps)
        return idx, [torch.where(vertex, raw[k], w[k]) for k in range(4)], fx, fy, face

    def flipped(d):                              # c. face 2 (+y) with u mirrored
        face, u, v = face_uv(d)
        return face, torch.where(face == 2, -u, u), v

    with monkeypatch.context() as m:
        m.setattr(so, "bilinear_taps", not_renormalised)
        assert _fails(weights, "weight sum")
    with monkeypatch.context() as m:             # b. the pull goes the wrong way: the off-face tap re-projects onto its own face
        m.setattr(so, "EPS_EDGE", -so.EPS_EDGE)
        assert _fails(seams, "seam edge")
    with monkeypatch.context() as m:
        m.setattr(so, "dir_to_face_uv", flipped)
        assert _fails(centres, "texel centre") and _fails(seams, "seam edge")
    centres(), seams(), weights()



# ---- 2. the lookup kernels ----------------------------------------------------------------------------------------------------------------
# every level an independent random tensor, not a box mip of the one above: a tap taken from the wrong level shows
LEVEL_SETS = ((1,), (2,), (3,), (7,), (33,), (128,), (128, 64, 32, 16), (33, 16, 8), (8, 4, 2, 1), (4, 2))
CAP_FORWARD, CAP_TEXELS, CAP_ROWS = 3e-6, 2e-5, 1e-4          # test_envmap_lookup_parity's
MIN_CLASS_ROWS, MAX_LEFT_OUT = 4, 0.01


def random_levels(res_list, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(6, r, r, 3, generator=g) for r in res_list]


def lookup_statement(mips, dirs, rough, go, dtype):
    """so.env_lookup in `dtype` on the CPU: (out, [g_level ...], g_dirs, g_roughness or None)."""
    leaves = [m.to(dtype).clone().requires_grad_(True) for m in mips]
    d = dirs.to(dtype).clone().requires_grad_(True)
    r = None if rough is None else rough.to(dtype).clone().requires_grad_(True)
    out = so.env_lookup(leaves, d, r)
    out.backward(go.to(dtype))
    return out.detach(), [t.grad for t in leaves], d.grad, None if r is None else r.grad


def lookup_hip(device, mips, dirs, rough, go):
    from materialrefgs_amd.shading import _EnvLookup
    leaves = [m.to(device).requires_grad_(True) for m in mips]
    d = dirs.to(device).requires_grad_(True)
    r = None if rough is None else rough.to(device).requires_grad_(True)
    out = _EnvLookup.apply(d, r, 0.08, 0.5, *leaves)
    out.backward(go.to(device))
    return out.detach().cpu(), [t.grad.cpu() for t in leaves], d.grad.cpu(), None if r is None else r.grad.cpu()


class LookupCase:
    """One input of the lookup kernels with its float64 and fp32 statements and the rows' classification, built once on the CPU."""

    def __init__(self, res_list, dirs, rough, seed):
        self.res_list, self.dirs, self.rough = res_list, dirs, rough
        self.mips = random_levels(res_list, seed)
        self.go = torch.randn(dirs.shape[0], 3, generator=torch.Generator().manual_seed(seed + 1))
        self.ref = lookup_statement(self.mips, dirs, rough, self.go, F64)
        self.lit = lookup_statement(self.mips, dirs, rough, self.go, torch.float32)
        self.cls = ep.classify(res_list, dirs, rough)


@functools.lru_cache(maxsize=None)
def lookup_case(res_list):
    dirs, rough = ep.probe_rows(res_list)
    return LookupCase(res_list, dirs, rough, 7000 + sum(res_list))


def capped(label, got, ref, lit, cap, relative, rows=None):
    """One tensor against the float64 statement: max |got - ref| (over `rows`), relative to the statement's largest entry where the
    cap is stated so, must be within `cap` -- or, by the truth-leg rule of DESIGN section 3, no further from float64 than 1.5 x the
    fp32 statement on the same inputs.  Prints both errors; returns the kernel's."""
    got, ref, lit = got.double(), ref.double(), lit.double()
    scale = max(float(ref.abs().max()), 1e-30) if relative else 1.0
    if rows is not None:
        got, ref, lit = got[rows], ref[rows], lit[rows]
    e_hip = float((got - ref).abs().max()) / scale if ref.numel() else 0.0
    e_lit = float((lit - ref).abs().max()) / scale if ref.numel() else 0.0
    line = f"{label}: kernel {e_hip:.2e}, fp32 statement {e_lit:.2e}, cap {cap:.0e}"
    print(line)
    assert e_hip <= cap or e_hip <= 1.5 * e_lit, line
    return e_hip


def assert_lookup_case(case, got, tag):
    out, g_levels, g_dirs, g_rough = got
    ref, lit, cls = case.ref, case.lit, case.cls
    worst = {"forward": capped(f"{tag} forward", out, ref[0], lit[0], CAP_FORWARD, False)}
    worst["texels"] = max(capped(f"{tag} texels {r}^2", g_levels[i], ref[1][i], lit[1][i], CAP_TEXELS, True) for i, r in enumerate(case.res_list))
    worst["g_dirs"] = capped(f"{tag} g_dirs", g_dirs, ref[2], lit[2], CAP_ROWS, True, cls["keep"])
    if g_rough is not None:
        worst["g_roughness"] = capped(f"{tag} g_roughness", g_rough, ref[3], lit[3], CAP_ROWS, True, cls["keep"] & ~cls["knot"])
    left, fewest, which = ep.coverage(cls)
    print(f"{tag}: N={case.dirs.shape[0]} worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f" (caps {CAP_FORWARD:.0e} / {CAP_TEXELS:.0e} / {CAP_ROWS:.0e}); left out {left:.4f}, smallest class {fewest} rows {which}")


@pytest.mark.parametrize("res_list", LEVEL_SETS, ids=lambda r: "x".join(map(str, r)))
def test_lookup_probes_cover_every_class_with_margin(res_list):
    """The conditions of the comparison, on every input the GPU part uses: at most 1 % of the rows left out of the per-row gradients
    for a tap coordinate within 1e-3 texel of an integer or a face gap under 1e-4, and every (level, face, side) border class and
    every (level, face, corner) vertex class that exists (a 1^2 level has vertex cells only) still with >= 4 rows -- also after the
    rows whose roughness sits on a knot have left, which g_roughness alone leaves out (they are there by construction: every integer
    level is probed, for the forward, the texel gradients and g_dirs, all continuous in the level)."""
    case = lookup_case(res_list)
    assert case.dirs.shape[0] <= 10000
    left, fewest, which = ep.coverage(case.cls)
    _, fewest_r, which_r = ep.coverage(case.cls, ~case.cls["knot"])
    n_classes = len(case.cls["classes"])
    print(f"{res_list}: N={case.dirs.shape[0]}, left out {left:.4f}, {n_classes} classes, smallest {fewest} rows {which}; "
          f"off the knots {fewest_r} rows {which_r}, on a knot {float(case.cls['knot'].double().mean()):.2f} of the rows")
    assert n_classes == sum(48 if r >= 2 else 24 for r in res_list)
    assert left <= MAX_LEFT_OUT and fewest >= MIN_CLASS_ROWS and fewest_r >= MIN_CLASS_ROWS
    # the share on a knot is the cycle's own: 2 n + 1 distinct values (below min, n integer levels, n - 1 half levels, above 1;
    # max_roughness and 1 are the levels n - 2 and n - 1), the n integer levels on a knot -- under one half, and exactly that
    n = len(res_list)
    on_knot = float(case.cls["knot"].double().mean())
    assert on_knot == (0.0 if n == 1 else pytest.approx(n / (2 * n + 1), abs=1e-12)), (res_list, on_knot)


@pytest.mark.gpu
def test_hip_lookup_texel_centres_all_faces(gpu_device):
    check_texel_centres(hip_fetch(gpu_device), EPS32, _sigmoid, 8 * EPS32)


@pytest.mark.gpu
def test_hip_lookup_seams_all_edges_and_vertices(gpu_device):
    check_seam_continuity(hip_fetch(gpu_device))


@pytest.mark.gpu
def test_hip_lookup_weights_sum_to_one_and_gradient_is_tangential(gpu_device):
    check_weights_and_tangent(hip_fetch(gpu_device), EPS32, zero_map=True)


@pytest.mark.gpu
@pytest.mark.parametrize("res_list", [(128, 64, 32, 16), (8, 4, 2, 1), (4, 2)], ids=lambda r: "x".join(map(str, r)))
def test_hip_lookup_level_shares_sum_per_level(gpu_device, res_list):
    """On an all-zero chain (sigmoid_fast(0) = 1/2 exactly, y (1 - y) = 1/4) the texel gradients of level l sum to
    sum_n go_n share_l(n) / 4 per channel, share = (1 - f, f) of the float64 statement: pins the blend factors, the two clamps of
    env_levels and the select chains level_res / level_tex (a gradient sent to another level changes two sums).
    Bound, per level and channel, over the B_l rows within one level of l: (B_l + 8) eps sum |go| / 4 as in check_weights_and_tangent,
    plus the share's own rounding -- the fp32 level is (c - lo) * rcp(hi - lo) * (n - 2): c - lo, the reciprocal (1 ulp), two products
    and float(lo), float(hi) for the double constants, each a relative rounding of a level <= n - 1, eight roundings allowed:
    8 (n - 1) eps sum |go| / 4."""
    case = lookup_case(res_list)
    n, B = len(res_list), case.dirs.shape[0]
    zeros = [torch.zeros_like(m) for m in case.mips]
    _, g_levels, _, _ = lookup_hip(gpu_device, zeros, case.dirs, case.rough, case.go)
    share, _ = ep.level_shares(case.rough, n)
    lc = torch.clamp(so.get_mip(case.rough.double(), n), 0, n - 1)
    go = case.go.double()
    for l, r in enumerate(res_list):
        near = (lc - l).abs() <= 1
        want = 0.25 * (go * share[l].unsqueeze(-1)).sum(0)
        got = g_levels[l].double().sum(dim=(0, 1, 2))
        bound = (int(near.sum()) + 8 + 8 * (n - 1)) * EPS32 * 0.25 * go[near].abs().sum(0)
        print(f"level shares {res_list} level {r}^2: |sum error| {float((got - want).abs().max()):.3e}, bound {float(bound.min()):.3e}, sum {want.tolist()}")
        assert bool(((got - want).abs() <= bound).all()), (res_list, r, got - want, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("res_list", LEVEL_SETS, ids=lambda r: "x".join(map(str, r)))
def test_hip_lookup_matches_float64_in_every_border_and_vertex_cell(gpu_device, res_list):
    """2b: forward, the texel gradients of every level, g_dirs and g_roughness against so.env_lookup in float64 on the cell probes
    with every roughness of the cycle."""
    case = lookup_case(res_list)
    assert_lookup_case(case, lookup_hip(gpu_device, case.mips, case.dirs, case.rough, case.go), "x".join(map(str, res_list)))


def _sub_case(case, rows):
    return LookupCase(case.res_list, case.dirs[rows].clone(), None if case.rough is None else case.rough[rows].clone(), 7100 + len(rows))


PARTIAL_N = (1, 63, 65, 321)


@functools.lru_cache(maxsize=None)
def partial_wave_cases(N):
    """2c's inputs: N rows taken with a stride from the probes of the chain (128, 64, 32, 16), and from those of 33^2 alone."""
    full, lone = lookup_case((128, 64, 32, 16)), lookup_case((33,))
    rows = torch.arange(N) * (full.dirs.shape[0] // N) + (full.dirs.shape[0] // 2 + 2 if N == 1 else 0)
    return _sub_case(full, rows), _sub_case(lone, rows % lone.dirs.shape[0])


@functools.lru_cache(maxsize=None)
def scatter_case():
    """2d's input.  Wave 0: 64 different probes (far more than four distinct texels per tap: most lanes fall through to plain
    atomics); wave 1: one vertex-cell direction and one roughness 64 times (one round); wave 2: five distinct directions (the fifth
    texel falls through)."""
    full = lookup_case((128, 64, 32, 16))
    per = len(ep.roughness_cycle(4))
    stride = torch.arange(64) * (full.dirs.shape[0] // 64)
    vertex_row = int(torch.nonzero(full.cls["classes"][(0, "v", 2, 3)] & full.cls["keep"] & ~full.cls["knot"])[0])
    five = torch.arange(64) % 5 * per * 7 + 3
    return _sub_case(full, torch.cat([stride, torch.full((64,), vertex_row), five]))


def test_lookup_sub_cases_keep_rows_with_margin():
    """The conditions of 2c and 2d (they are about lane counts, not about classes): every sub-case keeps rows for g_dirs and, off the
    knots, for g_roughness -- the single row of N = 1 is such a row --, at most 1 % of a sub-case of a hundred rows or more are left
    out, and the 64 equal rows of 2d's second wave sit in a vertex cell of the 128^2 level with margin and off the knots."""
    for N in PARTIAL_N:
        chain, lone = partial_wave_cases(N)
        for case in (chain, lone):
            keep = case.cls["keep"]
            assert case.dirs.shape[0] == N and int(keep.sum()) >= 1
            assert N < 100 or float((~keep).double().mean()) <= MAX_LEFT_OUT
        assert int((chain.cls["keep"] & ~chain.cls["knot"]).sum()) >= 1
    case = scatter_case()
    wave1 = torch.arange(64, 128)
    vertex = torch.stack([m for k, m in case.cls["classes"].items() if k[0] == 0 and k[1] == "v"]).any(0)
    assert bool((case.cls["keep"] & ~case.cls["knot"] & vertex)[wave1].all()) and bool((case.dirs[wave1] == case.dirs[64]).all())
    assert len(torch.unique(case.dirs[128:], dim=0)) == 5 and len(torch.unique(case.dirs[:64], dim=0)) > 4
    assert float((~case.cls["keep"]).double().mean()) <= MAX_LEFT_OUT


@pytest.mark.gpu
@pytest.mark.parametrize("N", PARTIAL_N)
def test_hip_lookup_partial_waves(gpu_device, N):
    """2c: N = 1 and N off the multiples of 64 and 256 -- the backward keeps its out-of-range lanes alive for the convergent scatter,
    reading row N - 1 with a zero gradient: the texel sums must not see them."""
    case, single = partial_wave_cases(N)
    assert_lookup_case(case, lookup_hip(gpu_device, case.mips, case.dirs, case.rough, case.go), f"N={N}")
    assert_lookup_case(single, lookup_hip(gpu_device, single.mips, single.dirs, single.rough, single.go), f"N={N} 33^2 alone")


@pytest.mark.gpu
def test_hip_lookup_scatter_rounds_and_fall_through(gpu_device):
    """2d: texel_scatter elects at most four leaders a call (scatter_case: many texels, one texel, five texels a wave).  Sums within
    2b's caps."""
    case = scatter_case()
    assert_lookup_case(case, lookup_hip(gpu_device, case.mips, case.dirs, case.rough, case.go), "scatter rounds")


# ---- 3. the fused shading -----------------------------------------------------------------------------------------------------------------
FRAMES = ((48, 64), (48, 128))          # 4 and 8 tiles of 64 x 12 pixels: the second is more than one workgroup's window of four
SHADE_LEVELS = (128, 64, 32, 16)        # the two coarse levels sit in the dense LDS copy, the two fine ones go through the hash table
LUT_MARGIN = 1e-3                       # texels of the split-sum table


class ShadeFrame:
    """A probe frame, built once on the CPU: for pixel p the mirror direction of the view ray about normal = normalize(w_o + r) is the
    cell probe r (skipping targets nearly opposite to w_o, |w_o + r| < 0.2); everything that classifies the pixels comes from the
    float64 statement on the fp32 inputs (so.mirror_dirs, so.shade_taps) -- the view rays included (rays_dtype): the reference sets
    them up in float32, where `pixel_world - rays_o` cancels the camera distance and leaves the ray 3-4 ulp from the exact one; at
    128^2 a fetch magnifies that by 64 texels per unit, so a "float64" reading on float32 rays sits 1.9e-5 .. 2.4e-5 from the exact
    one on these frames, as far as any fp32 evaluation does.  The fp32 leg of the truth-leg rule keeps the reference's float32 rays."""

    def __init__(self, H, W):
        from materialrefgs_amd.shading import load_fg_lut
        from materialrefgs_amd.synthetic import orbit_camera
        self.H, self.W, N = H, W, H * W
        self.cam = cam = orbit_camera(1, H, W)
        K = cam.HWK[2]
        rays, _ = so.sample_camera_rays(H, W, K, cam.R, cam.T, F64)
        w_o = -rays.reshape(-1, 3).double()
        probes = torch.nn.functional.normalize(ep.cell_probes(SHADE_LEVELS[0], 6), dim=1)
        M = probes.shape[0]
        cyc = torch.tensor(ep.roughness_cycle(len(SHADE_LEVELS)))
        pick = torch.arange(N) % M
        for _ in range(M):
            bad = (w_o + probes[pick]).norm(dim=1) < 0.2
            if not bool(bad.any()):
                break
            pick = torch.where(bad, (pick + 1) % M, pick)
        self.target = probes[pick]
        g = torch.Generator().manual_seed(31 * W)
        self.normal = torch.nn.functional.normalize(w_o + self.target, dim=1).float().reshape(H, W, 3)
        self.rough = cyc[(torch.arange(N) // M + pick) % len(cyc)].reshape(H, W, 1)
        self.albedo, self.refl = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 1, generator=g) * 0.9 + 0.05
        self.alpha = torch.rand(H, W, 1, generator=g) * 0.8 + 0.2
        self.base, self.indirect = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
        self.mips = random_levels(SHADE_LEVELS, 9000 + W)
        self.lut = load_fg_lut("cpu")
        self.dirs, _ = so.mirror_dirs(H, W, K, cam.R, cam.T, self.normal.double(), F64)
        self.taps = so.shade_taps(list(SHADE_LEVELS), H, W, K, cam.R, cam.T, self.normal.double(), self.rough.double(), rays_dtype=F64)
        self.cls = ep.classify(SHADE_LEVELS, self.dirs, self.rough.reshape(-1))
        lut_xy = self.taps["lut_uv"] * self.lut.shape[0] - 0.5
        self.cls["keep"] = self.cls["keep"] & ((lut_xy - torch.round(lut_xy)).abs().min(dim=1).values >= LUT_MARGIN)
        self.ups = [torch.randn(s, generator=g) for s in ((3, H, W), (3, H, W), (H, W, 3), (3, H, W), (3, H, W))]   # spec, direct, weight, render, diffuse
        self.positive = torch.rand(3, H, W, generator=g) + 0.5

    def statement(self, dtype):
        """so.specular_color_surfel and render_surfel's compositing (diffuse = (1 - refl) base, render = diffuse + specular +
        bg (1 - alpha), linear) in `dtype`: outputs (spec, direct, weight, render, diffuse) and the gradients of
        (albedo, normal, alpha, refl, rough, base, *levels) under self.ups."""
        cam, H, W = self.cam, self.H, self.W
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (self.albedo, self.normal, self.alpha, self.refl, self.rough, self.base)]
        levels = [m.to(dtype).clone().requires_grad_(True) for m in self.mips]
        albedo, normal, alpha, refl, rough, base = leaves
        spec, direct, weight = so.specular_color_surfel(levels, self.lut.to(dtype), albedo, H, W, cam.HWK[2], cam.R, cam.T, normal, alpha, refl, rough,
                                                        rays_dtype=dtype)
        diffuse = (1 - refl.permute(2, 0, 1)) * base
        render = diffuse + spec + BG.to(dtype)[:, None, None] * (1 - alpha.permute(2, 0, 1))
        outs = (spec, direct, weight, render, diffuse)
        g_shade = torch.autograd.grad(outs[:3], leaves[:5] + levels, [u.to(dtype) for u in self.ups[:3]], retain_graph=True)
        g_fused = torch.autograd.grad(outs, leaves + levels, [u.to(dtype) for u in self.ups])
        return [o.detach() for o in outs], g_shade, g_fused


BG = torch.tensor([0.2, 0.4, 0.6])
SHADE_LEAVES = ("albedo", "normal", "alpha", "refl", "rough")


@functools.lru_cache(maxsize=None)
def shade_frame(H, W):
    f = ShadeFrame(H, W)
    f.ref, f.lit = f.statement(F64), f.statement(torch.float32)
    return f


@pytest.mark.parametrize("H,W", FRAMES)
def test_shading_probe_frames_cover_every_class_with_margin(H, W):
    """The conditions of part 3's comparisons: the realised mirror directions sit on their targets (4e-6), at most 1 % of the pixels
    are left out of the per-pixel gradients (cell, face, LUT cell), and every border and vertex class of all four levels keeps >= 4
    pixels, also off the roughness knots."""
    f = shade_frame(H, W)
    off = float((torch.nn.functional.normalize(f.dirs, dim=1) - f.target).norm(dim=1).max())
    left, fewest, which = ep.coverage(f.cls)
    _, fewest_r, _ = ep.coverage(f.cls, ~f.cls["knot"])
    print(f"frame {H}x{W}: mirror directions within {off:.2e} of their targets, left out {left:.4f}, smallest class {fewest} pixels {which}, "
          f"off the knots {fewest_r}")
    assert off <= 4e-6 and left <= MAX_LEFT_OUT and fewest >= MIN_CLASS_ROWS and fewest_r >= MIN_CLASS_ROWS
    assert len(f.cls["classes"]) == 4 * 48


def support_sets(f):
    """Per level, the texels that MUST receive a gradient when every pixel sends a strictly positive one -- so.shade_taps' keys of the
    pixels with margin, and for a pixel whose roughness sits on a knot the taps of the level it rounds to -- and the texels that MAY
    in addition: a knot pixel's taps on the two levels beside it (fp32 may put the level a rounding to either side), and for a pixel
    without margin the taps of its direction moved by up to 3e-3 texel of the level / 3e-4 of the face gap along each axis."""
    import itertools
    n, keep, knot = len(SHADE_LEVELS), f.cls["keep"], f.cls["knot"]
    lc = torch.clamp(so.get_mip(f.rough.reshape(-1).double(), n), 0, n - 1)
    keys = f.taps["keys"][keep & ~knot]
    keys = keys[keys >= 0]
    required = [set((keys[(keys >> 24) == l] & 0xffffff).tolist()) for l in range(n)]
    allowed = [set() for _ in range(n)]

    def taps_of(l, dirs):
        idx, w, _, _, _ = so.bilinear_taps(SHADE_LEVELS[l], dirs)
        return set(torch.stack(idx)[torch.stack(w) != 0].tolist())
    loose = torch.nonzero(~keep).reshape(-1)
    for l in range(n):
        near = torch.round(lc).long()
        required[l] |= taps_of(l, f.dirs[keep & knot & (near == l)])
        allowed[l] |= taps_of(l, f.dirs[keep & knot & ((near - l).abs() == 1)])
        rows = loose[(lc[loose] - l).abs() < 1 + ep.KNOT_MARGIN]
        d = f.dirs[rows]
        big = d.abs().max(dim=1, keepdim=True).values
        for size in (3e-3 * 2 / SHADE_LEVELS[l], 3e-4):
            for s in itertools.product((-1.0, 0.0, 1.0), repeat=3):
                allowed[l] |= taps_of(l, d + torch.tensor(s, dtype=F64) * size * big)
    return required, allowed


def assert_support(f, g_levels, tag):
    required, allowed = support_sets(f)
    for l, r in enumerate(SHADE_LEVELS):
        got = set(torch.nonzero(g_levels[l].reshape(-1, 3).abs().sum(1)).reshape(-1).tolist())
        missing, extra = required[l] - got, got - required[l] - allowed[l]
        print(f"{tag} support {r}^2: {len(got)} texels with a gradient, {len(required[l])} required, {len(allowed[l] - required[l])} slack; "
              f"missing {len(missing)}, unexpected {len(extra)}")
        assert not missing and not extra, (tag, r, sorted(missing)[:8], sorted(extra)[:8])


def assert_shade_grads(f, names, got, ref, lit, tag):
    rows = {"normal": f.cls["keep"], "rough": f.cls["keep"] & ~f.cls["knot"]}
    worst = {}
    for name, a, r, b in zip(names, got, ref, lit):
        sel = rows.get(name)
        if sel is not None:
            a, r, b = (t.reshape(f.H * f.W, -1) for t in (a, r, b))
        worst[name] = capped(f"{tag} d/d{name}", a, r, b, 1e-4, True, sel)
    return worst


def _shade_env(device, f):
    from materialrefgs_amd.shading import EnvLight
    env = EnvLight(device=device, min_res=16, max_res=16)          # (its own 16^2 chain is replaced: no 128^2 filter is built)
    env.specular = [m.to(device).requires_grad_(True) for m in f.mips]
    return env


def _fwd_cap(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", FRAMES)
def test_hip_specular_shading_in_every_border_and_vertex_cell(gpu_device, H, W):
    """get_specular_color_surfel (shade_specular_fwd_kernel, shade_fused_bwd_kernel without the compositing) on a probe frame against
    so.specular_color_surfel in float64: the caps of test_shade_specular_parity with the truth-leg fallback; then the exact support
    of the texel gradients under a strictly positive gradient on direct_light."""
    from materialrefgs_amd.shading import get_specular_color_surfel
    f = shade_frame(H, W)
    camd = f.cam.to(gpu_device)
    tag = f"specular {H}x{W}"

    def run():      # (a fresh graph for each backward, as in the composite test below, whose node serves one backward only)
        env = _shade_env(gpu_device, f)
        chw = [t.permute(2, 0, 1).contiguous().to(gpu_device).requires_grad_(True) for t in (f.albedo, f.normal, f.alpha, f.refl, f.rough)]
        hwc = [t.permute(1, 2, 0) for t in chw]          # strided inputs, as render_surfel passes them
        spec, extra = get_specular_color_surfel(env, hwc[0], f.cam.HWK, camd.R, camd.T, hwc[1], hwc[2], refl_strength=hwc[3], roughness=hwc[4])
        return env, chw, (spec, extra["direct_light"], extra["specular_weight"])
    env, chw, outs = run()
    fw = max(capped(f"{tag} {n}", o.detach().cpu(), r, b, _fwd_cap(r), False) / _fwd_cap(r)
             for n, o, r, b in zip(("specular", "direct_light", "specular_weight"), outs, f.ref[0], f.lit[0]))
    grads = torch.autograd.grad(outs, chw + env.specular, [u.to(gpu_device) for u in f.ups[:3]])
    got = [g.permute(1, 2, 0).cpu() for g in grads[:5]] + [g.cpu() for g in grads[5:]]
    names = SHADE_LEAVES + tuple(f"level {r}^2" for r in SHADE_LEVELS)
    worst = assert_shade_grads(f, names, got, f.ref[1], f.lit[1], tag)
    left, fewest, which = ep.coverage(f.cls)
    print(f"{tag}: worst forward / cap {fw:.2e}; gradients (cap 1e-4) " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; left out {left:.4f}, smallest class {fewest} pixels")
    env, chw, outs = run()
    g_levels = torch.autograd.grad(outs[1], env.specular, f.positive.to(gpu_device))
    assert_support(f, [g.cpu() for g in g_levels], tag)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", FRAMES)
def test_hip_shade_and_composite_in_every_border_and_vertex_cell(gpu_device, H, W):
    """shade_and_composite_surfel (the forward with the compositing, mrgs_surfel_shade_composite_backward: the other backward kernel)
    on the same probe frames: all five outputs and the gradients of base_color, the whole feature stack, normal_map, render_alpha and
    every level; then the exact support."""
    from materialrefgs_amd.shading import shade_and_composite_surfel
    f = shade_frame(H, W)
    camd = f.cam.to(gpu_device)
    hw = lambda t: t.permute(2, 0, 1)
    tag = f"composite {H}x{W}"
    feat = torch.cat([hw(f.refl), hw(f.rough), hw(f.albedo), f.indirect]).contiguous()

    def run():
        env = _shade_env(gpu_device, f)
        leaves = [t.contiguous().to(gpu_device).requires_grad_(True) for t in (f.base, feat, f.normal, hw(f.alpha))]
        render, diffuse, spec, extra = shade_and_composite_surfel(env, *leaves[:2], f.cam.HWK, camd.R, camd.T, *leaves[2:], BG.to(gpu_device), False)
        return env, leaves, (spec, extra["direct_light"], extra["specular_weight"], render, diffuse)
    env, leaves, outs = run()
    fw = max(capped(f"{tag} {n}", o.detach().cpu(), r, b, _fwd_cap(r), False) / _fwd_cap(r)
             for n, o, r, b in zip(("specular", "direct_light", "specular_weight", "render", "diffuse"), outs, f.ref[0], f.lit[0]))
    grads = torch.autograd.grad(outs, leaves + env.specular, [u.to(gpu_device) for u in f.ups])
    g_base, g_feat, g_normal, g_alpha = (g.cpu() for g in grads[:4])
    assert float(g_feat[5:8].abs().max()) == 0.0          # the indirect channels feed nothing without a tracer
    chw = lambda t: t.permute(1, 2, 0)
    got = [chw(g_feat[2:5]), g_normal, chw(g_alpha), chw(g_feat[0:1]), chw(g_feat[1:2]), g_base] + [g.cpu() for g in grads[4:]]
    names = SHADE_LEAVES + ("base",) + tuple(f"level {r}^2" for r in SHADE_LEVELS)
    worst = assert_shade_grads(f, names, got, f.ref[2], f.lit[2], tag)
    left, fewest, which = ep.coverage(f.cls)
    print(f"{tag}: worst forward / cap {fw:.2e}; gradients (cap 1e-4) " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; left out {left:.4f}, smallest class {fewest} pixels")
    env, leaves, outs = run()                             # (the node's texel buffers serve one backward)
    g_levels = torch.autograd.grad(outs[1], env.specular, f.positive.to(gpu_device))
    assert_support(f, [g.cpu() for g in g_levels], tag)


# ---- 4. the volume stage ------------------------------------------------------------------------------------------------------------------
# csrc/mrgs_volume.hip restates the taps for fp64 coordinates (dir_to_face_d, volume_taps, volume_fetch).  Rule and helpers are
# tests/test_volume_features.py's: err(native) <= 1.5 err(torch chain) + 1e-6 per tensor against tests/volume_statement.py in float64,
# rows under decision_margin 1e-4 left out of the per-row leaves only.
VOLUME_LEVELS, DIFFUSE_RES = (128, 64, 32, 16), 16
VOLUME_MIP_LEVELS = (-1.0, 0.5, 1.25, 1.5, 2.5, 2.8)     # -1: a roughness below min_roughness; no row on a knot (the roughness is a sigmoid)


def _quat_z_to(n, g):
    """Unit quaternions (w, x, y, z) whose rotation takes e_z to the unit vectors n [P,3], times a random turn about e_z in front
    (which leaves the third column where it is) and a random length."""
    q = torch.stack([1 + n[:, 2], -n[:, 1], n[:, 0], torch.zeros_like(n[:, 0])], 1)
    q = q / q.norm(dim=1, keepdim=True)
    phi = torch.rand(n.shape[0], generator=g, dtype=F64) * 6.28
    c, s = torch.cos(phi / 2), torch.sin(phi / 2)
    w, x, y, z = q.unbind(1)
    out = torch.stack([w * c - z * s, x * c + y * s, y * c - x * s, w * s + z * c], 1)
    return out * (0.5 + torch.rand(n.shape[0], 1, generator=g, dtype=F64))


def _unit_near(a, g, least):
    """Unit vectors b [P,3] with a . b > `least`, drawn around the unit vectors a (redrawn where the draw misses; b_z > -0.9)."""
    b = a.clone()
    todo = torch.ones(a.shape[0], dtype=torch.bool)
    for _ in range(64):
        if not bool(todo.any()):
            break
        cand = torch.nn.functional.normalize(a + 0.8 * torch.nn.functional.normalize(torch.randn(a.shape, generator=g, dtype=F64), dim=1), dim=1)
        ok = todo & ((cand * a).sum(1) > least) & (cand[:, 2] > -0.9)
        b[ok] = cand[ok]
        todo &= ~ok
    assert not bool(todo.any())
    return b


class VolumeCase:
    """The probe rows of the volume stage, built once on the CPU.  Set B: the mirror direction of the row hits a cell probe r of the
    128^2 specular level -- a facing normal n with n . r > 0.3, w_o = 2 (n . r) n - r, the centre on the ray from the camera along
    -w_o, the quaternion taking e_z to n.  Set A: the facing normal itself hits a cell probe of the 16^2 diffuse map, the centre
    placed so that n . w_o > 0.3 (the flip sign is unambiguous in both sets).  Row 0, whose LUT value every row shares, is an ordinary
    interior row."""

    def __init__(self):
        from materialrefgs_amd.shading import load_fg_lut
        from materialrefgs_amd.synthetic import orbit_camera
        from test_volume_features import VIEW, H, W, _rays_o
        g = torch.Generator().manual_seed(404)
        self.cam = cam = orbit_camera(VIEW, H, W)
        self.campos, self.rays_o = cam.camera_center.double(), _rays_o(cam, F64)
        n_lev = len(VOLUME_LEVELS)
        cyc = torch.tensor([0.04 if l < 0 else ep.level_roughness(l, n_lev) for l in VOLUME_MIP_LEVELS], dtype=F64)
        r = torch.nn.functional.normalize(ep.cell_probes(VOLUME_LEVELS[0], 6), dim=1).repeat_interleave(len(cyc), dim=0)       # set B
        n_b = _unit_near(r, g, 0.3)
        wo_b = 2 * (n_b * r).sum(1, keepdim=True) * n_b - r
        rough_b = cyc.repeat(r.shape[0] // len(cyc))
        n_a = torch.nn.functional.normalize(ep.cell_probes(DIFFUSE_RES, 6), dim=1).repeat_interleave(2, dim=0)                  # set A
        n_a = n_a[n_a[:, 2] > -0.9]
        wo_a = _unit_near(n_a, g, 0.3)
        rough_a = torch.rand(n_a.shape[0], generator=g, dtype=F64) * 0.8 + 0.1
        n0 = torch.nn.functional.normalize(torch.tensor([[0.3, -0.5, 0.8]], dtype=F64), dim=1)                                # row 0
        wo0 = torch.nn.functional.normalize(n0 + torch.tensor([[0.2, 0.1, -0.3]], dtype=F64), dim=1)
        n, wo = torch.cat([n0, n_b, n_a]), torch.cat([wo0, wo_b, wo_a])
        rough = torch.cat([torch.tensor([0.35], dtype=F64), rough_b, rough_a])
        self.P = P = n.shape[0]
        self.n_b = n_b.shape[0]
        xyz = self.rays_o - (2.0 + 3.0 * torch.rand(P, 1, generator=g, dtype=F64)) * wo
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)
        raw = [xyz, rnd(P, 2) * 0.3 - 3.0, _quat_z_to(n, g), rnd(P, 1), rnd(P, 1), torch.log(rough / (1 - rough)).unsqueeze(1), rnd(P, 3)]
        self.raw32 = [t.float() for t in raw]
        self.spec32 = random_levels(VOLUME_LEVELS, 4040)
        self.diffuse32 = random_levels((DIFFUSE_RES,), 4041)[0]
        self.lut = load_fg_lut("cpu").double()
        self.raw_o = [t.double().requires_grad_(True) for t in self.raw32]
        self.spec_o = [t.double().requires_grad_(True) for t in self.spec32]
        self.diffuse_o = self.diffuse32.double().requires_grad_(True)
        detached = [t.detach() for t in self.raw_o]
        self.margin = vs.decision_margin(detached, self.campos, self.rays_o, self.lut, self.spec32, self.diffuse32)
        self.normal, _, self.mirror, _ = vs._geometry(detached[0], detached[2], self.campos, self.rays_o)
        self.rough = torch.sigmoid(detached[5]).reshape(-1)
        self.target_b, self.target_a = r, n_a



@functools.lru_cache(maxsize=None)
def volume_case():
    return VolumeCase()


def _volume_classes(c):
    from test_volume_features import MARGIN
    spec = ep.classify(VOLUME_LEVELS, c.mirror, c.rough)
    diff = ep.classify((DIFFUSE_RES,), c.normal, None)
    for cls in (spec, diff):
        cls["keep"] = c.margin >= MARGIN
    return spec, diff


def test_volume_probe_rows_cover_every_class_with_margin():
    """The conditions of part 4: about 2 300 rows (more than one 256-row workgroup: the privatised copies are in use), the realised
    mirror directions (set B) and facing normals (set A) on their targets, at most 1 % of the rows under the decision margin, and >= 4
    kept rows in every border and vertex class of the four specular levels and of the diffuse map."""
    c = volume_case()
    off_b = float((c.mirror[1:1 + c.n_b] - c.target_b).norm(dim=1).max())
    off_a = float((c.normal[1 + c.n_b:] - c.target_a).norm(dim=1).max())
    spec, diff = _volume_classes(c)
    left, fewest_s, which_s = ep.coverage(spec)
    _, fewest_d, which_d = ep.coverage(diff)
    print(f"volume rows: P={c.P}, set B within {off_b:.1e} / set A within {off_a:.1e} of their targets, under the margin {left:.4f}, "
          f"smallest specular class {fewest_s} rows {which_s}, smallest diffuse class {fewest_d} rows {which_d}")
    assert 2200 <= c.P <= 2400 and max(off_a, off_b) <= 4e-6
    assert left <= MAX_LEFT_OUT and fewest_s >= MIN_CLASS_ROWS and fewest_d >= MIN_CLASS_ROWS
    assert len(spec["classes"]) == 4 * 48 and len(diff["classes"]) == 48


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["2dgs", "pgsr"])
def test_hip_volume_features_in_every_border_and_vertex_cell(gpu_device, flag):
    from materialrefgs_amd.renderer import SurfelModel
    from materialrefgs_amd.shading import EnvLight, _VolumeFeatures, load_fg_lut
    from test_volume_features import MARGIN, OUT_NAMES, PER_ROW, _assert_rule, _err, _leaf_grads, _upstreams
    dev, c = gpu_device, volume_case()
    cam_d = c.cam.to(dev)
    vm64 = c.cam.world_view_transform.double() if flag != "2dgs" else None
    ref = vs.volume_statement(c.raw_o, c.campos, c.rays_o, c.lut, c.spec_o, c.diffuse_o, viewmatrix=vm64)
    raw_h = [t.to(dev).requires_grad_(True) for t in c.raw32]
    env = EnvLight(device=dev, min_res=DIFFUSE_RES, max_res=DIFFUSE_RES)          # (its own chain is replaced by the random levels)
    env.specular = [t.to(dev).requires_grad_(True) for t in c.spec32]
    env._diffuse = c.diffuse32.to(dev).requires_grad_(True)
    pc_h = SurfelModel(*raw_h[:4], torch.zeros(c.P, 1, 3, device=dev), torch.zeros(c.P, 15, 3, device=dev), refl_strength=raw_h[4],
                       roughness=raw_h[5], ori_color=raw_h[6])
    pc_h.env_map_2 = env
    nat = _VolumeFeatures.apply(*raw_h, cam_d.camera_center, c.rays_o.float().to(dev), load_fg_lut(dev),
                                cam_d.world_view_transform if flag != "2dgs" else None, env.min_roughness, env.max_roughness, True,
                                env.diffuse, *env.specular)
    tor = vs.torch_chain(pc_h, cam_d, flag)
    label = f"volume probes {flag}"
    _assert_rule([(n, _err(a, r), _err(b, r)) for n, a, b, r in zip(OUT_NAMES, nat, tor, ref)], f"{label} forward")
    keep = c.margin >= MARGIN
    up = _upstreams(c.P, ref[4].shape[1])
    leaves_o = c.raw_o + c.spec_o + [c.diffuse_o]
    leaves_h = raw_h + env.specular + [env.diffuse]
    names = vs.RAW_NAMES + tuple(f"specular {r}^2" for r in VOLUME_LEVELS) + ("diffuse map",)
    used = (1, 1, 1, 1, 1)
    g_ref = _leaf_grads(ref, up, used, c.raw_o[0], up[5], leaves_o)
    g_nat = _leaf_grads(nat[:5], up, used, nat[5], up[5], leaves_h)
    g_tor = _leaf_grads(tor, up, used, raw_h[0], up[5], leaves_h)
    rows = [(n, _err(a, r, keep if n in PER_ROW else None), _err(b, r, keep if n in PER_ROW else None))
            for n, a, b, r in zip(names, g_nat, g_tor, g_ref)]
    _assert_rule(rows, f"{label} gradients")
    spec, diff = _volume_classes(c)
    print(f"{label}: P={c.P}, worst native error {max(r[1] for r in rows):.2e} ({max(rows, key=lambda r: r[1])[0]}), under the margin "
          f"{ep.coverage(spec)[0]:.4f}, smallest class {min(ep.coverage(spec)[1], ep.coverage(diff)[1])} rows")
