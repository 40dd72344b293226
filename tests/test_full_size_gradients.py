"""Full-size gradients against float64 (-m gpu): the two backward kernels that add per-primitive gradients across many rays or pixels through
LDS tables and atomics, at the sizes where that machinery switches on.

A. The surfel tracer's backward (csrc/mrgs_surfel_trace.hip: replay of the forward's record, same-surfel lane merge, lone rays four to a
   wave or in their block's wave, the walk again without a record) against autograd of the dense statement restricted to each chunk's
   candidates (oracle/surfel_trace_oracle.trace_dense_restricted), float64 on the GPU: a 40 000-surfel view with upstream on every ray,
   C3trace (300 000 surfels, 800 x 800) and C4trace (1 000 000, 1600 x 1600) with upstream on whole 8 x 8 blocks and on rays stratified by
   the path the forward took, and the production record path (HardwareRendering.render_gaussians -> mrgs_surfel_trace_prep_raw_*) against
   GaussianModel's activations + eval_sh + the dense statement.  The walk again (MRGS_TRACE_NO_RECORD, read once per process) runs the
   first two in a child process.
B. The fused shading backward shade_fused_bwd_kernel<false / true> (csrc/mrgs_shade.hip on the fetch of csrc/mrgs_envmap.h: dense LDS levels, the 4 096-entry hash table, its
   mid-loop flush and 8-probe global fallback) at 800^2 and 1600^2 on the 128 -> 16 chain with every level a leaf, against
   oracle/shading_oracle.specular_color_surfel in float64 on the GPU; a host model of the tile schedule proves that the hash paths run.
"""
import os
import re
import subprocess
import sys
import time
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import surfel_trace_oracle as sto  # noqa: E402
from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera  # noqa: E402
from oracle import render_oracle  # noqa: E402
from oracle import shading_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu
PIPE = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
NO_RECORD = os.environ.get("MRGS_TRACE_NO_RECORD") is not None
OUT_C = {"rgb": 3, "dpt": 1, "acc": 1, "norm": 3, "dist": 1, "aux": 2}
TRACE_LEAVES = ("means", "scales", "rotations", "opacities", "colors", "others", "o", "d")


# ---- A. tracer backward ----------------------------------------------------------------------------------------------------------

def _mirror_view(P, H, W, dev):
    """make_surfel_model's scene, view 0 rendered by render_surfel, and the mirror rays of every pixel as [H,W,3] (so that the tracer forms
    its 8 x 8 packets as in render_surfel_with_envgs)."""
    from materialrefgs_amd.gs_utils import safe_normalize
    from materialrefgs_amd.renderer import _mirror_rays, render_surfel
    pc, env, _ = make_surfel_model(P, max(H, W), dev)
    cam = orbit_camera(0, H, W).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        env.build_mips()
        out = render_surfel(cam, pc, PIPE, bg, srgb=False, opt=SimpleNamespace(indirect=False))
        nmap = safe_normalize(out["rend_normal"].permute(1, 2, 0) / out["rend_alpha"].permute(1, 2, 0).clamp_min(1e-6))
        ro, rd = _mirror_rays(cam, nmap, out["surf_depth"])
    return pc, cam, bg, ro.detach().reshape(H, W, 3).contiguous(), rd.detach().reshape(H, W, 3).contiguous()


def _trace_getters(dev, L, bg, H, W):
    from materialrefgs_amd.surfel_tracing import SurfelTracer, SurfelTracingSettings
    tr = SurfelTracer()
    v = sto.quad_vertices(L["means"].detach(), L["scales"].detach(), L["rotations"].detach()).reshape(-1, 3)
    tr.build_acceleration_structure(v, None)
    eye = torch.eye(4, device=dev)
    ts = SurfelTracingSettings(H, W, 1.0, 1.0, bg, 1.0, eye, eye, 0, torch.zeros(3, device=dev), False, False)
    rgb, dpt, acc, norm, dist, aux, _mid, _wet = tr(L["o"], L["d"], v, means3D=L["means"], grads3D=None, shs=None, colors_precomp=L["colors"],
                                                   others_precomp=L["others"], opacities=L["opacities"], scales=L["scales"],
                                                   rotations=L["rotations"], cov3D_precomp=None, tracer_settings=ts)
    n = H * W
    outs = dict(rgb=rgb.reshape(n, 3), dpt=dpt.reshape(n), acc=acc.reshape(n), norm=norm.reshape(n, 3), dist=dist.reshape(n), aux=aux.reshape(n, 2))
    return outs, tr


PATHS = ("packet, one pass", "packet, several passes", "alone, one pass", "alone, several passes", "no hit")


def _paths(state):
    """The path every ray took in the forward (SurfelTracer.last_state: word 2 = hits blended, word 3 = passes, negative in a packet)."""
    hits, passes = state[:, 2], state[:, 3]
    none = hits == 0
    return {PATHS[0]: (passes < 0) & (passes.abs() <= 1) & ~none, PATHS[1]: (passes < 0) & (passes.abs() > 1) & ~none,
            PATHS[2]: (passes > 0) & (passes <= 1) & ~none, PATHS[3]: (passes > 1) & ~none, PATHS[4]: none}


def _sample(state, H, W, n_blocks, per_path, seed):
    """Whole 8 x 8 blocks + up to `per_path` scattered rays of every path; returns (sorted ray indices, {path: (population, sampled)})."""
    g = torch.Generator().manual_seed(seed)
    dev = state.device
    bx, by = W // 8, H // 8
    blocks = torch.randperm(bx * by, generator=g)[:n_blocks]
    yy, xx = torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")
    rows = [((b // bx) * 8 + yy) * W + (b % bx) * 8 + xx for b in blocks.tolist()]
    idx = [torch.cat([r.reshape(-1) for r in rows])] if rows else []
    counts = {}
    for name, m in _paths(state).items():
        pop = torch.nonzero(m).reshape(-1).cpu()
        take = pop[torch.randperm(pop.numel(), generator=g)[:per_path]]
        idx.append(take)
        counts[name] = [int(pop.numel()), int(take.numel())]
    idx = torch.unique(torch.cat(idx)).to(dev)
    for name, m in _paths(state).items():
        counts[name][1] = int(m[idx].sum())
    return idx, counts


def _decision_band(hip, ref, hits_hip, idx):
    """The `same` mask of test_surfel_tracing.py: a ray whose fp32 decision at a threshold differs from float64 leaves the loss."""
    same = hits_hip[idx].double() == ref["hits"].double()
    for k in OUT_C:
        a = hip[k].detach()[idx].double()
        err = (a - ref[k]).abs().reshape(idx.numel(), -1).max(dim=1).values
        same &= err <= 2e-4 * max(1.0, float(ref[k].abs().max()))          # NaN counts as a mismatch
    return same


def _upstream(n, idx, keep, seed, dev):
    """Random upstream of all six outputs on the sampled rays that stay in the loss, exact zeros elsewhere: ({k: [n,c] fp32},
    {k: [len(idx),c] float64})."""
    g = torch.Generator().manual_seed(seed)
    full, samp = {}, {}
    m = keep.double()
    for k, c in OUT_C.items():
        u = torch.randn(idx.numel(), c, generator=g).to(idx.device, torch.float64) * m[:, None]
        f = torch.zeros(n, c, dtype=torch.float32, device=idx.device)
        f[idx] = u.float()
        full[k], samp[k] = f.squeeze(-1) if c == 1 else f, u.squeeze(-1) if c == 1 else u
    return full, samp


def _report(tag, hip, ref, names, lit32_fn, bar):
    """render_oracle.leaf_gradient_report with the literal fp32 leg evaluated only when a leaf is above the bar."""
    rows, ok = render_oracle.leaf_gradient_report(hip, ref, names, bar=bar)
    if not ok:
        ref = dict(ref, lit32=lit32_fn())
        rows, ok = render_oracle.leaf_gradient_report(hip, ref, names, bar=bar)
    for n in names:
        r_ = rows[n]
        print(f"  [{tag}] grad {n:14s} {r_['err']:.2e}  {r_['rule']}" + (f" (fp32 dense: {r_['lit32_err']:.2e})" if "lit32_err" in r_ else ""))
    return rows, ok


def _tier(dev, P, H, W, sample, seed, chunk):
    """One tracer tier through SurfelTracer with leaves for every input.  sample: None (upstream on every ray) or (blocks, per_path)."""
    t0 = time.time()
    pc, cam, bg, ro, rd = _mirror_view(P, H, W, dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        base = dict(means=pc.get_xyz, scales=pc.get_scaling, rotations=pc.get_rotation, opacities=pc.get_opacity,
                    colors=torch.rand(P, 3, generator=g).to(dev), others=torch.rand(P, 2, generator=g).to(dev), o=ro, d=rd)
    L = {k: v.detach().float().contiguous().clone().requires_grad_(True) for k, v in base.items()}
    hip, tr = _trace_getters(dev, L, bg, H, W)
    n = H * W
    state = tr.last_state.clone()
    from materialrefgs_amd.surfel_tracing import record_summary
    rs = record_summary(tr)
    assert rs["rays"] == n and rs["record_usable"] == (not NO_RECORD), rs
    if sample is None:
        idx, counts = torch.arange(n, device=dev), {k: [int(m.sum())] * 2 for k, m in _paths(state).items()}
    else:
        idx, counts = _sample(state, H, W, sample[0], sample[1], seed)
    for name, (pop, got) in counts.items():
        assert pop == 0 or got > 0, (name, counts)
    assert counts[PATHS[0]][1] > 0 and counts[PATHS[4]][1] > 0, counts
    f64 = {k: v.detach().double() for k, v in L.items()}
    surf = [f64[k] for k in sto.LEAVES]
    o64, d64 = f64["o"].reshape(n, 3)[idx], f64["d"].reshape(n, 3)[idx]
    ref, _, _ = sto.trace_dense_restricted(o64, d64, *surf, bg.double(), chunk=chunk)
    keep = _decision_band(hip, ref, state[:, 2], idx)
    removed = int((~keep).sum())
    assert removed <= idx.numel() // 200, (removed, idx.numel())
    up_full, up_s = _upstream(n, idx, keep, seed + 1, dev)
    torch.autograd.backward([hip[k] for k in OUT_C], [up_full[k] for k in OUT_C])
    _, gref, cand = sto.trace_dense_restricted(o64, d64, *surf, bg.double(), up=up_s, chunk=chunk)
    got = {k: L[k].grad.detach() for k in sto.LEAVES}
    got["o"], got["d"] = L["o"].grad.reshape(n, 3)[idx], L["d"].grad.reshape(n, 3)[idx]

    def lit32():
        _, g32, _ = sto.trace_dense_restricted(o64.float(), d64.float(), *[t.float() for t in surf], bg.float(),
                                               up={k: v.float() for k, v in up_s.items()}, chunk=chunk)
        return {k: v.double().cpu().numpy() for k, v in g32.items()}

    tag = f"P={P} {H}x{W}"
    rows, ok = _report(tag, {k: v.double().cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in gref.items()},
                       list(TRACE_LEAVES), lit32, 3e-4)
    # cross-talk: a surfel no kept ray can hit and a ray without upstream receive exact zeros
    zero_rows = {k: float(L[k].grad[~cand].abs().max()) if bool((~cand).any()) else 0.0 for k in sto.LEAVES}
    silent = torch.ones(n, dtype=torch.bool, device=dev)
    silent[idx[keep]] = False
    zero_rays = max(float(L[k].grad.reshape(n, 3)[silent].abs().max()) for k in ("o", "d")) if bool(silent.any()) else 0.0
    print(f"  [{tag}] rays in the loss {int(keep.sum())} of {n}, removed by the decision band {removed} ({removed / idx.numel():.1e}), "
          f"candidate surfels {int(cand.sum())} of {P}; paths (population, sampled): {counts}; record usable {rs['record_usable']}; "
          f"{time.time() - t0:.1f} s")
    assert ok, rows
    assert max(zero_rows.values()) == 0.0, zero_rows
    assert zero_rays == 0.0, zero_rays
    for k in TRACE_LEAVES:
        assert bool(torch.isfinite(L[k].grad).all()), k


def test_tracer_backward_tier1_every_ray(gpu_device):
    """40 000 surfels, 256 x 256 mirror rays, upstream on every ray."""
    _tier(gpu_device, 40_000, 256, 256, None, 21, chunk=512)


@pytest.mark.parametrize("P,H,W,blocks,per_path,chunk", [(300_000, 800, 800, 8, 200, 128), (1_000_000, 1600, 1600, 4, 100, 64)],
                         ids=["c3trace", "c4trace"])
def test_tracer_backward_full_size(gpu_device, P, H, W, blocks, per_path, chunk):
    """C3trace / C4trace: whole 8 x 8 blocks and rays stratified by path, zero upstream elsewhere."""
    _tier(gpu_device, P, H, W, (blocks, per_path), 31, chunk)


def test_tracer_backward_production_record_path(gpu_device):
    """HardwareRendering.render_gaussians at C3trace size from the model's raw leaves (_PrepRaw -> mrgs_surfel_trace_prep_raw_*) against the
    float64 chain: GaussianModel's activations, eval_sh from camera_center, the restricted dense statement."""
    from materialrefgs_amd.gs_utils import eval_sh
    from materialrefgs_amd.surfel_tracing import HardwareRendering
    t0 = time.time()
    dev = gpu_device
    P, H, W, chunk = 300_000, 800, 800, 128
    pc, cam, bg, ro, rd = _mirror_view(P, H, W, dev)
    raw_names = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
    for nm in raw_names:
        getattr(pc, nm).grad = None
    hw = HardwareRendering().train()
    out = hw.render_gaussians(cam, ro, rd, pc, PIPE, bg)
    n = H * W
    col = lambda x, c: x.permute(1, 2, 0).reshape(n, c) if c > 1 else x.reshape(n)
    hip = dict(rgb=col(out["render"], 3), dpt=col(out["surf_depth"], 1), acc=col(out["rend_alpha"], 1), norm=col(out["rend_normal"], 3),
               dist=col(out["rend_dist"], 1), aux=torch.cat([out["specular"], out["roughness"]], 0).permute(1, 2, 0).reshape(n, 2))
    state = hw.tracer.last_state.clone()
    idx, counts = _sample(state, H, W, 8, 200, 41)

    def chain(dt, need_grad):
        raw = {nm: getattr(pc, nm).detach().to(dt).clone().requires_grad_(need_grad) for nm in raw_names}
        shs = torch.cat([raw["_features_dc"], raw["_features_rest"]], dim=1)
        dirs = raw["_xyz"] - cam.camera_center.to(dt).reshape(1, 3)
        colors = torch.clamp_min(eval_sh(pc.active_sh_degree, shs.transpose(1, 2), dirs / dirs.norm(dim=1, keepdim=True)) + 0.5, 0.0)
        act = [raw["_xyz"], torch.exp(raw["_scaling"]), torch.nn.functional.normalize(raw["_rotation"]), torch.sigmoid(raw["_opacity"]), colors,
               torch.full((P, 2), 0.01, dtype=dt, device=dev)]
        return raw, act

    raw64, act64 = chain(torch.float64, True)
    o64, d64 = ro.reshape(n, 3)[idx].double(), rd.reshape(n, 3)[idx].double()
    ref, _, _ = sto.trace_dense_restricted(o64, d64, *[a.detach() for a in act64], bg.double(), chunk=chunk)
    keep = _decision_band(hip, ref, state[:, 2], idx)
    removed = int((~keep).sum())
    assert removed <= idx.numel() // 200, (removed, idx.numel())
    up_full, up_s = _upstream(n, idx, keep, 43, dev)
    torch.autograd.backward([hip[k] for k in OUT_C], [up_full[k] for k in OUT_C])
    _, gref, cand = sto.trace_dense_restricted(o64, d64, *[a.detach() for a in act64], bg.double(), up=up_s, chunk=chunk)
    torch.autograd.backward(act64[:5], [gref[k] for k in sto.LEAVES[:5]])
    names = [nm[1:] for nm in raw_names]
    got = {nm[1:]: getattr(pc, nm).grad.detach().double().cpu().numpy() for nm in raw_names}
    want = {nm[1:]: raw64[nm].grad.cpu().numpy() for nm in raw_names}

    def lit32():
        raw32, act32 = chain(torch.float32, True)
        _, g32, _ = sto.trace_dense_restricted(o64.float(), d64.float(), *[a.detach() for a in act32], bg.float(),
                                               up={k: v.float() for k, v in up_s.items()}, chunk=chunk)
        torch.autograd.backward(act32[:5], [g32[k] for k in sto.LEAVES[:5]])
        return {nm[1:]: raw32[nm].grad.double().cpu().numpy() for nm in raw_names}

    rows, ok = _report("render_gaussians C3", got, want, names, lit32, 3e-4)
    zero = max(float(getattr(pc, nm).grad[~cand].abs().max()) for nm in raw_names) if bool((~cand).any()) else 0.0
    print(f"  [render_gaussians C3] rays in the loss {int(keep.sum())}, removed {removed} ({removed / idx.numel():.1e}), candidates "
          f"{int(cand.sum())} of {P}; paths {counts}; {time.time() - t0:.1f} s")
    assert ok, rows
    assert zero == 0.0, zero


@pytest.mark.skipif(NO_RECORD, reason="this is the parent of the walk-again run")
def test_tracer_backward_walks_again_at_full_size(gpu_device):
    """MRGS_TRACE_NO_RECORD (read once per process): the backward walks the hierarchy again instead of replaying the record -- at full size
    the record is always usable, so only this switch takes a full-size scene down that path.  Tier 1 and C3trace in a child process."""
    t0 = time.time()
    env = dict(os.environ, MRGS_TRACE_NO_RECORD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-p", "no:cacheprovider",
                        "-k", "tier1_every_ray or c3trace"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("  [")))
    print(f"  [walk again] {time.time() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert re.search(r"\b2 passed", r.stdout), r.stdout[-1000:]


# ---- B. fused shading backward ------------------------------------------------------------------------------------------------------

LEVELS = (128, 64, 32, 16)
LDS_FLOATS = 23552          # MRGS_SHADE_LDS_FLOATS: the levels that fit, coarsest first, accumulate in a dense LDS copy


def _hashed_levels():
    dense, used = set(), 0
    for li in range(len(LEVELS) - 1, -1, -1):
        n = 6 * LEVELS[li] ** 2 * 3
        if used + n > LDS_FLOATS:
            break
        dense.add(li)
        used += n
    return [li for li in range(len(LEVELS)) if li not in dense]


def _smooth(g, H, W, c, cells):
    """A smooth random field [H,W,c]: Gaussian noise on a coarse grid, bicubic upsampling."""
    coarse = torch.randn(1, c, cells, cells, generator=g, dtype=torch.float64)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)


def _shading_maps(H, W, kind, seed):
    """[H,W,c] float64 maps: albedo, normal, alpha, refl, roughness.  coherent: smooth normals and roughness patches; adversarial: i.i.d.
    normals, roughness mostly below 0.29 (both taps in the hashed levels 128 and 64)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    albedo, alpha, refl = u(H, W, 3), 0.05 + 0.95 * u(H, W, 1), u(H, W, 1)
    if kind == "coherent":
        normal = torch.nn.functional.normalize(_smooth(g, H, W, 3, 12) + torch.tensor([0.0, 0.0, -0.5], dtype=torch.float64), dim=-1)
        rough = 0.02 + 0.96 * torch.sigmoid(2.0 * _smooth(g, H, W, 1, 20))
    else:
        normal = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g, dtype=torch.float64), dim=-1)
        low = u(H, W, 1) < 0.9
        rough = torch.where(low, 0.29 * u(H, W, 1), 0.29 + 0.7 * u(H, W, 1))
    return albedo, normal, alpha, refl, rough


@pytest.mark.parametrize("composite", [False, True], ids=["specular", "composite"])
@pytest.mark.parametrize("kind", ["coherent", "adversarial"])
@pytest.mark.parametrize("size", [800, 1600])
def test_fused_shading_backward_at_production_sizes(gpu_device, size, kind, composite):
    """get_specular_color_surfel (shade_fused_bwd_kernel<false>) and render_surfel's shade-and-composite node (<true>,
    mrgs_surfel_shade_composite_backward) against specular_color_surfel in float64 on the GPU.  Every cubemap level is a leaf.  Bars of
    test_shading.py: 1e-4 of the maximum per leaf and per level; per-pixel gradients away from the pixels whose taps sit within 1e-5 of a
    cell, level or face decision (where the exact derivative jumps), texel gradients everywhere."""
    from materialrefgs_amd.shading import EnvLight, get_specular_color_surfel, load_fg_lut, shade_and_composite_surfel
    t0 = time.time()
    dev = gpu_device
    H = W = size
    cam = orbit_camera(1, H, W)
    camd = cam.to(dev)
    K = cam.HWK[2]
    seed = 5 + size + (0 if kind == "coherent" else 1)
    r32 = lambda t: t.float().double().to(dev)            # both sides read the same (fp32-exact) inputs
    maps = [r32(m) for m in _shading_maps(H, W, kind, seed)]
    g = torch.Generator().manual_seed(seed + 100)
    levels0 = [r32(torch.randn(6, r, r, 3, generator=g, dtype=torch.float64)) for r in LEVELS]
    lut = load_fg_lut(dev)
    # ---- where the pixels fetch: the schedule model proves the hash table's fallback and mid-loop flush run
    taps = so.shade_taps(LEVELS, H, W, K, cam.R, cam.T, maps[1], maps[4])
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    sched = so.fused_bwd_schedule(taps["keys"], H, W, n_cu, _hashed_levels())
    print(f"\n  [shade {size}^2 {kind}] tiles {sched['ntiles']} on {sched['grid']} workgroups ({sched['tiles_per_wg']} per workgroup); "
          f"distinct hashed keys per 4-tile window <= {sched['max_window_keys']}, windows beyond the table {sched['windows_over_table']}; "
          f"workgroup 0 replayed: {sched['sim'][0]}")
    if kind == "adversarial":
        assert sched["windows_over_table"] > 0 and sched["sim"][0]["fallbacks"] > 0, sched
        if size == 1600:
            assert sched["sim"][0]["mid_flushes"] > 0, sched
    # ---- pixels at a discontinuity of the per-pixel derivative
    dist = lambda x: (x - torch.round(x)).abs()
    lres = lut.shape[0]
    luv = taps["lut_uv"] * lres - 0.5
    rough = maps[4].reshape(-1)
    # (fp32 rounds the kernel's texel coordinates in proportion to their size -- one ulp of fx in [64, 128) is 7.6e-6 texel, and fx / fy
    #  reach the kernel through a reflection and a face projection: the band is 4e-7 of the level's width, 5.1e-5 texel at 128^2; the LUT's
    #  u = NdotV likewise, 6e-5 of a cell at 256; the mip level's fraction and NdotV's clamps are well resolved at 1e-5)
    parts = {"tap": (taps["cell_edge"] < 4e-7) | (taps["level_edge"] < 1e-5) | (taps["face_gap"] < 1e-5),
             "lut": (taps["ndv"].abs() < 1e-5) | ((taps["ndv"] - 1).abs() < 1e-5) | (dist(luv[:, 0]) < 6e-5) | (dist(luv[:, 1]) < 1e-5),
             "clamp": ((rough - 0.08).abs() < 1e-6) | ((rough - 0.5).abs() < 1e-6)}
    near = (parts["tap"] | parts["lut"] | parts["clamp"]).reshape(H, W)
    frac = float(near.double().mean())
    print("  excluded: " + ", ".join(f"{k} {float(v.double().mean()):.1e}" for k, v in parts.items()))
    # ---- float64 statement
    lv64 = [t.clone().requires_grad_(True) for t in levels0]
    m64 = [t.clone().requires_grad_(True) for t in maps]
    gen = torch.Generator().manual_seed(seed + 200)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dev)
    if composite:
        base64 = r32(torch.rand(3, H, W, generator=gen, dtype=torch.float64)).requires_grad_(True)
        bg = torch.tensor([0.2, 0.4, 0.6], dtype=torch.float64, device=dev)
        ups = dict(render=rnd(3, H, W), diffuse=rnd(3, H, W), spec=rnd(3, H, W), direct=rnd(3, H, W), weight=rnd(H, W, 3))
    else:
        ups = dict(spec=rnd(3, H, W), direct=rnd(3, H, W), weight=rnd(H, W, 3))
    spec_o, direct_o, weight_o = so.specular_color_surfel(lv64, lut.double(), m64[0], H, W, K, cam.R, cam.T, m64[1], m64[2], m64[3], m64[4])
    outs_o = dict(spec=spec_o, direct=direct_o, weight=weight_o)
    if composite:
        outs_o["diffuse"] = (1 - m64[3].permute(2, 0, 1)) * base64
        outs_o["render"] = outs_o["diffuse"] + spec_o + bg[:, None, None] * (1 - m64[2].permute(2, 0, 1))
    torch.autograd.backward([outs_o[k] for k in ups], [ups[k] for k in ups])
    # ---- HIP
    env = EnvLight(device=dev, min_res=16, max_res=128, trainable=True)
    lvh = [t.float().contiguous().requires_grad_(True) for t in levels0]
    env.specular = lvh
    if composite:
        # features [8,H,W] = (refl, roughness, albedo, indirect), channel-first as the rasterizer writes them
        feat = torch.cat([maps[3], maps[4], maps[0], torch.zeros(H, W, 3, dtype=torch.float64, device=dev)], -1).permute(2, 0, 1).float().contiguous()
        feat.requires_grad_(True)
        nmap = maps[1].float().contiguous().requires_grad_(True)
        alpha = maps[2].permute(2, 0, 1).float().contiguous().requires_grad_(True)
        baseh = base64.detach().float().requires_grad_(True)
        render, diffuse, spec, extra = shade_and_composite_surfel(env, baseh, feat, cam.HWK, camd.R, camd.T, nmap, alpha, bg.float(), False, fg_lut=lut)
        outs_h = dict(render=render, diffuse=diffuse, spec=spec, direct=extra["direct_light"], weight=extra["specular_weight"])
    else:
        chw = [m.permute(2, 0, 1).float().contiguous().requires_grad_(True) for m in maps]
        hwc = [t.permute(1, 2, 0) for t in chw]
        spec, extra = get_specular_color_surfel(env, hwc[0], cam.HWK, camd.R, camd.T, hwc[1], hwc[2], refl_strength=hwc[3], roughness=hwc[4], fg_lut=lut)
        outs_h = dict(spec=spec, direct=extra["direct_light"], weight=extra["specular_weight"])
    torch.autograd.backward([outs_h[k] for k in ups], [ups[k].float() for k in ups])
    torch.cuda.synchronize(dev)
    # ---- per-pixel leaves ([H,W,c] on both sides)
    if composite:
        pix = {"base": (baseh.grad.permute(1, 2, 0), base64.grad.permute(1, 2, 0)), "normal": (nmap.grad, m64[1].grad),
               "alpha": (alpha.grad.permute(1, 2, 0), m64[2].grad),
               "features": (feat.grad.permute(1, 2, 0),
                            torch.cat([m64[3].grad, m64[4].grad, m64[0].grad, torch.zeros(H, W, 3, dtype=torch.float64, device=dev)], -1))}
    else:
        pix = {n_: (t.grad.permute(1, 2, 0), m.grad) for n_, t, m in zip(("albedo", "normal", "alpha", "refl", "rough"), chw, m64)}
    fails = []
    for n_, (a, b) in pix.items():
        scale = float(b.abs().max())
        err = (a.double() - b).abs()
        e_all = float(err.max()) / scale
        e = float(err[~near].max()) / scale
        print(f"  [shade {size}^2 {kind} {'composite' if composite else 'specular'}] grad {n_:9s} {e:.2e} (all pixels {e_all:.2e})")
        if not e <= 1e-4:
            badp = torch.nonzero((err.amax(dim=-1) > 1e-4 * scale) & ~near).reshape(-1, 2)[:8]
            for y_, x_ in badp.tolist():
                q = y_ * W + x_
                print(f"    pixel ({y_},{x_}) err {float(err[y_, x_].max()) / scale:.1e} cell edge {float(taps['cell_edge'][q]):.1e} face_gap "
                      f"{float(taps['face_gap'][q]):.1e} lut {[round(float(v), 6) for v in luv[q]]} level {float(taps['level'][q]):.6f}")
            fails.append((n_, e))
    for li, (a, b) in enumerate(zip(lvh, lv64)):
        scale = float(b.grad.abs().max())
        e = float((a.grad.double() - b.grad).abs().max()) / scale
        print(f"  [shade {size}^2 {kind} {'composite' if composite else 'specular'}] level {LEVELS[li]:3d}^2 {e:.2e}"
              f"{' (hashed)' if li in _hashed_levels() else ' (dense LDS)'}")
        if not e <= 1e-4:
            fails.append((f"level {LEVELS[li]}", e))
    print(f"  [shade {size}^2 {kind}] pixels excluded near a discontinuity {frac:.1e}; {time.time() - t0:.1f} s")
    assert not fails, fails
    assert frac < 1e-3, frac
