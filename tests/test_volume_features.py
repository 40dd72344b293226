"""shading.volume_features -- render_volume's per-gaussian stage as HIP kernels (csrc/mrgs_volume.hip) -- against its float64 statement
(tests/volume_statement.py), beside the chain of torch ops it replaces.

The rule is the truth-leg rule of DESIGN section 3 with its 1.5x margin: per tensor, in the max-norm relative to the statement,
err(native) <= 1.5 err(torch chain) + 1e-6, both legs on the same inputs in the same test; the 1e-6 floor is the fp32 rounding of the
inputs.  Rows whose decision margin (volume_statement.decision_margin) is under 1e-4 are left out of the per-row leaves (xyz, rotation,
roughness) only -- a float32 leg may take a texel cell, a mip slope or a facing sign the other way there, which moves those gradients
by O(1) -- never out of env.base, the other leaves or the forward values, which are continuous across those decisions.  The CPU part
checks that such rows are at most 1 % for every scene the GPU part uses: a condition of the comparison, not a tolerance of it."""
import functools
from types import SimpleNamespace

import pytest
import torch

import volume_statement as vs
from test_render_e2e import _models
from materialrefgs_amd.synthetic import orbit_camera

H, W = 96, 128
VIEW = 1
# (P, seed): a lone row 0, a partial wave, a full wave, a wave + 1, a workgroup + 1, several workgroups; the whole render's scene
CASES = ((1, 11), (63, 11), (64, 11), (65, 12), (257, 13), (1000, 14))
RENDER_CASE = (3000, 2)
MARGIN = 1e-4
PER_ROW = ("xyz", "rotation", "roughness")
RAW_ATTRS = ("_xyz", "_scaling", "_rotation", "_opacity", "_refl_strength", "_roughness", "_ori_color")
OUT_NAMES = ("opacity", "scales", "rotations", "colors_precomp", "features")


def _rays_o(cam, dt):
    Rt = cam.R.to(dt).T
    return (-Rt.T @ cam.T.to(dt).unsqueeze(-1)).flatten()


@functools.lru_cache(maxsize=None)
def _scene(P, seed):
    """CPU side of a case, built once: float64 leaves, the float64 chain of the environment, the camera, the rows under the margin."""
    from oracle.render_oracle import _OracleBuildMips
    from materialrefgs_amd.shading import load_fg_lut
    pc_o, base_o, _, _ = _models(P, H, W, seed)
    cam = orbit_camera(VIEW, H, W)
    raw_o = [getattr(pc_o, n) for n in RAW_ATTRS]
    *spec, diffuse = _OracleBuildMips.apply(base_o, 8, 0.08, 0.5)
    lut = load_fg_lut("cpu").double()
    campos, rays_o = cam.camera_center.double(), _rays_o(cam, torch.float64)
    margin = vs.decision_margin(raw_o, campos, rays_o, lut, [s.detach() for s in spec], diffuse.detach())
    return SimpleNamespace(pc_o=pc_o, base_o=base_o, raw_o=raw_o, cam=cam, spec=spec, diffuse=diffuse, lut=lut, campos=campos, rays_o=rays_o,
                           margin=margin)


def _upstreams(P, C, seed=77):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(P, w, generator=g, dtype=torch.float64) for w in (1, 2, 4, 3, C)] + [torch.randn(P, 3, generator=g, dtype=torch.float64)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def _small_statement_inputs(P=6, seed=7):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d = torch.nn.functional.normalize(rnd(P, 3), dim=1)
    raw = [d * 1.0, rnd(P, 2) * 0.3 - 3.0, rnd(P, 4), rnd(P, 1), rnd(P, 1), rnd(P, 1), rnd(P, 3)]
    spec = [rnd(6, 8, 8, 3), rnd(6, 4, 4, 3), rnd(6, 2, 2, 3)]
    diffuse = rnd(6, 2, 2, 3)
    lut = torch.rand(16, 16, 2, generator=g, dtype=torch.float64)
    campos = torch.tensor([0.3, -3.5, 1.2], dtype=torch.float64)
    rays_o = campos + 1e-3
    vm = torch.eye(4, dtype=torch.float64)
    vm[3, :3] = torch.tensor([0.1, 0.2, 4.0], dtype=torch.float64)
    return raw, spec, diffuse, lut, campos, rays_o, vm


def test_statement_gradcheck_with_the_row0_coupling():
    raw, spec, diffuse, lut, campos, rays_o, vm = _small_statement_inputs()
    margin = vs.decision_margin(raw, campos, rays_o, lut, spec, diffuse)
    assert float(margin.min()) > 1e-3, margin                # gradcheck's finite differences (1e-6) stay inside every cell
    leaves = [t.clone().requires_grad_(True) for t in raw] + [t.clone().requires_grad_(True) for t in spec + [diffuse]]

    def fn(*a):
        return vs.volume_statement(a[:7], campos, rays_o, lut, list(a[7:10]), a[10], viewmatrix=vm)
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)
    # moving row 0's roughness changes every row's specular, moving another row's only that row's
    out = vs.volume_statement(leaves[:7], campos, rays_o, lut, leaves[7:10], leaves[10])
    spec_rows = out[4][:, 5:8].sum(dim=1)
    J = torch.stack([torch.autograd.grad(spec_rows[i], leaves[5], retain_graph=True)[0].reshape(-1) for i in range(spec_rows.shape[0])])
    assert bool((J[:, 0].abs() > 0).all())
    off = J.clone()
    off[:, 0] = 0
    off.fill_diagonal_(0)
    assert float(off.abs().max()) == 0.0
    assert bool((J.diagonal()[1:].abs() > 0).all())


@pytest.mark.parametrize("P,seed", CASES + (RENDER_CASE,))
def test_rows_under_the_decision_margin_are_rare(P, seed):
    """At most 1 % of a scene's rows sit closer than 1e-4 to a decision (none at all in the scenes of under a hundred rows)."""
    s = _scene(P, seed)
    parts = vs.decision_margin(s.raw_o, s.campos, s.rays_o, s.lut, [m.detach() for m in s.spec], s.diffuse.detach(), parts=True)
    print({k: float((v < MARGIN).double().mean()) for k, v in parts.items()})
    assert float((s.margin < MARGIN).double().mean()) <= 0.01


def _c_arguments(P=4):
    """Well-formed arguments of the two entry points on host addresses: for the checks that precede every HIP call."""
    import ctypes
    from materialrefgs_amd import _lib
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63
    prm = _lib.MrgsVolumeParams(P, *([p] * 10), None, 16, 0)
    chain = _lib.MrgsEnvMips()
    chain.n_levels, chain.res[0], chain.tex[0], chain.min_roughness, chain.max_roughness = 1, 4, p, 0.08, 0.5
    grads = _lib.MrgsVolumeGrads(*([p] * 7))
    return _lib, _lib.lib(), ctypes, p, prm, chain, grads, buf


def test_entry_points_check_their_arguments_before_any_launch():
    _lib, L, ctypes, p, prm, chain, grads, _buf = _c_arguments()
    BAD, OK = _lib.MRGS_E_BAD_ARG, _lib.MRGS_OK
    ref = ctypes.byref
    nws = L.mrgs_volume_features_ws_bytes()
    assert 16 <= nws <= 4096
    assert ctypes.sizeof(_lib.MrgsVolumeParams) == 8 + 11 * 8 + 8 and ctypes.sizeof(_lib.MrgsVolumeGrads) == 8 + 7 * 8
    fwd = lambda prm_=prm, spec=chain, diff=chain, feat=p: L.mrgs_volume_features_forward(ref(prm_), ref(spec), ref(diff), p, p, p, p, feat, None)
    bwd = lambda prm_=prm, g=grads, ws=p, n=nws: L.mrgs_volume_features_backward(ref(prm_), ref(chain), ref(chain), p, p, p, p, p, ref(g), None, ws, n, None)
    empty = _lib.MrgsVolumeParams(0, *([None] * 11), 16, 0)
    assert fwd(empty) == OK and bwd(empty) == OK                     # P = 0: nothing to launch
    wrong = _lib.MrgsVolumeParams(4, *([p] * 10), None, 16, 0)
    wrong.struct_size -= 8
    assert fwd(wrong) == BAD and bwd(wrong) == BAD
    assert fwd(_lib.MrgsVolumeParams(-1, *([p] * 10), None, 16, 0)) == BAD
    assert fwd(_lib.MrgsVolumeParams(4, *([p] * 10), None, 0, 0)) == BAD          # lut_res
    assert fwd(_lib.MrgsVolumeParams(4, *([p] * 8), None, p, None, 16, 0)) == BAD  # rays_o missing
    assert fwd(feat=p + 4) == BAD                                                 # feature rows leave as 16-byte pieces
    no_levels = _lib.MrgsEnvMips()
    assert fwd(spec=no_levels) == BAD and fwd(diff=no_levels) == BAD
    short = _lib.MrgsVolumeGrads(*([p] * 6), None)
    assert bwd(g=short) == BAD and bwd(ws=None) == BAD and bwd(n=nws - 1) == BAD
    g_wrong = _lib.MrgsVolumeGrads(*([p] * 7))
    g_wrong.struct_size = 7 * 8
    assert bwd(g=g_wrong) == BAD


@pytest.mark.skipif(torch.cuda.device_count() != 0, reason="host addresses as arguments: only for a machine without a device")
def test_launch_failure_goes_through_the_one_status_path():
    """Without a device the HIP calls fail: MRGS_E_HIP, and mrgs_last_hip_error() names this file (as tests/test_status.py shows for the others)."""
    _lib, L, ctypes, p, prm, chain, grads, _buf = _c_arguments()
    ref = ctypes.byref
    assert L.mrgs_volume_features_forward(ref(prm), ref(chain), ref(chain), p, p, p, p, p, None) == _lib.MRGS_E_HIP
    text = L.mrgs_last_hip_error()
    assert text and b" at mrgs_volume.hip:" in text, text
    assert L.mrgs_volume_features_backward(ref(prm), ref(chain), ref(chain), p, p, p, p, p, ref(grads), None, p, L.mrgs_volume_features_ws_bytes(),
                                           None) == _lib.MRGS_E_HIP
    assert b" at mrgs_volume.hip:" in L.mrgs_last_hip_error()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _device_model(P, seed, dev):
    _, _, pc_h, env = _models(P, H, W, seed, dev=dev)
    pc_h.env_map_2 = env
    env.build_mips()
    return pc_h, env


def _leaf_grads(outs, upstream, used, xyz, g_xyz, leaves):
    loss = sum((o * u.to(o.dtype).to(o.device)).sum() for o, u, on in zip(outs, upstream, used) if on)
    if g_xyz is not None:
        loss = loss + (xyz * g_xyz.to(xyz.dtype).to(xyz.device)).sum()
    return torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)


def _err(a, ref, rows=None):
    a, ref = a.detach().cpu().double(), ref.detach()
    scale = max(float(ref.abs().max()), 1e-30)
    if rows is not None:
        a, ref = a[rows], ref[rows]
    return float((a - ref).abs().max()) / scale if ref.numel() else 0.0


def _assert_rule(rows, label):
    print("\n".join(f"{label} {n:16s} native {en:.3e}  torch chain {ec:.3e}" for n, en, ec in rows))
    for n, en, ec in rows:
        assert en <= 1.5 * ec + 1e-6, (label, n, en, ec)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["2dgs", "pgsr"])
@pytest.mark.parametrize("P,seed", CASES)
def test_forward_and_every_gradient_against_the_statement(gpu_device, P, seed, flag):
    from materialrefgs_amd import shading
    dev = gpu_device
    s = _scene(P, seed)
    pc_h, env = _device_model(P, seed, dev)
    cam_d = s.cam.to(dev)
    vm = s.cam.world_view_transform.double() if flag != "2dgs" else None
    ref = vs.volume_statement(s.raw_o, s.campos, s.rays_o, s.lut, s.spec, s.diffuse, viewmatrix=vm)
    nat = shading.volume_features(pc_h, cam_d, env, flag=flag, pass_xyz=True)
    tor = vs.torch_chain(pc_h, cam_d, flag)
    assert nat[5].shape == (P, 3) and nat[4].shape == (P, 11 if flag == "2dgs" else 12)
    _assert_rule([(n, _err(a, r), _err(b, r)) for n, a, b, r in zip(OUT_NAMES, nat, tor, ref)], f"P={P} {flag} forward")

    keep = s.margin >= MARGIN
    up = _upstreams(P, ref[4].shape[1])
    leaves_o = s.raw_o + [s.base_o]
    leaves_h = [getattr(pc_h, n) for n in RAW_ATTRS] + [env.base]
    names = vs.RAW_NAMES + ("env.base",)
    for label, used, with_xyz in (("all five + g_xyz", (1, 1, 1, 1, 1), True), ("all five", (1, 1, 1, 1, 1), False),
                                  ("colors + rotations only", (0, 0, 1, 1, 0), False)):
        gx = up[5] if with_xyz else None
        g_ref = _leaf_grads(ref, up, used, s.raw_o[0], gx, leaves_o)
        g_nat = _leaf_grads(nat[:5], up, used, nat[5], gx, leaves_h)
        g_tor = _leaf_grads(tor, up, used, pc_h._xyz, gx, leaves_h)
        rows = []
        for n, a, b, r in zip(names, g_nat, g_tor, g_ref):
            zero = lambda t, like: torch.zeros_like(like) if t is None else t
            r = zero(r, leaves_o[names.index(n)])
            a, b = zero(a, leaves_h[names.index(n)]), zero(b, leaves_h[names.index(n)])
            sel = keep if n in PER_ROW else None
            rows.append((n, _err(a, r, sel), _err(b, r, sel)))
        _assert_rule(rows, f"P={P} {flag} {label}")


VOL_KEYS = ("render", "refl_strength_map", "diffuse_map", "specular_map", "base_color_map", "roughness_map", "rend_alpha", "rend_normal",
            "rend_dist", "surf_depth", "surf_normal")
PARAMS = RAW_ATTRS


@pytest.mark.gpu
@pytest.mark.parametrize("flag,srgb", [("2dgs", False), ("2dgs", True), ("pgsr", False), ("pgsr", True)])
def test_render_volume_native_beside_the_torch_chain(gpu_device, monkeypatch, flag, srgb):
    from materialrefgs_amd import renderer
    from oracle import render_oracle
    dev = gpu_device
    P, seed = RENDER_CASE
    pc_o, base_o, pc_h, env = _models(P, H, W, seed, dev=dev)
    for t in pc_o.parameters() + [base_o]:
        t.grad = None
    cam = orbit_camera(VIEW, H, W)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, use_asg=False, compute_cov3D_python=False)
    bg = torch.tensor([0.1, 0.2, 0.3])
    keys = VOL_KEYS + (("rend_distance",) if flag != "2dgs" else ())

    def loss(out, dv):
        g = torch.Generator().manual_seed(5)
        tot = 0
        for k in keys:
            w = torch.rand(out[k].shape, generator=g).to(out[k].dtype).to(dv)
            tot = tot + (out[k] * w).sum() * (0.01 if k == "surf_depth" else 1.0)
        return tot

    def run(native):
        monkeypatch.setattr(renderer, "_NATIVE_VOLUME", native)
        for n in PARAMS:
            getattr(pc_h, n).grad = None
        env.base.grad = None
        env.build_mips()
        out = renderer.render_volume(cam.to(dev), pc_h, pipe, bg.to(dev), srgb=srgb, opt=SimpleNamespace(indirect=False), flag=flag)
        loss(out, dev).backward()
        grads = {n: getattr(pc_h, n).grad.clone() for n in PARAMS}
        grads["env.base"], grads["viewspace_points"] = env.base.grad.clone(), out["viewspace_points"].grad.clone()
        return out, grads
    out_n, g_n = run(True)
    out_t, g_t = run(False)
    out_o = render_oracle.render_volume_oracle(cam, pc_o, base_o, 8, pipe, bg, srgb=srgb, flag=flag)
    loss(out_o, "cpu").backward()
    g_o = {n: getattr(pc_o, n).grad for n in PARAMS}
    g_o["env.base"], g_o["viewspace_points"] = base_o.grad, out_o["viewspace_points"].grad
    assert torch.equal(out_n["radii"].cpu(), out_o["radii"]) and torch.equal(out_n["radii"], out_t["radii"])
    _assert_rule([(k, _err(out_n[k], out_o[k]), _err(out_t[k], out_o[k])) for k in keys], f"{flag} srgb={srgb} map")
    _assert_rule([(n, _err(g_n[n], g_o[n]), _err(g_t[n], g_o[n])) for n in g_o], f"{flag} srgb={srgb} grad")


@pytest.mark.gpu
def test_no_host_synchronisation(gpu_device):
    from materialrefgs_amd import shading
    dev = gpu_device
    pc_h, env = _device_model(257, 13, dev)
    cam_d = orbit_camera(VIEW, H, W).to(dev)
    shading.load_fg_lut(dev)                                   # (uploaded once per device)
    env.diffuse
    up = [u.float().to(dev) for u in _upstreams(257, 12)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for flag in ("2dgs", "pgsr"):
            outs = shading.volume_features(pc_h, cam_d, env, flag=flag, pass_xyz=True)
            tot = sum((o * u[:, :o.shape[1]]).sum() for o, u in zip(outs[:5], up)) + (outs[5] * up[5]).sum()
            tot.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert float(pc_h._roughness.grad.abs().max()) > 0 and float(env.base.grad.abs().max()) > 0


@pytest.mark.gpu
def test_refusals_and_the_branches_that_stay_with_torch(gpu_device, monkeypatch):
    from materialrefgs_amd import renderer, shading
    dev = gpu_device
    P = 65
    pc_h, env = _device_model(P, 12, dev)
    cam_d = orbit_camera(VIEW, H, W).to(dev)

    def variant(**kw):
        pc = SimpleNamespace(**{n: getattr(pc_h, n).detach() for n in RAW_ATTRS})
        for k, v in kw.items():
            setattr(pc, k, v)
        return pc
    with pytest.raises(RuntimeError, match="no CPU path"):
        shading.volume_features(variant(_xyz=pc_h._xyz.detach().cpu()), cam_d, env)
    with pytest.raises(ValueError, match="float32"):
        shading.volume_features(variant(_rotation=pc_h._rotation.detach().double()), cam_d, env)
    with pytest.raises(ValueError, match="contiguous"):
        shading.volume_features(variant(_ori_color=pc_h._ori_color.detach().t().contiguous().t()), cam_d, env)
    with pytest.raises(ValueError, match="_scaling"):
        shading.volume_features(variant(_scaling=torch.zeros(P, 3, device=dev)), cam_d, env)
    empty = variant(**{n: getattr(pc_h, n).detach()[:0].clone().requires_grad_(True) for n in RAW_ATTRS})
    outs = shading.volume_features(empty, cam_d, env, flag="pgsr", pass_xyz=True)
    assert [tuple(o.shape) for o in outs] == [(0, 1), (0, 2), (0, 4), (0, 3), (0, 12), (0, 3)]
    sum(o.sum() for o in outs).backward()
    assert empty._roughness.grad.shape == (0, 1)

    # opt.indirect and compute_cov3D_python take the torch chain whatever the flag says: bit for bit the same render
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    for opt, cov in ((SimpleNamespace(indirect=True), False), (SimpleNamespace(indirect=False), True)):
        pipe = SimpleNamespace(depth_ratio=0.0, debug=False, use_asg=False, compute_cov3D_python=cov)
        outs = []
        for native in (True, False):
            monkeypatch.setattr(renderer, "_NATIVE_VOLUME", native)
            outs.append(renderer.render_volume(cam_d, pc_h, pipe, bg, opt=opt))
        for k in VOL_KEYS:
            assert torch.equal(outs[0][k], outs[1][k]), k
