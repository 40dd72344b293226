"""Shading half of the hot path: oracle known-answer tests on CPU, HIP-vs-oracle parity on the GPU.
The nvdiffrast sampling rules are restated (parity unpinned, see oracle/shading_oracle.py); the cube face convention is
pinned by the reference's cube_to_dir through the texel-centre known-answer test."""
import math

import numpy as np
import pytest
import torch

from oracle import shading_oracle as so


def make_mips(seed=0, max_res=32, min_res=4, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    mips = [torch.randn(6, max_res, max_res, 3, generator=g) * scale]
    while mips[-1].shape[1] > min_res:
        mips.append(torch.nn.functional.avg_pool2d(mips[-1].permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1).contiguous())
    return mips


def texel_centre_dirs(res):
    dirs, vals = [], []
    lin = torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    for s in range(6):
        dirs.append(so.cube_to_dir(s, gx, gy).reshape(-1, 3))
    return torch.cat(dirs, 0)


def test_oracle_cube_lookup_known_answer_at_texel_centres():
    """scene/light_utils.py:24-31 pins the convention: a lookup at cube_to_dir(texel centre) returns that texel exactly."""
    tex = make_mips(1, 16, 16)[0]
    d = texel_centre_dirs(16)
    out = so.cube_fetch(tex, d)
    np.testing.assert_allclose(out.numpy(), tex.reshape(-1, 3).numpy(), rtol=0, atol=1e-5)
    out2 = so.cube_fetch(tex, d * 3.7)     # un-normalised directions address the same texel
    np.testing.assert_allclose(out2.numpy(), tex.reshape(-1, 3).numpy(), rtol=0, atol=1e-5)


def test_oracle_cube_lookup_is_seamless():
    """Approaching a cube edge from both faces gives the same value (continuity across faces and at corners)."""
    tex = make_mips(2, 8, 8)[0]
    g = torch.Generator().manual_seed(5)
    t = torch.rand(200, generator=g) * 1.8 - 0.9
    eps = 1e-4
    a = torch.stack([torch.ones_like(t), t, torch.full_like(t, 1.0 - eps)], -1)   # on face +x next to the +z edge
    b = torch.stack([torch.full_like(t, 1.0 - eps), t, torch.ones_like(t)], -1)   # on face +z next to the +x edge
    np.testing.assert_allclose(so.cube_fetch(tex, a).numpy(), so.cube_fetch(tex, b).numpy(), atol=5e-3)
    c = torch.tensor([[1.0, 1.0 - eps, 1.0 - 2 * eps], [1.0 - eps, 1.0, 1.0 - 2 * eps], [1.0 - 2 * eps, 1.0 - eps, 1.0]])
    v = so.cube_fetch(tex, c).numpy()
    assert np.abs(v - v[0]).max() < 5e-3


def test_oracle_get_mip_and_trilinear():
    n = 4
    r = torch.tensor([0.0, 0.08, 0.29, 0.5, 0.75, 1.0, 1.3])
    expect = torch.tensor([0.0, 0.0, (0.29 - 0.08) / 0.42 * 2, 2.0, 2.5, 3.0, 3.0])
    np.testing.assert_allclose(so.get_mip(r, n).numpy(), expect.numpy(), atol=1e-6)
    mips = make_mips(3, 32, 4)
    d = torch.nn.functional.normalize(torch.randn(50, 3, generator=torch.Generator().manual_seed(1)), dim=-1)
    # roughness 0.08 -> level 0 exactly, 1.0 -> last level exactly
    lo = so.env_lookup(mips, d, torch.full((50,), 0.08))
    hi = so.env_lookup(mips, d, torch.full((50,), 1.0))
    np.testing.assert_allclose(lo.numpy(), torch.sigmoid(so.cube_fetch(mips[0], d)).numpy(), atol=1e-6)
    np.testing.assert_allclose(hi.numpy(), torch.sigmoid(so.cube_fetch(mips[-1], d)).numpy(), atol=1e-6)


def test_oracle_lut_known_answer():
    lut = torch.rand(16, 16, 2, generator=torch.Generator().manual_seed(2))
    c = (torch.arange(16).float() + 0.5) / 16
    uu, vv = torch.meshgrid(c, c, indexing="xy")
    out = so.lut_fetch(lut, torch.stack([uu.reshape(-1), vv.reshape(-1)], -1)).reshape(16, 16, 2)
    np.testing.assert_allclose(out.numpy(), lut.numpy(), atol=1e-6)
    edge = so.lut_fetch(lut, torch.tensor([[0.0, 0.0], [1.0, 1.0]]))          # clamp boundary
    np.testing.assert_allclose(edge.numpy(), torch.stack([lut[0, 0], lut[15, 15]]).numpy(), atol=1e-6)


def test_fg_lut_asset_matches_schlick_row():
    """Row v = 0 of the generated split-sum table is analytic: roughness -> 0 gives (1 - (1-c)^5, (1-c)^5)."""
    import os
    lut = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "materialrefgs_amd", "assets", "fg_lut_256.npy"))
    assert lut.shape == (256, 256, 2) and lut.dtype == np.float32
    c = (np.arange(256) + 0.5) / 256
    np.testing.assert_allclose(lut[0, :, 1], (1 - c) ** 5, atol=2e-3)
    np.testing.assert_allclose(lut[0, :, 0], 1 - (1 - c) ** 5, atol=2e-3)
    # the two reference probe texels quoted in SURVEY.md (2a #23): [y=0,x=0] and [y=255,x=255]
    np.testing.assert_allclose(lut[0, 0], [0.0097, 0.990], atol=2e-3)
    np.testing.assert_allclose(lut[255, 255], [0.309, 3.5e-5], atol=2e-3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU parity
# ---------------------------------------------------------------------------------------------------------------------
def _frame(H=40, W=56, seed=0):
    from materialrefgs_amd.synthetic import orbit_camera
    g = torch.Generator().manual_seed(seed)
    cam = orbit_camera(seed % 8, H, W)
    albedo = torch.rand(H, W, 3, generator=g)
    normal = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1) * (0.7 + 0.6 * torch.rand(H, W, 1, generator=g))
    alpha = torch.rand(H, W, 1, generator=g)
    refl = torch.rand(H, W, 1, generator=g)
    rough = torch.rand(H, W, 1, generator=g) * 1.1 - 0.05       # a few values outside [0,1] exercise the clamps
    return cam, albedo, normal, alpha, refl, rough


@pytest.mark.gpu
def test_envmap_lookup_parity(gpu_device):
    from materialrefgs_amd.shading import EnvLight
    mips = make_mips(4, 32, 4)
    env = EnvLight(device=gpu_device, min_res=4, max_res=32, trainable=True)
    with torch.no_grad():
        env.base.copy_(mips[0])

    def box_chain():   # this test is about the lookup kernels: plain box mips with torch's own autograd (build_mips has its own test)
        env.specular = [env.base]
        while env.specular[-1].shape[1] > 4:
            env.specular.append(torch.nn.functional.avg_pool2d(env.specular[-1].permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1).contiguous())
    box_chain()
    g = torch.Generator().manual_seed(9)
    N = 5000
    d = torch.randn(N, 3, generator=g)
    d[:384] = texel_centre_dirs(8) * 2.0                 # includes exact face-centre / edge-adjacent directions
    d[600:650, 0] = 1.0; d[600:650, 2] = 0.999                 # near a cube edge
    d[384:] = torch.nn.functional.normalize(d[384:], dim=-1)   # unit directions, as the shading code passes them
    rough = torch.rand(N, generator=g) * 1.2 - 0.1
    # forward + known answer on the GPU
    kat = env(texel_centre_dirs(32).to(gpu_device), mode="pure_env")
    np.testing.assert_allclose(kat.detach().cpu().numpy(), torch.sigmoid(mips[0].reshape(-1, 3)).numpy(), atol=2e-6)
    for use_rough in (True, False):
        base_o = mips[0].clone().requires_grad_(True)
        mips_o = [base_o]
        while mips_o[-1].shape[1] > 4:
            mips_o.append(torch.nn.functional.avg_pool2d(mips_o[-1].permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1))
        d_o, r_o = d.clone().requires_grad_(True), rough.clone().requires_grad_(True)
        out_o = so.env_lookup(mips_o, d_o, r_o if use_rough else None)
        d_h, r_h = d.to(gpu_device).requires_grad_(True), rough.to(gpu_device).requires_grad_(True)
        env.base.grad = None
        box_chain()
        out_h = env(d_h, roughness=r_h) if use_rough else env(d_h, mode="pure_env")
        np.testing.assert_allclose(out_h.detach().cpu().numpy(), out_o.detach().numpy(), atol=3e-6)
        gout = torch.randn(N, 3, generator=torch.Generator().manual_seed(3))
        out_o.backward(gout)
        out_h.backward(gout.to(gpu_device))
        np.testing.assert_allclose(env.base.grad.cpu().numpy(), base_o.grad.numpy(), atol=2e-5 * float(base_o.grad.abs().max()))
        # rows 0..383 sit exactly on texel centres, where the bilinear derivative is one-sided (left/right cell chosen by the
        # last ulp of fx): compare the direction gradient on the generic directions only
        gd_h, gd_o = d_h.grad.cpu().numpy()[384:], d_o.grad.numpy()[384:]
        bad = np.abs(gd_h - gd_o).max(axis=1) > 1e-4 * np.abs(gd_o).max()
        assert not bad.any(), (np.nonzero(bad)[0][:10] + 384, d[384:][bad][:5], gd_h[bad][:5], gd_o[bad][:5])
        if use_rough:
            assert np.abs(r_h.grad.cpu().numpy() - r_o.grad.numpy()).max() <= 1e-4 * float(r_o.grad.abs().max())


def test_fused_backward_schedule_model():
    """CPU: the host model of shade_fused_bwd_kernel's tile schedule (oracle/shading_oracle.fused_bwd_schedule) on hand-made keys, and the
    keys shade_taps gives for a real frame against the taps of the oracle's own fetch."""
    H, W = 48, 128                        # 2 x 4 tiles of 64 x 12 on one workgroup: the check after tile 4 flushes, tiles 5-8 follow
    keys = torch.arange(H * W * 8, dtype=torch.int64).reshape(H * W, 8)        # all distinct, level 0
    keys[:, 2:] = -1                                                           # two taps a pixel: 1 536 keys a tile, 6 144 a window
    s = so.fused_bwd_schedule(keys, H, W, n_cu=1, hashed_levels=[0])
    assert (s["ntiles"], s["grid"], s["tiles_per_wg"]) == (8, 1, 8)
    assert s["max_window_keys"] == 4 * 64 * 12 * 2 and s["windows_over_table"] == 2
    sim = s["sim"][0]
    assert sim["fallbacks"] > 0 and sim["fallbacks"] == H * W * 2 - sim["inserts"] and sim["mid_flushes"] == 1
    s = so.fused_bwd_schedule(keys, H, W, n_cu=256, hashed_levels=[0])          # a workgroup per tile: every window fits the table
    assert s["grid"] == 8 and s["windows_over_table"] == 0 and s["sim"][0] == dict(fallbacks=0, mid_flushes=0, inserts=64 * 12 * 2)
    s = so.fused_bwd_schedule(keys, H, W, n_cu=1, hashed_levels=[1])            # level 0 sits in the dense LDS copy: nothing hashed
    assert s["max_window_keys"] == 0 and s["sim"][0]["inserts"] == 0
    # the keys shade_taps gives for a real frame are the oracle fetch's taps of non-zero weight, and those taps reproduce env_lookup
    cam, albedo, normal, alpha, refl, rough = _frame(24, 40, 6)
    Hf, Wf, K = cam.HWK
    mips = make_mips(2, 32, 4)
    t = so.shade_taps([m.shape[1] for m in mips], Hf, Wf, K, cam.R, cam.T, normal.double(), rough.double())
    dirs, _ = so.mirror_dirs(Hf, Wf, K, cam.R, cam.T, normal.double())
    lev = so.get_mip(rough.reshape(-1).double(), len(mips)).clamp(0, len(mips) - 1)
    vals = torch.zeros(Hf * Wf, 3, dtype=torch.float64)
    want = torch.full((Hf * Wf, 4 * len(mips)), -1, dtype=torch.int64)
    for li, m in enumerate(mips):
        idx, w, _, _, _ = so.bilinear_taps(m.shape[1], dirs)
        share = torch.clamp(1 - (lev - li).abs(), min=0)
        for k in range(4):
            vals += (share * w[k])[:, None] * m.reshape(-1, 3).double()[idx[k]]
            want[:, 4 * li + k] = torch.where((share * w[k]) != 0, (li << 24) | idx[k], want[:, 4 * li + k])
    assert torch.equal(want.sort(dim=1, descending=True).values[:, :8], t["keys"].sort(dim=1, descending=True).values)
    assert float((torch.sigmoid(vals) - so.env_lookup([m.double() for m in mips], dirs, rough.reshape(-1).double())).abs().max()) < 1e-12
    assert float(t["cell_edge"].min()) >= 0.0 and float(t["level_edge"].min()) >= 0.0 and bool((t["face_gap"] >= 0).all())


@pytest.mark.gpu
def test_shade_specular_parity(gpu_device):
    from materialrefgs_amd.shading import EnvLight, get_specular_color_surfel, load_fg_lut
    cam, albedo, normal, alpha, refl, rough = _frame(40, 56, 3)
    H, W, K = cam.HWK
    mips = make_mips(7, 32, 4)
    lut = load_fg_lut("cpu")
    # ---- oracle
    leaves_o = [t.clone().requires_grad_(True) for t in (albedo, normal, alpha, refl, rough)]
    base_o = mips[0].clone().requires_grad_(True)
    mips_o = [base_o]
    while mips_o[-1].shape[1] > 4:
        mips_o.append(torch.nn.functional.avg_pool2d(mips_o[-1].permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1))
    spec_o, direct_o, weight_o = so.specular_color_surfel(mips_o, lut, leaves_o[0], H, W, K, cam.R, cam.T, leaves_o[1], leaves_o[2],
                                                          leaves_o[3], leaves_o[4])
    # ---- HIP (strided inputs: channel-first tensors permuted to HWC, as render_surfel passes them)
    env = EnvLight(device=gpu_device, min_res=4, max_res=32, trainable=True)
    with torch.no_grad():
        env.base.copy_(mips[0])
    env.specular = [env.base]          # plain box mips, as the oracle side of this test (build_mips has its own test)
    while env.specular[-1].shape[1] > 4:
        env.specular.append(torch.nn.functional.avg_pool2d(env.specular[-1].permute(0, 3, 1, 2), (2, 2)).permute(0, 2, 3, 1).contiguous())
    chw = [t.permute(2, 0, 1).contiguous().to(gpu_device).requires_grad_(True) for t in (albedo, normal, alpha, refl, rough)]
    hwc = [t.permute(1, 2, 0) for t in chw]
    camd = cam.to(gpu_device)
    spec_h, extra = get_specular_color_surfel(env, hwc[0], cam.HWK, camd.R, camd.T, hwc[1], hwc[2], refl_strength=hwc[3], roughness=hwc[4])
    tol = lambda ref: 1e-5 * max(1.0, float(ref.abs().max()))
    np.testing.assert_allclose(spec_h.detach().cpu().numpy(), spec_o.detach().numpy(), atol=tol(spec_o))
    np.testing.assert_allclose(extra["direct_light"].detach().cpu().numpy(), direct_o.detach().numpy(), atol=1e-5)
    np.testing.assert_allclose(extra["specular_weight"].detach().cpu().numpy(), weight_o.detach().numpy(), atol=tol(weight_o))
    # ---- gradients (all three outputs feed the loss)
    g = torch.Generator().manual_seed(11)
    gs, gd, gw = torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g), torch.randn(H, W, 3, generator=g)
    (spec_o * gs).sum().add((direct_o * gd).sum()).add((weight_o * gw).sum()).backward()
    torch.autograd.backward([spec_h, extra["direct_light"], extra["specular_weight"]], [gs.to(gpu_device), gd.to(gpu_device), gw.to(gpu_device)])
    for name, th, to in zip(("albedo", "normal", "alpha", "refl", "rough"), chw, leaves_o):
        a, b = th.grad.permute(1, 2, 0).cpu().numpy(), to.grad.numpy()
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (name, np.abs(a - b).max(), np.abs(b).max())
    a, b = env.base.grad.cpu().numpy(), base_o.grad.numpy()
    assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()


@pytest.mark.gpu
def test_render_surfel_end_to_end(gpu_device):
    """The reference-shaped render functions run on the HIP path and produce the reference's dictionary keys; gradients reach
    every parameter group including the environment cubemap."""
    from types import SimpleNamespace
    from materialrefgs_amd.renderer import SurfelModel, render_initial, render_surfel
    from materialrefgs_amd.shading import EnvLight
    from materialrefgs_amd.synthetic import make_shell_scene, orbit_camera
    P, H, W = 3000, 96, 128
    sc = make_shell_scene(P, S=0, seed=1, radius_px=6.0, image_size=128).to(gpu_device)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(gpu_device)
    env = EnvLight(device=gpu_device, trainable=True)
    with torch.no_grad():
        env.base.copy_(rnd(6, 128, 128, 3))
    env.build_mips()
    inv_sig = lambda x: torch.log(x / (1 - x))
    pc = SurfelModel(sc.means3D.clone(), torch.log(sc.scales), sc.rotations.clone(), inv_sig(sc.opacities.clamp(1e-4, 1 - 1e-4)),
                     sc.shs[:, :1].clone(), sc.shs[:, 1:].clone(), refl_strength=rnd(P, 1), roughness=rnd(P, 1), ori_color=rnd(P, 3),
                     indirect_dc=rnd(P, 1, 3) * 0.1, indirect_rest=rnd(P, 15, 3) * 0.01, envmap=env)
    for t in pc.parameters():
        t.requires_grad_(True)
    cam = orbit_camera(1, H, W).to(gpu_device)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device=gpu_device)
    out = render_surfel(cam, pc, pipe, bg, srgb=True, opt=SimpleNamespace(indirect=False))
    for k in ("render", "refl_strength_map", "diffuse_map", "diffuse_map_ori", "specular_map", "base_color_map", "roughness_map",
              "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal"):
        assert k in out, k
    assert out["render"].shape == (3, H, W) and torch.isfinite(out["render"]).all()
    loss = out["render"].mean() + 0.1 * out["rend_dist"].mean() + 0.1 * (out["rend_normal"] * out["surf_normal"]).sum(0).mean()
    loss.backward()
    for t in pc.parameters():
        assert t.grad is not None and torch.isfinite(t.grad).all()
    assert env.base.grad is not None and float(env.base.grad.abs().sum()) > 0
    assert out["viewspace_points"].grad is not None and out["viewspace_points"].grad.shape == (P, 3)
    ini = render_initial(cam, pc, pipe, bg)
    assert ini["render"].shape == (3, H, W) and set(("rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal")) <= set(ini)
    wo = render_surfel(cam, pc, pipe, bg, wo_render_img=True)
    assert "render" not in wo and wo["surf_normal"] is None and "base_color_map" in wo


@pytest.mark.gpu
def test_surfel_features_match_the_reference_ops(gpu_device):
    """mrgs_surfel_features_forward/backward (one HIP kernel each way) against the reference's own chain of torch ops
    (GaussianModel getters, get_normal, mirror direction, eval_sh, clamp, cat) evaluated in float64 on the CPU."""
    from materialrefgs_amd.renderer import SurfelModel, surfel_features
    from oracle.glue_oracle import surfel_features_reference
    torch.manual_seed(7)
    # (zero_ind: the upstream gradient of the indirect-radiance channels is exactly zero for whole waves of rows -- none of them, the first
    #  640 rows, all: the backward's shortcut for such waves must give what the full path gives)
    for P, zero_ind in ((1, 0), (63, 0), (64, 0), (1000, 0), (4097, 0), (1000, 640), (4097, 4097), (63, 63)):
        raw = dict(xyz=torch.randn(P, 3) * 2, scaling=torch.randn(P, 2) * 0.5 - 2, rotation=torch.randn(P, 4), opacity=torch.randn(P, 1),
                   refl=torch.randn(P, 1), rough=torch.randn(P, 1), ori=torch.randn(P, 3), idc=torch.randn(P, 1, 3) * 0.5,
                   irest=torch.randn(P, 15, 3) * 0.2)
        campos = torch.tensor([0.3, -4.0, 1.5])

        def model(dev, dtype):
            t = {k: v.to(device=dev, dtype=dtype).clone().requires_grad_(True) for k, v in raw.items()}
            pc = SurfelModel(t["xyz"], t["scaling"], t["rotation"], t["opacity"], torch.zeros(P, 1, 3, device=dev, dtype=dtype),
                             torch.zeros(P, 15, 3, device=dev, dtype=dtype), refl_strength=t["refl"], roughness=t["rough"],
                             ori_color=t["ori"], indirect_dc=t["idc"], indirect_rest=t["irest"])
            return pc, t
        pc_g, tg = model(gpu_device, torch.float32)
        pc_c, tc = model("cpu", torch.float64)
        outs_g = surfel_features(pc_g, campos.to(gpu_device))
        outs_c = surfel_features_reference(pc_c, campos.double())
        ups = [torch.randn_like(o) for o in outs_c]
        if zero_ind:
            feat_i = next(i for i, o in enumerate(outs_c) if o.dim() == 2 and o.shape[1] == 8)
            ups[feat_i][:zero_ind, 5:8] = 0.0
        for og, oc in zip(outs_g, outs_c):
            assert og.shape == oc.shape
            assert float((og.detach().cpu().double() - oc.detach()).abs().max()) <= 2e-6 * max(1.0, float(oc.abs().max()))
        torch.autograd.backward(list(outs_g), [u.float().to(gpu_device) for u in ups])
        torch.autograd.backward(list(outs_c), ups)
        for k in raw:
            a, b = tg[k].grad.detach().cpu().double(), tc[k].grad
            assert float((a - b).abs().max()) <= 1e-5 * max(1e-3, float(b.abs().max())), (P, zero_ind, k)


PD_LEAVES = ("xyz", "scaling", "rotation", "opacity", "refl", "rough", "ori", "idc", "irest")     # the glue node's nine raw leaves, in its order
PD_KINK = 1e-2              # |n_cam . c_cam| below this: the row sits on the kink of |.|, its plane distance takes no upstream gradient
# (name, pass_xyz, the outputs that receive an upstream gradient; the others arrive at the node as None)
PD_VARIANTS = [("four outputs", False, (0, 1, 2, 3)), ("five outputs", True, (0, 1, 2, 3, 4))] + \
              [(f"output {i} alone", True, (i,)) for i in range(5)]


def _plane_distance_case(P):
    """Raw leaves, camera and upstream gradients of the plane-distance test for P rows (fixed per P), and the float64 checker's outputs:
    (opacity, scales, rotations, [features 8 | plane distance | 0 0 0], centres) with glue_oracle.surfel_features_reference and
    glue_oracle.get_distance.  Camera centre and view matrix come from ONE camera.  Returns the share of kink rows as well."""
    from materialrefgs_amd.renderer import SurfelModel
    from materialrefgs_amd.synthetic import orbit_camera
    from oracle.glue_oracle import get_distance, surfel_features_reference
    g = torch.Generator().manual_seed(1000 + P)
    rnd = lambda *s: torch.randn(*s, generator=g)
    raw = dict(xyz=rnd(P, 3) * 2, scaling=rnd(P, 2) * 0.5 - 2, rotation=rnd(P, 4), opacity=rnd(P, 1), refl=rnd(P, 1), rough=rnd(P, 1),
               ori=rnd(P, 3), idc=rnd(P, 1, 3) * 0.5, irest=rnd(P, 15, 3) * 0.2)
    cam = orbit_camera(3, 48, 64)

    def model(dev, dtype):
        t = {k: v.to(device=dev, dtype=dtype).clone().requires_grad_(True) for k, v in raw.items()}
        pc = SurfelModel(t["xyz"], t["scaling"], t["rotation"], t["opacity"], torch.zeros(P, 1, 3, device=dev, dtype=dtype),
                         torch.zeros(P, 15, 3, device=dev, dtype=dtype), refl_strength=t["refl"], roughness=t["rough"],
                         ori_color=t["ori"], indirect_dc=t["idc"], indirect_rest=t["irest"])
        return pc, [t[k] for k in PD_LEAVES]

    pc_c, leaves_c = model("cpu", torch.float64)
    op, sc, rot, feat = surfel_features_reference(pc_c, cam.camera_center.double())
    outs_c = (op, sc, rot, torch.cat((feat, get_distance(pc_c, cam), torch.zeros(P, 3, dtype=torch.float64)), dim=-1), pc_c.get_xyz)
    with torch.no_grad():       # the signed n_cam . c_cam of get_distance, float64
        Wv = cam.world_view_transform.double()
        d = pc_c.get_xyz - cam.camera_center.double()
        signed = ((pc_c.get_normal(1.0, d / d.norm(dim=1, keepdim=True)) @ Wv[:3, :3]) * (pc_c.get_xyz @ Wv[:3, :3] + Wv[3, :3])).sum(-1)
    kink = signed.abs() < PD_KINK
    ups = [rnd(*o.shape).double() for o in outs_c]
    ups[3][:, 9:] = 0.0
    ups[3][kink, 8] = 0.0
    return cam, model, leaves_c, outs_c, ups, float(kink.double().mean())


def _grads_of(outs, leaves, ups, which):
    got = torch.autograd.grad([outs[i] for i in which], leaves, [ups[i].to(outs[i].dtype) for i in which], retain_graph=True, allow_unused=True)
    return [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(got, leaves)]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000, 4097])
def test_surfel_features_with_the_plane_distance_match_float64(gpu_device, P):
    """mrgs_surfel_features_forward/backward with a view matrix (the "pgsr" rows: twelve floats, the plane distance |n_cam . c_cam| of
    get_distance in column 8, zeros behind it) against the reference's torch ops in float64 on the CPU: glue_oracle.surfel_features_reference
    next to glue_oracle.get_distance.  Forward: columns 0..7 as in the test above, column 8 within 2e-6 max(1, max|ref|) of the float64
    distance, columns 9..11 exact zeros.  Backward, every raw leaf within 1e-5 max(1e-3, max|ref|), for: all four outputs with an upstream
    gradient; all five with pass_xyz (the centres' own gradient joins inside the kernel); each of the five outputs alone (the others reach
    the node as None: set_materialize_grads(False)).  The node writes into torch.empty_like buffers: NaN-filled tensors of the leaves'
    shapes are allocated and dropped just before each backward, so that a leaf the kernel left unwritten reads NaN.  Rows within 1e-2 of
    the kink of |.| (at most 1 % of the rows) take no upstream gradient on column 8; their forward value is compared all the same."""
    from materialrefgs_amd.renderer import surfel_features
    cam, model, leaves_c, outs_c, ups, kink_share = _plane_distance_case(P)
    assert kink_share <= 0.01, kink_share
    camd = cam.to(gpu_device)
    worst = {}
    for name, pass_xyz, which in PD_VARIANTS:
        pc_g, leaves_g = model(gpu_device, torch.float32)
        outs_g = surfel_features(pc_g, camd.camera_center, pass_xyz=pass_xyz, viewmatrix=camd.world_view_transform)
        assert len(outs_g) == (5 if pass_xyz else 4)
        for i, og in enumerate(outs_g):
            a, b = og.detach().cpu().double(), outs_c[i].detach()
            assert a.shape == b.shape, (name, i)
            if i == 3:
                assert float((a[:, :8] - b[:, :8]).abs().max()) <= 2e-6 * max(1.0, float(b[:, :8].abs().max())), name
                assert float((a[:, 8] - b[:, 8]).abs().max()) <= 2e-6 * max(1.0, float(b[:, 8].abs().max())), (name, float((a[:, 8] - b[:, 8]).abs().max()))
                assert float(a[:, 9:].abs().max()) == 0.0, name
            else:
                assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max())), (name, i)
        want = _grads_of(outs_c, leaves_c, ups, which)
        poison = [torch.full_like(t, float("nan")) for t in leaves_g]
        del poison
        torch.autograd.backward([outs_g[i] for i in which], [ups[i].float().to(gpu_device) for i in which])
        for k, t, b in zip(PD_LEAVES, leaves_g, want):
            assert t.grad is not None, (name, k)
            a = t.grad.detach().cpu().double()
            assert bool(torch.isfinite(a).all()), (P, name, k)
            e = float((a - b).abs().max()) / max(1e-3, float(b.abs().max()))
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= 1e-5, (P, name, k, e)
    print(f"P={P}: kink share {kink_share:.4f}; worst leaf errors " + ", ".join(f"{k} {e:.1e}" for k, e in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("depth_ratio", [0.0, 0.3, 1.0])
def test_fused_maps_match_the_reference_ops(gpu_device, depth_ratio):
    """mrgs_surfel_maps_forward/backward against compute_2dgs_normal_and_regularizations + depth_to_normal + the normal_map
    division evaluated with the reference's torch ops in float64 on the CPU (including pixels with alpha = 0 -> nan_to_num)."""
    from types import SimpleNamespace
    from materialrefgs_amd.renderer import compute_2dgs_normal_and_regularizations
    from oracle.glue_oracle import compute_2dgs_normal_and_regularizations_reference
    from materialrefgs_amd.synthetic import orbit_camera
    H, W = 37, 53
    cam = orbit_camera(2, H, W)
    g = torch.Generator().manual_seed(11)
    allmap = torch.rand(7, H, W, generator=g)
    allmap[1] = allmap[1] * 0.9 + 0.05
    allmap[0] = allmap[1] * (3.0 + torch.rand(H, W, generator=g))          # expected depth 3..4
    allmap[5] = 3.0 + torch.rand(H, W, generator=g)
    allmap[2:5] = torch.randn(3, H, W, generator=g) * allmap[1]
    hole = torch.rand(H, W, generator=g) < 0.1                                # untouched pixels: alpha = depth = 0
    allmap[:, hole] = 0.0
    pipe = SimpleNamespace(depth_ratio=depth_ratio)

    am_c = allmap.double().requires_grad_(True)
    cam_c = cam._replace(world_view_transform=cam.world_view_transform.double(), full_proj_transform=cam.full_proj_transform.double())
    ref = compute_2dgs_normal_and_regularizations_reference(am_c, cam_c, pipe)
    nm_ref = ref["render_normal"].permute(1, 2, 0) / ref["render_alpha"].permute(1, 2, 0).clamp_min(1e-6)
    am_g = allmap.to(gpu_device).requires_grad_(True)
    out = compute_2dgs_normal_and_regularizations(am_g, cam.to(gpu_device), pipe, return_normal_map=True)
    pairs = [(out["render_normal"], ref["render_normal"]), (out["surf_depth"], ref["surf_depth"]), (out["surf_normal"], ref["surf_normal"]),
             (out["normal_map"], nm_ref)]
    ups = [torch.randn(r.shape, generator=g, dtype=torch.float64) for _, r in pairs]
    for (a, b), name in zip(pairs, ("render_normal", "surf_depth", "surf_normal", "normal_map")):
        assert a.shape == b.shape, name
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 2e-5 * max(1.0, float(b.detach().abs().max())), name
    torch.autograd.backward([a for a, _ in pairs], [u.float().to(gpu_device) for u in ups])
    torch.autograd.backward([b for _, b in pairs], ups)
    ga, gb = am_g.grad.detach().cpu().double(), am_c.grad
    # the reference's autograd yields NaN at alpha = 0 (0 * d(x/0)); the rasterizer never reads those pixels (they have no
    # contributors).  The fused kernel writes zeros there; everywhere else the two must agree.
    ok = torch.isfinite(gb)
    assert torch.isfinite(ga).all() and float(ok.double().mean()) > 0.85
    assert float((ga - gb)[ok].abs().max()) <= 2e-4 * float(gb[ok].abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("srgb", [False, True])
def test_fused_composite_matches_the_reference_ops(gpu_device, srgb):
    from materialrefgs_amd.gs_utils import linear_to_srgb
    from materialrefgs_amd.renderer import _SurfelComposite
    H, W = 19, 33
    g = torch.Generator().manual_seed(5)
    base, spec = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g) * 0.5
    refl, alpha, bg = torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g), torch.tensor([0.1, 0.5, 0.9])
    base[:, :2] *= 1e-3                                                       # exercises the linear branch of the sRGB curve
    spec[:, :2] *= 1e-3
    tc = [t.double().requires_grad_(True) for t in (base, refl, spec, alpha)]
    tg = [t.to(gpu_device).requires_grad_(True) for t in (base, refl, spec, alpha)]
    diffuse_c = (1 - tc[1]) * tc[0]
    fin = diffuse_c + tc[2]
    if srgb:
        fin = linear_to_srgb(fin)
    render_c = fin + bg.double()[:, None, None] * (1 - tc[3])
    render_g, diffuse_g = _SurfelComposite.apply(tg[0], tg[1], tg[2], tg[3], bg.to(gpu_device), srgb)
    assert float((render_g.detach().cpu().double() - render_c.detach()).abs().max()) <= 2e-6
    assert float((diffuse_g.detach().cpu().double() - diffuse_c.detach()).abs().max()) <= 2e-6
    u1, u2 = torch.randn(3, H, W, generator=g, dtype=torch.float64), torch.randn(3, H, W, generator=g, dtype=torch.float64)
    torch.autograd.backward([render_c, diffuse_c], [u1, u2])
    torch.autograd.backward([render_g, diffuse_g], [u1.float().to(gpu_device), u2.float().to(gpu_device)])
    for a, b in zip(tg, tc):
        assert float((a.grad.detach().cpu().double() - b.grad).abs().max()) <= 2e-5 * max(1.0, float(b.grad.abs().max()))


@pytest.mark.gpu
def test_build_mips_prefilter_matches_dense_oracle(gpu_device):
    """EnvLight.build_mips (box mips + GGX prefilter as sparse operators + the reference's mip backward rule) against the dense
    float64 restatement of renderutils' cubemap kernels, forward and backward, on a 32 -> 16 -> 8 chain; plus the diffuse map."""
    from oracle import envfilter_oracle as eo
    from materialrefgs_amd.shading import EnvLight
    g = torch.Generator().manual_seed(3)
    env = EnvLight(device=gpu_device, min_res=8, max_res=32, trainable=True)
    base = torch.randn(6, 32, 32, 3, generator=g)
    with torch.no_grad():
        env.base.copy_(base.to(gpu_device))
    env.build_mips()
    spec_o, diff_o, ops = eo.build_mips(base.double().numpy(), 8)
    assert [tuple(m.shape) for m in env.specular] == [(6, 32, 32, 3), (6, 16, 16, 3), (6, 8, 8, 3)]
    for a, b in zip(env.specular, spec_o):
        assert float(np.abs(a.detach().cpu().double().numpy() - b).max()) <= 2e-5 * max(1.0, float(np.abs(b).max()))
    assert float(np.abs(env.diffuse.detach().cpu().double().numpy() - diff_o).max()) <= 2e-5 * max(1.0, float(np.abs(diff_o).max()))
    ups = [torch.randn(m.shape, generator=g) for m in env.specular]
    torch.autograd.backward(env.specular, [u.to(gpu_device) for u in ups])
    g_o = eo.build_mips_backward(ops, [u.double().numpy() for u in ups])
    assert float(np.abs(env.base.grad.detach().cpu().double().numpy() - g_o).max()) <= 2e-5 * float(np.abs(g_o).max())


@pytest.mark.gpu
def test_blocked_filter_rows_equal_the_plain_csr(gpu_device, monkeypatch):
    """The long-row filter levels stored as blocks of four columns (mrgs_csr_spmv3, val_bytes 8) against the same operator kept as one
    (column, weight) pair per non-zero: same quantised weights, only the order of the sums differs."""
    import materialrefgs_amd.shading as sh
    g = torch.Generator().manual_seed(11)
    for res, rough in ((16, 1.0), (32, 0.5)):
        x = torch.randn(6, res, res, 3, generator=g).to(gpu_device)
        monkeypatch.setattr(sh, "_NO_BLOCKED", True)
        plain = sh.CubemapFilterOp(gpu_device, res, 0, rough, 0.99)
        monkeypatch.setattr(sh, "_NO_BLOCKED", False)
        blocked = sh.CubemapFilterOp(gpu_device, res, 0, rough, 0.99)
        assert plain.val.dim() == 1 and blocked.val.dim() == 2 and blocked.val.shape[1] == 2
        assert int(blocked.row_ptr[-1]) * 4 >= blocked.nnz and int(blocked.row_ptr[-1]) * 4 < 1.35 * blocked.nnz     # slots mostly used
        for tr in (False, True):
            a, b = plain.apply_matrix(x, transpose=tr), blocked.apply_matrix(x, transpose=tr)
            assert float((a - b).abs().max()) <= 2e-6 * float(a.abs().max())


@pytest.mark.gpu
def test_symmetric_filter_rows_equal_the_full_operator(gpu_device, monkeypatch):
    """The long-row levels of the reference's default chain (64 / 0.29, 32 / 0.5, 16 / 1.0 and the diffuse map) as rows of one fundamental
    domain of the cube's symmetries (MrgsSpmvDesc.image_rows, the batched launch) against the full blocked matrices (mrgs_csr_spmv3), both
    ways, in one batch as build_mips runs them; the build-time check of each operator passed (they are in use, not the fall-back)."""
    import materialrefgs_amd.shading as sh
    g = torch.Generator().manual_seed(17)
    ops = [sh.CubemapFilterOp.get(gpu_device, 64, 0, 0.29, 0.99), sh.CubemapFilterOp.get(gpu_device, 32, 0, 0.5, 0.99),
           sh.CubemapFilterOp.get(gpu_device, 16, 0, 1.0, 0.99), sh.CubemapFilterOp.get(gpu_device, 16, 1)]
    for op in ops:
        assert op.sym is not None and op.t_sym is not None and max(op.sym_error) <= sh._SYM_TOL, (op.res, op.kind, op.sym_error)
        m = (op.res // 2) * (op.res // 2 + 1) // 2
        assert op.sym.n_rows == m and int(op.sym.tile_ptr[-1]) == m and op.sym.patches * 256 * 2 * 30 < op.nnz * 4    # (dense tiles, zeros included: < 1/30 of the full matrix)
    xs = [torch.randn(6, op.res, op.res, 3, generator=g).to(gpu_device) * 3.0 for op in ops]
    for tr in (False, True):
        got = sh._spmv_batched(ops, xs, transpose=tr, cache=False)
        for op, x, y in zip(ops, xs, got):
            full = op.apply_matrix(x, transpose=tr)
            assert float((y - full).abs().max()) <= 2e-5 * float(x.abs().max()), (op.res, op.kind, tr)
    # one operator absent from the batch
    got = sh._spmv_batched(ops, [xs[0], None, xs[2], None], transpose=False, cache=False)
    assert got[1] is None and got[3] is None and float((got[2] - ops[2].apply_matrix(xs[2])).abs().max()) <= 2e-5 * float(xs[2].abs().max())
    # the fall-back (and MRGS_NO_SYMMETRIC_SPMV=1): the full blocked matrices in the same batched launch, next to a symmetric level
    monkeypatch.setattr(sh, "_NO_SYM", True)
    full32 = sh.CubemapFilterOp(gpu_device, 32, 0, 0.5, 0.99)
    assert full32.sym is None and full32.val.dim() == 2
    for tr in (False, True):
        a = sh._spmv_batched([ops[0], full32], [xs[0], xs[1]], transpose=tr, cache=False)
        b = sh._spmv_batched([ops[0], ops[1]], [xs[0], xs[1]], transpose=tr, cache=False)
        assert float((a[1] - b[1]).abs().max()) <= 2e-5 * float(xs[1].abs().max()) and torch.equal(a[0], b[0])


def _unpack_blocks(bptr, bcol, packed, m, ncols):
    """dense [m, ncols] integer weights of a blocked-rows matrix (host check of CubemapFilterOp._block4 / _block4_general)"""
    out = np.zeros((m, ncols), dtype=np.int64)
    bp = bptr.long().numpy()
    bc = (bcol.long() & 0xFFFF).numpy()
    w = (packed.long() & 0xFFFFFFFF).numpy()
    rows = np.repeat(np.arange(m), np.diff(bp))
    for j, (word, sh) in enumerate(((0, 0), (0, 16), (1, 0), (1, 16))):
        out[rows, 4 * bc + j] = (w[:, word] >> sh) & 0xFFFF
    return out


@pytest.mark.parametrize("kind,rough", [(0, 1.0), (1, 1.0)])
def test_symmetric_rows_reproduce_the_dense_filter(kind, rough):
    """The prefilter operator kept as the rows of ONE fundamental domain of the cube's 48 symmetries (CubemapFilterOp._symmetric, the host
    side of MrgsSpmvDesc.image_rows -- rows in 4 x 4 tiles, block indices local to the tile's panel; mrgs_cube_symmetry_rows is host code
    of the library): y[g r0] = post * sum_c W'(r0, c) (pre x)[g c] evaluated in numpy equals the dense oracle operator (16 x 16 faces: the reference's last specular level and its diffuse map) both ways,
    every texel written exactly once."""
    from oracle import envfilter_oracle as eo
    from materialrefgs_amd import shading as sh
    N = 16
    n = 6 * N * N
    img = sh._cube_symmetry_rows(N).long().numpy()
    assert img.shape == (48, n) and all(np.array_equal(np.sort(p), np.arange(n)) for p in img) and np.array_equal(img[0], np.arange(n))
    D = eo.cube_to_dir(N)
    for g in (1, 7, 13, 29, 47):                       # a symmetry is a signed axis permutation of the texel directions
        Mg = np.linalg.lstsq(D, D[img[g]], rcond=None)[0].T
        assert np.allclose(np.abs(Mg).round(6).sum(0), 1.0) and np.allclose(np.abs(Mg).round(6).sum(1), 1.0) and np.allclose(D @ Mg.T, D[img[g]], atol=1e-12)
    if kind == 0:
        Wd = eo.specular_weights(N, rough, eo.cos_cutoff(rough))
        nsum = Wd.sum(1)
        A = Wd / nsum[:, None]
    else:
        A = eo.diffuse_matrix(N)
        nsum = np.ones(n)
    area = sh._pixel_area(N).astype(np.float64)
    assert np.allclose(area, eo.pixel_area(N), rtol=1e-6)
    op = object.__new__(sh.CubemapFilterOp)
    op.res, op.nrows = N, n
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, 3))
    for tr in (False, True):
        M = A.T if tr else A
        r, c = np.nonzero(M)
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])).to(torch.int32)
        col, val = torch.from_numpy(c).to(torch.int32), torch.from_numpy(M[r, c]).float()
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
        if not tr:
            S = op._symmetric(ptr, col, val, t(1.0 / area), t(area), t(nsum))
        else:
            S = op._symmetric(ptr, col, val, t(nsum), t(1.0 / nsum), t(1.0 / area))
        m = S.n_rows
        assert m == (N // 2) * (N // 2 + 1) // 2 and S.image_rows.shape == (m, 48) and int(S.tile_ptr[-1]) == m
        ir = S.image_rows.numpy()
        assert np.array_equal(np.sort(ir[ir >= 0]), np.arange(n))                      # every texel written exactly once
        # the dense tiles back to rows of global columns: [patch of the panel][lane = 16 (x & 3) + row in tile][patch row y & 3]
        tp, pp = S.tile_ptr.long().numpy(), S.panel_ptr.long().numpy()
        assert S.n_tiles == len(tp) - 1 == len(pp) - 1 and int(np.diff(tp).max()) <= 16 and pp[-1] == S.patches
        src = (S.panel_src.long() & 0xFFFF).numpy()
        dense = (S.val.long() & 0xFFFF).numpy().reshape(-1, 4, 16, 4)                   # [patch, x & 3, row in tile, y & 3]
        Wq = np.zeros((m, n))
        npf = N // 4
        for ti in range(S.n_tiles):
            rows_t = tp[ti + 1] - tp[ti]
            for k in range(pp[ti], pp[ti + 1]):
                assert not dense[k, :, rows_t:, :].any()
                ps, py, px = src[k] // (npf * npf), (src[k] // npf) % npf, src[k] % npf
                for j in range(4):
                    c0 = (ps * N + 4 * py + j) * N + 4 * px
                    Wq[tp[ti]:tp[ti + 1], c0:c0 + 4] = dense[k, :, :rows_t, j].T
        post, pre = S.post, S.pre
        xs = pre.double().numpy()[:, None] * x
        y = np.zeros((n, 3))
        for g in range(48):
            rows = ir[:, g]
            yg = Wq @ xs[img[g]]                                                        # (pre x)[g c] for the columns c of the canonical rows
            y[rows[rows >= 0]] = (post.double().numpy()[rows[rows >= 0], None] * yg[rows >= 0])
        ref = M @ x
        assert float(np.abs(y - ref).max()) <= 1e-5 * float(np.abs(x).max())


def test_block4_conversion_reproduces_the_csr_matrix():
    """CubemapFilterOp._block4 (host side of the blocked prefilter rows, pure torch): every (row, column, weight) of a random CSR
    matrix with 16-bit columns and weights comes back from the (block column, four weights) form, padding slots are zero, rows keep
    their order and the block columns ascend inside a row."""
    from materialrefgs_amd.shading import CubemapFilterOp
    g = torch.Generator().manual_seed(5)
    n = 96                                   # columns = rows (square filters), a multiple of 4
    counts = torch.randint(0, 30, (n,), generator=g)
    counts[7] = 0                            # an empty row
    rows = torch.repeat_interleave(torch.arange(n), counts)
    cols = torch.cat([torch.randperm(n, generator=g)[:int(c)] for c in counts]) if int(counts.sum()) else torch.zeros(0, dtype=torch.long)
    q = torch.randint(1, 65536, (cols.shape[0],), generator=g)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)]).to(torch.int32)
    bptr, bcol, packed = CubemapFilterOp._block4(ptr, (cols & 0xFFFF).to(torch.int16), (q & 0xFFFF).to(torch.int16), counts)
    dense = torch.zeros(n, n, dtype=torch.long)
    dense[rows, cols] = q
    back = torch.zeros(n, n, dtype=torch.long)
    bptr_l = bptr.long()
    assert bptr_l[0] == 0 and bptr_l[-1] == bcol.shape[0] == packed.shape[0]
    for r in range(n):
        bc = (bcol[bptr_l[r]:bptr_l[r + 1]].long() & 0xFFFF)
        assert bool((bc[1:] > bc[:-1]).all())
        for k, b in zip(range(int(bptr_l[r]), int(bptr_l[r + 1])), bc.tolist()):
            w = packed[k].long() & 0xFFFFFFFF
            four = [int(w[0]) & 0xFFFF, int(w[0]) >> 16, int(w[1]) & 0xFFFF, int(w[1]) >> 16]
            for j in range(4):
                back[r, 4 * b + j] = four[j]
    assert torch.equal(back, dense)


def test_envfilter_oracle_known_answers():
    """CPU: the dense restatement of renderutils' cubemap filters -- rows of the specular operator are normalised (a constant
    cubemap stays constant), the diffuse operator integrates cos / pi over the hemisphere (~1 for a constant map), the mip
    backward rule conserves the mass of the gradient (bilinear weights sum to 1, times 4 fine texels * 0.25), cut-off angles grow
    with roughness."""
    from oracle import envfilter_oracle as eo
    N = 8
    P = eo.specular_matrix(N, 0.5)
    assert np.allclose(P.sum(1), 1.0) and (P >= 0).all()
    const = np.full((6, 32, 32, 3), 0.7)
    spec, diffuse, ops = eo.build_mips(const, 8)           # 32 -> 16 -> 8 (the reference's roughness schedule needs >= 3 levels)
    for s in spec:
        assert np.allclose(s, 0.7)
    assert 0.7 < float(diffuse.mean()) / 0.7 < 1.1      # atan-product texel areas are coarse at 8x8 (the reference's formula)
    # the reference's 16x16-tile interval test (cubemap.cu:203-214) is not conservative when one tile spans a face: at 16x16 and
    # roughness 0.08 most windows come out empty (0 / 0 in the reference); from 32x32 on nothing that qualifies is dropped
    D16, c08 = eo.cube_to_dir(16), np.float32(eo.cos_cutoff(0.08))
    assert int((~(eo.bounds_mask(16, c08) & (D16 @ D16.T >= c08)).any(1)).sum()) > 1000
    D32 = eo.cube_to_dir(32)
    for r in (0.08, 0.29):
        cc = np.float32(eo.cos_cutoff(r))
        full = D32 @ D32.T >= cc
        assert not (full & ~eo.bounds_mask(32, cc)).any()
    assert eo.cos_cutoff(0.08) > eo.cos_cutoff(0.29) > eo.cos_cutoff(0.5) > eo.cos_cutoff(1.0) > 0.0
    g = np.random.default_rng(0).normal(size=(6, 4, 4, 3))
    assert np.allclose(eo.mip_backward(g).sum(axis=(0, 1, 2)), g.sum(axis=(0, 1, 2)), rtol=1e-6, atol=1e-9)
    d = eo.cube_to_dir(N)
    assert np.allclose((d * d).sum(-1), 1.0) and abs(float(eo.pixel_area(N).sum()) - 4 * np.pi) < 0.25 * 4 * np.pi


def test_maps_frame_matches_depths_to_points():
    """CPU: the camera constants handed to the fused map kernels (built on the host in float64) reproduce the reference's
    depths_to_points (utils/point_utils.py:9-24): point(x, y) = depth * (M (x, y, 1)) + o."""
    from materialrefgs_amd.renderer import _maps_frame
    from oracle.glue_oracle import depths_to_points
    from materialrefgs_amd.synthetic import orbit_camera
    H, W = 21, 34
    cam = orbit_camera(5, H, W)
    fr = _maps_frame(cam, 0.25)
    assert (fr.H, fr.W) == (H, W) and abs(fr.depth_ratio - 0.25) < 1e-7
    depth = torch.rand(1, H, W, dtype=torch.float64) * 3 + 1
    cam64 = cam._replace(world_view_transform=cam.world_view_transform.double(), full_proj_transform=cam.full_proj_transform.double())
    ref = depths_to_points(cam64, depth).reshape(H, W, 3).numpy()
    M = np.array(list(fr.ray_matrix), dtype=np.float64).reshape(3, 3)
    o = np.array(list(fr.ray_origin), dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rays = np.stack([xs, ys, np.ones_like(xs)], -1).astype(np.float64) @ M.T
    mine = depth[0].numpy()[..., None] * rays + o
    assert np.abs(mine - ref).max() <= 1e-5 * np.abs(ref).max()
    V = np.array(list(fr.view_rot), dtype=np.float64).reshape(3, 3)
    assert np.allclose(V, cam.world_view_transform[:3, :3].double().numpy(), atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("srgb", [False, True])
def test_shade_and_composite_node_matches_the_separate_ops(gpu_device, srgb):
    """The single autograd node render_surfel uses (whole [8,H,W] material map in, one gradient tensor out) against the
    reference-shaped sequence get_specular_color_surfel -> compositing on channel slices, which the other tests check."""
    from materialrefgs_amd.renderer import _SurfelComposite
    from materialrefgs_amd.shading import EnvLight, get_specular_color_surfel, shade_and_composite_surfel
    from materialrefgs_amd.synthetic import orbit_camera
    H, W = 40, 56
    g = torch.Generator().manual_seed(21)
    cam = orbit_camera(3, H, W).to(gpu_device)
    env = EnvLight(device=gpu_device, min_res=4, max_res=16, trainable=True)
    with torch.no_grad():
        env.base.copy_(torch.randn(6, 16, 16, 3, generator=g).to(gpu_device))
    vals = dict(base=torch.rand(3, H, W, generator=g), feat=torch.rand(8, H, W, generator=g),
                nmap=torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1), alpha=torch.rand(1, H, W, generator=g))
    bg = torch.tensor([0.2, 0.4, 0.6], device=gpu_device)
    ups = [torch.randn(3, H, W, generator=g).to(gpu_device) for _ in range(3)]
    res = []
    for fused in (True, False):
        t = {k: v.to(gpu_device).clone().requires_grad_(True) for k, v in vals.items()}
        env.base.grad = None
        env.build_mips()
        if fused:
            render, diffuse, spec, _ = shade_and_composite_surfel(env, t["base"], t["feat"], cam.HWK, cam.R, cam.T, t["nmap"], t["alpha"], bg, srgb)
        else:
            f = t["feat"]
            spec, _ = get_specular_color_surfel(env, f[2:5].permute(1, 2, 0), cam.HWK, cam.R, cam.T, t["nmap"], t["alpha"].permute(1, 2, 0),
                                                refl_strength=f[0:1].permute(1, 2, 0), roughness=f[1:2].permute(1, 2, 0))
            render, diffuse = _SurfelComposite.apply(t["base"], f[0:1], spec, t["alpha"], bg, srgb)
        torch.autograd.backward([render, diffuse, spec], ups)
        res.append(([render, diffuse, spec], [t[k].grad for k in ("base", "feat", "nmap", "alpha")] + [env.base.grad.clone()]))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(res[0][1], res[1][1]):
        assert float((a - b).abs().max()) <= 1e-5 * max(1e-6, float(b.abs().max()))


@pytest.mark.gpu
def test_surfel_factored_sh_exchange_equals_the_dense_sum(gpu_device):
    """mrgs_sh_grad_expand_surfel on the real gradients of render_surfel from three views: the four SH gradient tensors rebuilt
    from 6 floats per gaussian and the camera centres equal the sum of the per-view dense gradients."""
    from types import SimpleNamespace
    from materialrefgs_amd import dist as mdist
    from materialrefgs_amd.renderer import SurfelModel, render_surfel
    from materialrefgs_amd.shading import EnvLight
    from materialrefgs_amd.synthetic import make_shell_scene, orbit_camera
    P, H, W = 4000, 96, 128
    sc = make_shell_scene(P, S=0, seed=2, radius_px=6.0, image_size=128).to(gpu_device)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(gpu_device)   # noqa: E731
    env = EnvLight(device=gpu_device, trainable=True)
    with torch.no_grad():
        env.base.copy_(rnd(6, 128, 128, 3))
    env.build_mips()
    inv_sig = lambda x: torch.log(x / (1 - x))   # noqa: E731
    pc = SurfelModel(sc.means3D.clone(), torch.log(sc.scales), sc.rotations.clone() * 1.7, inv_sig(sc.opacities.clamp(1e-4, 1 - 1e-4)),
                     sc.shs[:, :1].clone(), sc.shs[:, 1:].clone(), refl_strength=rnd(P, 1), roughness=rnd(P, 1), ori_color=rnd(P, 3),
                     indirect_dc=rnd(P, 1, 3) * 0.3, indirect_rest=rnd(P, 15, 3) * 0.1, envmap=env, active_sh_degree=2)
    for t in pc.parameters():
        t.requires_grad_(True)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False)
    bg = torch.zeros(3, device=gpu_device)
    # the indirect radiance only reaches the image through the visibility blend: give the model an occluder
    from materialrefgs_amd.raytracing import RayTracer
    from materialrefgs_amd.synthetic import sphere_mesh
    v1, t1 = sphere_mesh(16, 24, 0.9)
    v2, t2 = sphere_mesh(12, 16, 1.2, centre=(0.0, 2.6, 0.5))
    pc.ray_tracer = RayTracer(np.concatenate([v1, v2]), np.concatenate([t1, t2 + len(v1)]), device=gpu_device)
    names = ("features_dc", "features_rest", "indirect_dc", "indirect_rest")
    dense = {n: 0 for n in names}
    rows = []
    for view in range(3):
        cam = orbit_camera(view, H, W).to(gpu_device)
        for t in pc.parameters():
            t.grad = None
        out = render_surfel(cam, pc, pipe, bg, srgb=False, opt=SimpleNamespace(indirect=True))
        (out["render"] * torch.linspace(0.5, 1.5, W, device=gpu_device)).sum().backward()
        gr = {"features_dc": pc._features_dc.grad, "features_rest": pc._features_rest.grad, "indirect_dc": pc._indirect_dc.grad,
              "indirect_rest": pc._indirect_rest.grad}
        for n in names:
            dense[n] = dense[n] + gr[n]
        rows.append(torch.cat([(gr["features_dc"][:, 0, :] / mdist.SH_C0).reshape(-1), (gr["indirect_dc"][:, 0, :] / mdist.SH_C0).reshape(-1),
                               cam.camera_center.reshape(-1)]))
    gathered = torch.stack(rows).contiguous()
    got = mdist.expand_surfel_sh_gradients(gathered, pc._xyz, pc._rotation, 2)
    assert float(dense["indirect_rest"].abs().max()) > 0 and float(dense["features_rest"].abs().max()) > 0
    assert float(dense["features_rest"][:, 8:].abs().max()) == 0          # active degree 2: coefficients 9..15 untouched
    for n, t in zip(names, got):
        scale = float(dense[n].abs().max())
        assert float((t - dense[n]).abs().max()) < 3e-5 * scale, n


@pytest.mark.gpu
@pytest.mark.parametrize("res,steps", [(128, 3), (64, 3), (32, 2), (16, 1)])
def test_mip_chain_in_one_launch_equals_the_level_by_level_kernel(gpu_device, res, steps):
    """mrgs_cubemap_mip_chain_forward (three levels per launch; four lanes per coarsest texel for a full three-level chain) writes the very
    values mrgs_cubemap_mip_forward produces level by level: the same 2x2 sums in the same order."""
    import ctypes
    from materialrefgs_amd import _lib
    from materialrefgs_amd.shading import _mip_forward
    g = torch.Generator().manual_seed(res + steps)
    base = torch.randn(6, res, res, 3, generator=g).to(gpu_device)
    ref, cur = [], base
    for _ in range(steps):
        cur = _mip_forward(cur)
        ref.append(cur)
    outs = [torch.empty_like(r) for r in ref]
    ptrs = (ctypes.c_void_p * steps)(*[t.data_ptr() for t in outs])
    _lib.check(_lib.lib().mrgs_cubemap_mip_chain_forward(res, steps, base.data_ptr(), ptrs, _lib.stream_ptr(gpu_device)))
    torch.cuda.synchronize(gpu_device)
    for a, b in zip(outs, ref):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("res,levels", [(128, 4), (64, 4), (32, 3), (16, 2), (8, 1)])
def test_mip_backward_chain_in_one_launch_equals_the_level_by_level_kernel(gpu_device, res, levels):
    """mrgs_cubemap_mip_chain_backward accumulates the very values mrgs_cubemap_mip_backward produces level by level, coarse to fine --
    repeatedly, on two streams at once.  (The test was written for a one-launch form of the chain that waited between its levels on device
    counters: it passed, and the launch took 91 us against 20 -- DESIGN section 9; the call is a launch per level again.)"""
    import ctypes
    from materialrefgs_amd import _lib
    from materialrefgs_amd.shading import _mip_backward_accumulate
    g = torch.Generator().manual_seed(res * 10 + levels)
    gl = [torch.randn(6, res >> k, res >> k, 3, generator=g).to(gpu_device) for k in range(levels)]
    ref = [t.clone() for t in gl]
    for k in range(levels - 2, -1, -1):
        _mip_backward_accumulate(ref[k + 1], ref[k])
    side = torch.cuda.Stream(device=gpu_device)
    for rep in range(6):
        outs = [[t.clone() for t in gl] for _ in range(2)]
        torch.cuda.synchronize(gpu_device)
        for o, st in zip(outs, (torch.cuda.current_stream(gpu_device), side)):
            ptrs = (ctypes.c_void_p * levels)(*[t.data_ptr() for t in o])
            with torch.cuda.stream(st):
                _lib.check(_lib.lib().mrgs_cubemap_mip_chain_backward(res, levels, ptrs, ctypes.c_void_p(st.cuda_stream)))
        torch.cuda.synchronize(gpu_device)
        for o in outs:
            for a, b in zip(o, ref):
                assert torch.equal(a, b), (rep, tuple(a.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("max_res,min_res", [(128, 16), (64, 16), (64, 8)])
def test_build_mips_with_symmetric_tiles_equals_the_full_matrices(gpu_device, monkeypatch, max_res, min_res):
    """EnvLight.build_mips end to end -- every prefiltered level and the gradient of the base texels -- with the long-row levels applied from
    the dense tiles of one fundamental domain (the default) against the same chain on the full matrices (the MRGS_NO_SYMMETRIC_SPMV switch),
    for the reference's default chain and two shorter ones."""
    import materialrefgs_amd.shading as sh
    g = torch.Generator().manual_seed(max_res + min_res)
    base = torch.rand(6, max_res, max_res, 3, generator=g)
    ups = None
    res = {}
    for mode in ("sym", "full"):
        monkeypatch.setattr(sh, "_NO_SYM", mode == "full")
        monkeypatch.setattr(sh.CubemapFilterOp, "_cache", {})
        sh._SPMV_DESCS.clear()
        env = sh.EnvLight(device=gpu_device, min_res=min_res, max_res=max_res, trainable=True)
        with torch.no_grad():
            env.base.copy_(base.to(gpu_device))
        env.build_mips()
        ops = list(sh.CubemapFilterOp._cache.values())
        assert any(o.sym is not None for o in ops) == (mode == "sym")
        spec = [m for m in env.specular]
        if ups is None:
            ups = [torch.randn(m.shape, generator=g).to(gpu_device) for m in spec]
        torch.autograd.backward(spec, ups)
        res[mode] = ([m.detach().clone() for m in spec], env.base.grad.detach().clone())
    for a, b in zip(res["sym"][0], res["full"][0]):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    ga, gb = res["sym"][1], res["full"][1]
    assert float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max())
    sh._SPMV_DESCS.clear()


def test_cube_symmetry_rows_form_the_octahedral_group():
    """mrgs_cube_symmetry_rows (host code of the library): 48 distinct permutations of the texels, the identity first, closed under composition
    and under inversion -- the symmetry group of the cube acting on the texel grid -- and consistent between resolutions (the image of a
    texel of the 2N grid lies in the image of the N-grid texel that contains it)."""
    from materialrefgs_amd import shading as sh
    for N in (4, 8):
        P = sh._cube_symmetry_rows(N).long().numpy()
        n = 6 * N * N
        assert P.shape == (48, n) and np.array_equal(P[0], np.arange(n))
        keys = {p.tobytes(): g for g, p in enumerate(P)}
        assert len(keys) == 48
        inv = np.empty_like(P)
        for g in range(48):
            inv[g][P[g]] = np.arange(n)
            assert inv[g].tobytes() in keys
        for g1 in range(0, 48, 5):
            for g2 in range(48):
                assert P[g1][P[g2]].tobytes() in keys
    P4, P8 = sh._cube_symmetry_rows(4).long().numpy(), sh._cube_symmetry_rows(8).long().numpy()
    t = np.arange(6 * 64)
    parent = lambda idx, N: ((idx // (N * N)) * (N // 2) + ((idx // N) % N) // 2) * (N // 2) + (idx % N) // 2      # texel of the N/2 grid that contains it
    for g in range(48):
        assert np.array_equal(parent(P8[g][t], 8), P4[g][parent(t, 8)])


def test_split_channels_only_takes_over_a_stack_it_was_given():
    """renderer._SplitChannels.backward reuses the base of its head gradient as its own output ONLY when that base is the very tensor
    shading._SurfelShade.backward left for it on the call's hand-off object: a head gradient that is a view into somebody else's [S,H,W]
    tensor -- torch.cat of the eight maps with another branch's maps hands out exactly that -- is copied from, and the other branch's rows
    stay what they were (CPU: pure torch)."""
    from materialrefgs_amd import shading as sh
    from materialrefgs_amd.renderer import _SplitChannels
    H, W = 4, 5
    maps = torch.randn(12, H, W, requires_grad=True)
    decoy = sh.GradStackHandoff(12)
    head, one = _SplitChannels.apply(maps, 8, True, decoy)
    decoy.stack = torch.zeros(12, H, W)             # a stack is on offer, but the head gradient below is not a view of IT
    other = torch.randn(4, H, W, requires_grad=True)
    torch.cat((head, other * 2.0)).mul(torch.arange(12.0).reshape(12, 1, 1)).sum().backward()     # head's gradient: rows 0..7 of a [12,H,W] tensor
    assert torch.equal(other.grad, (2.0 * torch.arange(8.0, 12.0)).reshape(4, 1, 1).expand(4, H, W))
    assert torch.equal(maps.grad[:8], torch.arange(8.0).reshape(8, 1, 1).expand(8, H, W)) and float(maps.grad[8].abs().max()) == 0.0
    # ... and the stack the hand-off object holds IS taken over (no copy): the returned gradient is that very memory
    stack = torch.zeros(12, H, W)
    stack[:8] = 3.0
    handoff = sh.GradStackHandoff(12)
    maps2 = torch.randn(12, H, W, requires_grad=True)
    returned = []
    maps2.register_hook(returned.append)
    h2, o2 = _SplitChannels.apply(maps2, 8, True, handoff)
    handoff.stack = stack                            # what _SurfelShade.backward does with the stack it allocated for this node
    torch.autograd.backward([h2, o2], [stack[:8], torch.full((1, H, W), 5.0)], retain_graph=True)
    assert float(stack[8].min()) == 5.0 and handoff.stack is None          # written in place, the mark consumed
    assert len(returned) == 1 and returned[0].data_ptr() == stack.data_ptr() and tuple(returned[0].shape) == (12, H, W)
    assert torch.equal(maps2.grad[:8], torch.full((8, H, W), 3.0)) and torch.equal(maps2.grad[8], torch.full((H, W), 5.0))
    # consumed exactly once: the same head gradient again, nothing on offer any more -> copied from, the stack stays as it is
    torch.autograd.backward([h2, o2], [stack[:8], torch.full((1, H, W), 7.0)])
    assert len(returned) == 2 and returned[1].data_ptr() != stack.data_ptr() and handoff.stack is None
    assert float(stack[8].min()) == 5.0 and float(stack[8].max()) == 5.0 and torch.equal(returned[1][8], torch.full((H, W), 7.0))


def test_blocked_float64_prefilter_operator_equals_the_dense_one():
    """oracle/envfilter_oracle.BlockedSpecular (what the full-size checks apply at 128^2 and 64^2, where the dense operator does not fit)
    against the dense operator of the same level at 32^2, both directions; and build_mips / build_mips_backward give the same levels
    and base gradient whichever form carries the 32^2 level."""
    from oracle import envfilter_oracle as eo
    rng = np.random.default_rng(5)
    P = eo.specular_matrix(32, 0.08)
    B = eo.BlockedSpecular(32, 0.08, device="cpu", block=512)
    x = rng.normal(size=(6 * 32 * 32, 3))
    assert np.abs(B.matvec(x) - P @ x).max() < 1e-12 and np.abs(B.rmatvec(x) - P.T @ x).max() < 1e-12
    base = rng.normal(size=(6, 32, 32, 3))
    spec_d, _, ops_d = eo.build_mips(base, 8)
    ops_b = [B] + list(ops_d[1:])
    ups = [rng.normal(size=s_.shape) for s_ in spec_d]
    assert np.abs(ops_b[0].matvec(base).reshape(base.shape) - spec_d[0]).max() < 1e-12
    assert np.abs(eo.build_mips_backward(ops_b, ups) - eo.build_mips_backward(ops_d, ups)).max() < 1e-12


def test_symmetric_rows_refuse_a_panel_longer_than_the_kernel_takes(monkeypatch):
    """CubemapFilterOp._symmetric returns None (the caller then keeps the full matrices) when a tile's panel has more patches than a
    workgroup of the product kernel walks (MRGS_SPMV_MAX_PANEL): checked with the limit lowered under the 16 x 16 level's panels."""
    from oracle import envfilter_oracle as eo
    from materialrefgs_amd import shading as sh
    N = 16
    n = 6 * N * N
    A = eo.diffuse_matrix(N)
    r, c = np.nonzero(A)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])).to(torch.int32)
    col, val = torch.from_numpy(c).to(torch.int32), torch.from_numpy(A[r, c]).float()
    op = object.__new__(sh.CubemapFilterOp)
    op.res, op.nrows = N, n
    area = torch.from_numpy(sh._pixel_area(N))
    ones = torch.ones(n)
    full = op._symmetric(ptr, col, val, 1.0 / area, area, ones)
    assert full is not None and 1 < full.max_panel <= sh._SYM_MAX_PANEL
    monkeypatch.setattr(sh, "_SYM_MAX_PANEL", full.max_panel - 1)
    assert op._symmetric(ptr, col, val, 1.0 / area, area, ones) is None
