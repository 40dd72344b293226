"""cubemapencoder fetch primitive (north star; SURVEY 8a row 9 / VERDICT a-12): the HIP kernels against the numpy restatement of
submodules/cubemapencoder/src/cubemapencoder.cu, plus known answers of the restatement itself; the two modules' forward and backward,
their input handling, state_dict keys and level sizes.  (The checks that need no restatement are in test_cubemap_seams.py.)"""
import numpy as np
import pytest
import torch

from oracle import cubemap_encoder_oracle as co


def _dirs(n, seed, L):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    # force every seam class: points right at face edges and at cube vertices, axis directions, a zero vector (fail value)
    e = 1.0 - 0.3 / L
    special = np.array([[1, e, 0.2], [1, -e, 0.1], [1, 0.3, e], [-1, 0.3, -e], [e, 1, 0.2], [0.1, -1, e], [0.2, e, 1], [e, 0.1, -1],
                        [1, e, e], [1, -e, e], [-1, e, -e], [e, 1, e], [-e, -1, e], [e, e, 1], [-e, e, -1], [1, 0, 0], [0, -1, 0], [0, 0, 1],
                        [0, 0, 0], [1, 1, 1], [-1, -1, -1]], dtype=np.float64)
    return np.concatenate([special, d]).astype(np.float32)


def boundary_count(dirs, L, interp):
    """How many directions sit where fp32 and fp64 may pick different taps: a pixel coordinate pu or pv (float64) within 1e-5 L of an
    integer (nearest: the truncation) or of an integer + 0.5 (bilinear: the floor of p - 0.5).  The direction seeds of the parity
    cases below were chosen on the CPU so that this count is at most 3 (nearest) or 0.5 % of B (bilinear): the caps of
    _compare_with_restatement are then conditions the inputs respect by themselves.  Not counted: the zero vector, and the specials
    whose components are all 0 or +-1 (the axes and the two diagonals) -- their u, v are 0 or +-1 and their pixel coordinates 0, L/2 or
    L in fp32 and in fp64 alike, so they cannot flip although they sit on a boundary by construction."""
    d = np.asarray(dirs, np.float64)
    d = d[~np.isin(d, (0.0, 1.0, -1.0)).all(1)]
    pu, pv = co.pixel_coords(d, L)
    off = 0.0 if interp == 0 else 0.5
    near = lambda p: np.abs((p - off) - np.round(p - off)) < 1e-5 * L
    return int((near(pu) | near(pv)).sum())


def test_oracle_known_answers():
    """Texel-centre directions return that texel (all modes); a constant map returns the constant, also across seams and at
    vertices; bilinear weights sum to one; the seamless fetch is continuous across an edge where the plain one is not."""
    L, C = 8, 2
    rng = np.random.default_rng(0)
    cm = rng.normal(size=(6, C, L, L))
    fail = np.array([7.0, -3.0])
    # texel centres of face 4 (+z): u = x/z, v = -y/z (:176-181) -> pixel (u*.5+.5)L, (-v*.5+.5)L with LEFT_TOP
    ys, xs = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    u = (xs + 0.5) / L * 2 - 1
    vv = (ys + 0.5) / L * 2 - 1            # pixel row = (-v * .5 + .5) L  =>  v_uv = -(row centre)
    d = np.stack([u, vv, np.ones_like(u)], -1).reshape(-1, 3)      # y = -v_uv * z with v_uv = -vv ... face 4: v = y/z then negated
    for interp, seam in ((0, 0), (1, 0), (1, 1)):
        out = co.encode(d, cm, fail, interp, seam)
        np.testing.assert_allclose(out, cm[4].reshape(C, -1), atol=1e-12)
    const = np.full((6, C, L, L), 2.5)
    dirs = _dirs(500, 1, L)
    out = co.encode(dirs, const, fail, 1, 1)
    nz = np.any(dirs != 0, axis=1)
    np.testing.assert_allclose(out[:, nz], 2.5, atol=1e-12)
    np.testing.assert_allclose(out[:, ~nz], fail[:, None] * np.ones((1, int((~nz).sum()))))
    # continuity across the +x / +y edge
    eps = 1e-6
    a = co.encode(np.array([[1.0, 1.0 - eps, 0.3]]), cm, fail, 1, 1)
    b = co.encode(np.array([[1.0 - eps, 1.0, 0.3]]), cm, fail, 1, 1)
    assert np.abs(a - b).max() < 1e-4
    a0 = co.encode(np.array([[1.0, 1.0 - eps, 0.3]]), cm, fail, 1, 0)
    b0 = co.encode(np.array([[1.0 - eps, 1.0, 0.3]]), cm, fail, 1, 0)
    assert np.abs(a0 - b0).max() > 1e-2


def test_oracle_backward_is_the_derivative_of_its_forward():
    L, C = 6, 3
    rng = np.random.default_rng(3)
    cm = rng.normal(size=(6, C, L, L))
    fail = rng.normal(size=C)
    dirs = _dirs(40, 5, L).astype(np.float64)
    dirs = dirs[np.any(dirs != 0, axis=1)]
    dirs += 1e-3 * rng.normal(size=dirs.shape)                      # off the exact seams: the fetch is piecewise smooth
    go = rng.normal(size=(C, len(dirs)))
    out, g_in, g_cm, g_fail = co.encode(dirs, cm, fail, 1, 1, go)
    loss = lambda dd, cc: float((co.encode(dd, cc, fail, 1, 1) * go).sum())
    h = 1e-6
    for n in range(0, len(dirs), 3):
        for k in range(3):
            dp, dm = dirs.copy(), dirs.copy()
            dp[n, k] += h; dm[n, k] -= h
            fd = (loss(dp, cm) - loss(dm, cm)) / (2 * h)
            assert abs(fd - g_in[n, k]) < 1e-4 * max(1.0, abs(fd)), (n, k, fd, g_in[n, k])
    idx = np.argwhere(np.abs(g_cm) > 0)[::17][:20]
    for f, c, y, x in idx:
        cp, cq = cm.copy(), cm.copy()
        cp[f, c, y, x] += h; cq[f, c, y, x] -= h
        fd = (loss(dirs, cp) - loss(dirs, cq)) / (2 * h)
        assert abs(fd - g_cm[f, c, y, x]) < 1e-6 * max(1.0, abs(fd))


def test_shim_package_and_cpu_rejection():
    import cubemapencoder
    from materialrefgs_amd import cubemap_encoder as ce
    assert cubemapencoder.CubemapEncoder is ce.CubemapEncoder and cubemapencoder.cubemap_encode is ce.cubemap_encode
    enc = ce.CubemapEncoder(output_dim=3, resolution=8)
    assert tuple(enc.params['Cubemap_texture'].shape) == (6, 3, 8, 8) and tuple(enc.params['Cubemap_failv'].shape) == (3,)
    mip = ce.MipCubemapEncoder(num_levels=3, level_dim=2, per_level_scale=2, base_resolution=4)
    assert [tuple(p.shape) for p in mip.params_list] == [(6, 2, 4, 4), (6, 2, 8, 8), (6, 2, 16, 16)] and mip.output_dim == 6
    with pytest.raises(RuntimeError, match="CUDA"):
        enc(torch.randn(4, 3))


def _compare_with_restatement(gpu_device, interp, seamless, cm, fail, dirs, go):
    """cubemap_encode on the GPU against the restatement: forward, grad_cubemap, grad_fail, and the direction gradient where the tap
    sets agree.  The caps (3 flipped samples in nearest mode, none in bilinear, 99.5 % of the direction gradients) are conditions."""
    from materialrefgs_amd.cubemap_encoder import cubemap_encode
    C = cm.shape[1]
    out_o, gi_o, gc_o, gf_o = co.encode(dirs, cm, fail, interp, seamless, go)
    t = lambda a: torch.tensor(a, device=gpu_device, requires_grad=True)
    td, tc, tf = t(dirs), t(cm), t(fail)
    out = cubemap_encode(td, tc, tf, interp, seamless)
    assert tuple(out.shape) == (C, len(dirs))
    # a direction whose pixel coordinate lands within rounding of a texel boundary may pick the neighbouring tap set in fp32: the
    # bilinear value is continuous there (same result), the nearest one is not -- allow a handful of such samples for nearest only
    d = np.abs(out.detach().cpu().numpy() - out_o)
    bad = (d > 2e-5 * max(1.0, np.abs(out_o).max())).any(0)
    assert bad.sum() <= (3 if interp == 0 else 0), int(bad.sum())
    out.backward(torch.tensor(go, device=gpu_device))
    ok = ~bad
    if interp == 1:
        a, b = td.grad.cpu().numpy(), gi_o
        # the direction gradient is the slope of the bilinear patch: discontinuous across texel boundaries, so compare where the
        # fp32 and fp64 tap sets agree (everywhere except samples within rounding of a boundary)
        close = np.abs(a - b).max(1) <= 2e-3 * max(1.0, np.abs(b).max())
        assert close.mean() > 0.995, float(close.mean())
    else:
        assert float(td.grad.abs().max()) == 0.0
    np.testing.assert_allclose(tf.grad.cpu().numpy(), gf_o, rtol=1e-5, atol=1e-5)
    if not bad.any():
        scale = max(1.0, float(np.abs(gc_o).max()))
        assert float(np.abs(tc.grad.cpu().numpy() - gc_o).max()) <= 1e-4 * scale
    assert ok.sum() > 0


def _restatement_case(gpu_device, interp, seamless, L, C, dirs):
    rng = np.random.default_rng(L + C)
    cm = rng.normal(size=(6, C, L, L)).astype(np.float32)
    fail = rng.normal(size=C).astype(np.float32)
    go = rng.normal(size=(C, len(dirs))).astype(np.float32)
    _compare_with_restatement(gpu_device, interp, seamless, cm, fail, dirs, go)


@pytest.mark.gpu
@pytest.mark.parametrize("interp,seamless", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("L,C", [(8, 3), (33, 6)])
def test_hip_cubemap_encode_matches_the_restatement(gpu_device, interp, seamless, L, C):
    _restatement_case(gpu_device, interp, seamless, L, C, _dirs(3000, 2, L))


def _checked_dirs(dirs, L, interp):
    """`dirs`, after asserting that their seed respects the rule of boundary_count."""
    n, cap = boundary_count(dirs, L, interp), (3 if interp == 0 else 0.005 * len(dirs))
    assert n <= cap, (n, cap)
    return dirs


@pytest.mark.gpu
@pytest.mark.parametrize("interp,seamless", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("C", [1, 6])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_hip_cubemap_encode_matches_the_restatement_at_small_levels(gpu_device, interp, seamless, L, C):
    """The smallest levels of a pyramid: at L = 1 every seamless sample is a vertex sample, at L = 2 every off-centre one crosses an
    edge.  Direction seed 2: boundary_count is 0 in both rules at each of these L (1 at L = 3, bilinear, with seed 0)."""
    _restatement_case(gpu_device, interp, seamless, L, C, _checked_dirs(_dirs(1000, 2, L), L, interp))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_hip_cubemap_encode_matches_the_restatement_at_workgroup_edges(gpu_device, B):
    """One sample, and one below / at / above the 256-lane workgroup.  The specials are cut to fit; whenever B > 1 the zero vector is
    among them.  Direction seed 2: boundary_count is 0 at each B."""
    L, C = 16, 3
    dirs = _dirs(max(B - 21, 0), 2, L)[:B]
    assert len(dirs) == B and (B == 1 or (dirs == 0).all(1).sum() == 1)
    _restatement_case(gpu_device, 1, 1, L, C, _checked_dirs(dirs, L, 1))


@pytest.mark.gpu
def test_hip_cubemap_encode_matches_the_restatement_at_the_default_level(gpu_device):
    """The reference's default CubemapEncoder / top pyramid level: L = 256, C = 6, seamless.  Direction seed 146: the first seed whose
    boundary_count, 15, is within 0.5 % of B = 3021 (the rule's window, 1e-5 L, is 2.6e-3 of a texel here and holds ~1 % of random
    directions: seed 2 has 26)."""
    L, C = 256, 6
    _restatement_case(gpu_device, 1, 1, L, C, _checked_dirs(_dirs(3000, 146, L), L, 1))


MANY_SEED = 2        # boundary_count (nearest rule) of the 65 537 random directions: 3, the first seed within the cap


@pytest.mark.gpu
def test_hip_many_samples_on_one_texel_lose_no_update(gpu_device):
    """65 537 nearest samples on the 24 texels of an L = 2, C = 1 map whose texel values are their own linear index, plus 300 zero
    vectors: the forward returns the fetched ids exactly; with go = 1 grad_cubemap is the histogram of those ids and grad_fail is 300,
    exactly -- the counts are integers below 2^24, every fp32 atomic add is exact, so one lost or doubled update shows.  The ids are the
    restatement's but for at most 3 samples (the nearest cap)."""
    from materialrefgs_amd.cubemap_encoder import cubemap_encode
    L, n_rand, n_zero = 2, 65537, 300
    rng = np.random.default_rng(MANY_SEED)
    dirs = np.concatenate([rng.normal(size=(n_rand, 3)), np.zeros((n_zero, 3))]).astype(np.float32)
    _checked_dirs(dirs, L, 0)
    cm = np.arange(24, dtype=np.float32).reshape(6, 1, L, L)
    fail = np.array([-1.0], np.float32)
    ids_o = co.encode(dirs, cm, fail, 0, 0)[0]
    t = lambda a: torch.tensor(a, device=gpu_device, requires_grad=True)
    td, tc, tf = t(dirs), t(cm), t(fail)
    out = cubemap_encode(td, tc, tf, 0, 0)
    ids = out.detach().cpu().numpy()[0]
    assert np.array_equal(ids[n_rand:], np.full(n_zero, -1.0)) and np.array_equal(ids[:n_rand], np.round(ids[:n_rand]))
    assert ids[:n_rand].min() >= 0 and ids[:n_rand].max() <= 23
    assert int((ids != ids_o).sum()) <= 3, int((ids != ids_o).sum())
    out.backward(torch.ones_like(out))
    hist = np.bincount(ids[:n_rand].astype(np.int64), minlength=24)
    assert hist.min() > 1000                                        # every texel takes thousands of colliding updates
    assert np.array_equal(tc.grad.cpu().numpy().reshape(-1), hist.astype(np.float32))
    assert float(tf.grad.item()) == float(n_zero)
    assert float(td.grad.abs().max()) == 0.0


# ---- the two modules ------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


@pytest.mark.gpu
@pytest.mark.parametrize("interpolation,seamless", [("linear", True), ("nearest", True), ("linear", 0), ("linear", False)])
def test_cubemap_encoder_module_forward_and_backward(gpu_device, interpolation, seamless):
    """CubemapEncoder.forward: leading batch dimensions, the sigmoid, the interpolation and `seamless` switches (an int in the
    reference, a bool here: both are given).  Direction seed 4: boundary_count is 0 in both rules, so nearest cannot flip either."""
    from materialrefgs_amd.cubemap_encoder import CubemapEncoder
    L, C = 8, 3
    interp, seam = (0 if interpolation == "nearest" else 1), (1 if seamless else 0)
    rng = np.random.default_rng(4)
    dirs = rng.normal(size=(5, 7, 3)).astype(np.float32)
    dirs[2, 3] = 0.0
    assert boundary_count(dirs.reshape(-1, 3), L, 0) == 0 and boundary_count(dirs.reshape(-1, 3), L, 1) == 0
    tex = rng.uniform(-5, 5, size=(6, C, L, L)).astype(np.float32)
    failv = rng.normal(size=C).astype(np.float32)
    go = rng.normal(size=(5, 7, 3)).astype(np.float32)
    enc = CubemapEncoder(output_dim=C, resolution=L, interpolation=interpolation).to(gpu_device)
    enc.seamless = seamless
    with torch.no_grad():
        enc.params['Cubemap_texture'].copy_(torch.tensor(tex))
        enc.params['Cubemap_failv'].copy_(torch.tensor(failv))
    out = enc(torch.tensor(dirs, device=gpu_device))
    assert tuple(out.shape) == (5, 7, 3) and out.dtype == torch.float32
    raw = co.encode(dirs.reshape(-1, 3), tex, failv, interp, seam)                      # [C, B]
    sig = _sigmoid(raw)
    assert float(np.abs(out.detach().cpu().numpy().reshape(-1, 3) - sig.T).max()) <= 2e-5
    assert abs(float(out.detach()[2, 3, 0]) - _sigmoid(float(failv[0]))) <= 2e-5             # the zero vector fetched the fail value
    out.backward(torch.tensor(go, device=gpu_device))
    go_raw = go.reshape(-1, 3).T.astype(np.float64) * sig * (1.0 - sig)                 # through the sigmoid, in float64
    _, _, gc_o, gf_o = co.encode(dirs.reshape(-1, 3), tex, failv, interp, seam, go_raw)
    for name, want in (("Cubemap_texture", gc_o), ("Cubemap_failv", gf_o)):
        got = enc.params[name].grad.cpu().numpy()
        assert np.abs(want).max() > 0 and float(np.abs(got - want).max()) <= 1e-4 * float(np.abs(want).max()), name


@pytest.mark.gpu
@pytest.mark.parametrize("concat", [True, False])
def test_mip_cubemap_encoder_module_forward_and_backward(gpu_device, concat):
    """MipCubemapEncoder.forward over levels 2, 4, 8: level-major columns when concatenated ([B, 6]: torch.cat over [C, B] along dim 0,
    then the permute, reference :151-160), the sum otherwise ([B, 2]); one fail value shared by the levels, its gradient their sum;
    each level's gradient the restatement's for that level.  Tolerances of _compare_with_restatement.  Direction seed 3:
    boundary_count (bilinear rule) is 0 at each of the three levels."""
    from materialrefgs_amd.cubemap_encoder import MipCubemapEncoder
    levels, C = [2, 4, 8], 2
    dirs = _dirs(279, 3, 8)                                                             # 300 samples: two workgroups, one zero vector
    B = len(dirs)
    assert all(boundary_count(dirs, L, 1) == 0 for L in levels)
    rng = np.random.default_rng(12)
    texs = [rng.normal(size=(6, C, L, L)).astype(np.float32) for L in levels]
    failv = rng.normal(size=C).astype(np.float32)
    mip = MipCubemapEncoder(num_levels=3, level_dim=C, per_level_scale=2, base_resolution=2, concat=concat).to(gpu_device)
    assert [int(p.shape[-1]) for p in mip.params_list] == levels
    with torch.no_grad():
        for p, tex in zip(mip.params_list, texs):
            p.copy_(torch.tensor(tex))
        mip.fail_value.copy_(torch.tensor(failv))
    out = mip(torch.tensor(dirs, device=gpu_device))
    assert tuple(out.shape) == ((B, 6) if concat else (B, 2)) and mip.output_dim == out.shape[1]
    go = rng.normal(size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.tensor(go, device=gpu_device))
    per_level = []
    for i, tex in enumerate(texs):
        go_i = (go[:, C * i:C * (i + 1)] if concat else go).T                          # [C, B] reaching level i
        per_level.append(co.encode(dirs, tex, failv, 1, 1, go_i))
    want = np.concatenate([r[0] for r in per_level]).T if concat else sum(r[0] for r in per_level).T
    assert float(np.abs(out.detach().cpu().numpy() - want).max()) <= 2e-5 * max(1.0, float(np.abs(want).max()))
    for p, r in zip(mip.params_list, per_level):
        assert float(np.abs(p.grad.cpu().numpy() - r[2]).max()) <= 1e-4 * max(1.0, float(np.abs(r[2]).max()))
    gf = sum(r[3] for r in per_level)
    assert np.abs(gf).max() > 0
    np.testing.assert_allclose(mip.fail_value.grad.cpu().numpy(), gf, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_cubemap_encode_input_handling(gpu_device):
    """What the reference's custom_fwd(cast_inputs=torch.float32) gives: float64, half and non-contiguous directions fetch what the
    float32 contiguous tensor of the same (for half: rounded) values fetches, bit for bit, forward and backward; B = 0 gives an empty
    [0, out_dim] output whose backward leaves zero parameter gradients."""
    from materialrefgs_amd.cubemap_encoder import CubemapEncoder, MipCubemapEncoder, cubemap_encode
    L, C, B = 8, 3, 300
    rng = np.random.default_rng(21)
    cm = torch.tensor(rng.normal(size=(6, C, L, L)).astype(np.float32), device=gpu_device)
    fail = torch.tensor(rng.normal(size=C).astype(np.float32), device=gpu_device)
    go = torch.tensor(rng.normal(size=(C, B)).astype(np.float32), device=gpu_device)
    d64 = rng.normal(size=(B, 3))
    d64[7] = 0.0

    def run(d):
        d = d.clone().requires_grad_(True)
        tc, tf = cm.clone().requires_grad_(True), fail.clone().requires_grad_(True)
        out = cubemap_encode(d, tc, tf, 1, 1)
        assert out.dtype == torch.float32
        out.backward(go)
        return out.detach(), d.grad, tc.grad, tf.grad

    def same(a, b):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].float(), b[1].float()) and torch.equal(a[3], b[3])
        assert float((a[2] - b[2]).abs().max()) <= 1e-6 * float(b[2].abs().max())      # atomics reorder

    t64 = torch.tensor(d64, device=gpu_device)
    assert (t64.float().double() != t64).any()                                          # values that float32 does round
    r64 = run(t64)
    assert r64[1].dtype == torch.float64
    same(r64, run(t64.float()))
    t16 = t64.half()
    r16 = run(t16)
    assert r16[1].dtype == torch.float16
    ref16 = run(t16.float())
    assert torch.equal(r16[0], ref16[0]) and torch.equal(r16[3], ref16[3]) and torch.equal(r16[1], ref16[1].half())
    # a [B, 4][:, :3] view: rows 16 bytes apart
    base = torch.zeros(B, 4, device=gpu_device)
    base[:, :3] = t64.float()
    base[:, 3] = 99.0
    base.requires_grad_(True)
    tc = cm.clone().requires_grad_(True)
    view = base[:, :3]
    assert not view.is_contiguous()
    out = cubemap_encode(view, tc, fail, 1, 1)
    out.backward(go)
    ref = run(t64.float())
    assert torch.equal(out.detach(), ref[0]) and torch.equal(base.grad[:, :3], ref[1]) and float(base.grad[:, 3].abs().max()) == 0.0
    # no samples
    enc = CubemapEncoder(output_dim=3, resolution=4).to(gpu_device)
    mip = MipCubemapEncoder(num_levels=2, level_dim=2, per_level_scale=2, base_resolution=2).to(gpu_device)
    for mod, width in ((enc, 3), (mip, 4)):
        out = mod(torch.zeros(0, 3, device=gpu_device))
        assert tuple(out.shape) == (0, width)
        out.sum().backward()
        grads = [p.grad for p in mod.parameters()]
        assert all(g is not None and g.shape == p.shape and float(g.abs().max()) == 0.0 for g, p in zip(grads, mod.parameters()))
    raw = cubemap_encode(torch.zeros(0, 3, device=gpu_device), cm, fail, 1, 1)
    assert tuple(raw.shape) == (C, 0)


def test_module_state_dict_keys_and_reference_shapes():
    """The state_dict keys are the reference's (they are what a checkpoint of scene/gaussian_model.py's env_map holds), and tensors of
    the reference's shapes load: for the pyramid those are the level sizes of its recurrence, non-integer scale included."""
    from materialrefgs_amd.cubemap_encoder import CubemapEncoder, MipCubemapEncoder
    enc = CubemapEncoder(output_dim=3, resolution=8)
    assert sorted(enc.state_dict().keys()) == ["params.Cubemap_failv", "params.Cubemap_texture"]
    enc.load_state_dict({"params.Cubemap_texture": torch.full((6, 3, 8, 8), 2.0), "params.Cubemap_failv": torch.full((3,), 3.0)})
    assert float(enc.params["Cubemap_texture"].detach().min()) == 2.0 and float(enc.params["Cubemap_failv"].detach().max()) == 3.0
    sizes = [1, 2, 2, 2, 3, 4, 4, 6]                       # the reference's levels for base 1, scale 2^(1/3)
    mip = MipCubemapEncoder(num_levels=8, level_dim=2, per_level_scale=2 ** (1 / 3), base_resolution=1)
    assert sorted(mip.state_dict().keys()) == ["fail_value"] + [f"params_list.{i}" for i in range(8)]
    assert [tuple(p.shape) for p in mip.params_list] == [(6, 2, r, r) for r in sizes]
    state = {f"params_list.{i}": torch.full((6, 2, r, r), float(i)) for i, r in enumerate(sizes)}
    state["fail_value"] = torch.full((2,), 5.0)
    mip.load_state_dict(state)
    assert all(float(p.detach().max()) == float(i) for i, p in enumerate(mip.params_list)) and float(mip.fail_value.detach().min()) == 5.0
    dflt = MipCubemapEncoder()
    assert [int(p.shape[-1]) for p in dflt.params_list] == [4, 16, 64, 256] and tuple(dflt.fail_value.shape) == (6,)


# level sizes by the reference's recurrence (L = float(base); per level ceil(L), then L *= scale), 12 levels: (base, scale) -> sizes
_CBRT2, _SQRT2 = 2 ** (1 / 3), 2 ** 0.5
REFERENCE_LEVELS = {
    # where ceil(base * scale^i) differs: the running product lands on the integer, the power just above it (levels 6 and 9)
    (1, _CBRT2): [1, 2, 2, 2, 3, 4, 4, 6, 7, 8, 11, 13],
    (2, _CBRT2): [2, 3, 4, 4, 6, 7, 8, 11, 13, 16, 21, 26],
    (3, _CBRT2): [3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 31, 39],
    (4, _CBRT2): [4, 6, 7, 8, 11, 13, 16, 21, 26, 32, 41, 51],
    (16, _CBRT2): [16, 21, 26, 32, 41, 51, 64, 81, 102, 128, 162, 204],
    # where both agree
    (1, 1): [1] * 12, (2, 1): [2] * 12, (3, 1): [3] * 12, (4, 1): [4] * 12, (16, 1): [16] * 12,
    (1, 1.5): [1, 2, 3, 4, 6, 8, 12, 18, 26, 39, 58, 87],
    (2, 1.5): [2, 3, 5, 7, 11, 16, 23, 35, 52, 77, 116, 173],
    (3, 1.5): [3, 5, 7, 11, 16, 23, 35, 52, 77, 116, 173, 260],
    (4, 1.5): [4, 6, 9, 14, 21, 31, 46, 69, 103, 154, 231, 346],
    (16, 1.5): [16, 24, 36, 54, 81, 122, 183, 274, 411, 616, 923, 1384],
    (1, 2): [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048],
    (2, 2): [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096],
    (3, 2): [3, 6, 12, 24, 48, 96, 192, 384, 768, 1536, 3072, 6144],
    (4, 2): [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192],
    (16, 2): [16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768],
    (1, 4): [1, 4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576, 4194304],
    (2, 4): [2, 8, 32, 128, 512, 2048, 8192, 32768, 131072, 524288, 2097152, 8388608],
    (3, 4): [3, 12, 48, 192, 768, 3072, 12288, 49152, 196608, 786432, 3145728, 12582912],
    (4, 4): [4, 16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576, 4194304, 16777216],
    (16, 4): [16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576, 4194304, 16777216, 67108864],
    (1, _SQRT2): [1, 2, 3, 3, 5, 6, 9, 12, 17, 23, 33, 46],
    (2, _SQRT2): [2, 3, 5, 6, 9, 12, 17, 23, 33, 46, 65, 91],
    (3, _SQRT2): [3, 5, 7, 9, 13, 17, 25, 34, 49, 68, 97, 136],
    (4, _SQRT2): [4, 6, 9, 12, 17, 23, 33, 46, 65, 91, 129, 182],
    (16, _SQRT2): [16, 23, 33, 46, 65, 91, 129, 182, 257, 363, 513, 725],
    (1, 1.1): [1, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3],
    (2, 1.1): [2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6],
    (3, 1.1): [3, 4, 4, 4, 5, 5, 6, 6, 7, 8, 8, 9],
    (4, 1.1): [4, 5, 5, 6, 6, 7, 8, 8, 9, 10, 11, 12],
    (16, 1.1): [16, 18, 20, 22, 24, 26, 29, 32, 35, 38, 42, 46],
}


def test_mip_resolutions_follow_the_reference_recurrence():
    from materialrefgs_amd.cubemap_encoder import MipCubemapEncoder, mip_resolutions
    assert len(REFERENCE_LEVELS) == 5 * 7
    wrong = {k: mip_resolutions(12, *k) for k, want in REFERENCE_LEVELS.items() if mip_resolutions(12, *k) != want}
    assert not wrong, wrong
    mip = MipCubemapEncoder(num_levels=8, per_level_scale=2 ** (1 / 3), base_resolution=1)
    assert [tuple(p.shape) for p in mip.params_list] == [(6, 6, r, r) for r in [1, 2, 2, 2, 3, 4, 4, 6]]


@pytest.mark.gpu
def test_single_level_fetch_agrees_with_envmap_lookup_away_from_seams(gpu_device):
    """the two cube fetches of the path -- EnvLight's (nvdiffrast convention, [6,L,L,3]) and the cubemapencoder's
    ([6,C,L,L], its own face orientation) -- are the same bilinear fetch once the texels are put in each other's layout: for
    directions well inside a face both must return the same interpolated value of the same texel grid."""
    from materialrefgs_amd.cubemap_encoder import cubemap_encode
    from materialrefgs_amd.shading import EnvLight
    from oracle import shading_oracle as so
    L = 16
    rng = np.random.default_rng(8)
    env_tex = rng.normal(size=(6, L, L, 3)).astype(np.float32)
    # resample the EnvLight cubemap into the cubemapencoder layout texel by texel: encoder texel (face, y, x) sits at direction
    # d(face, u, v); the EnvLight texel at that direction is found with the pinned cube_to_dir inverse (shading_oracle.dir_to_face_uv)
    enc_tex = np.zeros((6, 3, L, L), np.float32)
    centres = (np.arange(L) + 0.5) / L * 2 - 1
    for f in range(6):
        for y in range(L):
            for x in range(L):
                u, v = centres[x], -centres[y]                       # pixel row = (-v * .5 + .5) L
                d = co.face_dir(f, u, v)                             # inverse of Compute_Cubemap_UV (:147-187)
                ff, uu, vv2 = so.dir_to_face_uv(torch.tensor(d[None], dtype=torch.float64))
                xi = int(np.clip(np.floor((float(uu) * 0.5 + 0.5) * L), 0, L - 1)); yi = int(np.clip(np.floor((float(vv2) * 0.5 + 0.5) * L), 0, L - 1))
                enc_tex[f, :, y, x] = env_tex[int(ff), yi, xi]
    dirs = rng.normal(size=(4000, 3)).astype(np.float32)
    a = np.abs(dirs); m = a.max(1, keepdims=True)
    inner = (np.sort(a / m, axis=1)[:, 1] < 1 - 2.5 / L)             # second-largest |component| well below the largest: inside a face
    dirs = dirs[inner]
    out_enc = cubemap_encode(torch.tensor(dirs, device=gpu_device), torch.tensor(enc_tex, device=gpu_device), torch.zeros(3, device=gpu_device), 1, 1)
    env = EnvLight(device=gpu_device, min_res=L, max_res=L)
    with torch.no_grad():
        env.base.copy_(torch.tensor(env_tex))
    out_env = env(torch.tensor(dirs, device=gpu_device), mode="pure_env")          # sigmoid(fetch)
    got = torch.sigmoid(out_enc.permute(1, 0))
    assert float((got - out_env).abs().max()) < 2e-5
