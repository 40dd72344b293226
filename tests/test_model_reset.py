"""mrgs_model_reset (csrc/mrgs_model_reset.hip): the float64 statement (tests/model_statement.py) against the reference's own methods
(tests/golden/reference_model.npz), the entry point's refusals without a GPU, and on the GPU the kernel against the statement -- every
rule, every keep bit, block and wave edges, the moments, the guard row -- and its counter generator."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import model_statement as ms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_model.npz")
MIN_MARGIN = 1e-3


# ---- the statement against the reference ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    model = {k: z[f"in_{k}"].astype(np.float64) for k in ms.GROUPS}
    model.update(zip(("refl_msk_thr", "rough_msk_thr", "enlarge_scale"), (float(v) for v in z["settings"])))
    u = {k: z[f"u_{k}"].astype(np.float64) for k in ("f_dc", "ori_color")}
    return z, model, z["in_exclusive"].astype(bool), u


def _rows(model, keep, exclusive, like):
    rows, _ = ms.keep_rows(keep, model["refl_strength"], model["roughness"], exclusive, model["refl_msk_thr"], model["rough_msk_thr"])
    return np.broadcast_to(rows.reshape((-1,) + (1,) * (like.ndim - 1)), like.shape)


def _check(z, key, group, model, new_model, margin, tol, exact=None):
    """reference output of `key` for `group` against the statement's, element by element; `exact`: elements that must be src's bits."""
    assert margin >= MIN_MARGIN, (key, margin)
    ref, want = z[f"{key}__{group}"].astype(np.float64), new_model[group]
    assert ref.shape == want.shape
    err = np.abs(ref - want)
    bound = tol(want) if callable(tol) else np.full(want.shape, tol)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if tol is not None else 0.0
    print(f"{key}/{group}: max |ref - statement| = {err.max():.3e}, worst error / bound = {worst:.3f}, margin = {margin:.3e}")
    if exact is not None:
        assert np.array_equal(ref[exact], model[group][exact]), (key, group)
        err, bound = err[~exact], bound[~exact]
    assert np.all(err <= bound), (key, group, float(err.max()))


def test_fixture_inputs_satisfy_the_margin_condition(golden):
    z, model, excl, u = golden
    assert model["opacity"].shape == (64, 1) and all(np.abs(model[k]).max() <= 6.0 for k in ms.GROUPS)
    assert 0 < excl.sum() < 64
    for mg in (ms.reset_opacity0(model)[1], ms.reset_opacity1(model, excl)[1], ms.reset_refl(model, excl)[1], ms.reset_refl(model, excl, 0.3)[1],
               ms.reset_refl_strength2(model)[1], ms.dist_color(model, u["f_dc"], excl)[1], ms.reset_scale(model, excl)[1]):
        assert mg >= MIN_MARGIN
    # every branch occurs: both sides of each decision, kept and unkept rows of each mask
    s = ms.sigmoid(model["opacity"])
    assert (s > 0.9).any() and (s < 0.9).any() and (s > 0.01).any() and (s < 0.01).any()
    r = ms.sigmoid(model["refl_strength"])
    assert (r < 0.1).any() and (r > 0.1).any() and (r < 0.02).any() and (ms.sigmoid(model["roughness"]) > 0.1).any()
    for keep in (ms.KEEP_REFL_ABOVE, ms.KEEP_REFL_BELOW | ms.KEEP_ROUGH_ABOVE):
        rows, _ = ms.keep_rows(keep, model["refl_strength"], model["roughness"], None, 0.02, 0.1)
        assert 0 < rows.sum() < 64


def test_statement_sigmoid_rules_against_the_reference(golden):
    z, model, excl, _u = golden
    E = ms.KEEP_EXCLUSIVE
    _check(z, "reset_opacity0", "opacity", model, *ms.reset_opacity0(model, literal=True), ms.logit_tol)
    lift_same = ms.sigmoid(model["opacity"]) > ms.f32(0.9)
    _check(z, "reset_opacity1", "opacity", model, *ms.reset_opacity1(model), ms.logit_tol, exact=lift_same)
    _check(z, "reset_opacity1_excl", "opacity", model, *ms.reset_opacity1(model, excl), ms.logit_tol,
           exact=lift_same | _rows(model, E, excl, model["opacity"]))
    _check(z, "reset_refl", "refl_strength", model, *ms.reset_refl(model, literal=True), ms.logit_tol)
    _check(z, "reset_refl_excl", "refl_strength", model, *ms.reset_refl(model, excl, literal=True), ms.logit_tol,
           exact=_rows(model, E, excl, model["refl_strength"]))
    _check(z, "reset_refl_excl_030", "refl_strength", model, *ms.reset_refl(model, excl, 0.3, literal=True), ms.logit_tol,
           exact=_rows(model, E, excl, model["refl_strength"]))
    _check(z, "reset_refl_strength", "refl_strength", model, *ms.reset_refl_strength(model), ms.logit_tol)
    _check(z, "reset_refl_strength2", "refl_strength", model, *ms.reset_refl_strength2(model, literal=True), ms.logit_tol)
    _check(z, "reset_roughness", "roughness", model, *ms.reset_roughness(model, 0.25), ms.logit_tol)


def test_statement_literal_switch_only_touches_the_unchanged_side(golden):
    _z, model, _excl, _u = golden
    a, _ = ms.reset_opacity0(model)
    b, _ = ms.reset_opacity0(model, literal=True)
    same = ~(ms.sigmoid(model["opacity"]) > ms.f32(0.01))
    assert np.array_equal(a["opacity"][same], model["opacity"][same]) and np.array_equal(a["opacity"][~same], b["opacity"][~same])
    assert same.any() and np.all(np.abs(b["opacity"][same] - model["opacity"][same]) <= 1e-12)      # the round trip, harmless in float64


def test_statement_drawing_rules_against_the_reference(golden):
    z, model, excl, u = golden
    _check(z, "reset_ori_color", "ori_color", model, *ms.reset_ori_color(model, u["ori_color"]), lambda x: ms.jitter_const_tol(x, 0.5, 0.05))
    above = ms.KEEP_REFL_ABOVE
    _check(z, "dist_color", "f_dc", model, *ms.dist_color(model, u["f_dc"]), ms.jitter_tol, exact=_rows(model, above, None, model["f_dc"]))
    _check(z, "dist_color_excl", "f_dc", model, *ms.dist_color(model, u["f_dc"], excl), ms.jitter_tol,
           exact=_rows(model, above | ms.KEEP_EXCLUSIVE, excl, model["f_dc"]))
    _check(z, "dist_albedo_excl", "ori_color", model, *ms.dist_albedo(model, u["ori_color"], excl), ms.jitter_tol,
           exact=_rows(model, above | ms.KEEP_EXCLUSIVE, excl, model["ori_color"]))


def test_statement_scale_and_fill_rules_against_the_reference(golden):
    z, model, excl, _u = golden
    keep = ms.KEEP_REFL_BELOW | ms.KEEP_ROUGH_ABOVE
    _check(z, "reset_scale", "scaling", model, *ms.reset_scale(model), ms.enlarge_tol, exact=_rows(model, keep, None, model["scaling"]))
    _check(z, "reset_scale_excl", "scaling", model, *ms.reset_scale(model, excl), ms.enlarge_tol,
           exact=_rows(model, keep | ms.KEEP_EXCLUSIVE, excl, model["scaling"]))
    act, margin = ms.enlarge_refl_scales(model, ret_raw=False, exclusive=excl)
    ref = z["enlarge_refl_scales_activated_excl"].astype(np.float64)
    assert margin >= MIN_MARGIN and np.all(np.abs(ref - act) <= 2 * ms.EPS * np.abs(act))      # exp within one ulp, the product half of one
    new, margin = ms.reset_features(model)
    for g in ("f_dc", "f_rest"):
        assert np.array_equal(z[f"reset_features__{g}"], new[g]) and not new[g].any()


def test_statement_sequences_against_the_reference(golden):
    z, model, excl, u = golden
    E = ms.KEEP_EXCLUSIVE
    new, margin = ms.normal_propagation_step(model, u["f_dc"], excl)
    key = "seq_normal_propagation"
    _check(z, key, "opacity", model, new, margin, ms.logit_tol, exact=(ms.sigmoid(model["opacity"]) > ms.f32(0.9)) | _rows(model, E, excl, model["opacity"]))
    _check(z, key, "f_dc", model, new, margin, ms.jitter_tol, exact=_rows(model, E | ms.KEEP_REFL_ABOVE, excl, model["f_dc"]))
    _check(z, key, "scaling", model, new, margin, ms.enlarge_tol, exact=_rows(model, E | ms.KEEP_REFL_BELOW | ms.KEEP_ROUGH_ABOVE, excl, model["scaling"]))
    new, margin = ms.opacity_reset_step(model, excl, 0.1, literal=True)
    _check(z, "seq_opacity_reset", "opacity", model, new, margin, ms.logit_tol)
    _check(z, "seq_opacity_reset", "refl_strength", model, new, margin, ms.logit_tol, exact=_rows(model, E, excl, model["refl_strength"]))
    new, margin = ms.material_reset_step(model, u["ori_color"], 0.2, features=True)
    _check(z, "seq_material_reset", "ori_color", model, new, margin, lambda x: ms.jitter_const_tol(x, 0.5, 0.05))
    _check(z, "seq_material_reset", "refl_strength", model, new, margin, ms.logit_tol)
    _check(z, "seq_material_reset", "roughness", model, new, margin, ms.logit_tol)
    for g in ("f_dc", "f_rest"):
        assert np.array_equal(z[f"seq_material_reset__{g}"], new[g])


# ---- refusals, before any HIP call ----------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    from materialrefgs_amd import _lib
    from materialrefgs_amd._lib import MrgsResetConfig, MrgsResetItem
    L = _lib.lib()
    OK, BAD = _lib.MRGS_OK, _lib.MRGS_E_BAD_ARG
    p = 0x1000                                             # never dereferenced: every call below is refused or launches nothing
    assert ctypes.sizeof(MrgsResetItem) == 5 * 8 + 4 * 4 + 2 * 8 and ctypes.sizeof(MrgsResetConfig) == 8 + 8 + 3 * 8 + 2 * 4 + 8

    def call(n_items=1, P=4, cfg_kw=None, **kw):
        item = dict(src=p, dst=p, exp_avg_dst=None, exp_avg_sq_dst=None, noise=None, width=1, rule=_lib.MRGS_RESET_CAP, keep=0, reserved=0, a=0.5, b=0.0)
        item.update(kw)
        cfg = MrgsResetConfig(P, p, p, p, 0.02, 0.1, 0)
        for k, v in (cfg_kw or {}).items():
            setattr(cfg, k, v)
        arr = (MrgsResetItem * 8)(*[MrgsResetItem(**item) for _ in range(8)])
        return L.mrgs_model_reset(ctypes.byref(cfg), arr, n_items, None)

    assert call(P=0) == OK                                                    # nothing to launch
    assert call(P=0, src=None, dst=None) == OK
    assert call(P=0, cfg_kw=dict(struct_size=ctypes.sizeof(MrgsResetConfig) - 8)) == BAD
    assert call(P=0, n_items=0) == BAD and call(P=0, n_items=9) == BAD and call(P=0, n_items=8) == OK
    assert call(P=0, width=0) == BAD and call(P=0, rule=8) == BAD and call(P=0, rule=-1) == BAD and call(P=0, keep=16) == BAD
    assert call(P=0, exp_avg_dst=p) == BAD and call(P=0, exp_avg_sq_dst=p) == BAD and call(P=0, exp_avg_dst=p, exp_avg_sq_dst=p) == OK
    assert call(P=0, keep=_lib.MRGS_RESET_KEEP_EXCLUSIVE, cfg_kw=dict(exclusive=None)) == BAD
    assert call(P=0, keep=_lib.MRGS_RESET_KEEP_REFL_ABOVE, cfg_kw=dict(refl_raw=None)) == BAD
    assert call(P=0, keep=_lib.MRGS_RESET_KEEP_REFL_BELOW, cfg_kw=dict(refl_raw=None)) == BAD
    assert call(P=0, keep=_lib.MRGS_RESET_KEEP_ROUGH_ABOVE, cfg_kw=dict(rough_raw=None)) == BAD
    assert call(P=0, keep=15) == OK and call(P=0, cfg_kw=dict(refl_raw=None, rough_raw=None, exclusive=None)) == OK
    assert call(src=None) == BAD and call(dst=None) == BAD
    for rule in (_lib.MRGS_RESET_CAP, _lib.MRGS_RESET_FLOOR, _lib.MRGS_RESET_LIFT, _lib.MRGS_RESET_CONST):
        for a in (0.0, 1.0, -0.1, 1.5, math.nan):
            assert call(P=0, rule=rule, a=a) == BAD
    for rule in (_lib.MRGS_RESET_FILL, _lib.MRGS_RESET_JITTER, _lib.MRGS_RESET_JITTER_CONST, _lib.MRGS_RESET_ENLARGE):
        assert call(P=0, rule=rule, a=1.5) == OK                              # no logit is taken of these
    assert L.mrgs_model_reset(None, None, 1, None) == BAD


@pytest.mark.skipif(torch.cuda.device_count() != 0, reason="host addresses as arguments: only for a machine without a device")
def test_launch_failure_goes_through_the_one_status_path():
    """Without a device the launch fails: MRGS_E_HIP, and mrgs_last_hip_error() names this file (as tests/test_status.py shows for the others)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    item = (_lib.MrgsResetItem * 1)(_lib.MrgsResetItem(p, p + 128, None, None, None, 1, _lib.MRGS_RESET_CONST, 0, 0, 0.5, 0.0))
    cfg = _lib.MrgsResetConfig(4, None, None, None, 0.02, 0.1, 0)
    assert L.mrgs_model_reset(ctypes.byref(cfg), item, 1, None) == _lib.MRGS_E_HIP
    text = L.mrgs_last_hip_error()
    assert text and b" at mrgs_model_reset.hip:" in text, text


# ---- the kernel against the statement ------------------------------------------------------------------------------------------------
RULE_ARGS = {ms.CAP: (0.3, 0.0), ms.FLOOR: (0.6, 0.0), ms.LIFT: (0.7, 0.0), ms.CONST: (0.15, 0.0), ms.FILL: (-1.25, 0.0), ms.JITTER: (0.4, 0.0),
             ms.JITTER_CONST: (0.5, 0.05), ms.ENLARGE: (1.5, 0.0)}
REFL_THR, ROUGH_THR = 0.3, 0.6


def _inputs(P, widths, seed):
    """fp32 sources per width, mask inputs and uniforms whose every decision keeps the margin (resampled until it does)."""
    rng = np.random.default_rng(seed)

    def draw(shape, lo, hi, thresholds):
        """uniform fp32 values whose sigmoid keeps the margin from every threshold: the elements that do not are drawn again"""
        v = rng.uniform(lo, hi, shape).astype(np.float32)
        while True:
            s = ms.sigmoid(v)
            close = np.zeros(shape, dtype=bool)
            for t in thresholds:
                close |= np.abs(s - ms.f32(t)) < 2 * MIN_MARGIN * t
            if not close.any():
                return v
            v[close] = rng.uniform(lo, hi, int(close.sum())).astype(np.float32)
    src = [draw((P + 1, w), -6, 6, [RULE_ARGS[r][0] for r in (ms.CAP, ms.FLOOR, ms.LIFT)]) for w in widths]          # one guard row
    refl, rough = draw((P,), -3, 3, [REFL_THR]), draw((P,), -3, 3, [ROUGH_THR])
    excl = rng.random(P) < 0.3
    noise = [rng.random((P, w)).astype(np.float32) for w in widths]
    margin = min([ms.keep_rows(15, refl, rough, excl, REFL_THR, ROUGH_THR)[1]] +
                 [ms.apply_rule(rule, s[:P], RULE_ARGS[rule][0])[2] for s in src for rule in (ms.CAP, ms.FLOOR, ms.LIFT)])
    assert margin >= MIN_MARGIN
    return src, refl, rough, excl, noise


def _launch(dev, P, specs, refl, rough, excl, seed=0, moments=True):
    """specs: (src np [P + 1, w], rule, keep, a, b, noise np or None).  Returns per item (dst [P + 1, w], m, v) as numpy; the guard row of
    dst and of the moments is pre-filled with a sentinel."""
    from materialrefgs_amd import _lib
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    hold, arr = [], (_lib.MrgsResetItem * len(specs))()
    for i, (src, rule, keep, a, b, noise) in enumerate(specs):
        s, u = t(src), t(noise)
        d = torch.full_like(s, 777.0)
        m, v = (torch.full_like(s, 777.0), torch.full_like(s, 777.0)) if moments else (None, None)
        hold.append((s, d, m, v, u))
        arr[i] = _lib.MrgsResetItem(s.data_ptr(), d.data_ptr(), _lib.ptr(m), _lib.ptr(v), _lib.ptr(u), src.shape[1], rule, keep, 0, a, b)
    r, g, e = t(refl), t(rough), t(None if excl is None else excl.astype(np.uint8))
    cfg = _lib.MrgsResetConfig(P, r.data_ptr(), g.data_ptr(), _lib.ptr(e), REFL_THR, ROUGH_THR, seed)
    _lib.check(_lib.lib().mrgs_model_reset(ctypes.byref(cfg), arr, len(specs), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    return [(d.cpu().numpy(), None if m is None else m.cpu().numpy(), None if v is None else v.cpu().numpy()) for _s, d, m, v, _u in hold]


def _jitter_fp32_torch(v, u, a):
    """The reference's fp32 form on the CPU, in the stated operation order."""
    v, u = torch.from_numpy(v), torch.from_numpy(u)
    a = torch.tensor(a, dtype=torch.float32)
    return (v + ((u * a) * 2.0 - a)).numpy()


def _verify(P, spec, got, refl, rough, excl):
    src, rule, keep, a, b, noise = spec
    dst, m, v = got
    want, same, margin = ms.reset_item(src[:P], rule, keep, a, b, noise, refl, rough, excl, REFL_THR, ROUGH_THR)
    assert margin >= MIN_MARGIN
    assert np.all(dst[P] == 777.0), "the row beyond P was written"
    out = dst[:P]
    assert np.array_equal(out[same].view(np.uint32), src[:P][same].view(np.uint32)), (rule, keep)     # kept rows / unchanged side: src's bits
    free, x = ~same, want[~same]
    err = np.abs(out[free].astype(np.float64) - x)
    if rule in (ms.CAP, ms.FLOOR, ms.LIFT, ms.CONST):
        assert np.all(out[free] == np.float32(ms.L(a))), rule                                           # the constant, rounded once
    elif rule == ms.FILL:
        assert np.all(out[free] == np.float32(a))
    elif rule == ms.JITTER:
        assert np.array_equal(out[free], _jitter_fp32_torch(src[:P], noise, a)[free]) and np.all(err <= ms.jitter_tol(x))
    elif rule in (ms.JITTER_CONST, ms.ENLARGE):
        tol = ms.jitter_const_tol(x, a, b) if rule == ms.JITTER_CONST else ms.enlarge_tol(x)
        i = int(np.argmax(err / tol)) if err.size else 0
        assert np.all(err <= tol), (rule, float(err[i] / tol[i]), float(src[:P][free][i]), float(out[free][i]), float(x[i]))
    if m is not None:
        assert not m[:P].any() and not v[:P].any() and np.all(m[P] == 777.0) and np.all(v[P] == 777.0)   # 0 for EVERY row, kept ones too


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1000])
def test_kernel_every_rule_and_keep_bit(gpu_device, P):
    """Eight items a launch (all rules), widths {1, 2, 3, 45}; each of the sixteen keep combinations, with moments."""
    widths = (1, 2, 3, 45)
    src, refl, rough, excl, noise = _inputs(P, widths, seed=P)
    for keep in range(16):
        specs = []
        for rule in range(8):
            k = (rule + keep) % 4
            specs.append((src[k], rule, keep, *RULE_ARGS[rule], noise[k] if rule in (ms.JITTER, ms.JITTER_CONST) else None))
        got = _launch(gpu_device, P, specs, refl, rough, excl)
        for spec, g in zip(specs, got):
            _verify(P, spec, g, refl, rough, excl)


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", [1, 3, 8])
@pytest.mark.parametrize("moments", [False, True])
def test_kernel_item_counts_moments_and_no_exclusive(gpu_device, n_items, moments):
    """n_items 1 / 3 / 8, with and without moments, with and without the exclusive vector; every width meets every rule."""
    P, widths = 257, (1, 2, 3, 45)
    src, refl, rough, excl, noise = _inputs(P, widths, seed=7)
    for shift in range(4):
        for use_excl in (True, False):
            keep = 15 if use_excl else 14
            rules = [(r + 3 * shift) % 8 for r in range(n_items)]
            specs = [(src[(i + shift) % 4], rule, keep if i % 2 else keep & 9, *RULE_ARGS[rule],
                      noise[(i + shift) % 4] if rule in (ms.JITTER, ms.JITTER_CONST) else None) for i, rule in enumerate(rules)]
            if not use_excl:
                specs = [(s, r, k & ~1, a, b, n) for s, r, k, a, b, n in specs]
            got = _launch(gpu_device, P, specs, refl, rough, excl if use_excl else None, moments=moments)
            for spec, g in zip(specs, got):
                _verify(P, spec, g, refl, rough, excl if use_excl else None)


@pytest.mark.gpu
def test_kernel_every_width_meets_every_rule(gpu_device):
    P, widths = 65, (1, 2, 3, 45)
    src, refl, rough, excl, noise = _inputs(P, widths, seed=3)
    for k in range(4):
        specs = [(src[k], rule, 9, *RULE_ARGS[rule], noise[k] if rule in (ms.JITTER, ms.JITTER_CONST) else None) for rule in range(8)]
        for spec, g in zip(specs, _launch(gpu_device, P, specs, refl, rough, excl, moments=False)):
            _verify(P, spec, g, refl, rough, excl)


@pytest.mark.gpu
def test_philox_path(gpu_device):
    """Without `noise`: the same seed gives the same bits, another seed others; every unmasked element lies in [v - a, v + a); the mean of
    the offsets and the occupancy of 16 equal bins of u are those of a uniform variable (five standard deviations)."""
    P, w, a = 1000, 3, 0.4
    src, refl, rough, excl, _noise = _inputs(P, (w,), seed=5)
    spec = (src[0], ms.JITTER, ms.KEEP_REFL_ABOVE | ms.KEEP_EXCLUSIVE, a, 0.0, None)
    run = lambda seed: _launch(gpu_device, P, [spec], refl, rough, excl, seed=seed)[0][0][:P]
    one, again, other = run(1234567890123), run(1234567890123), run(99)
    assert np.array_equal(one.view(np.uint32), again.view(np.uint32)) and not np.array_equal(one, other)
    rows, _ = ms.keep_rows(spec[2], refl, rough, excl, REFL_THR, ROUGH_THR)
    v = src[0][:P]
    assert np.array_equal(one[rows], v[rows]) and 100 < (~rows).sum() < 900
    af = np.float32(a)
    for out in (one, other):
        d = (out[~rows].astype(np.float64) - v[~rows].astype(np.float64)).reshape(-1)
        # [v - a, v + a) holds for the exact sum: u <= 1 - 2^-24 puts the offset (u a) 2 - a in [-a, a (1 - 2^-23)].  The kernel's last fp32
        # addition rounds that sum, and where ulp(v) / 2 exceeds a 2^-23 (|v| above ~0.8 here) the nearest float to a sum just below
        # v + a can be fl(v + a) itself: the end point is therefore compared closed, against the fp32 images fl(v - a), fl(v + a), and
        # the distance from v additionally stays below a plus one ulp of the largest |v| (2^-21 at |v| < 8).  u itself is half-open:
        # recovered from the fp32 result it is clipped, so u < 1 is asserted where the sum is exact enough to tell (|v| < 0.5).
        lo, hi = (v[~rows] - af), (v[~rows] + af)
        small = np.abs(v[~rows]).reshape(-1) < 0.5
        exact_u = ((out[~rows].astype(np.float64) - v[~rows].astype(np.float64)).reshape(-1)[small] + float(af)) / (2 * float(af))
        assert small.sum() > 20 and np.all(exact_u < 1.0) and np.all(exact_u >= -2.0 ** -24)
        assert np.all(out[~rows] >= lo) and np.all(out[~rows] <= hi) and np.all(d < float(af) + 2.0 ** -21)
        n = d.size
        assert abs(d.mean()) <= 5 * a / math.sqrt(3 * n)
        u = np.clip((d + float(af)) / (2 * float(af)), 0.0, 1.0 - 1e-12)
        bins = np.bincount((u * 16).astype(int), minlength=16)
        assert np.all(np.abs(bins - n / 16) <= 5 * math.sqrt(n * 15 / 256)), bins
    # JITTER_CONST draws from the same generator: item index and column enter the counter, so two items of one call differ
    specs = [(src[0], ms.JITTER_CONST, 0, 0.5, 0.05, None), (src[0], ms.JITTER_CONST, 0, 0.5, 0.05, None)]
    c0, c1 = (g[0][:P] for g in _launch(gpu_device, P, specs, refl, rough, excl, seed=5))
    assert not np.array_equal(c0, c1) and not np.array_equal(c0[:, 0], c0[:, 1])
    assert np.all(np.abs(c0) <= ms.L(0.525) + 1e-6) and np.all(np.abs(c1) <= ms.L(0.525) + 1e-6)
