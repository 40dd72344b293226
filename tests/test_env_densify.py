"""EnvGaussianModel.densify_and_prune and add_densification_stats (materialrefgs_amd/env_model.py, csrc/mrgs_env_densify.hip) against the
six-stage statement of tests/env_densify_statement.py.  Every input set keeps g, max(s) of every generation, o and the radius >= 1e-3
(relative) away from their thresholds -- asserted on the statement's side -- so that the decision sets, the counts and the row order must
agree EXACTLY; the weight path (the three maxima, wavg, q, the top-k set) is float32 on both sides and compared without any margin.
Copied rows and moments are compared bit for bit, the two computed tensors within the statement's per-generation bounds."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import env_densify_statement as es

# the six groups of EnvGaussianModel.training_setup (env_gaussian_model.py:167-174) with their row shapes
GROUPS = [("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (2,)), ("rotation", (4,))]
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
PERCENT_DENSE, EXTENT, MAX_GRAD, MIN_OPACITY = 0.01, 5.0, 5e-5, 0.05
T = PERCENT_DENSE * EXTENT
OPT = SimpleNamespace(position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
                      features_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3, percent_dense=0.5)


# ---------------------------------------------------------------- without a GPU ------------------------------------------------------
def test_quantile_rule_on_known_vectors():
    """rank = 0.1f (n - 1) in float32: n = 1 -> the value; n = 2 -> rank 0.1: v0 + 0.1f (v1 - v0); n = 11 -> rank 1 exactly: the second
    smallest; n = 12 -> rank fl(1.1f) = 1.1000000238: lo 1, hi 2, f = fl(rank - 1)."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    assert float(es.quantile_rule(f32([3.5]))) == 3.5
    assert es.quantile_rule(f32([4.0, 2.0])).item() == (f32(2.0) + f32(0.1) * f32(2.0)).item()
    v11 = f32([9.0, 0.5, 7.0, 3.0, 1.0, 8.0, 2.0, 10.0, 4.0, 6.0, 5.0])
    assert float(es.quantile_rule(v11)) == 1.0
    v12 = torch.cat((v11, f32([11.0])))
    rank = f32(0.1) * f32(11.0)
    f = rank - f32(1.0)
    assert 0.0 < float(f) < 0.5 and float(es.quantile_rule(v12)) == (f32(1.0) + f * f32(1.0)).item()
    assert abs(float(es.quantile_rule(v12)) - 1.1) < 1e-6
    # f >= 0.5 takes the other branch of lerp: n = 7 -> rank 0.6
    v7 = f32([0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0])
    r7 = f32(0.1) * f32(6.0)
    assert float(r7) >= 0.5 and float(es.quantile_rule(v7)) == (f32(10.0) - f32(10.0) * (f32(1.0) - r7)).item()
    # torch's own fp32 quantile agrees up to whether it fuses the multiply-add
    big = torch.rand(1000, generator=torch.Generator().manual_seed(0))
    assert abs(float(es.quantile_rule(big)) - float(torch.quantile(big, 0.1))) <= 2.0 ** -23


def test_philox_counter_layout_known_answers():
    """Philox4x32-10 (Random123 kat_vectors): zero, all-ones, and the pi-digits vector read as the stage-4 layout -- key = seed (low word,
    high word), counter = (row low word, row high word, child j, 1 + sigma)."""
    words = lambda c: [int(x[0]) for x in c]
    assert words(es.philox_words(0, 0, 0, 0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert words(es.philox_words(2 ** 64 - 1, *([0xffffffff] * 4))) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    seed, row, j, sigma = 0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e, 0x03707343
    assert words(es.philox_words(seed, row & 0xffffffff, row >> 32, j, 1 + sigma)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    z = es.philox_normals(seed, np.array([row], dtype=np.uint64), j, 1 + sigma)[0]
    u0, u1 = ((0xd16cfe09 >> 8) + 1) * 2.0 ** -24, ((0x94fdcceb >> 8) + 1) * 2.0 ** -24
    r = math.sqrt(-2.0 * math.log(u0))
    assert abs(z[0] - r * math.cos(2 * math.pi * u1)) < 1e-12 and abs(z[1] - r * math.sin(2 * math.pi * u1)) < 1e-12
    # stage 2 keeps the existing layout (c3 = 0): the same words as the main set's generator
    import densify_statement as ds
    _n0, _n1, z_old = ds.philox_normals(7, np.arange(5), 1)
    assert np.array_equal(z_old, es.philox_normals(7, np.arange(5), 1))


def test_statement_on_a_hand_worked_case():
    """Eight rows, t = 0.1, world limit 1, max_grad = 0.5, min_opacity = 0.05, max_screen_size = 20, identity rotations, every stage fires:
       row 0  g = 2/2 = 1, s = 0.05, w = 4, d = 2             -> cloned; W0 = max w = 8, the clone's weight 4 * 8 = 32
       row 1  g = 1.5, s = (0.4, 0.2), w = 2, d = 2           -> split in 2 (W1 = max(8, 32) = 32): children weigh 64, s = (0.25, 0.125)
       row 2  o = sigmoid(-5) < 0.05                          -> stage 3 removes it
       row 3  g = 0.1, s = (2, 0.05) > 1, w = 8, d = 1        -> big, wavg 8 >= q: five children, s = (0.8, 0.02)
       row 4  g = 0/1 = 0, w = 2, d = 1                       -> kept, wavg 2
       row 5  0/0 -> g = 0, w = 0, d = 0, s = (1.6, 0.05)     -> big, wavg 0/0 -> 0 < q: stage 4 prunes it
       row 6  g = 4, s = (3.2, 0.1), w = 1, d = 1             -> split in 2: children s = (2, 0.0625), weight 32, big: five children EACH, s = (0.8, 0.025)
       row 7  g = 0.2, r = 64 > 20, w = 3, d = 1              -> big on the screen: five children, s = 0.02
    Stage 4 sees n = 10 rows with wavg (2, 8, 2, 0, 3 | 16 | 32, 32, 32, 32): rank 0.1f * 9 rounds to f = 0.90000004, q = 2 - 2 (1 - f) = 1.8.
    W4 = 64 (the children of row 1).  25 rows reach stage 5 with wavg (2, 2, 16, 32, 32, then 512 / 192 / 2048 / 2048 five times); n_after
    = 24, one row goes: rows 0 and 4 tie at 2 and the earlier one, row 0, is it."""
    lg = math.log
    f = lambda rows: torch.tensor(rows, dtype=torch.float64)
    small = [lg(0.05)] * 2
    params = {"xyz": f([[i, i, i] for i in range(8)]),
              "scaling": f([small, [lg(0.4), lg(0.2)], small, [lg(2.0), lg(0.05)], small, [lg(1.6), lg(0.05)], [lg(3.2), lg(0.1)], small]),
              "rotation": f([[1, 0, 0, 0]] * 8), "opacity": f([[0], [0], [-5], [0], [0], [0], [0], [0]]),
              "f_dc": f([[10 + i] for i in range(8)])}
    moments = {k: (v + 100.0, v + 200.0) for k, v in params.items()}
    accum, denom = f([2, 3, 0.1, 0.1, 0, 0, 4, 0.2]), f([2, 2, 1, 1, 1, 0, 1, 1])
    radii, weight = f([0, 0, 0, 0, 0, 0, 0, 64]), f([4, 2, 1, 8, 2, 0, 1, 3])
    noise = torch.zeros(8, 2, 2, dtype=torch.float64)
    noise[1], noise[6] = f([[1, -1], [0.5, 2]]), f([[1, 1], [-1, 0.5]])
    noise4 = torch.zeros(8, 4, 5, 2, dtype=torch.float64)
    for j in range(5):
        noise4[:, :, j, 0], noise4[:, :, j, 1] = 0.1 * (j + 1), -0.2 * (j + 1)
    r = es.densify_and_prune(params, moments, accum, denom, radii, weight, 0.01, 0.5, 0.05, 10.0, 20, noise, noise4, max_gs=24.5 / 0.9)
    i = r.info
    assert (i.n_clone, i.n_split, i.n_stage3, i.n_pruned4, i.n_split4, i.n_pruned5) == (1, 2, 10, 1, 4, 1)
    assert (float(i.W0), float(i.W1), float(i.W4)) == (8.0, 32.0, 64.0)
    rank = torch.tensor(0.1, dtype=torch.float32) * torch.tensor(9.0, dtype=torch.float32)
    assert float(i.q) == (torch.tensor(2.0) - torch.tensor(2.0) * (torch.tensor(1.0) - rank)).item() and abs(float(i.q) - 1.8) < 1e-6
    assert i.wavg4.tolist() == [2.0, 8.0, 2.0, 0.0, 3.0, 16.0, 32.0, 32.0, 32.0, 32.0] and i.low.tolist() == [False] * 3 + [True] + [False] * 6
    assert i.wavg5.tolist() == [2.0, 2.0, 16.0, 32.0, 32.0] + [512.0, 192.0, 2048.0, 2048.0] * 5 and float(i.cut) == 2.0
    assert r.rows == 24
    assert r.row.tolist() == [4, 0, 1, 1] + [3, 7, 6, 6] * 5 and r.slot.tolist() == [0, 1, 2, 3] + [0, 0, 2, 3] * 5
    assert r.child4.tolist() == [-1] * 4 + [j for j in range(5) for _ in range(4)] and r.gen.tolist() == [0, 0, 1, 1] + [1, 1, 2, 2] * 5
    assert es.segments(r) == (1, 1, 1, 1) + (2, 0, 1, 1) * 5       # rows 3 and 7 share "child j of an original"
    want_scaling = [small, small, [lg(0.25), lg(0.125)], [lg(0.25), lg(0.125)]] + [[lg(0.8), lg(0.02)], [lg(0.02)] * 2, [lg(0.8), lg(0.025)], [lg(0.8), lg(0.025)]] * 5
    assert torch.allclose(r.tensors["scaling"], f(want_scaling), atol=1e-14, rtol=0)
    want_xyz = [[4, 4, 4], [0, 0, 0], [1.4, 0.8, 1], [1.2, 1.4, 1]]
    for j in range(5):
        z0, z1 = 0.1 * (j + 1), -0.2 * (j + 1)
        want_xyz += [[3 + 2 * z0, 3 + 0.05 * z1, 3], [7 + 0.05 * z0, 7 + 0.05 * z1, 7],
                     [6 + 3.2 + 2 * z0, 6 + 0.1 + 0.0625 * z1, 6], [6 - 3.2 + 2 * z0, 6 + 0.05 + 0.0625 * z1, 6]]
    assert torch.allclose(r.tensors["xyz"], f(want_xyz), atol=1e-13, rtol=0)
    assert torch.equal(r.tensors["f_dc"], f([[14], [10], [11], [11]] + [[13], [17], [16], [16]] * 5))
    for k in params:
        m, v = r.moments[k]
        assert torch.equal(m[:1], params[k][[4]] + 100.0) and torch.equal(v[:1], params[k][[4]] + 200.0)        # the one surviving original
        assert float(m[1:].abs().sum()) == 0.0 and float(v[1:].abs().sum()) == 0.0
    assert all(s.shape[0] == 24 and float(s.abs().sum()) == 0.0 for s in r.stats) and r.stats[3].dim() == 1
    assert abs(r.margin - 0.2) < 1e-9                                # a stage-4 child's s = 0.8 against the world limit 1
    # the cap idle: 25 rows, row 0 first; without max_screen_size row 7 is not big and stays
    r2 = es.densify_and_prune(params, None, accum, denom, radii, weight, 0.01, 0.5, 0.05, 10.0, 20, noise, noise4)
    assert r2.rows == 25 and r2.row.tolist()[:2] == [0, 4] and r2.moments is None and r2.info.n_pruned5 == 0
    r3 = es.densify_and_prune(params, None, accum, denom, radii, weight, 0.01, 0.5, 0.05, 10.0, None, noise, noise4)
    assert r3.rows == 21 and r3.row.tolist()[:3] == [0, 4, 7] and r3.info.n_split4 == 3
    # the per-iteration lines
    a, d, w = es.add_densification_stats(f([[1], [2]]), f([[3], [4]]), f([[5], [6]]), f([[3, 4, 12], [1, 1, 1]]), torch.tensor([True, False]),
                                         f([[0.5], [9]]))
    assert a.tolist() == [[14.0], [2.0]] and d.tolist() == [[4.0], [4.0]] and w.tolist() == [[5.5], [6.0]]


def test_size_query_and_argument_validation_without_gpu():
    """Every contract violation is a status code before any HIP call; P = 0 is MRGS_OK with nothing launched."""
    from materialrefgs_amd import _lib
    from materialrefgs_amd._lib import MrgsDensifyTensor, MrgsEnvDensifyConfig
    L = _lib.lib()
    OK, BAD_ARG, UNSUPPORTED = 0, 1, 6
    assert ctypes.sizeof(MrgsEnvDensifyConfig) == 72 and _lib.MRGS_ENV_DENSIFY_COUNTS == 40
    align = lambda v: (v + 255) // 256 * 256
    assert L.mrgs_env_densify_ws_bytes(0) > 0
    for P in (1, 1000, 5000):
        assert L.mrgs_env_densify_ws_bytes(P) == 8192 + align(40 * P) + align(4 * P) + 2 * align(96 * ((P + 255) // 256))
    assert L.mrgs_env_select_ws_bytes() >= 32 + 4 * 256 * 4
    buf = (ctypes.c_float * 8192)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256                                 # never dereferenced: every call below is refused
    mk = lambda P=10, mg=0.1, flags=1, n_after=100, ptrs=(p, p, p): MrgsEnvDensifyConfig(flags, P, n_after, mg, 0.05, 0.1, 1.0, 20.0, 0.0, *ptrs)

    def classify(cfg, a=p, d=p, r=p, w=p, s=p, o=p, ws=p, wsb=1 << 20, cnt=p):
        return L.mrgs_env_densify_classify(ctypes.byref(cfg), a, d, r, w, s, o, ws, wsb, cnt, None)
    assert classify(mk(mg=0.0)) == BAD_ARG and classify(mk(mg=-1.0)) == BAD_ARG and classify(mk(mg=float("nan"))) == BAD_ARG
    assert classify(mk(P=-1)) == BAD_ARG and classify(mk(n_after=-1)) == BAD_ARG and classify(mk(flags=4)) == BAD_ARG
    for name in ("a", "d", "r", "w", "s", "o", "ws", "cnt"):
        assert classify(mk(), **{name: None}) == BAD_ARG, name
    assert classify(mk(), wsb=4096) == BAD_ARG                                     # workspace too small
    assert classify(mk(), ws=p + 4) == BAD_ARG                                     # ... or not 256-byte aligned
    bad = mk()
    bad.struct_size = 64
    assert classify(bad) == BAD_ARG
    assert classify(mk(flags=2)) == UNSUPPORTED and classify(mk(flags=3)) == UNSUPPORTED      # split_screen_threshold given
    assert classify(mk(P=(1 << 31) // 10 + 1)) == UNSUPPORTED                      # 10 P rows would not fit 31 bits
    assert classify(mk(P=0), a=None, ws=None, cnt=None) == OK
    ten = lambda rows=((p, p, 3, 2),): (MrgsDensifyTensor * len(rows))(*[MrgsDensifyTensor(*r) for r in rows])
    emit = lambda cfg, t, n=1, ws=p, rows=5: L.mrgs_env_densify_emit(ctypes.byref(cfg), ws, rows, t, n, 0, None, None, None)
    assert emit(bad, ten()) == BAD_ARG and emit(mk(mg=0.0), ten()) == BAD_ARG and emit(mk(flags=2), ten()) == UNSUPPORTED
    assert emit(mk(), None) == BAD_ARG and emit(mk(), ten(), ws=None) == BAD_ARG and emit(mk(), ten(), n=-1) == BAD_ARG
    assert emit(mk(), ten(), rows=-1) == BAD_ARG and emit(mk(), ten(), rows=101) == BAD_ARG      # more than 10 P rows
    assert emit(mk(), ten(((None, p, 3, 0),))) == BAD_ARG and emit(mk(), ten(((p, None, 3, 0),))) == BAD_ARG
    assert emit(mk(), ten(((p, p, 4, 2),))) == BAD_ARG                             # an XYZ row is three wide
    assert emit(mk(), ten(((p, p, 3, 3),))) == BAD_ARG                             # a SCALING row two
    assert emit(mk(), ten(((p, p, 3, 7),))) == BAD_ARG and emit(mk(), ten(((p, p, -1, 0),))) == BAD_ARG
    assert emit(mk(ptrs=(p, p, None)), ten()) == BAD_ARG                           # role XYZ needs the rotation
    assert emit(mk(P=0), ten()) == OK and emit(mk(), ten(), n=0) == OK
    assert emit(mk(), ten(), rows=0) == OK                                         # nothing survives: nothing to write
    assert emit(mk(), ten(((p, None, 3, 2),)), rows=0) == OK                       # ... and an empty destination has no address
    select = lambda n=10, v=p, k=0, ws=p, wsb=1 << 16, out=p: L.mrgs_env_select(n, v, k, ws, wsb, out, None)
    assert select(n=-1) == BAD_ARG and select(k=-1) == BAD_ARG and select(k=10) == BAD_ARG and select(n=1 << 31) == BAD_ARG
    assert select(v=None) == BAD_ARG and select(ws=None) == BAD_ARG and select(out=None) == BAD_ARG and select(wsb=64) == BAD_ARG
    assert select(n=0, v=None, ws=None, out=None) == OK
    stats = lambda P=10, g=p, v=p, wa=None, a=p, d=p, w=p: L.mrgs_env_densify_stats(P, g, v, wa, a, d, w, None)
    assert stats(P=-1) == BAD_ARG and stats(g=None) == BAD_ARG and stats(v=None) == BAD_ARG and stats(a=None) == BAD_ARG and stats(d=None) == BAD_ARG
    assert stats(wa=p, w=None) == BAD_ARG                                          # a weight to add but nowhere to add it
    assert stats(P=0, g=None, v=None, a=None, d=None, w=None) == OK


# ---------------------------------------------------------------- on the GPU ---------------------------------------------------------
MIXES = {   # g categories (never moved / below / above max_grad), max(s) categories, share of faint rows, of large radii, of unseen quiet rows
    "unseen": ([0.45, 0.20, 0.35], [0.50, 0.25, 0.15, 0.10], 0.10, 0.15, 0.6),
    "seen": ([0.45, 0.20, 0.35], [0.50, 0.25, 0.15, 0.10], 0.10, 0.15, 0.0),
    "none": ([0.5, 0.5, 0.0], [0.5, 0.5, 0.0, 0.0], 0.0, 0.0, 0.0),
    "all_pruned": ([0.45, 0.20, 0.35], [0.50, 0.25, 0.15, 0.10], 1.0, 0.15, 0.3),
}


def make_inputs(P, mix, seed):
    """Parameters, moments, the four statistics and both noises of P rows on the CPU (float32).  Every decision quantity is drawn from bands
    that stay clear of its threshold in every generation: g in {0, [0.2, 0.6], [1.5, 4]} max_grad; max(s) in t x {[0.3, 0.7], [2, 4],
    [12, 15], [30, 38]} against t and the world limit 10 t -- a stage-2 child has s / 1.6: [1.25, 2.5], [7.5, 9.4], [18.75, 23.75]; a
    stage-4 child s / 2.5 or s / 4: [4.8, 6], [12, 15.2], [7.5, 9.5] --; o in {0.018, >= 0.62}; radii in {0..5, 60..100} against 20
    (r / 1.6 >= 37.5).  A quiet row may never have been seen: accum = denom = weight = 0."""
    g_cat, s_cat, o_low, r_big, unseen = MIXES[mix]
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g)
    pick = lambda probs: torch.multinomial(torch.tensor(probs), P, replacement=True, generator=g)
    params = {n: torch.randn((P,) + sh, generator=g) for n, sh in GROUPS}
    params["xyz"] = params["xyz"] * 2.0
    gc, sc = pick(g_cat), pick(s_cat)
    gval = torch.where(gc == 0, torch.zeros(P), torch.where(gc == 1, 0.2 + 0.4 * u(P), 1.5 + 2.5 * u(P))) * MAX_GRAD
    denom = torch.randint(1, 6, (P,), generator=g).float()
    never = (gc == 0) & (u(P) < unseen)
    denom = torch.where(never, torch.zeros(P), denom)
    accum = gval * denom
    weight = denom * (0.02 + 2.0 * u(P))
    lo = torch.tensor([0.3, 2.0, 12.0, 30.0])[sc]
    hi = torch.tensor([0.7, 4.0, 15.0, 38.0])[sc]
    smax = (lo + (hi - lo) * u(P)) * T
    other = smax * (0.1 + 0.85 * u(P))
    first = u(P) < 0.5
    params["scaling"] = torch.log(torch.stack([torch.where(first, smax, other), torch.where(first, other, smax)], dim=1))
    params["opacity"] = torch.where(u(P, 1) < o_low, torch.full((P, 1), -4.0), 0.5 + 2.0 * u(P, 1))
    radii = torch.where(u(P) < r_big, 60.0 + torch.floor(41.0 * u(P)), torch.floor(6.0 * u(P)))
    moments = {n: (torch.randn(v.shape, generator=g), torch.rand(v.shape, generator=g)) for n, v in params.items()}
    stats = SimpleNamespace(accum=accum.reshape(P, 1), denom=denom.reshape(P, 1), radii=radii, weight=weight.reshape(P, 1))
    return params, moments, stats, torch.randn(P, 2, 2, generator=g), torch.randn(P, 4, 5, 2, generator=g)


def make_model(params, moments, stats, dev, stepped=True, max_gs=2e6):
    from materialrefgs_amd.env_model import EnvGaussianModel
    model = EnvGaussianModel(3)
    for n, _ in GROUPS:
        setattr(model, ATTRS[n], torch.nn.Parameter(params[n].to(dev)))
    model.spatial_lr_scale = 1.0
    model.training_setup(OPT)
    assert model.percent_dense == PERCENT_DENSE
    model.max_gs = max_gs
    if stepped:
        for gr in model.optimizer.param_groups:
            m, v = moments[gr["name"]]
            model.optimizer.state[gr["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": m.to(dev), "exp_avg_sq": v.to(dev)}
    model.xyz_gradient_accum, model.denom = stats.accum.to(dev), stats.denom.to(dev)
    model.max_radii2D, model.xyz_weight_accum = stats.radii.to(dev), stats.weight.to(dev)
    return model


def bits(x):
    return torch.as_tensor(x, dtype=torch.float32).reshape(1).view(torch.int32).item()


def check_against_statement(model, ref, counts, stepped=True):
    """Order and counts exact, copies bit for bit, zero moments on every new row, four zero statistics of the right length, a consistent
    optimizer, the two computed tensors within the statement's bounds (one generation's bound per generation, summed)."""
    i = ref.info
    assert counts.rows == ref.rows and counts.segments == es.segments(ref), (counts.segments, es.segments(ref))
    assert (counts.n_clone, counts.n_split, counts.n_stage3, counts.n_pruned4, counts.n_split4, counts.n_pruned5) == \
        (i.n_clone, i.n_split, i.n_stage3, i.n_pruned4, i.n_split4, i.n_pruned5)
    # the weight path: the same float32 bits
    assert bits(counts.W0) == bits(i.W0)
    if i.W1 is not None:
        assert bits(counts.W1) == bits(i.W1)
    if i.W4 is not None:
        assert bits(counts.W4) == bits(i.W4)
    if i.q is not None:
        assert bits(counts.q) == bits(i.q), (counts.q, float(i.q))
    if i.n_pruned5:
        assert counts.capped and float(counts.cut) == float(i.cut)
    opt = model.optimizer
    new = (ref.gen > 0) | (ref.slot == 1)
    assert [g["name"] for g in opt.param_groups] == [n for n, _ in GROUPS]
    for gr in opt.param_groups:
        p, name = gr["params"][0], gr["name"]
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.dtype == torch.float32
        assert getattr(model, ATTRS[name]) is p
        got, want = p.detach().cpu().double(), ref.tensors[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if name == "scaling":
            assert torch.equal(got[ref.gen == 0], want[ref.gen == 0])
            bound = ref.gen.double().unsqueeze(1) * es.SCALING_REL * want.abs().clamp(min=1.0)
            assert bool(((got - want).abs() <= bound).all())
        elif name == "xyz":
            assert torch.equal(got[ref.gen == 0], want[ref.gen == 0])
            err = (got - want).abs().max(dim=1).values
            assert bool((err <= ref.xyz_bound).all()), float((err / ref.xyz_bound.clamp(min=1e-30)).max())
        else:
            assert torch.equal(got, want), name
        if stepped:
            st = opt.state[p]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
            for kind, want_m in zip(("exp_avg", "exp_avg_sq"), ref.moments[name]):
                assert st[kind].dtype == torch.float32 and torch.equal(st[kind].cpu().double(), want_m), (name, kind)
                assert float(st[kind][new.to(st[kind].device)].abs().sum()) == 0.0
        else:
            assert p not in opt.state
    assert len(opt.state) == (len(opt.param_groups) if stepped else 0)
    rows = ref.rows
    assert model.xyz_gradient_accum.shape == (rows, 1) and model.denom.shape == (rows, 1) and model.xyz_weight_accum.shape == (rows, 1)
    assert model.max_radii2D.shape == (rows,)
    for s in (model.xyz_gradient_accum, model.denom, model.xyz_weight_accum, model.max_radii2D):
        assert s.dtype == torch.float32 and s.is_cuda and float(s.abs().sum()) == 0.0


def run_case(dev, P, mix, seed, max_screen_size=20, stepped=True, max_gs=2e6, inputs=None):
    params, moments, stats, noise, noise4 = inputs or make_inputs(P, mix, seed)
    ref = es.densify_and_prune(params, moments if stepped else None, stats.accum, stats.denom, stats.radii, stats.weight, PERCENT_DENSE, MAX_GRAD,
                               MIN_OPACITY, EXTENT, max_screen_size, noise, noise4, max_gs=max_gs)
    assert ref.margin >= 1e-3, ref.margin                                                # the condition of the exact comparison
    model = make_model(params, moments, stats, dev, stepped, max_gs)
    counts = model.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, noise=noise.to(dev), noise4=noise4.to(dev))
    check_against_statement(model, ref, counts, stepped)
    return model, ref, params


def single_row_fate(ref):
    if ref.rows == 0:
        return "pruned"
    if int(ref.gen.max()) == 0:
        return "cloned" if ref.info.n_clone else "kept"
    return "split once" if int(ref.gen.max()) == 1 else "split twice"


SINGLE_ROW_SEEDS = (17, 0, 5, 3, 51)       # pruned, kept, cloned, split once, split twice (make_inputs(1, "seen", seed))


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 5000, 11009])     # 11 009 rows: 44 blocks, 24 * 44 = 1056 count words, two scan steps
def test_row_counts_around_the_block_edge(gpu_device, P):
    if P == 1:
        fates = [single_row_fate(run_case(gpu_device, 1, "seen", seed)[1]) for seed in SINGLE_ROW_SEEDS]
        assert fates == ["pruned", "kept", "cloned", "split once", "split twice"]
        return
    _m, ref, _p = run_case(gpu_device, P, "seen", P)
    i = ref.info
    assert min(i.n_clone, i.n_split, i.n_pruned4, i.n_split4) > 0 and int(ref.gen.max()) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1023, 5000])
def test_unseen_mix_has_a_zero_quantile_and_still_splits_in_five(gpu_device, P):
    _m, ref, _p = run_case(gpu_device, P, "unseen", 20 + P)
    assert float(ref.info.q) == 0.0 and ref.info.n_pruned4 == 0 and ref.info.n_split4 > 0
    assert int((ref.info.wavg4 == 0).sum()) >= 0.1 * ref.info.n_stage3


@pytest.mark.gpu
def test_seen_mix_prunes_and_splits_at_stage_four(gpu_device):
    _m, ref, _p = run_case(gpu_device, 5000, "seen", 31)
    assert float(ref.info.q) > 0.0 and ref.info.n_pruned4 > 0 and ref.info.n_split4 > 0
    assert int((ref.gen == 2).sum()) > 0 and int(((ref.child4 >= 0) & (ref.slot == 1)).sum()) > 0       # grandchildren, and children of clones


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["idle", "half", "ties"])
def test_visibility_cap(gpu_device, setting):
    """max_gs above the row count: stage 5 idle; at about half: rows - int(max_gs 0.9) rows go; and so that the cut falls inside the group of
    wavg == 0 rows, where the earlier row goes first."""
    P = 1025
    inputs = make_inputs(P, "unseen", 41)
    params, moments, stats, noise, noise4 = inputs
    free = es.densify_and_prune(params, None, stats.accum, stats.denom, stats.radii, stats.weight, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY, EXTENT, 20,
                                noise, noise4)
    zeros = int((free.info.wavg5 == 0).sum())
    assert free.info.n_pruned5 == 0 and zeros > 20
    n_after = {"idle": free.rows + 1, "half": free.rows // 2, "ties": free.rows - zeros // 2}[setting]
    max_gs = (n_after + 0.5) / 0.9
    assert int(max_gs * 0.9) == n_after
    _m, ref, _p = run_case(gpu_device, P, "unseen", 41, max_gs=max_gs, inputs=inputs)
    assert ref.rows == min(free.rows, n_after) and ref.info.n_pruned5 == free.rows - ref.rows
    if setting == "ties":
        assert float(ref.info.cut) == 0.0 and 0 < ref.info.n_pruned5 < zeros
    if setting == "half":
        assert float(ref.info.cut) > 0.0


@pytest.mark.gpu
def test_nothing_selected_nothing_pruned_is_the_identity(gpu_device):
    model, ref, params = run_case(gpu_device, 5000, "none", 12)
    assert ref.rows == 5000 and es.segments(ref)[0] == 5000
    for n, _ in GROUPS:
        assert torch.equal(getattr(model, ATTRS[n]).detach().cpu(), params[n])


@pytest.mark.gpu
def test_every_row_pruned_leaves_a_consistent_empty_model(gpu_device):
    model, ref, _p = run_case(gpu_device, 5000, "all_pruned", 14)
    assert ref.rows == 0 and ref.info.q is None and model._xyz.shape == (0, 3) and model._features_rest.shape == (0, 15, 3)


@pytest.mark.gpu
def test_max_screen_size_none_against_twenty(gpu_device):
    _m, with_limit, _p = run_case(gpu_device, 5000, "seen", 15, max_screen_size=20)
    _m, without, _p = run_case(gpu_device, 5000, "seen", 15, max_screen_size=None)
    assert with_limit.info.n_split4 + with_limit.info.n_pruned4 > without.info.n_split4 + without.info.n_pruned4 > 0


@pytest.mark.gpu
def test_before_the_optimizers_first_step(gpu_device):
    run_case(gpu_device, 1025, "seen", 17, stepped=False)


@pytest.mark.gpu
def test_empty_model_and_refusals(gpu_device):
    params = {n: torch.zeros((0,) + sh) for n, sh in GROUPS}
    moments = {n: (v.clone(), v.clone()) for n, v in params.items()}
    stats = SimpleNamespace(accum=torch.zeros(0, 1), denom=torch.zeros(0, 1), radii=torch.zeros(0), weight=torch.zeros(0, 1))
    model = make_model(params, moments, stats, gpu_device)
    before = [gr["params"][0] for gr in model.optimizer.param_groups]
    counts = model.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20)
    assert counts.rows == 0 and all(a is b["params"][0] for a, b in zip(before, model.optimizer.param_groups))
    assert model.xyz_gradient_accum.shape == (0, 1) and model.xyz_weight_accum.shape == (0, 1) and model.max_radii2D.shape == (0,)
    with pytest.raises(NotImplementedError, match="split_screen_threshold"):
        model.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, 20, 0.1)


# ---- the generator -------------------------------------------------------------------------------------------------------------
def unit_model(P, dev):
    """xyz = 0, identity rotation, raw scaling 0 (s = 1), g = 2 max_grad, every weight 1: every row is split in 2, and with extent 5 (world
    limit 0.5 < 0.625) each child again in 5 -- all wavg are equal, so q = wavg and nothing is low."""
    params = {n: torch.zeros((P,) + sh) for n, sh in GROUPS}
    params["rotation"][:, 0] = 1.0
    params["opacity"] += 2.0
    stats = SimpleNamespace(accum=torch.full((P, 1), 2.0 * MAX_GRAD), denom=torch.ones(P, 1), radii=torch.zeros(P), weight=torch.ones(P, 1))
    return make_model(params, None, stats, dev, stepped=False)


@pytest.mark.gpu
def test_generator_against_the_numpy_statement(gpu_device):
    dev, P = gpu_device, 3000
    seed = 0x9E3779B97F4A7C15
    rows = np.arange(P)
    # stage 2 alone (extent 50: t = 0.5 < 1 < the world limit 5): a child's centre IS (z0, z1, 0)
    model = unit_model(P, dev)
    counts = model.densify_and_prune(MAX_GRAD, MIN_OPACITY, 50.0, None, seed=seed)
    assert counts.segments[:4] == (0, 0, P, P) and counts.rows == 2 * P
    z2 = model._xyz.detach().cpu().reshape(2, P, 3)
    assert float(z2[..., 2].abs().max()) == 0.0
    for k in range(2):
        # angle in fp32: 2 pi 2^-24 = 3.7e-7 on cos, x radius <= 5.77 = 2.2e-6; the radius's <= 4 ulp: 2.8e-6; 1e-5 is the sum doubled
        assert np.abs(z2[k, :, :2].double().numpy() - es.philox_normals(seed, rows, k)).max() <= 1e-5
    # both generations (extent 5): child j of stage-2 child k sits at z2[k] + 0.625 z4[2 + k, j]; the bound is one generation's per generation
    model = unit_model(P, dev)
    counts = model.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, seed=seed)
    assert counts.rows == 10 * P and counts.segments[:4] == (0, 0, 0, 0) and counts.q == 1.0
    z = model._xyz.detach().cpu().reshape(5, 2, P, 3)
    s1 = math.exp(math.log(1.0 / 1.6))
    for j in range(5):
        for k in range(2):
            want = es.philox_normals(seed, rows, k) + s1 * es.philox_normals(seed, rows, j, 1 + 2 + k)
            assert np.abs(z[j, k, :, :2].double().numpy() - want).max() <= 1e-5 * (1 + s1)
    again = unit_model(P, dev)
    again.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, seed=seed)
    assert torch.equal(again._xyz, model._xyz)                                           # same seed: identical bits
    other = unit_model(P, dev)
    other.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, seed=seed + 1)
    assert not bool((other._xyz[:, :2] == model._xyz[:, :2]).any())
    # noise / noise4 take over: zeros put every child on its source; noise alone leaves stage 4 to the generator
    zero2, zero4 = torch.zeros(P, 2, 2, device=dev), torch.zeros(P, 4, 5, 2, device=dev)
    m0 = unit_model(P, dev)
    m0.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, noise=zero2, noise4=zero4)
    assert float(m0._xyz.abs().max()) == 0.0
    m1 = unit_model(P, dev)
    m1.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, seed=seed, noise=zero2)
    want = s1 * es.philox_normals(seed, rows, 4, 1 + 3)
    assert np.abs(m1._xyz.detach().cpu().reshape(5, 2, P, 3)[4, 1, :, :2].double().numpy() - want).max() <= 1e-5 * s1
    m2 = unit_model(P, dev)
    m2.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None, seed=seed, noise4=zero4)
    assert torch.equal(m2._xyz.reshape(5, 2 * P, 3)[3], z2.reshape(2 * P, 3).to(dev))
    # seed=None: torch's CPU default generator governs the call
    outs = []
    for s in (7, 7, 8):
        torch.manual_seed(s)
        m = unit_model(64, dev)
        m.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None)
        outs.append(m._xyz)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---- the select kernel alone ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_select_kernel_against_sort(gpu_device, n):
    from materialrefgs_amd.env_model import select_kth
    g = torch.Generator().manual_seed(n)
    mixed = torch.randn(n, generator=g) * 3.0
    mixed[torch.rand(n, generator=g) < 0.2] = 0.0
    mixed[torch.rand(n, generator=g) < 0.1] = -0.0
    mixed[torch.rand(n, generator=g) < 0.05] = float("inf")
    few = torch.randint(-2, 3, (n,), generator=g).float()                                # many ties, negatives
    vectors = {"equal": torch.full((n,), 1.5), "zeros": torch.where(torch.rand(n, generator=g) < 0.5, 0.0, -0.0), "mixed": mixed, "few": few,
               "inf": torch.full((n,), float("inf"))}
    for name, v in vectors.items():
        s = torch.sort(v).values
        for k in sorted({0, n - 1, n // 10, n // 2, min(n - 1, 255), min(n - 1, 256)}):
            value, less, equal = select_kth(v.to(gpu_device), k)
            want = float(s[k])
            assert value == want, (name, k, value, want)                                 # -0 == +0: one value
            assert less == int((v < want).sum()) and equal == int((v == want).sum()), (name, k)


# ---- the statistics kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1025, 5000])
@pytest.mark.parametrize("mask", ["half", "none", "all"])
def test_statistics_kernel(gpu_device, P, mask):
    from materialrefgs_amd.env_model import EnvGaussianModel
    dev = gpu_device
    g = torch.Generator().manual_seed(P)
    accum, denom = torch.rand(P, 1, generator=g), torch.randint(0, 9, (P, 1), generator=g).float()
    wacc, radii = torch.rand(P, 1, generator=g) * 4.0, torch.randint(0, 40, (P,), generator=g).float()
    grad, wnew = torch.randn(P, 3, generator=g) * 1e-3, torch.rand(P, 1, generator=g)
    vis = {"half": torch.rand(P, generator=g) < 0.5, "none": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool)}[mask]
    leaf = torch.zeros(P, 3, device=dev, requires_grad=True)
    leaf.grad = grad.to(dev)
    for with_weight in (True, False):
        want_a, want_d, want_w = es.add_densification_stats(accum, denom, wacc, grad, vis, wnew if with_weight else None)
        model = EnvGaussianModel(3)
        model.xyz_gradient_accum, model.denom, model.xyz_weight_accum, model.max_radii2D = accum.to(dev), denom.to(dev), wacc.to(dev), radii.to(dev)
        addr = tuple(t.data_ptr() for t in (model.xyz_gradient_accum, model.denom, model.xyz_weight_accum))
        model.add_densification_stats(leaf, vis.to(dev), wnew.to(dev) if with_weight else None)
        assert addr == tuple(t.data_ptr() for t in (model.xyz_gradient_accum, model.denom, model.xyz_weight_accum))      # in place
        got_a, got_d, got_w = model.xyz_gradient_accum.cpu(), model.denom.cpu(), model.xyz_weight_accum.cpu()
        assert torch.equal(got_d.double(), want_d) and torch.equal(model.max_radii2D.cpu(), radii)                       # max_radii2D is not touched
        # the norm's six roundings and the add stay within one ulp of the sum; the weight is one rounded add
        ulp = lambda t: 2.0 ** torch.floor(torch.log2(t.abs().clamp(min=1e-30))) * 2.0 ** -23
        assert bool(((got_a.double() - want_a).abs() <= ulp(want_a)).all())
        assert bool(((got_w.double() - want_w).abs() <= ulp(want_w)).all())
        assert torch.equal(got_a[~vis], accum[~vis]) and torch.equal(got_d[~vis], denom[~vis]) and torch.equal(got_w[~vis], wacc[~vis])
        if not with_weight:
            assert torch.equal(got_w, wacc)
