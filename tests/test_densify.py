"""densify_and_prune and the densification statistics (materialrefgs_amd/densify.py, csrc/mrgs_densify.hip) against the float64
three-stage statement of tests/densify_statement.py.  Every input set keeps each decision quantity >= 1e-3 (relative) away from its
threshold -- asserted on the statement's side -- so that the decision sets, the counts and the row order must agree EXACTLY; copied rows
and moments are compared bit for bit, the two computed quantities (a child's raw scaling and centre) within bounds derived below."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import densify_statement as ds

# the sixteen per-gaussian groups of GaussianModel.training_setup (gaussian_model.py:422-447) with their row shapes
GROUPS = [("xyz", (3,)), ("refl_strength", (1,)), ("metalness", (1,)), ("roughness", (1,)), ("ori_color", (3,)), ("diffuse_color", (3,)),
          ("normal1", (3,)), ("normal2", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("ind_dc", (1, 3)), ("ind_rest", (15, 3)),
          ("ind_asg", (32, 5)), ("opacity", (1,)), ("scaling", (2,)), ("rotation", (4,))]
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "refl_strength": "_refl_strength", "ori_color": "_ori_color", "diffuse_color": "_diffuse_color",
         "roughness": "_roughness", "metalness": "_metalness", "normal1": "_normal1", "normal2": "_normal2", "ind_dc": "_indirect_dc",
         "ind_rest": "_indirect_rest", "ind_asg": "_indirect_asg"}
PERCENT_DENSE, EXTENT, MAX_GRAD, MIN_OPACITY = 0.01, 5.0, 0.0002, 0.05
T = PERCENT_DENSE * EXTENT


# ---------------------------------------------------------------- without a GPU ------------------------------------------------------
def test_group_attribute_map_covers_training_setup():
    from materialrefgs_amd import densify
    assert len(ATTRS) == 16 and densify.GROUP_ATTRS == ATTRS
    assert all(densify.group_attr(n) == a for n, a in ATTRS.items())
    assert densify.group_attr("anything_else") == "_anything_else"
    assert densify.SKIP_GROUPS == ("mlp", "env", "env2")


def test_size_query_and_argument_validation_without_gpu():
    """Every contract violation is a status code before any HIP call; P = 0 is MRGS_OK with nothing launched."""
    from materialrefgs_amd import _lib, densify
    from materialrefgs_amd._lib import MrgsDensifyConfig, MrgsDensifyTensor
    L = _lib.lib()
    OK, BAD_ARG, UNSUPPORTED = 0, 1, 6
    assert ctypes.sizeof(MrgsDensifyConfig) == 56 and ctypes.sizeof(MrgsDensifyTensor) == 24
    assert L.mrgs_densify_ws_bytes(0) > 0
    assert L.mrgs_densify_ws_bytes(5000) >= 5000 + 6 * 5 * 4                       # a class byte a row, 2 x 3 words a block
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)                                                      # never dereferenced: every call below is refused
    mk = lambda N=2, P=10, mg=0.1, ptrs=(p, p, p): MrgsDensifyConfig(N, P, mg, 0.05, 0.1, 0.0, *ptrs)
    classify = lambda cfg, a=p, ws=p, wsb=1 << 20, cnt=p: L.mrgs_densify_classify(ctypes.byref(cfg), a, p, p, p, ws, wsb, cnt, None)
    assert classify(mk(N=0)) == BAD_ARG and classify(mk(N=9)) == BAD_ARG
    assert classify(mk(mg=0.0)) == BAD_ARG and classify(mk(mg=-1.0)) == BAD_ARG and classify(mk(mg=float("nan"))) == BAD_ARG
    assert classify(mk(P=-1)) == BAD_ARG
    assert classify(mk(), a=None) == BAD_ARG and classify(mk(), ws=None) == BAD_ARG and classify(mk(), cnt=None) == BAD_ARG
    assert classify(mk(), wsb=16) == BAD_ARG                                       # workspace too small
    bad = mk()
    bad.struct_size = 48
    assert classify(bad) == BAD_ARG
    assert classify(mk(P=1 << 30)) == UNSUPPORTED                                  # 2 P rows would not fit 31 bits
    assert classify(mk(N=8, P=1 << 28)) == UNSUPPORTED
    assert classify(mk(P=0), a=None, ws=None, cnt=None) == OK
    counts = (ctypes.c_int64 * 3)(5, 1, 1)
    ten = lambda rows=((p, p, 3, 2),): (MrgsDensifyTensor * len(rows))(*[MrgsDensifyTensor(*r) for r in rows])
    emit = lambda cfg, t, n=1, ws=p, c=counts: L.mrgs_densify_emit(ctypes.byref(cfg), ws, c, t, n, 0, None, None)
    assert emit(mk(N=9), ten()) == BAD_ARG and emit(bad, ten()) == BAD_ARG
    assert emit(mk(), None) == BAD_ARG and emit(mk(), ten(), ws=None) == BAD_ARG and emit(mk(), ten(), c=None) == BAD_ARG
    assert emit(mk(), ten(((None, p, 3, 0),))) == BAD_ARG and emit(mk(), ten(((p, None, 3, 0),))) == BAD_ARG
    assert emit(mk(), ten(((p, p, 4, 2),))) == BAD_ARG                             # an XYZ row is three wide
    assert emit(mk(), ten(((p, p, 3, 3),))) == BAD_ARG                             # a SCALING row two
    assert emit(mk(), ten(((p, p, 3, 7),))) == BAD_ARG and emit(mk(), ten(((p, p, -1, 0),))) == BAD_ARG
    assert emit(mk(ptrs=(p, p, None)), ten()) == BAD_ARG                           # role XYZ needs the rotation
    assert emit(mk(), ten(), c=(ctypes.c_int64 * 3)(11, 0, 0)) == BAD_ARG          # more rows kept than there are
    assert emit(mk(), ten(), c=(ctypes.c_int64 * 3)(0, -1, 0)) == BAD_ARG
    assert emit(mk(P=0), ten()) == OK and emit(mk(), ten(), n=0) == OK
    assert emit(mk(), ten(), c=(ctypes.c_int64 * 3)(0, 0, 0)) == OK                # nothing survives: nothing to write
    assert emit(mk(), ten(((p, None, 3, 2),)), c=(ctypes.c_int64 * 3)(0, 0, 0)) == OK      # ... and an empty destination has no address
    stats = lambda P=10, g=p, v=p, a=p, d=p: L.mrgs_densify_stats(P, g, v, None, a, d, None, None)
    assert stats(P=-1) == BAD_ARG and stats(g=None) == BAD_ARG and stats(v=None) == BAD_ARG and stats(a=None) == BAD_ARG and stats(d=None) == BAD_ARG
    assert stats(P=0, g=None, v=None, a=None, d=None) == OK
    # the Python surface refuses before it touches the library
    model = SimpleNamespace(optimizer=None)
    for mg in (0.0, -0.1):
        with pytest.raises(ValueError, match="max_grad"):
            densify.densify_and_prune(model, mg, 0.05, 5.0, None)
    with pytest.raises(ValueError, match="N must"):
        densify.densify_and_prune(model, 0.1, 0.05, 5.0, None, N=0)
    with pytest.raises(ValueError, match="N must"):
        densify.densify_and_prune(model, 0.1, 0.05, 5.0, None, N=9)


def _cpu_model(widths=None):
    P = 4
    groups = [{"params": [torch.nn.Parameter(torch.zeros((P,) + sh))], "lr": 0.01, "name": n} for n, sh in GROUPS if widths is None or n in widths]
    m = SimpleNamespace(optimizer=torch.optim.Adam(groups, lr=0.0, eps=1e-15), percent_dense=0.01, xyz_gradient_accum=torch.zeros(P, 1),
                        denom=torch.zeros(P, 1), max_radii2D=torch.zeros(P))
    for g in groups:
        setattr(m, ATTRS[g["name"]], g["params"][0])
    return m


def test_python_surface_refuses_what_it_does_not_serve():
    """CPU tensors, non-fp32 parameters, scaling rows that are not two wide, a per-gaussian group without its attribute: all raise."""
    from materialrefgs_amd import densify
    with pytest.raises(RuntimeError, match="device tensor"):
        densify.densify_and_prune(_cpu_model(), 0.1, 0.05, 5.0, None)
    m = _cpu_model()
    del m._normal1
    with pytest.raises(AttributeError, match="_normal1"):
        densify.densify_and_prune(m, 0.1, 0.05, 5.0, None)
    with pytest.raises(ValueError, match="rotation"):
        densify.densify_and_prune(_cpu_model(widths=("xyz", "scaling", "opacity")), 0.1, 0.05, 5.0, None)
    with pytest.raises(RuntimeError, match="device tensor"):
        densify.add_densification_stats((torch.zeros(4, 1), torch.zeros(4, 1)), torch.zeros(4, 3), torch.ones(4, dtype=torch.bool))


def test_statement_on_a_hand_worked_case():
    """Six rows, t = 0.1, max_grad = 0.5, min_opacity = 0.05, world limit 0.1 * extent = 1, N = 2, identity rotations:
       row 0  g = 2/2 = 1,   s = 0.05          -> cloned            row 3  g = 0.1, s = (2, 0.05) > 1    -> pruned (over-sized)
       row 1  g = 3/2 = 1.5, s = (0.4, 0.2)    -> split, removed    row 4  0/0 -> g = 0                  -> kept
       row 2  g = 0.1, o = sigmoid(-5) < 0.05  -> pruned            row 5  g = 0.2                       -> kept
    children of row 1: scale (0.4, 0.2) / 1.6 = (0.25, 0.125); centres (1,2,3) + (0.4 z0, 0.2 z1, 0) with z = (1,-1) and (0.5, 2).
    Result: originals 0, 4, 5; the clone of 0; first child; second child."""
    lg = math.log
    f = lambda rows: torch.tensor(rows, dtype=torch.float64)
    params = {"xyz": f([[0, 0, 0], [1, 2, 3], [2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 5]]),
              "scaling": f([[lg(0.05)] * 2, [lg(0.4), lg(0.2)], [lg(0.05)] * 2, [lg(2.0), lg(0.05)], [lg(0.05)] * 2, [lg(0.05)] * 2]),
              "rotation": f([[1, 0, 0, 0]] * 6), "opacity": f([[0], [0], [-5], [0], [0], [0]]),
              "f_dc": f([[10], [11], [12], [13], [14], [15]])}
    moments = {k: (v + 100.0, v + 200.0) for k, v in params.items()}
    accum, denom = f([[2], [3], [0.1], [0.1], [0], [0.2]]), f([[2], [2], [1], [1], [0], [1]])
    noise = torch.zeros(6, 2, 2, dtype=torch.float64)
    noise[1] = f([[1, -1], [0.5, 2]])
    r = ds.densify_and_prune(params, moments, accum, denom, 0.01, 0.5, 0.05, 10.0, 20, noise, N=2)
    assert r.counts == (3, 1, 1)
    assert r.row.tolist() == [0, 4, 5, 0, 1, 1] and r.kind.tolist() == [0, 0, 0, 1, 2, 3]
    assert r.clone.tolist() == [True, False, False, False, False, False] and r.split.tolist() == [False, True, False, False, False, False]
    assert torch.allclose(r.tensors["xyz"], f([[0, 0, 0], [4, 4, 4], [5, 5, 5], [0, 0, 0], [1.4, 1.8, 3], [1.2, 2.4, 3]]), atol=1e-14, rtol=0)
    assert torch.allclose(r.tensors["scaling"], f([[lg(0.05)] * 2] * 4 + [[lg(0.25), lg(0.125)]] * 2), atol=1e-14, rtol=0)
    assert torch.equal(r.tensors["f_dc"], f([[10], [14], [15], [10], [11], [11]]))
    assert torch.equal(r.tensors["opacity"], torch.zeros(6, 1, dtype=torch.float64))
    for k in params:
        m, v = r.moments[k]
        assert torch.equal(m[:3], params[k][[0, 4, 5]] + 100.0) and torch.equal(v[:3], params[k][[0, 4, 5]] + 200.0)
        assert torch.equal(m[3:], torch.zeros_like(m[3:])) and torch.equal(v[3:], torch.zeros_like(v[3:]))
    assert all(s.shape[0] == 6 and float(s.abs().sum()) == 0.0 for s in r.stats) and r.stats[2].dim() == 1
    assert abs(r.margin - 0.5) < 1e-12                               # s = 0.05 against t = 0.1 is the closest call of the case
    # without max_screen_size the over-sized row stays; with the transparent row opaque it stays too
    r2 = ds.densify_and_prune(params, None, accum, denom, 0.01, 0.5, 0.05, 10.0, None, noise, N=2)
    assert r2.counts == (4, 1, 1) and r2.row.tolist() == [0, 3, 4, 5, 0, 1, 1] and r2.moments is None
    # the per-iteration lines
    a, d, mr = ds.add_densification_stats(f([[1], [2]]), f([[3], [4]]), f([5, 1]), f([[3, 4, 12], [1, 1, 1]]), torch.tensor([True, False]),
                                          torch.tensor([7, 9], dtype=torch.int32))
    assert a.tolist() == [[14.0], [2.0]] and d.tolist() == [[4.0], [4.0]] and mr.tolist() == [7.0, 1.0]


def test_philox_statement_known_answer():
    """Philox4x32-10 with zero key and counter gives the published first words 6627e8d5 e169c58d (Random123 kat_vectors)."""
    n0, n1, z = ds.philox_normals(0, np.array([0]), 0)
    assert int(n0[0]) == (0x6627e8d5 >> 8) + 1 and int(n1[0]) == (0xe169c58d >> 8) + 1
    assert np.all(np.isfinite(z))


# ---------------------------------------------------------------- on the GPU ---------------------------------------------------------
def make_decision_inputs(P, mix, g):
    """The decision inputs of P rows from generator g: accum [P,1], denom [P,1], raw scaling [P,2], raw opacity [P,1] (CPU, float32).  Every
    decision quantity is drawn from bands that stay well clear of its threshold: g in {0, [0.2, 0.6] max_grad, [1.5, 4] max_grad}; max(s) in
    t x {[0.3, 0.7], [2, 4], [11, 14], [30, 40]} (world limit 0.1 extent = 10 t; children are s / (0.8 N), N = 2, 3: [1.25, 2.5] t,
    [4.6, 8.75] t, [12.5, 25] t); o in {0.018, >= 0.62}."""
    u = lambda *sh: torch.rand(*sh, generator=g)
    pick = lambda probs: torch.multinomial(torch.tensor(probs), P, replacement=True, generator=g)
    g_cat = {"typical": [0.35, 0.35, 0.30], "none": [0.5, 0.5, 0.0], "all_split": [0.0, 0.0, 1.0], "all_pruned": [0.35, 0.35, 0.30]}[mix]
    s_cat = {"typical": [0.65, 0.25, 0.05, 0.05], "none": [0.5, 0.5, 0.0, 0.0], "all_split": [0.0, 0.8, 0.2, 0.0], "all_pruned": [0.6, 0.3, 0.05, 0.05]}[mix]
    o_low = {"typical": 0.10, "none": 0.0, "all_split": 0.0, "all_pruned": 1.0}[mix]
    gc, sc = pick(g_cat), pick(s_cat)
    gval = torch.where(gc == 0, torch.zeros(P), torch.where(gc == 1, 0.2 + 0.4 * u(P), 1.5 + 2.5 * u(P))) * MAX_GRAD
    denom = torch.randint(1, 6, (P,), generator=g).float()
    denom = torch.where((gc == 0) & (u(P) < 0.3), torch.zeros(P), denom)                  # never seen: 0 / 0
    accum = gval * denom
    lo = torch.tensor([0.3, 2.0, 11.0, 30.0])[sc]
    hi = torch.tensor([0.7, 4.0, 14.0, 40.0])[sc]
    smax = (lo + (hi - lo) * u(P)) * T
    other = smax * (0.1 + 0.85 * u(P))
    first = u(P) < 0.5
    scaling = torch.log(torch.stack([torch.where(first, smax, other), torch.where(first, other, smax)], dim=1))
    opacity = torch.where(u(P, 1) < o_low, torch.full((P, 1), -4.0), 0.5 + 2.0 * u(P, 1))
    return accum.reshape(P, 1), denom.reshape(P, 1), scaling, opacity


def make_inputs(P, mix, seed, N=2):
    """Parameters, moments, statistics and noise of P rows on the CPU (float32); the decision inputs are make_decision_inputs'."""
    g = torch.Generator().manual_seed(seed)
    params = {n: torch.randn((P,) + sh, generator=g) for n, sh in GROUPS}
    params["xyz"] = params["xyz"] * 2.0
    accum, denom, params["scaling"], params["opacity"] = make_decision_inputs(P, mix, g)
    moments = {n: (torch.randn(v.shape, generator=g), torch.rand(v.shape, generator=g)) for n, v in params.items()}
    noise = torch.randn(P, N, 2, generator=g)
    return params, moments, accum, denom, noise


def make_model(params, moments, accum, denom, dev, stepped=True):
    from materialrefgs_amd.optim import Adam
    groups = [{"params": [torch.nn.Parameter(params[n].to(dev))], "lr": 0.01, "name": n} for n, _ in GROUPS]
    env = torch.nn.Parameter(torch.ones(6, 4, 4, 3, device=dev))
    groups.insert(6, {"params": [env], "lr": 0.01, "name": "env"})
    opt = Adam(groups, lr=0.0, eps=1e-15)
    if stepped:
        for gr in opt.param_groups:
            p = gr["params"][0]
            m, v = (moments[gr["name"]] if gr["name"] != "env" else (torch.ones(p.shape), torch.ones(p.shape)))
            opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": m.to(dev), "exp_avg_sq": v.to(dev)}
    P = accum.shape[0]
    model = SimpleNamespace(optimizer=opt, percent_dense=PERCENT_DENSE, xyz_gradient_accum=accum.to(dev), denom=denom.to(dev),
                            max_radii2D=torch.full((P,), 50.0, device=dev), env=env)          # radii beyond any max_screen_size: the quirk
    for gr in opt.param_groups:
        if gr["name"] != "env":
            setattr(model, ATTRS[gr["name"]], gr["params"][0])
    return model


def check_against_statement(model, ref, params, N, stepped=True):
    """Everything the issue lists: order and counts exact, copies bit for bit, zero moments and statistics, the two computed tensors
    within their bounds, and a consistent optimizer."""
    opt = model.optimizer
    rows = ref.tensors["xyz"].shape[0]
    child = ref.kind >= 2
    for gr in opt.param_groups:
        p = gr["params"][0]
        if gr["name"] == "env":
            assert p is model.env and p.shape == (6, 4, 4, 3)
            if stepped:
                assert float(opt.state[p]["exp_avg"].sum()) == p.numel()
            continue
        name = gr["name"]
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.dtype == torch.float32
        assert getattr(model, ATTRS[name]) is p
        got, want = p.detach().cpu().double(), ref.tensors[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if name == "scaling":
            assert torch.equal(got[~child], want[~child])
            # exp and log at <= 2 ulp each, one division, the fp32 0.8 N: ~3e-7, factor three
            assert bool(((got[child] - want[child]).abs() <= 1e-6 * want[child].abs().clamp(min=1.0)).all())
        elif name == "xyz":
            assert torch.equal(got[~child], want[~child])
            # normalisation, nine rotation entries of two products each, two products and two sums per coordinate, one add
            parent = params["xyz"].double()[ref.row]                                      # the bound's ||xyz|| is the parent's centre
            bound = 16 * 2.0 ** -24 * (parent.abs().max(dim=1).values + ref.offset_norm)
            err = (got - want).abs().max(dim=1).values
            assert bool((err[child] <= bound[child]).all()), float((err[child] / bound[child]).max())
        else:
            assert torch.equal(got, want), name
        if stepped:
            st = opt.state[p]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
            for kind, want_m in zip(("exp_avg", "exp_avg_sq"), ref.moments[name]):
                assert st[kind].dtype == torch.float32 and torch.equal(st[kind].cpu().double(), want_m), (name, kind)
                assert float(st[kind][ref.kind.to(st[kind].device) > 0].abs().sum()) == 0.0
        else:
            assert p not in opt.state
    assert len(opt.state) == (len(opt.param_groups) if stepped else 0)
    assert model.xyz_gradient_accum.shape == (rows, 1) and model.denom.shape == (rows, 1) and model.max_radii2D.shape == (rows,)
    for s in (model.xyz_gradient_accum, model.denom, model.max_radii2D):
        assert s.dtype == torch.float32 and s.is_cuda and float(s.abs().sum()) == 0.0


def run_case(dev, P, mix, seed, N=2, max_screen_size=20, stepped=True):
    from materialrefgs_amd import densify
    params, moments, accum, denom, noise = make_inputs(P, mix, seed, N)
    ref = ds.densify_and_prune(params, moments if stepped else None, accum, denom, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size,
                               noise, N=N)
    assert ref.margin >= 1e-3, ref.margin                                                # the condition of the exact comparison
    model = make_model(params, moments, accum, denom, dev, stepped)
    counts = densify.densify_and_prune(model, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N=N, noise=noise.to(dev))
    assert counts == ref.counts, (counts, ref.counts)
    check_against_statement(model, ref, params, N, stepped)
    return model, ref, params


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 5000])
def test_row_counts_around_the_block_edge(gpu_device, P):
    fates = set()
    for seed in ((0, 1, 4, 9) if P == 1 else (0,)):                                      # a single row: pruned, kept, cloned, split
        _m, ref, _p = run_case(gpu_device, P, "typical", seed)
        fates.add(ref.counts)
    if P == 1:
        assert fates == {(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1)}
    if P >= 1023:
        assert min(ref.counts) > 0


@pytest.mark.gpu
def test_offsets_carry_across_the_scan_step(gpu_device):
    """P = 1024 * 1024 + 1027 rows are 1026 row blocks: the one-workgroup scan takes 1024 block counts a step, so the last two blocks'
    offsets need the first step's total, in each of the three segments.  Straight through mrgs_densify_classify and mrgs_densify_emit with
    one COPY tensor of one float a row that holds the row index (exact in fp32 below 2^24), against the three masks of the statement."""
    from materialrefgs_amd import _lib
    dev, P, N = gpu_device, 1024 * 1024 + 1027, 2
    accum, denom, scaling, opacity = make_decision_inputs(P, "typical", torch.Generator().manual_seed(7))
    params = {"xyz": torch.zeros(P, 3), "scaling": scaling, "rotation": torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1), "opacity": opacity}
    ref = ds.densify_and_prune(params, None, accum, denom, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY, EXTENT, 20, torch.zeros(P, N, 2), N=N)
    assert ref.margin >= 1e-3, ref.margin                                                # the condition of the exact comparison
    keep, clone, child = (torch.zeros(P, dtype=torch.bool).index_fill_(0, ref.row[ref.kind == k], True) for k in (0, 1, 2))
    assert int(keep[-1027:].sum()) > 0 and int(clone[-1027:].sum()) > 0 and int(child[-1027:].sum()) > 0     # the second step has all three
    L = _lib.lib()
    accum, denom, scaling, opacity = (t.to(dev).contiguous() for t in (accum, denom, scaling, opacity))
    idx = torch.arange(P, dtype=torch.float32, device=dev)
    cfg = _lib.MrgsDensifyConfig(N, P, MAX_GRAD, MIN_OPACITY, PERCENT_DENSE * EXTENT, 0.1 * EXTENT, None, scaling.data_ptr(), None)
    with _lib.guard(dev):
        st = _lib.stream_ptr(dev)
        ws = torch.empty(L.mrgs_densify_ws_bytes(P), dtype=torch.uint8, device=dev)
        cnt = torch.empty(3, dtype=torch.int64, device=dev)
        assert L.mrgs_densify_classify(ctypes.byref(cfg), accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(), opacity.data_ptr(),
                                       ws.data_ptr(), ws.numel(), cnt.data_ptr(), st) == 0
        counts = cnt.tolist()
        assert counts == [int(keep.sum()), int(clone.sum()), int(child.sum())] and tuple(counts) == ref.counts
        dst = torch.full((counts[0] + counts[1] + N * counts[2],), -1.0, device=dev)
        arr = (_lib.MrgsDensifyTensor * 1)(_lib.MrgsDensifyTensor(idx.data_ptr(), dst.data_ptr(), 1, _lib.MRGS_DENSIFY_COPY))
        assert L.mrgs_densify_emit(ctypes.byref(cfg), ws.data_ptr(), (ctypes.c_int64 * 3)(*counts), arr, 1, 0, None, st) == 0
    want = torch.arange(P, dtype=torch.float32)
    assert torch.equal(dst.cpu(), torch.cat([want[keep], want[clone]] + [want[child]] * N))


@pytest.mark.gpu
def test_typical_mix_at_5000(gpu_device):
    _m, ref, params = run_case(gpu_device, 5000, "typical", 11)
    P = 5000
    assert 0.15 * P < int(ref.clone.sum()) < 0.25 * P and 0.07 * P < int(ref.split.sum()) < 0.14 * P
    assert ref.counts[1] < int(ref.clone.sum()) and ref.counts[2] < int(ref.split.sum())     # some of either are pruned with their source


@pytest.mark.gpu
def test_nothing_selected_nothing_pruned_is_the_identity(gpu_device):
    model, ref, params = run_case(gpu_device, 5000, "none", 12)
    assert ref.counts == (5000, 0, 0)
    for n, _ in GROUPS:
        assert torch.equal(getattr(model, ATTRS[n]).detach().cpu(), params[n])


@pytest.mark.gpu
def test_every_row_split(gpu_device):
    _m, ref, _p = run_case(gpu_device, 5000, "all_split", 13, max_screen_size=None)
    assert ref.counts == (0, 0, 5000)


@pytest.mark.gpu
def test_every_row_pruned_leaves_a_consistent_empty_model(gpu_device):
    model, ref, _p = run_case(gpu_device, 5000, "all_pruned", 14)
    assert ref.counts == (0, 0, 0) and model._xyz.shape == (0, 3) and model._indirect_asg.shape == (0, 32, 5)


@pytest.mark.gpu
def test_max_screen_size_none_against_twenty(gpu_device):
    _m, with_limit, _p = run_case(gpu_device, 5000, "typical", 15, max_screen_size=20)
    _m, without, _p = run_case(gpu_device, 5000, "typical", 15, max_screen_size=None)
    assert sum(without.counts) > sum(with_limit.counts)                                  # only the world-space term differs: radii of 50 prune nothing


@pytest.mark.gpu
def test_three_children(gpu_device):
    _m, ref, _p = run_case(gpu_device, 5000, "typical", 16, N=3)
    assert ref.counts[2] > 0 and ref.tensors["xyz"].shape[0] == ref.counts[0] + ref.counts[1] + 3 * ref.counts[2]


@pytest.mark.gpu
def test_before_the_optimizers_first_step(gpu_device):
    run_case(gpu_device, 1025, "typical", 17, stepped=False)


@pytest.mark.gpu
def test_empty_model(gpu_device):
    from materialrefgs_amd import densify
    params = {n: torch.zeros((0,) + sh) for n, sh in GROUPS}
    moments = {n: (v.clone(), v.clone()) for n, v in params.items()}
    accum, denom = torch.zeros(0, 1), torch.zeros(0, 1)
    model = make_model(params, moments, accum, denom, gpu_device)
    before = [gr["params"][0] for gr in model.optimizer.param_groups]
    assert densify.densify_and_prune(model, MAX_GRAD, MIN_OPACITY, EXTENT, 20) == (0, 0, 0)
    assert all(a is b["params"][0] for a, b in zip(before, model.optimizer.param_groups))
    assert model.xyz_gradient_accum.shape == (0, 1) and model.denom.shape == (0, 1) and model.max_radii2D.shape == (0,)


# ---- the generator -------------------------------------------------------------------------------------------------------------
def unit_model(P, dev):
    """xyz = 0, identity rotation, raw scaling 0 (s = 1 > t), g = 2 max_grad: every row is split and a child's centre IS (z0, z1, 0)."""
    params = {n: torch.zeros((P,) + sh) for n, sh in GROUPS}
    params["rotation"][:, 0] = 1.0
    params["opacity"] += 2.0
    return make_model(params, None, torch.full((P, 1), 2.0 * MAX_GRAD), torch.ones(P, 1), dev, stepped=False)


@pytest.mark.gpu
def test_generator_against_the_numpy_statement(gpu_device):
    from materialrefgs_amd import densify
    P, N = 5000, 2

    def draw(seed, P=P, N=N):
        model = unit_model(P, gpu_device)
        assert densify.densify_and_prune(model, MAX_GRAD, MIN_OPACITY, EXTENT, None, N=N, seed=seed) == (0, 0, P)
        return model._xyz.detach().cpu().reshape(N, P, 3)
    seed = 0x9E3779B97F4A7C15
    z = draw(seed)
    assert float(z[..., 2].abs().max()) == 0.0                                           # the third coordinate is exactly 0
    for k in range(N):
        n0, n1, want = ds.philox_normals(seed, np.arange(P), k)
        assert n0.min() >= 1 and n0.max() <= 1 << 24 and n1.min() >= 1 and n1.max() <= 1 << 24
        # angle in fp32: 2 pi 2^-24 = 3.7e-7 on cos, x radius <= 5.77 = 2.2e-6; the radius's <= 4 ulp: 2.8e-6; 1e-5 is the sum doubled
        err = np.abs(z[k, :, :2].double().numpy() - want).max()
        assert err <= 1e-5, err
    assert torch.equal(draw(seed), z)                                                    # same seed: identical bits
    other = draw(seed + 1)
    assert not bool((other[..., :2] == z[..., :2]).any())                                # another seed
    assert not bool((z[0, :, :2] == z[1, :, :2]).any())                                  # another child index
    assert not bool((z[0, 1:, :2] == z[0, :-1, :2]).any())                               # another row
    flat = z[..., :2].double().reshape(-1)
    n = flat.numel()
    assert n == 2 * P * N
    assert abs(float(flat.mean())) <= 5 / math.sqrt(n) and abs(float(flat.var()) - 1.0) <= 5 * math.sqrt(2 / n)
    # rows are keyed by themselves, not by the grid: the first 1000 rows of a smaller model draw the same values
    assert torch.equal(draw(seed, P=1000)[:, :, :2], z[:, :1000, :2])
    # seed=None: torch's CPU default generator governs the call
    torch.manual_seed(7)
    m1 = unit_model(64, gpu_device)
    densify.densify_and_prune(m1, MAX_GRAD, MIN_OPACITY, EXTENT, None)
    torch.manual_seed(7)
    m2 = unit_model(64, gpu_device)
    densify.densify_and_prune(m2, MAX_GRAD, MIN_OPACITY, EXTENT, None)
    m3 = unit_model(64, gpu_device)
    densify.densify_and_prune(m3, MAX_GRAD, MIN_OPACITY, EXTENT, None)
    assert torch.equal(m1._xyz, m2._xyz) and not torch.equal(m1._xyz, m3._xyz)


# ---- the statistics kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 1025, 5000])
@pytest.mark.parametrize("mask", ["half", "none", "all"])
def test_statistics_kernel(gpu_device, P, mask):
    from materialrefgs_amd import densify
    dev = gpu_device
    g = torch.Generator().manual_seed(P)
    accum, denom = torch.rand(P, 1, generator=g), torch.randint(0, 9, (P, 1), generator=g).float()
    max_r = torch.randint(0, 40, (P,), generator=g).float()
    grad = torch.randn(P, 3, generator=g) * 1e-3
    radii = torch.randint(0, 60, (P,), generator=g, dtype=torch.int32)
    vis = {"half": torch.rand(P, generator=g) < 0.5, "none": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool)}[mask]
    want_a, want_d, want_r = ds.add_densification_stats(accum, denom, max_r, grad, vis, radii)
    model = SimpleNamespace(xyz_gradient_accum=accum.to(dev), denom=denom.to(dev), max_radii2D=max_r.to(dev))
    leaf = torch.zeros(P, 3, device=dev, requires_grad=True)
    leaf.grad = grad.to(dev)
    addr = (model.xyz_gradient_accum.data_ptr(), model.denom.data_ptr(), model.max_radii2D.data_ptr())
    densify.add_densification_stats(model, leaf, vis.to(dev), radii.to(dev))
    assert addr == (model.xyz_gradient_accum.data_ptr(), model.denom.data_ptr(), model.max_radii2D.data_ptr())      # in place
    got_a, got_d, got_r = model.xyz_gradient_accum.cpu(), model.denom.cpu(), model.max_radii2D.cpu()
    assert torch.equal(got_d.double(), want_d) and torch.equal(got_r.double(), want_r)
    # six half-ulp roundings (three squares, two sums... the root, the add): 3.6e-7, factor three
    assert bool(((got_a.double() - want_a).abs() <= 1e-6 * want_a.abs()).all())
    assert torch.equal(got_a[~vis], accum[~vis]) and torch.equal(got_d[~vis], denom[~vis]) and torch.equal(got_r[~vis], max_r[~vis])
    # a uint8 filter and the tuple form give identical results; radii=None leaves max_radii2D alone
    a2, d2, r2 = accum.to(dev), denom.to(dev), max_r.to(dev)
    densify.add_densification_stats((a2, d2, r2), leaf, vis.to(torch.uint8).to(dev), radii.to(dev))
    assert torch.equal(a2.cpu(), got_a) and torch.equal(d2.cpu(), got_d) and torch.equal(r2.cpu(), got_r)
    a3, d3, r3 = accum.to(dev), denom.to(dev), max_r.to(dev)
    densify.add_densification_stats((a3, d3, r3), grad.to(dev), vis.to(dev))
    assert torch.equal(a3.cpu(), got_a) and torch.equal(d3.cpu(), got_d) and torch.equal(r3.cpu(), max_r)
