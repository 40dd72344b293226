"""optim.SparseAdam (mrgs_adam_step_rows, csrc/mrgs_optim.hip): rows whose visibility byte is 0 keep their bits, visible rows follow the
float64 statement of the rule (tests/sparse_adam_statement.py), an all-ones mask is the dense Adam bit for bit.

Shapes: row widths 1, 2, 3, 4, 5, 45 and 160 floats (most no multiple of a 16-byte piece; 3, 45 and 160 put a 4096-element chunk boundary
inside a row), an `env` group stepped densely, and one tensor viewed at a 4-byte offset into a larger buffer (the scalar path).
P = 1, 63, 65 (one wave of pieces and its neighbours), 1367 (1367 * 3 = 4101: the first chunk boundary falls inside a row) and 5000 (several
chunks in every tensor, 196 in the widest)."""
import copy
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sparse_adam_statement as sas  # noqa: E402
from materialrefgs_amd.optim import Adam, SparseAdam  # noqa: E402

ROW_SHAPES = {"w1": (1,), "w2": (2,), "w3": (3,), "w4": (4,), "w5": (5,), "w45": (15, 3), "w160": (32, 5), "off": (3,)}
ENV_SHAPE = (6, 16, 16, 3)
LRS = {"w1": 0.05, "w2": 5e-3, "w3": 1.6e-4, "w4": 1e-3, "w5": 1e-2, "w45": 1.25e-4, "w160": 2.5e-3, "off": 1e-3, "env": 0.01}
SIZES = (1, 63, 65, 1367, 5000)
KINDS = ("zeros", "row0", "last", "alternating", "runs", "random", "pair")
STEPS = 6


# ---- CPU: the rule, the argument checks ---------------------------------------------------------------------------------------------------
def test_statement_with_every_row_visible_is_torch_adam():
    """The visible branch of the rule is Adam's: float64 torch.optim.Adam(eps=1e-15) over 5 steps, to 1e-12."""
    g = torch.Generator().manual_seed(0)
    start = torch.randn(37, 5, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(start.clone())
    opt = torch.optim.Adam([p], lr=3e-3, eps=1e-15)
    st = sas.Tensor(start.numpy())
    for it in range(5):
        gr = torch.randn(37, 5, generator=g, dtype=torch.float64) * 10.0 ** (it - 2)
        p.grad = gr.clone()
        opt.step()
        sas.step(st, gr.numpy(), 3e-3, vis=np.ones(37, dtype=bool))
    assert np.abs(st.p - p.data.numpy()).max() < 1e-12
    assert np.abs(st.m - opt.state[p]["exp_avg"].numpy()).max() < 1e-12
    assert np.abs(st.v - opt.state[p]["exp_avg_sq"].numpy()).max() < 1e-12
    # and an invisible row is left alone while the count advances
    before = st.p.copy()
    sas.step(st, np.ones((37, 5)), 3e-3, vis=np.arange(37) != 5)
    assert st.t == 6 and np.array_equal(st.p[5], before[5]) and not np.array_equal(st.p[4], before[4])


def _cpu_optimizer(shapes):
    ps = {k: torch.nn.Parameter(torch.zeros(*s)) for k, s in shapes.items()}
    opt = SparseAdam([{"params": [p], "lr": 1e-3, "name": k} for k, p in ps.items()], lr=0.0, eps=1e-15)
    for p in ps.values():
        p.grad = torch.ones_like(p)
    return ps, opt


def test_argument_errors():
    ps, opt = _cpu_optimizer({"xyz": (8, 3), "env": (6, 4, 4, 3)})
    ok = torch.ones(8, dtype=torch.bool)
    with pytest.raises(ValueError, match="xyz"):                         # wrong mask length: the per-gaussian group does not fit it
        opt.step(visibility=torch.ones(9, dtype=torch.bool))
    with pytest.raises(TypeError):                                       # a float mask
        opt.step(visibility=torch.ones(8))
    with pytest.raises(ValueError):                                      # a sequence of masks of two lengths
        opt.step(visibility=[ok, torch.ones(9, dtype=torch.bool)])
    with pytest.raises(ValueError):
        opt.step(visibility=torch.ones(8, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="device tensors only"):       # CPU parameters: as Adam, with and without a mask
        opt.step(visibility=ok)
    with pytest.raises(RuntimeError, match="device tensors only"):
        opt.step()
    assert len(opt.state) == 0                                           # nothing refused has advanced a step count
    ps, opt = _cpu_optimizer({"xyz": (8, 3), "sky": (6, 4, 4, 3)})       # a group that is not per-gaussian and not named dense
    with pytest.raises(ValueError, match="sky"):
        opt.step(visibility=ok)
    assert SparseAdam([torch.nn.Parameter(torch.zeros(2))], dense_groups=("sky",)).dense_groups == ("sky",)
    with pytest.raises(NotImplementedError):
        SparseAdam([torch.nn.Parameter(torch.zeros(2))], amsgrad=True)


def test_training_setup_selects_the_class_by_optimizer_type():
    from materialrefgs_amd import checkpoint

    def model():
        z = lambda *s: torch.nn.Parameter(torch.zeros(4, *s))
        return SimpleNamespace(_xyz=z(3), _features_dc=z(1, 3), _features_rest=z(15, 3), _opacity=z(1), _scaling=z(2), _rotation=z(4),
                               _refl_strength=z(1), _ori_color=z(3), _diffuse_color=z(3), _roughness=z(1), _metalness=z(1), _normal1=z(3),
                               _normal2=z(3), _indirect_dc=z(1, 3), _indirect_rest=z(15, 3), _indirect_asg=z(32, 5), spatial_lr_scale=1.0)
    args = checkpoint.default_training_args()
    assert not hasattr(args, "optimizer_type")
    assert type(checkpoint.training_setup(model(), args)) is Adam        # attribute absent: nothing changes
    args.optimizer_type = "default"
    assert type(checkpoint.training_setup(model(), args)) is Adam
    args.optimizer_type = "sparse_adam"
    opt = checkpoint.training_setup(model(), args)
    assert type(opt) is SparseAdam and opt.bias_correction and opt.dense_groups == ("mlp", "env", "env2")
    assert type(checkpoint.training_setup(model(), args, optimizer_cls=Adam)) is Adam      # an explicit class wins


def test_c_entry_refuses_bad_arguments_without_gpu():
    """Contract violations of mrgs_adam_step_rows are status codes before any HIP call (no device needed; no pointer is dereferenced)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    BAD_ARG, UNSUPPORTED = _lib.MRGS_E_BAD_ARG, 6
    p = 0x10000
    T = _lib.MrgsAdamRowsTensor
    assert ctypes.sizeof(T) == 4 * 8 + 8 + 4 * 4

    def call(tensors, n_rows=10, masks=(p,), n_masks=None, bias=1):
        arr = (T * max(1, len(tensors)))(*tensors)
        mp = (ctypes.c_void_p * max(1, len(masks)))(*masks)
        return L.mrgs_adam_step_rows(arr, len(tensors), n_rows, mp, len(masks) if n_masks is None else n_masks, bias, 0.9, 0.999, 1e-15, None)
    good = T(p, p, p, p, 30, 3, 1e-3, 1, 0)
    assert call([T(p, p, p, p, 31, 3, 1e-3, 1, 0)]) == BAD_ARG                       # numel != n_rows * row_floats
    assert call([good, T(p, p, p, p, 40, 3, 1e-3, 1, 0)]) == BAD_ARG                 # ... in any entry of the list
    assert call([good], masks=(None,)) == BAD_ARG                                    # a null mask
    assert call([good], masks=(p, None)) == BAD_ARG
    assert call([good], masks=(p,) * 5) == BAD_ARG                                   # five masks
    assert call([good], n_masks=0) == BAD_ARG
    assert call([T(None, p, p, p, 30, 3, 1e-3, 1, 0)]) == BAD_ARG                    # a null tensor pointer
    assert call([T(p, p, p, p, -30, -3, 1e-3, 1, 0)]) == BAD_ARG                     # negative sizes
    assert call([good], n_rows=-1) == BAD_ARG
    assert call([T(p, p, p, p, 30, 3, 1e-3, 0, 0)]) == BAD_ARG                       # the step count is 1-based
    assert call([T(p, p, p, p, 10 * 40000, 40000, 1e-3, 1, 0)]) == UNSUPPORTED       # a row wider than MRGS_ADAM_ROWS_MAX_WIDTH
    assert L.mrgs_adam_step_rows(None, 1, 10, (ctypes.c_void_p * 1)(p), 1, 1, 0.9, 0.999, 1e-15, None) == BAD_ARG
    assert L.mrgs_adam_step_rows((T * 1)(good), 1, 10, None, 1, 1, 0.9, 0.999, 1e-15, None) == BAD_ARG
    assert call([T(None, None, None, None, 0, 3, 1e-3, 1, 0)], n_rows=0) == 0        # an empty model: nothing to launch


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _values(P, seed=0, names=tuple(ROW_SHAPES) + ("env",)):
    g = torch.Generator().manual_seed(1000 * seed + P)
    return {k: torch.randn(*(ENV_SHAPE if k == "env" else (P,) + ROW_SHAPES[k]), generator=g) for k in names}


def _make(opt_cls, values, dev, lrs=LRS, **kw):
    ps = {}
    for k, v in values.items():
        if k == "off":                                          # contiguous, but 4 bytes into its buffer: no 16-byte alignment
            buf = torch.zeros(v.numel() + 8, device=dev)
            view = buf[1:1 + v.numel()].view(v.shape)
            view.copy_(v)
            assert view.data_ptr() % 16 == 4
            ps[k] = torch.nn.Parameter(view)
        else:
            ps[k] = torch.nn.Parameter(v.clone().to(dev))
    return ps, opt_cls([{"params": [ps[k]], "lr": lrs[k], "name": k} for k in ps], lr=0.0, eps=1e-15, **kw)


def _preload(opt, ps, seed):
    """Non-zero moments in every row before the first step (the state `load_state_dict` would leave), so that a kept row shows bits that
    a stray write would change; returns them as numpy."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, p in ps.items():
        m, v = torch.randn(*p.shape, generator=g) * 0.01, torch.rand(*p.shape, generator=g) * 1e-4
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": m.to(p.device), "exp_avg_sq": v.to(p.device)}
        out[k] = (m.numpy().copy(), v.numpy().copy())
    return out


def _masks(kind, P, it):
    """The masks of step `it` as a list of numpy arrays (bool; uint8 with the values 0 and 2 for "runs": any non-zero byte is visible)."""
    r = np.arange(P)
    if kind == "zeros":
        return [np.zeros(P, dtype=bool)]
    if kind == "ones":
        return [np.ones(P, dtype=bool)]
    if kind == "row0":
        return [r == 0]
    if kind == "last":
        return [r == P - 1]
    if kind == "alternating":
        return [r % 2 == 0]
    if kind == "runs":
        return [((r % 128) < 37).astype(np.uint8) * 2]
    rng = np.random.default_rng(7919 * P + it)
    if kind == "random":
        return [rng.random(P) < 0.53]
    if kind == "pair":
        return [rng.random(P) < 0.3, rng.random(P) < 0.3]
    raise KeyError(kind)


def _grads(ps, g, it, skip=()):
    scale = 10.0 ** ((it % 4) - 3)
    return {k: None if k in skip else torch.randn(*p.shape, generator=g) * scale for k, p in ps.items()}


@functools.lru_cache(maxsize=None)
def _run(P, kind, bias_correction):
    """STEPS masked steps of SparseAdam on the full parameter set beside the statement; everything the tests look at, on the host."""
    dev = torch.device("cuda")
    values = _values(P)
    ps, opt = _make(SparseAdam, values, dev, bias_correction=bias_correction)
    moments = _preload(opt, ps, P)
    st = {k: sas.Tensor(values[k].numpy()).load(*moments[k], 0) for k in ps}
    g = torch.Generator().manual_seed(P + 5)
    ever = np.zeros(P, dtype=bool)
    for it in range(STEPS):
        masks = _masks(kind, P, it)
        vis = np.logical_or.reduce([m != 0 for m in masks])
        ever |= vis
        grads = _grads(ps, g, it)
        for k, p in ps.items():
            p.grad = grads[k].to(dev)
            sas.step(st[k], grads[k].numpy(), LRS[k], vis=None if k == "env" else vis, bias_correction=bias_correction)
        dm = [torch.from_numpy(m).to(dev) for m in masks]
        opt.step(visibility=dm[0] if len(dm) == 1 else dm)
    torch.cuda.synchronize()
    got = {k: (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy(), int(opt.state[p]["step"]))
           for k, p in ps.items()}
    start = {k: (values[k].numpy(),) + moments[k] for k in ps}
    return SimpleNamespace(got=got, start=start, statement=st, never=~ever)


CASES = [(P, kind, True) for P in SIZES for kind in KINDS] + [(P, kind, False) for P in SIZES for kind in ("random", "pair")]


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind,bias_correction", CASES)
def test_invisible_rows_keep_their_bits(P, kind, bias_correction):
    """A row whose mask byte was 0 in all six steps has the param, exp_avg and exp_avg_sq it started with, bit for bit, in every tensor."""
    r = _run(P, kind, bias_correction)
    if kind in ("zeros", "alternating", "runs") and P > 1 or kind == "zeros":
        assert r.never.any()
    for k in ROW_SHAPES:
        for got, start, what in zip(r.got[k][:3], r.start[k], ("param", "exp_avg", "exp_avg_sq")):
            assert np.array_equal(got[r.never].view(np.uint32), start[r.never].view(np.uint32)), (k, what)


def _close(got, want, rtol, atol, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = err > atol + rtol * np.abs(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} off, worst {err.max():.3e} (atol {atol:.3e}, rtol {rtol:.1e})"


def _matches_statement(got, st, lr, steps, name):
    """tests/test_optim.py's tolerances: moments rtol 2e-6 with atol 5e-7 max, parameters rtol 1e-5 with atol 2e-6 lr steps."""
    p, m, v, t = got
    assert t == st.t, name
    _close(m, st.m, 2e-6, 5e-7 * np.abs(st.m).max(), f"{name} exp_avg")
    _close(v, st.v, 2e-6, 5e-7 * np.abs(st.v).max(), f"{name} exp_avg_sq")
    _close(p, st.p, 1e-5, 2e-6 * lr * steps, f"{name} param")


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind,bias_correction", CASES)
def test_visible_rows_follow_the_rule(P, kind, bias_correction):
    r = _run(P, kind, bias_correction)
    for k in r.got:
        assert r.got[k][3] == STEPS, k                                   # one count per parameter, also where no row was ever visible
        _matches_statement(r.got[k], r.statement[k], LRS[k], STEPS, k)


@pytest.mark.gpu
def test_a_row_that_leaves_the_view_is_frozen_while_dense_adam_drifts():
    """Rows 100 .. 399 are visible in step 1 and invisible in steps 2 .. 6: bit-frozen from step 2 on under SparseAdam; dense Adam on a
    copy keeps moving them by their decaying momentum although their gradient is zero -- the behaviour the feature exists for."""
    dev = torch.device("cuda")
    P = 1367
    values = _values(P, 1)
    pa, oa = _make(SparseAdam, values, dev)
    pb, ob = _make(Adam, values, dev)
    g = torch.Generator().manual_seed(11)
    gone = (np.arange(P) >= 100) & (np.arange(P) < 400)
    gone_t = torch.from_numpy(gone).to(dev)
    snap = None
    for it in range(STEPS):
        vis = torch.ones(P, dtype=torch.bool, device=dev) if it == 0 else ~gone_t
        for k, gr in _grads(pa, g, it).items():
            gr = gr.to(dev)
            if k != "env":
                gr[~vis] = 0.0                                           # what the backward of a view leaves in rows it did not touch
            pa[k].grad, pb[k].grad = gr.clone(), gr.clone()
        oa.step(visibility=vis)
        ob.step()
        if it == 0:
            snap = {k: [t.clone() for t in (pa[k].data, oa.state[pa[k]]["exp_avg"], oa.state[pa[k]]["exp_avg_sq"])] for k in ROW_SHAPES}
            for k in ROW_SHAPES:
                assert torch.equal(pa[k].data, pb[k].data), k           # step 1 saw every row: the two agree
    for k in ROW_SHAPES:
        now = (pa[k].data, oa.state[pa[k]]["exp_avg"], oa.state[pa[k]]["exp_avg_sq"])
        for a, b in zip(now, snap[k]):
            assert torch.equal(a[gone_t], b[gone_t]), k
        assert not torch.equal(pa[k].data[~gone_t], snap[k][0][~gone_t]), k
        moved = (pb[k].data[gone_t] != snap[k][0][gone_t]).float().mean()
        assert float(moved) > 0.9, (k, float(moved))                     # dense Adam has moved them


@pytest.mark.gpu
@pytest.mark.parametrize("P", SIZES)
def test_all_ones_mask_and_no_mask_equal_dense_adam_bit_for_bit(P):
    """Six steps with the learning-rate edit and the `grad = None` step of test_adam_matches_torch_adam_over_steps: SparseAdam under an
    all-ones mask and SparseAdam without a mask equal Adam in every bit of every tensor; under a 53 % mask its `env` group (stepped
    densely) still does."""
    dev = torch.device("cuda")
    values = _values(P, 2)
    runs = [_make(Adam, values, dev), _make(SparseAdam, values, dev), _make(SparseAdam, values, dev), _make(SparseAdam, values, dev)]
    ones = torch.ones(P, dtype=torch.bool, device=dev)
    g = torch.Generator().manual_seed(P)
    for it in range(STEPS):
        grads = _grads(runs[0][0], g, it, skip=("w5",) if it % 3 == 1 else ())
        for ps, opt in runs:
            for k in ps:
                ps[k].grad = None if grads[k] is None else grads[k].to(dev)
            if it == 3:
                for grp in opt.param_groups:
                    if grp["name"] == "w3":
                        grp["lr"] = 3.3e-5
        runs[0][1].step()
        runs[1][1].step(visibility=ones)
        runs[2][1].step()
        runs[3][1].step(visibility=torch.from_numpy(_masks("random", P, it)[0]).to(dev))
    (pa, oa), (pb, ob), (pc, oc), (pd, od) = runs
    for k in pa:
        for ps, opt, what in ((pb, ob, "all-ones mask"), (pc, oc, "visibility=None")) + (((pd, od, "env under a mask"),) if k == "env" else ()):
            sa, sb = oa.state[pa[k]], opt.state[ps[k]]
            assert int(sa["step"]) == int(sb["step"]) == (4 if k == "w5" else STEPS), (k, what)
            assert torch.equal(pa[k].data, ps[k].data), (k, what)
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (k, what)


def _state_of(opt, ps):
    return {k: (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy(), int(opt.state[p]["step"]))
            for k, p in ps.items()}


@pytest.mark.gpu
def test_state_interchange_with_adam_and_compaction():
    """Adam -> SparseAdam and SparseAdam -> Adam through load_state_dict, then densify.prune_optimizer on the SparseAdam and a masked step
    with a mask of the new length: all against the statement."""
    from materialrefgs_amd import densify
    dev = torch.device("cuda")
    P = 1367
    values = _values(P, 3)
    g = torch.Generator().manual_seed(21)
    st = {k: sas.Tensor(values[k].numpy()) for k in values}
    pa, oa = _make(Adam, values, dev)
    for it in range(3):                                                  # three dense steps with Adam
        for k, gr in _grads(pa, g, it).items():
            pa[k].grad = gr.to(dev)
            sas.step(st[k], gr.numpy(), LRS[k])
        oa.step()
    pb, ob = _make(SparseAdam, {k: v.detach().cpu() for k, v in pa.items()}, dev)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    vis = _masks("random", P, 0)[0]
    for k, gr in _grads(pb, g, 3).items():                               # one masked step with SparseAdam
        pb[k].grad = gr.to(dev)
        sas.step(st[k], gr.numpy(), LRS[k], vis=None if k == "env" else vis)
    ob.step(visibility=torch.from_numpy(vis).to(dev))
    for k, got in _state_of(ob, pb).items():
        _matches_statement(got, st[k], LRS[k], 4, f"Adam -> SparseAdam, {k}")
    pc, oc = _make(Adam, {k: v.detach().cpu() for k, v in pb.items()}, dev)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    for k, gr in _grads(pc, g, 4).items():                               # and one dense step with Adam again
        pc[k].grad = gr.to(dev)
        sas.step(st[k], gr.numpy(), LRS[k])
    oc.step()
    for k, got in _state_of(oc, pc).items():
        _matches_statement(got, st[k], LRS[k], 5, f"SparseAdam -> Adam, {k}")
    # compaction of the SparseAdam's state, as test_prune_matches_boolean_indexing does it, then a masked step at the new length
    keep = np.random.default_rng(5).random(P) < 0.7
    kept, _ = densify.prune_optimizer(ob, torch.from_numpy(keep).to(dev))
    assert "env" not in kept and set(kept) == set(ROW_SHAPES)
    n = int(keep.sum())
    st2 = {}
    for k in pb:
        full = _state_of(ob, {k: kept[k] if k in kept else pb[k]})[k]
        st2[k] = sas.Tensor(full[0]).load(full[1], full[2], full[3])
        assert full[0].shape[0] == (n if k != "env" else ENV_SHAPE[0]) and full[3] == 4
    vis2 = _masks("random", n, 1)[0]
    now = dict(kept, env=pb["env"])
    for k, p in now.items():
        gr = torch.randn(*p.shape, generator=g) * 0.01
        p.grad = gr.to(dev)
        sas.step(st2[k], gr.numpy(), LRS[k], vis=None if k == "env" else vis2)
    ob.step(visibility=torch.from_numpy(vis2).to(dev))
    for k, got in _state_of(ob, now).items():
        _matches_statement(got, st2[k], LRS[k], 1, f"after compaction, {k}")
    with pytest.raises(ValueError, match="w1"):                          # the mask of the old length no longer fits
        ob.step(visibility=torch.from_numpy(vis).to(dev))


@pytest.mark.gpu
def test_more_tensors_than_a_launch_table_and_more_masks_than_the_entry_takes():
    """70 masked tensors and 3 dense ones in one call (three launches of 32, 32 and 6 table entries; the second list starts inside one),
    under six masks (the entry point takes four: the rest is ORed first)."""
    dev = torch.device("cuda")
    P = 65
    widths = [(1,), (2,), (3,), (5,), (15, 3), (32, 5), (4,)]
    g = torch.Generator().manual_seed(9)
    names = [f"t{i}" for i in range(70)] + ["mlp", "env", "env2"]
    shapes = {n: ((P,) + widths[i % 7]) if i < 70 else (7, 3 + i) for i, n in enumerate(names)}
    lrs = {n: 1e-3 * (1 + i % 5) for i, n in enumerate(names)}
    values = {n: torch.randn(*shapes[n], generator=g) for n in names}
    ps, opt = _make(SparseAdam, values, dev, lrs=lrs)
    st = {n: sas.Tensor(values[n].numpy()) for n in names}
    ever = np.zeros(P, dtype=bool)
    for it in range(2):
        rng = np.random.default_rng(it)
        masks = [rng.random(P) < 0.12 for _ in range(6)]
        vis = np.logical_or.reduce(masks)
        ever |= vis
        assert 0 < vis.sum() < P and (vis != np.logical_or.reduce(masks[:4])).any()
        for n in names:
            gr = torch.randn(*shapes[n], generator=g) * 0.1
            ps[n].grad = gr.to(dev)
            sas.step(st[n], gr.numpy(), lrs[n], vis=None if n in ("mlp", "env", "env2") else vis)
        opt.step(visibility=[torch.from_numpy(m).to(dev) for m in masks])
    for n, got in _state_of(opt, ps).items():
        _matches_statement(got, st[n], lrs[n], 2, n)
        if n.startswith("t"):
            assert (~ever).any() and np.array_equal(got[0][~ever], values[n].numpy()[~ever]) and not got[1][~ever].any()
    # an empty model: nothing to launch, the count still advances
    p0 = torch.nn.Parameter(torch.zeros(0, 3, device=dev))
    o0 = SparseAdam([{"params": [p0], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)
    p0.grad = torch.zeros(0, 3, device=dev)
    o0.step(visibility=torch.zeros(0, dtype=torch.bool, device=dev))
    assert int(o0.state[p0]["step"]) == 1
