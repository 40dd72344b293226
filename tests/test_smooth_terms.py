"""The Sobel smoothness terms (csrc/mrgs_smooth.hip: smooth_terms_fwd / _finalize / _bwd, behind materialrefgs_amd.smoothness.view_smooth_terms,
smooth_loss, first_order_edge_aware_loss and albedo_smooth_loss, and behind the same names of materialrefgs_amd.losses for fp32 device
tensors) against the float64 statement of tests/smooth_statement.py.

kornia is not installed here and the reference's own two functions need it, so they cannot be run to make a fixture: the statement is
`losses.spatial_gradient` applied in float64 exactly as the two reference lines write it, with the mask multiplied in first, and it rests on
the ramp pins of kornia's documented Sobel in tests/test_losses.py, as materialrefgs_amd/losses.py already does.

CPU: the C ABI's argument checks; the input conditions on every size; the wrappers' errors; the torch route of `losses.*` for other inputs.
GPU (-m gpu): the native node against the statement at the SIZES below, every item kind alone and four together with distinct upstream
gradients; repeatability; partial upstream gradients; no host read; albedo_smooth_loss; calculate_loss with both smoothness lambdas.
Bars (those of the sibling loss terms, test_prior_terms.py and test_multiview_ncc.py): every term within 1e-5 relative of the statement, or
exactly 0 where the statement is 0; every texel of every gradient map within 1e-4 of the largest element of that map, none excluded (the
inputs are built so that no sign decision can differ: tests/smooth_statement.py); the gradient exactly 0 at the texels at least two pixels
inside the flat rectangle.
"""
import ctypes
import functools
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import smooth_statement as ss  # noqa: E402


def _constant(name):
    src = open(os.path.join(ROOT, "materialrefgs_amd", "csrc", "mrgs_smooth.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


T = _constant("SMOOTH_TILE")
MAX_BLOCKS = _constant("SMOOTH_MAX_BLOCKS")
FINALIZE_THREADS = 256        # smooth_terms_finalize: one row of partial sums per thread and pass
# 1 x 1 .. 3 x 3: every border fold, and a texel that is first and last at once (a dimension of 1 or 2).  T + 1: one pixel more than a tile
# in each direction.  37 x 53: odd, the last tile partial both ways.  The last size: the forward leaves one row per workgroup and a workgroup
# per tile while there are no more than SMOOTH_MAX_BLOCKS tiles, so the finalize step makes a second pass from FINALIZE_THREADS + 1 = 257
# tiles on; 257 is prime, so the image with exactly that many tiles is one tile high, and the smallest one is 1 x (256 T + 1) = 1 x 8193.
SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (T + 1, T + 1), (37, 53), (1, FINALIZE_THREADS * T + 1))
assert FINALIZE_THREADS + 1 <= MAX_BLOCKS
# the item kinds: name -> (map, masked, edge-aware)
KINDS = {"plain1": ("single", False, False), "plain1_mask": ("single", True, False), "plain3": ("albedo", False, False),
         "plain3_mask": ("albedo", True, False), "edge3": ("normal", False, True), "edge1": ("depth", False, True)}
TOGETHER = ("plain3_mask", "plain1", "edge3", "edge1")        # four in one call ...
UP = (0.7, 1.3, 0.9, 1.1)                                     # ... with these upstream gradients


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    return ss.inputs(H, W)


@functools.lru_cache(maxsize=None)
def _reference(H, W):
    """The float64 statement on the inputs, once per size: kind -> (term, the gradient map of the term alone)."""
    inp = _inputs(H, W)
    out = {}
    for kind, (name, masked, edge) in KINDS.items():
        x = inp[name].double().requires_grad_(True)
        t = ss.first_order_edge_aware_loss(x, inp["img"].double()) if edge else ss.smooth_loss(x, inp["mask"] if masked else None)
        t.backward()
        out[kind] = (float(t.detach()), x.grad)
    return out


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES + ((131, 257),))
def test_inputs_meet_the_conditions(H, W):
    zeros, negative = ss.check_conditions(_inputs(H, W))
    print(H, W, f"exact zeros {zeros:.3f}, negative among the rest {negative:.3f}")
    if ss.flat_rect(H, W) is not None:
        assert zeros >= 0.03 and 0.4 <= negative <= 0.6


def _cfg(H=37, W=53):
    from materialrefgs_amd import _lib
    return _lib.MrgsSmoothConfig(H, W, 0)


def test_smooth_abi_argument_checks_without_gpu():
    """The three entry points exist, ws_bytes is 0 for sizes the calls refuse and bounded for huge ones, and every contract violation is
    MRGS_E_BAD_ARG (1) before anything is launched (no pointer below is ever dereferenced)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    row = 4 * _lib.MRGS_SMOOTH_MAX_ITEMS
    assert L.mrgs_smooth_ws_bytes(37, 53) == 4 * row and L.mrgs_smooth_ws_bytes(T + 1, T + 1) == 4 * row and L.mrgs_smooth_ws_bytes(1, 1) == row
    assert L.mrgs_smooth_ws_bytes(*SIZES[-1]) == (FINALIZE_THREADS + 1) * row
    assert L.mrgs_smooth_ws_bytes(4000, 4000) == MAX_BLOCKS * row == L.mrgs_smooth_ws_bytes(2 ** 31 - 1, 2 ** 31 - 1)      # the grid is bounded
    for bad in ((0, 53), (37, 0), (-1, 53), (37, -5)):
        assert L.mrgs_smooth_ws_bytes(*bad) == 0, bad
    hdr = open(os.path.join(ROOT, "include", "mrgs.h")).read()
    for sym in ("mrgs_smooth_ws_bytes", "mrgs_smooth_terms_forward", "mrgs_smooth_terms_backward"):
        assert sym in hdr and hasattr(L, sym)
    assert "#define MRGS_SMOOTH_MAX_ITEMS 4" in hdr and _lib.MRGS_SMOOTH_MAX_ITEMS == 4
    assert ctypes.sizeof(_lib.MrgsSmoothConfig) == 16 and ctypes.sizeof(_lib.MrgsSmoothItem) == 32
    assert L.mrgs_abi_version() == 10                                                   # entry points only: the revision stays
    p, big = 0x1000, 1 << 20
    Item = _lib.MrgsSmoothItem

    def items(*its):
        return (Item * max(len(its), 1))(*its)

    good = (Item(p, p, p, 3, 0), Item(p, None, p, 1, 1))
    table = (ctypes.c_void_p * 4)(p, p, p, p)

    def fwd(cfg=None, img=p, its=good, n=None, ws=p, ws_bytes=big, out=p):
        return L.mrgs_smooth_terms_forward(ctypes.byref(cfg or _cfg()), img, items(*its), len(its) if n is None else n, ws, ws_bytes, out, None)

    def bwd(cfg=None, img=p, its=good, n=None, table=table):
        return L.mrgs_smooth_terms_backward(ctypes.byref(cfg or _cfg()), img, items(*its), len(its) if n is None else n, table, None)

    bad = _cfg()
    bad.struct_size -= 4
    assert fwd(bad) == 1 and bwd(bad) == 1
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(flags=1)):
        c = _cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        assert fwd(c) == 1 and bwd(c) == 1, kw
    assert L.mrgs_smooth_terms_forward(None, p, items(*good), 2, p, big, p, None) == 1
    assert L.mrgs_smooth_terms_forward(ctypes.byref(_cfg()), p, None, 2, p, big, p, None) == 1
    for n in (0, -1, 5):                                                                # n_items outside 1..4
        assert fwd(its=(good[0],) * 5, n=n) == 1 and bwd(its=(good[0],) * 5, n=n) == 1, n
    assert fwd(its=(Item(None, p, p, 3, 0),)) == 1 and bwd(its=(Item(None, p, p, 3, 0),)) == 1             # an item without data
    for C in (0, 5, -1):                                                                # a plain item: C in 1..4
        assert fwd(its=(Item(p, None, p, C, 0),)) == 1 and bwd(its=(Item(p, None, p, C, 0),)) == 1, C
    for C in (0, 2, 4):                                                                 # an edge-aware one: C in {1, 3}
        assert fwd(its=(Item(p, None, p, C, 1),)) == 1 and bwd(its=(Item(p, None, p, C, 1),)) == 1, C
    assert fwd(its=(Item(p, None, p, 3, 2),)) == 1                                      # edge_aware is 0 or 1
    assert fwd(img=None) == 1 and bwd(img=None) == 1                                    # an edge-aware item without img
    assert fwd(ws=None) == 1 and fwd(out=None) == 1 and fwd(ws=p + 4) == 1
    assert fwd(ws_bytes=4 * row - 1) == 1                                               # a workspace that is too small
    assert bwd(table=None) == 1
    assert bwd(its=(good[0], Item(p, None, None, 1, 1))) == 1                           # an upstream gradient for an item without g_data
    none = (ctypes.c_void_p * 4)()
    assert bwd(its=(Item(p, p, None, 3, 0), Item(p, None, None, 1, 1)), table=none) == 0     # nothing to write: nothing launched


def test_wrappers_raise_without_gpu():
    """A CPU tensor, another dtype, a shape the kernels do not serve or an image that requires grad raises before anything native is
    touched."""
    from materialrefgs_amd import smoothness as sm
    H, W = 6, 10
    n3, n1, img = torch.rand(3, H, W), torch.rand(1, H, W), torch.rand(3, H, W)
    score = torch.rand(1, H, W) > 0.5
    with pytest.raises(RuntimeError, match="device tensor"):
        sm.smooth_loss(n3)
    with pytest.raises(RuntimeError, match="device tensor"):
        sm.first_order_edge_aware_loss(n1, img)
    with pytest.raises(RuntimeError, match="device tensor"):
        sm.albedo_smooth_loss(n3, score)
    with pytest.raises(RuntimeError, match="device tensor"):
        sm.view_smooth_terms(img, [(n3, None, True), (n1, None, True)])
    with pytest.raises(TypeError, match="float32"):
        sm.smooth_loss(n3.double())
    with pytest.raises(TypeError, match="float32"):
        sm.first_order_edge_aware_loss(n3, img.half())
    with pytest.raises(TypeError, match="tensor"):
        sm.smooth_loss(n3.numpy())
    with pytest.raises(ValueError, match="shape"):
        sm.smooth_loss(torch.rand(5, H, W))
    with pytest.raises(ValueError, match="shape"):
        sm.first_order_edge_aware_loss(torch.rand(2, H, W), img)
    with pytest.raises(ValueError, match="shape"):
        sm.first_order_edge_aware_loss(n3, torch.rand(3, H, W + 1))
    with pytest.raises(ValueError, match="shape"):
        sm.first_order_edge_aware_loss(n3, torch.rand(1, H, W))
    with pytest.raises(ValueError, match="shape"):
        sm.view_smooth_terms(img, [(n3, None, True), (torch.rand(1, H + 1, W), None, True)])
    with pytest.raises(ValueError, match="needs img"):
        sm.view_smooth_terms(None, [(n3, None, True)])
    with pytest.raises(ValueError, match="items"):
        sm.view_smooth_terms(img, [])
    with pytest.raises(ValueError, match="items"):
        sm.view_smooth_terms(img, [(n3, None, False)] * 5)
    with pytest.raises(ValueError, match="requires grad"):
        sm.first_order_edge_aware_loss(n3, img.clone().requires_grad_(True))


def test_losses_keep_the_torch_statement_for_other_inputs():
    """float64 CPU tensors (what tests/test_losses.py passes) and fp32 CPU tensors stay on the torch statement, gradients included."""
    from materialrefgs_amd import losses
    inp = _inputs(37, 53)
    ref = _reference(37, 53)
    for dtype, tol, gtol in ((torch.float64, 1e-14, 1e-12), (torch.float32, 1e-5, 1e-5)):
        x = inp["albedo"].to(dtype).requires_grad_(True)
        t = losses.smooth_loss(x)
        assert t.dtype is dtype and abs(float(t.detach()) - ref["plain3"][0]) <= tol * ref["plain3"][0]
        t.backward()
        assert float((x.grad.double() - ref["plain3"][1]).abs().max()) <= gtol * float(ref["plain3"][1].abs().max())
        for kind in ("edge3", "edge1"):
            d = inp[KINDS[kind][0]].to(dtype)
            t = losses.first_order_edge_aware_loss(d, inp["img"].to(dtype))
            assert t.dtype is dtype and abs(float(t) - ref[kind][0]) <= tol * ref[kind][0], kind


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _items(inp, dev, kinds):
    """(leaves, SmoothItems) of `kinds` on `dev`."""
    from materialrefgs_amd.smoothness import SmoothItem
    mask = inp["mask"].to(dev)
    leaves = [inp[KINDS[k][0]].to(dev).clone().requires_grad_(True) for k in kinds]
    return leaves, [SmoothItem(x, mask if KINDS[k][1] else None, KINDS[k][2]) for x, k in zip(leaves, kinds)]


def _check_term(mine, ref, what):
    assert mine.dim() == 0 and mine.is_cuda and mine.dtype is torch.float32
    v = float(mine.detach())
    if ref == 0:
        assert v == 0, (what, v)
        return 0.0
    fig = abs(v - ref) / abs(ref)
    assert fig <= 1e-5, (what, v, ref)
    return fig


def _check_grad(g, gref, H, W, what):
    """One gradient map against the statement's (module docstring: the bars)."""
    assert g is not None and g.shape == gref.shape, what
    g = g.double().cpu()
    assert bool(torch.isfinite(g).all()), what
    scale = float(gref.abs().max())
    rect = ss.flat_rect(H, W)
    if rect is not None:
        y0, y1, x0, x1 = rect
        inner = g[:, y0 + 2:y1 - 2, x0 + 2:x1 - 2]
        assert inner.numel() > 0 and bool((inner == 0).all()), what
        assert bool((gref[:, y0 + 2:y1 - 2, x0 + 2:x1 - 2] == 0).all())
    if scale == 0:
        assert bool((g == 0).all()), what
        return 0.0
    fig = float((g - gref).abs().max()) / scale
    assert fig <= 1e-4, (what, fig)
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [(k,) for k in KINDS] + [TOGETHER], ids=lambda k: "+".join(k))
@pytest.mark.parametrize("H,W", SIZES)
def test_native_against_statement(gpu_device, H, W, kinds):
    from materialrefgs_amd import smoothness as sm
    inp, ref = _inputs(H, W), _reference(H, W)
    leaves, items = _items(inp, gpu_device, kinds)
    terms = sm.view_smooth_terms(inp["img"].to(gpu_device), items)
    assert len(terms) == len(kinds)
    up = UP if len(kinds) > 1 else (1.0,)
    figs = {k: _check_term(t, ref[k][0], k) for k, t in zip(kinds, terms)}
    sum(u * t for u, t in zip(up, terms)).backward()
    for k, u, x in zip(kinds, up, leaves):
        figs["g_" + k] = _check_grad(x.grad, u * ref[k][1], H, W, k)
    print(H, W, {k: f"{v:.2e}" for k, v in figs.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(37, 53), SIZES[-1]])
def test_forward_and_backward_are_bitwise_repeatable(gpu_device, H, W):
    from materialrefgs_amd import smoothness as sm
    inp = _inputs(H, W)
    img = inp["img"].to(gpu_device)
    runs = []
    for _ in range(2):
        leaves, items = _items(inp, gpu_device, TOGETHER)
        terms = sm.view_smooth_terms(img, items)
        sum(u * t for u, t in zip(UP, terms)).backward()
        runs.append([t.detach().clone() for t in terms] + [x.grad.clone() for x in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_partial_upstream_gradients(gpu_device):
    """backward() through two of four terms: the other items' maps are not requested (their leaves get no gradient) and the two are the
    statement's.  At the C entry point a map that is given without an upstream gradient is written as zeros, and an item without a map
    is left alone."""
    from materialrefgs_amd import _lib, smoothness as sm
    dev = gpu_device
    H, W = 37, 53
    inp, ref = _inputs(H, W), _reference(H, W)
    img = inp["img"].to(dev)
    leaves, items = _items(inp, dev, TOGETHER)
    terms = sm.view_smooth_terms(img, items)
    (UP[0] * terms[0] + UP[3] * terms[3]).backward()
    assert leaves[1].grad is None and leaves[2].grad is None
    _check_grad(leaves[0].grad, UP[0] * ref[TOGETHER[0]][1], H, W, TOGETHER[0])
    _check_grad(leaves[3].grad, UP[3] * ref[TOGETHER[3]][1], H, W, TOGETHER[3])
    # the entry point itself: item 0 with an upstream gradient, item 1 with a map and none, item 2 with neither
    L, cfg, p = _lib.lib(), _cfg(H, W), _lib.ptr
    data = [x.detach() for x in leaves[:3]]
    outs = [torch.full_like(data[0], float("nan")), torch.full_like(data[1], float("nan")), None]
    mask = inp["mask"].to(dev).view(torch.uint8)
    its = (_lib.MrgsSmoothItem * 3)(_lib.MrgsSmoothItem(p(data[0]), p(mask), p(outs[0]), 3, 0), _lib.MrgsSmoothItem(p(data[1]), None, p(outs[1]), 1, 0),
                                    _lib.MrgsSmoothItem(p(data[2]), None, None, 3, 1))
    one = torch.full((), UP[0], device=dev)
    table = (ctypes.c_void_p * 3)(one.data_ptr(), None, None)
    _lib.check(L.mrgs_smooth_terms_backward(ctypes.byref(cfg), p(img), its, 3, table, _lib.stream_ptr(dev)))
    _check_grad(outs[0], UP[0] * ref[TOGETHER[0]][1], H, W, "entry point")
    assert bool((outs[1] == 0).all())


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    """Forward and backward of four items in one call and of each drop-in: no synchronising call."""
    from materialrefgs_amd import losses, smoothness as sm
    dev = gpu_device
    inp = _inputs(37, 53)
    img, score = inp["img"].to(dev), inp["score"].to(dev)
    leaves, items = _items(inp, dev, TOGETHER)
    up = [torch.tensor(u, device=dev) for u in UP]
    sm.smooth_loss(leaves[1].detach())                                       # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        terms = sm.view_smooth_terms(img, items)
        total = sum(u * t for u, t in zip(up, terms))
        a = sm.albedo_smooth_loss(leaves[0], score)
        b = losses.first_order_edge_aware_loss(leaves[2], img)
        c = losses.smooth_loss(leaves[1])
        (total + a + b + c).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for x in leaves:
        assert float(x.grad.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(3, 3), (37, 53)])
def test_albedo_smooth_loss(gpu_device, H, W):
    """train_refreal.py:1261 with the bool [1,H,W] score on the host and on the device, and as uint8: the statement's
    smooth_loss(base * score)."""
    from materialrefgs_amd import smoothness as sm
    inp, ref = _inputs(H, W), _reference(H, W)
    term, gref = ref["plain3_mask"]
    assert inp["score"].dtype is torch.bool and inp["score"].shape == (1, H, W) and not inp["score"].is_cuda
    for score in (inp["score"], inp["score"].to(gpu_device), inp["score"].to(torch.uint8)):
        base = inp["albedo"].to(gpu_device).requires_grad_(True)
        t = sm.albedo_smooth_loss(base, score)
        _check_term(t, term, "albedo")
        t.backward()
        _check_grad(base.grad, gref, H, W, "albedo")


@pytest.mark.gpu
def test_calculate_loss_with_both_smoothness_terms(gpu_device):
    """calculate_loss on an analytic render_pkg with both smoothness lambdas on, against the same call with both at 0: the two tb_dict
    entries are the statement's terms; the difference of the two losses and of the two runs' rend_normal / surf_depth gradients is lambda
    times the statement's terms and gradients."""
    from materialrefgs_amd import losses
    dev = gpu_device
    H, W = 37, 53
    inp, ref = _inputs(H, W), _reference(H, W)
    lam_n, lam_d = 0.3, 0.7
    cam = SimpleNamespace(original_image=inp["img"].to(dev))
    pc = SimpleNamespace(get_xyz=torch.zeros(5, 3))

    def run(ln, ld):
        pkg = {"render": (0.8 * inp["img"] + 0.1).to(dev).requires_grad_(True), "rend_normal": inp["normal"].to(dev).requires_grad_(True),
               "surf_normal": inp["normal"].to(dev), "surf_depth": inp["depth"].to(dev).requires_grad_(True), "rend_dist": torch.zeros(1, H, W, device=dev)}
        opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.0, normal_loss_start=0, lambda_dist=0.0, dist_loss_start=0,
                              lambda_normal_smooth=ln, lambda_depth_smooth=ld, normal_smooth_from_iter=0, normal_smooth_until_iter=10 ** 9,
                              use_perceptual_loss=False)
        loss, tb = losses.calculate_loss(cam, pc, pkg, opt, 5000)
        loss.backward()
        zeros = lambda k: torch.zeros_like(pkg[k]) if pkg[k].grad is None else pkg[k].grad
        return loss.detach(), tb, zeros("rend_normal"), zeros("surf_depth")

    loss1, tb1, gn1, gd1 = run(lam_n, lam_d)
    loss0, tb0, gn0, gd0 = run(0.0, 0.0)
    assert float(tb0["loss_normal_smooth"]) == 0 and float(tb0["loss_depth_smooth"]) == 0
    figs = {"normal": _check_term(tb1["loss_normal_smooth"], ref["edge3"][0], "loss_normal_smooth"),
            "depth": _check_term(tb1["loss_depth_smooth"], ref["edge1"][0], "loss_depth_smooth")}
    want = lam_n * ref["edge3"][0] + lam_d * ref["edge1"][0]
    figs["loss"] = abs((float(loss1) - float(loss0)) - want) / want
    assert figs["loss"] <= 1e-5, figs
    assert float(tb1["loss"]) == float(loss1)
    figs["g_normal"] = _check_grad(gn1 - gn0, lam_n * ref["edge3"][1], H, W, "rend_normal")
    figs["g_depth"] = _check_grad(gd1 - gd0, lam_d * ref["edge1"][1], H, W, "surf_depth")
    print(figs)
