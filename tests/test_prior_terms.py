"""The per-pixel prior terms (csrc/mrgs_prior.hip: prior_terms_fwd / _finalize / _bwd, behind materialrefgs_amd.priors.view_prior_terms,
mono_normal_loss, mask_entropy_loss and ref_score_loss) against the float64 statement of tests/prior_statement.py and against
tests/golden/reference_prior.npz, the reference's own mono_normal_loss run in float64 by tests/golden/gen_reference_prior_vectors.py.

CPU: the statement against every fixture case (scalars 1e-10 relative, gradients 1e-6 of the map's maximum: the fixture is float32 -- the
bars of the sibling fixtures); the input conditions on every analytic input and fixture case; the C ABI's argument checks; the
wrappers' errors.
GPU (-m gpu): the native node against the statement on analytic inputs at 37x53 (odd, N mod 4 = 1, two workgroups, the second partial), 131x257
(33 workgroups, the last one partial) and 511x515 (see SIZES), each with and without the normal mask, every group alone and all
together; the drop-in mono_normal_loss against the fixture; repeatability; no host read; the NaN cases; partial upstream gradients; one
render_surfel view end to end.
Bars (those of the sibling loss terms, test_multiview_ncc.py): every term within 1e-5 relative; every texel of every gradient map
within 1e-4 of the largest element of that map taken over the pixels with |v_p| > 0, none excluded.  The exact-zero-normal pixels are
compared separately: their gradient is g / 1e-12 and would hide every other texel; each such pixel's gradient (its three channels)
within 1e-5 of that pixel's own largest channel -- relative to the pixel, not to a single channel, because the rotation back to world
space sums three products that may cancel in one channel.
"""
import ctypes
import functools
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prior_statement as ps  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
Z = np.load(os.path.join(GOLDEN, "reference_prior.npz"))
CASES = sorted(k[: -len("_terms")] for k in Z.files if k.endswith("_terms"))
# 511 x 515 = 263 165 pixels = 65 791 quads of four = 257 workgroups of 256 threads: the smallest count above the 256 rows the finalize
# step's 256 threads take per pass, so this is the smallest size (among odd ones with N mod 4 = 1) at which it makes a second pass
SIZES = ((37, 53), (131, 257), (511, 515))
UP = (0.7, 1.3, 0.9, 1.1, 0.8, 1.2, 0.6, 1.4, 0.5, 0.75)       # upstream gradients of the ten terms of prior_statement.NAMES
GROUPS = {"normal": ("surf_normal", "rend_normal"), "entropy": ("rend_alpha",), "ref": ("refl", "rough")}
TERMS = {"normal": ps.NAMES[0:4], "entropy": ps.NAMES[4:5], "ref": ps.NAMES[5:10]}


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def _fixture(name, dtype=torch.float64, dev="cpu"):
    tag, kind = name.split("_")
    f = lambda k: torch.from_numpy(Z[f"{tag}_{k}"].astype(np.float32)).to(dev, dtype)
    mask = (torch.from_numpy(Z[f"{tag}_mask"].astype(np.float32)) / 255).to(dev, dtype) if kind == "mask" else None
    return SimpleNamespace(R=f("R"), surf_normal=f("surf_normal"), rend_normal=f("rend_normal"), prior=f("prior"), mask=mask,
                           terms=Z[f"{name}_terms"], g_surf=Z[f"{name}_g_surf"], g_rend=Z[f"{name}_g_rend"], up=Z["up"])


def test_fixture_cases():
    """Both sizes with and without the mask, and no larger than the sibling fixture."""
    assert CASES == sorted(f"{H}x{W}_{k}" for H, W in ((37, 53), (24, 40)) for k in ("mask", "nomask"))
    assert os.path.getsize(os.path.join(GOLDEN, "reference_prior.npz")) <= os.path.getsize(os.path.join(GOLDEN, "reference_warp.npz"))


@pytest.mark.parametrize("name", CASES)
def test_statement_matches_reference(name):
    """The float64 statement against the reference's own mono_normal_loss: the four scalars and both gradient maps."""
    c = _fixture(name)
    surf, rend = c.surf_normal.clone().requires_grad_(True), c.rend_normal.clone().requires_grad_(True)
    o = ps.prior_terms(R=c.R, surf_normal=surf, rend_normal=rend, prior=c.prior, mask=c.mask)
    for k, ref in zip(ps.NAMES[:4], c.terms):
        assert abs(float(o[k].detach()) - ref) <= 1e-10 * abs(ref), (k, float(o[k].detach()), ref)
    sum(u * o[k] for u, k in zip(c.up, ps.NAMES[:4])).backward()
    for leaf, gref, zero in ((surf, c.g_surf, o["zero_surf"]), (rend, c.g_rend, o["zero_rend"])):
        g, gref = leaf.grad.numpy(), gref.astype(np.float64)
        assert np.abs(g - gref).max() <= 1e-6 * np.abs(gref).max()                       # fixture stored as float32
        live = ~zero.numpy().reshape(gref.shape[1:])                                     # and without the g / 1e-12 entries in the scale
        assert np.abs(g - gref)[:, live].max() <= 1e-6 * np.abs(gref)[:, live].max()


@functools.lru_cache(maxsize=None)
def _inputs(H, W):
    return ps.analytic_inputs(H, W)


@pytest.mark.parametrize("H,W", SIZES)
def test_analytic_inputs_meet_the_conditions(H, W):
    inp = _inputs(H, W)
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    o = ps.prior_terms(R=d["R"], surf_normal=d["surf_normal"], rend_normal=d["rend_normal"], prior=d["prior"], mask=d["mask"], rend_alpha=d["rend_alpha"],
                       alpha_mask=d["mask"], refl=d["refl"], rough=d["rough"], score=d["score"])
    ps.check_conditions(inp, o["margin"])
    o2 = ps.prior_terms(R=d["R"], surf_normal=d["surf_normal"], rend_normal=d["rend_normal"], prior=d["prior"], mask=None)
    assert o2["margin"] >= 1e-4                                                          # without the mask every pixel counts
    assert (H * W) % 4 != 0


@pytest.mark.parametrize("name", CASES)
def test_fixture_inputs_meet_the_conditions(name):
    c = _fixture(name)
    o = ps.prior_terms(R=c.R, surf_normal=c.surf_normal, rend_normal=c.rend_normal, prior=c.prior, mask=c.mask)
    N = c.prior.shape[0]
    assert o["margin"] >= 1e-4
    inside = (c.mask.reshape(-1) > 0) if c.mask is not None else torch.ones(N, dtype=torch.bool)
    assert int(o["zero_rend"].sum()) >= 0.05 * N and int((o["zero_rend"] & inside).sum()) >= 0.01 * N
    if c.mask is not None:
        assert int(((c.mask > 0) & (c.mask < 1)).sum()) > 0


def _cfg(H=37, W=53):
    from materialrefgs_amd import _lib
    return _lib.MrgsPriorConfig(H, W, 0)


def test_prior_abi_argument_checks_without_gpu():
    """The three entry points exist, ws_bytes is 0 for sizes the calls refuse, and every contract violation is MRGS_E_BAD_ARG (1) before
    anything is launched (no pointer below is ever dereferenced)."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    assert L.mrgs_prior_ws_bytes(37, 53) == 2 * 48 and L.mrgs_prior_ws_bytes(131, 257) == 33 * 48 and L.mrgs_prior_ws_bytes(511, 515) == 257 * 48
    assert L.mrgs_prior_ws_bytes(4000, 4000) == 1024 * 48                              # the grid is bounded
    for bad in ((0, 53), (37, 0), (-1, 53), (37, -5)):
        assert L.mrgs_prior_ws_bytes(*bad) == 0, bad
    hdr = open(os.path.join(ROOT, "include", "mrgs.h")).read()
    for sym in ("mrgs_prior_ws_bytes", "mrgs_prior_terms_forward", "mrgs_prior_terms_backward"):
        assert sym in hdr
    assert L.mrgs_abi_version() == 10                                                   # entry points only: the revision stays
    p = 0x1000
    rt = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    big = 1 << 20
    names = ("surf", "rend", "prior", "mask", "alpha", "amask", "refl", "rough", "score")

    def fwd(cfg=None, rt=rt, ws=p, ws_bytes=big, out=p, **kw):
        a = dict.fromkeys(names, p)
        a.update(kw)
        return L.mrgs_prior_terms_forward(ctypes.byref(cfg or _cfg()), rt, *(a[n] for n in names), ws, ws_bytes, out, None)

    def bwd(cfg=None, rt=rt, terms=p, table=(ctypes.c_void_p * 16)(), outs=(p, p, p, p, p), **kw):
        a = dict.fromkeys(names, p)
        a.update(kw)
        return L.mrgs_prior_terms_backward(ctypes.byref(cfg or _cfg()), rt, *(a[n] for n in names), terms, table, *outs, None)

    bad = _cfg()
    bad.struct_size -= 4
    assert fwd(bad) == 1 and bwd(bad) == 1
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(flags=1)):
        c = _cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        assert fwd(c) == 1 and bwd(c) == 1, kw
    assert L.mrgs_prior_terms_forward(None, rt, *([p] * 9), p, big, p, None) == 1
    for n in names:                                            # a group with only some of its pointers (the mask alone is optional)
        if n != "mask":
            assert fwd(**{n: None}) == 1 and bwd(**{n: None}) == 1, n
    assert fwd(**dict.fromkeys(names, None)) == 1 and bwd(**dict.fromkeys(names, None)) == 1          # no group at all
    assert fwd(surf=None, rend=None, prior=None) == 1          # a mask without the normal group
    assert fwd(rt=None) == 1 and bwd(rt=None) == 1
    assert fwd(ws=None) == 1 and fwd(out=None) == 1 and fwd(ws=p + 4) == 1
    assert fwd(ws_bytes=2 * 48 - 1) == 1                       # a workspace that is too small
    assert bwd(terms=None) == 1 and bwd(table=None) == 1
    off = dict(surf=None, rend=None, prior=None, mask=None)
    assert bwd(**off) == 1                                     # gradient maps of a group that is off
    assert bwd(outs=(None, None, None, None, None)) == 0       # nothing to write: nothing launched


def test_wrappers_raise_without_gpu():
    """A CPU tensor, another dtype or a shape that does not match H x W raises before anything native is touched."""
    from materialrefgs_amd import priors
    H, W = 6, 10
    cam = SimpleNamespace(R=np.eye(3, dtype=np.float32), T=np.zeros(3, dtype=np.float32), HWK=(H, W, np.eye(3, dtype=np.float32)), image_name="a")
    n3, n1 = torch.rand(3, H, W), torch.rand(1, H, W)
    normals, masks = {"a": torch.rand(H * W, 3)}, {"a": torch.rand(H * W, 1)}
    with pytest.raises(RuntimeError, match="device tensor"):
        priors.mono_normal_loss(cam, n3, n3, masks, normals, 1.0, 7)
    with pytest.raises(RuntimeError, match="device tensor"):
        priors.mask_entropy_loss(n1, masks["a"])
    with pytest.raises(RuntimeError, match="device tensor"):
        priors.ref_score_loss(n1, n1, n1 > 0.5, 0.1)
    with pytest.raises(TypeError, match="float32"):
        priors.mono_normal_loss(cam, n3.double(), n3, masks, normals, 1.0, 7)
    with pytest.raises(TypeError, match="float32"):
        priors.mask_entropy_loss(n1.half(), masks["a"])
    with pytest.raises(TypeError, match="float32"):
        priors.ref_score_loss(n1, n1.double(), n1 > 0.5, 0.1)
    with pytest.raises(ValueError, match="shape"):
        priors.mono_normal_loss(cam, n3, torch.rand(3, H, W + 1), masks, normals, 1.0, 7)
    with pytest.raises(ValueError, match="shape"):
        priors.ref_score_loss(n1, torch.rand(1, H + 1, W), n1 > 0.5, 0.1)
    with pytest.raises(ValueError, match="shape"):
        priors.mono_normal_loss(cam, torch.rand(4, H, W), n3, masks, normals, 1.0, 7)
    with pytest.raises(ValueError, match="no group"):
        priors.view_prior_terms(cam)
    with pytest.raises(ValueError, match="needs"):
        priors.view_prior_terms(cam, surf_normal=n3, rend_normal=n3)
    with pytest.raises(ValueError, match="needs"):
        priors.view_prior_terms(rend_alpha=n1)
    with pytest.raises(ValueError, match="needs"):
        priors.view_prior_terms(refl_strength_map=n1, ref_score_image=n1 > 0.5)
    moved = priors.to_device({"a": torch.ones(2), "b": None}, "cpu")
    assert moved["b"] is None and torch.equal(moved["a"], torch.ones(2)) and priors.to_device(None, "cpu") is None


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _camera(R, H, W):
    return SimpleNamespace(R=R.cpu().numpy().astype(np.float32), T=np.zeros(3, dtype=np.float32), HWK=(H, W, np.eye(3, dtype=np.float32)),
                           image_name="view")


@functools.lru_cache(maxsize=None)
def _reference(H, W, masked):
    """The float64 statement of all three groups on the analytic inputs, once per (size, mask): terms, the gradient maps of
    sum_k UP_k term_k, and where the rotated normals are exactly zero."""
    inp = _inputs(H, W)
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")}
    o = ps.prior_terms(R=d["R"], prior=d["prior"], mask=d["mask"] if masked else None, alpha_mask=d["mask"], score=d["score"], **leaves)
    sum(u * o[k] for u, k in zip(UP, ps.NAMES)).backward()
    return dict(terms={k: float(o[k].detach()) for k in ps.NAMES}, grads={k: v.grad for k, v in leaves.items()},
                zero={"surf_normal": o["zero_surf"], "rend_normal": o["zero_rend"]})


def _leaves(inp, dev, names=("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")):
    return {k: inp[k].to(dev).clone().requires_grad_(True) for k in names}


def _native(inp, dev, leaves, groups, masked, cpu_priors=False):
    from materialrefgs_amd import priors
    H, W = inp["rend_alpha"].shape[-2:]
    mv = (lambda t: t) if cpu_priors else (lambda t: t.to(dev))
    mask = mv(inp["mask"])
    kw = {}
    if "normal" in groups:
        kw.update(surf_normal=leaves["surf_normal"], rend_normal=leaves["rend_normal"], normal_prior=mv(inp["prior"]), normal_mask=mask if masked else None)
    if "entropy" in groups:
        kw.update(rend_alpha=leaves["rend_alpha"], alpha_mask=mask)
    if "ref" in groups:
        kw.update(refl_strength_map=leaves["refl"], roughness_map=leaves["rough"], ref_score_image=mv(inp["score"]))
    return priors.view_prior_terms(_camera(inp["R"], H, W) if "normal" in groups else None, **kw)


def _check_terms(t, ref, groups):
    figs = {}
    for grp, names in TERMS.items():
        for k in names:
            mine = getattr(t, k)
            if grp not in groups:
                assert mine is None, k
                continue
            assert mine.dim() == 0 and mine.is_cuda
            figs[k] = abs(float(mine.detach()) - ref["terms"][k]) / abs(ref["terms"][k])
            assert figs[k] <= 1e-5, (k, float(mine.detach()), ref["terms"][k])
    return figs


def _check_grad(key, g, ref, figs):
    """One gradient map against the statement's (module docstring: the bars)."""
    gref = ref["grads"][key].to(g.device)
    g = g.double().reshape(gref.shape)
    assert bool(torch.isfinite(g).all()), key
    zero = ref["zero"].get(key)
    if zero is None:
        scale = float(gref.abs().max())
        figs[key] = float((g - gref).abs().max()) / scale
        assert scale > 0 and figs[key] <= 1e-4, (key, figs)
        return
    zero = zero.to(g.device).reshape(gref.shape[1:])
    scale = float(gref[:, ~zero].abs().max())
    figs[key] = float((g - gref)[:, ~zero].abs().max()) / scale
    assert scale > 0 and figs[key] <= 1e-4, (key, figs)
    own = gref[:, zero].abs().max(dim=0).values                # per exact-zero pixel: its largest channel (0 outside the mask)
    err = (g - gref)[:, zero].abs().max(dim=0).values
    assert bool((err <= 1e-5 * own).all()), (key, float((err / own.clamp_min(1e-300)).max()))
    figs[key + "_zero"] = float((err[own > 0] / own[own > 0]).max()) if bool((own > 0).any()) else 0.0
    assert int((own > 0).sum()) > 0                            # such pixels exist and carry the g / 1e-12 gradient
    assert float(own.max()) > 1e3 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [("normal",), ("entropy",), ("ref",), ("normal", "entropy", "ref")], ids=lambda g: "+".join(g))
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("H,W", SIZES)
def test_native_against_statement(gpu_device, H, W, masked, groups):
    inp, ref = _inputs(H, W), _reference(H, W, masked)
    leaves = _leaves(inp, gpu_device)
    t = _native(inp, gpu_device, leaves, groups, masked)
    figs = _check_terms(t, ref, groups)
    sum(u * getattr(t, k) for u, k in zip(UP, ps.NAMES) if getattr(t, k) is not None).backward()
    for grp, keys in GROUPS.items():
        for key in keys:
            if grp in groups:
                _check_grad(key, leaves[key].grad, ref, figs)
            else:
                assert leaves[key].grad is None, key
    print(H, W, masked, groups, {k: f"{v:.2e}" for k, v in figs.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_drop_in_replays_reference(gpu_device, name):
    """mono_normal_loss with the reference's arguments (prior dictionaries on the host, as its loaders leave them) against the
    reference's own numbers."""
    from materialrefgs_amd import priors
    dev = gpu_device
    c = _fixture(name, torch.float32)
    H, W = c.surf_normal.shape[-2:]
    surf, rend = c.surf_normal.to(dev).requires_grad_(True), c.rend_normal.to(dev).requires_grad_(True)
    cam = SimpleNamespace(R=c.R.to(dev), T=torch.zeros(3, device=dev), HWK=(H, W, np.eye(3, dtype=np.float32)), image_name="view")   # R as a device tensor
    masks = {"view": c.mask.reshape(-1, 1)} if c.mask is not None else None
    r = priors.mono_normal_loss(cam, surf, rend, masks, {"view": c.prior}, 1.0, 3000, None, None)
    assert len(r) == 4
    for mine, ref in zip(r, c.terms):
        assert mine.dim() == 0 and mine.device == surf.device
        assert abs(float(mine) - ref) <= 1e-5 * abs(ref), (float(mine), ref)
    sum(float(u) * t for u, t in zip(c.up, r)).backward()
    d = _fixture(name)
    o = ps.prior_terms(R=d.R, surf_normal=d.surf_normal, rend_normal=d.rend_normal, prior=d.prior, mask=d.mask)
    ref = dict(grads={"surf_normal": torch.from_numpy(c.g_surf).double(), "rend_normal": torch.from_numpy(c.g_rend).double()},
               zero={"surf_normal": o["zero_surf"], "rend_normal": o["zero_rend"]})
    figs = {}
    _check_grad("surf_normal", surf.grad, ref, figs)
    _check_grad("rend_normal", rend.grad, ref, figs)
    print(name, figs)


@pytest.mark.gpu
def test_forward_and_backward_are_bitwise_repeatable(gpu_device):
    inp = _inputs(131, 257)
    runs = []
    for _ in range(3):
        leaves = _leaves(inp, gpu_device)
        t = _native(inp, gpu_device, leaves, ("normal", "entropy", "ref"), True)
        sum(u * x for u, x in zip(UP, t)).backward()
        runs.append([x.detach().clone() for x in t] + [leaves[k].grad.clone() for k in sorted(leaves)])
    for run in runs[1:]:
        for a, b in zip(run, runs[0]):
            assert torch.equal(a, b)


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    """Forward and backward of all groups, of each drop-in and with a camera whose R is a numpy array: no synchronising call."""
    from materialrefgs_amd import priors
    dev = gpu_device
    inp = _inputs(37, 53)
    leaves = _leaves(inp, dev)
    dv = {k: v.to(dev) for k, v in inp.items()}
    cam = _camera(inp["R"], 37, 53)
    masks, normals = {"view": dv["mask"]}, {"view": dv["prior"]}
    up = [torch.tensor(u, device=dev) for u in UP]
    priors.mask_entropy_loss(leaves["rend_alpha"].detach(), dv["mask"])       # (the library is loaded)
    from materialrefgs_amd._camconst import consts
    consts(cam, dev).rt_host                                                  # the camera's constants: uploaded once per camera and pose
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t = priors.view_prior_terms(cam, surf_normal=leaves["surf_normal"], rend_normal=leaves["rend_normal"], normal_prior=dv["prior"],
                                    normal_mask=dv["mask"], rend_alpha=leaves["rend_alpha"], alpha_mask=dv["mask"],
                                    refl_strength_map=leaves["refl"], roughness_map=leaves["rough"], ref_score_image=dv["score"])
        total = sum(u * x for u, x in zip(up, t))
        a = priors.mono_normal_loss(cam, leaves["surf_normal"], leaves["rend_normal"], masks, normals, 1.0, 3000)
        b = priors.mask_entropy_loss(leaves["rend_alpha"], dv["mask"])
        c = priors.ref_score_loss(leaves["refl"], leaves["rough"], dv["score"], 0.05)
        (total + a[0] + a[3] + 0.01 * b + c).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for k, v in leaves.items():
        assert float(v.grad.abs().max()) > 0, k


@pytest.mark.gpu
def test_nan_exactly_where_the_statement_has_it(gpu_device):
    """An all-zero mask and an empty S (and an empty complement): NaN in the terms the statement has NaN in, the other groups finite."""
    dev = gpu_device
    base = _inputs(37, 53)
    for change in ("mask", "S", "notS"):
        inp = dict(base)
        if change == "mask":
            inp["mask"] = torch.zeros_like(base["mask"])
        else:
            inp["score"] = torch.zeros_like(base["score"]) if change == "S" else torch.ones_like(base["score"])
        d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
        o = ps.prior_terms(R=d["R"], surf_normal=d["surf_normal"], rend_normal=d["rend_normal"], prior=d["prior"], mask=d["mask"],
                           rend_alpha=d["rend_alpha"], alpha_mask=base["mask"].double(), refl=d["refl"], rough=d["rough"], score=d["score"])
        from materialrefgs_amd import priors
        t = priors.view_prior_terms(_camera(inp["R"], 37, 53), surf_normal=inp["surf_normal"].to(dev), rend_normal=inp["rend_normal"].to(dev),
                                    normal_prior=inp["prior"].to(dev), normal_mask=inp["mask"].to(dev), rend_alpha=inp["rend_alpha"].to(dev),
                                    alpha_mask=base["mask"].to(dev), refl_strength_map=inp["refl"].to(dev), roughness_map=inp["rough"].to(dev),
                                    ref_score_image=inp["score"].to(dev))
        nans = {k for k in ps.NAMES if math.isnan(float(o[k]))}
        assert nans == {"mask": set(ps.NAMES[0:4]), "S": {"ref_metallic", "ref_roughness", "ref_sum"},
                        "notS": {"ref_metallic_bg", "ref_roughness_bg", "ref_sum"}}[change]
        for k in ps.NAMES:
            mine = float(getattr(t, k))
            if k in nans:
                assert math.isnan(mine), (change, k, mine)
            else:
                assert abs(mine - float(o[k])) <= 1e-5 * abs(float(o[k])), (change, k, mine, float(o[k]))


@pytest.mark.gpu
@pytest.mark.parametrize("term", ["cos_rend", "l1_surf", "mask_entropy", "ref_roughness_bg", "ref_sum"])
def test_backward_through_one_term(gpu_device, term):
    """backward() through a single term, every other upstream gradient None: the statement's gradient maps of that term alone; the maps
    no term reaches get no gradient."""
    dev = gpu_device
    H, W = 37, 53
    inp = _inputs(H, W)
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()}
    ref_leaves = {k: d[k].clone().requires_grad_(True) for k in ("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")}
    o = ps.prior_terms(R=d["R"], prior=d["prior"], mask=d["mask"], alpha_mask=d["mask"], score=d["score"], **ref_leaves)
    o[term].backward()
    ref = dict(grads={k: v.grad for k, v in ref_leaves.items()}, zero={"surf_normal": o["zero_surf"], "rend_normal": o["zero_rend"]})
    leaves = _leaves(inp, dev)
    t = _native(inp, dev, leaves, ("normal", "entropy", "ref"), True)
    getattr(t, term).backward()
    figs = {}
    for key, leaf in leaves.items():
        if ref["grads"][key] is None:
            assert leaf.grad is None, key
        else:
            _check_grad(key, leaf.grad, ref, figs)
    print(term, figs)


@pytest.mark.gpu
def test_maps_of_a_group_without_upstream_are_zeros(gpu_device):
    """The C entry point writes every gradient map it is given in full: zeros for a group none of whose upstream gradients is set."""
    from materialrefgs_amd import _lib
    dev = gpu_device
    H, W = 37, 53
    inp = {k: v.to(dev) for k, v in _inputs(H, W).items()}
    L, cfg = _lib.lib(), _cfg(H, W)
    rt = (ctypes.c_float * 9)(*inp["R"].T.reshape(-1).tolist())
    p = _lib.ptr
    ws = torch.empty(L.mrgs_prior_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    terms = torch.empty(16, device=dev)
    score = inp["score"].view(torch.uint8)
    maps = (p(inp["surf_normal"]), p(inp["rend_normal"]), p(inp["prior"]), p(inp["mask"]), p(inp["rend_alpha"]), p(inp["mask"]), p(inp["refl"]),
            p(inp["rough"]), p(score))
    st = _lib.stream_ptr(dev)
    _lib.check(L.mrgs_prior_terms_forward(ctypes.byref(cfg), rt, *maps, p(ws), ws.numel(), p(terms), st))
    one = torch.ones((), device=dev)
    table = (ctypes.c_void_p * 16)()
    table[4] = one.data_ptr()                                   # only the entropy has an upstream gradient
    outs = [torch.full_like(inp[k], float("nan")) for k in ("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")]
    _lib.check(L.mrgs_prior_terms_backward(ctypes.byref(cfg), rt, *maps, p(terms), table, *(p(o) for o in outs), st))
    for o, k in zip(outs, ("surf_normal", "rend_normal", "rend_alpha", "refl", "rough")):
        assert (float(o.abs().max()) > 0) == (k == "rend_alpha") and bool(torch.isfinite(o).all()), k


def _torch_form(cam_R, pkg, prior, mask, score, weight):
    """The literal float32 torch form of the three groups as the scripts write them, on the device."""
    o = ps.prior_terms(R=cam_R, surf_normal=pkg["surf_normal"], rend_normal=pkg["rend_normal"], prior=prior, mask=mask, rend_alpha=pkg["rend_alpha"],
                       alpha_mask=mask, refl=pkg["refl_strength_map"], rough=pkg["roughness_map"], score=score, terms_only=True)
    return (0.01 * (o["l1_surf"] + o["cos_surf"] + o["l1_rend"] + o["cos_rend"]) + 0.01 * o["mask_entropy"] + weight * o["ref_metallic"] +
            weight * o["ref_roughness"] + weight * o["ref_metallic_bg"] + .5 * weight * o["ref_roughness_bg"])


def end_to_end_figures(dev):
    """One render_surfel view; total = calculate_loss + the prior terms, once with the native node and once with the float32 torch form on
    the same rendered maps.  Returns the largest leaf-gradient difference between the two (relative to the leaf's largest element) and,
    per rendered map, the distance of each path's map gradient from the float64 statement (same scale)."""
    from materialrefgs_amd import losses, priors
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    H, W = 64, 80
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False, use_asg=False)
    pc, env, leaves = make_surfel_model(800, max(H, W), dev, seed=1, radius_px=5.0, env_res=64, env_min=16)
    cam = orbit_camera(1, H, W, n_views=8).to(dev)
    env.build_mips()
    pkg = render_surfel(cam, pc, pipe, torch.zeros(3, device=dev), srgb=False, opt=SimpleNamespace(indirect=False))
    keys = ("surf_normal", "rend_normal", "rend_alpha", "refl_strength_map", "roughness_map")
    for k in keys:
        pkg[k].retain_grad()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        alpha = pkg["rend_alpha"].reshape(-1, 1)
        # the image mask: fractional at the object's edge, zero where nothing was rendered (a pixel with an exactly zero normal inside the
        # mask has a gradient of g / 1e-12, which no leaf comparison survives; test_native_against_statement covers those pixels)
        mask = (alpha.clamp(0, 1) * 1.2).clamp(0, 1) * (pkg["rend_normal"].abs().sum(0).reshape(-1, 1) > 0) * (pkg["surf_normal"].abs().sum(0).reshape(-1, 1) > 0)
        mask = (torch.round(mask * 255) / 255).contiguous()
        prior = torch.nn.functional.normalize(pkg["rend_normal"].reshape(3, -1).T @ cam.R + 0.3 * torch.randn(H * W, 3, generator=g).to(dev), dim=-1).contiguous()
        score = (pkg["refl_strength_map"] > pkg["refl_strength_map"].median()).contiguous()
        gt = (pkg["render"] + 0.05 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
    view = SimpleNamespace(R=cam.R, T=cam.T, HWK=cam.HWK, image_name="v", original_image=gt)
    opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.05, normal_loss_start=0, lambda_dist=100.0, dist_loss_start=0,
                          lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                          use_perceptual_loss=False)
    weight = 0.1

    def grads(total):
        for t in leaves + [pkg[k] for k in keys]:
            t.grad = None
        total.backward(retain_graph=True)
        return ([t.grad.detach().clone() for t in leaves],
                {k: torch.zeros_like(pkg[k]) if pkg[k].grad is None else pkg[k].grad.detach().clone() for k in keys})

    base, _tb = losses.calculate_loss(view, pc, pkg, opt, 1, losses.image_weight(gt), None)
    _l, only_base = grads(base)                                 # calculate_loss's own share of the map gradients (normals)
    t = priors.view_prior_terms(view, surf_normal=pkg["surf_normal"], rend_normal=pkg["rend_normal"], normal_prior=prior, normal_mask=mask,
                                rend_alpha=pkg["rend_alpha"], alpha_mask=mask, refl_strength_map=pkg["refl_strength_map"],
                                roughness_map=pkg["roughness_map"], ref_score_image=score)
    native = base + 0.01 * (t.l1_surf + t.cos_surf + t.l1_rend + t.cos_rend) + 0.01 * t.mask_entropy + weight * t.ref_sum
    leaf_n, map_n = grads(native)
    torch_total = base + _torch_form(cam.R, pkg, prior, mask, score, weight)
    leaf_t, map_t = grads(torch_total)
    d = lambda x: x.detach().double()
    p64 = {k: d(pkg[k]).requires_grad_(True) for k in keys}
    _torch_form(d(cam.R), p64, d(prior), d(mask), score, weight).backward()
    figs = {"total": (float(native), float(torch_total)),
            "leaf": max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(leaf_n, leaf_t) if float(b.abs().max()) > 0)}
    for k in keys:
        ref = p64[k].grad
        scale = float(ref.abs().max())
        figs[k] = (float((d(map_n[k]) - d(only_base[k]) - ref).abs().max()) / scale, float((d(map_t[k]) - d(only_base[k]) - ref).abs().max()) / scale)
    figs["mask_pixels"] = int((mask > 0).sum())
    return figs


@pytest.mark.gpu
def test_end_to_end_with_calculate_loss(gpu_device):
    """render_surfel -> view_prior_terms + calculate_loss -> backward, against the same scalar built from the float32 torch form of the
    terms: both paths share every kernel below the terms, and every leaf gradient agrees within 2e-6 of the leaf's largest element
    (measured on an MI355X: 4.2e-7; the map gradients of the two paths are 1.4e-8 .. 2.4e-7 of a map's largest element from the
    float64 statement, the native path no further than the torch form except on rend_alpha, 1.60e-7 against 1.56e-7)."""
    figs = end_to_end_figures(gpu_device)
    print(figs)
    assert figs["mask_pixels"] > 500
    assert abs(figs["total"][0] - figs["total"][1]) <= 1e-5 * abs(figs["total"][1])
    assert figs["leaf"] <= 2e-6, figs
