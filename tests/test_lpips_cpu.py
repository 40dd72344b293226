"""The native LPIPS (VGG16) term without a GPU: the float64 statement (tests/lpips_statement.py) against the reference's own
lpipsPyTorch run (tests/golden/reference_lpips.npz), the C ABI's exports and argument checks, the weight loader's three key layouts,
the decision machinery of the GPU gradient test with the literal fp32 torch reading standing in for the kernel, and the MRGS_LPIPS_WEIGHTS
hook of materialrefgs_amd.losses with the lpipsPyTorch shim.
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lpips_statement as ls  # noqa: E402

NET_SIZES = ((16, 16), (19, 22), (33, 40), (64, 48))      # those of tests/test_lpips_gpu.py, same seeds
SEED = 0


def test_statement_equals_the_reference_fixture():
    """float64 against float64, the same operations: outputs and dx to 1e-12 relative (dx: of its largest element)."""
    fix = np.load(os.path.join(ROOT, "tests", "golden", "reference_lpips.npz"))
    w = ls.cast_weights(ls.random_weights(int(fix["seed"])))
    for tag in "abc":
        x = torch.from_numpy(fix[f"{tag}_x"]).double().requires_grad_(True)
        y = torch.from_numpy(fix[f"{tag}_y"]).double()
        run = ls.lpips(w, x, y)
        run.total.backward()
        want, dx = float(fix[f"{tag}_out"].reshape(())), torch.from_numpy(fix[f"{tag}_dx"])
        assert abs(float(run.total) - want) <= 1e-12 * want, tag
        assert float((x.grad - dx).abs().max()) <= 1e-12 * float(dx.abs().max()), tag
        f5 = run.x.acts[12].detach()
        f5 = f5 / (f5.pow(2).sum(0, keepdim=True).sqrt() + ls.EPS)
        assert float((f5 - torch.from_numpy(fix[f"{tag}_feat5"])).abs().max()) <= 1e-12
        assert float(torch.from_numpy(fix[f"{tag}_feat1_norm"]).min()) > 0.5      # no all-zero vector: the one rule that differs is not met


def test_abi_exports_sizes_and_argument_checks():
    from materialrefgs_amd import _lib
    L = _lib.lib()
    for name in ("mrgs_lpips_weights_bytes", "mrgs_lpips_pack_weights", "mrgs_lpips_ws_bytes", "mrgs_lpips_ws_offsets", "mrgs_lpips_forward",
                 "mrgs_lpips_backward", "mrgs_lpips_debug_conv", "mrgs_lpips_debug_pool", "mrgs_lpips_debug_head"):
        assert name in _lib.SYMBOLS and getattr(L, name)
    n_w = sum(9 * ci * co for ci, co in __import__("materialrefgs_amd.lpips", fromlist=["x"]).CONV_CHANNELS)
    assert L.mrgs_lpips_weights_bytes() >= 4 * (2 * n_w + 4224 + 1472) and L.mrgs_lpips_weights_bytes() % 256 == 0
    # the workspace: 0 for refused sizes, growing with either dimension and with with_grad, at least the stated floats
    last = 0
    for s in (16, 17, 31, 32, 100, 800):
        small, big = L.mrgs_lpips_ws_bytes(s, s, 0), L.mrgs_lpips_ws_bytes(s, s, 1)
        assert last < small < big and big >= 4 * 600 * (s // 16 * 16) ** 2 * 0.9 and small >= 4 * 256 * s * s
        assert L.mrgs_lpips_ws_bytes(s, s + 1, 1) >= big and L.mrgs_lpips_ws_bytes(s + 1, s, 1) >= big
        last = small
    assert abs(L.mrgs_lpips_ws_bytes(800, 800, 1) / (600 * 640000 * 4) - 1) < 0.01
    for H, W, g in ((15, 16, 0), (16, 15, 1), (0, 0, 0), (-1, 64, 0), (16, 16, 2), (1 << 13, 1 << 13, 0)):
        assert L.mrgs_lpips_ws_bytes(H, W, g) == 0
    offs = (ctypes.c_size_t * 18)()
    assert L.mrgs_lpips_ws_offsets(19, 22, offs) == 0 and list(offs) == sorted(offs) and offs[17] < L.mrgs_lpips_ws_bytes(19, 22, 1)
    assert L.mrgs_lpips_ws_offsets(15, 22, offs) == _lib.MRGS_E_BAD_ARG and L.mrgs_lpips_ws_offsets(19, 22, None) == _lib.MRGS_E_BAD_ARG
    # every contract violation returns MRGS_E_BAD_ARG with no pointer dereferenced: the pointers below are not mapped
    bad, P = _lib.MRGS_E_BAD_ARG, 0x1000
    ok = _lib.MrgsLpipsConfig(16, 16, 1.0, 0.0, 1)
    big = 1 << 40
    terms = P

    def fwd(cfg=ok, blob=P, x=P, y=P, ws=P, n=big, t=terms):
        return L.mrgs_lpips_forward(ctypes.byref(cfg) if cfg is not None else None, blob, x, y, ws, n, t, None)
    assert fwd(cfg=None) == bad
    for k in ("blob", "x", "y", "ws", "t"):
        assert fwd(**{k: None}) == bad, k
    assert fwd(blob=P + 16) == bad and fwd(ws=P + 128) == bad
    assert fwd(n=L.mrgs_lpips_ws_bytes(16, 16, 1) - 1) == bad
    for cfg in (_lib.MrgsLpipsConfig(15, 16, 1.0, 0.0, 0), _lib.MrgsLpipsConfig(16, 15, 1.0, 0.0, 0), _lib.MrgsLpipsConfig(16, 16, 1.0, 0.0, 2)):
        assert fwd(cfg=cfg) == bad
    wrong = _lib.MrgsLpipsConfig(16, 16, 1.0, 0.0, 1)
    wrong.struct_size -= 4
    assert fwd(cfg=wrong) == bad

    def bwd(cfg=ok, blob=P, ws=P, g=P, gx=P):
        return L.mrgs_lpips_backward(ctypes.byref(cfg) if cfg is not None else None, blob, ws, g, gx, None)
    assert bwd(cfg=None) == bad and bwd(cfg=_lib.MrgsLpipsConfig(16, 16, 1.0, 0.0, 0)) == bad and bwd(cfg=_lib.MrgsLpipsConfig(15, 16, 1.0, 0.0, 1)) == bad
    for k in ("blob", "ws", "g", "gx"):
        assert bwd(**{k: None}) == bad, k
    tab = (ctypes.c_void_p * 13)(*([P] * 13))
    tab5 = (ctypes.c_void_p * 5)(*([P] * 5))
    hole = (ctypes.c_void_p * 13)(*([P] * 12 + [None]))
    assert L.mrgs_lpips_pack_weights(None, tab, tab5, P, None) == bad and L.mrgs_lpips_pack_weights(tab, tab, tab5, None, None) == bad
    assert L.mrgs_lpips_pack_weights(hole, tab, tab5, P, None) == bad and L.mrgs_lpips_pack_weights(tab, tab, tab5, P + 8, None) == bad

    def conv(H=5, W=5, ci=64, co=64, n=2, backward=0, relu=0, zs=0, inp=P, w=P, out=P, ws=P, nb=big, add=None, gate=None):
        cfg = _lib.MrgsLpipsConvConfig(H, W, ci, co, n, backward, relu, zs, 1.0, 0.0)
        return L.mrgs_lpips_debug_conv(ctypes.byref(cfg), inp, w, None, add, gate, out, ws, nb, None)
    for kw in (dict(H=0), dict(W=0), dict(ci=64, co=256), dict(ci=32), dict(n=0), dict(n=3), dict(backward=2), dict(relu=2), dict(inp=None), dict(w=None),
               dict(out=None), dict(ws=None), dict(inp=P + 4), dict(nb=36 * 64 * 64 - 1), dict(ci=3, add=P), dict(ci=3, backward=1, gate=P)):
        assert conv(**kw) == bad, kw
    assert L.mrgs_lpips_debug_pool(0, 4, 64, P, None, P, None) == bad and L.mrgs_lpips_debug_pool(4, 4, 6, P, None, P, None) == bad
    assert L.mrgs_lpips_debug_pool(4, 4, 64, None, None, P, None) == bad
    assert L.mrgs_lpips_debug_head(0, 64, P, P, P, P, big, P, None, None, None) == bad
    assert L.mrgs_lpips_debug_head(5, 96, P, P, P, P, big, P, None, None, None) == bad
    assert L.mrgs_lpips_debug_head(5, 64, P, P, P, P, 100, P, None, None, None) == bad
    assert L.mrgs_lpips_debug_head(5, 64, P, P, P, P, big, P, None, P, None) == bad


@pytest.mark.skipif(torch.cuda.device_count() != 0, reason="host addresses as arguments: only for a machine without a device")
def test_launch_failure_goes_through_the_one_status_path():
    """Without a device every launch fails: MRGS_E_HIP, and mrgs_last_hip_error() names this file (as tests/test_status.py shows for the
    others), from each entry point that launches."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    P = (ctypes.addressof(buf) + 255) & ~255
    big = 1 << 40
    cfg = _lib.MrgsLpipsConfig(16, 16, 1.0, 0.0, 1)
    conv = _lib.MrgsLpipsConvConfig(4, 4, 64, 64, 1, 0, 1, 0, 1.0, 0.0)
    tab, tab5 = (ctypes.c_void_p * 13)(*([P] * 13)), (ctypes.c_void_p * 5)(*([P] * 5))
    calls = {"pack": lambda: L.mrgs_lpips_pack_weights(tab, tab, tab5, P, None),
             "forward": lambda: L.mrgs_lpips_forward(ctypes.byref(cfg), P, P, P, P, big, P, None),
             "backward": lambda: L.mrgs_lpips_backward(ctypes.byref(cfg), P, P, P, P, None),
             "conv": lambda: L.mrgs_lpips_debug_conv(ctypes.byref(conv), P, P, None, None, None, P, P, big, None),
             "pool": lambda: L.mrgs_lpips_debug_pool(4, 4, 64, P, None, P, None),
             "head": lambda: L.mrgs_lpips_debug_head(5, 64, P, P, P, P, big, P, None, None, None)}
    seen = set()
    for name, call in calls.items():
        assert call() == _lib.MRGS_E_HIP, name
        text = L.mrgs_last_hip_error()
        assert text and b" at mrgs_lpips.hip:" in text, (name, text)
        seen.add(text)
    assert len(seen) == len(calls)                        # each entry point reports its own line


def _layouts():
    from materialrefgs_amd.lpips import CONV_INDEX
    conv_w, conv_b, lin_w = ls.random_weights(3)
    lin4 = [w.reshape(1, -1, 1, 1) for w in lin_w]
    tv, pk, ref = {}, {}, {}
    slice_of = lambda n: 1 + sum(n > e for e in (3, 8, 15, 22))
    for i, n in enumerate(CONV_INDEX):
        for kind, t in (("weight", conv_w[i]), ("bias", conv_b[i])):
            tv[f"features.{n}.{kind}"] = t
            pk[f"net.slice{slice_of(n)}.{n}.{kind}"] = t
            ref[f"net.layers.{n}.{kind}"] = t
    tv.update({"classifier.0.weight": torch.zeros(8, 8), "classifier.0.bias": torch.zeros(8)})      # what a whole vgg16 state dict also holds
    pk.update({"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)})
    ref.update({"net.mean": torch.zeros(1, 3, 1, 1), "net.std": torch.ones(1, 3, 1, 1)})
    for k, w in enumerate(lin4):
        pk[f"lin{k}.model.1.weight"] = w
        pk[f"lins.{k}.model.1.weight"] = w
        ref[f"lin.{k}.1.weight"] = w
    lin_pk = {f"lin{k}.model.1.weight": w for k, w in enumerate(lin4)}
    return (conv_w, conv_b, lin_w), tv, pk, ref, lin_pk


def test_loader_key_layouts_and_errors(tmp_path):
    from materialrefgs_amd.lpips import LPIPS
    (conv_w, conv_b, lin_w), tv, pk, ref, lin_pk = _layouts()
    bare = {k[len("features."):]: v for k, v in tv.items() if k.startswith("features.")}
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin_pk.items()}      # the keys behind the reference's get_state_dict
    torch.save(tv, tmp_path / "vgg16.pth")
    torch.save(lin_pk, tmp_path / "vgg.pth")
    nets = [LPIPS.from_tensors(conv_w, conv_b, lin_w), LPIPS.load(tv, lin_pk), LPIPS.load(bare, renamed), LPIPS.load(pk), LPIPS.load(ref),
            LPIPS.load(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"))]
    for net in nets[1:]:
        for a, b in zip(nets[0].conv_w + nets[0].conv_b + nets[0].lin_w, net.conv_w + net.conv_b + net.lin_w):
            assert a.shape == b.shape and torch.equal(a, b)
    with pytest.raises(ValueError, match=r"no lin vector of level 0.*found in vgg: features\.0\.weight \(64, 3, 3, 3\)"):
        LPIPS.load(tv)
    missing = dict(tv)
    del missing["features.17.bias"]
    with pytest.raises(ValueError, match=r"no bias of convolution features\.17"):
        LPIPS.load(missing, lin_pk)
    misshaped = dict(tv)
    misshaped["features.5.weight"] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(ValueError, match=r"features\.5\.weight \(128, 32, 3, 3\)"):
        LPIPS.load(misshaped, lin_pk)
    swapped = dict(lin_pk)
    swapped["lin1.model.1.weight"] = lin_pk["lin2.model.1.weight"]
    with pytest.raises(ValueError, match=r"level 1 needs \(1, 128, 1, 1\)"):
        LPIPS.load(tv, swapped)
    for net_type in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match="vgg"):
            LPIPS.load(tv, lin_pk, net_type=net_type)
    with pytest.raises(FileNotFoundError):
        LPIPS.load(str(tmp_path / "absent.pth"))
    with pytest.raises(ValueError):
        LPIPS.from_tensors(conv_w[:12], conv_b, lin_w)
    a, b = LPIPS.random(5), LPIPS.random(5)
    assert all(torch.equal(s, t) for s, t in zip(a.conv_w + a.lin_w, b.conv_w + b.lin_w)) and all(float(w.min()) >= 0 for w in a.lin_w)
    with pytest.raises(RuntimeError, match="device tensor"):
        a(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="H, W >= 16"):
        a(torch.zeros(1, 3, 15, 16), torch.zeros(1, 3, 15, 16))


@pytest.mark.parametrize("H,W", NET_SIZES)
def test_decision_machinery_with_the_fp32_reading(H, W):
    """The literal fp32 torch reading stands in for the kernel: its decisions are read from its ReLU outputs and fed to the float64
    statement.  Every decision that differs from the pure float64 run lies inside the margin of the GPU test (2e-5 of the layer's RMS),
    no more than 1 in 10 000 differ, and under the fp32 run's decisions its gradient is within 1e-4 of the statement's largest element
    (measured here: total within 1.6e-7, gradient within 1.3e-6)."""
    w32 = ls.random_weights(SEED)
    w64, wf = ls.cast_weights(w32), ls.cast_weights(w32, torch.float32)
    g = torch.Generator().manual_seed(1000 * H + W)
    x = (torch.rand(3, H, W, generator=g) * 2 - 1).float()
    y = (torch.rand(3, H, W, generator=g) * 2 - 1).float()
    with torch.no_grad():
        pure = ls.lpips(w64, x.double(), y.double())
    xf = x.clone().requires_grad_(True)
    low = ls.lpips(wf, xf, y)
    low.total.backward()
    dec = ls.decisions_of([a.detach() for a in low.x.acts])
    n_diff, n_total, margin = ls.differing_decisions(pure.x, dec)
    x64 = x.double().requires_grad_(True)
    fed = ls.lpips(w64, x64, y.double(), decisions=dec)
    fed.total.backward()
    figs = {"differ": f"{n_diff} of {n_total} ({n_diff / n_total:.2e})", "margin": margin,
            "total": abs(float(low.total) - float(pure.total)) / float(pure.total),
            "fed_total": abs(float(fed.total) - float(pure.total)) / float(pure.total),
            "g_x": float((xf.grad.double() - x64.grad).abs().max() / x64.grad.abs().max())}
    print(f"{H}x{W}: {figs}")
    assert margin < 2e-5 and n_diff * 10000 <= n_total, figs
    assert figs["total"] <= 1e-5 and figs["fed_total"] <= 1e-5 and figs["g_x"] <= 1e-4, figs
    # given decisions are used as given: flipping one open gate changes the value
    flipped = SimpleNamespace(gates=[t.clone() for t in dec.gates], winners=dec.winners)
    idx = tuple(int(v) for v in torch.nonzero(flipped.gates[12])[0])
    flipped.gates[12][idx] = False
    with torch.no_grad():
        assert float(ls.lpips(w64, x.double(), y.double(), decisions=flipped).total) != float(fed.total)


def test_environment_variable_and_shim(monkeypatch, tmp_path):
    """Unset: today's behaviour (the NotImplementedError that names set_lpips_fn, unless the `lpips` package exists).  A path that does not
    exist raises an error naming the variable, from lpips_loss and from check_loss_config.  The shim imports and serves only vgg."""
    from materialrefgs_amd import losses
    import lpipsPyTorch
    assert callable(lpipsPyTorch.lpips) and lpipsPyTorch.LPIPS
    try:
        import lpips  # noqa: F401
        have = True
    except ImportError:
        have = False
    x = torch.zeros(1, 3, 16, 16)
    opt = SimpleNamespace(use_perceptual_loss=True, perceptual_loss_start_iter=18000)
    monkeypatch.delenv("MRGS_LPIPS_WEIGHTS", raising=False)
    assert losses._LPIPS_FN is None
    if not have:
        with pytest.raises(NotImplementedError, match="set_lpips_fn"):
            losses.lpips_loss(x, x)
        with pytest.raises(NotImplementedError, match="no-use_perceptual_loss"):
            losses.check_loss_config(opt)
    with pytest.raises(NotImplementedError, match="MRGS_LPIPS_WEIGHTS"):
        lpipsPyTorch.lpips(x, x, net_type="vgg")
    monkeypatch.setenv("MRGS_LPIPS_WEIGHTS", str(tmp_path / "absent.pth"))
    with pytest.raises(FileNotFoundError, match="MRGS_LPIPS_WEIGHTS"):
        losses.lpips_loss(x, x)
    with pytest.raises(FileNotFoundError, match="MRGS_LPIPS_WEIGHTS"):
        losses.check_loss_config(opt)
    with pytest.raises(FileNotFoundError, match="MRGS_LPIPS_WEIGHTS"):
        lpipsPyTorch.lpips(x, x)
    with pytest.raises(NotImplementedError, match="vgg"):
        lpipsPyTorch.lpips(x, x, net_type="alex")
    # a registered callable still wins over the variable
    losses.set_lpips_fn(lambda a, b: (a - b).abs().mean((1, 2, 3)))
    try:
        assert float(losses.lpips_loss(x, x + 0.5)) == 1.0       # |2 x 0.5|: the callable ran, on images scaled to [-1, 1]
        losses.check_loss_config(opt)
    finally:
        losses.set_lpips_fn(None)
    # a file written from LPIPS.random is loaded (the network itself needs the device: tests/test_lpips_gpu.py)
    _, tv, _, _, lin_pk = _layouts()
    torch.save(tv, tmp_path / "vgg16.pth")
    torch.save(lin_pk, tmp_path / "vgg.pth")
    monkeypatch.setenv("MRGS_LPIPS_WEIGHTS", f"{tmp_path / 'vgg16.pth'}:{tmp_path / 'vgg.pth'}")
    losses.check_loss_config(opt)
    with pytest.raises(RuntimeError, match="device tensor"):
        losses.lpips_loss(x, x)
