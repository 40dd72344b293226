"""The native LPIPS (VGG16) term (csrc/mrgs_lpips.hip behind materialrefgs_amd.lpips.LPIPS, losses.lpips_loss and the lpipsPyTorch shim) on
the GPU against the float64 statement of tests/lpips_statement.py.

Per layer (mrgs_lpips_debug_conv): all eight (Cin, Cout) pairs, forward and backward-to-data, batch 2, at SIZES.  Inputs are drawn in
fp32, so nothing is rounded on entry.  Bound: an output is a sum of K = 9 x (input channels of the launch) products by fmaf chains (one
per chunk of 144, the chunk sums added in order: never more roundings on a path than one chain of K) plus a bias, so it lies within 1.01 (K + 2) 2^-24 sum |a| |w| (+ |b|) of the exact value, the sum taken by a float64 convolution of absolute values;
no element is excluded.  With `add` one more rounding and |add| joins the sum.
Head alone (mrgs_lpips_debug_head): level terms within 1e-5 relative, gradients within 1e-4 of the map's largest element, all-zero
pixels give 0 and gradient 0.
Whole network with LPIPS.random at NET_SIZES: total and level terms within 1e-5 relative of the pure float64 run; every stored ReLU output
within the chain bound E_l = g_l conv(|a_l-1| + E_l-1, |w_l|) + conv(E_l-1, |w_l|) (g_l the per-layer bound above; the first term is the
layer's own rounding on the values it really read, the second the error it inherits; ReLU is 1-Lipschitz and the 2 x 2 maximum maps E to
its window maximum; E of the z-scored input = 4 x 2^-24 (|a| + |shift|) / scale for the transform's roundings).  Gradient: the statement
run with the kernel's decisions, g_x within 1e-4 of its largest element, no pixel excluded; every decision that differs from the pure
float64 run has a margin below 2e-5 there and no more than 1 in 10 000 differ.
The bars 1e-5 / 1e-4 are those of the sibling loss terms (test_prior_terms.py, test_smooth_terms.py).
Measured on an MI355X (2026-10-20): layers at most 0.13 of their bound (3-64 forward; under 0.01 for the matrix-pipe pairs); head terms
3.1e-9 - 4.4e-8, head gradients 2.0e-7; network total 2.6 - 5.4e-8, level terms 1.9 - 7.5e-7, stored ReLU outputs at most 0.13 of the chain
bound, g_x 6.8e-7 - 1.1e-6, no decision of 76 800 - 921 600 differing from the float64 run.
"""
import ctypes
import functools
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lpips_statement as ls  # noqa: E402

pytestmark = pytest.mark.gpu


def _constant(name):
    src = open(os.path.join(ROOT, "materialrefgs_amd", "csrc", "mrgs_lpips.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


T = _constant("LPIPS_TILE")
HEAD_MAX_BLOCKS = _constant("HEAD_MAX_BLOCKS")
# 1 x 1 and 2 x 3: smaller than a halo; one pixel more than a tile and two tiles plus one, both ways; an odd size with partial tiles
SIZES = ((1, 1), (2, 3), (T + 1, T + 1), (2 * T + 1, 2 * T + 1), (7, 21))
PAIRS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512))
NET_SIZES = ((16, 16), (19, 22), (33, 40), (64, 48))
SEED = 0
U = 2.0 ** -24


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _debug_conv(dev, x, w, bias, backward, relu=0, add=None, gate=None):
    """x [N,C,H,W] fp32 on the host -> the launch's output [N,C',H,W] on the host"""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    co, ci = w.shape[:2]
    c_in, c_out = (co, ci) if backward else (ci, co)
    N, _, H, W = x.shape
    planes_in, planes_out = c_in == 3, c_out == 3
    xin = (x.contiguous() if planes_in else _nhwc(x)).to(dev)
    out = torch.full((N, c_out, H, W) if planes_out else (N, H, W, c_out), float("nan"), device=dev)
    wd = w.contiguous().to(dev)
    ws = torch.empty(36 * ci * co, dtype=torch.uint8, device=dev)
    cfg = _lib.MrgsLpipsConvConfig(H, W, ci, co, N, int(backward), int(relu), 0, 1.0, 0.0)
    dv = lambda t: None if t is None else _nhwc(t).to(dev)
    held = (dv(add), dv(gate), None if bias is None else bias.to(dev))
    p = _lib.ptr
    _lib.check(L.mrgs_lpips_debug_conv(ctypes.byref(cfg), p(xin), p(wd), p(held[2]), p(held[0]), p(held[1]), p(out), p(ws), ws.numel(),
                                       _lib.stream_ptr(dev)))
    out = out.cpu()
    return out if planes_out else _nchw(out)


def _conv_case(ci, co, backward, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
    b = None if backward else 0.1 * torch.randn(co, generator=g)
    x = torch.randn(2, co if backward else ci, H, W, generator=g)
    if backward:
        want = F.conv_transpose2d(x.double(), w.double(), padding=1)
        scale = F.conv_transpose2d(x.double().abs(), w.double().abs(), padding=1)
    else:
        want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        scale = ls.conv_abs_sum(x, w, b)
    return x, w, b, want, scale


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("ci,co", PAIRS)
def test_every_layer_shape_within_the_fmaf_chain_bound(gpu_device, ci, co, backward):
    worst = 0.0
    for k, (H, W) in enumerate(SIZES):
        x, w, b, want, scale = _conv_case(ci, co, backward, H, W, 100 + k)
        got = _debug_conv(gpu_device, x, w, b, backward)
        K = 9 * x.shape[1]
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), (H, W)
        ratio = float(((got.double() - want).abs() / (ls.conv_bound(K) * scale)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{ci}->{co} backward={backward} {H}x{W}: error / bound = {ratio}"
    print(f"{ci}->{co} backward={backward}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("ci,co,backward", [(64, 128, 0), (128, 64 * 2, 1), (256, 512, 1)])
def test_add_relu_and_a_gate_from_a_given_tensor(gpu_device, ci, co, backward):
    """+ add, ReLU, then exactly 0 where the given gate tensor is <= 0"""
    H, W = T + 3, 2 * T + 1
    x, w, b, want, scale = _conv_case(ci, co, backward, H, W, 7)
    g = torch.Generator().manual_seed(8)
    add = torch.randn(want.shape, generator=g)
    gate = torch.randn(want.shape, generator=g)
    gate[:, :, 0, :] = 0.0                                # a zero gate is off, as a ReLU output of exactly 0 is
    K = 9 * x.shape[1]
    for relu in (0, 1):
        got = _debug_conv(gpu_device, x, w, b, backward, relu=relu, add=add, gate=gate)
        ref = want + add.double()
        if relu:
            ref = ref.clamp_min(0)
        off = gate <= 0
        assert bool((got[off] == 0).all()) and bool(off.any())
        bound = 1.01 * (K + 3) * U * (scale + add.double().abs())
        assert bool(((got.double() - ref).abs() <= bound)[~off].all())
        if relu:
            assert bool((got >= 0).all())


def _pool(dev, a, g=None):
    """a [C,H,W] host; g [C,H//2,W//2] or None -> host result in the same layout"""
    from materialrefgs_amd import _lib
    C, H, W = a.shape
    ad = a.permute(1, 2, 0).contiguous().to(dev)
    gd = None if g is None else g.permute(1, 2, 0).contiguous().to(dev)
    out = torch.full((H, W, C) if g is not None else (H // 2, W // 2, C), float("nan"), device=dev)
    _lib.check(_lib.lib().mrgs_lpips_debug_pool(H, W, C, _lib.ptr(ad), _lib.ptr(gd), _lib.ptr(out), _lib.stream_ptr(dev)))
    return out.cpu().permute(2, 0, 1)


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (T + 1, 2 * T + 3), (3, 2)])
def test_pool_forward_and_backward_odd_sizes_and_ties(gpu_device, H, W):
    """Values from {0, 1, 2}: most windows hold a tie.  The gradient of a window goes to its FIRST maximum in row-major order; a last odd
    row or column gets 0."""
    g = torch.Generator().manual_seed(H * 100 + W)
    C = 64
    a = torch.randint(0, 3, (C, H, W), generator=g).float()
    a[0, :2, :2] = 1.0                                    # a window of four equal entries
    if H >= 2:
        want = F.max_pool2d(a[None], 2)[0]
        assert torch.equal(_pool(gpu_device, a), want)
    gp = torch.randn(C, H // 2, W // 2, generator=g)
    got = _pool(gpu_device, a, gp)
    want = torch.zeros(C, H, W)
    if H >= 2:
        k = ls.first_max(ls.windows_of(a))
        for j in range(4):
            want[:, j // 2:H // 2 * 2:2, j % 2:W // 2 * 2:2] = torch.where(k == j, gp, torch.zeros_like(gp))
        assert float(got[0, 0, 0]) == float(gp[0, 0, 0]) and float(got[0, 0, 1]) == 0 and float(got[0, 1, 0]) == 0 and float(got[0, 1, 1]) == 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("C,P", [(64, 4 * HEAD_MAX_BLOCKS + 37), (128, 301), (256, 77), (512, 50), (512, 1)])
def test_head_alone(gpu_device, C, P):
    """P > 4 HEAD_MAX_BLOCKS: the workgroups stride over the pixels and the finalize step makes more than one pass over the rows."""
    from materialrefgs_amd import _lib
    dev = gpu_device
    g = torch.Generator().manual_seed(C + P)
    fx, fy = torch.rand(P, C, generator=g) * (torch.rand(P, C, generator=g) > 0.4), torch.rand(P, C, generator=g) * (torch.rand(P, C, generator=g) > 0.4)
    zero = []
    if P > 8:
        fx[3] = 0; fy[5] = 0; fx[7] = 0; fy[7] = 0
        zero = [3, 5, 7]
    w = torch.rand(C, generator=g) * (2.0 / C)
    up = 0.7
    x64 = fx.double().requires_grad_(True)
    term = ls.head_level(x64.t()[:, :, None], fy.double().t()[:, :, None], w.double())
    (up * term).backward()
    ws = torch.empty(HEAD_MAX_BLOCKS * 16, dtype=torch.uint8, device=dev)
    out, gout = torch.empty(1, device=dev), torch.full((P, C), float("nan"), device=dev)
    fxd, fyd, wd, gd = fx.to(dev), fy.to(dev), w.to(dev), torch.full((1,), up, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().mrgs_lpips_debug_head(P, C, p(fxd), p(fyd), p(wd), p(ws), ws.numel(), p(out), p(gd), p(gout), _lib.stream_ptr(dev)))
    rel = abs(float(out) - float(term)) / float(term) if float(term) > 0 else abs(float(out))
    gerr = float((gout.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max().clamp_min(1e-300))
    print(f"head C={C} P={P}: term rel {rel:.2e}, gradient {gerr:.2e} of the largest element")
    assert rel <= 1e-5 and gerr <= 1e-4
    for i in zero:
        assert bool((gout[i] == 0).all())
    if P == 1:
        return
    # the zero pixels contribute 0: the term of the other pixels alone, rescaled to the same count
    if zero:
        keep = [i for i in range(P) if i not in zero]
        alone = ls.head_level(fx[keep].double().t()[:, :, None], fy[keep].double().t()[:, :, None], w.double()) * len(keep) / P
        assert abs(float(alone) - float(term)) <= 1e-12 * float(term)


# ---- the whole network ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights():
    return ls.cast_weights(ls.random_weights(SEED))


@functools.lru_cache(maxsize=None)
def _images(H, W, scale=2.0, offset=-1.0):
    g = torch.Generator().manual_seed(1000 * H + W)
    return (torch.rand(3, H, W, generator=g) * scale + offset).float(), (torch.rand(3, H, W, generator=g) * scale + offset).float()


@functools.lru_cache(maxsize=None)
def _pure(H, W, scale=2.0, offset=-1.0):
    """The pure float64 run, once per size (its gradient is taken under the kernel's decisions, per test)."""
    x, y = _images(H, W, scale, offset)
    with torch.no_grad():
        return ls.lpips(_weights(), x.double(), y.double())


@functools.lru_cache(maxsize=None)
def _net():
    from materialrefgs_amd.lpips import LPIPS
    return LPIPS.random(SEED)


def _chain_bounds(ref, x):
    """E_l of the module docstring for the 13 ReLU outputs of the float64 record `ref` of image x."""
    conv_w = _weights()[0]
    a = (x.double() - torch.tensor(ls.SHIFT).double()[:, None, None]) / torch.tensor(ls.SCALE).double()[:, None, None]
    E = 4 * U * (x.double().abs() + torch.tensor(ls.SHIFT).double().abs()[:, None, None]) / torch.tensor(ls.SCALE).double()[:, None, None]
    out = []
    for i in range(13):
        if i > 0 and ls.CONV_STAGE[i] != ls.CONV_STAGE[i - 1]:
            a, E = F.max_pool2d(a[None], 2)[0], F.max_pool2d(E[None], 2)[0]
        wabs = conv_w[i].abs()
        own = ls.conv_bound(9 * conv_w[i].shape[1]) * (F.conv2d((a.abs() + E)[None], wabs, _weights()[1][i].abs(), padding=1)[0])
        E = own + F.conv2d(E[None], wabs, padding=1)[0]
        a = ref.acts[i]
        out.append(E)
    return out


@pytest.mark.parametrize("H,W", NET_SIZES)
def test_whole_network_against_the_statement(gpu_device, H, W):
    dev = gpu_device
    net, ref = _net(), _pure(H, W)
    x, y = _images(H, W)
    xd = x.to(dev)[None].requires_grad_(True)
    out = net(xd, y.to(dev)[None])
    assert out.shape == (1, 1, 1, 1) and net.level_terms.shape == (1, 5)
    figs = {"total": abs(float(out) - float(ref.total)) / float(ref.total),
            "levels": float(((net.level_terms[0].cpu().double() - ref.terms).abs() / ref.terms).max())}
    xs, ys = net.stored_activations()
    xs = [a.permute(2, 0, 1).cpu() for a in xs]
    ys = [a.permute(2, 0, 1).cpu() for a in ys]
    out.sum().backward()
    # every stored ReLU output inside the chain bound
    figs["acts"] = max(float(((a.double() - r).abs() / E).max()) for a, r, E in zip(xs, ref.x.acts, _chain_bounds(ref.x, x)))
    figs["y_taps"] = max(float(((a.double() - ref.y.acts[c]).abs() / E[c]).max()) for a, c, E in
                         zip(ys, ls.TAP_CONV, [_chain_bounds(ref.y, y)] * 5))
    # the gradient under the kernel's decisions
    dec = ls.decisions_of(xs)
    n_diff, n_total, margin = ls.differing_decisions(ref.x, dec)
    x64 = x.double().requires_grad_(True)
    ls.lpips(_weights(), x64, y.double(), decisions=dec).total.backward()
    figs["g_x"] = float((xd.grad[0].cpu().double() - x64.grad).abs().max() / x64.grad.abs().max())
    figs["decisions"] = f"{n_diff} of {n_total} differ, worst margin {margin:.2e}"
    print(f"{H}x{W}: {figs}")
    assert figs["total"] <= 1e-5 and figs["levels"] <= 1e-5, figs
    assert figs["acts"] <= 1.0 and figs["y_taps"] <= 1.0, figs
    assert margin < 2e-5 and n_diff * 10000 <= n_total, figs
    assert figs["g_x"] <= 1e-4, figs


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------------
def test_no_grad_repeat_retain_and_no_host_read(gpu_device):
    dev = gpu_device
    net = _net()
    H, W = 19, 22
    x, y = _images(H, W)
    xd, yd = x.to(dev)[None], y.to(dev)[None]
    with torch.no_grad():
        v0 = net(xd, yd)
    small = net.last_workspace_bytes
    runs = []
    for _ in range(2):
        leaf = xd.clone().requires_grad_(True)
        v = net(leaf, yd)
        big = net.last_workspace_bytes
        v.sum().backward(retain_graph=True)
        g1 = leaf.grad.clone()
        leaf.grad = None
        v.sum().backward()                                # a second backward over the retained graph
        assert torch.equal(g1, leaf.grad)
        runs.append((v.detach().clone(), g1))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # the same bits twice
    assert torch.equal(v0, runs[0][0])                    # the no-grad call: the small workspace, the same value
    from materialrefgs_amd import _lib
    assert big == _lib.lib().mrgs_lpips_ws_bytes(H, W, 1) and _lib.lib().mrgs_lpips_ws_bytes(H, W, 0) < big
    assert small == _lib.lib().mrgs_lpips_ws_bytes(H, W, 0)
    with pytest.raises(ValueError, match="requires grad"):
        net(xd, yd.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="device tensor"):
        net(x[None], y[None])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        leaf = xd.clone().requires_grad_(True)
        net(leaf, yd).sum().backward()
        with torch.no_grad():
            net(xd, yd)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(leaf.grad, runs[0][1])


def test_calculate_loss_with_a_native_network_registered(gpu_device):
    """iteration > perceptual_loss_start_iter: tb_dict["perceptual_loss"] is the statement's value on the images scaled to [-1, 1], and
    lambda times its gradient reaches render_pkg["render"] (compared under the kernel's decisions)."""
    from materialrefgs_amd import losses
    dev = gpu_device
    H, W = 33, 40
    x, y = _images(H, W, 1.0, 0.0)                        # [0, 1] images, as a render and a ground truth are
    net = _net()
    cam = SimpleNamespace(original_image=y.to(dev))
    pc = SimpleNamespace(get_xyz=torch.zeros(5, 3))
    lam = 0.1

    def run(use):
        pkg = {"render": x.to(dev).requires_grad_(True), "rend_normal": torch.zeros(3, H, W, device=dev), "surf_normal": torch.zeros(3, H, W, device=dev),
               "surf_depth": torch.zeros(1, H, W, device=dev), "rend_dist": torch.zeros(1, H, W, device=dev)}
        opt = SimpleNamespace(lambda_dssim=0.2, lambda_normal_render_depth=0.0, normal_loss_start=0, lambda_dist=0.0, dist_loss_start=0,
                              lambda_normal_smooth=0.0, lambda_depth_smooth=0.0, normal_smooth_from_iter=0, normal_smooth_until_iter=0,
                              use_perceptual_loss=use, lambda_perceptual_loss=lam, perceptual_loss_start_iter=18000)
        loss, tb = losses.calculate_loss(cam, pc, pkg, opt, 18001)
        dec = ls.decisions_of([a.permute(2, 0, 1).cpu() for a in net.stored_activations()[0]]) if use else None
        loss.backward()
        return loss.detach(), tb, pkg["render"].grad, dec

    losses.set_lpips_fn(net)
    try:
        loss1, tb1, g1, dec = run(True)
        loss0, tb0, g0, _ = run(False)
    finally:
        losses.set_lpips_fn(None)
    assert "perceptual_loss" not in tb0
    x64 = x.double().requires_grad_(True)
    ref = ls.lpips(_weights(), x64 * 2.0 - 1.0, y.double() * 2.0 - 1.0)
    assert abs(float(tb1["perceptual_loss"]) - float(ref.total)) <= 1e-5 * float(ref.total)
    assert abs((float(loss1) - float(loss0)) - lam * float(ref.total)) <= 1e-5 * float(loss1)
    x64d = x.double().requires_grad_(True)
    ls.lpips(_weights(), x64d * 2.0 - 1.0, y.double() * 2.0 - 1.0, decisions=dec).total.backward()
    err = float(((g1 - g0).cpu().double() - lam * x64d.grad).abs().max() / (lam * x64d.grad.abs().max()))
    print(f"calculate_loss: gradient of the perceptual term {err:.2e} of its largest element")
    assert err <= 1e-4      # the gradient bar of the network test; the difference of two fp32 maps adds roundings of 6e-8 of the other terms' gradients


def test_shim_and_environment_variable(gpu_device, monkeypatch, tmp_path):
    """lpipsPyTorch.lpips(x, y) hands the images over unscaled; MRGS_LPIPS_WEIGHTS names a file written from LPIPS.random and is picked up
    by the shim and by losses.lpips_loss."""
    import lpipsPyTorch
    from materialrefgs_amd import losses
    dev = gpu_device
    H, W = 19, 22
    x, y = _images(H, W, 1.0, 0.0)
    conv_w, conv_b, lin_w = ls.random_weights(SEED)
    sd = {}
    for i, n in enumerate(ls_index()):
        sd[f"features.{n}.weight"], sd[f"features.{n}.bias"] = conv_w[i], conv_b[i]
    lin = {f"lin{k}.model.1.weight": w.reshape(1, -1, 1, 1) for k, w in enumerate(lin_w)}
    torch.save(sd, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    monkeypatch.setenv("MRGS_LPIPS_WEIGHTS", f"{tmp_path / 'vgg16.pth'}:{tmp_path / 'vgg.pth'}")
    with torch.no_grad():
        ref = ls.lpips(_weights(), x.double(), y.double())
        ref11 = ls.lpips(_weights(), x.double() * 2 - 1, y.double() * 2 - 1)
    got = lpipsPyTorch.lpips(x.to(dev)[None], y.to(dev)[None], net_type="vgg")
    assert got.shape == (1, 1, 1, 1) and abs(float(got) - float(ref.total)) <= 1e-5 * float(ref.total)
    assert losses._LPIPS_FN is None
    got = losses.lpips_loss(x.to(dev)[None], y.to(dev)[None])
    assert abs(float(got) - float(ref11.total)) <= 1e-5 * float(ref11.total)
    losses.check_loss_config(SimpleNamespace(use_perceptual_loss=True, perceptual_loss_start_iter=18000))
    with pytest.raises(NotImplementedError):
        lpipsPyTorch.lpips(x.to(dev)[None], y.to(dev)[None], net_type="alex")


def ls_index():
    from materialrefgs_amd.lpips import CONV_INDEX
    return CONV_INDEX
