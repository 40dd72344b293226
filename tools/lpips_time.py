"""Times the native LPIPS (VGG16) term (materialrefgs_amd.lpips.LPIPS on csrc/mrgs_lpips.hip; allocation of the workspace included):
forward alone (no-grad call) and forward plus backward to x, at 800 x 800 and 1600 x 1600, beside the fp32 torch form of the same network
on the same GPU in the same run (an F.conv2d / relu / max_pool2d chain with the same LPIPS.random weights and the same head, TF32 off,
autograd to x only).  The window is a host clock between two device synchronisations around a batch of BATCH calls, the two forms
alternate, the first pair is the warm-up, the minimum and every run are printed, and both forms must agree to 1e-4 relative: asserted.
The torch form is a yardstick only: it cannot be a product path here.

Per-layer times come from a kernel trace, taken in a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --output-format csv -d OUT -o lpips -- python tools/lpips_time.py --once 800
    python tools/lpips_time.py --layers OUT/.../lpips_kernel_trace.csv 800
`--once` runs one warm-up and one forward plus backward; `--layers` reads the trace's last 26 convolution dispatches (13 forward with
both images, 13 backward with one) and prints each one's time and achieved TFLOP/s (2 x 9 Cin Cout products per pixel and image).
Developer tool."""
import csv
import os
import re
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd.lpips import CONV_CHANNELS, CONV_STAGE, LPIPS, SCALE, SHIFT, TAP_CONV  # noqa: E402

BATCH = 5
SEED = 0


def conv_flops(H, W, i, images):
    ci, co = CONV_CHANNELS[i]
    return 2.0 * 9 * ci * co * (H >> CONV_STAGE[i]) * (W >> CONV_STAGE[i]) * images


def torch_form(net, dev):
    cw, cb, lw = ([t.to(dev) for t in ts] for ts in (net.conv_w, net.conv_b, net.lin_w))
    shift, scale = torch.tensor(SHIFT, device=dev)[None, :, None, None], torch.tensor(SCALE, device=dev)[None, :, None, None]

    def feats(a):
        a = (a - shift) / scale
        taps = []
        for i in range(13):
            if i > 0 and CONV_STAGE[i] != CONV_STAGE[i - 1]:
                a = F.max_pool2d(a, 2)
            a = F.relu(F.conv2d(a, cw[i], cb[i], padding=1))
            if i in TAP_CONV:
                taps.append(a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10))
        return taps

    def run(x, y):
        with torch.no_grad():
            fy = feats(y)
        return sum((w[None, :, None, None] * (u - v) ** 2).sum(1).mean() for u, v, w in zip(feats(x), fy, lw))
    return run


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / BATCH, out


def images(S, dev):
    g = torch.Generator(device=dev).manual_seed(S)
    return torch.rand(1, 3, S, S, generator=g, device=dev) * 2 - 1, torch.rand(1, 3, S, S, generator=g, device=dev) * 2 - 1


def step(fn, x, y):
    leaf = x.clone().requires_grad_(True)
    v = fn(leaf, y).sum()
    v.backward()
    return v.detach(), leaf.grad


def layers(path, S):
    rows = [r for r in csv.DictReader(open(path)) if "lpips_conv" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-26:]
    assert len(rows) == 26, f"{len(rows)} convolution dispatches in {path}"
    order = [(i, 2) for i in range(13)] + [(i, 1) for i in range(12, -1, -1)]
    total = 0.0
    for r, (i, n) in zip(rows, order):
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        name = re.search(r"lpips_\w+", r["Kernel_Name"]).group(0)
        total += ms
        print(f"{'forward ' if n == 2 else 'backward'} conv {i + 1:2d} {CONV_CHANNELS[i][0]:3d}->{CONV_CHANNELS[i][1]:3d} stage {CONV_STAGE[i]}: {ms:8.3f} ms, "
              f"{conv_flops(S, S, i, n) / ms * 1e-9:6.1f} TFLOP/s  ({name})")
    print(f"26 convolution launches: {total:.3f} ms")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--layers":
        return layers(args[1], int(args[2]))
    once = bool(args) and args[0] == "--once"
    sizes = [int(a) for a in args if not a.startswith("--")] or [800, 1600]
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = LPIPS.random(SEED)
    ref = torch_form(net, dev)
    fmt = lambda xs: ", ".join(f"{x:.2f}" for x in xs)
    for S in sizes:
        x, y = images(S, dev)
        if once:
            step(net, x, y)
            torch.cuda.synchronize()
            step(net, x, y)
            torch.cuda.synchronize()
            continue
        runs = {k: [] for k in ("native fwd", "torch fwd", "native fwd+bwd", "torch fwd+bwd")}
        for rep in range(4):                              # alternating; the first round is the warm-up
            with torch.no_grad():
                runs["native fwd"].append(host_ms(lambda: [net(x, y) for _ in range(BATCH)])[0])
                runs["torch fwd"].append(host_ms(lambda: [ref(x, y) for _ in range(BATCH)])[0])
            ms, out_n = host_ms(lambda: [step(net, x, y) for _ in range(BATCH)])
            runs["native fwd+bwd"].append(ms)
            ms, out_t = host_ms(lambda: [step(ref, x, y) for _ in range(BATCH)])
            runs["torch fwd+bwd"].append(ms)
        (vn, gn), (vt, gt) = out_n[-1], out_t[-1]
        rel, grel = abs(float(vn) - float(vt)) / float(vt), float((gn - gt).abs().max() / gt.abs().max())
        far = float(((gn - gt).abs() > 1e-4 * gt.abs().max()).float().mean())
        assert rel <= 1e-4, (float(vn), float(vt))
        fwd = sum(conv_flops(S, S, i, 2) for i in range(13))
        both = fwd + sum(conv_flops(S, S, i, 1) for i in range(13))
        for k, v in runs.items():
            v = v[1:]
            fl = both if "bwd" in k else fwd
            print(f"{S} x {S}: {k:15s} {min(v):8.2f} ms a call (runs {fmt(v)}), {fl * 1e-12:.3f} TFLOP of convolution = {fl / min(v) * 1e-9:.1f} TFLOP/s "
                  f"end to end", flush=True)
        print(f"{S} x {S}: native against torch: value {rel:.1e} relative, gradient {grel:.1e} of its largest element at worst, "
              f"{far:.1e} of its elements further than 1e-4 (fp32 both; a ReLU gate or a pooling winner that falls the other way moves a patch)",
              flush=True)


if __name__ == "__main__":
    main()
