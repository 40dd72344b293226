"""Times the masked optimizer step (mrgs_adam_step_rows, csrc/mrgs_optim.hip) against the dense one (mrgs_adam_step) at P = 300 000 for
both parameter sets: the 111 floats per surfel that render_surfel trains and the 275 of tests/test_optim.py::test_adam_full_size_properties.
Masks: all ones; the `visibility_filter` of one orbit_camera view of the bench scene (synthetic.make_surfel_model at the C3 settings) and
a random mask of its density; the rows that view's backward left a non-zero gradient in (what dist.TouchedRowsExchange masks) and a random
mask of that density; 10 %; all zeros.

Method: both entry points are called straight through ctypes on prebuilt tables (no optimizer bookkeeping in the window); a window is
CALLS back-to-back calls between two device events; after a warm-up of every (set, mask) the dense and the masked window alternate in one
process, PAIRS times, and every figure is printed as median [min .. max] microseconds per call.

The byte model (model_bytes below) is printed beside each figure as the time the dense kernel's own measured rate predicts:
  * 28 B per element (16 read, 12 written) of every 16-byte piece that holds an element of a visible row, 0 B for any other piece;
  * the mask bytes once per tensor;
  * and, as a second figure, the same with a piece counted when its 128-byte line holds any visible element: what the memory system
    moves when loads and stores are whole lines.  The tensors of 1 to 4 floats per row save traffic only where a whole line is invisible
    (32 to 8 consecutive rows), which a scattered mask of ~50 % almost never offers: the saving to expect sits in the 45- and 160-float tensors.
Developer tool; needs a GPU."""
import ctypes
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import _lib  # noqa: E402

P = 300000
SETS = {
    "111 floats (render_surfel)": [3, 2, 4, 1, 3, 45, 1, 1, 3, 3, 45],
    "275 floats (full model)": [3, 3, 45, 1, 2, 4, 1, 3, 3, 1, 1, 3, 45, 160],
}
CALLS, PAIRS = 20, 15


def model_bytes(widths, vis, n_masks=1, line_bytes=16):
    """Bytes the masked step moves for tensors [len(vis), w], w in widths: 28 per element of every `line_bytes` piece of a tensor that holds an
    element of a visible row, plus the mask once per tensor."""
    vis = np.asarray(vis) != 0
    per = line_bytes // 4
    total = 0
    for w in widths:
        el = np.repeat(vis, w)
        n = el.size
        pad = (-n) % per
        pieces = np.concatenate([el, np.zeros(pad, dtype=bool)]).reshape(-1, per).any(axis=1)
        live = int(pieces.sum()) * per - (pad if pieces[-1] else 0)
        total += 28 * live + n_masks * vis.size
    return total


def dense_bytes(widths, rows):
    return 28 * rows * sum(widths)


def scene_masks(dev):
    """View 0 of the bench scene (bench.py's C3 settings: P = 300 000, 800 x 800, radius_px = 7): its `visibility_filter` (radii > 0: every
    surfel in the frustum, occluded or not), and the rows its backward left a non-zero gradient in (the mask dist.TouchedRowsExchange builds:
    the surfels that were blended into a pixel), with bench.py's upstream gradients."""
    from materialrefgs_amd.renderer import render_surfel
    from materialrefgs_amd.synthetic import make_surfel_model, orbit_camera
    pc, env, leaves = make_surfel_model(P, 800, dev, seed=0, radius_px=7.0)
    pipe = SimpleNamespace(depth_ratio=0.0, debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    env.build_mips()
    out = render_surfel(orbit_camera(0, 800, 800, n_views=8).to(dev), pc, pipe, torch.zeros(3, device=dev), srgb=False, opt=SimpleNamespace(indirect=False))
    outs = [out[k] for k in ("render", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal")]
    torch.autograd.backward(outs, [torch.ones_like(outs[0])] + [torch.full_like(o, 0.1) for o in outs[1:]])
    touched = torch.stack([(t.grad.reshape(P, -1) != 0).any(dim=1) for t in leaves if t.grad is not None and t.shape[0] == P]).any(dim=0)
    return out["visibility_filter"].clone(), touched


def masks(dev):
    g = torch.Generator().manual_seed(0)
    scene, touched = scene_masks(dev)
    density, t_density = float(scene.float().mean()), float(touched.float().mean())
    return [("all ones", torch.ones(P, dtype=torch.bool, device=dev)),
            (f"bench view, visibility_filter ({100 * density:.1f} %)", scene),
            (f"random, same density ({100 * density:.1f} %)", (torch.rand(P, generator=g) < density).to(dev)),
            (f"bench view, rows with a gradient ({100 * t_density:.1f} %)", touched),
            (f"random, same density ({100 * t_density:.1f} %)", (torch.rand(P, generator=g) < t_density).to(dev)),
            ("random 10 %", (torch.rand(P, generator=g) < 0.10).to(dev)),
            ("all zeros", torch.zeros(P, dtype=torch.bool, device=dev))]


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS          # microseconds per call


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    mask_list = masks(dev)
    stream = _lib.stream_ptr(dev)
    fmt = lambda xs: f"{statistics.median(xs):7.1f} [{min(xs):.1f} .. {max(xs):.1f}]"
    print(f"P = {P}; {CALLS} calls per window, {PAIRS} alternated pairs; microseconds per call as median [min .. max]")
    for set_name, widths in SETS.items():
        tensors = [[torch.randn(P, w, device=dev) * s for s in (1.0, 0.01, 0.01, 1e-4)] for w in widths]      # param, grad, exp_avg, exp_avg_sq
        for t in tensors:
            t[3].abs_()
        dense = (_lib.MrgsAdamTensor * len(widths))(*[_lib.MrgsAdamTensor(*[x.data_ptr() for x in t], t[0].numel(), 1e-6, 100) for t in tensors])
        rows = (_lib.MrgsAdamRowsTensor * len(widths))(*[_lib.MrgsAdamRowsTensor(*[x.data_ptr() for x in t], t[0].numel(), w, 1e-6, 100, 0)
                                                         for t, w in zip(tensors, widths)])

        def run_dense():
            _lib.check(L.mrgs_adam_step(dense, len(widths), 0.9, 0.999, 1e-15, stream))
        full = dense_bytes(widths, P)
        print(f"\n{set_name}: {len(widths)} tensors, {sum(widths) * P / 1e6:.1f} M elements, dense model {full / 1e6:.0f} MB")
        for name, mask in mask_list:
            ptrs = (ctypes.c_void_p * 1)(mask.data_ptr())

            def run_rows():
                _lib.check(L.mrgs_adam_step_rows(rows, len(widths), P, ptrs, 1, 1, 0.9, 0.999, 1e-15, stream))
            for fn in (run_dense, run_rows):                       # warm-up of this pair
                window(fn)
            td, tr = [], []
            for _ in range(PAIRS):
                td.append(window(run_dense))
                tr.append(window(run_rows))
            vis = mask.cpu().numpy()
            b16, b128 = model_bytes(widths, vis), model_bytes(widths, vis, line_bytes=128)
            d = statistics.median(td)
            print(f"  {name:46s} dense {fmt(td)}   masked {fmt(tr)}   ratio {statistics.median(tr) / d:.3f}   masked faster in "
                  f"{sum(x < y for x, y in zip(tr, td)):2d} of {PAIRS} pairs   model at the dense rate: 16-B pieces {d * b16 / full:6.1f} us "
                  f"({b16 / 1e6:.0f} MB), 128-B lines {d * b128 / full:6.1f} us ({b128 / 1e6:.0f} MB)   dense rate {full / d / 1e6:.2f} TB/s", flush=True)
        del tensors


if __name__ == "__main__":
    main()
