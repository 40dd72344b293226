"""Times the two things a device-resident view store changes (materialrefgs_amd.viewstore, csrc/mrgs_image.hip), each as alternated
batches in one process, wall clock with a closing synchronise:

  fetch   the per-iteration cost of a view's ground truth, mask prior and normal prior: the native decode (one launch from the byte planes
          on the device: gt, grey, mask, normal) against the reference's form -- the same data as fp32 tensors in pageable host memory and
          three `.cuda()` calls (train_refnerf.py:1176, :1212, :222-223) -- at 800 x 800 and 1600 x 1200.
  load    upload + compositing + resize of 100 synthetic RGBA views from 1600 x 1200 at -r 2 (the store's `add`), against Pillow's resize
          of the same views on the host when Pillow imports (the reference's loader, without its float64 compositing).

    python tools/scene_time.py [fetch] [load]
Per-kernel times: rocprofv3 --kernel-trace --stats -d OUT -o s -- python tools/scene_time.py fetch
Developer tool; prints one line per measurement, every run included."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import viewstore as vs  # noqa: E402

PAIRS, BATCH = 7, 50


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fetch(dev):
    rng = np.random.default_rng(0)
    for H, W in ((800, 800), (1600, 1200)):
        store = vs.ViewStore(dev)
        rgb, normal, mask = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W, 3), (H, W, 3), (H, W)))
        store.add("v", rgb)
        store.add_prior("v", normal=normal, mask=mask)
        want = ("gt", "grey", "mask", "normal")
        got = store.fetch("v", want)
        # the reference's form: fp32 tensors in pageable host memory, as Camera and load_normal_prior leave them
        host = [got["gt"].cpu().clone(), got["mask"].cpu().clone(), got["normal"].cpu().clone()]
        assert not any(t.is_pinned() for t in host)

        def native():
            return store.fetch("v", want)

        def upload():
            return [t.cuda() for t in host]
        for f in (native, upload):
            for _ in range(5):
                f()
        tn, tu = [], []
        for _ in range(PAIRS):
            tn.append(wall(native, BATCH))
            tu.append(wall(upload, BATCH))
        fmt = lambda xs: ", ".join(f"{v:.3f}" for v in xs)
        wins = sum(a < b for a, b in zip(tn, tu))
        mb_u8, mb_f32 = H * W * 7 / 1e6, H * W * 7 * 4 / 1e6
        print(f"fetch {W}x{H}: native decode {min(tn):.3f} ms ({mb_u8:.1f} MB of planes -> {mb_f32 + H * W * 4 / 1e6:.1f} MB fp32), three pageable uploads "
              f"{min(tu):.3f} ms ({mb_f32:.1f} MB), decode faster in {wins}/{PAIRS} alternated pairs of {BATCH} (decode {fmt(tn)} / uploads {fmt(tu)})",
              flush=True)


def load(dev):
    n, H, W = 100, 1200, 1600
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (H + n, W, 4), dtype=np.uint8)
    views = [np.ascontiguousarray(base[k:k + H]) for k in range(n)]
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def native():
        store = vs.ViewStore(dev)
        for k, a in enumerate(views):
            store.add(k, a, size=(H // 2, W // 2), white_background=True)
        return store

    def pillow():
        return [np.array(Image.fromarray(a[:, :, :3], "RGB").resize((W // 2, H // 2))) for a in views]
    native()
    tn, tp = [], []
    for _ in range(3):
        tn.append(wall(native, 1))
        if Image is not None:
            tp.append(wall(pillow, 1))
    fmt = lambda xs: ", ".join(f"{v:.0f}" for v in xs)
    host = f"Pillow's resize alone on the host {min(tp):.0f} ms (runs {fmt(tp)})" if tp else "Pillow is not installed: no host figure"
    print(f"load {n} RGBA views {W}x{H} at -r 2: upload + compositing + resize {min(tn):.0f} ms (runs {fmt(tn)}), {native().nbytes / 1e6:.0f} MB kept; {host}",
          flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["fetch", "load"]
    device = torch.device("cuda:0")
    if "fetch" in what:
        fetch(device)
    if "load" in what:
        load(device)
