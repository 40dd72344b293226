"""Writes tests/golden/pil_resize.npz: inputs and Pillow's own `Image.resize((W, H))` outputs (default filter: BICUBIC) for the size list
of tests/test_scene_resize.py, on uniform random bytes and on {0, 255} masks, as L and as RGB images.  Needs Pillow; the tests do not.

    python tests/golden/gen_pil_vectors.py
"""
import os

import numpy as np
import PIL
from PIL import Image

# (h, w) -> (H, W)
SIZES = (((29, 37), (14, 18)), ((41, 50), (13, 16)), ((20, 24), (40, 48)), ((20, 24), (20, 12)), ((20, 24), (7, 24)), ((33, 17), (1, 1)),
         ((16, 16), (16, 16)), ((64, 48), (63, 47)), ((9, 200), (9, 3)), ((257, 130), (128, 65)))


def main():
    rng = np.random.default_rng(20261020)
    out = {"sizes": np.array([[h, w, H, W] for (h, w), (H, W) in SIZES], dtype=np.int32), "pillow_version": np.array(PIL.__version__)}
    for k, ((h, w), (H, W)) in enumerate(SIZES):
        for kind in ("random", "mask"):
            for mode, shape in (("L", (h, w)), ("RGB", (h, w, 3))):
                a = rng.integers(0, 256, shape, dtype=np.uint8) if kind == "random" else (rng.integers(0, 2, shape, dtype=np.uint8) * 255)
                r = np.array(Image.fromarray(a, mode).resize((W, H)))
                out[f"{k}_{kind}_{mode}_in"], out[f"{k}_{kind}_{mode}_out"] = a, r
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
