"""Generates tests/golden/reference_prior.npz by running the reference's OWN mono_normal_loss -- the function text of train_refnerf.py
(train_glossy.py and train_refreal.py hold the same body), lifted out of the file with gen_reference_warp_vectors.lift because the
training scripts import the whole CUDA stack at module level -- on the analytic inputs of tests/prior_statement.py.  As in that
generator `.cuda()` and `.float()` are the identity and the default dtype is float64, so the reference runs in float64 on inputs that
are exact in float32.  The iteration is 1: the `iteration % 3000` debug dump (imageio, a ./debug directory) is not taken.
The mask-entropy and ref-score lines are inline in training() and cannot be lifted; tests/prior_statement.py is their definition.

Recorded per case: the inputs (normal maps and prior quantised to 1/64 and stored as float16, the mask as its 8-bit levels), the four
scalars and the gradients of sum_k up_k term_k with respect to both normal maps (float32).  Only data is committed; the reference source
never travels.

    python tests/golden/gen_reference_prior_vectors.py       # needs /root/reference (absent on the GPU box)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_reference_warp_vectors import lift  # noqa: E402  (also: float64 default dtype, .cuda() / .float() as the identity)

import prior_statement as ps  # noqa: E402   (the analytic inputs only)

SIZES = ((37, 53), (24, 40))
UP = (0.7, 1.3, 0.9, 1.1)
STEPS = 64


def main():
    ns = {"torch": torch, "np": np, "os": os, "imageio": None}
    lift("train_refnerf.py", ["mono_normal_loss"], ns)
    out = {"up": np.array(UP)}
    for H, W in SIZES:
        inp = ps.analytic_inputs(H, W, seed=1, steps=STEPS)
        tag = f"{H}x{W}"
        for k in ("surf_normal", "rend_normal", "prior"):
            half = inp[k].to(torch.float16)
            assert torch.equal(half.to(torch.float32), inp[k]), k                     # the quantised values are exact in float16
            out[f"{tag}_{k}"] = half.numpy()
        levels = torch.round(inp["mask"] * 255)
        assert torch.equal((levels / 255).to(torch.float32), inp["mask"])
        out[f"{tag}_mask"] = levels.to(torch.uint8).numpy()
        out[f"{tag}_R"] = inp["R"].numpy()
        cam = SimpleNamespace(R=inp["R"].double(), image_name="view")
        for masked in (True, False):
            surf = inp["surf_normal"].double().requires_grad_(True)
            rend = inp["rend_normal"].double().requires_grad_(True)
            masks = {"view": inp["mask"].double()} if masked else None
            terms = ns["mono_normal_loss"](cam, surf, rend, masks, {"view": inp["prior"].double()}, 1.0, 1)
            sum(u * t for u, t in zip(UP, terms)).backward()
            name = f"{tag}_{'mask' if masked else 'nomask'}"
            out[f"{name}_terms"] = np.array([float(t.detach()) for t in terms])
            out[f"{name}_g_surf"] = surf.grad.numpy().astype(np.float32)
            out[f"{name}_g_rend"] = rend.grad.numpy().astype(np.float32)
            print(name, out[f"{name}_terms"])
    path = os.path.join(HERE, "reference_prior.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; reference_warp.npz has", os.path.getsize(os.path.join(HERE, "reference_warp.npz")))


if __name__ == "__main__":
    main()
