"""Per-view evaluation metrics (csrc/mrgs_eval.hip: mrgs_eval_metrics behind materialrefgs_amd.evaluate.image_metrics): the statement
against the reference's own ssim / psnr / l1_loss run as eval.py and train_refreal.py call them (tests/golden/reference_eval.npz), the
HIP call against the reference's float64 values with the bars the fused loss's terms are held to (tests/test_losses.py:147, :223)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_statement as es  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_eval.npz"))
CASES = {"a": (37, 45), "b": (9, 70), "c": (64, 48), "d": (11, 11)}
KEYS = ("psnr_image", "ssim", "l1", "psnr_channels")                  # columns 0..3 of a row
SSIM_ATOL = 2e-6                                                       # tests/test_losses.py:223
RTOL, ATOL = 5e-6, 1e-6                                                # tests/test_losses.py:147


def _pair(tag, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(GOLD[f"{tag}_img"]).to(device, dtype), torch.from_numpy(GOLD[f"{tag}_gt"]).to(device, dtype)


def _within_bars(got, tag, what):
    """got: dict of the four numbers; the fixture's float64 values are the reference."""
    for k in KEYS:
        want = float(GOLD[f"{tag}_f64_{k}"])
        err = abs(float(got[k]) - want)
        print(f"{what} {tag} {k}: {float(got[k])!r} vs {want!r}, off by {err:.3e}")
        if k == "ssim":
            assert err <= SSIM_ATOL, (what, tag, k, err)
        else:
            assert err <= ATOL + RTOL * abs(want), (what, tag, k, err)


# ---------------------------------------------------------------- CPU
def test_fixture_is_what_the_generator_describes():
    assert np.array_equal(es.window_2d(torch.float32).numpy(), GOLD["window_2d"])
    for tag, (H, W) in CASES.items():
        img, gt = GOLD[f"{tag}_img"], GOLD[f"{tag}_gt"]
        assert img.shape == gt.shape == (3, H, W) and img.dtype == np.float32
        outside = (((img < 0) | (img > 1)).mean() + ((gt < 0) | (gt > 1)).mean()) / 2
        assert 0.12 < outside < 0.3                                    # unclamped: the clamp of eval.py:44-46 matters
        assert (gt[:, : max(1, H // 4), : max(1, W // 3)] == 0).all()  # the flat block


@pytest.mark.parametrize("tag", CASES)
def test_statement_in_float64_is_the_reference(tag):
    img, gt = _pair(tag, torch.float64)
    row = es.metrics(img, gt)
    for i, k in enumerate(KEYS):
        assert abs(float(row[i]) - float(GOLD[f"{tag}_f64_{k}"])) < 1e-12, (k, float(row[i]), float(GOLD[f"{tag}_f64_{k}"]))
    assert float(row[7]) == 0.0
    assert abs(float(row[4:7].mean()) - 10 ** (-float(row[0]) / 10)) < 1e-14          # the whole-image mse is the mean of the three
    # without the clamp the numbers are others: the fixture does exercise it
    a, b = img, gt
    assert abs(float((a - b).abs().mean()) - float(GOLD[f"{tag}_f64_l1"])) > 1e-4


@pytest.mark.parametrize("tag", CASES)
def test_reference_float32_run_lies_within_the_gpu_bars_of_its_float64_run(tag):
    """The bars of the GPU test are reachable by a float32 evaluation: the reference's own is inside them on every shape."""
    _within_bars({k: GOLD[f"{tag}_f32_{k}"] for k in KEYS}, tag, "reference fp32")


def test_bad_arguments_are_refused_before_any_launch():
    """No GPU needed: every check precedes the first HIP call."""
    from materialrefgs_amd import _lib
    L = _lib.lib()
    BAD_ARG, WORKSPACE = 1, 5
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p = (p + 15) & ~15
    need = L.mrgs_eval_metrics_ws_bytes(37, 45)
    assert need == 2 * 2 * 3 * 16 and L.mrgs_eval_metrics_ws_bytes(0, 45) == 0

    def call(H=37, W=45, image=p, gt=p, ws=p, ws_bytes=need, out=p, size=None, flags=0):
        cfg = _lib.MrgsEvalConfig(H, W, flags)
        if size is not None:
            cfg.struct_size = size
        return L.mrgs_eval_metrics(ctypes.byref(cfg), image, gt, ws, ws_bytes, out, None)
    assert call(H=0) == BAD_ARG and call(W=-3) == BAD_ARG
    assert call(image=None) == BAD_ARG and call(gt=None) == BAD_ARG and call(out=None) == BAD_ARG and call(ws=None) == BAD_ARG
    assert call(size=12) == BAD_ARG and call(flags=1) == BAD_ARG
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert L.mrgs_eval_metrics(None, p, p, p, need, p, None) == BAD_ARG


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES)
def test_hip_metrics_match_the_reference(tag, gpu_device):
    from materialrefgs_amd import evaluate as ev
    img, gt = _pair(tag, device=gpu_device)
    row = ev.image_metrics(img, gt)
    assert row.shape == (8,) and row.dtype == torch.float32 and row.device == img.device
    host = row.cpu().numpy()
    _within_bars(dict(zip(KEYS, host[:4])), tag, "hip")
    want = es.metrics(*_pair(tag, torch.float64)).numpy()
    np.testing.assert_allclose(host[4:7], want[4:7], rtol=RTOL, atol=1e-9)
    assert host[7] == 0.0
    assert torch.equal(ev.image_metrics(img, gt), row)                 # fixed reduction order: the same bits again
    assert torch.equal(img, torch.from_numpy(GOLD[f"{tag}_img"]).to(gpu_device))     # nothing clamped in place


@pytest.mark.gpu
def test_hip_metrics_edge_cases(gpu_device):
    from materialrefgs_amd import evaluate as ev, losses
    img, gt = _pair("a", device=gpu_device)
    # identical images: mse 0 -> +inf as the reference's 20 log10(1 / sqrt(0)), ssim 1
    same = ev.image_metrics(img, img.clone()).cpu()
    assert float(same[0]) == float("inf") and float(same[3]) == float("inf") and abs(float(same[1]) - 1.0) < 1e-6
    assert float(same[2]) == 0.0 and (same[4:] == 0).all()
    # values that differ only outside [0, 1] are identical after the clamp
    far = img.clone()
    far[img > 1] += 3.0
    far[img < 0] -= 3.0
    assert torch.equal(ev.image_metrics(far, gt), ev.image_metrics(img, gt))
    # a 4-channel ground truth passes its first three channels (eval.py:47), contiguous or not; a leading batch of 1 is dropped
    row = ev.image_metrics(img, gt)
    gt4 = torch.cat([gt, torch.full_like(gt[:1], 7.0)])
    assert torch.equal(ev.image_metrics(img, gt4), row)
    wide = torch.cat([gt4, gt4], dim=2)[:, :, : gt.shape[2]]
    assert not wide.is_contiguous() and torch.equal(ev.image_metrics(img[None], wide), row)
    # row k of a table: the other rows stay as they were
    table = torch.full((5, 8), -2.0, device=gpu_device)
    assert ev.image_metrics(img, gt, out=table[3]).data_ptr() == table[3].data_ptr()
    assert torch.equal(table[3], row) and (table[[0, 1, 2, 4]] == -2.0).all()
    # psnr_channels is out_terms[6] of the fused loss on pre-clamped inputs
    a, b = img.clamp(0, 1), gt.clamp(0, 1)
    terms = losses.fused_loss(a, b)[1].cpu()
    got = row.cpu()
    assert abs(float(got[3]) - float(terms[6])) <= 5e-6 * abs(float(terms[6]))
    np.testing.assert_allclose(got[4:7].numpy(), terms[7:10].numpy(), rtol=5e-6)
    # more than one workgroup per channel row and column, a size that is no multiple of the tile, against the float64 statement
    g = torch.Generator().manual_seed(11)
    big_a, big_b = torch.rand(3, 70, 131, generator=g) * 1.4 - 0.2, torch.rand(3, 70, 131, generator=g) * 1.4 - 0.2
    want = es.metrics(big_a.double(), big_b.double()).numpy()
    got = ev.image_metrics(big_a.to(gpu_device), big_b.to(gpu_device)).cpu().numpy()
    assert abs(got[1] - want[1]) <= SSIM_ATOL
    np.testing.assert_allclose(got[[0, 2, 3]], want[[0, 2, 3]], rtol=RTOL, atol=ATOL)
    with pytest.raises(RuntimeError, match="device tensor"):
        ev.image_metrics(img.cpu(), gt.cpu())
    with pytest.raises(ValueError):
        ev.image_metrics(img, gt[:, :-1])
