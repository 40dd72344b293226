"""Every MRGS_E_HIP carries its reason: each translation unit of libmrgs.so reports a failed HIP call through the one status helper
(csrc/mrgs_internal.h), so mrgs_last_hip_error() names the file and line of the call that failed, on the thread it failed on.

Runs only where there is NO device: every HIP call then returns "no ROCm-capable device is detected" and nothing is launched, which is the
one way to see the failure path of every file without a failure on a GPU.  The pointers are host addresses and must never reach a machine
that can launch, hence the skip, decided before the library is touched."""
import ctypes
import os
import re
import threading

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.device_count() != 0, reason="host addresses as arguments: only for a machine without a device")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = (ctypes.c_float * 65536)()
P = (ctypes.addressof(_BUF) + 63) & ~63        # every pointer argument (the k-NN workspace has to be 16-byte aligned)
_BG = (ctypes.c_float * 3)(0.0, 0.0, 0.0)       # the tracer's background colour is read on the host


def _surfel_features(L):
    from materialrefgs_amd._lib import MrgsSurfelParams
    prm = MrgsSurfelParams(4, *([P] * 10), None)
    return L.mrgs_surfel_features_forward(ctypes.byref(prm), P, P, P, P, None)


def _loss(L):
    from materialrefgs_amd._lib import MrgsLossConfig
    cfg = MrgsLossConfig(16, 16, 3, 0.2, 0.0, 0.0)
    return L.mrgs_loss_forward(ctypes.byref(cfg), P, P, None, None, None, None, P, L.mrgs_loss_ws_bytes(16, 16, 3), P, P, None)


def _ncc_backward(L):
    from materialrefgs_amd._lib import MrgsWarpConfig
    cfg = MrgsWarpConfig(8, 8, 4, 1, -1, 0, 0, 0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    return L.mrgs_warp_ncc_backward(ctypes.byref(cfg), P, P, 1.0, P, P, P, None)


def _prior_terms(L):
    from materialrefgs_amd._lib import MrgsPriorConfig
    cfg = MrgsPriorConfig(8, 8, 0)          # the alpha group alone: rend_alpha and alpha_mask
    return L.mrgs_prior_terms_forward(ctypes.byref(cfg), None, None, None, None, None, P, P, None, None, None, P, L.mrgs_prior_ws_bytes(8, 8), P, None)


def _mips():
    """A chain of one 4 x 4 level."""
    from materialrefgs_amd._lib import MrgsEnvMips
    m = MrgsEnvMips()
    m.n_levels, m.res[0], m.tex[0], m.min_roughness, m.max_roughness = 1, 4, P, 0.08, 0.5
    return m


def _bounce(L):
    from materialrefgs_amd._lib import MrgsBounceConfig
    cfg = MrgsBounceConfig(0, 4, 10, 12, 4, 8)
    return L.mrgs_bounce_shade_forward(ctypes.byref(cfg), ctypes.byref(_mips()), P, P, P, P, P, None, P, P, P, P, P, None)


def _smooth(L):
    """Both directions: the forward is checked here, the backward's status is returned; its text names another line of the same file."""
    from materialrefgs_amd import _lib
    cfg = _lib.MrgsSmoothConfig(4, 4, 0)
    its = (_lib.MrgsSmoothItem * 1)(_lib.MrgsSmoothItem(P, None, P, 3, 1))
    table = (ctypes.c_void_p * 1)(P)
    assert L.mrgs_smooth_terms_forward(ctypes.byref(cfg), P, its, 1, P, L.mrgs_smooth_ws_bytes(4, 4), P, None) == _lib.MRGS_E_HIP
    forward = L.mrgs_last_hip_error()
    assert forward and b" at mrgs_smooth.hip:" in forward, forward
    rc = L.mrgs_smooth_terms_backward(ctypes.byref(cfg), P, its, 1, table, None)
    assert L.mrgs_last_hip_error() != forward
    return rc


# one well-formed call per translation unit that has launch entry points: file -> call(L) -> status
CALLS = {
    "mrgs_api": lambda L: L.mrgs_mark_visible(4, P, P, P, P, None),
    "mrgs_shade": lambda L: L.mrgs_envmap_lookup_forward(ctypes.byref(_mips()), 4, P, None, P, None),
    "mrgs_prefilter": lambda L: L.mrgs_cubemap_mip_forward(2, P, P, None),
    "mrgs_bounce": _bounce,
    "mrgs_smooth": _smooth,
    "mrgs_edges": lambda L: L.mrgs_edge_mask(P, 4, 4, 7, 0.0, 80.0, 1, P, None, P, L.mrgs_edges_ws_bytes(4, 4), None),
    "mrgs_maps": lambda L: L.mrgs_surfel_composite_forward(2, 2, 0, *([P] * 7), None),
    "mrgs_surfel": _surfel_features,
    "mrgs_loss": _loss,
    "mrgs_multiview": _ncc_backward,
    "mrgs_trace_prep": lambda L: L.mrgs_traced_blend_forward(1, 1, P, P, 1, 3, P, 1, P, None),
    "mrgs_surfel_hier": lambda L: L.mrgs_surfel_bvh_build(P, 4, P, L.mrgs_surfel_bvh_bytes(4), P, L.mrgs_surfel_bvh_ws_bytes(4), None),
    # an empty model: the forward clears the maps of its 4 rays, the first HIP call of that file
    "mrgs_surfel_trace": lambda L: L.mrgs_surfel_trace_forward(None, 0, 4, 0, P, P, None, None, _BG, P, P, P, P, P, P, None, None, 0, None),
    "mrgs_bvh": lambda L: L.mrgs_bvh_trace(P, 4, 4, P, P, P, P, P, P, None),
    "mrgs_knn": lambda L: L.mrgs_knn_mean_dist2(P, 64, P, P, L.mrgs_knn_ws_bytes(64), None),
    "mrgs_densify": lambda L: L.mrgs_densify_stats(4, *([P] * 6), None),
    "mrgs_env_densify": lambda L: L.mrgs_env_densify_stats(4, P, P, None, P, P, None, None),
    "mrgs_mesh": lambda L: L.mrgs_mesh_select(4, 0, None, P, P, 1, P, None, None),
    "mrgs_prior": _prior_terms,
    "mrgs_optim": lambda L: L.mrgs_compact_count(0, P, P, L.mrgs_compact_ws_bytes(0), P, None),
    "mrgs_cubemapenc": lambda L: L.mrgs_cubemap_encode_forward(P, P, P, P, 0, 0, 4, 3, 1, None),
}


def _lib():
    from materialrefgs_amd import _lib
    return _lib, _lib.lib()


def test_calls_cover_every_file_that_returns_a_launch_status():
    csrc = os.path.join(ROOT, "materialrefgs_amd", "csrc")
    using = {f[:-4] for f in os.listdir(csrc) if f.endswith(".hip") and "MRGS_LAUNCH_STATUS()" in open(os.path.join(csrc, f)).read()}
    assert using == set(CALLS)


@pytest.mark.parametrize("stem", sorted(CALLS))
def test_hip_failure_names_its_file(stem):
    lib, L = _lib()
    assert CALLS[stem](L) == lib.MRGS_E_HIP
    text = L.mrgs_last_hip_error()
    assert text and f" at {stem}.hip:".encode() in text, text


def test_no_stale_text():
    """The text belongs to the LAST failing call, whichever file it is in."""
    lib, L = _lib()
    for first, second in (("mrgs_api", "mrgs_trace_prep"), ("mrgs_knn", "mrgs_api")):
        assert CALLS[first](L) == lib.MRGS_E_HIP and f" at {first}.hip:".encode() in L.mrgs_last_hip_error()
        assert CALLS[second](L) == lib.MRGS_E_HIP
        text = L.mrgs_last_hip_error()
        assert f" at {second}.hip:".encode() in text and f"{first}.hip".encode() not in text, text


def test_text_is_per_thread():
    lib, L = _lib()
    assert CALLS["mrgs_api"](L) == lib.MRGS_E_HIP
    mine = L.mrgs_last_hip_error()
    seen = {}

    def worker():
        seen["fresh"] = L.mrgs_last_hip_error()
        seen["rc"] = CALLS["mrgs_densify"](L)
        seen["after"] = L.mrgs_last_hip_error()
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert seen["fresh"] == b""
    assert seen["rc"] == lib.MRGS_E_HIP and b" at mrgs_densify.hip:" in seen["after"]
    assert L.mrgs_last_hip_error() == mine and b" at mrgs_api.hip:" in mine


def test_check_raises_with_the_file_name():
    lib, L = _lib()
    with pytest.raises(RuntimeError, match=r"libmrgs: HIP runtime error .* at mrgs_maps\.hip:\d+"):
        lib.check(CALLS["mrgs_maps"](L))


def test_status_constants_equal_the_headers_enum():
    from materialrefgs_amd import _lib as lib          # (no library call: this one needs no device either way, but shares the module's skip)
    src = open(os.path.join(ROOT, "include", "mrgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = next(b for b in re.findall(r"enum\s*\{(.*?)\}", src, flags=re.S) if "MRGS_OK" in b)
    enum = {name: int(value) for name, value in re.findall(r"\b(MRGS_\w+)\s*=\s*(\d+)", body)}
    assert list(enum) == ["MRGS_OK", "MRGS_E_BAD_ARG", "MRGS_E_TOO_MANY_FEATURES", "MRGS_E_NEED_COLORS", "MRGS_E_HIP", "MRGS_E_WORKSPACE",
                          "MRGS_E_UNSUPPORTED", "MRGS_E_INTERNAL"]
    for name, value in enum.items():
        assert getattr(lib, name) == value, name
