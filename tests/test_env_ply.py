"""env_point_cloud.ply of the environment set (scene/env_gaussian_model.py:198-277): env_model.save_ply / load_ply (functions of the
model; the class keeps no methods of those names) on materialrefgs_amd.io.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from materialrefgs_amd import io  # noqa: E402
from materialrefgs_amd import env_model  # noqa: E402
from materialrefgs_amd.env_model import EnvGaussianModel  # noqa: E402

ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _model(P=7, degree=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = EnvGaussianModel(degree)
    K = (degree + 1) ** 2 - 1
    for name, shape in zip(ATTRS, ((P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 2), (P, 4))):
        setattr(m, name, torch.nn.Parameter(torch.randn(*shape, generator=g)))
    return m


def _reference_names(K):
    """construct_list_of_attributes (:198-210)."""
    return ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * K)] + ["opacity"] + \
        [f"scale_{i}" for i in range(2)] + [f"rot_{i}" for i in range(4)]


def test_header_lists_the_reference_attributes_in_order(tmp_path):
    m = _model()
    path = str(tmp_path / "point_cloud" / "iteration_7" / "env_point_cloud.ply")      # the directory is made, as mkdir_p does (:213)
    env_model.save_ply(m, path)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert head[3:] == [f"property float {n}" for n in _reference_names(15)]
    names, data = io.read_ply_vertices(path)
    assert names == _reference_names(15) and data.shape == (7, 61) and data.dtype == np.float32


def test_rows_are_the_transposed_sh_layout(tmp_path):
    m = _model()
    path = str(tmp_path / "env_point_cloud.ply")
    env_model.save_ply(m, path)
    raw = open(path, "rb").read().split(b"end_header\n", 1)[1]
    rows = np.frombuffer(raw, dtype="<f4").reshape(7, 61)
    d = lambda t: t.detach().numpy()
    # save_ply :215-226: xyz, zeros, f_dc.transpose(1, 2).flatten(1), f_rest.transpose(1, 2).flatten(1), opacity, scale, rotation
    want = np.concatenate([d(m._xyz), np.zeros((7, 3), np.float32), d(m._features_dc.transpose(1, 2).flatten(start_dim=1)),
                           d(m._features_rest.transpose(1, 2).flatten(start_dim=1)), d(m._opacity), d(m._scaling), d(m._rotation)], axis=1)
    assert rows.tobytes() == np.ascontiguousarray(want, dtype="<f4").tobytes()
    assert rows[0, 9] == d(m._features_rest)[0, 0, 0] and rows[0, 10] == d(m._features_rest)[0, 1, 0]      # channel-major: f_rest_1 is coefficient 1 of red
    assert rows[0, 9 + 15] == d(m._features_rest)[0, 0, 1]


@pytest.mark.parametrize("degree", (3, 1, 0))
def test_save_load_round_trips_every_bit(degree, tmp_path):
    m = _model(P=11, degree=degree, seed=degree)
    path = str(tmp_path / "env_point_cloud.ply")
    env_model.save_ply(m, path)
    back = EnvGaussianModel(degree)
    assert back.active_sh_degree == 0
    env_model.load_ply(back, path, device="cpu")
    assert back.active_sh_degree == degree                              # :277
    for name in ATTRS:
        a, b = getattr(m, name), getattr(back, name)
        assert isinstance(b, torch.nn.Parameter) and b.requires_grad and b.is_contiguous()
        assert b.shape == a.shape and b.dtype == torch.float32
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes()
    assert torch.equal(back.get_features, m.get_features)


def test_wrong_f_rest_count_is_refused(tmp_path):
    m = _model(degree=2)                                                # 24 f_rest properties
    path = str(tmp_path / "env_point_cloud.ply")
    env_model.save_ply(m, path)
    with pytest.raises(ValueError, match="f_rest"):                     # the reference asserts the count (:251)
        env_model.load_ply(EnvGaussianModel(3), path, device="cpu")
    env_model.load_ply(EnvGaussianModel(2), path, device="cpu")


def test_the_gaussian_models_ply_is_written_as_before(tmp_path):
    """save_ply of the main model goes through the same writer: its bytes are those of the layout it documents."""
    g = torch.Generator().manual_seed(1)
    shapes = {"xyz": (4, 3), "normal1": (4, 3), "normal2": (4, 3), "features_dc": (4, 1, 3), "features_rest": (4, 15, 3), "indirect_dc": (4, 1, 3),
              "indirect_rest": (4, 15, 3), "indirect_asg": (4, 32, 5), "opacity": (4, 1), "refl_strength": (4, 1), "metalness": (4, 1),
              "roughness": (4, 1), "ori_color": (4, 3), "diffuse_color": (4, 3), "scaling": (4, 2), "rotation": (4, 4)}
    t = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    path = str(tmp_path / "point_cloud.ply")
    io.save_ply(path, t)
    back = io.load_ply(path)
    for k in shapes:
        assert torch.equal(back[k], t[k]), k
