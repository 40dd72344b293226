"""bench.py's plain run and --dump-outputs (-m gpu): the plain line carries the headline and nothing that takes runs of its own, --steps
is the number of timed steps, and the dump is the last timed step's outputs and gradients in float32 / float64 within 64 MB; two runs
with the same arguments dump the same arrays (same names, shapes, and values up to the run-to-run order of float atomics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(out_dir, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out_dir)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.parametrize("workload", ["tiny", "tinyfull"])
def test_plain_run_and_dumped_outputs(gpu_device, tmp_path, workload):
    line, a = _bench(tmp_path / "a", "--workload", workload, "--steps", "3", "--warmup", "2")
    assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "views/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["value"] > 0
    assert abs(line["ms_per_step"] * 3 / 1000.0 - line["timed_region_s"]) <= 1e-4      # both rounded: ms to 1e-4, s to 1e-4
    assert not {"roofline", "stage_ms", "cpu_baseline", "exchange_model", "cold_ms_per_step", "secondary_raster"} & set(line)
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    want = {"render", "grad_xyz", "grad_features_rest", "grad_env_base", "grad_viewspace_points"} if workload == "tinyfull" else \
        {"color", "allmap", "feature", "radii", "grad_means3D", "grad_sh", "grad_means2D"}
    assert want <= set(a), sorted(a)
    assert any(float(np.abs(v).max()) > 0 for k, v in a.items() if k.startswith("grad_"))
    _, b = _bench(tmp_path / "b", "--workload", workload, "--steps", "3", "--warmup", "2")
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
        m = max(float(np.abs(a[k]).max()), 1e-30)
        assert float(np.abs(a[k].astype(np.float64) - b[k]).max()) <= 1e-4 * m, k
