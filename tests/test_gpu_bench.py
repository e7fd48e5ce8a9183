"""-m gpu: bench.py's own command line on one GPU -- what a plain run reports, what --full adds, and that --dump-outputs writes the
same inputs' outputs from run to run (a small scene: the protocol, not the headline's size)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--gaussians", "100000"]
FULL_ONLY = ("value_warm", "ms_per_step_warm", "pipelined", "roofline", "roofline_fwd", "stage_ms", "host")


def _bench(args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GSRAST_SINGLE_DEVICE", "GSRAST_FORCE_COLLECTIVES"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_times_the_headline_only_and_dumps_the_same_outputs_every_run(tmp_path):
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / f"run{k}"
        lines.append(_bench(SMALL + ["--dump-outputs", str(d)]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    for r in lines:
        assert r["steps"] == 3 and r["warmup"] == 2 and r["n_gpus"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
        assert abs(r["value"] - 1e3 / r["ms_per_step"]) <= 1e-3 * r["value"] + 1e-2
        assert r["dtype"] == "f32" and r["unit"] == "views/s" and r["higher_is_better"] is True
        assert not [k for k in FULL_ONLY if k in r] and "cpu_baseline" not in r and "sweep_1080p_cold" not in r
    a, b = dumps
    assert sorted(a) == ["color", "depth", "grad_means2D", "grad_means3D", "grad_opacities", "grad_rotations", "grad_scales", "grad_shs", "radii", "rows"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["color"].shape == (3, 1080, 1920) and a["depth"].shape == (1, 1080, 1920) and a["grad_shs"].shape == (65536, 16, 3)
    assert np.abs(a["color"]).max() > 0 and (a["radii"] > 0).any() and np.abs(a["grad_means3D"]).max() > 0
    # the forward is deterministic: the same camera and scene give the same bits; the backward's float atomics sum in another order every
    # run (parity with the oracle is the other tests' business: here only that both runs computed the same thing)
    for name in ("rows", "color", "depth", "radii"):
        assert np.array_equal(a[name], b[name]), name
    for name in ("grad_means2D", "grad_means3D", "grad_opacities", "grad_rotations", "grad_scales", "grad_shs"):
        x, y = a[name].astype(np.float64), b[name].astype(np.float64)
        assert (np.abs(x - y) <= 1e-4 * np.abs(x).max() + 1e-3 * np.abs(x)).all(), name


def test_full_run_keeps_the_side_measurements():
    r = _bench(SMALL + ["--full", "--sweep", "", "--no-cpu-baseline"])
    assert r["steps"] == 3 and r["value"] > 0 and r["ms_per_step"] > 0
    for k in FULL_ONLY + ("value_no_list_cut",):
        assert r.get(k) is not None, k
    assert r["roofline"]["bound"] == "hbm" and r["roofline"]["avg_launch_ms"] > 0
    assert r["config"]["R_eff"] > 0 and r["config"]["visible"] > 0
