"""GPU tests of bench.py's one-GPU line at a small size: a plain run prints the headline figure and what the timed steps leave
behind, and nothing that takes work of its own; --full adds the counted walk launch, the CPU baseline with its force check, the
resident-step and the SPH figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--ngrid", "32", "--steps", "2", "--warmup", "1"]
                       + list(extra), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE), out.keys()
    assert out["unit"] == "particle-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert abs(out["value"] - 32**3 / (1e-3 * out["ms_per_step"])) < 1e-6 * out["value"]
    k = out["kernels"]
    assert k["tree_walk_ms"] > 0 and k["tree_interactions_per_target"] > 0 and k["pm_ms"]["total"] > 0
    # nothing that needs a run of its own
    for key in ("cpu_baseline", "force_error", "roofline_sph_density", "roofline_sph_hydro"):
        assert key not in out, key
    for key in ("tree_walk_with_counters_ms", "tree_lane_efficiency", "resident_full_step_ms", "find_timesteps_ms", "fof_ms",
                "sph_density_iteration_ms", "c3_force_step_ms"):
        assert key not in k, key
    for name in ("index", "gravpm", "pm_potential", "tree_accel", "tree_potential", "ninteractions"):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.shape[0] == 32**3 and np.all(np.isfinite(a)), name


def test_bench_full_run_adds_the_extra_figures():
    out = _bench("--full", "--sph-ngrid", "16")
    assert all(k in out for k in HEADLINE), out.keys()
    assert out["value"] > 0
    k = out["kernels"]
    assert k["tree_walk_with_counters_ms"] > 0 and 0 < k["tree_lane_efficiency"] <= 1
    assert out["cpu_baseline"]["value"] > 0
    fe = out["force_error"]
    assert fe["rms_rel_tree_force_error_vs_cpu_walk"] < fe["tolerance_north_star"], fe
    assert k["resident_full_step_ms"] > 0 and k["find_timesteps_ms"] > 0 and k["fof_ms"] > 0
    assert k["sph_density_iteration_ms"] > 0 and k["c3_force_step_ms"] > 0
    assert out["roofline_sph_density"]["achieved"] > 0 and out["roofline_sph_hydro"]["achieved"] > 0
