"""bench.py keeps the driver's contract: one JSON line with the agreed keys; with --full, roofline and cpu_baseline objects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "tiny", "--steps", "2", "--warmup", "1", "--substeps", "30",
                          "--cpu-budget", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k, t in dict(metric=str, value=float, unit=str, n_gpus=int, steps=int, warmup=int, ms_per_step=float, higher_is_better=bool, scaling=str,
                     dtype=str, data=str, config=dict, roofline=dict, cpu_baseline=dict).items():
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["higher_is_better"]
    assert d["unit"] == "env-steps/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert "traffic" in r and r["achieved"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["unit"] == "env-steps/s" and isinstance(c["sample"], str) and c["value"] > 0
    assert abs(d["value"] - d["config"]["envs_per_gpu"] * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert set(d["phases"]) >= {"free", "contact", "note"} and d["phases"]["free"]["steps"] >= 1
    for k in ("traffic_source", "hbm_actual_frac", "valu_busy_frac", "algorithmic_bytes_per_launch", "avg_launch_us", "frac_shared_topology",
              "traffic_over_shared", "bound_in_practice"):
        assert k in r, k
    assert r["frac_shared_topology"] <= r["frac"] + 1e-12
    assert c["threads"]["physics"] == c["cores"] and "libr2s_cpu_baseline" in c["sample"]
    g = d["parity_gate"]
    assert g["passed"] and "flavour" in g and "threshold_flip_pixels" in g and g["hard_rgb_mismatch_pixels"] == 0, g
    cl = d["closed_loop_get_obs"]
    assert cl["env_steps_per_s"] > 0 and 0 < cl["ratio"] <= 1.05 and "re_rendered_batches" in cl, cl


def test_headline_schedule_contains_free_motion_finger_contact_and_live_self_collision():
    """the timed window of the headline workload must not be a contact-free best case.  A 2-env cut of
    configs[2] (same object, same 667 substeps, same action trace): the window starts in free motion; from the second step of the
    closing ramp (round 6: the commanded opening falls by 0.1 per step from six steps before the window's middle, so that the grasp
    latches from the stepper's own forces inside the window) particles are inside the fingers' collision margin, then live
    self-collision candidates (the toy's arms pressed together) and the graph flavour with the self-collision variant of the fused
    kernel plus the finishing code, and the grasp state machine latches: the window's last steps are the held grasp."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--envs", "2", "--steps", "16", "--warmup", "2", "--no-cpu-baseline", "--episodes", "0",
                          "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith("{")][-1])
    free, contact = d["phases"]["free"], d["phases"]["contact"]
    assert free["steps"] == 3 and contact["steps"] == 13            # the ramp starts at timed step 16 / 2 - 6 = 2, the pads arrive one step later
    assert contact["grasped_envs"] == 2, contact                    # ... and the grasp latches from the stepper's own forces
    assert free["mesh_contacts"] == 0 and free["self_collision_candidates"] == 0
    assert contact["mesh_contacts"] > 0 and contact["self_collision_candidates"] > 0, contact
    # SELF=true + finishing code (round 5: at the head of the next substep's launch, k_substep_pf; before: k_contact_finish as a launch of its own)
    assert any(",true," in f and ("k_contact_finish" in f or "k_substep_pf" in f) for f in contact["kernel_flavours"]), contact["kernel_flavours"]
    assert all(",true," not in f for f in free["kernel_flavours"]), free["kernel_flavours"]
    assert "sloth_32env" in d["config"]["workload"] and "grasp" in d["config"]["workload"]


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full) sets up, warms up, times --steps steps and prints the headline line, with nothing that takes work
    of its own (gate, other windows, per-kernel figures, CPU baseline, episodes).  --dump-outputs writes what the last timed step
    computed as float32 .npy within 64 MB, and two runs with the same arguments write the same arrays."""
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "tiny", "--steps", "3", "--warmup", "1", "--substeps", "30",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        runs.append((json.loads(lines[0]), d))
    r, d = runs[0]
    for k, t in dict(metric=str, value=float, unit=str, ms_per_step=float, higher_is_better=bool, dtype=str).items():
        assert isinstance(r[k], t), (k, r[k])
    assert r["steps"] == 3 and r["warmup"] == 1 and len(r["window"]["step_latency_ms"]["per_step"]) == 3
    assert abs(r["value"] - r["config"]["envs_per_gpu"] * 1000.0 / r["ms_per_step"]) < 1e-6 * r["value"]
    for k in ("parity_gate", "phases", "roofline", "raster", "cpu_baseline", "episodes", "synchronised_window", "throughput_mode", "closed_loop_get_obs"):
        assert k not in r, k
    files = sorted(os.listdir(d))
    assert files == sorted(f"{n}.npy" for n in r["outputs"]["arrays"]) and {"image_0.npy", "depth_0.npy", "particles_x.npy"} <= set(files)
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(d / f), np.load(runs[1][1] / f)
        assert a.dtype == np.float32 and a.size > 0 and np.array_equal(a, b, equal_nan=True), f
