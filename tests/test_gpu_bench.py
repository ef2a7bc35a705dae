"""GPU: the bench.py contract, as the driver invokes it.  One JSON line on stdout with the fields the driver reads;
N > 1 through `python -m torch.distributed.run` exactly as the driver launches it, on this one-GPU box with the
test knobs MVD_DIST_BACKEND=gloo / MVD_FORCE_DEVICE=0 (RCCL needs one GPU per rank; everything else is the same code).
The roofline object is measured with --full; a plain run carries the headline fields only."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}
REQUIRED = HEADLINE | {"roofline"}


def _one_json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines       # exactly ONE line on stdout
    return json.loads(lines[0])


def _check(d, n_gpus, steps, warmup, full=True):
    assert (REQUIRED if full else HEADLINE) <= set(d), (REQUIRED if full else HEADLINE) - set(d)
    assert d["n_gpus"] == n_gpus and d["steps"] == steps and d["warmup"] == warmup
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6
    assert "workload" in d["config"] and "model" not in d["config"]
    if not full:
        return
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0 < r["frac"] < 1


def test_bench_single_gpu_line():
    p = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _one_json_line(p.stdout)
    _check(d, 1, 2, 1)
    assert d["config"]["views_per_gpu"] == 16


def test_bench_plain_run_times_the_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run (no --full) measures the headline figure only, and --dump-outputs writes what the last timed step returned:
    x_prev of all 16 views, float32, identical from run to run with the same arguments."""
    runs = []
    for tag in ("a", "b"):
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / tag)], cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        d = _one_json_line(p.stdout)
        _check(d, 1, 3, 1, full=False)
        assert not {"roofline", "families", "cpu_baseline", "ddim50_wall_s"} & set(d), sorted(d)
        assert os.listdir(tmp_path / tag) == ["x_prev.npy"]
        x = np.load(tmp_path / tag / "x_prev.npy")
        assert x.dtype == np.float32 and x.shape == (1, 16, 4, 32, 32) and np.isfinite(x).all() and x.std() > 0
        runs.append(x)
        print(f"[property] plain bench run {tag}: {d['ms_per_step']:.2f} ms per step")
    assert np.array_equal(runs[0], runs[1])


def test_bench_long_run_starts_a_new_trajectory_every_50_steps(tmp_path):
    """Many timed steps are consecutive 50-step DDIM trajectories, each from x_T: the run stays finite however long it is, and
    its last step returns what the same position of the first trajectory returns (310 steps vs 10, both after 1 warmup step)."""
    outs = []
    for steps in (10, 310):
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs",
                            str(tmp_path / str(steps))], cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        _check(_one_json_line(p.stdout), 1, steps, 1, full=False)
        outs.append(np.load(tmp_path / str(steps) / "x_prev.npy"))
    assert np.isfinite(outs[1]).all() and np.array_equal(outs[0], outs[1])


def test_bench_two_ranks_as_the_driver_launches_it(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MVD_DIST_BACKEND="gloo", MVD_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _one_json_line(p.stdout)        # rank 0 only
    _check(d, 2, 2, 1)
    assert d["config"]["views_per_gpu"] == 8 and d["scaling"] == "strong"
    x = np.load(tmp_path / "x_prev.npy")  # both ranks' views, gathered on rank 0
    assert x.shape == (1, 16, 4, 32, 32) and np.isfinite(x).all()


def test_bench_line_carries_counter_traffic_when_the_pmc_summary_is_of_this_build():
    """roofline.traffic comes from profiles/pmc_traffic.json (rocprofv3 --pmc passes) and is reported only when that file is
    stamped with the hash of THIS tree's library sources: a committed summary of another build must read as null, a current
    one as a number."""
    sys.path.insert(0, ROOT)
    from morphablediffusion_amd.lib import csrc_sha16
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        pmc = json.load(f)
    p = subprocess.run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    r = _one_json_line(p.stdout)["roofline"]
    current = pmc.get("csrc_sha16") == csrc_sha16() and r["kernel"] in pmc["bytes_per_launch"]
    print(f"[property] pmc_traffic.json stamp {pmc.get('csrc_sha16')} vs sources {csrc_sha16()}: traffic = {r['traffic']}")
    assert (r["traffic"] is not None) == current
    if current:
        assert r["traffic"] > 0


def test_bench_train_at_config3_per_gpu_shape():
    """BASELINE configs[3] at the PER-GPU shape its stated scale implies (batch 140 over 8 GPUs = 18 samples per GPU, FaceScape's
    bilinear topology = 26317 vertices per mesh, a new mesh per sample, bf16): the complete training step -- conditioner and UNet
    forward, loss, both backward passes, AdamW, re-pack -- runs at full width with finite, non-increasing-by-much losses and no
    skipped optimiser step.  (Parity of that step against the reference is tests/test_gpu_train*.py at 2 - 4 samples.)"""
    env = dict(os.environ, MVD_DTYPE="bf16")
    p = subprocess.run([sys.executable, "bench.py", "--config", "train", "--train-batch", "18", "--train-vertices", "26317",
                        "--steps", "2", "--warmup", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _one_json_line(p.stdout)
    assert d["unit"] == "samples/s" and d["dtype"] == "bf16" and d["n_gpus"] == 1 and d["scaling"] == "weak"
    assert d["config"]["batch_per_gpu"] == 18 and d["config"]["mesh_vertices_after_voxel_dedup"] > 15000
    first, last = d["loss_first_last"]
    assert 0.5 < first < 2.0 and 0.5 < last < 2.0, d["loss_first_last"]   # MSE of a random-init UNet against unit noise
    assert d["optimizer_steps_skipped"] == 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 18.0) < 1e-6
    print(f"[property] config-3 per-GPU shape: {d['ms_per_step']:.1f} ms per step, {d['value']:.1f} samples/s, "
          f"losses {first:.4f} -> {last:.4f}")
