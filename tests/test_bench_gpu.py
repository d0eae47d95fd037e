"""GPU tests (-m gpu) that EXECUTE bench.py's multi-rank branches on the one-GPU box, so that the round-end 8-GPU run is not
their first automated execution: the process group, OPT_WORKGROUPS = CUs - 8, the bucketed asynchronous MAX all-reduce, the
evidence keys, strong scaling (one grid dealt to the ranks: SURVEY.md 8e), and the level-sharded stream / e2e forms
(BASELINE.json configs[3] / [4]).  Two ranks share cuda:0 over gloo (RCCL refuses two ranks on one device); RCCL itself runs
with one rank (--force-dist).  Numbers from these runs mean nothing; winners are checked inside bench.py (it exits non-zero on a
wrong one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--steps", "5", "--warmup", "2", "--clock-warmup-ms", "0", "--no-cpu-baseline", "--no-call-site"]
TWO = ["--gpus", "2", "--backend", "gloo", "--all-on-device0"]


def bench(*argv, timeout=420):
    if torch.cuda.device_count() < 1:  # (counting devices does not open the GPU: the ranks need the box's few process slots)
        pytest.fail("gpu tests need a HIP device")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (argv, r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_default_line_is_the_contracts_blocking_metric_with_throughput_beside_it():
    d = bench(*QUICK)
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["steps"] == 5 and d["unit"] == "evals/s"
    assert "blocking" in d["metric"] and d["step_mode"].startswith("blocking call per step")
    assert abs(d["value"] - 729 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert abs(d["value"] - d["blocking_call_evals_per_s"]) <= 1e-6 * d["value"]
    assert d["value"] > 50000 and d["throughput_evals_per_s"] > 50000     # BASELINE.json's target, by two orders of magnitude
    # (over 2,000 steps the back-to-back figure is the larger one, 9.2 M against 8.4 M; over these 5 cold steps either may be)
    assert d["collective_ranks"] == 1 and d["rccl"] is False
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["kernel"] == "nmi_grid_kernel" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9


def test_dump_outputs_hold_the_last_steps_winner_in_either_step_mode(tmp_path):
    """--dump-outputs writes what the last timed step returned; the inputs are seeded, and the blocking call and the
    back-to-back steps return the same winner to the bit."""
    got = {}
    for mode in ("blocking", "throughput"):
        d = bench(*QUICK, f"--{mode}", "--dump-outputs", str(tmp_path / mode))
        assert d["steps"] == 5 and d["ms_per_step"] > 0
        got[mode] = {n: np.load(tmp_path / mode / f"{n}.npy") for n in ("best_index", "best_score")}
        assert sorted(os.listdir(tmp_path / mode)) == ["best_index.npy", "best_score.npy"]
    for g in got.values():
        assert g["best_index"].dtype == np.float64 and g["best_score"].dtype == np.float32
        assert g["best_index"].tolist() == [13 * 27 + 13] and 0 < g["best_score"][0] <= 1   # the planted centre cell
    assert (got["blocking"]["best_score"].view(np.uint32) == got["throughput"]["best_score"].view(np.uint32)).all()


def test_rccl_branch_with_one_rank():
    d = bench("--force-dist", *QUICK)
    assert d["n_gpus"] == 1 and d["collective_ranks"] == 1 and d["rccl"] is True and d["backend"].startswith("nccl")
    assert "throughput" in d["metric"] and d["config"]["collective"].startswith("MAX all-reduce")


@pytest.mark.parametrize("config,cells", [("c2", 729), ("c4", 4096)])
def test_two_ranks_weak(config, cells):
    d = bench("--config", config, *TWO, *QUICK)
    assert d["n_gpus"] == 2 and d["collective_ranks"] == 2 and d["rccl"] is False and d["backend"] == "gloo"
    assert d["scaling"] == "weak" and d["config"]["candidates_total"] == 2 * cells and d["config"]["candidates_per_gpu"] == cells
    assert d["device_ordinals"] == [0, 0]


@pytest.mark.parametrize("config,cells,share", [("c2", 729, 14 * 27), ("c3", 4096, 32 * 64)])
def test_two_ranks_strong(config, cells, share):
    d = bench("--config", config, "--scaling", "strong", *TWO, *QUICK)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["candidates_total"] == cells and d["config"]["candidates_per_gpu"] == share   # rank 0's block
    assert abs(d["value"] - cells / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]


def test_four_ranks_strong():
    """27 renders over 4 ranks: blocks of 7, 7, 7, 6 renders x 27 warps (over 8 ranks a rank has 81 or 108 candidates and runs
    nmi_pix_kernel: tests/test_pix_kernel.py covers that kernel behind the shard entry points).  Four ranks, not eight: the box
    admits six processes on its GPU, and the test runner is one of them."""
    d = bench("--config", "c2", "--scaling", "strong", "--gpus", "4", "--backend", "gloo", "--all-on-device0", *QUICK)
    assert d["n_gpus"] == 4 and d["config"]["candidates_per_gpu"] == 7 * 27 and d["config"]["candidates_total"] == 729
    assert d["device_ordinals"] == [0, 0, 0, 0]


@pytest.mark.parametrize("config", ["stream", "e2e"])
def test_level_sharded_forms_two_ranks(config):
    d = bench("--config", config, "--shard", "level", *TWO, "--keyframes", "4")
    assert d["n_gpus"] == 2 and d["collective_ranks"] == 2 and d["unit"] == "keyframes/s" and d["scaling"] == "strong"
    assert "level-sharded" in d["config"]["parallelism"]


def test_level_sharded_e2e_mesh_two_ranks():
    d = bench("--config", "e2e", "--map", "mesh", "--shard", "level", *TWO, "--keyframes", "3")
    assert d["n_gpus"] == 2 and d["map"] == "mesh"
