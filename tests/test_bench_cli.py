"""bench.py's launch contract: `--gpus N` means N ranks -- started by bench.py itself when no
launcher is around it -- and a world size that is not the one asked for is an error, never a silent 1-rank run.  A plain
run measures the headline alone, `--full` everything else, `--dump-outputs` writes what the timed steps computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(kw)
    return e


def test_world_size_mismatch_exits_2_before_touching_the_gpu():
    # a launcher that started 3 ranks for a run that asks for 2: refuse (checked before torch is even imported)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert "WORLD_SIZE=3" in r.stderr
    # ... and the default --gpus 1 under a 2-rank launcher likewise
    r = subprocess.run([sys.executable, BENCH], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])


@pytest.mark.gpu
def test_gpus_2_without_a_launcher_runs_two_ranks():
    """`python bench.py --gpus 2` (no torchrun around it): bench.py starts the two ranks as a child launcher; rehearsed
    on one card over gloo (DSL_BENCH_BACKEND), the library's slab driver on a host-staged transport."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--n3", "96", "--steps", "3", "--warmup", "2"],
                       env=_env(DSL_BENCH_BACKEND="gloo", DSL_BENCH_WATCHDOG_S="240"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["n_ranks_seen_by_rccl"] == 2
    assert out["slab_overflow"] == 0 and out["value"] > 0


def test_arguments_a_run_cannot_honour_exit_2_before_touching_the_gpu():
    for extra in (["--steps", "0"], ["--gpus", "2", "--dump-outputs", "never_written"]):
        r = subprocess.run([sys.executable, BENCH] + extra, env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (extra, r.returncode, r.stderr[-400:])
    assert not os.path.exists("never_written")


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline alone; --dump-outputs writes the state
    those steps left: the same bits as the same scene stepped through the binding with the same calls."""
    import numpy as np
    from dieselfluid_amd import SPHEngine, scenes
    n3, steps, warmup = 24, 4, 3
    r = subprocess.run([sys.executable, BENCH, "--n3", str(n3), "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(n3 ** 3 / out["ms_per_step"] / 1e3, rel=1e-2)
    assert not {"roofline", "kernels_ms", "exact", "developed", "skin", "cpu_baseline"} & set(out)
    p, pos = scenes.dambreak_scene(n3, math_mode=1)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    eng.wcsph_step(warmup)
    eng.wcsph_step(steps)
    for name in ("positions", "velocities", "densities"):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), eng.download(name).view(np.uint32)), name
    eng.close()


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements():
    r = subprocess.run([sys.executable, BENCH, "--full", "--n3", "24", "--steps", "3", "--warmup", "2",
                        "--developed-steps", "500", "--cpu-n3", "8"], env=_env(), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["kernel_events"].startswith("density / force kernels in the timed region")
    assert out["roofline"]["avg_ms"] > 0 and out["kernels_ms"]["density"] > 0
    assert out["exact"]["steps"] == 5 and out["developed"]["after_steps"] == 2 + 3 + 3 + 500
    assert out["skin"] is not None and out["cpu_baseline"]["value"] > 0
