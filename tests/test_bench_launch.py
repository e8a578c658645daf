"""bench.py's launch layer: `--gpus N` must measure N ranks however the script is started.
CPU: the self-launch, the rendezvous and the collectives of an N-rank run with the device work left out (gloo);
GPU (one device): two ranks sharing device 0 (gloo: RCCL refuses two ranks on one device), the strong-scaling cut and the
single-process mode over nyx_hip_propagate_batch_sharded."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "NYX_BENCH_SELF_LAUNCHED"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, env=e, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


@pytest.mark.parametrize("n", [2, 3])
def test_self_launch_starts_n_ranks(n):
    p, line = _run(["--gpus", str(n), "--selftest-launch"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["n_gpus"] == n and line["ranks"] == n and line["self_launched"] is True
    assert line["gathered_sum"] == 28.0 * sum(range(1, n + 1))        # every rank's piece arrived at rank 0
    assert line["max_time"] == 0.5 + (n - 1)                           # max over ranks
    assert line["per_rank_kernel_ms"] == [10.0 * (r + 1) for r in range(n)]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("{")]) == 1   # ONE line, from rank 0


def test_a_failing_rank_ends_the_run_instead_of_hanging_it():
    """The launcher polls ALL its ranks: rank 1 dies before the rendezvous, rank 0 waits in it - the run must end with rank 1's code."""
    import time
    t0 = time.time()
    p, line = _run(["--gpus", "2", "--selftest-launch"], env={"NYX_BENCH_SELFTEST_FAIL_RANK": "1"}, timeout=120)
    assert p.returncode == 3 and line is None and time.time() - t0 < 60


def test_world_size_must_agree_with_gpus():
    p, line = _run(["--gpus", "2", "--selftest-launch"], env={"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and line is None and "WORLD_SIZE=3" in p.stderr


def test_stale_traffic_is_not_quoted(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    from kernel_stamp import kernel_source_stamp
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    import kernel_stamp
    real = kernel_source_stamp()
    monkeypatch.setattr(kernel_stamp, "kernel_source_stamp", lambda root=None: real)
    rec = {"config": 2, "n": 10000, "hours": 24.0, "degree": 70, "hbm_bytes_per_launch": 1.0e11}
    (prof / "roundXX_cfg2_hbm_traffic.json").write_text(json.dumps(rec))                       # unstamped: a pass of an unknown build
    t, src = bench.measured_traffic(2, 10000, 24.0, 70)
    assert t is None and src.startswith("stale:")
    (prof / "roundXY_cfg2_hbm_traffic.json").write_text(json.dumps(dict(rec, kernel_source_stamp="0123456789abcdef")))
    t, src = bench.measured_traffic(2, 10000, 24.0, 70)
    assert t is None and "0123456789abcdef" in src
    (prof / "roundXZ_cfg2_hbm_traffic.json").write_text(json.dumps(dict(rec, kernel_source_stamp=real)))
    t, src = bench.measured_traffic(2, 10000, 24.0, 70)
    assert t == 1.0e11 and src.endswith("roundXZ_cfg2_hbm_traffic.json")
    assert bench.measured_traffic(3, 5000, 720.0, 0) == (None, None)


SMALL = ["--n", "256", "--hours", "0.25", "--degree", "8", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-dense-output", "--no-host-call"]


@pytest.mark.gpu
def test_two_ranks_on_one_device():
    p, line = _run(["--gpus", "2", "--oversubscribe", "--backend", "gloo", *SMALL])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["n_gpus"] == 2 and line["launch"] == "self-launched ranks" and line["backend"] == "gloo"
    assert line["config"]["trajectories_total"] == 512 and len(line["per_rank_kernel_ms"]) == 2 and line["all_gather_ms"] is not None
    assert line["value"] > 0 and line["scaling"] == "weak"


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [[], ["--config", "4", "--n", "64"]])
def test_the_rccl_path_runs_with_one_rank(cfg):
    """The N > 1 launches of the driver are the first time RCCL sees this script; `--force-collectives` issues every collective of
    a step (all-gather of the final states, all-reduce of the 55 moments, the reductions of the report) on a one-rank nccl group,
    on the tensors and streams the N-rank run uses.  Plain kernel and the covariance-mapping loop."""
    p, line = _run(["--gpus", "1", "--force-collectives", *SMALL, *cfg])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["n_gpus"] == 1 and line["launch"] == "single rank, collectives forced"
    assert line["backend"] == "nccl" and line["rccl_ranks"] == 1 and line["all_gather_ms"] is not None and line["all_gather_ms"] >= 0.0
    if not cfg:
        assert line["ensemble_moments"]["count"] == 256.0 and line["ensemble_moments"]["trace_cov_pos_km2"] > 0.0


@pytest.mark.gpu
def test_strong_scaling_cuts_one_ensemble():
    p, line = _run(["--gpus", "2", "--oversubscribe", "--backend", "gloo", "--scaling", "strong", *SMALL[:1], "257", *SMALL[2:]])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["scaling"] == "strong" and line["config"]["trajectories_total"] == 257 and line["config"]["trajectories_per_gpu"] == 129


@pytest.mark.gpu
def test_single_process_mode_drives_the_sharded_entry():
    p, line = _run(["--gpus", "2", "--oversubscribe", "--single-process", *SMALL])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["launch"] == "single-process" and line["contexts"] == 2 and line["config"]["trajectories_total"] == 512
    assert len(line["per_rank_kernel_ms"]) == 2 and line["value"] > 0


@pytest.mark.gpu
def test_plain_run_leaves_the_side_measurements_to_full():
    """A plain run is the headline alone; `--full` adds the measurements beside it (here the two device ones)."""
    base = [a for a in SMALL if not a.startswith("--no-")]
    p, line = _run(["--gpus", "1", *base])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert not {"host_call", "dense_output", "other_configs", "strong_scaling_projection", "cpu_baseline"} & set(line)
    p, line = _run(["--gpus", "1", *base, "--full", "--no-cpu-baseline"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["host_call"]["value"] > 0 and line["dense_output"]["states_written"] > 0 and "cpu_baseline" not in line


@pytest.mark.gpu
def test_rccl_refuses_shared_device_with_a_message():
    import torch
    if torch.cuda.device_count() > 1:
        pytest.skip("needs a box where two ranks must share a device")
    p, line = _run(["--gpus", "2", "--oversubscribe", *SMALL])
    assert p.returncode != 0 and line is None


def test_dump_outputs_writes_float64_and_keeps_under_the_limit(tmp_path, monkeypatch):
    """`--dump-outputs`: one float64 .npy per array; past the size limit a fixed, seeded sample of trajectories, the same every run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from nyx_amd import _abi
    n = 1000
    st, stats = _abi.StateBatch(n), _abi.StatsBatch(n)
    st.x_km[:] = np.arange(n)
    st.epoch_ns[:] = 757_339_200 * 10**9 + np.arange(n)
    stats.n_evals[:] = 3 * np.arange(n)
    mom = np.linspace(0.0, 1.0, 55)
    bench.dump_outputs(str(tmp_path / "all"), st, stats, {"ensemble_moments": mom}, epoch0_ns=757_339_200 * 10**9)
    got = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(got) >= {*_abi.F64_FIELDS, "epoch_offset_ns", "step_ns", "status", "n_evals", "ensemble_moments"}
    assert "sample_index" not in got and all(v.dtype == np.float64 for v in got.values())
    assert (got["x_km"] == np.arange(n)).all() and (got["epoch_offset_ns"] == np.arange(n)).all() and (got["ensemble_moments"] == mom).all()

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 1024)
    for k in ("a", "b"):
        bench.dump_outputs(str(tmp_path / k), st, stats, {"ensemble_moments": mom}, epoch0_ns=757_339_200 * 10**9)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").iterdir()}
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 * 1024 + 128 * len(a)   # (+ the .npy headers)
    idx = a["sample_index"].astype(np.int64)
    assert 0 < len(idx) < n and (np.diff(idx) > 0).all()
    assert (a["x_km"] == idx).all() and (a["n_evals"] == 3 * idx).all() and (a["ensemble_moments"] == mom).all()
    assert all((a[k] == b[k]).all() for k in a)


@pytest.mark.gpu
def test_dump_outputs_are_the_same_whatever_the_step_count(tmp_path):
    """Same arguments, same inputs: the last timed step's outputs do not depend on how many steps ran before it."""
    import numpy as np
    got = []
    for k, steps in (("one", "1"), ("two", "2")):
        args = list(SMALL)
        args[args.index("--steps") + 1] = steps
        p, line = _run(["--gpus", "1", *args, "--dump-outputs", str(tmp_path / k)])
        assert p.returncode == 0, p.stderr[-2000:]
        assert line["steps"] == int(steps) and line["ms_per_step"] > 0
        got.append({q.stem: np.load(q) for q in (tmp_path / k).iterdir()})
    a, b = got
    assert a["x_km"].shape == (256,) and (a["status"] == 0).all() and (a["epoch_offset_ns"] == 900 * 10**9).all()
    assert a["ensemble_moments"][0] == 256.0
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
