"""bench.py as its own launcher (SURVEY.md §8(e) "Reporting"): `python bench.py --gpus N` without
a launcher around it must start N ranks itself, relay ONE result line that says n_gpus = N, and refuse a mismatch
between --gpus and WORLD_SIZE.  The GPU-free part of that is exercised here through --dry-run (gloo rendezvous + the
all-gather of dummy records; nothing is scored and no value is reported)."""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_launcher_command_is_one_process_per_gpu_under_torchrun():
    b = _bench_module()
    argv = ["--gpus", "4", "--steps", "7", "--scaling", "strong"]
    cmd = b.launcher_command(b.parse(argv), argv, port=12345)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "12345"
    assert cmd[-len(argv) - 1] == BENCH and cmd[-len(argv):] == argv          # the ranks get the same arguments


def test_defaults_are_the_headline_configuration():
    b = _bench_module()
    a = b.parse([])
    assert (a.gpus, a.workload, a.scaling) == (1, "C3", "weak") and a.dump_outputs is None
    # one stream, batches strictly back to back: with more contexts the FIM kernels of two batches share the CUs and the
    # per-launch durations behind `roofline` stop measuring the kernel
    assert a.pipeline == 1 and b.parse(["--pipeline", "2"]).pipeline == 2


def test_full_is_off_by_default():
    """A plain run times the headline alone; everything that takes runs of its own waits for --full, which travels to the
    ranks with the other arguments."""
    b = _bench_module()
    assert b.parse([]).full is False and b.parse(["--full"]).full is True
    argv = ["--gpus", "2", "--full"]
    assert b.launcher_command(b.parse(argv), argv, port=12345)[-1] == "--full"


def test_steps_is_the_number_of_timed_steps():
    """--steps K is the whole timed window (ms_per_step = window / K): nothing may stretch it to more steps, and it has one."""
    b = _bench_module()
    assert b.parse(["--steps", "7"]).steps == 7
    for argv in (["--steps", "0"], ["--repeats", "5"], ["--min-timed-seconds", "0.5"]):
        with pytest.raises(SystemExit):
            b.parse(argv)


def test_dump_outputs_writes_every_record_field(tmp_path):
    b = _bench_module()
    fs = importlib.import_module("fit-slam_amd")
    rng = np.random.default_rng(7)
    rec = np.zeros(1000, dtype=fs.RECORD_DTYPE)
    for k in fs.RECORD_DTYPE.names:
        t = rec.dtype[k]
        rec[k] = rng.standard_normal(1000) if t.kind == "f" else rng.integers(np.iinfo(t).min, np.iinfo(t).max, size=1000, endpoint=True)
    singular = rng.random(1000) < 0.1
    rec["logdet"][singular] = -np.inf                                   # a singular FIM (include/fitslam_frontier.h)
    b.dump_outputs(str(tmp_path / "out"), rec)
    for k in fs.RECORD_DTYPE.names:
        a = np.load(tmp_path / "out" / f"{k}.npy")
        assert a.dtype == (np.float32 if rec.dtype[k].kind == "f" else np.float64) and np.all(np.isfinite(a))
        if k == "logdet":
            np.testing.assert_array_equal(a, np.where(singular, 0.0, rec[k]).astype(np.float32))
        else:
            np.testing.assert_array_equal(a, rec[k])                  # integer fields exactly, uint32 flags included
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "logdet_singular.npy"), singular.astype(np.float32))
    assert not (tmp_path / "out" / "sample_index.npy").exists()


def test_dump_outputs_refuses_values_the_record_cannot_hold(tmp_path):
    """Only logdet may be -inf; a NaN anywhere, or +inf, is a broken record and must not be written as data."""
    b = _bench_module()
    fs = importlib.import_module("fit-slam_amd")
    for k, v in (("info_ref", np.nan), ("trace", np.inf), ("logdet", np.nan), ("logdet", np.inf)):
        rec = np.zeros(10, dtype=fs.RECORD_DTYPE)
        rec[k][3] = v
        with pytest.raises(ValueError, match=k):
            b.dump_outputs(str(tmp_path / "out"), rec)


def test_dump_outputs_samples_past_64_mb(tmp_path, monkeypatch):
    """Over the limit the same seeded rows of every field, their indices beside them; the same rows on every run."""
    b = _bench_module()
    fs = importlib.import_module("fit-slam_amd")
    rec = np.zeros(5000, dtype=fs.RECORD_DTYPE)
    rec["arrival"] = np.arange(5000)
    rec["info_ref"] = np.arange(5000) * 0.5
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", (1 << 16) + 100 * 60)  # room for 100 rows: 4 x 8 B + 4 x 4 B + logdet_singular + the index
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), rec)
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.shape == (100,) and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "arrival.npy"), idx)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "info_ref.npy"), (idx * 0.5).astype(np.float32))
    for k in list(fs.RECORD_DTYPE.names) + ["logdet_singular", "sample_index"]:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy"))
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= b.DUMP_LIMIT_BYTES


def test_two_ranks_are_spawned_and_rank0_line_is_relayed():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["dry_run"] is True and j["n_gpus"] == 2 and j["order_restored"] is True and j["value"] is None
    assert "dry-run rank 0/2" in r.stderr and "dry-run rank 1/2" in r.stderr              # both ranks ran


def test_gpus_must_match_world_size():
    env = _clean_env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE 1" in r.stderr and not r.stdout.strip()


def test_source_hash_tracks_the_kernel_sources():
    b = _bench_module()
    h = b.source_hash()
    assert len(h) == 16 and h == b.source_hash()
    # a counter profile is only replayed into the bench line when it names exactly these sources
    assert b.counter_profile("no-such-workload", 0) is None


def test_counter_profiles_are_replayed_only_for_what_they_measured():
    """bench.py copies counter-derived figures (HBM traffic, what limits the kernel) into its line only from a profile that was
    collected on exactly these kernel sources, this workload AND this visibility volume — the cone-off request runs another FIM
    worker instantiation, with counters of its own (profiles/pmc_summary_ref_request.json)."""
    b = _bench_module()
    for name, angle in (("pmc_summary.json", 1.0), ("pmc_summary_ref_request.json", 4.0)):
        j = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert float(j.get("fim_angle", 1.0)) == angle and j["workload"] == "C3"
        if j["source_hash"] == b.source_hash():                      # (a committed profile of older sources is simply not replayed)
            assert b.counter_profile("C3", 0, angle)["fim_angle"] == angle
    assert b.counter_profile("C3", 0, 2.5) is None and b.counter_profile("C5", 0, 1.0) is None and b.counter_profile("C3", 160, 1.0) is None
