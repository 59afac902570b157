"""bench.py's plain run and its --full run on one GPU: a plain run is setup, warm-up, the timed window and the line, with
every entry that takes runs of its own left null; --full adds them after the window, and the records of the last timed step
it dumps are the plain run's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "C2", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir), *extra], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines[:5]
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out_dir.glob("*.npy")}


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(fs, tmp_path):
    plain, d_plain = _bench(tmp_path / "plain")
    assert plain["full"] is False and plain["value"] > 0 and plain["steps"] == 3 and plain["warmup"] == 2
    assert plain["value"] == pytest.approx(plain["config"]["total_candidates"] / (plain["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("kernels_ms_per_step", "cpu_baseline", "parity", "ranked_step", "strong_scaling", "multi_gpu", "other_operating_points"):
        assert plain[k] is None, k
    assert plain["roofline"]["achieved"] is None and plain["roofline"]["m_tested_per_candidate"] > 0

    full, d_full = _bench(tmp_path / "full", "--full", "--cpu-seconds", "0", "--no-parity")
    assert full["full"] is True and full["value"] > 0
    assert full["kernels_ms_per_step"]["fs_fim_kernel"] > 0 and full["roofline"]["achieved"] > 0
    assert full["ranked_step"]["order_is_a_permutation"] and full["ranked_step"]["costs_ascending"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "config"):
        assert plain[k] == full[k], k

    # the same timed steps on the same inputs: the same records (info_ref may move by an ulp, bench.py "Outputs")
    assert sorted(d_plain) == sorted(d_full) == sorted(list(fs.RECORD_DTYPE.names) + ["logdet_singular"])
    for k, a in d_plain.items():
        if k == "info_ref":
            np.testing.assert_allclose(a, d_full[k], rtol=1e-6, atol=0)
        else:
            np.testing.assert_array_equal(a, d_full[k], err_msg=k)
