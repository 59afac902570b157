"""What only a box with two (or more) physical GPUs can show — skipped on the one-GPU leases this build is developed on, the
first real evidence on the driver's multi-GPU node:

  * fs_multi_create({0, 1}): the records of a list scored half on each device equal a single context's (north_star's partition,
    the reference's in-process call shape: DEP/src/ExplorationBT.cpp:376-410);
  * bench.py --gpus 2 through its own launcher (the driver's command shape): two ranks over RCCL, one all-gather per step,
    n_gpus == 2 in the line, the weak value AND the strong-scaling block (160 k candidates split over the ranks), each gathered
    list gated against the oracle in every rank's share, both ranks named in the log;
  * fs_multi_get_frontier_costs on {0, 1}: member 1's block over the peer link (or the bounce) into the list on GPU 0.

torch.cuda.device_count() does not initialise the GPU on this image, so collecting this module is harmless anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_devices():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


# FS_REHEARSE_TWO_DEVICES=1 on a one-GPU box: the two fs_multi tests below run with BOTH members on device 0 — not evidence of anything
# a second GPU would show (test_multi_device.py already covers [0, 0]); it only proves that these never-run test bodies execute.
REHEARSE = bool(os.environ.get("FS_REHEARSE_TWO_DEVICES")) and _n_devices() < 2
DEVICES = (0, 0) if REHEARSE else (0, 1)
two_gpus = pytest.mark.skipif(_n_devices() < 2 and not REHEARSE, reason="needs two physical GPUs")
two_real_gpus = pytest.mark.skipif(_n_devices() < 2, reason="needs two physical GPUs")


@two_gpus
def test_fs_multi_on_two_physical_devices_equals_a_single_context(fs):
    import importlib.util
    spec = importlib.util.spec_from_file_location("multi_device_helpers", os.path.join(ROOT, "tests", "test_multi_device.py"))
    helpers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helpers)
    _same_records, _stage = helpers._same_records, helpers._stage
    w = fs.synth.make_workload("C2")
    kw = dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
              robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    one = fs.FrontierScorer(device=0)
    mx1 = _stage(one, w, kw)
    want = one.score_candidates(w.goals, w.frontier_size, w.blacklisted)
    want_arr = one.score_arrival(w.goals, w.frontier_size, w.blacklisted)
    one.close()
    m = fs.MultiScorer(devices=DEVICES)
    assert _stage(m, w, kw) == mx1
    for _ in range(2):
        _same_records(m.score_candidates(w.goals, w.frontier_size, w.blacklisted), want)
    got_arr = m.score_arrival(w.goals, w.frontier_size, w.blacklisted, n_rays_total=int(want_arr["ray_counts"][0].size))
    for k in ("arrival", "argmax", "status", "achievable", "yaw"):
        np.testing.assert_array_equal(got_arr[k], want_arr[k], err_msg=k)
    np.testing.assert_array_equal(got_arr["ray_counts"].reshape(want_arr["ray_counts"].shape), want_arr["ray_counts"])
    # the second device really worked: its context counted landmark tests of its own
    import ctypes as C
    L = fs.load_library()
    v = C.c_int64()
    # (counter 0 = landmark tests performed, a running total; 10 / 11 are the sort's accumulators and are cleared by every sorted call —
    # the rehearsal of this body on one GPU, FS_REHEARSE_TWO_DEVICES, caught an assertion on 11 that could never have held)
    assert L.fs_get_counter(m.member(1), 0, C.byref(v), 0) == 0 and v.value > 0
    m.close()


@two_gpus
def test_fs_multi_get_frontier_costs_gathers_over_the_peer_link(fs):
    """The device_count() >= 2 twin of test_multi_get_frontier_costs_equals_one_context: member 1's block travels with
    hipMemcpyPeerAsync from GPU 1 into the gathered list on GPU 0 (or, where the runtime refuses peer access, through page-locked
    memory — fs_multi_gather_mode says which, and both must give the one-context results)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("multi_device_helpers", os.path.join(ROOT, "tests", "test_multi_device.py"))
    helpers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helpers)
    w = fs.synth.make_workload("C2")
    n = w.goals.shape[0]
    kw = dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
              robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    plen, phead = helpers._path_columns(n)
    one = fs.FrontierScorer(device=0)
    mx = helpers._stage(one, w, kw)
    one.set_arrival_limits(4000.0, mx["min_gt"])
    want = one.get_frontier_costs(w.goals, plen, phead, w.frontier_size, w.blacklisted, with_fim=True)
    one.close()
    m = fs.MultiScorer(devices=DEVICES)
    helpers._stage(m, w, kw)
    m.set_arrival_limits(4000.0, mx["min_gt"])
    auto = m.gather_mode()
    assert auto in (1, 2), auto
    for forced in (0, 2):                                            # what set-up chose, then the bounce
        m.set_option("multi.gather", forced)
        for _ in range(2):
            got = m.get_frontier_costs(w.goals, plen, phead, w.frontier_size, w.blacklisted, with_fim=True)
            helpers._same_records(got["records"], want["records"])
            for k in ("weighted_cost", "arrival_utility", "distance_utility", "order"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    m.close()


@two_real_gpus
def test_bench_two_ranks_over_rccl():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # the driver's own command shape: weak scaling as `value`, the strong-scaling block behind it in the same line
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                        "--warmup", "2", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["value"] > 0
    assert j["config"]["total_candidates"] == 40000
    assert j["parity"]["ok"], j["parity"]
    st = j["strong_scaling"]
    assert st["total_candidates"] == 160000 and st["candidate_goals_per_s"] > 0 and len(st["per_rank_ms_per_step"]) == 2
    assert st["parity"]["ok"], st["parity"]
    assert "rank 0/2" in r.stderr and "rank 1/2" in r.stderr
    mg = j["multi_gpu"]
    assert len(mg["per_rank_ms_per_step"]) == 2 and mg["all_gather_ms"] > 0 and mg["barrier_skew_ms"] >= 0
    assert j["ranked_step"]["order_is_a_permutation"] and j["ranked_step"]["costs_ascending"] and j["ranked_step"]["range_error"] == 0
