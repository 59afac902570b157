#!/usr/bin/env python3
"""What the REFERENCE grid search (fs_set_grid_search) costs on the MI355X against the converged search and against
the per-frontier loop a caller had before.

    python tools/grid_reference_probe.py [--out DIR] [--reps K]        # writes DIR/astar_gpu_ref2d.json (default profiles/planner)

REF2D (512^2), the robot of tools/planner_probe.py (the free cell, of 8 drawn, whose field reaches the most goal cells), 50 and
2 000 frontiers, in one process on one build:

    reference   fs_plan_paths under FS_GRID_SEARCH_REFERENCE: one wave per distinct goal cell, then the descents
    converged   fs_plan_paths under FS_GRID_SEARCH_CONVERGED with a new robot cell every call (no cached field)
    cpu_loop    the restatement's per-frontier loop on one core, planner_ref.plan(leg=REFERENCE_ASTAR)

Host wall time around calls that end in a synchronisation; medians of K calls (default 20) after a warm-up, cpu_loop of 3.  With
the counters of the reference calls: waves, slot batches, waves on the cycle budget, waves that dropped a push, chunks run again.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import planner_ref as R  # noqa: E402
from planner_probe import RES, med_ms, ref2d  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planner"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import torch  # noqa: F401  (one HIP runtime, loaded before the library, as bench.py does)
    fs = importlib.import_module("fit-slam_amd")
    w, pose, (rx, ry) = ref2d(2000)
    cells = w.cells[0]
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    free_x, free_y = R.free_cells(cells, np.random.default_rng(9), a.reps + 1)
    poses = [R.robot_pose(w.origin, RES, int(x), int(y), 0.7) for x, y in zip(free_x, free_y)]
    res = {"what": "REF2D (512^2), fs_plan_paths, ms, wall time of the host call, median of %d calls after a warm-up; cpu_loop: "
                   "planner_ref.plan(leg=REFERENCE_ASTAR) on one core, median of 3" % a.reps,
           "robot_cell": [rx, ry]}
    for n in (50, 2000):
        goals = w.goals[:n]
        row = {}
        sc.set_grid_search("reference")
        got = sc.plan_paths(pose, goals)                                   # warm-up (sizes the slots)
        xs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = sc.plan_paths(pose, goals)
            xs.append(time.perf_counter() - t0)
        row["reference_ms"] = med_ms(xs)
        row["reference_achievable"] = int(got["achievable"].sum())
        row["counters"] = dict(waves=sc.get_counter(1037), batches=sc.get_counter(1038), on_cycle_budget=sc.get_counter(1039),
                               dropped_a_push=sc.get_counter(1040), chunks_run_again=sc.get_counter(1041))
        sc.enable_kernel_timing(True)
        sc.plan_paths(pose, goals)
        row["reference_kernel_ms"] = {"waves": sc.kernel_time(7)[0], "descents": sc.kernel_time(8)[0]}
        sc.enable_kernel_timing(False)
        sc.set_grid_search("converged")
        sc.plan_paths(poses[-1], goals)                                    # warm-up
        xs = []
        for i in range(a.reps):
            t0 = time.perf_counter()
            conv = sc.plan_paths(poses[i], goals)                          # a new robot cell: a new field every call
            xs.append(time.perf_counter() - t0)
        row["converged_new_field_ms"] = med_ms(xs)
        conv = sc.plan_paths(pose, goals)
        row["converged_achievable"] = int(conv["achievable"].sum())
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})      # one core for the host loop
        xs = []
        for _ in range(3):
            t0 = time.perf_counter()
            cpu = R.plan(cells, w.origin, RES, pose, goals, leg=R.REFERENCE_ASTAR)
            xs.append(time.perf_counter() - t0)
        row["cpu_loop_ms"] = med_ms(xs)
        row["equal_to_cpu_loop"] = all(got[k].tobytes() == cpu[k].tobytes() for k in ("path_length", "path_length_m", "path_heading", "achievable"))
        row["speedup_vs_cpu_loop"] = round(row["cpu_loop_ms"] / row["reference_ms"], 2)
        res[f"frontiers_{n}"] = row
    sc.close()
    json.dump(res, open(os.path.join(a.out, "astar_gpu_ref2d.json"), "w"), indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
