#!/usr/bin/env python3
"""What fs_plan_paths_information costs on the MI355X against what the library offered before it.

    python tools/path_information_probe.py time  [--out DIR] [--reps K]   # writes DIR/ref2d.json (default profiles/pathinfo)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/path_information_probe.py trace      # the per-kernel split

REF2D (512^2), 100 000 landmarks, 50 and 2 000 frontiers, the robot on a well-placed cell, allow_unknown = 1, the default sampling
(1.5 m / 10 points), both visibility requests.  Three routes, alternated call by call inside one process after a warm-up of each:

    dedup      the call, one pose record per distinct (from cell, to cell)                       ("pathinfo.dedup" 1)
    every      the call, one pose record per way point                                            ("pathinfo.dedup" 0)
    by_hand    fs_plan_paths, the way points from the CPU restatement (tests/pathinfo_ref), fs_score_fim(info_only) over all of
               them: what a caller had to do before — the path points never left the device, so the host plans again

Host wall time around calls that end in a synchronisation; medians.  `trace` makes a few calls of the first two routes at 2 000
frontiers and nothing else, for a profiler run of its own.
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
import pathinfo_maps as M  # noqa: E402
import pathinfo_ref as P  # noqa: E402  (the restatement: the CPU leg of `by_hand`)
import planner_ref as R  # noqa: E402

RES = M.RES
VIS = ((14.0, 1.0), (14.0, 4.0))


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def setup(n_landmarks):
    import torch  # noqa: F401  (one HIP runtime, loaded before the library, as bench.py does)
    fs = importlib.import_module("fit-slam_amd")
    w = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=n_landmarks)
    cells = np.ascontiguousarray(w.cells[0])
    rx, ry = R.well_placed_robot(cells, np.random.default_rng(7))
    pose = R.robot_pose(w.origin, RES, rx, ry, 0.3)
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(w.cells, w.origin, RES)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    return sc, cells, w.origin, pose


def routes(sc, cells, origin, pose, goals, ach):
    def dedup():
        sc.set_option("pathinfo.dedup", 1)
        return sc.plan_paths_information(pose, goals, achievable_in=ach, allow_unknown=True)

    def every():
        sc.set_option("pathinfo.dedup", 0)
        return sc.plan_paths_information(pose, goals, achievable_in=ach, allow_unknown=True)

    split = {"plan": [], "waypoints_cpu": [], "score": []}

    def by_hand():
        t0 = time.perf_counter()
        sc.plan_paths(pose, goals, achievable_in=ach, allow_unknown=True)
        t1 = time.perf_counter()
        wp = P.waypoints(cells, origin, RES, pose, goals, achievable_in=ach, allow_unknown=True)
        poses = np.zeros((wp["xyyaw"].shape[0], 7))
        poses[:, :2] = wp["xyyaw"][:, :2]
        poses[:, 3:] = P.yaw_to_quat(wp["xyyaw"][:, 2])
        t2 = time.perf_counter()
        sc.score_fim(poses, info_only=True)
        t3 = time.perf_counter()
        split["plan"].append(t1 - t0); split["waypoints_cpu"].append(t2 - t1); split["score"].append(t3 - t2)
    return {"dedup": dedup, "every": every, "by_hand": by_hand}, split


def run_time(out_dir, reps, n_landmarks):
    sc, cells, origin, pose = setup(n_landmarks)
    res = {"what": f"REF2D (512^2), {n_landmarks} landmarks, allow_unknown 1, 1.5 m / 10 points; host wall ms around calls that end in a "
                   f"synchronisation, median of {reps} after one warm-up call per route, the routes alternated call by call",
           "routes": {"dedup": "fs_plan_paths_information, pathinfo.dedup 1", "every": "fs_plan_paths_information, pathinfo.dedup 0",
                      "by_hand": "fs_plan_paths + way points on the CPU (restatement) + fs_score_fim(info_only)"},
           "cases": []}
    for n in (50, 2000):
        goals, ach = M.goals(cells, origin, 11 + n, n)
        for vis in VIS:
            sc.set_fim_params(*vis)
            fn, split = routes(sc, cells, origin, pose, goals, ach)
            for f in fn.values():                     # warm-up: every buffer sized, the field cached
                f()
            for v in split.values():
                v.clear()
            t = {k: [] for k in fn}
            for _ in range(reps):
                for k, f in fn.items():
                    t0 = time.perf_counter()
                    f()
                    t[k].append(time.perf_counter() - t0)
            fn["dedup"]()
            counters = (sc.get_counter(1024), sc.get_counter(1025))
            case = dict(frontiers=n, max_dist=vis[0], max_angle=vis[1], way_points=counters[0], distinct_poses=counters[1],
                        ms={k: med_ms(v) for k, v in t.items()}, ms_min={k: round(min(v) * 1e3, 4) for k, v in t.items()},
                        by_hand_split_ms={k: med_ms(v) for k, v in split.items()})
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    sc.set_option("pathinfo.dedup", 1)
    sc.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "ref2d.json"), "w"), indent=1)


def run_trace(n_landmarks):
    sc, cells, origin, pose = setup(n_landmarks)
    goals, ach = M.goals(cells, origin, 2011, 2000)
    sc.set_fim_params(*VIS[1])
    fn, _ = routes(sc, cells, origin, pose, goals, ach)
    for _ in range(6):
        fn["dedup"]()
        fn["every"]()
    sc.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "trace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathinfo"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--landmarks", type=int, default=100_000)
    a = ap.parse_args()
    if a.mode == "time":
        run_time(a.out, max(a.reps, 15), a.landmarks)
    else:
        run_trace(a.landmarks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
