#!/usr/bin/env python3
"""What fs_fleet_allocate_roadmap and fs_allocate_tasks cost on the MI355X against the route a caller had before.

    python tools/fleet_probe.py [--out DIR] [--reps K]        # writes DIR/allocate_ref2d.json (default profiles/fleet)

REF2D (512^2) with the roadmap of tests/test_gpu_roadmap_astar.py's _setup recipe (305 node points), REF2D's ray parameters, frontiers
from its _goals recipe, R robots on free cells.  For R in {2, 4, 8, 16} x n in {50, 200, 2000}, alternated call by call inside
one process after a warm-up of each:

    fleet      fs_fleet_allocate_roadmap (assignment only: the matrices stay on the device)
    by_hand    what a caller had before: R sequential fs_get_frontier_costs_roadmap calls, the R cost rows on the host, the
               allocator's CPU restatement (tests/alloc_ref) on one core

and the solve alone, fs_allocate_tasks against the restatement on one core, at 8 x 50, 16 x 200, 64 x 2000 and 64 x 4096 for the
"u1" and "contested" matrix families of tests/alloc_ref.py.

Host wall time around calls that end in a synchronisation; medians.
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RES = 0.05
NAME = "REF2D"


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def timed(fn, reps):
    """medians of `reps` calls of every entry of fn, alternated call by call, after one warm-up call each"""
    for f in fn.values():
        f()
    t = {k: [] for k in fn}
    for _ in range(reps):
        for k, f in fn.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    return t


def setup():
    import torch  # noqa: F401  (one HIP runtime, loaded before the library, as bench.py does)
    import zlib
    fs = importlib.import_module("fit-slam_amd")
    from test_gpu_roadmap_astar import _map, _nodes
    cells, origin = _map(NAME)
    pts = _nodes(cells, origin, zlib.crc32(NAME.encode()), int(min(1500, max(40, cells.size * RES * RES / 2))))
    w = fs.synth.make_workload(NAME, n_cand=16, n_landmarks=16)
    sc = fs.FrontierScorer(device=0)
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(cells[None], origin, RES)
    sc.set_arrival_limits(4000.0, sc.max_arrival()["min_gt"])
    sc.roadmap_add_nodes(pts)
    sc.roadmap_rebuild()
    return sc, cells, origin, pts


def run(out_dir, reps):
    import alloc_ref as A
    import planner_ref as P
    import roadmap_ref as R
    from test_gpu_roadmap_astar import _goals
    sc, cells, origin, pts = setup()
    A.solve(np.ones((1, 1)))                                   # (compiles the restatement)
    res = {"what": f"REF2D (512^2), {pts.shape[0]} node points; host wall ms around calls that end in a synchronisation, median of {reps} "
                   f"after one warm-up call per route, the routes alternated call by call",
           "routes": {"fleet": "fs_fleet_allocate_roadmap, assignment only",
                      "by_hand": "R sequential fs_get_frontier_costs_roadmap calls + the allocator's CPU restatement on one core"},
           "cases": [], "solve": []}
    xs, ys = P.free_cells(cells, np.random.default_rng(3), 16)
    all_poses = np.array([R.pose7(origin[0] + (x + 0.5) * RES, origin[1] + (y + 0.5) * RES, 0.3 * k) for k, (x, y) in enumerate(zip(xs, ys))])
    for search, method in (("tree", "hungarian"), ("tree", "minpos"), ("reference", "hungarian")):
        sc.set_roadmap_search(search)
        for n_robots in (2, 4, 8, 16):
            poses = all_poses[:n_robots]
            for n in (50, 200, 2000):
                goals, _ = _goals(cells, origin, 31 + n, n, poses[0, :2])
                fsize = np.full(n, 12, dtype=np.int32)
                split = {"costs": [], "solve_cpu": []}

                def fleet():
                    return sc.fleet_allocate_roadmap(poses, goals, frontier_size=fsize, method=method)

                def by_hand():
                    t0 = time.perf_counter()
                    rows = [sc.get_frontier_costs_roadmap(p, goals, frontier_size=fsize) for p in poses]
                    t1 = time.perf_counter()
                    cost = np.stack([r["weighted_cost"] for r in rows]); dist = np.stack([r["path_length_m"] for r in rows])
                    out = A.allocate(cost, dist, method)
                    split["costs"].append(t1 - t0); split["solve_cpu"].append(time.perf_counter() - t1)
                    return out

                t = timed({"fleet": fleet, "by_hand": by_hand}, reps)
                for v in split.values():          # (timed()'s warm-up call)
                    del v[0]
                got, want = fleet(), by_hand()
                assert got["assignment"].tolist() == want["assignment"].tolist()
                case = dict(search=search, method=method, robots=n_robots, frontiers=n,
                            ms={k: med_ms(v) for k, v in t.items()}, ms_min={k: round(min(v) * 1e3, 4) for k, v in t.items()},
                            by_hand_split_ms={k: med_ms(v) for k, v in split.items()},
                            augmentations=sc.get_counter(1030), step5=sc.get_counter(1031), primes=sc.get_counter(1032))
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    for n_robots, n in ((8, 50), (16, 200), (64, 2000), (64, 4096)):
        for family in ("u1", "contested"):
            cost, dist = A.family(family, n_robots, n, 1000 * n_robots + n)
            for method in ("hungarian", "minpos"):
                t = timed({"device": lambda: sc.allocate_tasks(cost, dist, method=method),
                           "cpu_one_core": lambda: A.allocate(cost, dist, method)}, reps)
                case = dict(robots=n_robots, tasks=n, family=family, method=method, ms={k: med_ms(v) for k, v in t.items()},
                            ms_min={k: round(min(v) * 1e3, 4) for k, v in t.items()},
                            augmentations=sc.get_counter(1030), step5=sc.get_counter(1031), primes=sc.get_counter(1032))
                res["solve"].append(case)
                print(json.dumps(case), flush=True)
    sc.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "allocate_ref2d.json"), "w"), indent=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet"))
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    run(a.out, max(a.reps, 15))
    return 0


if __name__ == "__main__":
    sys.exit(main())
