#!/usr/bin/env python3
"""What fs_roadmap_routes costs on the MI355X against the route a caller had before it.

    python tools/roadmap_routes_probe.py time [--out DIR] [--reps K]    # writes DIR/routes_ref2d.json (default profiles/roadmap)
    python tools/roadmap_routes_probe.py plan [--out DIR] [--label L]   # fs_roadmap_plan alone: DIR/routes_plan_only_L.json

REF2D (512^2) with the roadmap of tests/test_gpu_roadmap_astar.py's _setup recipe (305 nodes), 100 000 landmarks, 50 and 2 000
frontiers from its _goals recipe, the robot on the free cell of tests/roadmap_route_maps.py, both roadmap searches.  Two routes,
alternated call by call inside one process after a warm-up of each:

    call       fs_roadmap_routes with the node and leg dumps (refine 1, with_information 1, "routes.dedup" 1)
    by_hand    fs_roadmap_plan, fs_roadmap_get_graph, the routes and refinePath by the CPU restatement on one core
               (tests/roadmap_route_ref), fs_score_fim(info_only) on the leg poses: what a caller had to do before — the routes never
               left the device, so the host searches again

and fs_roadmap_plan alone beside them (`plan`: the same timing by a script that uses nothing this feature added, so that it runs on
the commit before it too; its kernels are untouched, so the two figures must agree within the run-to-run spread).

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
VIS = (14.0, 1.0)
NAME = "REF2D"


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def setup(n_landmarks):
    """(scorer with the grid, the roadmap and the scoring state staged; cells, origin, node points, robot pose)"""
    import torch  # noqa: F401  (one HIP runtime, loaded before the library, as bench.py does)
    import zlib
    fs = importlib.import_module("fit-slam_amd")
    import planner_ref as P
    import roadmap_ref as R
    from test_gpu_roadmap_astar import _map, _nodes
    cells, origin = _map(NAME)
    pts = _nodes(cells, origin, zlib.crc32(NAME.encode()), int(min(1500, max(40, cells.size * RES * RES / 2))))
    xs, ys = P.free_cells(cells, np.random.default_rng(3), 1)
    pose = R.pose7(origin[0] + (xs[0] + 0.5) * RES, origin[1] + (ys[0] + 0.5) * RES, 0.3)
    w = fs.synth.make_workload(NAME, n_cand=16, n_landmarks=n_landmarks)
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    sc.roadmap_add_nodes(pts)
    sc.roadmap_rebuild()
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    sc.set_fim_params(*VIS)
    return sc, cells, origin, pts, pose


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


def run_time(out_dir, reps, n_landmarks):
    import roadmap_route_ref as RR
    from test_gpu_roadmap_astar import _goals
    sc, cells, origin, pts, pose = setup(n_landmarks)
    ref = RR.RouteRoadmap(cells, origin, RES)
    assert ref.populate(pts) == 0
    ref.rebuild()
    res = {"what": f"REF2D (512^2), {pts.shape[0]} node points, {n_landmarks} landmarks, visibility {VIS}; host wall ms around calls that end "
                   f"in a synchronisation, median of {reps} after one warm-up call per route, the routes alternated call by call",
           "routes": {"call": "fs_roadmap_routes with node and leg dumps", "plan": "fs_roadmap_plan alone",
                      "by_hand": "fs_roadmap_plan + fs_roadmap_get_graph + routes and refinePath on one CPU core (restatement) + "
                                 "fs_score_fim(info_only) on the leg poses"},
           "cases": []}
    for search, leg in (("tree", RR.TREE), ("reference", RR.REFERENCE_ASTAR)):
        sc.set_roadmap_search(search)
        for n in (50, 2000):
            goals, ach = _goals(cells, origin, 31 + n, n, pose[:2])
            split = {"plan": [], "graph": [], "routes_cpu": [], "refine_cpu": [], "score": []}

            def call():
                return sc.roadmap_routes(pose, goals, achievable_in=ach, want_nodes=True, want_legs=True)

            def plan():
                return sc.roadmap_plan(pose, goals, achievable_in=ach)

            def by_hand():
                t0 = time.perf_counter()
                sc.roadmap_plan(pose, goals, achievable_in=ach)
                t1 = time.perf_counter()
                sc.roadmap_graph()
                t2 = time.perf_counter()
                r = ref.routes(pose, goals, achievable_in=ach, leg=leg)
                t3 = time.perf_counter()
                f = ref.refine(r["node_offset"], r["node"])
                p7 = ref.leg_poses(f["refined_offset"], f["refined_node"])
                t4 = time.perf_counter()
                if p7.shape[0]:
                    sc.score_fim(p7, info_only=True)
                t5 = time.perf_counter()
                for k, v in zip(split, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    split[k].append(v)

            fn = {"call": call, "by_hand": by_hand, "plan": plan}
            by_hand()
            for v in split.values():
                v.clear()
            t = timed(fn, reps)
            for v in split.values():          # (timed()'s warm-up call)
                del v[0]
            out = call()
            case = dict(search=search, frontiers=n, routes=int(out["goal_node"].size), raw_nodes=int(out["node"].size),
                        refined_nodes=int(out["refined_node"].size), legs=int(out["n_legs"].sum()),
                        truncated=int((out["complete"] == 0).sum()), walks=sc.get_counter(1027), distinct_poses=sc.get_counter(1028),
                        ms={k: med_ms(v) for k, v in t.items()}, ms_min={k: round(min(v) * 1e3, 4) for k, v in t.items()},
                        by_hand_split_ms={k: med_ms(v) for k, v in split.items()})
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    sc.close(); ref.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "routes_ref2d.json"), "w"), indent=1)


def run_plan(out_dir, reps, n_landmarks, label):
    """fs_roadmap_plan alone, three rounds of medians (their spread is the run-to-run spread of one process)"""
    from test_gpu_roadmap_astar import _goals
    sc, cells, origin, pts, pose = setup(n_landmarks)
    res = {"what": f"fs_roadmap_plan alone on REF2D's roadmap; host wall ms, three medians of {reps} calls each after a warm-up", "label": label,
           "cases": []}
    for search in ("tree", "reference"):
        sc.set_roadmap_search(search)
        for n in (50, 2000):
            goals, ach = _goals(cells, origin, 31 + n, n, pose[:2])
            fn = {"plan": lambda: sc.roadmap_plan(pose, goals, achievable_in=ach)}
            meds = [med_ms(timed(fn, reps)["plan"]) for _ in range(3)]
            case = dict(search=search, frontiers=n, ms_medians=meds)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    sc.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, f"routes_plan_only_{label}.json"), "w"), indent=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "plan"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--landmarks", type=int, default=100_000)
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    if a.mode == "time":
        run_time(a.out, max(a.reps, 15), a.landmarks)
    else:
        run_plan(a.out, max(a.reps, 15), a.landmarks, a.label)
    return 0


if __name__ == "__main__":
    sys.exit(main())
