#!/usr/bin/env python3
"""What the next goal on the device (fs_roadmap_next_goal) costs, against the CPU restatement of the reference's
host code.  On the MI355X:

    python tools/tour_probe.py [--out DIR] [--reps N]     # -> DIR/pairs_ref2d.json, DIR/tours_ref2d.json (default profiles/tour)

On REF2D's map with a roadmap of random free-cell nodes (rebuilt on the device and in the restatement):
* pairs: the pair matrix at k = 5 (6 trees) — the restatement (tests/tour_ref.py pair_matrix: roadmap_ref's rr_tree per source,
  one core) against one fs_roadmap_next_goal call (the trees in one launch, the pair and tour kernels, one synchronisation) and
  against six fs_roadmap_plan calls from the six sources (a tree and a synchronisation each: what the device did per tree before).
* tours: one fs_roadmap_next_goal call at k = 5, 8, 10, 12 (the whole call; its trees are built anew every time, the roadmap is
  the same), with the restatement's tour loop (tour_ref.cpp tr_tour) at k = 5 and 8 and Held-Karp at every k for comparison.
Host wall clock around calls that end in a synchronisation; medians of --reps after two warm-up calls.
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import planner_ref as P  # noqa: E402
import roadmap_ref as R  # noqa: E402
import tour_ref as T  # noqa: E402


def med_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t0)
    return dict(median_ms=round(float(np.median(xs)) * 1e3, 4), min_ms=round(float(np.min(xs)) * 1e3, 4),
                max_ms=round(float(np.max(xs)) * 1e3, 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tour"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--search", choices=["tree", "reference"], default="tree",
                    help="the roadmap search of the pair lengths (fs_set_roadmap_search); reference writes *_reference.json")
    args = ap.parse_args()
    import torch  # noqa: F401  (the same load order as bench.py)
    fs = importlib.import_module("fit-slam_amd")
    w = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=16)
    cells, res = np.ascontiguousarray(w.cells[0]), float(w.resolution)
    origin = tuple(float(v) for v in w.origin)
    rng = np.random.default_rng(2024)
    k_nodes = int(min(1500, max(40, cells.size * res * res / 2)))
    xs, ys = P.free_cells(cells, rng, k_nodes)
    pts = np.stack([origin[0] + (xs + rng.uniform(0, 1, k_nodes)) * res, origin[1] + (ys + rng.uniform(0, 1, k_nodes)) * res], axis=1)
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, res)
    sc.roadmap_add_nodes(pts)
    sc.roadmap_rebuild()
    sc.set_roadmap_search(args.search)
    suffix = "" if args.search == "tree" else "_" + args.search
    ref = R.Roadmap(cells, origin, res)
    ref.populate(pts)
    ref.rebuild()
    g = sc.roadmap_graph()
    n_nodes, n_edges = int(g["xy"].shape[0]), int(g["col"].size)
    robot = pts[0]

    def frontier_list(k):
        r = np.random.default_rng(k)
        n = k + 5
        fx, fy = P.free_cells(cells, r, n)
        goal = np.zeros((n, 3))
        goal[:, 0] = origin[0] + (fx + 0.5) * res
        goal[:, 1] = origin[1] + (fy + 0.5) * res
        plm = np.concatenate([np.sort(r.uniform(0.5, 12.0, k + 1)), r.uniform(12.5, 50.0, 4)])
        return goal, plm, np.ones(n, np.uint8)

    os.makedirs(args.out, exist_ok=True)
    # ---- the pair matrix at k = 5
    goal, plm, ach = frontier_list(5)
    out = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=5, want_matrix=True, want_selection=True)
    sel = out["selection"]
    loc = np.flatnonzero((sel & 3) == 1)
    loc = loc[np.argsort(plm[loc], kind="stable")]
    cg = np.flatnonzero(sel & 4)
    nodes = np.concatenate([robot[None], goal[loc, :2], goal[cg, :2]])
    M_ref = T.pair_matrix(ref, nodes)
    if args.search == "tree":
        assert out["pair_length_m"].tobytes() == M_ref.tobytes(), "device pair matrix differs from the restatement"
    sources = nodes[:-1]
    pairs = dict(
        map="REF2D", search=args.search, roadmap_nodes=n_nodes, roadmap_edges=n_edges, k=5, trees=int(sources.shape[0]),
        matrix_bit_equal_to_restatement=bool(out["pair_length_m"].tobytes() == M_ref.tobytes()),
        host_restatement=med_ms(lambda: T.pair_matrix(ref, nodes), max(3, args.reps // 4)),
        device_next_goal_call=med_ms(lambda: sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=5), args.reps),
        device_one_plan_per_source=med_ms(lambda: [sc.roadmap_plan(R.pose7(*s), goal[:1]) for s in sources], args.reps),
        tree_rounds_of_the_batch=sc.get_counter(1009),
    )
    json.dump(pairs, open(os.path.join(args.out, f"pairs_ref2d{suffix}.json"), "w"), indent=1)
    print(json.dumps(pairs))
    # ---- the tour search at k = 5, 8, 10, 12
    tours = dict(map="REF2D", search=args.search, roadmap_nodes=n_nodes, roadmap_edges=n_edges, rows=[])
    for k in (5, 8, 10, 12):
        goal, plm, ach = frontier_list(k)
        reps = args.reps if k < 12 else max(5, args.reps // 2)
        out = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=k, want_matrix=True)
        M = out["pair_length_m"]
        sc.get_counter(1010, reset=True)
        row = dict(k=k, tours=math.factorial(k), device_next_goal_call=med_ms(
            lambda: sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=k), reps))
        row["tours_evaluated_per_call"] = sc.get_counter(1010) // (reps + 2)
        row["tour_length"], row["n_tied"] = out["tour_length"], out["n_tied"]
        hk = T.held_karp(M)
        row["held_karp_length"] = hk
        row["held_karp_equal"] = bool(hk == out["tour_length"])
        row["host_held_karp"] = med_ms(lambda: T.held_karp(M), 3, warm=1)
        if k <= 8:
            L, cnt, perm, _ = T.tour(M)
            row["host_reference_loop"] = med_ms(lambda: T.tour(M), 3, warm=1)
            row["host_reference_loop_equal"] = bool(L == out["tour_length"] and cnt == out["n_tied"])
        tours["rows"].append(row)
        print(json.dumps(row))
    json.dump(tours, open(os.path.join(args.out, f"tours_ref2d{suffix}.json"), "w"), indent=1)
    sc.close()
    ref.close()


if __name__ == "__main__":
    main()
