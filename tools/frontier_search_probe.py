#!/usr/bin/env python3
"""What the frontier search on the device (fs_search_frontiers) costs against the route it replaces.  On the MI355X:

    python tools/frontier_search_probe.py [--out DIR] [--reps N]     # -> DIR/search.json (default profiles/frontier_search)

Per map (REF2D 512^2 and a 1024^2 floor plan, a robot on a free cell, the reference's defaults M = 20, min = 1, lethal 160, 50 m):
* device: fs_search_frontiers (no every list) cold (the first call on a fresh context after its grid upload: the scratch is
  allocated in it) and warm (the same call again); the level count of the deepest component (counter 1014);
* the route it replaces: fs_frontier_clusters with the label image, then the host tail (tests/frontier_ref's walk, pieces and
  goal points with a real std::sort on one core; only the C call is timed, its buffers allocated beforehand — it includes the
  restatement's own pass over the label image, as the mirror's tail does);
* the one call fs_get_frontier_costs_searched against fs_search_frontiers + fs_get_frontier_costs_planned on its columns;
* Reference seeds (fs_set_frontier_seed_order FS_SEEDS_REFERENCE: the outer search walked on the device), cold and warm, with the
  outer levels walked and cells popped (counters 1019 / 1020), against the oracle's whole searchFrom (oracle/fso_frontier.cpp,
  serial, one core of the same host; only the C call is timed, its buffers allocated beforehand).
Host wall clock around calls that end in a synchronisation, output arrays for 4096 records (the Python default sizes them
from the grid: nx * ny records); medians of --reps.
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
import frontier_ref as FR  # noqa: E402
import oracle as O  # noqa: E402  (the checker, timed as the serial route)

fs = importlib.import_module("fit-slam_amd")


def stats_ms(xs):
    return dict(median_ms=round(float(np.median(xs)) * 1e3, 4), min_ms=round(float(np.min(xs)) * 1e3, 4),
                max_ms=round(float(np.max(xs)) * 1e3, 4), reps=len(xs))


def timed(f, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        out.append(time.perf_counter() - t)
    return out


def searchfrom_call(cells, origin, res, pos, lethal=160, min_cluster=1, max_cluster=20, max_distance=50.0):
    """A zero-argument callable that runs only the oracle's C searchFrom (its buffers allocated beforehand)"""
    import ctypes as C
    ny, nx = cells.shape
    c = np.ascontiguousarray(cells, dtype=np.uint8)
    cell_piece, cell_seed = np.zeros((ny, nx), np.int32), np.zeros((ny, nx), np.int32)
    cap = ny * nx
    goals, sizes, piece = np.zeros((cap, 2)), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n_out, n_every = C.c_int32(), C.c_int64()
    O.frontier_search(c, origin[:2], res, pos)                         # (sets the C function's argument types)
    f = O.lib().fso_frontier_search
    p = lambda a: a.ctypes.data_as(C.c_void_p)                         # noqa: E731
    args = (p(c), nx, ny, float(origin[0]), float(origin[1]), float(res), float(pos[0]), float(pos[1]), lethal, min_cluster,
            max_cluster, float(max_distance), p(cell_piece), p(cell_seed), cap, p(goals), p(sizes), p(piece), C.byref(n_out),
            C.byref(n_every))
    return lambda: f(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_search"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(777))
    ref = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=20_000)
    plan = fs.synth.make_grid(rng, 1024, 1)
    maps = [("REF2D_512", ref, ref.cells, ref.origin, ref.resolution),
            ("plan_1024", None, plan, (-25.6, -25.6, 0.0), 0.05)]
    result = {}
    for name, w, cells3, origin, res in maps:
        cells = np.ascontiguousarray(cells3[0])
        ny, nx = cells.shape
        free = np.argwhere(cells == 0)
        y, x = free[len(free) // 2]
        pos = (origin[0] + (x + 0.5) * res, origin[1] + (y + 0.5) * res)
        sc = fs.FrontierScorer(device=0)
        try:
            if w is not None:
                sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                                  robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
            sc.upload_grid(cells[None], origin, res)
            if w is not None:
                sc.upload_landmarks(w.landmarks)
                sc.lookup_generate()
                sc.set_fim_params(14.0, 1.0)
                sc.set_arrival_limits(4000.0, sc.max_arrival()["min_gt"])
            search = lambda: sc.search_frontiers(pos, want_every=False, max_records=4096)       # noqa: E731
            fr, _ = search()
            cold = []
            for _ in range(max(3, args.reps // 4)):
                fresh = fs.FrontierScorer(device=0)
                try:
                    fresh.upload_grid(cells[None], origin, res)
                    t = time.perf_counter()
                    fresh.search_frontiers(pos, want_every=False, max_records=4096)
                    cold.append(time.perf_counter() - t)
                finally:
                    fresh.close()
            warm = timed(search, args.reps)
            levels = sc.get_counter(1014)
            clusters = timed(lambda: sc.frontier_clusters((ny, nx), pos), args.reps)
            labels, _, _, _ = sc.frontier_clusters((ny, nx), pos)
            rc = int((pos[1] - origin[1]) / res) * nx + int((pos[0] - origin[0]) / res)
            tail = timed(FR.search_call(labels, origin, res, rc), args.reps)
            s = FR.search(labels, origin, res, rc)
            entry = dict(shape=[ny, nx], records=int(fr.shape[0]), cells=int(s["every_cells"].shape[0]), deepest_levels=int(levels),
                         search_cold=stats_ms(cold), search_warm=stats_ms(warm), clusters_with_labels=stats_ms(clusters),
                         host_tail_restatement=stats_ms(tail),
                         equal_to_restatement=bool(fr["goal_cell"].tolist() == s["goal_cell"].tolist()))
            if w is not None:
                pose = np.array([pos[0], pos[1], 0, 0, 0, 0, 1.0])
                goal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
                planned = timed(lambda: sc.get_frontier_costs_planned(pose, goal, frontier_size=fr["size"]), args.reps)
                one = timed(lambda: sc.get_frontier_costs_searched(pose, max_records=4096), args.reps)

                def chained():
                    f, _ = search()
                    g = np.stack([f["goal_x"], f["goal_y"], np.zeros(f.shape[0])], 1)
                    sc.get_frontier_costs_planned(pose, g, frontier_size=f["size"])
                chain = timed(chained, args.reps)
                entry.update(planned=stats_ms(planned), one_call=stats_ms(one), search_then_planned=stats_ms(chain))
            # Reference seeds: cold on a fresh context, warm, the outer walk's counters; the oracle's serial searchFrom
            sc.set_frontier_seed_order("reference")
            search_ref = lambda: sc.search_frontiers(pos, want_every=False, max_records=4096)   # noqa: E731
            fr_ref, _ = search_ref()
            cold_ref = []
            for _ in range(max(3, args.reps // 4)):
                fresh = fs.FrontierScorer(device=0)
                try:
                    fresh.upload_grid(cells[None], origin, res)
                    fresh.set_frontier_seed_order("reference")
                    t = time.perf_counter()
                    fresh.search_frontiers(pos, want_every=False, max_records=4096)
                    cold_ref.append(time.perf_counter() - t)
                finally:
                    fresh.close()
            warm_ref = timed(search_ref, args.reps)
            outer_levels, outer_popped = sc.get_counter(1019), sc.get_counter(1020)
            sc.set_frontier_seed_order("nearest")
            r = O.frontier_search(cells, origin[:2], res, pos)
            oracle_call = searchfrom_call(cells, origin, res, pos)
            host = timed(oracle_call, max(3, args.reps // 4))
            warm_ms = float(np.median(warm_ref)) * 1e3
            entry.update(reference=dict(
                records=int(fr_ref.shape[0]), outer_levels=int(outer_levels), outer_popped=int(outer_popped),
                search_cold=stats_ms(cold_ref), search_warm=stats_ms(warm_ref),
                warm_us_per_level=round((warm_ms - entry["search_warm"]["median_ms"]) * 1e3 / max(outer_levels, 1), 3),
                oracle_searchfrom_one_core=stats_ms(host),
                equal_to_oracle=bool(fr_ref.shape[0] == r["goals"].shape[0] and np.array_equal(
                    np.stack([fr_ref["goal_x"], fr_ref["goal_y"]], 1).view(np.uint64), r["goals"].view(np.uint64)))))
            result[name] = entry
            print(name, json.dumps(entry))
        finally:
            sc.close()
    with open(os.path.join(args.out, "search.json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
