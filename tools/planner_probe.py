#!/usr/bin/env python3
"""What the batched grid planner (fs_plan_paths) costs against the per-frontier planner it replaces, and how far
its paths are from that planner's.

    python tools/planner_probe.py cpu     [--out DIR]   # reference_astar CPU time (one core) on REF2D + the legs' comparison
    python tools/planner_probe.py gpu     [--out DIR]   # fs_plan_paths / fs_get_frontier_costs_planned on the MI355X

`cpu` writes astar_vs_converged.json (24 maps, both allow_unknown: achievability agreement, equal point-count share, max / p99
relative path_length_m difference) and cpu_ref2d.json (the two legs of the restatement on REF2D, 50 frontiers, wall time).
`gpu` writes gpu_ref2d.json: medians of the field alone, the field + 50 / 2 000 descents, descents on a cached field, and the
fused call against plan-on-host (the restatement's per-frontier A*) + fs_get_frontier_costs and against fs_plan_paths +
fs_get_frontier_costs.  Output directory: profiles/planner (default).
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
import planner_ref as R  # noqa: E402  (the restatement: the CPU legs)

RES = 0.05


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def ref2d(n, seed=3):
    fs = importlib.import_module("fit-slam_amd")
    w = fs.synth.make_workload("REF2D", n_cand=n, n_landmarks=20_000)
    rng = np.random.default_rng(seed)
    # the robot on the free cell (of 8 drawn) whose field reaches the most goal cells: a tick of a robot that can go somewhere
    xs, ys = R.free_cells(w.cells[0], rng, 8)
    gx = ((w.goals[:, 0] - w.origin[0]) / w.resolution).astype(int)
    gy = ((w.goals[:, 1] - w.origin[1]) / w.resolution).astype(int)
    reach = [int((R.converged_field(w.cells[0], x, y)[0][gy, gx] < R.POT_HIGH).sum()) for x, y in zip(xs, ys)]
    k = int(np.argmax(reach))
    rx, ry = int(xs[k]), int(ys[k])
    return w, R.robot_pose(w.origin, w.resolution, rx, ry, 0.7), (rx, ry)


def cpu(out_dir):
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})          # one core
    w, pose, _ = ref2d(50)
    cells = w.cells[0]
    t = {}
    for leg, name in ((R.REFERENCE_ASTAR, "reference_astar"), (R.CONVERGED, "converged")):
        xs = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = R.plan(cells, w.origin, RES, pose, w.goals, leg=leg)
            xs.append(time.perf_counter() - t0)
        t[name] = dict(ms=med_ms(xs), achievable=int(r["achievable"].sum()))
    json.dump(dict(what="REF2D (512^2), 50 frontiers, one core: the restatement's legs, wall ms (median of 5)", **t),
              open(os.path.join(out_dir, "cpu_ref2d.json"), "w"), indent=1)
    # the two legs' paths on the 24 maps of tests/test_planner_restatement.py
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_planner_restatement as T
    agree = clean_n = same_len = both_n = 0
    rel = []
    stalls = {"converged": 0, "reference_astar": 0}
    for seed, (c, origin, goals) in enumerate(T._floor_plans(24)):
        rng = np.random.default_rng(seed)
        rx, ry = R.free_cells(c, rng, 1)
        p = R.robot_pose(origin, RES, rx[0], ry[0], 0.3)
        for allow in (False, True):
            a = R.plan(c, origin, RES, p, goals, allow_unknown=allow)
            b = R.plan(c, origin, RES, p, goals, allow_unknown=allow, leg=R.REFERENCE_ASTAR)
            stalls["converged"] += int(((a["limit"] >> 8) == 4).sum())
            stalls["reference_astar"] += int(((b["limit"] >> 8) == 4).sum())
            clean = ((b["limit"] & 3) == 0) & ((a["limit"] >> 8) != 4) & ((b["limit"] >> 8) != 4)
            clean_n += int(clean.sum())
            agree += int((clean & (a["achievable"] == b["achievable"])).sum())
            both = (a["achievable"] == 1) & (b["achievable"] == 1)
            both_n += int(both.sum())
            same_len += int((both & (a["path_length"] == b["path_length"])).sum())
            m = both & (b["path_length_m"] > 0)
            rel.extend((np.abs(a["path_length_m"][m] - b["path_length_m"][m]) / b["path_length_m"][m]).tolist())
    rel = np.asarray(rel)
    res = dict(what="converged leg against the per-frontier A* (reference_astar) on 24 floor plans (synth.make_grid 128^2 and make_small_2d), "
                    "both allow_unknown; one robot cell per map",
               goals=2 * sum(g.shape[0] for _, _, g in T._floor_plans(24)), without_limits=clean_n, achievable_agree=agree,
               descent_out_of_cycles=stalls, both_achievable=both_n, equal_point_count_share=round(same_len / max(both_n, 1), 4),
               path_length_m_rel_diff=dict(max=round(float(rel.max()), 4), p99=round(float(np.percentile(rel, 99)), 4),
                                           p50=round(float(np.percentile(rel, 50)), 4), mean=round(float(rel.mean()), 4)))
    json.dump(res, open(os.path.join(out_dir, "astar_vs_converged.json"), "w"), indent=1)
    print(json.dumps(t), json.dumps(res))


def gpu(out_dir, reps=15):
    import torch  # noqa: F401  (one HIP runtime, loaded before the library, as bench.py does)
    fs = importlib.import_module("fit-slam_amd")
    w, pose, (rx, ry) = ref2d(2000)
    sc = fs.FrontierScorer(device=0)
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])
    g50, g2k = w.goals[:50], w.goals
    free_x, free_y = R.free_cells(w.cells[0], np.random.default_rng(9), reps + 4)
    poses = [R.robot_pose(w.origin, RES, int(x), int(y), 0.7) for x, y in zip(free_x, free_y)]
    res = {"what": "REF2D (512^2), ms, median over robot cells / repetitions; wall time of the host call"}

    def timed(fn, k=reps):
        xs = []
        for i in range(k):
            t0 = time.perf_counter()
            fn(i)
            xs.append(time.perf_counter() - t0)
        return med_ms(xs)

    sc.plan_paths(poses[-1], g50)                                                      # warm-up
    sc.get_counter(1002, reset=True); sc.get_counter(1004, reset=True)
    res["field_only"] = timed(lambda i: sc.navfn_potential(poses[i]))
    rounds = []
    for i in range(4):
        sc.navfn_potential(poses[reps + i])
        rounds.append(sc.get_counter(1003))
    res["field_rounds"] = rounds
    res["round_launches_per_field"] = round(sc.get_counter(1004) / sc.get_counter(1002), 1)
    sc.enable_kernel_timing(True)
    sc.plan_paths(R.robot_pose(w.origin, RES, rx, ry, 0.1), g50, allow_unknown=1)
    kt = {k: sc.kernel_time(k) for k in (6, 7, 8)}
    sc.enable_kernel_timing(False)
    res["kernel_ms_one_field_50_paths"] = {"setup": kt[6][0], "rounds": kt[7][0], "round_batches": kt[7][1], "paths": kt[8][0]}
    allow = [0]

    def fresh_plan(goals):
        def f(i):
            allow[0] ^= 1                                                              # a new field every call
            sc.plan_paths(poses[i], goals, allow_unknown=allow[0])
        return f
    res["field_plus_50_paths"] = timed(fresh_plan(g50))
    res["field_plus_2000_paths"] = timed(fresh_plan(g2k))
    res["cached_field_50_paths"] = timed(lambda i: sc.plan_paths(pose, g50))
    res["cached_field_2000_paths"] = timed(lambda i: sc.plan_paths(pose, g2k))
    # one tick: plan + score + rank for 50 frontiers, robot at a new cell (no cached field)
    fsz, bl = w.frontier_size[:50], w.blacklisted[:50]
    res["fused_planned_50"] = timed(lambda i: sc.get_frontier_costs_planned(poses[i], g50, frontier_size=fsz, blacklisted=bl))

    def two_calls(i):
        p = sc.plan_paths(poses[i], g50, allow_unknown=1)
        sc.get_frontier_costs(g50, p["path_length"], p["path_heading"], frontier_size=fsz, blacklisted=bl, achievable_in=p["achievable"])
    res["plan_paths_then_costs_50"] = timed(two_calls)

    def host_plan(i):
        p = R.plan(w.cells[0], w.origin, RES, poses[i], g50, leg=R.REFERENCE_ASTAR)
        sc.get_frontier_costs(g50, p["path_length"], p["path_heading"], frontier_size=fsz, blacklisted=bl, achievable_in=p["achievable"])
    res["host_astar_then_costs_50"] = timed(host_plan, 5)
    res["speedup_fused_vs_host_astar"] = round(res["host_astar_then_costs_50"] / res["fused_planned_50"], 1)
    sc.close()
    json.dump(res, open(os.path.join(out_dir, "gpu_ref2d.json"), "w"), indent=1)
    print(json.dumps(res))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cpu", "gpu"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planner"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    cpu(a.out) if a.mode == "cpu" else gpu(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
