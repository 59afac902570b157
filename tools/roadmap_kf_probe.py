#!/usr/bin/env python3
"""What the roadmap's key-frame anchors on the device (fs_roadmap_set_keyframes / fs_roadmap_optimize) cost, against
the CPU restatement of the reference's host code (tests/roadmap_kf_ref/) on one core.

    python tools/roadmap_kf_probe.py gpu   [--out DIR]        # on the MI355X -> gpu_ref2d.json, gpu_long.json
    python tools/roadmap_kf_probe.py cpu   [--out DIR]        # one core      -> cpu_ref2d.json, cpu_long.json
    python tools/roadmap_kf_probe.py split --stats CSV [...]  # a rocprofv3 --kernel-trace --stats run of `gpu --reps 3`
                                                                #   -> gpu_split.json

Two sizes.  `ref2d`: REF2D's map, a seeded robot walk of 240 ticks with a key frame per tick (~0.5 m apart), frontier and
robot-pose nodes per tick, a map message every 4 ticks, then a loop-closure correction of the second half; fs_roadmap_set_keyframes
is timed on every message after the first 10 ticks, fs_roadmap_optimize on the final state (its result does not change with
repetition).  `long`: a synthetic long run on a free 52 m map — 4 000 key frames (5 558 entries of a message, 2 223 cells), 20 000
nodes, one message anchoring all of them (~50 000 anchors), a rigid correction, optimise (radius_to_decide_edges 1.5).  Host wall clock around a synchronising call,
warmed, medians.  The CPU side times the restatement's mapDataCallback / optimizeSHM and tests/roadmap_ref's rebuild of the same node
list.  Output directory: profiles/roadmap_kf (default).
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import roadmap_kf_ref as K  # noqa: E402
import roadmap_ref as R  # noqa: E402

RES = 0.05


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4) if len(xs) else None


def ref2d_case():
    fs = importlib.import_module("fit-slam_amd")
    cells = np.ascontiguousarray(fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])
    origin = (-cells.shape[1] * RES / 2, -cells.shape[0] * RES / 2, 0.0)
    bounds = (origin[0] + 1.5, -origin[0] - 1.5, origin[1] + 1.5, -origin[1] - 1.5)
    poses, fronts = K.trajectory(2024, 240, bounds=bounds)
    half = len(poses) // 2
    fixed = poses.copy()
    fixed[half:] = K.correct(poses[half:], 0.35, -0.2, 0.08, about=tuple(poses[half, :2]))
    return dict(name="ref2d", cells=cells, origin=origin, params=(1.0, 6.1, 0.25, 0.25), poses=poses, fronts=fronts, fixed=fixed, every=4)


def long_case():
    cells = np.zeros((1040, 1040), np.uint8)
    origin = (-2.0, -2.0, 0.0)
    rng = np.random.default_rng(7)
    side, n_cells, n_ids, n_entries = 48, 2223, 4000, 5558
    sub = [(0.15 + 0.35 * i, 0.15 + 0.35 * j) for i in range(3) for j in range(3)]
    nodes = np.array([(c % side + dx, c // side + dy) for c in range(n_cells) for dx, dy in sub][:20000])
    # 5 558 entries of 4 000 ids (1 558 ids named twice, in two cells: the last pose counts), ~2.5 per node cell
    e = np.arange(n_entries)
    cx, cy = (e % n_cells) % side, (e % n_cells) // side
    ids = (e % n_ids).astype(np.int32)
    poses = np.array([K.pose(x + rng.uniform(0.05, 0.95), y + rng.uniform(0.05, 0.95), rng.uniform(-3, 3)) for x, y in zip(cx, cy)])
    fixed = K.correct(poses, 0.3, -0.15, 0.02, about=(24.0, 24.0))
    return dict(name="long", cells=cells, origin=origin, params=(1.0, 1.5, 0.25, 0.25), ids=ids, poses=poses, nodes=nodes, fixed=fixed)


def run_gpu(case, reps):
    fs = importlib.import_module("fit-slam_amd")
    sc = fs.FrontierScorer(device=0)
    try:
        sc.upload_grid(case["cells"][None], case["origin"], RES)
        sc.set_roadmap_params(*case["params"])
        t_set, info = [], {}
        ids_all = case.get("ids", np.arange(len(case["poses"]), dtype=np.int32))
        if case["name"] == "ref2d":
            for t in range(len(case["poses"])):
                for xy, robot in ((case["fronts"][t], False), (case["poses"][t, :2][None], True)):
                    try:
                        sc.roadmap_add_nodes(xy, robot)
                    except fs.FsError:
                        pass
                if t % case["every"] == case["every"] - 1:
                    ids = ids_all[:t + 1]
                    t0 = time.perf_counter()
                    sc.roadmap_set_keyframes(ids, case["poses"][ids])
                    if t >= 10:
                        t_set.append(time.perf_counter() - t0)
        else:
            for r in range(reps + 1):
                sc.set_roadmap_params(*case["params"])
                sc.roadmap_add_nodes(case["nodes"], True)
                t0 = time.perf_counter()
                sc.roadmap_set_keyframes(ids_all, case["poses"])
                if r:
                    t_set.append(time.perf_counter() - t0)
        sc.roadmap_set_keyframes(ids_all, case["fixed"])
        sc.roadmap_optimize()                              # warm
        t_opt = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sc.roadmap_optimize()
            t_opt.append(time.perf_counter() - t0)
        g = sc.roadmap_graph()
        info = dict(records=sc.get_counter(1016), points=sc.get_counter(1018), rounds=sc.get_counter(1017), nodes=int(g["xy"].shape[0]),
                    edges=int(g["col"].size))
        return dict(case=case["name"], set_keyframes_ms=med_ms(t_set), set_keyframes_calls=len(t_set), optimize_ms=med_ms(t_opt),
                    optimize_calls=len(t_opt), **info)
    finally:
        sc.close()


def run_cpu(case, reps):
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass
    ref = K.KfRoadmap(case["params"][0], case["params"][2], case["params"][3])
    t_set = []
    ids_all = case.get("ids", np.arange(len(case["poses"]), dtype=np.int32))
    if case["name"] == "ref2d":
        for t in range(len(case["poses"])):
            ref.add_nodes(case["fronts"][t]); ref.add_nodes(case["poses"][t, :2][None], True)
            if t % case["every"] == case["every"] - 1:
                ids = ids_all[:t + 1]
                t0 = time.perf_counter()
                ref.set_keyframes(ids, case["poses"][ids])
                if t >= 10:
                    t_set.append(time.perf_counter() - t0)
    else:
        for r in range(reps + 1):
            ref.close()
            ref = K.KfRoadmap(case["params"][0], case["params"][2], case["params"][3])
            ref.add_nodes(case["nodes"], True)
            t0 = time.perf_counter()
            ref.set_keyframes(ids_all, case["poses"])
            if r:
                t_set.append(time.perf_counter() - t0)
    ref.set_keyframes(ids_all, case["fixed"])
    t_opt = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ref.optimize()
        t_opt.append(time.perf_counter() - t0)
    nodes = ref.nodes()
    t0 = time.perf_counter()
    rr = R.Roadmap(case["cells"], case["origin"], RES, *case["params"])
    rr.populate(nodes)
    rr.rebuild()
    t_rebuild = time.perf_counter() - t0
    n_rec = int(ref.anchors()["kf_id"].size)
    ref.close(); rr.close()
    return dict(case=case["name"], what="the restatement on one core (mapDataCallback, optimizeSHM + populateNodes) and roadmap_ref's "
                "rebuild of the optimised node list, host wall ms, medians", set_keyframes_ms=med_ms(t_set), set_keyframes_calls=len(t_set),
                optimize_shm_ms=med_ms(t_opt), rebuild_ms=round(t_rebuild * 1e3, 3), optimize_total_ms=round(med_ms(t_opt) + t_rebuild * 1e3, 3),
                records=n_rec, nodes=int(nodes.shape[0]))


GROUPS = [("anchoring", ("kf_anchor_kernel",)), ("re-placement", ("kf_place_kernel",)),
          ("de-duplication", ("dd_clear", "dd_insert", "dd_fill", "dd_conflicts", "dd_block", "dd_round", "dd_cut", "dd_keep", "dd_compact")),
          ("rebuild", ("rm_candidates", "fs_segment", "segments", "rm_edges")), ("scans", ("rm_scan",))]


def split(stats_files):
    rows = {}
    for path in stats_files:
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            g = next((g for g, keys in GROUPS if any(k in name for k in keys)), "other")
            d = rows.setdefault(g, dict(calls=0, total_us=0.0, kernels={}))
            calls, ns = int(r.get("Calls", 0)), float(r.get("TotalDurationNs", 0))
            d["calls"] += calls; d["total_us"] += ns / 1e3
            d["kernels"][name[:80]] = dict(calls=calls, total_us=round(ns / 1e3, 2))
    for d in rows.values():
        d["total_us"] = round(d["total_us"], 2)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gpu", "cpu", "split"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap_kf"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stats", nargs="*", default=[])
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.mode == "split":
        res = dict(what="device time by group from rocprofv3 --kernel-trace --stats of `gpu --reps 3` (both sizes, every call of the run: "
                   "the growth and the timed calls); 'scans' are the one-workgroup exclusive scans all steps share", groups=split(a.stats))
        json.dump(res, open(os.path.join(a.out, "gpu_split.json"), "w"), indent=1)
        print(json.dumps(res, indent=1))
        return 0
    for case in (ref2d_case(), long_case()):
        res = run_gpu(case, a.reps) if a.mode == "gpu" else run_cpu(case, max(3, a.reps // 4))
        json.dump(res, open(os.path.join(a.out, f"{a.mode}_{case['name']}.json"), "w"), indent=1)
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
