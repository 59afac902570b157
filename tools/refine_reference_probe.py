#!/usr/bin/env python3
"""What the REFERENCE refine search (fs_set_refine_search) costs on the MI355X against the FIELD search and against the
reference's search on one CPU core.

    python tools/refine_reference_probe.py [--out DIR] [--reps K] [--no-worst]   # writes DIR/reference_search_ref2d.json (profiles/refine)

REF2D (512^2), the 13 legs of tools/refine_probe.py (13 distinct starts), in one process on one build, the filling call of
fs_refine_paths with its output arrays sized beforehand:

    reference   under FS_REFINE_SEARCH_REFERENCE: 1 leg and 13 legs in one call (one wavefront per leg), and each leg alone
    field       under FS_REFINE_SEARCH_FIELD, cold (a grid upload first: every field is built) and cached
    cpu         thetastar_ref's `reference` leg (the same search, std::priority_queue) on one core of this box, leg by leg

Host wall time around calls that end in a synchronisation; medians of K calls (default 10) after a warm-up.  With counters 1042-1046
of the 13-leg call (searches, batches, nodes popped, line-of-sight walks, largest heap), the pops of every leg, and — unless
--no-worst — one search that drains its component (a safe goal the start cannot reach): its pops and its time, once.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
import thetastar_ref as T  # noqa: E402
import thetastar_search_ref as S  # noqa: E402
from refine_probe import points, stats_ms  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-worst", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    import torch  # noqa: F401  (the same load order as bench.py)
    fs = importlib.import_module("fit-slam_amd")
    w = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=16)
    cells, res = np.ascontiguousarray(w.cells[0]), float(w.resolution)
    origin = tuple(float(v) for v in w.origin)
    rng = np.random.default_rng(4077)
    starts, goals = points(cells, origin, res, rng, 13), points(cells, origin, res, rng, 13)
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, res)
    L = sc._L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(s, g):
        s, g = np.ascontiguousarray(s), np.ascontiguousarray(g)
        n = len(s)
        st, cost, nv, npz = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        sc._check(L.fs_refine_paths(sc._h, n, vp(s), vp(g), 1, 1.0, 2.0, 8, vp(st), vp(cost), vp(nv), None, vp(npz), None))
        vert, pose = np.zeros((int(nv.sum()) + 1, 2)), np.zeros((int(npz.sum()) + 1, 2))
        return lambda: sc._check(L.fs_refine_paths(sc._h, n, vp(s), vp(g), 1, 1.0, 2.0, 8, vp(st), vp(cost), vp(nv), vp(vert), vp(npz), vp(pose)))

    def timed(fn, reps, before=None):
        fn()
        xs = []
        for _ in range(reps):
            if before:
                before()
            t0 = time.perf_counter(); fn(); xs.append(time.perf_counter() - t0)
        return xs

    out = dict(what="REF2D (512^2), fs_refine_paths (the filling call), wall time of the host call in ms, %d calls after a warm-up; cpu: "
                    "thetastar_ref's reference leg on one core" % args.reps,
               params=dict(allow_unknown=1, w_euc=1.0, w_traversal=2.0, corners=8))
    # ---- REFERENCE
    sc.set_refine_search("reference")
    got = sc.refine_paths(starts, goals)
    cpu_legs = [S.leg(cells, origin, res, starts[i], goals[i]) for i in range(13)]
    out["equal_to_the_header_on_the_cpu"] = all(
        int(got["status"][i]) == e["status"] and np.float64(got["cost"][i]).tobytes() == np.float64(e["cost"]).tobytes()
        and got["vertices"][i].tobytes() == e["vertices"].tobytes() and got["poses"][i].tobytes() == e["poses"].tobytes()
        for i, e in enumerate(cpu_legs))
    out["status"] = [int(v) for v in got["status"]]
    out["pops_per_leg"] = [e["pops"] for e in cpu_legs]
    out["walks_per_leg"] = [e["los_walks"] for e in cpu_legs]
    ref = {}
    ref["legs_1"] = stats_ms(timed(call(starts[:1], goals[:1]), args.reps))
    ref["legs_13"] = stats_ms(timed(call(starts, goals), args.reps))
    ref["counters_legs_13"] = dict(searches=sc.get_counter(1042), batches=sc.get_counter(1043), pops=sc.get_counter(1044),
                                   walks=sc.get_counter(1045), largest_heap=sc.get_counter(1046))
    per_leg = []
    for i in range(13):
        per_leg.append(float(np.median(timed(call(starts[i:i + 1], goals[i:i + 1]), 3))) * 1e3)
    ref["each_leg_alone_ms"] = [round(v, 4) for v in per_leg]
    ref["per_leg_median_ms"] = round(float(np.median(per_leg)), 4)
    ref["us_per_pop"] = [round(1e3 * per_leg[i] / max(1, cpu_legs[i]["pops"]), 3) for i in range(13)]
    out["reference"] = ref
    # ---- FIELD
    sc.set_refine_search("field")
    fld = {}
    for n in (1, 13):
        fn = call(starts[:n], goals[:n])
        fld[f"legs_{n}"] = dict(cold=stats_ms(timed(fn, args.reps, before=lambda: sc.upload_grid(cells[None], origin, res))),
                                cached=stats_ms(timed(fn, args.reps)))
    out["field"] = fld
    # ---- one core
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    T.leg(cells, origin, res, starts[0], goals[0], which=T.REFERENCE)
    per = []
    for i in range(13):
        xs = []
        for _ in range(3):
            t0 = time.perf_counter(); T.leg(cells, origin, res, starts[i], goals[i], which=T.REFERENCE); xs.append(time.perf_counter() - t0)
        per.append(float(np.median(xs)) * 1e3)
    out["cpu"] = dict(each_leg_ms=[round(v, 4) for v in per], per_leg_median_ms=round(float(np.median(per)), 4),
                      legs_13_ms=round(float(np.sum(per)), 4), legs_1_ms=round(per[0], 4),
                      note="tr_leg allocates and clears its 512^2 node store per call, and runs the search twice on a leg without a path")
    json.dump(out, open(os.path.join(args.out, "reference_search_ref2d.json"), "w"), indent=1)
    # ---- the worst case: a safe goal in another component
    if not args.no_worst:
        sx, sy = int((starts[0][0] - origin[0]) / res), int((starts[0][1] - origin[1]) / res)
        field = T.field(cells, sx, sy)
        ys, xs_ = np.nonzero((field >= T.DBL_MAX) & (cells < 254))
        if xs_.size:
            goal = np.array([[origin[0] + (xs_[0] + 0.5) * res, origin[1] + (ys[0] + 0.5) * res]])
            e = S.leg(cells, origin, res, starts[0], goal[0])
            sc.set_refine_search("reference")
            fn = call(starts[:1], goal)
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            out["worst_case"] = dict(status=e["status"], pops=e["pops"], walks=e["los_walks"], largest_heap=e["max_heap"],
                                     reference_ms=round(dt * 1e3, 3), us_per_pop=round(1e6 * dt / max(1, e["pops"]), 3),
                                     reached_cells=int((field < T.DBL_MAX).sum()))
        else:
            out["worst_case"] = "every free cell of REF2D is reachable from start 0"
    sc.close()
    json.dump(out, open(os.path.join(args.out, "reference_search_ref2d.json"), "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
