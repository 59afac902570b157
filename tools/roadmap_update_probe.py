#!/usr/bin/env python3
"""What fs_roadmap_update (UpdateRoadmapBT decided on the device) costs against the three calls it replaces —
fs_roadmap_add_nodes, fs_roadmap_add_nodes(robot pose), fs_roadmap_connect — on a second context with the same roadmap.

    python tools/roadmap_update_probe.py [--out DIR] [--reps N]      # on the MI355X -> update_ref2d.json

`ticks`: the ten simulated REF2D ticks of tools/roadmap_probe.py (the goal points of fs_frontier_clusters' clusters from the robot,
the robot pose).  Each tick is applied once to both contexts (the graphs are compared), then timed warm: the same list again changes
nothing (every point is a duplicate, every edge exists) and does the same closest-node searches, candidate lists and walks.  Host
wall clock around the call(s), which synchronise; medians.  Two settings per side: back to back, where every call finds the device
copy of the graph one generation old and uploads it again, and with an untimed fs_roadmap_plan between the timed calls, as in a
tick loop, which leaves the graph of the current generation on the device.
`long`: a free 52 m map with 20 000 nodes (tools/roadmap_kf_probe.py's long case, radius_to_decide_edges 1.5), rebuilt, then an
update of 430 points spread over it.  Output directory: profiles/roadmap (default).
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
import roadmap_ref as R  # noqa: E402
import roadmap_probe as RP  # noqa: E402  (REF2D and its robot cells)

RES = 0.05


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def timed(fn, reps, between=None):
    xs = []
    for _ in range(reps):
        if between:
            between()
        t0 = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t0)
    return med_ms(xs)


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("xy", "key", "row_ptr", "col"))


def pair(fs, cells, origin, params):
    out = []
    for _ in range(2):
        sc = fs.FrontierScorer(device=0)
        sc.upload_grid(cells[None] if cells.ndim == 2 else cells, origin, RES)
        sc.set_roadmap_params(*params)
        out.append(sc)
    return out


def measure(new, old, pts, robot, reps):
    """one tick: applied once to both (compared), then timed warm on both"""
    both = np.concatenate([pts, robot[None]])

    def three():
        if pts.shape[0]:
            old.roadmap_add_nodes(pts)
        old.roadmap_add_nodes(robot[None], is_robot_pose=True)
        old.roadmap_connect(both)

    t0 = time.perf_counter(); out = new.roadmap_update(pts, robot); first_new = time.perf_counter() - t0
    t0 = time.perf_counter(); three(); first_old = time.perf_counter() - t0
    assert same(new.roadmap_graph(), old.roadmap_graph()), "the two contexts disagree"
    pose = R.pose7(*robot, 0.7)
    goal = np.zeros((1, 3)); goal[0, :2] = both[0]
    row = dict(points=int(pts.shape[0]), nodes=int(new.roadmap_graph()["xy"].shape[0]), edges=int(new.roadmap_graph()["col"].size),
               update_first_ms=round(first_new * 1e3, 4), three_calls_first_ms=round(first_old * 1e3, 4),
               nodes_added=out["n_nodes_added"] + int(out["robot_added"]), edges_added=out["n_edges_added"])
    old.get_counter(1007, reset=True)
    row["three_calls_ms"] = timed(three, reps)
    row["three_calls_walks"] = int(old.get_counter(1007, reset=True) // reps)
    row["update_ms"] = timed(lambda: new.roadmap_update(pts, robot), reps)
    row["update_walks"], row["update_owners"] = int(new.get_counter(1033)), int(new.get_counter(1034))
    row["three_calls_after_plan_ms"] = timed(three, reps, between=lambda: old.roadmap_plan(pose, goal))
    row["update_after_plan_ms"] = timed(lambda: new.roadmap_update(pts, robot), reps, between=lambda: new.roadmap_plan(pose, goal))
    assert same(new.roadmap_graph(), old.roadmap_graph()), "the two contexts disagree after the timed calls"
    return row


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    fs = importlib.import_module("fit-slam_amd")
    w = RP.ref2d()
    cells = np.ascontiguousarray(w.cells[0])
    ticks = R.grow_ticks(fs, cells, w.origin, RES, RP.robot_cells(cells))
    new, old = pair(fs, cells, w.origin, (1.0, 6.1, 0.25, 0.25))
    rows = []
    for t, (fr, robot) in enumerate(ticks):
        row = dict(tick=t)
        row.update(measure(new, old, fr, robot, a.reps))
        rows.append(row)
        print(json.dumps(row), flush=True)
    new.close(); old.close()

    # the long case: 20 000 nodes on a free 52 m map, rebuilt (radius 1.5), then 430 points over it
    side, n_cells = 48, 2223
    sub = [(0.15 + 0.35 * i, 0.15 + 0.35 * j) for i in range(3) for j in range(3)]
    nodes = np.array([(c % side + dx, c // side + dy) for c in range(n_cells) for dx, dy in sub][:20000])
    big = np.zeros((1040, 1040), np.uint8)
    new, old = pair(fs, big, (-2.0, -2.0, 0.0), (1.0, 1.5, 0.25, 0.25))
    for sc in (new, old):
        sc.roadmap_add_nodes(nodes)
        sc.roadmap_rebuild()
    rng = np.random.default_rng(3)
    pts = rng.uniform(0.0, 47.0, (430, 2))
    long_row = measure(new, old, pts, np.array([24.0, 24.0]), a.reps)
    print(json.dumps(long_row), flush=True)
    new.close(); old.close()

    res = dict(what="fs_roadmap_update against fs_roadmap_add_nodes x 2 + fs_roadmap_connect on a second context, same roadmap; host wall "
                    "ms around synchronising calls, warm, medians of %d; *_after_plan: an untimed fs_roadmap_plan between the timed calls" % a.reps,
               ref2d_ticks=rows, long_20000_nodes=long_row)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "update_ref2d.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
