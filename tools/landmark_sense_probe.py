#!/usr/bin/env python3
"""What a landmark sweep on the device costs (fs_sense_landmarks) beside the route a caller needs without it:
fs_landmarks_in_view on a second context that holds the whole world cloud, the union of the lists on the host, then
fs_upload_landmarks of that union.

    python tools/landmark_sense_probe.py [--reps 9] [--landmarks 100000] [--out profiles/sense/landmark_sense_probe.json]

1 / 50 / 2 000 poses on REF2D and 50 poses on C3, a 100 k-point world cloud, the context's volume (14 m, 1.0 rad) with the line of
sight through the world grid.  Before every timed call the world cloud is staged afresh (not timed), so the call discovers what the
poses see and stages it; `again` is the same call repeated, which finds nothing new and stages nothing.  Per case: the median wall
time of the whole call, what it discovered, the median wall time of the host route and whether the two routes stage the same set
(they must).  The figures are reported, not gated: nothing else exists to compare against."""
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


def med(xs):
    return float(np.median(xs) * 1e3)


def poses_of(goals):
    """goal points as poses, the yaw stepping round the circle"""
    n = goals.shape[0]
    yaw = (np.arange(n) * 0.37) % (2 * np.pi) - np.pi
    p = np.zeros((n, 7))
    p[:, :3] = goals
    p[:, 5], p[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    return p


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--landmarks", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense", "landmark_sense_probe.json"))
    args = ap.parse_args()
    fs = importlib.import_module("fit-slam_amd")
    out = {"what": "fs_sense_landmarks on the device against fs_landmarks_in_view on a full-world context + union on the host + "
                   "fs_upload_landmarks; ms, medians of wall time", "reps": args.reps, "world_landmarks": args.landmarks, "cases": []}
    ok = True
    for name, counts in (("REF2D", (1, 50, 2000)), ("C3", (50,))):
        w = fs.synth.make_workload(name, n_cand=max(counts), n_landmarks=args.landmarks)
        world = np.array(w.cells, dtype=np.uint8, copy=True)
        world[world == 255] = 0
        cloud = np.ascontiguousarray(w.landmarks, dtype=np.float32)
        nz, ny, nx = world.shape
        dev, full = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
        for s in (dev, full):
            s.lookup_generate()
            s.set_fim_params(14.0, 1.0)
            s.upload_grid(world, w.origin, w.resolution)
        dev.upload_world(world)
        full.upload_landmarks(cloud)
        full.set_occlusion(True)
        for n in counts:
            poses = poses_of(w.goals[:n])
            t_dev, t_again, r = [], [], None
            for _ in range(args.reps + 2):
                dev.upload_world_landmarks(cloud)
                t0 = time.perf_counter()
                r = dev.sense_landmarks(poses)
                t_dev.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                dev.sense_landmarks(poses)
                t_again.append(time.perf_counter() - t0)
            index = dev.world_landmarks(views=False)["world_index"]
            t_host, union, entries = [], None, 0
            for _ in range(args.reps + 2):
                full.upload_landmarks(cloud)
                t0 = time.perf_counter()
                off, ent = full.landmarks_in_view(poses)
                union = np.unique(ent["index"])
                full.upload_landmarks(cloud[union])
                t_host.append(time.perf_counter() - t0)
                entries = int(off[-1])
            same = bool(np.array_equal(union, index))
            ok = ok and same
            out["cases"].append({"workload": name, "grid": [nx, ny, nz], "poses": n, "fs_sense_landmarks_ms": med(t_dev[2:]),
                                 "fs_sense_landmarks_again_ms": med(t_again[2:]), "sightings": int(r["n_in_view"].sum()),
                                 "n_discovered": int(r["n_discovered"]), "host_route_ms": med(t_host[2:]), "host_route_list_entries": entries,
                                 "routes_stage_the_same_set": same})
        dev.close(); full.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
