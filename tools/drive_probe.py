#!/usr/bin/env python3
"""What driving station lists on the device costs (fs_drive) beside the host loop over the calls it is made of —
fs_trace_segments on the staged map and on the world, fs_sense, fs_goals_mapped per step — on the same build.

    python tools/drive_probe.py [--reps 7] [--out profiles/sense/drive_probe.json]

REF2D's 512 x 512 grid with an open world inside an outer wall, so that every robot drives its whole list: one robot with 10, 50
and 200 stations and 8 robots with 50 stations each, two cells between stations, the FOV window looking along the row, goals that
are never mapped (the goal test runs at every step and never stops anybody).  The staged map starts all unknown before every
timed call (that snapshot is not timed).  Per case: the median wall time of fs_drive and of the host loop, the number of library
calls the loop made, and whether both routes leave the same staged map and the same outputs (they must).  The figures are
reported, not gated."""
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

DRIVING, ARRIVED, BLOCKED, COLLIDED, OFF_MAP, MAPPED = -1, 0, 1, 2, 3, 4


def host_loop(s, w, stations, goals, first, reach):
    """(status, reached, n_seen, n_revealed, library calls): the drive by the existing calls, all robots in lockstep"""
    R = len(stations)
    status, reached = np.full(R, DRIVING), np.zeros(R, dtype=np.int64)
    n_seen = n_revealed = calls = 0
    k = 0
    while (status == DRIVING).any():
        if k >= 1:
            for r in range(R):
                if status[r] == DRIVING and stations[r].shape[0] <= k:
                    status[r] = ARRIVED
            moving = [r for r in range(R) if status[r] == DRIVING]
            if moving:
                a, b = [stations[r][k - 1] for r in moving], [stations[r][k] for r in moving]
                on_s, on_w = s.trace_segments(a, b, reach), w.trace_segments(a, b, reach)
                calls += 2
                for j, r in enumerate(moving):
                    if not on_s["ok"][j]:
                        status[r] = OFF_MAP
                    elif on_s["hit"][j]:
                        status[r] = BLOCKED
                    elif on_w["hit"][j]:
                        status[r] = COLLIDED
                    else:
                        reached[r] = k
        who = [r for r in range(R) if status[r] == DRIVING]
        if not who:
            break
        got = s.sense([stations[r][k] for r in who], [first[r][k] for r in who])
        mapped = s.goals_mapped(goals[who])
        calls += 2
        n_seen += got["n_seen"]
        n_revealed += got["n_revealed"]
        for j, r in enumerate(who):
            if mapped[j]:
                status[r] = MAPPED
        k += 1
    return status, reached, n_seen, n_revealed, calls


def med(xs):
    return float(np.median(xs) * 1e3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense", "drive_probe.json"))
    args = ap.parse_args()
    fs = importlib.import_module("fit-slam_amd")
    wl = fs.synth.make_workload("REF2D", n_cand=8, n_landmarks=8)
    nz, ny, nx = wl.cells.shape
    world = np.zeros((1, ny, nx), dtype=np.uint8)
    world[0, 0, :] = world[0, -1, :] = world[0, :, 0] = world[0, :, -1] = 254
    blank = np.full_like(world, 255)
    res, (ox, oy, oz) = wl.resolution, wl.origin
    s, w = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    for c in (s, w):
        c.set_ray_params(max_camera_depth=wl.max_camera_depth, delta_theta=wl.delta_theta, camera_fov=wl.camera_fov,
                         robot_radius=wl.robot_radius, n_rays=wl.n_yaw, elev=wl.elev, polygon=wl.polygon)
    s.upload_grid(blank, wl.origin, res)
    s.upload_world(world)
    w.upload_grid(world, wl.origin, res)
    east = s.first_ray_for_yaw(0.0)
    out = {"what": "fs_drive against the host loop of fs_trace_segments (staged, world), fs_sense and fs_goals_mapped; ms, medians of wall time",
           "grid": [nx, ny, nz], "fan": [s.n_yaw, s.n_elev, s.window], "reps": args.reps, "cases": []}
    ok = True
    for robots, n in ((1, 10), (1, 50), (1, 200), (8, 50)):
        stations = [np.array([((20 + 2 * k + 0.5) * res + ox, (40 + 55 * r + 0.5) * res + oy, oz) for k in range(n)]) for r in range(robots)]
        first = [np.full(n, east, dtype=np.int32) for _ in range(robots)]
        goals = np.array([[ox - 1.0, oy - 1.0, oz]] * robots)            # off the map: never mapped
        t_dev, t_host, got, loop = [], [], None, None
        for _ in range(args.reps + 2):
            s.upload_grid(blank, wl.origin, res)
            t0 = time.perf_counter()
            got = s.drive(stations, goals, first)
            t_dev.append(time.perf_counter() - t0)
        merged = s.read_grid_region()
        for _ in range(args.reps + 2):
            s.upload_grid(blank, wl.origin, res)
            t0 = time.perf_counter()
            loop = host_loop(s, w, stations, goals, first, float(nx + ny))
            t_host.append(time.perf_counter() - t0)
        same = bool(np.array_equal(s.read_grid_region(), merged) and np.array_equal(loop[0], got["status"]) and
                    np.array_equal(loop[1], got["reached"]) and (loop[2], loop[3]) == (got["n_seen"], got["n_revealed"]))
        ok = ok and same and bool((got["reached"] == n - 1).all())
        d, h = med(t_dev[2:]), med(t_host[2:])
        out["cases"].append({"robots": robots, "stations_per_robot": n, "status": [int(v) for v in got["status"]],
                             "reached": [int(v) for v in got["reached"]], "n_seen": got["n_seen"], "n_revealed": got["n_revealed"],
                             "window": list(got["window"]), "fs_drive_ms": d, "host_loop_ms": h, "host_loop_calls": loop[4],
                             "speed_up": h / d if d > 0 else None, "routes_agree": same})
    s.close(); w.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
