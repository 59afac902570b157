#!/usr/bin/env python3
"""What a drive gated on Fisher information costs on the device (fs_drive_slam) beside the host loop over the calls
the library had before it — per step fs_trace_segments on the staged map and on the world, fs_sense, fs_sense_landmarks,
fs_score_fim (info only) and fs_goals_mapped — on the same build.  The host loop is the yardstick: it is not the code under test.

    python tools/drive_slam_probe.py [--reps 7] [--out profiles/sense/drive_slam_probe.json]

REF2D's 512 x 512 grid with an open world inside an outer wall, a world cloud of 100 000 landmarks uniform over the map up to 2 m
above the floor, none known; 1, 8 and 64 robots with 32 stations each, two cells between stations, looking along the row; goals
that are never mapped; gate off, so that every robot drives its whole list and both routes do the same work.  Before every timed
call the staged map goes back to all unknown and the world cloud to nothing discovered (not timed).  Two repeats warm up, the
median of the rest is reported: wall time of fs_drive_slam and of the host loop, the library calls and host waits of each, and
whether both routes leave the same map, counters, discovered set and integer outputs (they must) and information within 1e-4.
The figures are reported, not gated."""
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
WAITS, FALLBACKS = 1047, 1049
FIM = (6.0, 1.0)
SENSOR = dict(max_dist=6.0, max_angle=1.0, line_of_sight=1, min_views=1)


def host_loop(s, w, poses, goals, first, reach):
    """(status, reached, information, voxels, in_view, n_new, library calls): the gated drive by the existing calls, gate off"""
    R = len(poses)
    status, reached = np.full(R, DRIVING), np.zeros(R, dtype=np.int64)
    info = [np.zeros(p.shape[0], np.float32) for p in poses]
    vox = [np.zeros(p.shape[0], np.int32) for p in poses]
    view = [np.full(p.shape[0], -1, np.int32) for p in poses]
    n_new = calls = 0
    k = 0
    while (status == DRIVING).any():
        if k >= 1:
            for r in range(R):
                if status[r] == DRIVING and poses[r].shape[0] <= k:
                    status[r] = ARRIVED
            moving = [r for r in range(R) if status[r] == DRIVING]
            if moving:
                a, b = [poses[r][k - 1, :3] for r in moving], [poses[r][k, :3] for r in moving]
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
        here = np.stack([poses[r][k] for r in who])
        s.sense(here[:, :3], [first[r][k] for r in who])
        lm = s.sense_landmarks(here, SENSOR)
        fim = s.score_fim(here, info_only=True)
        mapped = s.goals_mapped(goals[who])
        calls += 4
        n_new += lm["n_new"]
        for j, r in enumerate(who):
            info[r][k], vox[r][k], view[r][k] = fim["info_ref"][j], fim["n_voxels"][j], lm["n_in_view"][j]
            if mapped[j]:
                status[r] = MAPPED
        k += 1
    return status, reached, info, vox, view, n_new, calls


def med(xs):
    return float(np.median(xs) * 1e3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense", "drive_slam_probe.json"))
    args = ap.parse_args()
    fs = importlib.import_module("fit-slam_amd")
    wl = fs.synth.make_workload("REF2D", n_cand=8, n_landmarks=8)
    nz, ny, nx = wl.cells.shape
    world = np.zeros((1, ny, nx), dtype=np.uint8)
    world[0, 0, :] = world[0, -1, :] = world[0, :, 0] = world[0, :, -1] = 254
    blank = np.full_like(world, 255)
    res, (ox, oy, oz) = wl.resolution, wl.origin
    rng = np.random.default_rng(3)
    cloud = np.stack([ox + rng.uniform(0.0, nx * res, 100000), oy + rng.uniform(0.0, ny * res, 100000), rng.uniform(0.0, 2.0, 100000)], 1).astype(np.float32)
    s, w = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    for c in (s, w):
        c.set_ray_params(max_camera_depth=wl.max_camera_depth, delta_theta=wl.delta_theta, camera_fov=wl.camera_fov,
                         robot_radius=wl.robot_radius, n_rays=wl.n_yaw, elev=wl.elev, polygon=wl.polygon)
    s.lookup_generate()
    s.set_fim_params(*FIM)
    s.upload_grid(blank, wl.origin, res)
    s.upload_world(world)
    w.upload_grid(world, wl.origin, res)
    east = s.first_ray_for_yaw(0.0)

    def reset():
        s.upload_grid(blank, wl.origin, res)
        s.upload_world_landmarks(cloud)

    out = {"what": "fs_drive_slam (gate off) against the host loop of fs_trace_segments (staged, world), fs_sense, fs_sense_landmarks, "
                   "fs_score_fim (info only) and fs_goals_mapped; ms, medians of wall time after two warm-up repeats",
           "grid": [nx, ny, nz], "fan": [s.n_yaw, s.n_elev, s.window], "world_landmarks": int(cloud.shape[0]), "fim": list(FIM),
           "reps": args.reps, "cases": []}
    ok = True
    n = 32
    for robots in (1, 8, 64):
        poses = []
        for r in range(robots):
            p = np.zeros((n, 7))
            p[:, 0] = (20 + 2 * np.arange(n) + 0.5) * res + ox
            p[:, 1] = (8 + 7 * r + 0.5) * res + oy
            p[:, 2] = oz
            p[:, 6] = 1.0                                                # looking east
            poses.append(p)
        first = [np.full(n, east, dtype=np.int32) for _ in range(robots)]
        goals = np.array([[ox - 1.0, oy - 1.0, oz]] * robots)            # off the map: never mapped
        t_dev, t_host, got, loop, waits = [], [], None, None, 0
        for _ in range(args.reps + 2):
            reset()
            t0 = time.perf_counter()
            got = s.drive_slam(poses, goals, first, lm_sensor=SENSOR, gate=False)
            t_dev.append(time.perf_counter() - t0)
            waits = s.get_counter(WAITS)
        merged, state = s.read_grid_region(), s.world_landmarks()
        for _ in range(args.reps + 2):
            reset()
            t0 = time.perf_counter()
            loop = host_loop(s, w, poses, goals, first, float(nx + ny))
            t_host.append(time.perf_counter() - t0)
        after = s.world_landmarks()
        same = bool(np.array_equal(s.read_grid_region(), merged) and np.array_equal(loop[0], got["status"]) and
                    np.array_equal(loop[1], got["reached"]) and loop[5] == got["n_new"] and
                    np.array_equal(after["views"], state["views"]) and np.array_equal(after["world_index"], state["world_index"]) and
                    all(np.array_equal(x, y) for x, y in zip(loop[3], got["voxels"])) and
                    all(np.array_equal(x, y) for x, y in zip(loop[4], got["in_view"])) and
                    all(np.allclose(x, y, rtol=1e-4, atol=0.0) for x, y in zip(got["information"], loop[2])))
        ok = ok and same and bool((got["reached"] == n - 1).all())
        d, h = med(t_dev[2:]), med(t_host[2:])
        out["cases"].append({"robots": robots, "stations_per_robot": n, "n_discovered": got["n_discovered"],
                             "largest_voxel_count": int(max(v.max() for v in got["voxels"])), "fs_drive_slam_ms": d, "host_loop_ms": h,
                             "fs_drive_slam_host_waits": int(waits), "host_loop_calls": loop[6], "speed_up": h / d if d > 0 else None,
                             "routes_agree": same})
    out["fallback_workgroups"] = int(s.get_counter(FALLBACKS))
    s.close(); w.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
