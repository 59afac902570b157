#!/usr/bin/env python3
"""What the robot-footprint disc costs fs_raymarch_kernel: the production library against the build in which the scan is
compiled out (FS_RAY_ABLATE_DISC — timing only, its `achievable` is wrong by construction and nothing else loads it), on C3
(class walk, four rings) and on REF2D (byte walk, one ring), alternating A / B / A / B in ONE process, hipEvent per launch.

    FS_RAY_ABLATE_DISC=1 python fit-slam_amd/_build.py          # once, where the compiler is (the probe builds nothing)
    python tools/ray_disc_probe.py [--workloads C3,REF2D] [--rounds 4] [--steps 10] [--build NAME=LIBRARY ...] [--out FILE]

Builds: `production` (the tree's library) and `ablated` unless --build names others — any library with the same C ABI, e.g. the
library of another checkout (`--build parent=/path/to/libfitslam_frontier.so`) or another FS_RAY_DISC_BATCH.  The first build is
the yardstick: every other build's kernel time is given as a gain over it, and every build must return its records unless its
name says `ablated`.

FETCH_SIZE comes from a counter run of its own per build (counters perturb the timing; one build per process keeps the rows
apart), the interpreter by its real path behind `--`:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR_A -- $(realpath $(which python3)) tools/ray_disc_probe.py \
        --workloads C3 --build production --rounds 1 --steps 4
    python tools/ray_disc_probe.py --no-gpu --merge FILE --fetch production=DIR_A --fetch ablated=DIR_B --out FILE

Prints (and with --out writes) one JSON object.
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fetch_size(d: str) -> dict:
    """mean FETCH_SIZE (KiB as rocprofv3 reports it, and MB) per fs_raymarch_kernel dispatch of a --pmc run's output directory"""
    vals = []
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "fs_raymarch_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "FETCH_SIZE":
                vals.append(float(r["Counter_Value"]))
    if not vals:
        return {"dispatches": 0}
    # (the first dispatches of a process are fs_max_arrival's one-candidate calibration fan and the warm-up: the median is a step's)
    med = float(np.median(vals))
    return {"dispatches": len(vals), "FETCH_SIZE_KiB_median": med, "MB_median": med * 1024 / 1e6, "FETCH_SIZE_KiB_max": float(max(vals))}


def measure(args, builds) -> dict:
    import torch                                   # (before the HIP library: both must bind to one runtime)
    fs = importlib.import_module("fit-slam_amd")
    shard = importlib.import_module("fit-slam_amd.shard")
    dev = torch.device("cuda", 0)
    libs = {name: fs.capi.load_library(build=False, path=path) for name, path in builds.items()}
    out = {}
    for wl in args.workloads.split(","):
        t0 = time.time()
        w = fs.synth.make_workload(wl)
        print(f"[disc] {wl}: workload built in {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        st = torch.cuda.Stream(device=dev)
        n = w.goals.shape[0]
        d_goal = torch.from_numpy(np.ascontiguousarray(w.goals)).to(dev)
        d_fs = torch.from_numpy(w.frontier_size).to(dev)
        d_bl = torch.from_numpy(w.blacklisted).to(dev)
        d_rec = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        scs = {}
        for name, L in libs.items():
            sc = fs.FrontierScorer(device=0, stream=st.cuda_stream, library=L)
            sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                              robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
            sc.upload_grid(w.cells, w.origin, w.resolution)
            sc.upload_landmarks(w.landmarks); sc.lookup_generate(); sc.set_fim_params(14.0, 1.0)
            sc.max_arrival()
            scs[name] = sc
        times = {name: [] for name in scs}
        recs = {}
        with torch.cuda.stream(st):
            for rnd in range(args.rounds):
                for name, sc in scs.items():
                    for _ in range(3):
                        sc.score_candidates_dev(n, d_goal.data_ptr(), d_fs.data_ptr(), d_bl.data_ptr(), 0, d_rec.data_ptr())
                    torch.cuda.synchronize(dev)
                    sc.enable_kernel_timing(True)
                    sc.kernel_time(0)
                    for _ in range(args.steps):
                        sc.score_candidates_dev(n, d_goal.data_ptr(), d_fs.data_ptr(), d_bl.data_ptr(), 0, d_rec.data_ptr())
                    torch.cuda.synchronize(dev)
                    ms, cnt = sc.kernel_time(0)
                    sc.enable_kernel_timing(False)
                    times[name].append(ms / max(cnt, 1))
                    if rnd == 0:
                        recs[name] = shard.records_to_numpy(d_rec).copy()
        first = next(iter(scs))
        base = float(np.median(times[first]))
        res = {"grid": list(w.cells.shape), "candidates": int(n), "rays_per_candidate": scs[first].n_yaw * scs[first].n_elev,
               "footprint_side_cells": 2 * int(np.ceil(w.robot_radius / w.resolution)) + 1,
               "share_of_candidates_scanned": float(np.mean(w.frontier_size < 10)), "yardstick": first, "builds": {}}
        for name in scs:
            med = float(np.median(times[name]))
            res["builds"][name] = {"fs_raymarch_kernel_ms": med, "rounds_ms": times[name], "range_ms": float(max(times[name]) - min(times[name])),
                                   "gain_over_yardstick_pct": 100.0 * (base - med) / base}
            if "ablated" not in name:
                res["builds"][name]["records_equal_yardstick"] = bool(all(np.array_equal(recs[name][k], recs[first][k]) for k in ("arrival", "argmax", "flags", "n_visible")))
        for sc in scs.values():
            sc.close()
        out[wl] = res
        del w, d_goal, d_rec
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,REF2D")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--build", action="append", default=[], metavar="NAME[=LIBRARY]", help="production | ablated | NAME=path of a library; the first is the yardstick")
    ap.add_argument("--fetch", action="append", default=[], metavar="NAME=DIR", help="output directory of that build's rocprofv3 --pmc FETCH_SIZE run")
    ap.add_argument("--no-gpu", action="store_true", help="measure nothing: only --merge / --fetch")
    ap.add_argument("--merge", metavar="FILE", help="start from this earlier result")
    ap.add_argument("--out", metavar="FILE")
    args = ap.parse_args()
    _build = importlib.import_module("fit-slam_amd._build")
    known = {"production": _build.LIB, "ablated": _build.dev_library(["-DFS_RAY_ABLATE_DISC"])}
    builds = {}
    for b in args.build or ["production", "ablated"]:
        name, _, path = b.partition("=")
        builds[name] = os.path.abspath(path) if path else known[name]
        if not os.path.exists(builds[name]):
            raise SystemExit(f"{builds[name]} is missing: build it first (ablated: FS_RAY_ABLATE_DISC=1 python fit-slam_amd/_build.py)")
    out = json.load(open(args.merge)) if args.merge else {
        "what": "fs_raymarch_kernel per launch (hipEvent, median over the rounds of `steps` launches each, builds alternating in one process)"}
    if not args.no_gpu:
        out["rounds"], out["steps"] = args.rounds, args.steps
        out.setdefault("workloads", {}).update(measure(args, builds))
    for f in args.fetch:
        name, _, d = f.partition("=")
        out.setdefault("fetch_size_per_launch_C3", {})[name] = fetch_size(d)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
