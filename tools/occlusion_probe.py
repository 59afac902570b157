#!/usr/bin/env python3
"""What line-of-sight visibility (fs_set_occlusion) costs in fs_score_fim, on the MI355X.

    python tools/occlusion_probe.py [--out DIR] [--workloads C3,REF2D] [--poses 1,50,2000]

Per workload (its map, its cloud, its first frontiers at random yaws) and number of poses: the host wall-clock median of
fs_score_fim with occlusion off and on (full columns; for one pose also the info-only form, isPoseSafe's call), their ratio, the
walks per pose (= landmarks the predicate accepts: n_visible with occlusion off), the share of them the rule hides, and the cells
per walk (fs_line_of_sight's tested_cells from a few poses to the landmarks in range).  The CPU figure is the composition the
tests check against — tests/occlusion_ref.py's restatement over the cloud, then the oracle on what is left — timed for ONE pose
on one core.  One JSON per workload: DIR/fim_occlusion_<workload>.json (default DIR: profiles/occlusion).
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

VIS = (14.0, 1.0)


def med_us(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t0)
    return round(float(np.median(xs)) * 1e6, 1)


def probe(fs, name, counts, with_cpu):
    w = fs.synth.make_workload(name, n_cand=max(counts))
    rng = np.random.default_rng(31)
    poses = fs.synth.poses_from_yaw(w.goals, rng.uniform(-np.pi, np.pi, size=w.goals.shape[0]))
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    sc.set_fim_params(*VIS)
    out = dict(workload=name, grid=list(w.cells.shape), resolution=w.resolution, n_landmarks=int(w.landmarks.shape[0]),
               max_dist=VIS[0], max_angle=VIS[1], occ=[254, 254], end_margin_m=0.3, clock="host wall clock, median, us", rows=[])
    for n in counts:
        p = poses[:n]
        reps = 30 if n <= 50 else 5
        row = dict(n_poses=n, reps=reps)
        for key, on in (("off", False), ("on", True)):
            sc.set_occlusion(on)
            row[f"score_fim_{key}_us"] = med_us(lambda: sc.score_fim(p, want_fim=False), reps)
            if n == 1:
                row[f"score_fim_info_only_{key}_us"] = med_us(lambda: sc.score_fim(p, info_only=True), reps)
            row[f"n_visible_{key}_mean"] = float(sc.score_fim(p, want_fim=False)["n_visible"].mean())
        row["on_over_off"] = round(row["score_fim_on_us"] / row["score_fim_off_us"], 2)
        row["walks_per_pose"] = row["n_visible_off_mean"]
        row["hidden_share"] = round(1.0 - row["n_visible_on_mean"] / max(row["n_visible_off_mean"], 1.0), 4)
        out["rows"].append(row)
    # cells per walk: the first poses' positions to every landmark in range
    lm64 = w.landmarks.astype(np.float64)
    cells = []
    for p in poses[:8]:
        t = p[:3].astype(np.float32).astype(np.float64)
        near = lm64[np.sum((lm64 - t) ** 2, axis=1) <= VIS[0] ** 2]
        if near.shape[0]:
            cells.append(sc.line_of_sight(np.repeat(t[None], near.shape[0], axis=0), near)["tested_cells"])
    if cells:
        c = np.concatenate(cells)
        out["cells_per_walk"] = dict(mean=float(c.mean()), max=int(c.max()), walks=int(c.size),
                                     note="tested_cells of the landmarks in range of 8 poses; a blocked walk stops earlier")
    sc.set_occlusion(False)
    if with_cpu:
        import occlusion_ref as OR
        import oracle as O
        G = O.Grid(w.cells, origin=w.origin, resolution=w.resolution)
        table = O.Table.generate()
        t0 = time.perf_counter()
        want = OR.occluded_pose_information(O, table, G, w.landmarks, poses[:1], *VIS)
        out["cpu_composition_one_pose_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        sc.set_occlusion(True)
        got = sc.score_fim(poses[:1], want_fim=False)
        sc.set_occlusion(False)
        out["cpu_composition_agrees"] = bool(got["n_visible"][0] == want["n_visible"][0] and got["n_voxels"][0] == want["n_voxels"][0])
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion"))
    ap.add_argument("--workloads", default="C3,REF2D")
    ap.add_argument("--poses", default="1,50,2000")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU composition (one pose, one core)")
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: both bind to one HIP runtime, as in bench.py)
    fs = importlib.import_module("fit-slam_amd")
    os.makedirs(args.out, exist_ok=True)
    counts = [int(v) for v in args.poses.split(",")]
    for name in args.workloads.split(","):
        res = probe(fs, name, counts, not args.no_cpu)
        path = os.path.join(args.out, f"fim_occlusion_{name}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
