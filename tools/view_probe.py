#!/usr/bin/env python3
"""What listing the landmarks in view (fs_landmarks_in_view) costs beside the scoring call, on the MI355X.

    python tools/view_probe.py [--out DIR] [--workloads REF2D,C3] [--poses 1,50,2000]
    python tools/view_probe.py --upload-only [--tree DIR] [--landmarks 100000]

Per workload (its cloud, its first frontiers at random yaws), visibility volume (the cone (14, 1.0) and the reference's own request
(14, 4.0)) and number of poses: the host wall-clock median of fs_landmarks_in_view in its count-only form and with room for every
entry, of fs_score_fim with full columns at the same poses (existing code: the yardstick), the ratios, the entries per pose and the
bytes the full call returns.  One JSON per workload: DIR/landmarks_in_view_<workload>.json (default DIR: profiles/view).

--upload-only times fs_upload_landmarks on a uniform cloud (what every upload now also pays: the kept permutation) and prints one
JSON line; --tree names the checkout whose package and library are used, so the same script measures a build of the parent
commit next to this one (alternate the two, a fresh process each).
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
VOLUMES = ((14.0, 1.0), (14.0, 4.0))


def med_us(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t0)
    return round(float(np.median(xs)) * 1e6, 1)


def probe(fs, name, counts):
    E = fs.capi
    L = fs.load_library()
    w = fs.synth.make_workload(name, n_cand=max(counts))
    rng = np.random.default_rng(31)
    poses = np.ascontiguousarray(fs.synth.poses_from_yaw(w.goals, rng.uniform(-np.pi, np.pi, size=w.goals.shape[0])), dtype=np.float64)
    sc = fs.FrontierScorer(device=0)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    out = dict(workload=name, n_landmarks=int(w.landmarks.shape[0]), clock="host wall clock, median, us", rows=[])
    for vis in VOLUMES:
        sc.set_fim_params(*vis)
        for n in counts:
            p = np.ascontiguousarray(poses[:n])
            reps = 30 if n <= 50 else 5
            off = np.zeros(n + 1, dtype=np.int64)

            def count_only():
                rc = L.fs_landmarks_in_view(sc._h, n, E._p(p), 0, E._p(off), None)
                assert rc == E.FS_OK, rc

            count_only()
            total = int(off[n])
            ent = np.zeros(max(total, 1), dtype=E.VIEW_DTYPE)

            def full():
                rc = L.fs_landmarks_in_view(sc._h, n, E._p(p), total, E._p(off), E._p(ent) if total else None)
                assert rc == E.FS_OK, rc

            row = dict(max_dist=vis[0], max_angle=vis[1], n_poses=n, reps=reps)
            row["view_count_only_us"] = med_us(count_only, reps)
            row["view_full_us"] = med_us(full, reps)
            row["score_fim_full_columns_us"] = med_us(lambda: sc.score_fim(p, want_fim=True), reps)
            if n == 1:
                row["score_fim_info_only_us"] = med_us(lambda: sc.score_fim(p, info_only=True), reps)
            row["count_only_over_score_fim"] = round(row["view_count_only_us"] / row["score_fim_full_columns_us"], 2)
            row["full_over_score_fim"] = round(row["view_full_us"] / row["score_fim_full_columns_us"], 2)
            row["entries_per_pose"] = round(total / n, 1)
            row["bytes_returned"] = total * E.VIEW_DTYPE.itemsize + (n + 1) * 8
            row["counts_equal_n_visible"] = bool(np.array_equal(np.diff(off), sc.score_fim(p, want_fim=False)["n_visible"]))
            out["rows"].append(row)
    sc.close()
    return out


def upload_only(fs, m, tree):
    rng = np.random.default_rng(3)
    lm = np.ascontiguousarray(rng.uniform(-12.0, 12.0, size=(m, 3)).astype(np.float32))
    lm[:, 2] = rng.uniform(0.0, 2.5, size=m)
    s = fs.FrontierScorer(device=0)
    ts = []
    for _ in range(23):
        t0 = time.perf_counter()
        s.upload_landmarks(lm)
        ts.append((time.perf_counter() - t0) * 1e3)
    s.close()
    ts = np.array(ts[3:])
    print(json.dumps(dict(tree=tree, landmarks=m, upload_landmarks_ms_median=round(float(np.median(ts)), 4), min=round(float(ts.min()), 4),
                          max=round(float(ts.max()), 4), runs=int(ts.size))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view"))
    ap.add_argument("--workloads", default="REF2D,C3")
    ap.add_argument("--poses", default="1,50,2000")
    ap.add_argument("--upload-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are measured (--upload-only)")
    ap.add_argument("--landmarks", type=int, default=100000)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree if args.upload_only else ROOT)
    sys.path.insert(0, tree)
    import torch  # noqa: F401  (before the library: both bind to one HIP runtime, as in bench.py)
    fs = importlib.import_module("fit-slam_amd")
    if args.upload_only:
        return upload_only(fs, args.landmarks, tree)
    os.makedirs(args.out, exist_ok=True)
    counts = [int(v) for v in args.poses.split(",")]
    for name in args.workloads.split(","):
        res = probe(fs, name, counts)
        path = os.path.join(args.out, f"landmarks_in_view_{name}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
