#!/usr/bin/env python3
"""What the information layer costs on REF2D's 512 x 512 map with its workload's cloud, beside the host route it
replaces.

    python tools/information_layer_probe.py [--reps 24] [--out profiles/sense/information_layer_probe.json]

Medians of wall time in ms over `reps` calls (at least 20) after 3 warm-up calls, for strides 5 and 10 with K = 8 headings over
the whole map and over a 64 x 64 window:
  fs_information_layer   the call (anchors, compaction, records, the FIM worker, reduce / cost / store; two waits)
  host_route             fs_read_grid_region of the window, anchors and poses in numpy, fs_score_fim with info_only, the reduction,
                         the cost and the store in numpy, fs_update_grid_region of the window — with the parts also on their own
info_lo and info_hi are the quartiles of the field a first call returns (write = 0, not timed): REF2D's cloud puts every value far
above the reference's threshold of 550, and a layer that changes no byte would compare nothing.  The raw map is staged again before
every timed call (not timed).  Both routes must leave the same grid.  Host buffers are pageable
numpy arrays, as a caller's costmap is.
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

K, MAX_COST = 8, 252


def med(xs):
    return float(np.median(xs) * 1e3)


def anchors_numpy(window_cells, s):
    """the rule's anchors of a window given as its own array, vectorised: (anchor y, anchor x) per block in window cells, -1 for an
    unscored block"""
    sy, sx = window_cells.shape
    nby, nbx = -(-sy // s), -(-sx // s)
    y, x = np.arange(nby * s), np.arange(nbx * s)
    cy, cx = np.minimum(y // s * s + s // 2, sy - 1), np.minimum(x // s * s + s // 2, sx - 1)
    key = (((y - cy) ** 2)[:, None] + ((x - cx) ** 2)[None, :]) << 10 | (y % s)[:, None] << 5 | (x % s)[None, :]
    padded = np.full((nby * s, nbx * s), 255, dtype=np.uint8)
    padded[:sy, :sx] = window_cells
    key = np.where(padded <= 252, key, 1 << 30)
    best = key.reshape(nby, s, nbx, s).transpose(0, 2, 1, 3).reshape(nby, nbx, s * s).min(axis=2)
    ok = best < (1 << 30)
    ay = np.where(ok, np.arange(nby)[:, None] * s + (best >> 5 & 31), -1)
    ax = np.where(ok, np.arange(nbx)[None, :] * s + (best & 31), -1)
    return ay, ax


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense", "information_layer_probe.json"))
    args = ap.parse_args()
    reps, warm = max(args.reps, 20), 3
    fs = importlib.import_module("fit-slam_amd")
    import information_layer_ref as L
    w = fs.synth.make_workload("REF2D", n_cand=8)
    cells = np.array(w.cells, dtype=np.uint8, copy=True)[0]
    ny, nx = cells.shape
    origin, res = tuple(float(v) for v in w.origin), float(w.resolution)
    assert (ny, nx) == (512, 512)
    out = {"what": "fs_information_layer beside read_grid_region + numpy poses + fs_score_fim(info_only) + numpy reduce / cost / store + "
                   "update_grid_region; ms, medians of %d calls after %d warm-up calls; 512 x 512 map, %d landmarks, K = %d, mean, "
                   "info_lo / info_hi the field's quartiles" % (reps, warm, w.landmarks.shape[0], K),
           "grid": [nx, ny], "landmarks": int(w.landmarks.shape[0]), "cases": {}}
    ok = True
    dev, host = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    for sc in (dev, host):
        sc.upload_landmarks(w.landmarks)
        sc.lookup_generate()
    quat = L.quat_zw(K)
    for s in (5, 10):
        for wname, win in (("whole_map", (0, 0, nx, ny)), ("window_64x64", (224, 224, 64, 64))):
            x0, y0, sx, sy = win
            dev.upload_grid(cells, origin, res)
            field = dev.information_layer(stride_cells=s, n_yaw=K, window=win, write=False).info
            LO, HI = (float(v) for v in np.percentile(field[~np.isnan(field)], (25, 75)))
            t_dev, t_read, t_pose, t_fim, t_host, t_write, got = [], [], [], [], [], [], None
            for r in range(warm + reps):
                dev.upload_grid(cells, origin, res)
                t0 = time.perf_counter()
                got = dev.information_layer(stride_cells=s, n_yaw=K, info_lo=LO, info_hi=HI, max_cost=MAX_COST, window=win)
                t_dev.append(time.perf_counter() - t0)
                host.upload_grid(cells, origin, res)
                t0 = time.perf_counter()
                grown = host.read_grid_region(x0, y0, 0, shape=(sy, sx))
                t1 = time.perf_counter()
                ay, ax = anchors_numpy(grown, s)
                scored = ay >= 0
                pose7 = np.zeros((int(scored.sum()), K, 7))
                pose7[:, :, 0] = (origin[0] + ((ax[scored] + x0).astype(np.float64) + 0.5) * res)[:, None]
                pose7[:, :, 1] = (origin[1] + ((ay[scored] + y0).astype(np.float64) + 0.5) * res)[:, None]
                pose7[:, :, 5] = quat[None, :, 0]
                pose7[:, :, 6] = quat[None, :, 1]
                t2 = time.perf_counter()
                values = host.score_fim(pose7.reshape(-1, 7), info_only=True)["info_ref"].reshape(-1, K)
                t3 = time.perf_counter()
                total = np.zeros(values.shape[0])
                for k in range(K):
                    total = total + values[:, k].astype(np.float64)
                cost = np.zeros(scored.shape, dtype=np.uint8)
                cost[scored] = L.cost_of((total / K).astype(np.float32), LO, HI, MAX_COST)
                per_cell = np.kron(cost, np.ones((s, s), dtype=np.uint8))[:sy, :sx]
                grown[...] = np.where(grown <= 252, np.maximum(grown, per_cell), grown)
                t4 = time.perf_counter()
                host.update_grid_region(x0, y0, 0, grown, view=True)
                t5 = time.perf_counter()
                t_read.append(t1 - t0); t_pose.append(t2 - t1); t_fim.append(t3 - t2); t_host.append(t4 - t3); t_write.append(t5 - t4)
            same = bool(np.array_equal(dev.read_grid_region(), host.read_grid_region()))
            ok = ok and same
            total_t = [a + b + c + d + e for a, b, c, d, e in zip(t_read, t_pose, t_fim, t_host, t_write)]
            out["cases"]["stride_%d/%s" % (s, wname)] = {
                "stride_cells": s, "window": list(win), "info_lo": LO, "info_hi": HI, "n_scored": got.n_scored, "poses": got.n_scored * K, "n_changed": got.n_changed,
                "fs_information_layer": med(t_dev[warm:]), "host_route": med(total_t[warm:]), "host_read_grid_region": med(t_read[warm:]),
                "host_anchors_and_poses": med(t_pose[warm:]), "host_fs_score_fim": med(t_fim[warm:]), "host_reduce_cost_store": med(t_host[warm:]),
                "host_update_grid_region": med(t_write[warm:]), "both_routes_leave_the_same_grid": same}
    dev.close(); host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
