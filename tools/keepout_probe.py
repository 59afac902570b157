#!/usr/bin/env python3
"""What the keep-out layer costs a staging call, on REF2D (512 x 512) and on C3's shape reduced to one slice.

    python tools/keepout_probe.py [--reps 24] [--out profiles/keepout/keepout_ref2d.json]

Medians of wall time in ms over `reps` calls (at least 20):
  add_fov                  fs_keepout_add_fov on a staged grid (mark + fold on the bounding box, one wait for the count)
  window_64x64[n]          fs_update_grid_region of a 64 x 64 window with n = 0, 1, 16, 256 zones stored
  upload[n]                fs_upload_grid with the same zone counts, geometry unchanged (one apply launch over the map)
  upload_new_origin[n]     fs_upload_grid with the origin moved: every stored request is rasterised again (2 n launches)
and what the same caller has to do without the layer: mark the zone on the host and send its bounding box through
fs_update_grid_region (host_marked_bbox_window; the host rasterisation itself is NOT in the figure — it is Python here), and
the full fs_upload_grid (= upload[0]).  Host buffers are pageable numpy arrays, as a caller's costmap is.
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


def med(xs):
    return float(np.median(xs) * 1e3)


def timed(f, *a, **k):
    t0 = time.perf_counter()
    f(*a, **k)
    return time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keepout", "keepout_ref2d.json"))
    args = ap.parse_args()
    reps = max(args.reps, 20)
    fs = importlib.import_module("fit-slam_amd")
    import keepout_ref as K                                   # the host-side marking of the comparison
    out = {"what": "keep-out layer: staging calls with n zones stored; ms, medians of %d calls" % reps, "workloads": {}}
    ok = True
    for name in ("REF2D", "C3_one_slice"):
        w = fs.synth.make_workload("REF2D" if name == "REF2D" else "C3", n_cand=8)
        cells = np.array(w.cells, dtype=np.uint8, copy=True)[:1]
        _, ny, nx = cells.shape
        origin, res = tuple(float(v) for v in w.origin), float(w.resolution)
        moved = (origin[0] + 8 * res, origin[1] - 8 * res, origin[2])
        rng = np.random.default_rng(5)

        def zone():
            return (K.FOV, float(rng.uniform(origin[0] + 1.0, origin[0] + nx * res - 1.0)),
                    float(rng.uniform(origin[1] + 1.0, origin[1] + ny * res - 1.0)), float(rng.uniform(-np.pi, np.pi)), 3.5)

        rec = {"grid": [nx, ny], "resolution": res}
        s = fs.FrontierScorer(device=0)
        s.upload_grid(cells, origin, res)
        window = np.zeros((64, 64), np.uint8)
        zones = []
        for n in (0, 1, 16, 256):
            added = []
            while len(zones) < n:
                z = zone()
                added.append(timed(s.keepout_add_fov, *z[1:]))
                zones.append(z)
            if n == 256:
                rec["add_fov"] = med(added[-reps:])
            pos = [(int(rng.integers(0, nx - 64)), int(rng.integers(0, ny - 64))) for _ in range(reps)]
            rec["window_64x64[%d]" % n] = med([timed(s.update_grid_region, x0, y0, 0, window) for x0, y0 in pos])
            rec["upload[%d]" % n] = med([timed(s.upload_grid, cells, origin, res) for _ in range(reps)])
            if n:
                rec["upload_new_origin[%d]" % n] = med([timed(s.upload_grid, cells, moved if r % 2 == 0 else origin, res) for r in range(reps)])
                s.upload_grid(cells, origin, res)
        # the caller's route without the layer: host-marked bounding box through fs_update_grid_region
        geom = (nx, ny, origin[0], origin[1], res)
        plain = fs.FrontierScorer(device=0)
        plain.upload_grid(cells, origin, res)
        host = cells[0].copy()
        bbox = []
        for z in zones[:reps]:
            idx = np.unique(np.array(K.zone_indices(z, geom), dtype=np.int64))
            host.reshape(-1)[idx] = K.COST
            ys, xs = idx // nx, idx % nx
            x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
            bbox.append(timed(plain.update_grid_region, x0, y0, 0, host[y0:y1 + 1, x0:x1 + 1], view=True))
        rec["host_marked_bbox_window"] = med(bbox)
        # both routes give the same grid for those zones
        check = fs.FrontierScorer(device=0)
        check.upload_grid(cells, origin, res)
        for z in zones[:reps]:
            check.keepout_add_fov(*z[1:])
        same = bool(np.array_equal(check.read_grid_region()[0], plain.read_grid_region()[0]))
        rec["device_marked_equals_host_marked"] = same
        ok = ok and same
        out["workloads"][name] = rec
        for c in (s, plain, check):
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
