#!/usr/bin/env python3
"""What the inflation layer costs on REF2D's 512 x 512 map, beside the host route it replaces.

    python tools/inflate_probe.py [--reps 24] [--out profiles/sense/inflate_probe.json]

Medians of wall time in ms over `reps` calls (at least 20) after 3 warm-up calls, for R = 100, 12 and 6 cells (the reference's
global inflation_layer, its local costmap's, its lethal_inflation_layer) over the whole map and over a 64 x 64 window:
  fs_inflate     the call (two launches, the re-cut of the class image's bricks, one wait for the counters)
  host_route     fs_read_grid_region of the window grown by R, a C-speed host inflation (scipy's Euclidean feature transform, the
                 cost table, the write rule in numpy: tests/inflation_ref.py), fs_update_grid_region of the window — with the
                 three parts also on their own
The raw map is staged again before every timed call (not timed): a second inflation of the same map changes nothing.  Both routes
must leave the same grid.  Host buffers are pageable numpy arrays, as a caller's costmap is.
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

PARAMS = {"R100_global": (5.0, 0.05, 0.6), "R12_local": (0.60, 0.05, 0.6), "R6_lethal": (0.3, 0.05, 0.6)}


def med(xs):
    return float(np.median(xs) * 1e3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense", "inflate_probe.json"))
    args = ap.parse_args()
    reps, warm = max(args.reps, 20), 3
    fs = importlib.import_module("fit-slam_amd")
    import inflation_ref as I
    w = fs.synth.make_workload("REF2D", n_cand=8)
    cells = np.array(w.cells, dtype=np.uint8, copy=True)[0]
    # the raw map a sensor sweep leaves: free, lethal, unknown (the synthetic map's hand-painted band goes back to free)
    cells[(cells != 254) & (cells != 255)] = 0
    ny, nx = cells.shape
    origin, res = tuple(float(v) for v in w.origin), 0.05
    assert (ny, nx) == (512, 512) and (cells == 254).any()
    out = {"what": "fs_inflate beside read_grid_region + host inflation (scipy EDT + table) + update_grid_region; ms, medians of %d calls "
                   "after %d warm-up calls; 512 x 512 map, resolution 0.05" % (reps, warm),
           "grid": [nx, ny], "lethal_cells": int((cells == 254).sum()), "unknown_cells": int((cells == 255).sum()), "cases": {}}
    ok = True
    dev, host = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    for name, params in PARAMS.items():
        R = I.cell_radius(params, res)
        for wname, win in (("whole_map", (0, 0, nx, ny)), ("window_64x64", (224, 224, 64, 64))):
            x0, y0, sx, sy = win
            gx0, gy0, gx1, gy1 = max(0, x0 - R), max(0, y0 - R), min(nx, x0 + sx + R), min(ny, y0 + sy + R)
            t_dev, t_read, t_host, t_write, counts = [], [], [], [], None
            for r in range(warm + reps):
                dev.upload_grid(cells, origin, res)
                t0 = time.perf_counter()
                counts = dev.inflate(*params, window=win)
                t_dev.append(time.perf_counter() - t0)
                host.upload_grid(cells, origin, res)
                t0 = time.perf_counter()
                grown = host.read_grid_region(gx0, gy0, 0, shape=(gy1 - gy0, gx1 - gx0))
                t1 = time.perf_counter()
                inflated = I.inflate_exact(grown, params, res, window=(x0 - gx0, y0 - gy0, sx, sy), method="edt")[0]
                t2 = time.perf_counter()
                host.update_grid_region(x0, y0, 0, inflated[y0 - gy0:y0 - gy0 + sy, x0 - gx0:x0 - gx0 + sx], view=True)
                t3 = time.perf_counter()
                t_read.append(t1 - t0); t_host.append(t2 - t1); t_write.append(t3 - t2)
            same = bool(np.array_equal(dev.read_grid_region(), host.read_grid_region()))
            ok = ok and same
            total = [a + b + c for a, b, c in zip(t_read, t_host, t_write)]
            out["cases"]["%s/%s" % (name, wname)] = {
                "R": R, "window": list(win), "n_seeds": counts[0], "n_changed": counts[1], "fs_inflate": med(t_dev[warm:]),
                "host_route": med(total[warm:]), "host_read_grid_region": med(t_read[warm:]), "host_inflation": med(t_host[warm:]),
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
