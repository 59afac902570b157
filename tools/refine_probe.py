#!/usr/bin/env python3
"""What the leg refinement on the device (fs_refine_paths) costs, and how far its restated definition lies from the
reference's Theta* search.  On the MI355X:

    python tools/refine_probe.py [--out DIR] [--reps N]     # -> DIR/device_ref2d.json, DIR/reference_vs_field.json (default profiles/refine)

On REF2D's map (allow_unknown, w_euc 1, w_traversal 2, 8 corners, as computePathBetweenPointsThetaStar plans):
* device: one fs_refine_paths call (the filling call, output arrays sized beforehand) for 1 leg and for 13 legs from 13 distinct
  starts, cold (a grid upload first: every field is built) and cached (the same call again); the sizing call (NULL point arrays)
  cached; refine_field's field build alone.  Host wall clock around calls that end in a synchronisation; medians of --reps.
* reference: the host time of the restatement's `reference` leg (tests/thetastar_ref.cpp: the reference's search, one core) per
  leg, and per leg the cost and the path length (sum of the vertex segments, metres) of the `reference` leg against the `field`
  leg: median, p95, and how many are lower / equal / higher, over --legs random legs on REF2D and two floor plans.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import thetastar_ref as T  # noqa: E402


def stats_ms(xs):
    return dict(median_ms=round(float(np.median(xs)) * 1e3, 4), min_ms=round(float(np.min(xs)) * 1e3, 4),
                max_ms=round(float(np.max(xs)) * 1e3, 4), reps=len(xs))


def points(cells, origin, res, rng, k):
    ys, xs = np.nonzero(cells < 254)
    i = rng.choice(xs.size, k, replace=False)
    return np.stack([origin[0] + (xs[i] + rng.uniform(0, 1, k)) * res, origin[1] + (ys[i] + rng.uniform(0, 1, k)) * res], axis=1)


def dist_summary(d):
    d = np.asarray(d, dtype=np.float64)
    return dict(n=int(d.size), median=float(np.median(d)), p95=float(np.percentile(d, 95)), p5=float(np.percentile(d, 5)),
                max_abs=float(np.abs(d).max()), lower=int((d < 0).sum()), equal=int((d == 0).sum()), higher=int((d > 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", type=int, default=120)
    args = ap.parse_args()
    import torch  # noqa: F401  (the same load order as bench.py)
    fs = importlib.import_module("fit-slam_amd")
    w = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=16)
    cells, res = np.ascontiguousarray(w.cells[0]), float(w.resolution)
    origin = tuple(float(v) for v in w.origin)
    rng = np.random.default_rng(4077)
    starts, goals = points(cells, origin, res, rng, 13), points(cells, origin, res, rng, 13)
    sc = fs.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, res)
    L = sc._L

    def call(n, fill=True):
        s, g = np.ascontiguousarray(starts[:n]), np.ascontiguousarray(goals[:n])
        st, cost = np.zeros(n, np.int32), np.zeros(n)
        nv, npz = np.zeros(n, np.int32), np.zeros(n, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        sc._check(L.fs_refine_paths(sc._h, n, vp(s), vp(g), 1, 1.0, 2.0, 8, vp(st), vp(cost), vp(nv), None, vp(npz), None))
        if not fill:
            return lambda: sc._check(L.fs_refine_paths(sc._h, n, vp(s), vp(g), 1, 1.0, 2.0, 8, vp(st), vp(cost), vp(nv), None, vp(npz), None))
        vert, pose = np.zeros((int(nv.sum()) + 1, 2)), np.zeros((int(npz.sum()) + 1, 2))
        return lambda: sc._check(L.fs_refine_paths(sc._h, n, vp(s), vp(g), 1, 1.0, 2.0, 8, vp(st), vp(cost), vp(nv), vp(vert), vp(npz), vp(pose)))

    device = dict(map="REF2D", shape=list(cells.shape), resolution=res, params=dict(allow_unknown=1, w_euc=1.0, w_traversal=2.0, corners=8))
    for n in (1, 13):
        fn = call(n)
        for _ in range(2):
            fn()
        cold, cached = [], []
        for _ in range(args.reps):
            sc.upload_grid(cells[None], origin, res)          # drops every field
            t0 = time.perf_counter(); fn(); cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); fn(); cached.append(time.perf_counter() - t0)
        rounds = sc.get_counter(1012)
        device[f"legs_{n}"] = dict(cold=stats_ms(cold), cached=stats_ms(cached), field_rounds_last=rounds)
        size_fn = call(n, fill=False)
        xs = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); size_fn(); xs.append(time.perf_counter() - t0)
        device[f"legs_{n}"]["sizing_call_cached"] = stats_ms(xs)
    sc.get_counter(1011, reset=True)
    xs = []
    for _ in range(args.reps):
        sc.upload_grid(cells[None], origin, res)
        t0 = time.perf_counter(); sc.refine_field(starts[0]); xs.append(time.perf_counter() - t0)
    device["refine_field_cold"] = stats_ms(xs)
    device["fields_built_in_refine_field_loop"] = sc.get_counter(1011)
    sc.close()

    # the reference's search on the host, and the reference leg against the field leg
    maps = [("REF2D", cells, origin)]
    prng = np.random.Generator(np.random.PCG64(99))
    for n in (192, 256):
        c = np.ascontiguousarray(fs.synth.make_grid(prng, n, 1)[0])
        maps.append((f"plan_{n}", c, (-n * res / 2, -n * res / 2)))
    T.lib()                                                     # (compiled once here, not inside the first timed leg)
    host_ms, dcost, dlen, rel_cost, quirks, both, total = [], [], [], [], 0, 0, 0
    per_map = {}
    for name, c, o in maps:
        r2 = np.random.default_rng(len(name))
        k = args.legs // len(maps)
        s, g = points(c, o, res, r2, k), points(c, o, res, r2, k)
        q = 0
        for a, b in zip(s, g):
            t0 = time.perf_counter()
            ref = T.leg(c, o, res, a, b, which=T.REFERENCE)
            host_ms.append(time.perf_counter() - t0)
            fld = T.leg(c, o, res, a, b)
            total += 1
            if ref["status"] == T.OK and fld["status"] == T.OK:
                both += 1
                dcost.append(fld["cost"] - ref["cost"])
                rel_cost.append((fld["cost"] - ref["cost"]) / ref["cost"])
                lf = float(np.linalg.norm(np.diff(fld["vertices"], axis=0), axis=1).sum())
                lr = float(np.linalg.norm(np.diff(ref["vertices"], axis=0), axis=1).sum())
                dlen.append(lf - lr)
            elif fld["status"] == T.OK and ref["quirk"]:
                q += 1
        quirks += q
        per_map[name] = dict(legs=k, quirk=q)
    cmp = dict(maps=per_map, legs=total, both_found=both, reference_loop_quirk=quirks,
               reference_host_ms=stats_ms(host_ms),
               cost_field_minus_reference=dist_summary(dcost), cost_relative=dist_summary(rel_cost),
               length_m_field_minus_reference=dist_summary(dlen))
    os.makedirs(args.out, exist_ok=True)
    for fname, obj in (("device_ref2d.json", device), ("reference_vs_field.json", cmp)):
        with open(os.path.join(args.out, fname), "w") as f:
            json.dump(obj, f, indent=1)
    print(json.dumps(dict(device=device, compare=cmp), indent=1))


if __name__ == "__main__":
    main()
