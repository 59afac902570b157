#!/usr/bin/env python3
"""What the frontier roadmap on the device (fs_roadmap_*) costs against the CPU restatement of the reference's
host code, and how far the tree's paths are from the per-goal A*'s.

    python tools/roadmap_probe.py deviation [--out DIR]   # CPU only: tree vs reference_astar on the test maps -> astar_vs_tree.json
    python tools/roadmap_probe.py gpu       [--out DIR] [--search tree|reference]   # on the MI355X -> gpu_ref2d.json and cpu_ref2d.json
    python tools/roadmap_probe.py astar     [--out DIR]   # on the MI355X: both roadmap searches -> astar_gpu_ref2d.json

`gpu` grows a roadmap on REF2D the way UpdateRoadmapBT does — per simulated tick, the goal points of fs_frontier_clusters' clusters
from the robot added as nodes, the robot pose added, both connected (constructNewEdges) — and after every tick times (host wall
clock, medians) fs_roadmap_rebuild, fs_roadmap_connect of the tick's list, fs_roadmap_plan for 50 and 2 000 frontiers with a fresh
and a cached tree, and fs_get_frontier_costs_roadmap for 50 frontiers.  The restatement's legs (rebuild, connect, the per-goal A*)
are timed on ONE core in a child process (`cpu-legs`) on the same node lists; the one-call form is compared with the restatement's
A* followed by fs_get_frontier_costs.  --search reference plans with the reference's per-goal A* (fs_set_roadmap_search) and
writes gpu_ref2d_reference.json instead.  `astar` times, on REF2D's roadmap of the tests (nodes on free cells, rebuilt), the two
roadmap searches side by side — fs_roadmap_plan at 50 and 2 000 frontiers, fs_get_frontier_costs_roadmap at 50, fs_roadmap_next_goal
at k = 5 — and the restatement's per-goal A* for the same 50 goals on one core.  Output directory: profiles/roadmap (default).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import planner_ref as P  # noqa: E402
import roadmap_ref as R  # noqa: E402  (the restatement: the CPU legs)

RES = 0.05
TICKS = 10


def med_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def timed(fn, k):
    xs = []
    for i in range(k):
        t0 = time.perf_counter()
        fn(i)
        xs.append(time.perf_counter() - t0)
    return med_ms(xs)


def ref2d():
    fs = importlib.import_module("fit-slam_amd")
    return fs.synth.make_workload("REF2D", n_cand=2000, n_landmarks=20_000)


def robot_cells(cells, seed=11):
    """TICKS robot cells along the free space: a walk of free cells drawn in turn, each near the last one"""
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(cells == 0)
    k = int(rng.integers(xs.size))
    out = [(int(xs[k]), int(ys[k]))]
    for _ in range(TICKS - 1):
        d = np.hypot(xs - out[-1][0], ys - out[-1][1])
        near = np.flatnonzero((d > 40) & (d < 120))
        k = int(rng.choice(near)) if near.size else int(rng.integers(xs.size))
        out.append((int(xs[k]), int(ys[k])))
    return out


def goals_of(w, n, seed):
    rng = np.random.default_rng(seed)
    return w.goals[rng.choice(w.goals.shape[0], n, replace=False)].copy()


def cpu_legs(ticks_file):
    """the restatement's legs on one core, tick by tick, on the node lists the parent grew"""
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    z = np.load(ticks_file)
    w = ref2d()
    cells = w.cells[0]
    ref = R.Roadmap(cells, w.origin, RES)
    rows = []
    for t in range(int(z["n_ticks"])):
        fr, robot = z[f"frontiers{t}"], z[f"robot{t}"]
        if fr.shape[0]:
            ref.populate(fr)
        ref.populate(robot[None], True)
        both = np.concatenate([fr, robot[None]])
        t0 = time.perf_counter(); ref.connect(both); connect = time.perf_counter() - t0
        reb = []
        for _ in range(3):
            t0 = time.perf_counter(); ref.rebuild(); reb.append(time.perf_counter() - t0)
        pose = R.pose7(*robot, 0.7)
        g50 = goals_of(w, 50, t)
        ast = []
        for _ in range(3):
            t0 = time.perf_counter(); ref.plan(pose, g50, leg=R.REFERENCE_ASTAR); ast.append(time.perf_counter() - t0)
        g = ref.graph()
        rows.append(dict(tick=t, nodes=int(g["xy"].shape[0]), edges=int(g["col"].size), rebuild_ms=med_ms(reb),
                         connect_ms=round(connect * 1e3, 4), astar_50_ms=med_ms(ast)))
    print(json.dumps(rows))


def gpu(out_dir, search="tree"):
    fs = importlib.import_module("fit-slam_amd")
    w = ref2d()
    cells = w.cells[0]
    ticks = R.grow_ticks(fs, cells, w.origin, RES, robot_cells(cells))
    tmp = tempfile.mkdtemp(prefix="roadmap_probe_")
    tf = os.path.join(tmp, "ticks.npz")
    arrays = {"n_ticks": np.array(len(ticks))}
    for t, (fr, robot) in enumerate(ticks):
        arrays[f"frontiers{t}"] = fr
        arrays[f"robot{t}"] = robot
    np.savez(tf, **arrays)

    sc = fs.FrontierScorer(device=0)
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    sc.set_roadmap_search(search)
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])
    rows = []
    for t, (fr, robot) in enumerate(ticks):
        if fr.shape[0]:
            sc.roadmap_add_nodes(fr)
        sc.roadmap_add_nodes(robot[None], is_robot_pose=True)
        both = np.concatenate([fr, robot[None]])
        sc.get_counter(1007, reset=True)
        t0 = time.perf_counter(); sc.roadmap_connect(both); connect = time.perf_counter() - t0
        connect_walks = sc.get_counter(1007, reset=True)
        connect_again = timed(lambda i: sc.roadmap_connect(both), 7)          # (idempotent: the same walks, no new edge)
        rebuild = timed(lambda i: sc.roadmap_rebuild(), 7)
        rebuild_walks = sc.get_counter(1007, reset=True) // 7
        g = sc.roadmap_graph()
        xy = g["xy"]
        poses = [R.pose7(*robot, 0.7), R.pose7(*xy[len(xy) // 2], 0.7)]       # two start nodes: every call builds a tree
        row = dict(tick=t, nodes=int(xy.shape[0]), edges=int(g["col"].size), frontiers=int(fr.shape[0]),
                   connect_first_ms=round(connect * 1e3, 4), connect_ms=connect_again, connect_walks=int(connect_walks),
                   rebuild_ms=rebuild, rebuild_walks=int(rebuild_walks))
        for n in (50, 2000):
            gl = goals_of(w, n, t)
            row[f"plan_{n}_fresh_tree_ms"] = timed(lambda i: sc.roadmap_plan(poses[i & 1], gl), 8)
            row[f"plan_{n}_cached_tree_ms"] = timed(lambda i: sc.roadmap_plan(poses[0], gl), 8)
        row["tree_rounds"] = sc.get_counter(1006)
        g50 = goals_of(w, 50, t)
        row["fused_50_ms"] = timed(lambda i: sc.get_frontier_costs_roadmap(poses[i & 1], g50), 8)

        def two_calls(i):
            p = sc.roadmap_plan(poses[i & 1], g50)
            sc.get_frontier_costs(g50, p["path_length"], p["path_heading"], achievable_in=p["achievable"])
        row["plan_then_costs_50_ms"] = timed(two_calls, 8)
        rows.append(row)
    # the host leg of the one-call comparison on the final roadmap: the restatement's per-goal A* (this process, not pinned) +
    # fs_get_frontier_costs
    ref = R.Roadmap(cells, w.origin, RES)
    for fr, robot in ticks:
        if fr.shape[0]:
            ref.populate(fr)
        ref.populate(robot[None], True)
        ref.connect(np.concatenate([fr, robot[None]]))
    ref.rebuild()
    pose = R.pose7(*ticks[-1][1], 0.7)
    g50 = goals_of(w, 50, 99)

    def host_plan(i):
        p = ref.plan(pose, g50, leg=R.REFERENCE_ASTAR)
        sc.get_frontier_costs(g50, p["path_length"], p["path_heading"], achievable_in=p["achievable"])
    host_then_costs = timed(host_plan, 5)
    sc.close()
    cpu = subprocess.run([sys.executable, os.path.abspath(__file__), "cpu-legs", "--ticks", tf], check=True, capture_output=True, text=True)
    cpu_rows = json.loads(cpu.stdout.strip().splitlines()[-1])
    for r, c in zip(rows, cpu_rows):
        assert (r["nodes"], r["edges"]) == (c["nodes"], c["edges"]), (r, c)
    crossover = next((r["nodes"] for r, c in zip(rows, cpu_rows) if r["rebuild_ms"] < c["rebuild_ms"]), None)
    res = dict(what="REF2D (512^2, 0.05 m), roadmap grown over %d simulated ticks (fs_frontier_clusters goal points + robot pose, "
                    "connected each tick); host wall ms, medians" % len(ticks),
               search=search, ticks=rows, host_astar_then_costs_50_final_ms=host_then_costs,
               rebuild_faster_than_one_core_from_nodes=crossover)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "gpu_ref2d.json" if search == "tree" else f"gpu_ref2d_{search}.json"), "w"), indent=1)
    json.dump(dict(what="the restatement's legs on one core, same node lists, host wall ms (rebuild / A*: medians of 3)", ticks=cpu_rows),
              open(os.path.join(out_dir, "cpu_ref2d.json"), "w"), indent=1)
    print(json.dumps(res))


def deviation(out_dir):
    """tree vs per-goal A* on the maps of tests/test_gpu_roadmap.py (random nodes on free / unknown cells, rebuilt roadmap)"""
    fs = importlib.import_module("fit-slam_amd")
    maps = [("REF2D", fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])]
    rng = np.random.Generator(np.random.PCG64(5151))
    for k, n in enumerate([64, 96, 128, 160, 200, 256, 300, 384, 512, 640, 768, 1024]):
        maps.append((f"plan{k}_{n}", fs.synth.make_grid(rng, n, 1)[0]))
    maps.append(("non_square", fs.synth.make_grid(rng, 256, 1)[0][:170, :]))
    maps.append(("spiral", P.spiral_map(512)[0]))
    goals_total = agree = both = differ = tree_longer = 0
    rel = []
    per_map = []
    for name, cells in maps:
        origin = (-cells.shape[1] * RES / 2, -cells.shape[0] * RES / 2, 0.0)
        r = np.random.default_rng(len(name) * 7919 + cells.size)
        k = int(min(1500, max(40, cells.size * RES * RES / 2)))
        ys, xs = np.nonzero(cells < 253)
        idx = r.choice(xs.size, k, replace=False)
        pts = np.stack([origin[0] + (xs[idx] + r.uniform(0, 1, k)) * RES, origin[1] + (ys[idx] + r.uniform(0, 1, k)) * RES], axis=1)
        ref = R.Roadmap(cells, origin, RES)
        ref.populate(pts)
        ref.rebuild()
        gi = r.choice(xs.size, 200, replace=False)
        goals = np.zeros((200, 3))
        goals[:, 0] = origin[0] + (xs[gi] + r.uniform(0, 1, 200)) * RES
        goals[:, 1] = origin[1] + (ys[gi] + r.uniform(0, 1, 200)) * RES
        pose = R.pose7(*pts[0], 0.3)
        t = ref.plan(pose, goals, leg=R.TREE)
        a = ref.plan(pose, goals, leg=R.REFERENCE_ASTAR)
        ok = (t["achievable"] == 1) & (a["achievable"] == 1)
        d = t["path_length_m"][ok] - a["path_length_m"][ok]
        m_rel = np.abs(d) / np.maximum(a["path_length_m"][ok], 1e-9)
        goals_total += 200
        agree += int((t["achievable"] == a["achievable"]).sum())
        both += int(ok.sum())
        differ += int((d != 0).sum())
        tree_longer += int((d > 0).sum())
        rel.extend(m_rel[d != 0].tolist())
        per_map.append(dict(map=name, nodes=int(ref.graph()["xy"].shape[0]), achievable=int(ok.sum()), differ=int((d != 0).sum())))
        ref.close()
    rel = np.array(rel) if rel else np.zeros(1)
    res = dict(what="tree (fs_roadmap_plan) vs the reference's per-goal squared-heuristic A*, 200 goals per map, %d maps" % len(maps),
               goals=goals_total, achievability_agrees=agree, achievable_both=both,
               path_length_m_differs=differ, share_differs=round(differ / max(both, 1), 4),
               tree_longer_in_metres=tree_longer,
               rel_diff_where_different=dict(median=round(float(np.median(rel)), 4), p99=round(float(np.percentile(rel, 99)), 4),
                                             max=round(float(rel.max()), 4)),
               per_map=per_map)
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "astar_vs_tree.json"), "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_map"}))


def astar_cpu(ticks_file):
    """child process pinned to one core: the restatement's per-goal A* and its tree leg for the 50 goals of `astar`"""
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    d = np.load(ticks_file)
    cells, origin = d["cells"], tuple(float(v) for v in d["origin"])
    ref = R.Roadmap(cells, origin, RES)
    ref.populate(d["pts"])
    ref.rebuild()
    pose, g50 = d["pose"], d["g50"]
    out = {}
    for leg, key in ((R.REFERENCE_ASTAR, "host_astar_50_ms"), (R.TREE, "host_tree_50_ms")):
        xs = []
        for _ in range(7):
            t0 = time.perf_counter(); ref.plan(pose, g50, leg=leg); xs.append(time.perf_counter() - t0)
        out[key] = med_ms(xs)
    print(json.dumps(out))


def astar(out_dir):
    """the two roadmap searches side by side on REF2D's roadmap of the tests"""
    fs = importlib.import_module("fit-slam_amd")
    w = ref2d()
    cells, origin = np.ascontiguousarray(w.cells[0]), tuple(float(v) for v in w.origin)
    rng = np.random.default_rng(2024)
    k_nodes = int(min(1500, max(40, cells.size * RES * RES / 2)))
    xs, ys = P.free_cells(cells, rng, k_nodes)
    pts = np.stack([origin[0] + (xs + rng.uniform(0, 1, k_nodes)) * RES, origin[1] + (ys + rng.uniform(0, 1, k_nodes)) * RES], axis=1)
    sc = fs.FrontierScorer(device=0)
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])
    sc.roadmap_add_nodes(pts)
    sc.roadmap_rebuild()
    g = sc.roadmap_graph()
    poses = [R.pose7(*pts[0], 0.7), R.pose7(*pts[len(pts) // 2], 0.7)]
    g50, g2000 = goals_of(w, 50, 0), goals_of(w, 2000, 0)
    rg = np.random.default_rng(5)
    fx, fy = P.free_cells(cells, rg, 10)
    ng = np.zeros((10, 3))
    ng[:, 0] = origin[0] + (fx + 0.5) * RES
    ng[:, 1] = origin[1] + (fy + 0.5) * RES
    nplm = np.concatenate([np.sort(rg.uniform(0.5, 12.0, 6)), rg.uniform(12.5, 50.0, 4)])
    nach = np.ones(10, np.uint8)
    res = dict(what="REF2D (512^2, 0.05 m), %d nodes / %d edges (nodes on free cells, rebuilt); host wall ms, medians of 15 after "
                    "one warm-up call; every plan call alternates two start nodes (the tree: a fresh tree per call)"
                    % (g["xy"].shape[0], g["col"].size),
               nodes=int(g["xy"].shape[0]), edges=int(g["col"].size), searches={})
    for search in ("tree", "reference"):
        sc.set_roadmap_search(search)
        row = {}
        for n, gl in ((50, g50), (2000, g2000)):
            sc.roadmap_plan(poses[1], gl)
            row[f"plan_{n}_ms"] = timed(lambda i: sc.roadmap_plan(poses[i & 1], gl), 15)
            if search == "reference":
                sc.get_counter(1021, reset=True)
                sc.roadmap_plan(poses[0], gl)
                row[f"plan_{n}_queries"] = sc.get_counter(1021, reset=True)
                row[f"plan_{n}_largest_query_pops"] = sc.get_counter(1022)
                row[f"plan_{n}_global_route_queries"] = sc.get_counter(1023, reset=True)
        sc.get_frontier_costs_roadmap(poses[1], g50)
        row["fused_50_ms"] = timed(lambda i: sc.get_frontier_costs_roadmap(poses[i & 1], g50), 15)
        sc.roadmap_next_goal(poses[0], ng, nplm, nach, n_local=5)
        row["next_goal_k5_ms"] = timed(lambda i: sc.roadmap_next_goal(poses[i & 1], ng, nplm, nach, n_local=5), 15)
        res["searches"][search] = row
    sc.set_roadmap_search("tree")
    sc.close()
    tf = os.path.join(tempfile.mkdtemp(prefix="roadmap_probe_"), "astar.npz")
    np.savez(tf, cells=cells, origin=np.array(origin), pts=pts, pose=poses[0], g50=g50)
    cpu = subprocess.run([sys.executable, os.path.abspath(__file__), "astar-cpu", "--ticks", tf], check=True, capture_output=True, text=True)
    res["one_core"] = json.loads(cpu.stdout.strip().splitlines()[-1])
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "astar_gpu_ref2d.json"), "w"), indent=1)
    print(json.dumps(res))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["deviation", "gpu", "astar", "cpu-legs", "astar-cpu"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roadmap"))
    ap.add_argument("--ticks")
    ap.add_argument("--search", choices=["tree", "reference"], default="tree")
    a = ap.parse_args()
    if a.mode == "deviation":
        deviation(a.out)
    elif a.mode == "gpu":
        gpu(a.out, a.search)
    elif a.mode == "astar":
        astar(a.out)
    elif a.mode == "astar-cpu":
        astar_cpu(a.ticks)
    else:
        cpu_legs(a.ticks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
