"""The batched grid planner off the GPU: its entry points are declared and exported, and the CPU restatement
(tests/navfn_ref/navfn_ref.cpp) the GPU tests hold it to gives known answers, a true fixed point with NavFn's reachability, and
the per-frontier planner's achievability wherever neither planner ran into a limit."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import planner_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fs_plan_paths", "fs_navfn_potential", "fs_get_frontier_costs_planned")
RES = 0.05


def test_planner_entry_points_declared_and_exported():
    fs = importlib.import_module("fit-slam_amd")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))
    lib = fs._build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT\s+(fs_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert name in declared and name in exported and name in fs.capi.EXPORTED_SYMBOLS, name


def _update(P, cost):
    """min(P, T(P)) for every cell, in numpy (float32 like NavFn; the quadratic in float64)"""
    l, r = np.roll(P, 1, axis=1), np.roll(P, -1, axis=1)
    u, d = np.roll(P, 1, axis=0), np.roll(P, -1, axis=0)
    tc = np.where(l < r, l, r)
    ta = np.where(u < d, u, d)
    hf = cost.astype(np.float32)
    dc = tc - ta
    neg = dc < 0
    dc = np.where(neg, -dc, dc)
    ta = np.where(neg, tc, ta)
    with np.errstate(all="ignore"):
        q = (dc / hf).astype(np.float32)
        q64 = q.astype(np.float64)
        v = (-0.2301 * q64 * q64 + 0.5307 * q64 + 0.7040).astype(np.float32)
        pot = np.where(dc >= hf, ta + hf, ta + hf * v).astype(np.float32)
    free = cost < 254
    return np.where(free & (pot < P), pot, P)


def _bfs(cost, rx, ry):
    ny, nx = cost.shape
    seen = np.zeros_like(cost, dtype=bool)
    seen[ry, rx] = True
    front = [(rx, ry)]
    while front:
        nxt = []
        for x, y in front:
            for a, b in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if 0 <= a < nx and 0 <= b < ny and not seen[b, a] and cost[b, a] < 254:
                    seen[b, a] = True
                    nxt.append((a, b))
        front = nxt
    return seen


def test_open_map_straight_line():
    cells = np.zeros((64, 64), dtype=np.uint8)
    origin = (-1.6, -1.6, 0.0)
    pot, st = R.converged_field(cells, 10, 32)
    assert pot[32, 10] == 0.0 and st["rounds"] >= 2
    assert pot[32, 11] == 50.0                          # one neighbour away: ta + hf
    pose = R.robot_pose(origin, RES, 10, 32, 0.0)
    gx, gy = R.cell_centre(origin, RES, 50, 32)
    out = R.plan(cells, origin, RES, pose, [[gx, gy, 0.0]])
    assert out["achievable"][0] == 1
    # gradient steps of half a cell from x = 50 while the nearest cell is not the robot's (x = 10.5 rounds onto it): 50, 49.5, ...,
    # 11, then the robot cell itself
    assert out["path_length"][0] == (50 - 11) * 2 + 1 + 1
    # the segment (0, 1) is skipped: from cell 49 (49.5 truncated) to the robot's cell 10, straight along x
    assert out["path_length_m"][0] == pytest.approx((49 - 10) * RES, abs=1e-12)
    assert out["path_heading"][0] == 0.0
    # the per-frontier A* stops its wave at the goal: next to the cells it never reached calcPath follows the grid (whole-cell
    # steps), so fewer points, the same straight line
    ast = R.plan(cells, origin, RES, pose, [[gx, gy, 0.0]], leg=R.REFERENCE_ASTAR)
    assert ast["achievable"][0] == 1 and 41 <= ast["path_length"][0] <= 80
    assert ast["path_length_m"][0] == pytest.approx((49 - 10) * RES, abs=1e-12)


def test_corridor_follows_the_grid():
    """In a corridor one cell wide every neighbour across is an obstacle (POT_HIGH): calcPath follows the grid, one cell a step."""
    cells = np.full((16, 64), 254, dtype=np.uint8)
    cells[8, 1:63] = 0
    origin = (0.0, 0.0, 0.0)
    pose = R.robot_pose(origin, RES, 10, 8)
    goal = [list(R.cell_centre(origin, RES, 50, 8)) + [0.0]]
    pot, _ = R.converged_field(cells, 10, 8)
    assert (pot[8, 10:51] == 50.0 * np.arange(41, dtype=np.float32)).all()
    for leg in (R.CONVERGED, R.REFERENCE_ASTAR):
        out = R.plan(cells, origin, RES, pose, goal, leg=leg)
        assert out["path_length"][0] == 41                # cells 50 .. 11, then the robot's
        assert out["path_length_m"][0] == pytest.approx(39 * RES, abs=1e-12)


def test_closed_wall_is_unachievable_in_both_legs():
    cells = np.zeros((64, 80), dtype=np.uint8)
    cells[:, 40:42] = 254
    origin = (0.0, 0.0, 0.0)
    pose = R.robot_pose(origin, RES, 10, 30)
    goal = [list(R.cell_centre(origin, RES, 60, 30)) + [0.0]]
    pot, _ = R.converged_field(cells, 10, 30)
    assert (pot[:, 42:] == R.POT_HIGH).all()
    for leg in (R.CONVERGED, R.REFERENCE_ASTAR):
        out = R.plan(cells, origin, RES, pose, goal, leg=leg)
        assert out["achievable"][0] == 0 and out["path_length"][0] == R.DBL_MAX and out["path_length_m"][0] == R.DBL_MAX
        assert out["path_heading"][0] == R.DBL_MAX


def test_unknown_goal_needs_allow_unknown():
    cells = np.zeros((48, 48), dtype=np.uint8)
    cells[:, 30:] = 255
    origin = (0.0, 0.0, 0.0)
    pose = R.robot_pose(origin, RES, 8, 24)
    goal = [list(R.cell_centre(origin, RES, 36, 24)) + [0.0]]
    for leg in (R.CONVERGED, R.REFERENCE_ASTAR):
        assert R.plan(cells, origin, RES, pose, goal, allow_unknown=False, leg=leg)["achievable"][0] == 0
        out = R.plan(cells, origin, RES, pose, goal, allow_unknown=True, leg=leg)
        assert out["achievable"][0] == 1 and out["path_length"][0] > 20


def test_off_map_and_not_achievable_in():
    cells = np.zeros((32, 32), dtype=np.uint8)
    origin = (1.0, 2.0, 0.0)
    inside = list(R.cell_centre(origin, RES, 20, 20)) + [0.0]
    goals = np.array([inside, [origin[0] - 0.01, 2.5, 0.0], [1.5, origin[1] + 32 * RES, 0.0], inside])
    for leg in (R.CONVERGED, R.REFERENCE_ASTAR):
        out = R.plan(cells, origin, RES, R.robot_pose(origin, RES, 5, 5), goals, achievable_in=[1, 1, 1, 0], leg=leg)
        assert out["achievable"].tolist() == [1, 0, 0, 0]
        assert (out["path_length"][1:] == R.DBL_MAX).all() and (out["path_length_m"][1:] == R.DBL_MAX).all()
        off = np.array([origin[0] - 1.0, 2.5, 0, 0, 0, 0, 1.0])
        out = R.plan(cells, origin, RES, off, goals, leg=leg)
        assert not out["achievable"].any() and (out["path_length"] == R.DBL_MAX).all() and (out["path_heading"] == R.DBL_MAX).all()


def _floor_plans(k):
    fs = importlib.import_module("fit-slam_amd")
    out = []
    for seed in range(k):
        if seed % 2:
            w = fs.synth.make_small_2d(seed)
            out.append((w.cells[0], w.origin, w.goals))
        else:
            rng = np.random.Generator(np.random.PCG64(seed))
            cells = fs.synth.make_grid(rng, 128, 1)[0]
            origin = (-3.2, -3.2, 0.0)
            gx, gy = R.free_cells(cells, rng, 60)
            out.append((cells, origin, np.stack([origin[0] + (gx + 0.5) * RES, origin[1] + (gy + 0.5) * RES, np.zeros(gx.size)], axis=1)))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_converged_field_is_a_fixed_point_with_navfn_reachability(seed):
    cells, origin, _ = _floor_plans(6)[seed]
    rng = np.random.default_rng(seed)
    for allow in (False, True):
        rx, ry = R.free_cells(cells, rng, 1)
        pot, _ = R.converged_field(cells, rx[0], ry[0], allow_unknown=allow)
        cost = R.costs(cells, allow_unknown=allow)
        assert (_update(pot, cost) == pot).all()
        assert ((pot < R.POT_HIGH) == _bfs(cost, rx[0], ry[0])).all()
    spiral, centre, end = R.spiral_map(256)
    pot, st = R.converged_field(spiral, *centre)
    assert (_update(pot, R.costs(spiral)) == pot).all() and pot[end[1], end[0]] < R.POT_HIGH and st["rounds"] > 50


def test_legs_agree_on_achievability_without_limits():
    """On 24 maps (floor plans of synth.make_grid and make_small_2d), both allow_unknown: the converged leg and the per-frontier
    A* agree on `achievable` wherever neither ran into a limit — the wave's cycle budget or buffer cap (A*), or calcPath's
    own cycle budget (either leg: a descent that stalls on one field may not stall on the other).  Path lengths are not gated
    against each other; their distribution is profiles/planner/astar_vs_converged.json (tools/planner_probe.py)."""
    agree = total = 0
    for seed, (cells, origin, goals) in enumerate(_floor_plans(24)):
        rng = np.random.default_rng(seed)
        rx, ry = R.free_cells(cells, rng, 1)
        pose = R.robot_pose(origin, RES, rx[0], ry[0], 0.3)
        for allow in (False, True):
            a = R.plan(cells, origin, RES, pose, goals, allow_unknown=allow)
            b = R.plan(cells, origin, RES, pose, goals, allow_unknown=allow, leg=R.REFERENCE_ASTAR)
            clean = ((b["limit"] & 3) == 0) & ((a["limit"] >> 8) != 4) & ((b["limit"] >> 8) != 4)
            assert (a["achievable"][clean] == b["achievable"][clean]).all(), (seed, allow, np.nonzero(clean & (a["achievable"] != b["achievable"]))[0])
            agree += int(clean.sum())
            total += goals.shape[0]
            both = clean & (a["achievable"] == 1)
            assert (a["path_heading"][both] == b["path_heading"][both]).all()
    assert agree >= 0.95 * total
