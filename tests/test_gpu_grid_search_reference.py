"""The REFERENCE grid search on the GPU (fs_set_grid_search): the wave of fs_navfn_wave_potential and the columns of
fs_plan_paths against the reference's own compiled planner (reference_built.navfn_plan) bit for bit, the slot batching and the
lowered buffer cap against the header's CPU driver (tests/navfn_wave_ref), the one-call forms against their parts, the untouched
default, and the refusals.  Reads only oracle/_ref/, never the reference tree."""
import importlib
import struct
import zlib

import numpy as np
import pytest

import navfn_wave_ref as W
import pathinfo_ref
import planner_ref as P
import reference_built as B
from test_navfn_wave_restatement import spiral_ends

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = B.RES
MAPS = [m for m in B.planner_maps() if m[0] in ("plan_64", "plan_100", "plan_130", "plan_192x150", "spiral_128")]
IDS = [m[0] for m in MAPS]
COLS = ("path_length", "path_length_m", "path_heading", "achievable")
_REACHED = {B.PLAN_OK: 1, B.PLAN_NO_PATH: 1, B.PLAN_NO_WAVE: 0}
_robots = {}


def _bits(x):
    return struct.pack("<d", x)


def _robot(k):
    if k not in _robots:
        name, cells, origin = MAPS[k]
        _robots[k] = P.well_placed_robot(cells, np.random.default_rng(zlib.crc32(name.encode())))
    return _robots[k]


def _scorer(cells, origin, search=None):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    if search:
        sc.set_grid_search(search)
    return sc


def _goals(k, seed_add=3):
    """40 goals (8 unknown or wall cells, 2 walls, 2 off the map, 20 reachable), two of them in one cell at different points, and
    an achievable_in with two zeros"""
    name, cells, origin = MAPS[k]
    goals = B.planner_goals(cells, origin, zlib.crc32(name.encode()) + seed_add, _robot(k), off_map=2)
    gx, gy = B.cell_of(origin, goals[30])
    goals[31, 0], goals[31, 1] = origin[0] + (gx + 0.9) * RES, origin[1] + (gy + 0.1) * RES
    goals[30, 0], goals[30, 1] = origin[0] + (gx + 0.2) * RES, origin[1] + (gy + 0.7) * RES
    ach = np.ones(40, dtype=np.uint8)
    ach[[3, 25]] = 0
    return goals, ach


def _on_map(cells, origin, g):
    ny, nx = cells.shape
    return origin[0] <= g[0] < origin[0] + nx * RES and origin[1] <= g[1] < origin[1] + ny * RES


def _distinct_cells(cells, origin, goals, ach):
    return len({B.cell_of(origin, g) for g, a in zip(goals, ach) if a and _on_map(cells, origin, g)})


# ------------------------------------------------------------------ 1. the wave
@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
def test_wave_equals_the_reference_potarr(k):
    """7 goals from a well-placed robot (an unknown cell, a wall cell, the robot's own cell, four reachable ones) and one from a
    robot on the border ring, both allow_unknown; on spiral_128 also the wave the cycle budget ends"""
    B.require()
    name, cells, origin = MAPS[k]
    ny, nx = cells.shape
    rx, ry = _robot(k)
    goals = B.planner_goals(cells, origin, zlib.crc32(name.encode()) + 1, (rx, ry))
    own = np.array([*P.cell_centre(origin, RES, rx, ry), 0.0])
    picked = [goals[0], goals[8], own, goals[22], goals[27], goals[33], goals[39]]
    cases = [((rx, ry), g) for g in picked] + [((0, ny // 2), goals[39])]
    if name == "spiral_128":
        far, near = spiral_ends(cells)
        cases.append((far, np.array([*P.cell_centre(origin, RES, *near), 0.0])))
    sc = _scorer(cells, origin)
    try:
        limits = 0
        for allow in (False, True):
            for i, (robot, g) in enumerate(cases):
                pose = P.robot_pose(origin, RES, robot[0], robot[1], 0.3)
                want = B.navfn_plan(cells, origin, RES, pose[:2], g[:2], allow_unknown=allow, want_field=True)
                cpu = W.wave_of_cells(cells, robot, B.cell_of(origin, g), allow_unknown=allow)
                field, limit = sc.navfn_wave_potential(pose, g, allow_unknown=allow)
                gx, gy = B.cell_of(origin, g)
                what = (name, allow, i, want["status"], limit)
                print(what, "reached", int((field < B.POT_HIGH).sum()), "cells; replays", sc.get_counter(1041))
                assert field.tobytes() == want["potarr"].tobytes(), what
                assert int(field[gy, gx] < B.POT_HIGH) == _REACHED[want["status"]], what
                assert limit == cpu["limit"], what
                limits |= limit if i == 8 else 0
                assert sc.get_counter(1037) == 1 and sc.get_counter(1038) == 1
                assert sc.get_counter(1039) == (limit & 1) and sc.get_counter(1040) == (limit >> 1)
        if name == "spiral_128":
            assert limits == W.LIMIT_CYCLES               # (the wave along the whole corridor ends on the cycle budget)
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. the columns
@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
def test_columns_equal_the_reference_planner(k):
    B.require()
    name, cells, origin = MAPS[k]
    rx, ry = _robot(k)
    pose = P.robot_pose(origin, RES, rx, ry, -2.0)
    goals, ach = _goals(k)
    sc = _scorer(cells, origin)
    try:
        for allow in (False, True):
            got = sc.plan_paths(pose, goals, achievable_in=ach, allow_unknown=allow, search="reference")
            assert sc.get_counter(1037) == _distinct_cells(cells, origin, goals, ach) < 38
            one = sc.plan_paths(pose, goals[-1:], allow_unknown=allow, search="reference")
            assert sc.get_counter(1037) == 1
            rest = P.plan(cells, origin, RES, pose, goals, achievable_in=ach, allow_unknown=allow, leg=P.REFERENCE_ASTAR)
            found = 0
            for i, g in enumerate(goals):
                what = (name, allow, i)
                if not ach[i] or not _on_map(cells, origin, g):
                    assert got["achievable"][i] == 0 and got["path_length"][i] == P.DBL_MAX, what
                    continue
                want = B.navfn_plan(cells, origin, RES, pose[:2], g[:2], allow_unknown=allow)
                assert got["achievable"][i] == want["achievable"], what + (want["status"],)
                if want["achievable"]:
                    found += 1
                    assert got["path_length"][i] == float(want["len"]), what
                    assert _bits(got["path_length_m"][i]) == _bits(want["path_length_m"]), what
            for col in COLS:                           # the heading and every DBL_MAX convention
                assert got[col].tobytes() == rest[col].tobytes(), (name, allow, col)
                assert one[col].tobytes() == rest[col][-1:].tobytes(), (name, allow, col)
            assert got["achievable"][30] == got["achievable"][31] == 1 and got["path_heading"][30] != got["path_heading"][31]
            print(name, allow, "achievable", found, "of 40")
            assert found >= 10, (name, allow, found)
    finally:
        sc.close()


# ------------------------------------------------------------------ 3. batching and the cap
def test_results_do_not_depend_on_the_slot_count():
    k = IDS.index("plan_130")
    name, cells, origin = MAPS[k]
    pose = P.robot_pose(origin, RES, *_robot(k), 0.9)
    goals, ach = _goals(k)
    distinct = _distinct_cells(cells, origin, goals, ach)
    sc = _scorer(cells, origin, "reference")
    try:
        want = sc.plan_paths(pose, goals, achievable_in=ach, allow_unknown=True)
        assert sc.get_counter(1038) == 1
        for slots in (1, 3, 64):
            sc.set_option("navfn.wave_slots", slots)
            got = sc.plan_paths(pose, goals, achievable_in=ach, allow_unknown=True)
            assert sc.get_counter(1038) == -(-distinct // slots), slots
            assert sc.get_counter(1037) == distinct
            for col in COLS:
                assert got[col].tobytes() == want[col].tobytes(), (slots, col)
        assert want["achievable"].sum() >= 10
    finally:
        sc.close()


@pytest.mark.parametrize("cap", [64, 1000])
def test_lowered_cap_equals_the_cpu_driver(cap):
    """the reference's cap of 10 000 drops nothing on maps of this size; the cap's code is exercised at 64 and 1 000 entries"""
    k = IDS.index("plan_130")
    name, cells, origin = MAPS[k]
    rx, ry = _robot(k)
    pose = P.robot_pose(origin, RES, rx, ry, 0.0)
    goals = B.planner_goals(cells, origin, zlib.crc32(name.encode()) + 1, (rx, ry))
    cost = P.costs(cells, True)
    ys, xs = np.nonzero(cost < 254)
    far = int(np.argmax((xs - rx) ** 2 + (ys - ry) ** 2))
    picked = [np.array([*P.cell_centre(origin, RES, int(xs[far]), int(ys[far])), 0.0]), goals[0], goals[25], goals[39]]
    sc = _scorer(cells, origin)
    try:
        sc.set_option("navfn.wave_cap", cap)
        dropped = 0
        for i, g in enumerate(picked):
            cpu = W.wave(cost, (rx, ry), B.cell_of(origin, g), width=64, cap=cap)
            field, limit = sc.navfn_wave_potential(pose, g, allow_unknown=True)
            print(name, cap, i, "limit", limit, cpu["limit"])
            assert field.tobytes() == cpu["potarr"].tobytes(), (cap, i)
            assert limit == cpu["limit"], (cap, i)
            assert sc.get_counter(1040) == (limit >> 1)
            dropped += limit >> 1
        if cap == 64:
            assert dropped > 0
    finally:
        sc.close()


# ------------------------------------------------------------------ 4. the one-call forms
def _setup_scoring(sc, cells, origin):
    w = fsmod.synth.make_small_2d(31, n=64, n_cand=8)
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(cells[None], origin, RES)
    sc.set_option("fim.learn", 0)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    sc.set_fim_params(14.0, 1.0)
    sc.set_arrival_limits(4000.0, sc.max_arrival()["min_gt"])


def test_one_call_forms_under_reference():
    k = IDS.index("plan_64")
    name, cells, origin = MAPS[k]
    rx, ry = _robot(k)
    pose = P.robot_pose(origin, RES, rx, ry, 1.0)
    goals, _ = _goals(k)
    sc = fsmod.FrontierScorer(device=0)
    try:
        _setup_scoring(sc, cells, origin)
        conv = sc.plan_paths(pose, goals)
        sc.set_grid_search("reference")
        plan = sc.plan_paths(pose, goals)
        assert plan["achievable"].sum() >= 10
        # planned = plan, then score and rank
        want = sc.get_frontier_costs(goals, plan["path_length"], plan["path_heading"], achievable_in=plan["achievable"])
        got = sc.get_frontier_costs_planned(pose, goals)
        for col in ("weighted_cost", "arrival_utility", "distance_utility", "order", "records"):
            assert got[col].tobytes() == want[col].tobytes(), col
        assert got["path_length_m"].tobytes() == plan["path_length_m"].tobytes()
        # path information: the same four columns, the way-point counts follow from them
        info = sc.plan_paths_information(pose, goals)
        for col in COLS:
            assert info[col].tobytes() == plan[col].tobytes(), col
        assert info["n_waypoints"].tobytes() == pathinfo_ref.closed_form_counts(plan["path_length"], RES).tobytes()
        # searched = search, plan, score, rank by hand
        fr, _ = sc.search_frontiers(pose[:2], want_every=False)
        assert fr.shape[0] >= 1
        fgoal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
        fplan = sc.plan_paths(pose, fgoal)
        fwant = sc.get_frontier_costs(fgoal, fplan["path_length"], fplan["path_heading"], frontier_size=fr["size"], achievable_in=fplan["achievable"])
        got_fr, fgot = sc.get_frontier_costs_searched(pose)
        assert got_fr.tobytes() == fr.tobytes()
        for col in ("weighted_cost", "arrival_utility", "distance_utility", "order", "records"):
            assert fgot[col].tobytes() == fwant[col].tobytes(), col
        assert fgot["path_length_m"].tobytes() == fplan["path_length_m"].tobytes()
        assert sc.get_counter(1037) == len({B.cell_of(origin, g) for g in fgoal})
        # the per-call keyword leaves the context's setting alone, and the two searches do differ on this list
        again = sc.plan_paths(pose, goals, search="converged")
        for col in COLS:
            assert again[col].tobytes() == conv[col].tobytes(), col
        assert sc.plan_paths(pose, goals)["path_length_m"].tobytes() == plan["path_length_m"].tobytes()
        assert conv["path_length_m"].tobytes() != plan["path_length_m"].tobytes()
    finally:
        sc.close()


# ------------------------------------------------------------------ 5. the default is untouched
def test_default_is_untouched():
    k = IDS.index("plan_100")
    name, cells, origin = MAPS[k]
    pose = P.robot_pose(origin, RES, *_robot(k), 0.2)
    goals, ach = _goals(k)
    held = fsmod.FrontierScorer(device=0)
    try:
        before = held.get_counter(1036)
        fresh = _scorer(cells, origin)
        try:
            want = fresh.plan_paths(pose, goals, achievable_in=ach)
            assert fresh.get_counter(1002) == 1
            for counter in range(1037, 1042):
                assert fresh.get_counter(counter) == 0, counter
        finally:
            fresh.close()
        assert held.get_counter(1036) == before
        sc = _scorer(cells, origin)
        try:
            sc.set_grid_search("reference")
            sc.plan_paths(pose, goals, achievable_in=ach)
            assert sc.get_counter(1002) == 0                  # no converged field was built
            assert sc._L.fs_set_grid_search(sc._h, 2) == fsmod.capi.FS_E_INVALID
            assert sc._L.fs_set_grid_search(sc._h, -1) == fsmod.capi.FS_E_INVALID
            sc.plan_paths(pose, goals, achievable_in=ach)
            assert sc.get_counter(1002) == 0                  # (a refused value left the setting at REFERENCE)
            sc.set_grid_search("converged")
            got = sc.plan_paths(pose, goals, achievable_in=ach)
            assert sc.get_counter(1002) == 1
            sc.plan_paths(pose, goals, achievable_in=ach)
            assert sc.get_counter(1002) == 1                  # the cache serves the second call as before
            for col in COLS:
                assert got[col].tobytes() == want[col].tobytes(), col
            for key, bad in (("navfn.wave_slots", -1), ("navfn.wave_bytes", 0), ("navfn.wave_cap", 15), ("navfn.wave_cap", 10001)):
                with pytest.raises(fsmod.FsError):
                    sc.set_option(key, bad)
            for key, good in (("navfn.wave_slots", 0), ("navfn.wave_bytes", 1 << 30), ("navfn.wave_cap", 10000)):
                sc.set_option(key, good)
        finally:
            sc.close()
        assert held.get_counter(1036) == before               # a destroyed context returned the slots too
    finally:
        held.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    INVALID = fsmod.capi.FS_E_INVALID
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.set_grid_search("reference")
        sc.upload_grid(np.zeros((2, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        pose = P.robot_pose((0, 0, 0), RES, 3, 3)
        with pytest.raises(fsmod.FsError) as e:
            sc.plan_paths(pose, np.zeros((1, 3)) + 0.3)
        assert e.value.code == INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.navfn_wave_potential(pose, np.zeros(3) + 0.3)
        assert e.value.code == INVALID
        # a side above 4096 cells
        sc.upload_grid(np.zeros((1, 8, 4100), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError, match="4096") as e:
            sc.plan_paths(pose, np.zeros((1, 3)) + 0.3)
        assert e.value.code == INVALID
        with pytest.raises(fsmod.FsError, match="4096") as e:
            sc.navfn_wave_potential(pose, np.zeros(3) + 0.3)
        assert e.value.code == INVALID
        assert sc.plan_paths(pose, np.zeros((1, 3)) + 0.3, search="converged")["achievable"][0] == 1     # (the default takes it)
        # robot off the map: nothing is achievable, as fs_plan_paths has it; the wave call refuses, and a goal off the map too
        name, cells, origin = MAPS[0]
        sc.upload_grid(cells[None], origin, RES)
        goals, _ = _goals(0)
        off = np.array([origin[0] - 0.5, origin[1] + 1.0, 0, 0, 0, 0, 1.0])
        got = sc.plan_paths(off, goals)
        assert not got["achievable"].any()
        for col in COLS[:3]:
            assert (got[col] == P.DBL_MAX).all()
        assert sc.get_counter(1037) == 0 and sc.get_counter(1038) == 0
        on = P.robot_pose(origin, RES, *_robot(0))
        for pose_, goal_ in ((off, goals[20]), (on, np.array([origin[0] - 1.0, origin[1] + 1.0, 0.0]))):
            with pytest.raises(fsmod.FsError) as e:
                sc.navfn_wave_potential(pose_, goal_)
            assert e.value.code == INVALID
        # n == 0
        empty = sc.plan_paths(on, np.zeros((0, 3)))
        assert empty["achievable"].shape == (0,)
    finally:
        sc.close()
