"""The GPU calls against the reference's own compiled code (oracle/_ref/libfitslam_ref.so; loader tests/reference_built.py), with no
restatement in between: fs_allocate_tasks against HungarianAlgorithm::Solve and MinPosAlgo::getAssignmentMinPos, the field of
fs_navfn_potential under the reference's updateCell, fs_plan_paths against the reference's calcPath run on that field, and
fs_refine_paths' found / not-found class against the reference's Theta*.  Reads only oracle/_ref/, never the reference tree."""
import importlib
import struct
import zlib

import numpy as np
import pytest

import alloc_ref as A
import planner_ref as P
import reference_built as B
import thetastar_ref as T

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = B.RES
# both branches (R <= n, R > n), a wave per row with n no multiple of 64, more columns than the workgroup's 1024 threads
ALLOC_SHAPES = [(1, 1), (5, 2), (64, 3), (3, 8), (16, 17), (33, 64), (64, 200), (5, 1025), (64, 4096)]
MAPS = B.planner_maps()
IDS = [m[0] for m in MAPS]
_robots = {}


def _bits(x):
    return struct.pack("<d", x)


def _robot(k):
    if k not in _robots:
        name, cells, origin = MAPS[k]
        _robots[k] = P.well_placed_robot(cells, np.random.default_rng(zlib.crc32(name.encode())))
    return _robots[k]


def _scorer(cells, origin):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    return sc


@pytest.fixture(scope="module")
def sc():
    s = fsmod.FrontierScorer(device=0)
    yield s
    s.close()


@pytest.mark.parametrize("R,n", ALLOC_SHAPES)
def test_allocate_tasks_equals_the_reference(sc, R, n):
    B.require()
    for k, family in enumerate(A.FAMILIES):
        cost, dist = A.family(family, R, n, 1000 * R + n + k + 104729)
        for method in ("hungarian", "minpos"):
            want_a, want_total = B.allocate(cost, dist, method)
            got = sc.allocate_tasks(cost, dist if method == "minpos" else None, method=method)
            what = (R, n, family, method)
            print(what, "assignment", got["assignment"].tolist()[:8], "total", got["total_cost"], "reference", want_total)
            assert got["assignment"].tolist() == want_a.tolist(), what
            assert _bits(got["total_cost"]) == _bits(want_total), what


@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
def test_potential_is_a_fixed_point_of_the_reference_update(k):
    B.require()
    name, cells, origin = MAPS[k]
    rx, ry = _robot(k)
    sc = _scorer(cells, origin)
    try:
        for allow in (False, True):
            field = sc.navfn_potential(P.robot_pose(origin, RES, rx, ry, 0.4), allow_unknown=allow)
            lowered, costarr = B.navfn_fixed_point(cells, field, (rx, ry), allow_unknown=allow)
            reached = field < B.POT_HIGH
            print(name, allow, "lowered", lowered, "reached", int(reached.sum()), "of", int((costarr < 254).sum()), "free")
            assert lowered == 0, (name, allow)
            assert (field[costarr >= 254] == B.POT_HIGH).all(), (name, allow)
            assert (reached == B.component(costarr, rx, ry)).all(), (name, allow)
            assert field[ry, rx] == 0.0 and reached.sum() > 100
    finally:
        sc.close()


@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
def test_plan_paths_equal_the_reference_calcpath_on_the_gpu_field(k):
    """40 goals (unknown cells, walls, two off the map, half of them reachable) and a batch of one"""
    B.require()
    name, cells, origin = MAPS[k]
    rx, ry = _robot(k)
    pose = P.robot_pose(origin, RES, rx, ry, -2.0)
    goals = B.planner_goals(cells, origin, zlib.crc32(name.encode()) + 2, (rx, ry), off_map=2)
    ny, nx = cells.shape
    sc = _scorer(cells, origin)
    try:
        for allow in (False, True):
            field = sc.navfn_potential(pose, allow_unknown=allow)
            got = sc.plan_paths(pose, goals, allow_unknown=allow)
            one = sc.plan_paths(pose, goals[-1:], allow_unknown=allow)
            found = off = 0
            for i, g in enumerate(goals):
                what = (name, allow, i)
                on_map = origin[0] <= g[0] < origin[0] + nx * RES and origin[1] <= g[1] < origin[1] + ny * RES
                n, px, py = B.navfn_path_on_field(cells, field, (rx, ry), B.cell_of(origin, g), allow_unknown=allow) if on_map else (0, None, None)
                off += not on_map
                assert got["achievable"][i] == (1 if n > 0 else 0), what
                if n > 0:
                    found += 1
                    assert got["path_length"][i] == float(n), what
                    assert _bits(got["path_length_m"][i]) == _bits(B.length_m(px, py, origin, RES)), what
                else:
                    assert got["path_length"][i] == P.DBL_MAX and got["path_length_m"][i] == P.DBL_MAX, what
            print(name, allow, "found", found, "of", len(goals), "off the map", off)
            assert off == 2 and found >= 20
            for key in ("achievable", "path_length", "path_length_m"):
                assert one[key].tobytes() == got[key][-1:].tobytes(), (name, allow, key)
            assert one["achievable"][0] == 1
    finally:
        sc.close()


def _refine_maps():
    import test_gpu_refine as G
    return G, [m for m in G.MAPS if m[1].size <= 300 * 300]


@pytest.mark.parametrize("j", range(5))
def test_refine_paths_find_what_the_reference_theta_star_finds(j):
    B.require()
    G, maps = _refine_maps()
    assert len(maps) == 5
    name, cells, origin = maps[j]
    sc = _scorer(cells, origin)
    try:
        s, g = G._legs(cells, origin, zlib.crc32(name.encode()) + 5, 13)
        got = sc.refine_paths(s, g)
        quirks = found = 0
        for i in range(13):
            ref = B.theta_leg(cells, origin, RES, s[i], g[i])
            gpu_found, ref_found = bool(got["status"][i] == T.OK), ref["status"] == B.FOUND
            found += ref_found
            if gpu_found != ref_found:
                # the reference's search loop drops the entry it popped last; the restated reference leg flags it
                assert gpu_found and T.leg(cells, origin, RES, s[i], g[i], which=T.REFERENCE)["quirk"], (name, i, got["status"][i], ref["status"])
                quirks += 1
        print(name, "found by the reference", found, "of 13; quirks", quirks)
        assert quirks <= 4 and found >= 3
    finally:
        sc.close()
