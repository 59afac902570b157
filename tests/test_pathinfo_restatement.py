"""The way points of fs_plan_paths_information on the CPU: the restatement of setPlanForFrontier's sampling loop
(tests/pathinfo_ref/pathinfo_ref.cpp, the running path_cut_count) against hand-computed way points and against the closed form
the GPU sizes its offsets with; the declaration and the export of the entry point."""
import math
import os
import re

import numpy as np
import pytest

import pathinfo_maps as M
import pathinfo_ref as P
import planner_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = M.RES


def test_straight_corridor_by_hand():
    """Robot on cell 2, goal on cell 102 of a one-cell-wide corridor: 101 path points, point i on cell 102 - i.  s = (int)(1.5 / 0.05)
    = 30: the loop cuts after 31 points, at i = 70, 39, 8 = cells 32, 63, 94, each looking 10 points (cells) further towards the
    goal: yaw 0.  The mirrored corridor looks the other way: yaw pi."""
    cells, origin, pose, goal = M.corridor(120, 2, 102)
    w = P.waypoints(cells, origin, RES, pose, goal)
    assert w["path_length"][0] == 101.0 and w["count"].tolist() == [3] and w["offset"].tolist() == [0, 3]
    assert w["index"].tolist() == [70, 39, 8]
    want_x = [origin[0] + (c + 0.5) * RES for c in (32, 63, 94)]
    assert w["xyyaw"][:, 0].tolist() == want_x
    assert w["xyyaw"][:, 1].tolist() == [origin[1] + 1.5 * RES] * 3
    assert w["xyyaw"][:, 2].tolist() == [0.0, 0.0, 0.0]
    cells, origin, pose, goal = M.corridor(120, 102, 2)
    w = P.waypoints(cells, origin, RES, pose, goal)
    assert w["index"].tolist() == [70, 39, 8]
    assert w["xyyaw"][:, 0].tolist() == [origin[0] + (c + 0.5) * RES for c in (72, 41, 10)]
    assert w["xyyaw"][:, 2].tolist() == [math.pi] * 3
    # the last way point of a path looks at point 0 when fewer than `lookahead` points are left: still along the corridor
    w = P.waypoints(cells, origin, RES, pose, goal, lookahead=1000)
    assert w["xyyaw"][:, 2].tolist() == [math.pi] * 3


def test_a_path_shorter_than_the_sample_distance_has_no_way_point():
    for points, want in ((30, 0), (31, 1), (61, 1), (62, 2)):
        cells, origin, pose, goal = M.corridor(120, 5, 5 + points - 1)
        w = P.waypoints(cells, origin, RES, pose, goal)
        assert w["path_length"][0] == float(points)
        assert w["count"].tolist() == [want], points
        assert P.closed_form_counts(w["path_length"], RES).tolist() == [want]


def test_every_point_is_a_way_point_at_sample_distance_zero_and_lookahead_zero_looks_nowhere():
    cells, origin, pose, goal = M.corridor(64, 40, 3)
    w = P.waypoints(cells, origin, RES, pose, goal, sample_distance=0.0, lookahead=0)
    assert w["path_length"][0] == 38.0 and w["count"].tolist() == [38]
    assert w["index"].tolist() == list(range(37, -1, -1))
    assert w["xyyaw"][:, 0].tolist() == [origin[0] + (c + 0.5) * RES for c in range(40, 2, -1)]       # robot -> frontier
    assert (w["xyyaw"][:, 2] == 0.0).all()                                                              # atan2(0, 0)
    # a sample distance below one cell is s = 0 too
    w2 = P.waypoints(cells, origin, RES, pose, goal, sample_distance=0.049, lookahead=0)
    assert w2["count"].tolist() == [38]


MAPS = [("REF2D", M.ref2d), ("plan_128", lambda: M.floor_plan(4243, 128)), ("plan_256", lambda: M.floor_plan(4244, 256)),
        ("plan_200", lambda: M.floor_plan(4245, 200))]


@pytest.mark.parametrize("name,make", MAPS, ids=[m[0] for m in MAPS])
def test_closed_form_equals_the_loop(name, make):
    """len // (s + 1) way points, the k-th on point len - (k + 1)(s + 1): on every path of 200 goals, at three samplings."""
    cells = make()
    origin = M.origin_of(cells)
    rx, ry = R.well_placed_robot(cells, np.random.default_rng(7))
    pose = R.robot_pose(origin, RES, rx, ry, 0.3)
    g, ach_in = M.goals(cells, origin, 211, 200)
    plan = R.plan(cells, origin, RES, pose, g, achievable_in=ach_in, allow_unknown=True)
    seen = 0
    for sd, look in ((1.5, 10), (0.33, 3), (4.0, 25)):
        w = P.waypoints(cells, origin, RES, pose, g, achievable_in=ach_in, allow_unknown=True, sample_distance=sd, lookahead=look)
        assert w["path_length"].tobytes() == plan["path_length"].tobytes()
        assert w["count"].tolist() == P.closed_form_counts(w["path_length"], RES, sd).tolist()
        assert w["offset"].tolist() == np.concatenate([[0], np.cumsum(w["count"])]).tolist()
        for f in np.nonzero(w["count"])[0]:
            idx = P.closed_form_indices(int(w["path_length"][f]), RES, sd, look)
            assert w["index"][w["offset"][f]:w["offset"][f + 1]].tolist() == [j for j, _ in idx], (f, sd)
        seen += int(w["count"].sum())
        assert (w["count"][plan["achievable"] == 0] == 0).all()
    assert seen > 500


def test_entry_point_is_declared_and_exported(fs):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fs_plan_paths_information\s*\(", text)
    m = re.search(r"typedef\s+struct\s+fs_path_info_params\s*\{(.*?)\}\s*fs_path_info_params\s*;", text, flags=re.S)
    assert m and [t.split()[-1] for t in m.group(1).split(";") if t.strip()] == ["sample_distance_m", "lookahead_points", "fi_threshold"]
    assert "fs_plan_paths_information" in fs.capi.EXPORTED_SYMBOLS
    lib = fs.load_library()
    assert hasattr(lib, "fs_plan_paths_information")
    assert lib.fs_abi_version() == 1
    # no context: refused before anything else is looked at
    assert lib.fs_plan_paths_information(None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, 0, None, None,
                                         None, None) == fs.capi.FS_E_INVALID
    prm = fs.capi.PathInfoParamsC()
    assert (type(prm).sample_distance_m.offset, type(prm).lookahead_points.offset, type(prm).fi_threshold.offset) == (0, 8, 16)
