"""The CPU restatements under tests/*_ref/ against the reference's own compiled code (oracle/_ref/libfitslam_ref.so, built by
oracle/ref_build.py from the reference's sources; loader tests/reference_built.py): the task allocator (alloc_ref), the grid
planner's cost array, per-frontier A* leg, calcPath and fixed point (planner_ref), and the Theta* reference leg (thetastar_ref),
bit for bit.  Where a restatement differs, the restatement is wrong."""
import struct
import subprocess
import zlib

import numpy as np
import pytest

import alloc_ref as A
import planner_ref as P
import ref_build
import reference_built as B
import thetastar_ref as T

RES = B.RES
ALLOC_SHAPES = [(1, 1), (1, 5), (2, 2), (5, 2), (64, 3), (3, 8), (8, 8), (16, 17), (33, 64), (64, 64), (64, 200), (5, 1025), (64, 4096)]
METHODS = ("hungarian", "minpos")
MAPS = B.planner_maps()
IDS = [m[0] for m in MAPS]


def _bits(x):
    return struct.pack("<d", x)


def test_library_builds_and_exports_the_wrappers():
    """with a reference tree the library is built (or rebuilt when stale) and exports the six calls; never skipped"""
    if ref_build.reference_present():
        so = ref_build.build()
        assert ref_build.available()
        out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
        for sym in ref_build.SYMBOLS:
            assert f" T {sym}\n" in out, sym
    else:
        # nothing to build from: build() must leave whatever is there alone
        before = ref_build.available()
        ref_build.build()
        assert ref_build.available() == before


# ------------------------------------------------------------------ the allocator
def _same_allocation(cost, dist, method, what):
    want_a, want_total = B.allocate(cost, dist, method)
    got = A.allocate(cost, dist, method)
    assert not got["capped"], what
    assert got["assignment"].tolist() == want_a.tolist(), what
    assert _bits(got["total_cost"]) == _bits(want_total), (what, got["total_cost"], want_total)


@pytest.mark.parametrize("R,n", ALLOC_SHAPES)
def test_allocator_restatement_equals_the_reference(R, n):
    """every family and both methods; three seeds below n = 1000, one from there on"""
    B.require()
    for s in range(3 if n < 1000 else 1):
        for k, family in enumerate(A.FAMILIES):
            cost, dist = A.family(family, R, n, 1000 * R + n + k + 7919 * s)
            for method in METHODS:
                _same_allocation(cost, dist, method, (R, n, family, method, s))


def test_allocator_edge_cases():
    B.require()
    full = np.full((2, 2), A.DBL_MAX)
    for method in METHODS:
        a, total = B.allocate(full, np.ones((2, 2)), method)
        assert a.tolist() == [0, 1] and total == np.inf
        _same_allocation(full, np.ones((2, 2)), method, ("dbl_max", method))
    row = np.array([[4.0, 2.0, 7.0, 2.0, 9.0, 2.0]])
    a, total = B.hungarian(row)
    assert a.tolist() == [1] and total == 2.0
    for method in METHODS:
        _same_allocation(row, np.ones((1, 6)), method, ("one row", method))


# ------------------------------------------------------------------ the grid planner
@pytest.fixture(scope="module")
def planned():
    """per (map, allow_unknown): the robot, the 40 goals, and both legs of the restatement with their path points — computed
    once, read by every planner test"""
    cache = {}

    def get(k, allow):
        if (k, allow) not in cache:
            name, cells, origin = MAPS[k]
            rx, ry = P.well_placed_robot(cells, np.random.default_rng(zlib.crc32(name.encode())))
            pose = P.robot_pose(origin, RES, rx, ry, 0.7)
            goals = B.planner_goals(cells, origin, zlib.crc32(name.encode()) + 1, (rx, ry))
            field, _ = P.converged_field(cells, rx, ry, allow_unknown=allow)
            legs = {leg: P.plan(cells, origin, RES, pose, goals, allow_unknown=allow, leg=leg, points=True) for leg in (P.CONVERGED, P.REFERENCE_ASTAR)}
            for v in (field, goals, pose):
                v.setflags(write=False)
            cache[(k, allow)] = dict(robot=(rx, ry), pose=pose, goals=goals, field=field, legs=legs)
        return cache[(k, allow)]
    return get


def test_goals_cover_unknown_cells_and_walls(planned):
    for k, (name, cells, origin) in enumerate(MAPS):
        goals = planned(k, False)["goals"]
        assert goals.shape == (40, 3)
        at = np.array([cells[B.cell_of(origin, g)[::-1]] for g in goals])
        assert (at[:8] == (255 if (cells == 255).any() else 254)).all() and (at[8:10] == 254).all() and (at[10:] == 0).all(), name


@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
@pytest.mark.parametrize("allow", [False, True], ids=["known_only", "allow_unknown"])
def test_cost_array_and_fixed_point(planned, k, allow):
    B.require()
    name, cells, origin = MAPS[k]
    c = planned(k, allow)
    lowered, costarr = B.navfn_fixed_point(cells, c["field"], c["robot"], allow_unknown=allow)
    assert P.costs(cells, allow_unknown=allow).tobytes() == costarr.tobytes()
    assert lowered == 0
    assert ((c["field"] < B.POT_HIGH) == B.component(costarr, *c["robot"])).all()
    # the counter does count: one reachable cell raised by 3.0 is lowered again by the reference's update
    reach = np.argwhere((c["field"] < B.POT_HIGH) & (c["field"] > 0))
    y, x = reach[len(reach) // 2]
    raised = c["field"].copy()
    raised[y, x] += np.float32(3.0)
    assert B.navfn_fixed_point(cells, raised, c["robot"], allow_unknown=allow)[0] >= 1


@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
@pytest.mark.parametrize("allow", [False, True], ids=["known_only", "allow_unknown"])
def test_astar_leg_equals_the_reference_planner(planned, k, allow):
    """achievable, path_length, path_length_m and every path point of the REFERENCE_ASTAR leg, goal by goal"""
    B.require()
    name, cells, origin = MAPS[k]
    c = planned(k, allow)
    leg = c["legs"][P.REFERENCE_ASTAR]
    found = 0
    for i, g in enumerate(c["goals"]):
        want = B.navfn_plan(cells, origin, RES, c["pose"][:2], g[:2], allow_unknown=allow)
        what = (name, allow, i, want["status"], int(leg["limit"][i]))
        assert leg["achievable"][i] == want["achievable"], what
        if want["achievable"]:
            found += 1
            assert leg["path_length"][i] == float(want["len"]), what
            assert _bits(leg["path_length_m"][i]) == _bits(want["path_length_m"]), what
            assert leg["pathx"][i].tobytes() == want["pathx"].tobytes() and leg["pathy"][i].tobytes() == want["pathy"].tobytes(), what
        else:
            assert leg["path_length"][i] == P.DBL_MAX and leg["path_length_m"][i] == P.DBL_MAX, what
    assert found >= 20, (name, allow, found)


@pytest.mark.parametrize("k", range(len(MAPS)), ids=IDS)
@pytest.mark.parametrize("allow", [False, True], ids=["known_only", "allow_unknown"])
def test_converged_leg_equals_the_reference_calcpath(planned, k, allow):
    """the reference's calcPath on the restatement's converged field: the CONVERGED leg's columns and path points"""
    B.require()
    name, cells, origin = MAPS[k]
    c = planned(k, allow)
    leg = c["legs"][P.CONVERGED]
    found = 0
    for i, g in enumerate(c["goals"]):
        n, px, py = B.navfn_path_on_field(cells, c["field"], c["robot"], B.cell_of(origin, g), allow_unknown=allow)
        what = (name, allow, i, n, int(leg["limit"][i]))
        assert leg["achievable"][i] == (1 if n > 0 else 0), what
        if n > 0:
            found += 1
            assert leg["path_length"][i] == float(n), what
            assert _bits(leg["path_length_m"][i]) == _bits(B.length_m(px, py, origin, RES)), what
            assert leg["pathx"][i].tobytes() == px.tobytes() and leg["pathy"][i].tobytes() == py.tobytes(), what
    assert found >= 20, (name, allow, found)


# ------------------------------------------------------------------ Theta*
def _theta_maps():
    import test_gpu_refine as G          # the refinement's own maps, up to 300 x 300 (the GPU test holds the same ones to the reference)
    return MAPS + [m for m in G.MAPS if m[1].size <= 300 * 300]


THETA_MAPS = _theta_maps()
_CLASS = {T.OK: "found", T.START_OFF_MAP: "off", T.GOAL_OFF_MAP: "off", T.START_UNSAFE: "unsafe", T.GOAL_UNSAFE: "unsafe", T.NO_PATH: "none"}
_REF_CLASS = {B.FOUND: "found", B.START_OFF_MAP: "off", B.GOAL_OFF_MAP: "off", B.UNSAFE: "unsafe", B.NO_PATH: "none"}


def theta_legs(cells, origin, seed, n=30):
    """n legs between points on cells below 254: goals 2-4 on unknown cells, 5-7 on walls, 8 off the map, start 9 on a wall"""
    rng = np.random.default_rng(seed)

    def points(k, value=None):
        ys, xs = np.nonzero((cells < 254) if value is None else (cells == value))
        i = rng.choice(xs.size, k)
        return np.stack([origin[0] + (xs[i] + rng.uniform(0, 1, k)) * RES, origin[1] + (ys[i] + rng.uniform(0, 1, k)) * RES], axis=1)
    s, g = points(n), points(n)
    if (cells == 255).any():
        g[2:5] = points(3, 255)
    g[5:8] = points(3, 254)
    g[8] = (origin[0] + 1.0, origin[1] - 0.5)
    s[9] = points(1, 254)[0]
    return s, g


@pytest.mark.parametrize("name,cells,origin", THETA_MAPS, ids=[m[0] + f"_{i}" for i, m in enumerate(THETA_MAPS)])
def test_theta_reference_leg_equals_the_reference(name, cells, origin):
    B.require()
    s, g = theta_legs(cells, origin, zlib.crc32(name.encode()) + cells.shape[0])
    classes = []
    for i in range(len(s)):
        allow = i % 4 != 3                       # every fourth leg with allow_unknown off
        want = B.theta_leg(cells, origin, RES, s[i], g[i], allow_unknown=allow)
        got = T.leg(cells, origin, RES, s[i], g[i], allow_unknown=allow, which=T.REFERENCE)
        what = (name, i, got["status"], want["status"])
        assert _CLASS[got["status"]] == _REF_CLASS[want["status"]], what
        classes.append(_REF_CLASS[want["status"]])
        if want["status"] == B.FOUND:
            assert got["poses"].tobytes() == want["poses"].tobytes(), what
            # generatePath's list: backtrace pushes the last vertex twice
            assert np.vstack([got["vertices"], got["vertices"][-1:]]).tobytes() == want["raw"].tobytes(), what
    assert classes.count("found") >= 8 and classes.count("unsafe") >= 3 and classes.count("off") == 1, (name, classes)
