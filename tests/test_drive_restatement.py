"""The drive's restatement (tests/drive_ref.py) on the episode test's 96 x 96 world, staged all unknown: the table of DESIGN.md 4.24
(figures worked out once with a prototype and held here as numbers), the invariants of every drive, and drive_ref against the same
drive composed step by step from whole sense_ref / walk_cells / goals_mapped_ref calls.  No GPU.

Cells are (x, y); stations are cell centres every 5 cells.
  A  (10,10) -> (35,10) looking east                ARRIVED, reached 5, n_seen 1415, n_revealed 704
  B  (20,30) -> (60,30) looking east: the wall at x = 47 is seen     BLOCKED, reached 5 of 9, stations 6..8 at -1, n_revealed 297
  C  the same stations looking west                 COLLIDED, reached 5, n_revealed 715
  D  A's stations, lidar, goal at cell (30,10)      MAPPED at reached 2, 1734 known cells; without stop_when_mapped ARRIVED, 2126
  E  robot 0 as C, robot 1 parked at (36,30) for three stations looking east: robot 0 ends BLOCKED only because of robot 1;
     the robots swapped give the same grid and totals and the swapped statuses"""
import numpy as np
import pytest

import drive_ref as DR
import sense_ref as SR
import test_gpu_explore_episode as EP

WORLD = EP._world()
STAGED = np.full_like(WORLD, 255)
_RESULTS = {}


def cases():
    n_yaw, _, k = SR.fan_shape(EP.PARAMS)
    return DR.table_cases(EP.ORIGIN, EP.RES, (n_yaw, k))


def result(name):
    """drive_ref of a table case, computed once and shared (read-only)"""
    if name not in _RESULTS:
        _RESULTS[name] = DR.drive_ref(STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, **cases()[name])
    return _RESULTS[name]


def known(r):
    return int((r["grid"] != 255).sum())


def test_the_table():
    a = result("A")
    assert (list(a["status"]), list(a["reached"]), a["n_seen"], a["n_revealed"]) == ([DR.ARRIVED], [5], 1415, 704)
    assert (a["station_status"][0] == SR.OK).all()
    b = result("B")
    assert (list(b["status"]), list(b["reached"]), b["n_revealed"]) == ([DR.BLOCKED], [5], 297)
    assert list(b["station_status"][0]) == [0] * 6 + [-1] * 3 and not b["seen_unknown"][0][6:].any()
    assert b["grid"][0, 30, 47] == 254 and b["grid"][0, 30, 48] == 255                     # the wall's face is on the map: that is what blocks
    c = result("C")
    assert (list(c["status"]), list(c["reached"]), c["n_revealed"]) == ([DR.COLLIDED], [5], 715)
    assert (c["grid"][0, 30, 46:49] == 255).all()                        # looking west it never saw the wall
    d, d0 = result("D"), result("D_no_stop")
    assert (list(d["status"]), list(d["reached"]), known(d)) == ([DR.MAPPED], [2], 1734)
    assert list(d["station_status"][0]) == [0, 0, 0, -1, -1, -1]
    assert (list(d0["status"]), list(d0["reached"]), known(d0)) == ([DR.ARRIVED], [5], 2126)
    e, es = result("E"), result("E_swapped")
    assert list(e["status"]) == [DR.BLOCKED, DR.ARRIVED] and list(e["reached"]) == [5, 2]
    assert list(es["status"]) == [DR.ARRIVED, DR.BLOCKED] and list(es["reached"]) == [2, 5]
    np.testing.assert_array_equal(e["grid"], es["grid"])
    assert (e["n_seen"], e["n_revealed"], e["window"]) == (es["n_seen"], es["n_revealed"], es["window"])
    np.testing.assert_array_equal(e["seen_unknown"][0], es["seen_unknown"][1])
    np.testing.assert_array_equal(e["seen_unknown"][1], es["seen_unknown"][0])
    # robot 0 alone is case C: COLLIDED
    assert list(c["status"]) == [DR.COLLIDED] and c["reached"][0] == e["reached"][0]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "D_no_stop", "E", "E_swapped"])
def test_invariants_and_the_step_by_step_composition(name):
    r = result(name)
    assert r["n_revealed"] == known(r) - int((STAGED != 255).sum())
    assert (r["grid"] == WORLD)[r["grid"] != 255].all()
    zz, yy, xx = np.nonzero(r["grid"] != STAGED)                         # (staged all unknown: every changed cell was seen)
    x0, y0, _, sx, sy, _ = r["window"]
    assert x0 <= xx.min() and xx.max() < x0 + sx and y0 <= yy.min() and yy.max() < y0 + sy
    for st, n_reached in zip(r["station_status"], r["reached"]):
        assert (st[:n_reached + 1] >= 0).all() and (st[n_reached + 1:] == -1).all()
    c = DR.drive_composed(STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, **cases()[name])
    np.testing.assert_array_equal(c["grid"], r["grid"])
    DR.assert_same_drive(c, r, name)


def test_keepout_zone_blocks_before_and_after_a_merge():
    """a zone across A's row: painted on the staged map it blocks the first move; painted again after every merge it still does
    when world costs have been written over it"""
    a = cases()["A"]
    mask = np.zeros(WORLD.shape[1:], dtype=bool)
    mask[5:16, 13] = True                                                # between station 0 (x = 10) and station 1 (x = 15)
    staged = STAGED.copy()
    staged[0][mask] = DR.KEEPOUT_COST
    r = DR.drive_ref(staged, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, keepout=mask, **a)
    assert (list(r["status"]), list(r["reached"])) == ([DR.BLOCKED], [0])
    assert r["n_seen"] > 0 and (r["grid"][0][mask] == DR.KEEPOUT_COST).all()      # station 0 swept over the zone; it is painted again
    mask2 = np.zeros_like(mask)
    mask2[5:16, 23] = True                                               # between stations 2 and 3: seen from stations 0 to 2 first
    staged = STAGED.copy()
    staged[0][mask2] = DR.KEEPOUT_COST
    r = DR.drive_ref(staged, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, keepout=mask2, **a)
    assert (list(r["status"]), list(r["reached"])) == ([DR.BLOCKED], [2])
    assert (r["grid"][0][mask2] == DR.KEEPOUT_COST).all() and (WORLD[0][mask2] == 0).all()
    free = DR.drive_ref(staged, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, keepout=None, **a)           # not painted again: the merge wipes it
    assert list(free["status"]) == [DR.ARRIVED]
