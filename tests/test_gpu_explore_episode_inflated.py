"""tests/test_gpu_explore_episode.py's closed loop on a map a FIT-SLAM planner would see: after every sweep the whole staged map
goes through the inflation layer at the reference's global parameters, on the device.

A twin context takes the host route the layer replaces: the sweep's window through fs_update_grid_region, the map read back,
inflated by tests/inflation_ref.py's exact transform and sent again.  After every tick the two staged grids, the frontier lists,
the rankings, the chosen goals and the census are equal.  The same world as the plain episode, at most 12 of its 40 ticks."""
import numpy as np
import pytest

import inflation_ref as I
import sense_ref as SR
from test_gpu_explore_episode import ORIGIN, PARAMS, RES, _best, _tick, _world

pytestmark = pytest.mark.gpu

MAX_TICKS = 12
# the costmap's robot_radius (active_slam_nav2_params.yaml), which is the layer's inscribed radius.  With the plain episode's 0.15 m
# this episode ended after one tick on an MI355X: costs >= 240 reach two cells out from every wall, and a footprint of three cells
# more does not fit a doorway of six or seven
ROBOT_RADIUS = 0.05


def test_inflated_episode_on_the_device_equals_the_host_route(fs):
    world = _world()
    start = (-1.2 + RES / 2, -1.5 + RES / 2, 0.0)
    host = np.full_like(world, 255)                                   # the twin's master grid
    a, b = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (a, b):
            s.set_ray_params(robot_radius=ROBOT_RADIUS, **PARAMS)
            s.upload_grid(host, ORIGIN, RES)
            mx = s.max_arrival()
            s.set_arrival_limits(mx["max_gt"], 0.0)
        a.upload_world(world)
        inflated_cells = []

        def sweep(pose, first):
            """sense, then inflate: on the device in a, through the host in b; returns a's sweep"""
            got = a.sense([pose], None if first is None else [first], rays=True)
            n_seeds, n_changed = a.inflate(*I.GLOBAL)
            want = SR.sense_ref(host, world, ORIGIN, RES, PARAMS, [pose], None if first is None else [first])
            for k in ("status", "seen_unknown", "ray_unknown"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            assert (got["n_seen"], got["n_revealed"], got["window"]) == (want["n_seen"], want["n_revealed"], tuple(int(v) for v in want["window"]))
            x0, y0, z0, wx, wy, wz = want["window"]
            if wx:
                b.update_grid_region(x0, y0, z0, want["grid"][z0:z0 + wz, y0:y0 + wy, x0:x0 + wx])
            back = b.read_grid_region()
            np.testing.assert_array_equal(back, want["grid"])
            grid, seeds, changed = I.inflate_exact(back[0], I.GLOBAL, RES)
            b.update_grid_region(0, 0, 0, grid[None])
            assert (n_seeds, n_changed) == (seeds, changed)
            host[0] = grid
            inflated_cells.append(changed)
            return got

        first = sweep(start, None)
        assert first["n_revealed"] >= 1
        robot, black, ticks, done, known = start[:2], set(), 0, 0, 0
        while ticks < MAX_TICKS:
            np.testing.assert_array_equal(a.read_grid_region(), host)
            np.testing.assert_array_equal(b.read_grid_region(), host)
            census = a.grid_census()
            assert census == SR.census_ref(host) == b.grid_census()
            assert census["known"] >= known
            known = census["known"]
            ta, tb = _tick(a, robot, black), _tick(b, robot, black)
            assert (ta is None) == (tb is None)
            if ta is None:
                break
            np.testing.assert_array_equal(ta[0], tb[0])
            for k in ("records", "weighted_cost", "arrival_utility", "distance_utility", "order"):
                np.testing.assert_array_equal(ta[2][k], tb[2][k], err_msg=k)
            c = _best(ta[2], ta[3])
            assert c == _best(tb[2], tb[3])
            if c < 0:
                break
            ticks += 1
            goal = ta[1][c]
            got = sweep(tuple(goal), int(ta[2]["records"][c]["argmax"]))
            assert got["status"][0] == SR.OK
            mapped = a.goals_mapped([goal])
            np.testing.assert_array_equal(mapped, b.goals_mapped([goal]))
            if mapped[0]:
                done += 1
            else:
                black.add((float(goal[0]), float(goal[1])))
            gx, gy = int((goal[0] - ORIGIN[0]) / RES), int((goal[1] - ORIGIN[1]) / RES)
            if world[0, gy, gx] == 0:
                robot = (float(goal[0]), float(goal[1]))
        print(f"inflated episode: {ticks} ticks, {done} goals mapped, {len(black)} given up, {known} of {host.size} cells known, "
              f"cells changed by the layer per sweep {inflated_cells}")
        assert ticks >= 1 and len(inflated_cells) == ticks + 1 and sum(inflated_cells) > 1000
        lethal = host[0] == 254
        assert lethal.any() and (host[0][lethal] == world[0][lethal]).all() and ((host[0] > 0) & (host[0] < 253)).sum() > 500
    finally:
        a.close(); b.close()
