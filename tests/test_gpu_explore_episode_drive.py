"""The closed exploration loop of tests/test_gpu_explore_episode.py with the teleport replaced by a drive: search ->
score and rank -> refine_paths(robot -> best candidate) -> stations_along -> DRIVE: the robot senses at every station, stops when
a wall shows up on its path or when the goal is mapped, and ends the tick at station `reached`.

A twin context takes the same stations through the host loop over fs_trace_segments, fs_sense and fs_goals_mapped
(drive_ref.drive_by_calls).  After every tick the two staged grids, the rankings, the chosen goals and the census are equal, and
every output of the drive equals the host loop's.

A goal ends MAPPED (done), or is given up: no path to it, arrived without mapping it, or stopped short of it three times."""
import numpy as np
import pytest

import drive_ref as DR
import sense_ref as SR
import test_gpu_explore_episode as EP

pytestmark = pytest.mark.gpu

SPACING_M, MAX_TICKS, MAX_STOPS = 0.25, 40, 3
# What the twin's own run (the host loop over the calls the library already had, not the code under test) gave on an MI355X: 40
# ticks (the cap), 9 goals mapped, every drive ended before its last station.  Held as lower bounds for both; for
# the early stops the bound is that there is one.
MIN_TICKS, MIN_DONE, MIN_EARLY = 40, 9, 1


def test_driven_episode_equals_the_host_loop(fs):
    world = EP._world()
    start = (-1.2 + EP.RES / 2, -1.5 + EP.RES / 2, 0.0)
    blank = np.full_like(world, 255)
    a, b, w = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (a, b):
            s.set_ray_params(robot_radius=0.15, **EP.PARAMS)
            s.upload_grid(blank, EP.ORIGIN, EP.RES)
            mx = s.max_arrival()
            s.set_arrival_limits(mx["max_gt"], 0.0)
            s.upload_world(world)
        w.upload_grid(world, EP.ORIGIN, EP.RES)                          # the collision walk's map
        fan = dict(delta_theta=EP.PARAMS["delta_theta"], camera_fov=EP.PARAMS["camera_fov"], n_rays=EP.PARAMS["n_rays"])
        revealed = 0
        for s in (a, b):
            revealed = s.sense([start])["n_revealed"]                    # tick 0: the whole fan from the start cell
        robot, black, stops = start[:2], set(), {}
        ticks = done = early = n_stations = 0
        ends = {}
        known = 0
        while ticks < MAX_TICKS:
            ga, gb = a.read_grid_region(), b.read_grid_region()
            np.testing.assert_array_equal(ga, gb)
            census = a.grid_census()
            assert census == b.grid_census() == SR.census_ref(ga)
            assert census["known"] >= known and census["known"] == revealed
            known = census["known"]
            assert (ga == world)[ga != 255].all()
            ta, tb = EP._tick(a, robot, black), EP._tick(b, robot, black)
            assert (ta is None) == (tb is None)
            if ta is None:
                break
            np.testing.assert_array_equal(ta[0], tb[0])
            for k in ("records", "weighted_cost", "arrival_utility", "distance_utility", "order"):
                np.testing.assert_array_equal(ta[2][k], tb[2][k], err_msg=k)
            c = EP._best(ta[2], ta[3])
            assert c == EP._best(tb[2], tb[3])
            if c < 0:
                break
            ticks += 1
            goal = ta[1][c]
            key = (float(goal[0]), float(goal[1]))
            pa, pb = a.refine_paths([robot], [goal]), b.refine_paths([robot], [goal])
            assert pa["status"][0] == pb["status"][0]
            np.testing.assert_array_equal(pa["poses"][0], pb["poses"][0])
            if pa["status"][0] != 0 or pa["poses"][0].shape[0] == 0:
                black.add(key)                                           # no path: given up
                continue
            st, first, _ = fs.capi.stations_along(pa["poses"][0], SPACING_M, **fan)
            first[-1] = int(ta[2]["records"][c]["argmax"])               # at the goal: the window the scoring chose
            assert 1 <= st.shape[0] <= fs.capi.FS_DRIVE_MAX_STATIONS
            n_stations += st.shape[0]
            got = a.drive([st], [goal], [first])
            twin = DR.drive_by_calls(b, w, [st], [goal], [first])
            DR.assert_same_drive(got, twin, f"tick {ticks}")
            revealed += got["n_revealed"]
            status, reached = int(twin["status"][0]), int(twin["reached"][0])     # (the twin's: equal to the drive's, see above)
            ends[status] = ends.get(status, 0) + 1
            robot = (float(st[reached][0]), float(st[reached][1]))
            if reached < st.shape[0] - 1:
                early += 1
            if status == DR.MAPPED:
                done += 1
            elif status == DR.ARRIVED:
                black.add(key)                                           # there, and still not mapped: given up
            else:
                stops[key] = stops.get(key, 0) + 1
                if stops[key] >= MAX_STOPS:
                    black.add(key)
        print(f"driven episode: {ticks} ticks, {done} goals mapped, {early} drives ended before their last station, {len(black)} goals given up, "
              f"{n_stations} stations, {known} of {world.size} cells known; drives by final status {dict(sorted(ends.items()))}")
        np.testing.assert_array_equal(a.read_grid_region(), b.read_grid_region())
        assert ticks >= MIN_TICKS and done >= MIN_DONE and early >= MIN_EARLY
        assert a.grid_census()["known"] == revealed > 1000
    finally:
        a.close(); b.close(); w.close()
