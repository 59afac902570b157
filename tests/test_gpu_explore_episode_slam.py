"""The driven exploration loop of tests/test_gpu_explore_episode_drive.py with the drive gated on Fisher information:
search -> score and rank -> refine_paths(robot -> best candidate) -> stations_along and poses_along -> DRIVE_SLAM: the robot
senses the map and the landmarks at every station and stops when a wall shows up on its path, when the goal is mapped — or when the
landmarks discovered so far no longer carry its pose (FS_DRIVE_UNSAFE).

A twin context takes the same poses through the host loop over fs_trace_segments, fs_sense, fs_sense_landmarks, fs_score_fim and
fs_goals_mapped (drive_slam_ref.drive_slam_by_calls).  After every tick the two staged grids, the world clouds' counters and
discovered lists, the staged clouds (byte for byte), the rankings and every output of the drive are equal.

The threshold comes from the twin: an ungated scouting episode on the twin's route alone gives the information of every station it
drives on from; the threshold lies midway between the two smallest of those values that are far enough apart, and no value of the
scouting episode or, tick by tick, of the gated twin may lie within 1e-3 relative of it (a precondition on the inputs, asserted before the drive under test is compared)."""
import numpy as np
import pytest

import drive_ref as DR
import drive_slam_ref as DS
import test_gpu_explore_episode as EP

pytestmark = pytest.mark.gpu

SPACING_M, MAX_TICKS, MAX_STOPS, GAP = 0.25, 8, 2, 1.0e-3
FIM = (2.0, 1.0)
SENSOR = dict(max_dist=2.0, max_angle=1.0, line_of_sight=1, min_views=1)
FLOATS = ("info_ref", "trace", "logdet")


def _world_cloud(world):
    """one point on every lethal cell of the world, anywhere inside the cell, up to 0.6 m above the floor"""
    ys, xs = np.nonzero(world[0] == 254)
    rng = np.random.default_rng(23)
    px = EP.ORIGIN[0] + (xs + rng.uniform(0.05, 0.95, size=xs.shape[0])) * EP.RES
    py = EP.ORIGIN[1] + (ys + rng.uniform(0.05, 0.95, size=ys.shape[0])) * EP.RES
    return np.stack([px, py, rng.uniform(0.0, 0.6, size=xs.shape[0])], 1).astype(np.float32)


def _ctx(fs, world, cloud):
    s = fs.FrontierScorer(device=0)
    s.set_ray_params(robot_radius=0.15, **EP.PARAMS)
    s.lookup_generate()
    s.set_fim_params(*FIM)
    s.upload_grid(np.full_like(world, 255), EP.ORIGIN, EP.RES)
    mx = s.max_arrival()
    s.set_arrival_limits(mx["max_gt"], 0.0)
    s.upload_world(world)
    s.upload_world_landmarks(cloud)
    return s


def _same_tick(ta, tb, what):
    np.testing.assert_array_equal(ta[0], tb[0], err_msg=what)
    for k in ("weighted_cost", "arrival_utility", "distance_utility", "order"):
        np.testing.assert_array_equal(ta[2][k], tb[2][k], err_msg=f"{k} {what}")
    for f in ta[2]["records"].dtype.names:                              # (the Fisher float sums are not bit-stable from call to call)
        if f in FLOATS:
            np.testing.assert_allclose(ta[2]["records"][f], tb[2]["records"][f], rtol=1e-5, err_msg=f"{f} {what}")
        else:
            assert ta[2]["records"][f].tobytes() == tb[2]["records"][f].tobytes(), f"{f} {what}"


def _same_state(a, b, what):
    np.testing.assert_array_equal(a.read_grid_region(), b.read_grid_region(), err_msg=what)
    wa, wb = a.world_landmarks(), b.world_landmarks()
    assert wa["n_discovered"] == wb["n_discovered"], what
    np.testing.assert_array_equal(wa["world_index"], wb["world_index"], err_msg=what)
    np.testing.assert_array_equal(wa["views"], wb["views"], err_msg=what)
    sa, sb = a.staged_cloud(), b.staged_cloud()
    assert (sa["m"], sa["n_chunks"]) == (sb["m"], sb["n_chunks"]) and all(sa[k].tobytes() == sb[k].tobytes() for k in ("soa", "spheres", "perm")), what


def _episode(fs, a, b, w, world, threshold, gate):
    """the loop on the twin b (host loop) and, when a is given, on a (drive_slam) beside it.  Returns (ticks, ends by status,
    every information value the twin reported at a station >= 1 that it drove on from)."""
    start = (-1.2 + EP.RES / 2, -1.5 + EP.RES / 2, 0.0)
    fan = dict(delta_theta=EP.PARAMS["delta_theta"], camera_fov=EP.PARAMS["camera_fov"], n_rays=EP.PARAMS["n_rays"])
    both = [s for s in (a, b) if s is not None]
    for s in both:
        s.sense([start])                                                 # tick 0: the whole fan from the start cell
        s.sense_landmarks(DS.pose_rows([start], 0.0), SENSOR)
    robot, black, stops, ends, values, ticks = start[:2], set(), {}, {}, [], 0
    while ticks < MAX_TICKS:
        if a is not None:
            _same_state(a, b, f"before tick {ticks + 1}")
        tb = EP._tick(b, robot, black)
        if a is not None:
            ta = EP._tick(a, robot, black)
            assert (ta is None) == (tb is None)
            if ta is not None:
                _same_tick(ta, tb, f"tick {ticks + 1}")
        if tb is None:
            break
        c = EP._best(tb[2], tb[3])
        if c < 0:
            break
        ticks += 1
        goal = tb[1][c]
        key = (float(goal[0]), float(goal[1]))
        pb = b.refine_paths([robot], [goal])
        if a is not None:
            pa = a.refine_paths([robot], [goal])
            assert pa["status"][0] == pb["status"][0]
            np.testing.assert_array_equal(pa["poses"][0], pb["poses"][0])
        if pb["status"][0] != 0 or pb["poses"][0].shape[0] == 0:
            black.add(key)
            continue
        st, first, idx = fs.capi.stations_along(pb["poses"][0], SPACING_M, **fan)
        poses = fs.capi.poses_along(pb["poses"][0], idx)
        np.testing.assert_array_equal(poses[:, :3], st)
        kw = dict(lm_sensor=SENSOR, threshold=threshold, gate=gate)
        twin = DS.drive_slam_by_calls(b, w, [poses], [goal], [first], **kw)
        values += [float(v) for v in twin["information"][0][1:int(twin["reached"][0])]]     # (stations it drove on from)
        if gate:                                                         # the precondition, on the twin's values of this tick
            v = np.asarray(twin["information"][0], dtype=np.float64)
            assert (np.abs(v - threshold) > GAP * threshold).all(), (ticks, threshold, v)
        if a is not None:
            got = a.drive_slam([poses], [goal], [first], **kw)
            DS.assert_same_slam(got, twin, f"tick {ticks}")
        status, reached = int(twin["status"][0]), int(twin["reached"][0])
        ends[status] = ends.get(status, 0) + 1
        robot = (float(st[reached][0]), float(st[reached][1]))
        if status == DR.MAPPED:
            continue
        if status == DR.ARRIVED:
            black.add(key)
        else:                                                            # BLOCKED, COLLIDED, OFF_MAP, UNSAFE: tried again, then given up
            stops[key] = stops.get(key, 0) + 1
            if stops[key] >= MAX_STOPS:
                black.add(key)
    if a is not None:
        _same_state(a, b, "at the end")
    return ticks, ends, values


def test_gated_episode_equals_the_host_loop(fs):
    world = EP._world()
    cloud = _world_cloud(world)
    assert 400 <= cloud.shape[0] <= 1500
    w = fs.FrontierScorer(device=0)
    w.upload_grid(world, EP.ORIGIN, EP.RES)                              # the collision walk's map
    scout = _ctx(fs, world, cloud)
    try:
        ticks, ends, values = _episode(fs, None, scout, w, world, 0.0, False)
    finally:
        scout.close()
    values = np.unique(np.asarray(values))
    print(f"scouting episode: {ticks} ticks, drives by final status {dict(sorted(ends.items()))}, information {values.min():.2f} .. {values.max():.2f}")
    assert ticks >= 3 and values.shape[0] >= 2 and values[0] < values[1]
    # just above the smallest value of a station the scout drove on from: until the gated robot stands there it meets what the
    # scout met — or stops UNSAFE earlier, at a last station the scout's goal test did not end — so some tick ends UNSAFE
    j = next(j for j in range(1, values.shape[0]) if values[j] - values[j - 1] > 4.0 * GAP * values[j])    # (the first gap wide enough)
    threshold = DS.threshold_between([values], values[j - 1], values[j], GAP)
    a, b = _ctx(fs, world, cloud), _ctx(fs, world, cloud)
    try:
        ticks, ends, _ = _episode(fs, a, b, w, world, threshold, True)
        print(f"gated episode: threshold {threshold:.3f}, {ticks} ticks, drives by final status {dict(sorted(ends.items()))}, "
              f"{a.world_landmarks()['n_discovered']} of {cloud.shape[0]} landmarks discovered, {a.grid_census()['known']} cells known")
        assert ticks >= 2 and ends.get(DS.UNSAFE, 0) >= 1
        ga = a.read_grid_region()
        assert (ga == world)[ga != 255].all()
    finally:
        a.close(); b.close(); w.close()
