"""fs_drive on the GPU (fit-slam_amd/csrc/fs_drive.hip) against tests/drive_ref.py bit for bit — every output and the
whole staged map read back — and against a twin context driven step by step with the calls the library already had
(fs_trace_segments, fs_sense, fs_goals_mapped; drive_ref.drive_by_calls; the world walk on a third context whose staged grid is
the world).  The table of DESIGN.md 4.24 on the episode's 96 x 96 world, stations off the map, sweeps that see nothing, robots
with different station counts, a sensor of the call's own, stored keep-out zones, what the context computes after a drive, and
the error paths."""
import ctypes

import numpy as np
import pytest

import drive_ref as DR
import sense_ref as SR
import test_drive_restatement as TR
import test_gpu_explore_episode as EP

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
WORLD, STAGED = TR.WORLD, TR.STAGED
# what a refused sweep says, word for word
NO_GRID = "fs_upload_grid has not been called"
NO_WORLD = "fs_upload_world has not been called"
NO_SENSOR = "fs_set_ray_params has not been called and no sensor is given"
NOT_2D = "fs_drive is defined on a 2-D costmap (nz == 1)"


def _ctx(fs, staged, world, origin, res, params, zones=()):
    s = fs.FrontierScorer(device=0)
    s.set_ray_params(robot_radius=0.15, **params)
    for z in zones:
        s.keepout_add_disc(*z)
    s.upload_grid(staged, origin, res)
    if world is not None:
        s.upload_world(world)
    return s


def _trio(fs, staged, world, origin, res, params, zones=()):
    """(the driven context, its twin for the host loop, a context whose staged grid is the world)"""
    return (_ctx(fs, staged, world, origin, res, params, zones), _ctx(fs, staged, world, origin, res, params, zones),
            _ctx(fs, world, None, origin, res, params))


def _check(a, b, w, staged, world, origin, res, params, case, sensor=None, keepout=None, block=(253, 254)):
    """one drive on a, the restatement, the host loop on b: all equal, the staged maps too.  Returns the restatement's result."""
    got = a.drive(case["stations"], case["goals"], case["first_ray"], sensor=sensor, block=block, stop_when_mapped=case["stop_when_mapped"])
    want = DR.drive_ref(staged, world, origin, res, params if sensor is None else sensor, case["stations"], case["goals"], case["first_ray"],
                        block=block, stop_when_mapped=case["stop_when_mapped"], keepout=keepout)
    print("drive:", list(got["status"]), list(got["reached"]), got["n_seen"], got["n_revealed"], got["window"])
    DR.assert_same_drive(got, want, "restatement")
    np.testing.assert_array_equal(a.read_grid_region(), want["grid"])
    twin = DR.drive_by_calls(b, w, case["stations"], case["goals"], case["first_ray"], sensor=sensor, block=block,
                             stop_when_mapped=case["stop_when_mapped"])
    DR.assert_same_drive(got, twin, "host loop")
    np.testing.assert_array_equal(a.read_grid_region(), b.read_grid_region())
    return want


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "D_no_stop", "E", "E_swapped"])
def test_table_cases_equal_the_restatement_and_the_host_loop(fs, name):
    a, b, w = _trio(fs, STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS)
    try:
        case = TR.cases()[name]
        want = _check(a, b, w, STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, case)
        DR.assert_same_drive(want, TR.result(name), "the table's figures")
        assert a.grid_census()["known"] == want["n_revealed"]
    finally:
        a.close(); b.close(); w.close()


def _small(fs):
    """a 61 x 61 map: (world, staged with a block unknown, origin, res, params)"""
    wl = fs.synth.make_small_2d(461, n=61, n_cand=4, n_landmarks=4)
    world = np.array(wl.cells, dtype=np.uint8, copy=True)
    staged = world.copy()
    staged[:, 12:44, 15:46] = 255
    params = dict(max_camera_depth=wl.max_camera_depth, delta_theta=wl.delta_theta, camera_fov=wl.camera_fov, n_rays=wl.n_yaw,
                  elev=tuple(wl.elev), obst=(240, 254), trace=(255, 255), polygon=tuple(wl.polygon))
    return world, staged, tuple(wl.origin), wl.resolution, params


def _row(world, origin, res, y, xs):
    return np.array([DR.cell_centre(x, y, origin, res) for x in xs], dtype=np.float64)


def test_stations_off_the_map_sweeps_that_see_nothing_and_uneven_fleets(fs):
    world, staged, origin, res, params = _small(fs)
    n_yaw, _, k = SR.fan_shape(params)
    far = DR.cell_centre(1, 1, origin, res)
    open_world = np.zeros_like(world)                                    # nothing to hit: the statuses below are the stations' doing
    a, b, w = _trio(fs, staged, open_world, origin, res, params)
    try:
        def fresh():
            for s in (a, b):
                s.upload_grid(staged, origin, res)
        # (block = (300, 301) is an empty range of byte costs: the staged map's own walls never block here)
        # station 0 off the map: it sees nothing, the first move fails
        st = _row(world, origin, res, 20, [5, 10, 15])
        st[0, 0] = origin[0] - 1.0
        case = dict(stations=[st], goals=[far], first_ray=None, stop_when_mapped=False)
        r = _check(a, b, w, staged, open_world, origin, res, params, case, block=(300, 301))
        assert (list(r["status"]), list(r["reached"]), list(r["station_status"][0]), r["n_seen"]) == ([DR.OFF_MAP], [0], [SR.OFF_MAP, -1, -1], 0)
        # a middle station off the map, next to a robot that drives on
        fresh()
        st = _row(world, origin, res, 22, [5, 10, 15, 20, 25])
        st[2, 1] = origin[1] + 61 * res + 0.5
        ok = _row(world, origin, res, 40, [50, 45, 40, 35])
        case = dict(stations=[st, ok], goals=[far, far], first_ray=None, stop_when_mapped=False)
        r = _check(a, b, w, staged, open_world, origin, res, params, case, block=(300, 301))
        assert (list(r["status"]), list(r["reached"])) == ([DR.OFF_MAP, DR.ARRIVED], [1, 3])
        assert list(r["station_status"][0]) == [0, 0, -1, -1, -1]
        # a fan whose end points all leave the map: every station sees nothing and the drive goes on to the end
        fresh()
        gone = dict(params, polygon=(origin[0] + 100.0, -1e300, 1e300, 1e300))
        case = dict(stations=[ok], goals=[far], first_ray=[np.full(4, n_yaw - k, np.int32)], stop_when_mapped=False)
        r = _check(a, b, w, staged, open_world, origin, res, params, case, sensor=gone, block=(300, 301))
        assert (list(r["status"]), list(r["reached"]), list(r["station_status"][0]), r["window"]) == ([DR.ARRIVED], [3], [SR.OFF_MAP] * 4, (0,) * 6)
        np.testing.assert_array_equal(a.read_grid_region(), staged)
    finally:
        a.close(); b.close(); w.close()
    # the map's own walls: three robots with 9, 1 and 4 stations, NULL first_ray, then a sensor of the call's own with windows
    a, b, w = _trio(fs, staged, world, origin, res, params)
    try:
        fleet = [_row(world, origin, res, 30, range(8, 53, 5)), _row(world, origin, res, 10, [40]), _row(world, origin, res, 50, [50, 44, 38, 32])]
        goals = [DR.cell_centre(30, 28, origin, res), DR.cell_centre(40, 10, origin, res), DR.cell_centre(20, 14, origin, res)]   # two of them in the unknown block
        case = dict(stations=fleet, goals=goals, first_ray=None, stop_when_mapped=True)
        r = _check(a, b, w, staged, world, origin, res, params, case)
        assert r["reached"][1] == 0 and r["status"][1] in (DR.ARRIVED, DR.MAPPED) and r["n_seen"] > 0
        for s in (a, b):
            s.upload_grid(staged, origin, res)
        sensor = dict(params, max_camera_depth=2 * params["max_camera_depth"], obst=(253, 254), trace=(200, 255))
        first = [np.arange(f.shape[0], dtype=np.int32) % (n_yaw - k + 1) - (j == 1) for j, f in enumerate(fleet)]    # (robot 1: -1, the lidar)
        case = dict(stations=fleet, goals=goals, first_ray=first, stop_when_mapped=False)
        _check(a, b, w, staged, world, origin, res, params, case, sensor=sensor, block=(200, 254))
    finally:
        a.close(); b.close(); w.close()


def test_stored_keepout_zone_blocks_before_and_after_a_merge(fs):
    case = TR.cases()["A"]
    for x, first, reached in ((13, 26, 0), (23, 0, 2)):
        # a disc of two cells' radius on the row: looking west (x = 13) no sweep ever covers it; looking east (x = 23) the sweeps
        # from stations 0 to 2 write the world's free cells over it and the zone is painted again each time
        zone = (DR.cell_centre(x, 10, EP.ORIGIN, EP.RES)[0], DR.cell_centre(x, 10, EP.ORIGIN, EP.RES)[1], 2 * EP.RES)
        a, b, w = _trio(fs, STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, zones=[zone])
        try:
            mask = a.keepout_get()[2].astype(bool)
            assert mask[10, x] and 4 < mask.sum() < 40
            painted = STAGED.copy()
            painted[0][mask] = DR.KEEPOUT_COST
            np.testing.assert_array_equal(a.read_grid_region(), painted)
            c = dict(case, first_ray=[np.full(6, first, np.int32)])
            r = _check(a, b, w, painted, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, c, keepout=mask)
            assert (list(r["status"]), list(r["reached"])) == ([DR.BLOCKED], [reached])
            assert (a.read_grid_region()[0][mask] == DR.KEEPOUT_COST).all()
            if first == 0:
                seen = r["grid"] != painted
                assert seen[0, 10, x - 3] and seen[0, 10, x + 3]             # the sweeps did pass over the zone
        finally:
            a.close(); b.close(); w.close()


def _tick(s, robot):
    fr, _ = s.search_frontiers(robot, want_every=False)
    goals = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
    length = np.hypot(goals[:, 0] - robot[0], goals[:, 1] - robot[1])
    costs = s.get_frontier_costs(goals, length, np.zeros(fr.shape[0]), frontier_size=fr["size"])
    return fr, goals, costs


def test_context_after_a_drive_equals_a_fresh_snapshot(fs):
    case = TR.cases()["D_no_stop"]
    a = _ctx(fs, STAGED, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS)
    b = fs.FrontierScorer(device=0)
    try:
        mx = a.max_arrival()
        a.set_arrival_limits(mx["max_gt"], 0.0)
        start = case["stations"][0][0]
        a.sense([start])                                                 # something known, so that every derived image exists ...
        robot = (float(start[0]), float(start[1]))
        _tick(a, robot)                                                  # ... and the cached fields too, before the drive
        a.refine_paths([robot], [case["stations"][0][1][:2]])
        a.drive(case["stations"], case["goals"], case["first_ray"], stop_when_mapped=False)
        want = TR.result("D_no_stop")
        merged = a.read_grid_region()
        np.testing.assert_array_equal(merged, want["grid"])              # (station 0's extra sweep saw what the drive's sees again)
        b.set_ray_params(robot_radius=0.15, **EP.PARAMS)
        b.upload_grid(merged, EP.ORIGIN, EP.RES)
        b.set_arrival_limits(mx["max_gt"], 0.0)
        end = case["stations"][0][-1]
        robot = (float(end[0]), float(end[1]))
        ta, tb = _tick(a, robot), _tick(b, robot)
        np.testing.assert_array_equal(ta[0], tb[0])
        assert ta[0].shape[0] >= 1
        for k in ("records", "weighted_cost", "arrival_utility", "distance_utility", "order"):
            np.testing.assert_array_equal(ta[2][k], tb[2][k], err_msg=k)
        pa, pb = a.refine_paths([robot] * ta[1].shape[0], ta[1]), b.refine_paths([robot] * ta[1].shape[0], ta[1])
        for k in ("status", "cost", "n_vertices", "n_poses"):
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
        for x, y in zip(pa["poses"], pb["poses"]):
            np.testing.assert_array_equal(x, y)
        assert a.grid_census() == b.grid_census() == SR.census_ref(merged)
        # a sweep after the drive equals the restatement: the mark image was left clean
        pose = [DR.cell_centre(60, 30, EP.ORIGIN, EP.RES)]
        got = a.sense(pose, rays=True)
        ref = SR.sense_ref(merged, WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, pose)
        for k in ("status", "seen_unknown", "ray_unknown"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        assert (got["n_seen"], got["n_revealed"], got["window"]) == (ref["n_seen"], ref["n_revealed"], tuple(int(v) for v in ref["window"]))
        np.testing.assert_array_equal(a.read_grid_region(), ref["grid"])
    finally:
        a.close(); b.close()


def test_error_paths_leave_the_map_and_the_outputs_alone(fs):
    case = TR.cases()["E"]
    n_yaw, _, k = SR.fan_shape(EP.PARAMS)
    s = fs.FrontierScorer(device=0)
    try:
        def refused(code, f, *args, text=None, **kw):
            with pytest.raises(fs.capi.FsError) as e:
                f(*args, **kw)
            assert e.value.code == code
            assert text is None or str(e.value) == f"fitslam_frontier error {code}: {text}"
        run = lambda **kw: s.drive(case["stations"], case["goals"], case["first_ray"], **kw)
        refused(FS_E_STATE, run, text=NO_GRID)                           # no grid
        s.upload_grid(STAGED, EP.ORIGIN, EP.RES)
        refused(FS_E_STATE, run, text=NO_WORLD)                          # no world
        s.upload_world(WORLD)
        refused(FS_E_STATE, run, text=NO_SENSOR)                         # no ray parameters and no sensor
        assert run(sensor=EP.PARAMS)["n_seen"] == TR.result("E")["n_seen"]
        s.upload_grid(STAGED, EP.ORIGIN, EP.RES)
        s.set_ray_params(robot_radius=0.15, **EP.PARAMS)
        refused(FS_E_INVALID, run, sensor=dict(EP.PARAMS, elev=()))
        ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p)
        xyz = np.ascontiguousarray(np.concatenate(case["stations"]))
        goals = np.ascontiguousarray(case["goals"], dtype=np.float64)
        first = np.ascontiguousarray(np.concatenate(case["first_ray"]).astype(np.int32))
        T = xyz.shape[0]

        def raw(n_st, fr):
            n_st = np.asarray(n_st, dtype=np.int32)
            out = [np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(T, 77, np.int32), np.full(T, 77, np.int32), np.full(6, 77, np.int32)]
            n_seen, n_rev = ctypes.c_int64(77), ctypes.c_int64(77)
            rc = s._L.fs_drive(s._h, 2, ptr(xyz), ptr(n_st), ptr(fr), ptr(goals), None, None, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                               ctypes.byref(n_seen), ctypes.byref(n_rev), ptr(out[4]))
            assert all((o == 77).all() for o in out) and n_seen.value == 77 and n_rev.value == 77
            return rc
        for bad in (n_yaw - k + 1, -2):
            fr = first.copy(); fr[T - 2] = bad
            assert raw([9, 3], fr) == FS_E_INVALID
            assert s._L.fs_last_error(s._h).decode() == f"first_ray[{T - 2}] = {bad} is outside [-1, {n_yaw - k}]"
        assert raw([12, 0], first) == FS_E_INVALID                       # a robot without a station
        assert raw([fs.capi.FS_DRIVE_MAX_STATIONS + 1, 3], first) == FS_E_INVALID    # (refused before a station is read)
        np.testing.assert_array_equal(s.read_grid_region(), STAGED)
        # no robots: a no-op
        r = s.drive([], np.zeros((0, 3)))
        assert (r["n_seen"], r["n_revealed"], r["window"], r["status"].shape) == (0, 0, (0,) * 6, (0,))
        np.testing.assert_array_equal(s.read_grid_region(), STAGED)
        # a 3-D grid is refused
        c1 = fs.synth.make_workload("C1", n_cand=4, n_landmarks=4)
        s.upload_grid(c1.cells, c1.origin, c1.resolution)
        s.upload_world(c1.cells)
        refused(FS_E_INVALID, s.drive, [c1.goals[:2]], [c1.goals[0]], text=NOT_2D)
        np.testing.assert_array_equal(s.read_grid_region(), c1.cells)
    finally:
        s.close()


def test_which_refusal_comes_first(fs):
    """fs_sense and fs_drive check in the same order — the grid, the world, the fan's source, then the drive's own arguments,
    then first_ray: a call that is wrong in two ways is refused with the text of the earlier check"""
    def text(f, *args, **kw):
        with pytest.raises(fs.capi.FsError) as e:
            f(*args, **kw)
        return str(e.value)
    origin, res = (0.0, 0.0, 0.0), 0.1
    flat = np.zeros((1, 16, 16), np.uint8)
    pose = np.array([[0.85, 0.85, 0.0]])
    s = fs.FrontierScorer(device=0)
    try:
        # neither grid nor world: the grid's text
        assert text(s.sense, pose) == f"fitslam_frontier error {FS_E_STATE}: {NO_GRID}"
        assert text(s.drive, [pose], pose) == f"fitslam_frontier error {FS_E_STATE}: {NO_GRID}"
        # no ray parameters, no sensor and a first_ray out of range: the sensor's text
        s.upload_grid(flat, origin, res)
        s.upload_world(flat)
        assert text(s.sense, pose, [10 ** 6]) == f"fitslam_frontier error {FS_E_STATE}: {NO_SENSOR}"
        assert text(s.drive, [pose], pose, [[10 ** 6]]) == f"fitslam_frontier error {FS_E_STATE}: {NO_SENSOR}"
        # a 3-D grid and more robots than a drive takes: the grid's shape is looked at first
        vol = np.zeros((8, 16, 16), np.uint8)
        s.upload_grid(vol, origin, res)
        s.upload_world(vol)
        for R in (65, fs.capi.FS_DRIVE_MAX_ROBOTS + 1):
            assert text(s.drive, [pose] * R, np.repeat(pose, R, axis=0), sensor=EP.PARAMS) == f"fitslam_frontier error {FS_E_INVALID}: {NOT_2D}"
    finally:
        s.close()
