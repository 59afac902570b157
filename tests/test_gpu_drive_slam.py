"""fs_drive_slam on the GPU (fit-slam_amd/csrc/fs_drive_slam.hip) against tests/drive_slam_ref.py and against a twin
built only from calls the library had before it — a host loop per step of fs_trace_segments, fs_sense, fs_sense_landmarks,
fs_score_fim(info_only) and fs_goals_mapped on a second context (drive_slam_ref.drive_slam_by_calls).  Every integer bit for bit,
the whole staged grid, the world cloud's counters and discovered list, the staged cloud byte for byte, the information within the
project's Fisher tolerance of 1e-4 relative and exactly 0 where the twin's is 0.

A stop hangs on a float comparison, so each case's threshold is taken from the TWIN's ungated information (midway between two
stations, `between` of the case) after checking that no twin value lies within 1e-3 relative of it: a precondition on the inputs.

The cases are the table of tests/test_drive_slam_restatement.py; then a staged cloud replaced before the call, a pose with more
occupied voxels than the LDS tier takes, the host waits per call, what the context computes after a drive, the error paths."""
import ctypes

import numpy as np
import pytest

import drive_ref as DR
import drive_slam_ref as DS
import landmark_sense_ref as LR
import sense_ref as SR
import test_drive_restatement as TR
import test_drive_slam_restatement as TS
import test_gpu_explore_episode as EP

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
WORLD, STAGED, CLOUD = TR.WORLD, TR.STAGED, TS.CLOUD
WAITS, CAPACITY, FALLBACKS = 1047, 1048, 1049                           # fs_get_counter
RTOL = 1.0e-4


def _ctx(fs, staged, world, cloud=None, known=None, occlusion=None, fim=DS.FIM):
    s = fs.FrontierScorer(device=0)
    s.set_ray_params(robot_radius=0.15, **EP.PARAMS)
    s.lookup_generate()
    s.set_fim_params(*fim)
    s.set_arrival_limits(4000.0, 0.0)
    s.upload_grid(staged, EP.ORIGIN, EP.RES)
    if world is not None:
        s.upload_world(world)
    if cloud is not None:
        s.upload_world_landmarks(cloud, known)
    if occlusion is not None:
        s.set_occlusion(True, occ=occlusion["occ"], end_margin_m=occlusion["end_margin_m"])
    return s


def _trio(fs, case, cloud=CLOUD):
    """(the driven context, its twin for the host loop, a context whose staged grid is the world)"""
    return (_ctx(fs, STAGED, WORLD, cloud, case["known"], case["occlusion"]), _ctx(fs, STAGED, WORLD, cloud, case["known"], case["occlusion"]),
            _ctx(fs, WORLD, None))


def _kw(case, thr):
    return dict(first_ray=case["first_ray"], lm_sensor=case["lm_sensor"], stop_when_mapped=case["stop_when_mapped"], threshold=thr,
                gate=case["gate"], gate_first_station=case["gate_first_station"])


def _twin_threshold(b, w, case, cloud=CLOUD):
    """the ungated twin drive on b, the threshold its information gives, and b put back as it was"""
    free = DS.drive_slam_by_calls(b, w, case["poses"], case["goals"], **dict(_kw(case, 0.0), gate=False))
    r, hi, lo = case["between"]
    thr = DS.threshold_between(free["information"], free["information"][r][lo], free["information"][r][hi])
    b.upload_grid(STAGED, EP.ORIGIN, EP.RES)
    b.upload_world_landmarks(cloud, case["known"])
    return free, thr


def _same_state(a, b, want=None, what=""):
    np.testing.assert_array_equal(a.read_grid_region(), b.read_grid_region(), err_msg=f"{what} grid")
    wa, wb = a.world_landmarks(), b.world_landmarks()
    assert (wa["m_world"], wa["n_discovered"]) == (wb["m_world"], wb["n_discovered"]), what
    np.testing.assert_array_equal(wa["world_index"], wb["world_index"], err_msg=f"{what} world_index")
    np.testing.assert_array_equal(wa["views"], wb["views"], err_msg=f"{what} views")
    sa, sb = a.staged_cloud(), b.staged_cloud()
    assert (sa["m"], sa["n_chunks"]) == (sb["m"], sb["n_chunks"]), what
    for k in ("soa", "spheres", "perm"):
        assert sa[k].tobytes() == sb[k].tobytes(), f"{what} staged {k}"
    if want is not None:
        np.testing.assert_array_equal(a.read_grid_region(), want["grid"], err_msg=f"{what} grid (restatement)")
        np.testing.assert_array_equal(wa["world_index"], want["world_index"], err_msg=f"{what} world_index (restatement)")
        np.testing.assert_array_equal(wa["views"], want["views"], err_msg=f"{what} views (restatement)")


def _check(fs, oracle, table, case, before=None):
    """one drive_slam on a, the host loop on b, the restatement: all equal.  Returns (a's result, the twin's, the threshold)."""
    a, b, w = _trio(fs, case)
    try:
        free, thr = _twin_threshold(b, w, case)
        twin = DS.drive_slam_by_calls(b, w, case["poses"], case["goals"], **_kw(case, thr))
        if before is not None:
            before(a)
        got = a.drive_slam(case["poses"], case["goals"], **_kw(case, thr))
        print("drive_slam:", list(got["status"]), list(got["reached"]), [list(np.round(v, 3)) for v in got["information"]],
              [list(v) for v in got["voxels"]], got["n_new"], got["n_discovered"], "threshold", thr)
        print("twin:      ", list(twin["status"]), list(twin["reached"]), [list(np.round(v, 3)) for v in twin["information"]])
        DS.assert_same_slam(got, twin, "host loop", RTOL)
        want = TS.run(oracle, table, case, threshold=thr)
        DS.assert_same_slam(got, want, "restatement", RTOL)
        _same_state(a, b, want)
        return got, twin, thr
    finally:
        a.close(); b.close(); w.close()


def test_no_landmark_of_the_cloud_is_borderline_for_any_pose(oracle):
    """the restatement's predicate is float64, the device's float32: no (pose, landmark) pair of the table may sit on a boundary"""
    poses = np.concatenate([p for c in TS.cases().values() for p in c["poses"]])
    assert not LR.borderline(oracle, poses, CLOUD, [(2.0, 1.0), (1.0, 1.0), DS.FIM]).any()


@pytest.mark.parametrize("name", sorted(TS.TABLE))
def test_table_cases_equal_the_host_loop_and_the_restatement(fs, oracle, ref_table, name):
    case = TS.cases()[name]
    got, twin, thr = _check(fs, oracle, ref_table, case)
    status, reached, voxels, in_view, n_new, n_disc, n_seen, n_revealed = TS.TABLE[name]
    assert (list(got["status"]), list(got["reached"])) == (status, reached)                 # the table's figures
    assert [list(v) for v in got["voxels"]] == voxels and [list(v) for v in got["in_view"]] == in_view
    assert (got["n_new"], got["n_discovered"], got["n_seen"], got["n_revealed"]) == (n_new, n_disc, n_seen, n_revealed)


def test_staged_cloud_replaced_before_the_call(fs, oracle, ref_table):
    """fs_upload_landmarks in between leaves the world cloud alone: the gate still reads the discovered set, and afterwards the
    staged cloud is that set — also when the drive discovers nothing new"""
    case = TS.cases()["unsafe"]
    junk = np.random.default_rng(5).uniform(-2.0, 2.0, size=(70, 3)).astype(np.float32)
    _check(fs, oracle, ref_table, case, before=lambda a: a.upload_landmarks(junk))
    a = _ctx(fs, STAGED, WORLD, CLOUD)
    try:
        first = a.drive_slam(case["poses"], case["goals"], gate=False)
        staged = a.staged_cloud()
        a.upload_landmarks(junk)
        assert a.staged_cloud()["m"] == 70
        a.upload_grid(STAGED, EP.ORIGIN, EP.RES)
        again = a.drive_slam(case["poses"], case["goals"], gate=False)
        assert (again["n_new"], again["n_discovered"]) == (0, first["n_discovered"])
        now = a.staged_cloud()
        assert now["m"] == first["n_discovered"] and all(now[k].tobytes() == staged[k].tobytes() for k in ("soa", "spheres", "perm"))
        # everything was discovered before the second drive began: every station sees the whole discovered set
        assert all((x >= y - RTOL * y).all() for x, y in zip(again["information"], first["information"]))
        np.testing.assert_array_equal(np.concatenate(again["in_view"]), np.concatenate(first["in_view"]))
    finally:
        a.close()


def test_more_voxels_than_the_lds_tier_takes(fs, oracle, ref_table):
    """60 000 landmarks uniform in a 14 m ball around the station, all known, cone off: about 28 000 occupied voxels in the table's
    box, more than the LDS tier of the gate kernel holds — the fallback tier scores the pose, and scores it right"""
    rng = np.random.default_rng(17)
    centre = np.array(DR.cell_centre(20, 20, EP.ORIGIN, EP.RES))
    v = rng.normal(size=(60000, 3))
    ball = (centre + v / np.linalg.norm(v, axis=1)[:, None] * (14.0 * rng.uniform(0.0, 1.0, size=(60000, 1)) ** (1.0 / 3.0))).astype(np.float32)
    fim = (14.0, 4.0)
    poses = DS.pose_rows([centre, DR.cell_centre(25, 20, EP.ORIGIN, EP.RES)], 0.3)
    ball = LR.drop_borderline(oracle, poses, ball, [fim])
    want = oracle.pose_information(ref_table, ball, poses, fim[0], fim[1])
    a = _ctx(fs, STAGED, WORLD, ball, np.ones(ball.shape[0], bool), fim=fim)
    t = _ctx(fs, STAGED, None, fim=fim)
    try:
        capacity = a.get_counter(CAPACITY)
        print("occupied voxels (oracle):", list(want["n_voxels"]), "LDS tier capacity:", capacity)
        assert 20000 < want["n_voxels"].min() and capacity < want["n_voxels"].min()
        assert a.get_counter(FALLBACKS, reset=True) == 0
        got = a.drive_slam([poses], [DR.cell_centre(90, 90, EP.ORIGIN, EP.RES)],
                           lm_sensor=dict(max_dist=14.0, max_angle=4.0, line_of_sight=0, min_views=1), gate=False)
        assert a.get_counter(FALLBACKS) > 0
        t.upload_landmarks(ball)
        twin = t.score_fim(poses, info_only=True)
        print("information:", list(got["information"][0]), "twin:", list(twin["info_ref"]), "oracle:", list(want["info_f64"]))
        assert list(got["status"]) == [DR.ARRIVED] and list(got["reached"]) == [1]
        np.testing.assert_array_equal(got["voxels"][0], want["n_voxels"])
        np.testing.assert_array_equal(got["voxels"][0], twin["n_voxels"])
        np.testing.assert_array_equal(got["in_view"][0], want["n_visible"])
        np.testing.assert_allclose(got["information"][0], twin["info_ref"], rtol=RTOL, atol=0.0)
        np.testing.assert_allclose(got["information"][0], want["info_f64"], rtol=RTOL, atol=0.0)
        assert (got["n_new"], got["n_discovered"]) == (0, ball.shape[0])
    finally:
        a.close(); t.close()


def test_host_waits_do_not_grow_with_stations_or_robots(fs):
    case = TS.cases()["gate_off"]
    a = _ctx(fs, STAGED, WORLD, CLOUD)
    try:
        waits = []
        for poses, goals in (([case["poses"][0][:2]], case["goals"][:1]), ([case["poses"][0]], case["goals"][:1]), (case["poses"], case["goals"])):
            a.upload_grid(STAGED, EP.ORIGIN, EP.RES)
            a.upload_world_landmarks(CLOUD)
            r = a.drive_slam(poses, goals, gate=False)
            assert r["n_new"] > 0
            waits.append(a.get_counter(WAITS))
        assert waits == [2, 2, 2]                                        # the drive's one wait, and the one restaging's
        r = a.drive_slam(case["poses"], case["goals"], gate=False)       # nothing new, the staged cloud is the discovered set: no restaging
        assert r["n_new"] == 0 and a.get_counter(WAITS) == 1
    finally:
        a.close()


def test_context_after_a_drive_equals_a_fresh_snapshot(fs):
    case = TS.cases()["gate_off"]
    a = _ctx(fs, STAGED, WORLD, CLOUD)
    b = fs.FrontierScorer(device=0)
    try:
        a.drive_slam(case["poses"], case["goals"], lm_sensor=case["lm_sensor"], gate=False)
        merged, idx = a.read_grid_region(), a.world_landmarks()["world_index"]
        assert idx.shape[0] == 296
        b.set_ray_params(robot_radius=0.15, **EP.PARAMS)
        b.lookup_generate()
        b.set_fim_params(*DS.FIM)
        b.set_arrival_limits(4000.0, 0.0)
        b.set_option("cloud.order", 2)
        b.upload_grid(merged, EP.ORIGIN, EP.RES)
        b.upload_landmarks(CLOUD[idx])
        sa, sb = a.staged_cloud(), b.staged_cloud()
        assert all(sa[k].tobytes() == sb[k].tobytes() for k in ("soa", "spheres", "perm"))
        goals = np.concatenate([p[:, :3] for p in case["poses"]])
        ra, rb = a.score_candidates(goals), b.score_candidates(goals)
        for f in ra.dtype.names:
            if f in ("info_ref", "trace", "logdet"):
                np.testing.assert_allclose(ra[f], rb[f], rtol=1.0e-5, err_msg=f)         # (the Fisher float sums are not bit-stable from call to call)
            else:
                assert ra[f].tobytes() == rb[f].tobytes(), f
        assert (ra["n_visible"] > 0).any()
        poses = np.concatenate(case["poses"])
        (oa, ea), (ob, eb) = a.landmarks_in_view(poses), b.landmarks_in_view(poses)
        np.testing.assert_array_equal(oa, ob)
        assert ea.tobytes() == eb.tobytes() and oa[-1] > 0
        assert a.grid_census() == b.grid_census() == SR.census_ref(merged)
    finally:
        a.close(); b.close()


def test_refusals_in_their_order_leave_everything_alone(fs):
    case = TS.cases()["unsafe"]
    E = fs.capi
    p7 = np.ascontiguousarray(np.concatenate(case["poses"]))
    goals = np.ascontiguousarray(case["goals"], dtype=np.float64)
    n_st = np.array([p.shape[0] for p in case["poses"]], dtype=np.int32)
    T = p7.shape[0]
    ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    s = fs.FrontierScorer(device=0)
    try:
        def raw(n_st=n_st, lm=None, prm=None, first=None):
            ints = [np.full(n, 77, np.int32) for n in (2, 2, T, T, T, T, 6)]
            info = np.full(T, 77.0, np.float32)
            c64, c32 = [ctypes.c_int64(77), ctypes.c_int64(77)], [ctypes.c_int32(77), ctypes.c_int32(77)]
            rc = s._L.fs_drive_slam(s._h, 2, ptr(p7), ptr(np.asarray(n_st, dtype=np.int32)), None if first is None else ptr(first), ptr(goals), None,
                                    None if lm is None else ctypes.byref(lm), None if prm is None else ctypes.byref(prm), ptr(ints[0]),
                                    ptr(ints[1]), ptr(ints[2]), ptr(ints[3]), ptr(info), ptr(ints[4]), ptr(ints[5]), ctypes.byref(c64[0]),
                                    ctypes.byref(c64[1]), ptr(ints[6]), ctypes.byref(c32[0]), ctypes.byref(c32[1]))
            assert all((o == 77).all() for o in ints) and (info == 77.0).all() and all(v.value == 77 for v in c64 + c32)
            return rc, s._L.fs_last_error(s._h).decode()
        # 1. fs_drive's refusals come first, in fs_drive's order
        assert raw() == (FS_E_STATE, "fs_upload_grid has not been called")
        s.upload_grid(STAGED, EP.ORIGIN, EP.RES)
        assert raw() == (FS_E_STATE, "fs_upload_world has not been called")
        s.upload_world(WORLD)
        assert raw() == (FS_E_STATE, "fs_set_ray_params has not been called and no sensor is given")
        s.set_ray_params(robot_radius=0.15, **EP.PARAMS)
        bad_gate = E.DriveSlamParamsC(253, 254, 1, 2, 550.0, 1)
        assert raw(n_st=[13, 0], prm=bad_gate)[0] == FS_E_INVALID and "every robot needs a station" in raw(n_st=[13, 0], prm=bad_gate)[1]
        first = np.full(T, 10 ** 6, np.int32)
        assert "first_ray[0]" in raw(first=first, prm=bad_gate)[1]
        # 2. no world cloud, 3. no lookup table — before the sensor and the gate's parameters are looked at
        assert raw(prm=bad_gate) == (FS_E_STATE, "fs_upload_world_landmarks has not been called")
        s.upload_world_landmarks(CLOUD)
        assert raw(prm=bad_gate) == (FS_E_STATE, "no lookup table: call fs_lookup_generate / fs_lookup_load")
        s.lookup_generate()
        s.set_fim_params(*DS.FIM)
        # 4. the landmark sensor as fs_sense_landmarks refuses it, then gate, gate_first_station, the threshold
        assert raw(lm=E.LandmarkSensorC(2.0, 1.0, 1, 0, 254, 254, 0.3), prm=bad_gate) == (FS_E_INVALID, "sensor: min_views must be at least 1")
        assert raw(lm=E.LandmarkSensorC(-2.0, 1.0, 1, 1, 254, 254, 0.3))[0] == FS_E_INVALID
        assert raw(lm=E.LandmarkSensorC(2.0, 1.0, 2, 1, 254, 254, 0.3))[0] == FS_E_INVALID
        assert raw(prm=bad_gate) == (FS_E_INVALID, "gate must be 0 or 1")
        assert raw(prm=E.DriveSlamParamsC(253, 254, 1, 1, 550.0, -1)) == (FS_E_INVALID, "gate_first_station must not be negative")
        for thr in (float("nan"), float("inf"), -float("inf")):
            assert raw(prm=E.DriveSlamParamsC(253, 254, 1, 1, thr, 1)) == (FS_E_INVALID, "information_threshold must be finite")
        # nothing was touched by any of them: the map, the counters, the flags, the staged cloud
        np.testing.assert_array_equal(s.read_grid_region(), STAGED)
        wl = s.world_landmarks()
        assert wl["n_discovered"] == 0 and not wl["views"].any() and s.staged_cloud()["m"] == 0
        # no robots: a no-op that reports the standing total
        r = s.drive_slam([], np.zeros((0, 3)))
        assert (r["n_seen"], r["n_revealed"], r["window"], r["n_new"], r["n_discovered"], r["information"]) == (0, 0, (0,) * 6, 0, 0, [])
        # the defaults: threshold 550, gate 1 from station 1 — nothing in this room comes near 550
        r = s.drive_slam(case["poses"], case["goals"])
        assert list(r["status"]) == [E.FS_DRIVE_UNSAFE] * 2 and list(r["reached"]) == [1, 1] and r["n_discovered"] > 0
        r0 = s.drive_slam([], np.zeros((0, 3)))
        assert (r0["n_new"], r0["n_discovered"]) == (0, r["n_discovered"])
        # a 3-D grid is refused as fs_drive refuses it
        c1 = fs.synth.make_workload("C1", n_cand=4, n_landmarks=4)
        s.upload_grid(c1.cells, c1.origin, c1.resolution)
        s.upload_world(c1.cells)
        with pytest.raises(E.FsError) as e:
            s.drive_slam([DS.pose_rows(c1.goals[:2], 0.0)], [c1.goals[0]])
        assert e.value.code == FS_E_INVALID and "2-D costmap" in str(e.value)
    finally:
        s.close()
