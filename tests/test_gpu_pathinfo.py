"""fs_plan_paths_information on the GPU: the plan against fs_plan_paths and the way points against the CPU
restatement of setPlanForFrontier's sampling loop (tests/pathinfo_ref/pathinfo_ref.cpp) bit for bit, every way point's value
against the oracle within the project's 1e-4 relative bar, the per-frontier columns against a recomputation from the call's own
dump bit for bit and against the oracle's threshold decision, the de-duplication against scoring every way point, and the state
the call leaves behind."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pathinfo_maps as M
import pathinfo_ref as P
import planner_ref as R

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = M.RES
REL = 1e-4                       # info_ref against the oracle's fp64 sum
QUAT_ABS = 1e-12                 # device against host libm (atan2, sin, cos): a few ulp of a double
VIS = [(14.0, 1.0), (14.0, 4.0)]  # the build's cone and the request the reference itself makes (cone off)
N_LANDMARKS = 20_000
ORACLE_SAMPLE = 3000             # way points checked against the oracle where a list has more
ORACLE_SAMPLE_SEED = 20261
ORACLE_SAMPLE_PATHS = 150        # paths whose first and last way point the sample always holds (>= 100)

MAP_MAKERS = {
    "REF2D": M.ref2d,
    "plan_128": lambda: M.floor_plan(5001, 128),
    "plan_256": lambda: M.floor_plan(5002, 256),
    "plan_512": lambda: M.floor_plan(5003, 512),
    "non_square": lambda: np.ascontiguousarray(M.floor_plan(5004, 192)[:150, :]),
    "spiral_512": lambda: np.ascontiguousarray(R.spiral_map(512)[0]),
}


@functools.lru_cache(maxsize=None)
def _map(name):
    """(cells, origin, landmarks [20 000][3]: on obstacle cells, heights U(0, 2.5 m), as REF2D's)"""
    if name == "REF2D":
        w = fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=N_LANDMARKS)
        return np.ascontiguousarray(w.cells[0]), tuple(w.origin), w.landmarks
    cells = MAP_MAKERS[name]()
    origin = M.origin_of(cells)
    rng = np.random.Generator(np.random.PCG64(977))
    lm = fsmod.synth._landmarks(rng, cells[None], origin, RES, N_LANDMARKS)
    lm[:, 2] = rng.uniform(0.0, 2.5, size=lm.shape[0]).astype(np.float32)
    return cells, origin, lm


@functools.lru_cache(maxsize=None)
def _robots(name):
    """two robots that are not shut in: (pose7, allow_unknown)"""
    cells, origin, _ = _map(name)
    if name == "spiral_512":
        _, centre, outer = R.spiral_map(512)
        return ((R.robot_pose(origin, RES, centre[0], centre[1], 0.3), 1), (R.robot_pose(origin, RES, outer[0], outer[1], -2.0), 0))
    a = R.well_placed_robot(cells, np.random.default_rng(7))
    b = R.well_placed_robot(cells, np.random.default_rng(8))
    return ((R.robot_pose(origin, RES, a[0], a[1], 0.3), 1), (R.robot_pose(origin, RES, b[0], b[1], -2.0), 0))


def _new_scorer(name, stage_fim=True):
    cells, origin, lm = _map(name)
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    if stage_fim:
        sc.upload_landmarks(lm)
        sc.lookup_generate()
        sc.set_fim_params(*VIS[0])
    return sc


@pytest.fixture(scope="module")
def scorers():
    """one staged context per map, kept for the module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _new_scorer(name)
        return made[name]
    yield get
    for sc in made.values():
        sc.close()


def _columns_from_values(offset, values, threshold):
    """info_mean, info_min, first_unsafe as the header defines them, from a value dump: the fp64 sum of the positive values in
    way-point order (a sequential loop: numpy's sum is pairwise) over the number of way points"""
    n = offset.size - 1
    mean, mn, unsafe = np.zeros(n), np.full(n, np.inf, dtype=np.float32), np.full(n, -1, dtype=np.int32)
    for f in range(n):
        v = values[offset[f]:offset[f + 1]]
        if v.size == 0:
            continue
        s = 0.0
        for x in v:
            if x > 0:
                s += float(x)
        mean[f] = s / v.size
        mn[f] = v.min()
        bad = np.nonzero(~(v.astype(np.float64) > threshold))[0]
        if bad.size:
            unsafe[f] = bad[0]
    return mean, mn, unsafe


def _oracle_values(oracle, table, landmarks, poses, vis):
    """the oracle's fp64 scalar of every pose; equal poses are scored once"""
    uniq, inverse = np.unique(poses, axis=0, return_inverse=True)
    want = oracle.pose_information(table, landmarks, uniq, vis[0], vis[1], n_threads=16)["info_f64"]
    return want[inverse.reshape(-1)]


def _within_bar(got, want):
    scale = np.maximum(np.abs(want), 1e-6)
    return float(np.max(np.abs(got.astype(np.float64) - want) / scale)) if want.size else 0.0


def _oracle_sample(offset, total):
    """every way point, or the stated seeded sample that holds the first and the last way point of ORACLE_SAMPLE_PATHS paths"""
    if total <= ORACLE_SAMPLE:
        return np.arange(total)
    rng = np.random.default_rng(ORACLE_SAMPLE_SEED)
    with_wp = np.nonzero(np.diff(offset) > 0)[0]
    paths = rng.choice(with_wp, size=min(ORACLE_SAMPLE_PATHS, with_wp.size), replace=False)
    assert paths.size >= 100
    ends = np.unique(np.concatenate([offset[paths], offset[paths + 1] - 1]))
    rest = np.setdiff1d(np.arange(total), ends)
    pick = np.concatenate([ends, rng.choice(rest, size=ORACLE_SAMPLE - ends.size, replace=False)])
    assert pick.size == ORACLE_SAMPLE and np.isin(offset[paths], pick).all() and np.isin(offset[paths + 1] - 1, pick).all()
    return np.sort(pick)


NAMES = list(MAP_MAKERS)


@pytest.mark.parametrize("n", [1, 50, 2000])
@pytest.mark.parametrize("name", NAMES)
def test_plan_way_points_and_values(oracle, ref_table, scorers, name, n):
    cells, origin, lm = _map(name)
    sc = scorers(name)
    checked = 0
    for r, (pose, allow) in enumerate(_robots(name)):
        goals, ach_in = M.goals(cells, origin, 11 + n + r, n)
        if n == 1:
            ach_in = None                      # (the one goal is planned)
        ref = P.waypoints(cells, origin, RES, pose, goals, achievable_in=ach_in, allow_unknown=allow)
        for vis in VIS:
            sc.set_fim_params(*vis)
            got = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, want_waypoints=True)
            plan = sc.plan_paths(pose, goals, achievable_in=ach_in, allow_unknown=allow)
            tag = (name, n, r, vis)
            # the plan is fs_plan_paths' own
            for k in ("path_length", "path_length_m", "path_heading", "achievable"):
                assert got[k].tobytes() == plan[k].tobytes(), (tag, k)
            # counts, offsets and positions are the restatement's, bit for bit
            assert got["path_length"].tobytes() == ref["path_length"].tobytes(), tag
            assert got["n_waypoints"].tobytes() == ref["count"].tobytes(), tag
            assert got["waypoint_offset"].tobytes() == ref["offset"].tobytes(), tag
            total = int(ref["offset"][-1])
            p7 = got["waypoint_pose7"]
            assert p7.shape == (total, 7) and got["waypoint_info"].shape == (total,)
            assert sc.get_counter(1024) == total and 0 <= sc.get_counter(1025) <= total
            assert p7[:, :2].tobytes() == np.ascontiguousarray(ref["xyyaw"][:, :2]).tobytes(), tag
            assert (p7[:, 2] == 0.0).all() and (p7[:, 3:5] == 0.0).all()
            if total:
                assert np.max(np.abs(p7[:, 3:] - P.yaw_to_quat(ref["xyyaw"][:, 2]))) <= QUAT_ABS, tag
            # the values: the oracle at the dumped poses
            pick = _oracle_sample(got["waypoint_offset"], total)
            want = _oracle_values(oracle, ref_table, lm, p7[pick], vis)
            err = _within_bar(got["waypoint_info"][pick], want)
            print(f"{tag}: {total} way points, {sc.get_counter(1025)} distinct poses, {pick.size} against the oracle, max rel err {err:.3g}")
            assert err <= REL, (tag, err)
            checked += pick.size
            # the per-frontier columns: a pure function of the dumped values
            mean, mn, unsafe = _columns_from_values(got["waypoint_offset"], got["waypoint_info"], 550.0)
            assert got["info_mean"].tobytes() == mean.tobytes(), tag
            assert got["info_min"].tobytes() == mn.tobytes(), tag
            assert got["first_unsafe"].tobytes() == unsafe.tobytes(), tag
            none = got["n_waypoints"] == 0
            assert (got["info_mean"][none] == 0.0).all() and np.isposinf(got["info_min"][none]).all() and (got["first_unsafe"][none] == -1).all()
            assert (got["n_waypoints"][got["achievable"] == 0] == 0).all()
            # the same call without the dump returns the same columns
            lean = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow)
            assert "waypoint_info" not in lean
            for k in ("n_waypoints", "achievable", "path_length"):
                assert lean[k].tobytes() == got[k].tobytes(), (tag, k)
            np.testing.assert_allclose(lean["info_mean"], got["info_mean"], rtol=5e-6, atol=1e-6)
    sc.set_fim_params(*VIS[0])
    if n >= 50:
        assert checked > 0, "no way point on any path of the list"


@pytest.mark.parametrize("n", [50, 200])
@pytest.mark.parametrize("vis", VIS)
def test_first_unsafe_against_the_oracle(oracle, ref_table, scorers, n, vis):
    """The threshold sits in the widest gap of the central 40 % of the sorted oracle values (at least 1e-3 relative wide, ten
    times the bar, asserted): then first_unsafe is the oracle's decision on every frontier, none left out.  Measured on the CPU
    for these lists (REF2D, 20 000 landmarks): 0.5 % to 4 % relative."""
    cells, origin, lm = _map("REF2D")
    sc = scorers("REF2D")
    sc.set_fim_params(*vis)
    try:
        for r, (pose, allow) in enumerate(_robots("REF2D")):
            goals, ach_in = M.goals(cells, origin, 11 + n + r, n)
            dump = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, want_waypoints=True)
            off = dump["waypoint_offset"]
            want = _oracle_values(oracle, ref_table, lm, dump["waypoint_pose7"], vis)
            assert want.size > 300
            v = np.sort(want)
            mid = v[int(0.3 * v.size):int(0.7 * v.size)]
            i = int(np.argmax(np.diff(mid)))
            threshold = 0.5 * (mid[i] + mid[i + 1])
            gap = (mid[i + 1] - mid[i]) / threshold
            print(f"REF2D n={n} robot {r} vis {vis}: threshold {threshold:.6g}, gap {gap:.3g} relative")
            assert gap >= 1e-3, gap
            got = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, fi_threshold=threshold)
            _, _, unsafe = _columns_from_values(off, want, threshold)
            assert got["first_unsafe"].tobytes() == unsafe.tobytes(), (n, r, vis, np.nonzero(got["first_unsafe"] != unsafe)[0][:8])
            assert (unsafe >= 0).any() and (unsafe == -1).any()
    finally:
        sc.set_fim_params(*VIS[0])


def test_deduplication_changes_no_result(scorers):
    """"pathinfo.dedup" 0 scores every way point, 1 one pose per distinct (from cell, to cell): the integers are identical, the
    values agree within the bar (bit-equality is recorded in DESIGN.md 4.15, not asserted), and at 2 000 goals on REF2D the
    paths share enough of their trunks for the distinct poses to be a fraction of the way points."""
    cells, origin, _ = _map("REF2D")
    sc = scorers("REF2D")
    pose, allow = _robots("REF2D")[0]
    goals, ach_in = M.goals(cells, origin, 2011, 2000)
    out, counters = {}, {}
    try:
        for dedup in (1, 0):
            sc.set_option("pathinfo.dedup", dedup)
            out[dedup] = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, want_waypoints=True)
            counters[dedup] = (sc.get_counter(1024), sc.get_counter(1025))
    finally:
        sc.set_option("pathinfo.dedup", 1)
    for k in ("n_waypoints", "first_unsafe", "achievable", "waypoint_offset", "path_length", "path_length_m", "path_heading", "waypoint_pose7"):
        assert out[1][k].tobytes() == out[0][k].tobytes(), k
    assert _within_bar(out[1]["waypoint_info"], out[0]["waypoint_info"].astype(np.float64)) <= REL
    np.testing.assert_allclose(out[1]["info_mean"], out[0]["info_mean"], rtol=REL)
    np.testing.assert_allclose(out[1]["info_min"], out[0]["info_min"], rtol=REL, atol=1e-6)
    same = out[1]["waypoint_info"].tobytes() == out[0]["waypoint_info"].tobytes()
    print(f"dedup 1 / 0 counters (way points, poses scored): {counters}; values bit-equal: {same}")
    assert counters[0][0] == counters[0][1] == counters[1][0] > 20_000
    assert counters[1][1] < counters[1][0] // 2
    # equal (from cell, to cell) are equal poses (two keys can still share a pose: the same cell, the same bearing)
    assert np.unique(out[1]["waypoint_pose7"], axis=0).shape[0] <= counters[1][1]


@pytest.mark.parametrize("n", [50, 2000])
def test_dumped_poses_through_score_fim(scorers, n):
    """A pose of the dump handed to fs_score_fim makes the same pose record: the values agree within the bar (which lane adds which
    term differs from launch to launch: last bits)."""
    cells, origin, _ = _map("REF2D")
    sc = scorers("REF2D")
    pose, allow = _robots("REF2D")[1]
    goals, ach_in = M.goals(cells, origin, 77 + n, n)
    got = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, want_waypoints=True)
    assert got["waypoint_info"].size > 100
    again = sc.score_fim(got["waypoint_pose7"], info_only=True)["info_ref"]
    assert _within_bar(got["waypoint_info"], again.astype(np.float64)) <= REL


def test_every_point_and_no_lookahead_on_the_gpu(scorers):
    """sample_distance 0 (s = 0): every path point is a way point — with 1 200 goals more than the call makes room for unseen, so the
    total is read first; lookahead 0: every pose looks along +x.  Against the restatement, and the values against fs_score_fim."""
    name = "plan_128"
    cells, origin, _ = _map(name)
    sc = scorers(name)
    pose, allow = _robots(name)[0]
    for n, look in ((50, 0), (1200, 3)):
        goals, ach_in = M.goals(cells, origin, 311 + n, n)
        ref = P.waypoints(cells, origin, RES, pose, goals, achievable_in=ach_in, allow_unknown=allow, sample_distance=0.0, lookahead=look)
        got = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, sample_distance=0.0, lookahead=look,
                                        want_waypoints=True)
        assert got["n_waypoints"].tobytes() == ref["count"].tobytes() and got["waypoint_offset"].tobytes() == ref["offset"].tobytes()
        planned = got["achievable"] == 1
        assert planned.any() and (got["n_waypoints"][planned] == got["path_length"][planned]).all()
        p7 = got["waypoint_pose7"]
        assert p7[:, :2].tobytes() == np.ascontiguousarray(ref["xyyaw"][:, :2]).tobytes()
        assert np.max(np.abs(p7[:, 3:] - P.yaw_to_quat(ref["xyyaw"][:, 2]))) <= QUAT_ABS
        if look == 0:
            assert (p7[:, 3:] == np.array([0.0, 0.0, 0.0, 1.0])).all()
        pick = np.random.default_rng(5).choice(p7.shape[0], size=min(p7.shape[0], 4000), replace=False)
        again = sc.score_fim(p7[pick], info_only=True)["info_ref"]
        assert _within_bar(got["waypoint_info"][pick], again.astype(np.float64)) <= REL
        mean, mn, unsafe = _columns_from_values(got["waypoint_offset"], got["waypoint_info"], 550.0)
        assert got["info_mean"].tobytes() == mean.tobytes() and got["info_min"].tobytes() == mn.tobytes()
        assert got["first_unsafe"].tobytes() == unsafe.tobytes()


def test_first_call_of_a_fresh_context_and_the_field_cache(oracle, ref_table):
    """The call is the first thing a fresh context does after staging (no plan, no scoring call has sized any buffer); afterwards
    fs_plan_paths and fs_navfn_potential return what a context that never made the call returns, from the same cached field."""
    name = "plan_256"
    cells, origin, lm = _map(name)
    pose, allow = _robots(name)[0]
    goals, ach_in = M.goals(cells, origin, 909, 300)
    sc, other = _new_scorer(name), _new_scorer(name, stage_fim=False)
    try:
        got = sc.plan_paths_information(pose, goals, achievable_in=ach_in, allow_unknown=allow, want_waypoints=True)
        assert sc.get_counter(1002) == 1
        ref = P.waypoints(cells, origin, RES, pose, goals, achievable_in=ach_in, allow_unknown=allow)
        assert got["waypoint_offset"].tobytes() == ref["offset"].tobytes() and ref["offset"][-1] > 300
        want = _oracle_values(oracle, ref_table, lm, got["waypoint_pose7"], VIS[0])
        assert _within_bar(got["waypoint_info"], want) <= REL
        mean, mn, unsafe = _columns_from_values(got["waypoint_offset"], got["waypoint_info"], 550.0)
        assert got["info_mean"].tobytes() == mean.tobytes() and got["first_unsafe"].tobytes() == unsafe.tobytes()
        plan, field = sc.plan_paths(pose, goals, achievable_in=ach_in, allow_unknown=allow), sc.navfn_potential(pose, allow_unknown=allow)
        assert sc.get_counter(1002) == 1                      # the field the call built is the one both reuse
        want_plan, want_field = other.plan_paths(pose, goals, achievable_in=ach_in, allow_unknown=allow), other.navfn_potential(pose, allow_unknown=allow)
        for k in want_plan:
            assert plan[k].tobytes() == want_plan[k].tobytes() == got[k].tobytes(), k
        assert field.tobytes() == want_field.tobytes()
        # a longer list on the same context: every buffer grows
        goals2, ach2 = M.goals(cells, origin, 910, 2500)
        big = sc.plan_paths_information(pose, goals2, achievable_in=ach2, allow_unknown=allow, want_waypoints=True)
        ref2 = P.waypoints(cells, origin, RES, pose, goals2, achievable_in=ach2, allow_unknown=allow)
        assert big["waypoint_offset"].tobytes() == ref2["offset"].tobytes()
        again = sc.score_fim(big["waypoint_pose7"], info_only=True)["info_ref"]
        assert _within_bar(big["waypoint_info"], again.astype(np.float64)) <= REL
        assert sc.get_counter(1002) == 1
    finally:
        sc.close()
        other.close()


def _raw_call(sc, pose, goals, room, prm=None):
    """the C entry point itself, with a dump of `room` way points: (rc, n_total, offsets)"""
    n = goals.shape[0]
    p = (C.c_double * 7)(*[float(v) for v in pose])
    cols = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n),
            np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)]
    total = C.c_int64(-7)
    off = np.full(n + 1, -7, dtype=np.int32)
    poses, info = np.zeros((max(room, 1), 7)), np.zeros(max(room, 1), dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = sc._L.fs_plan_paths_information(sc._h, C.byref(p), 1, n, vp(goals), None, C.byref(prm) if prm is not None else None,
                                         *[vp(c) for c in cols], room, C.byref(total), vp(off), vp(poses), vp(info))
    return rc, total.value, off, cols


def test_edges_and_refusals(scorers):
    name = "plan_128"
    cells, origin, _ = _map(name)
    sc = scorers(name)
    pose, allow = _robots(name)[0]
    goals, _ = M.goals(cells, origin, 3, 40)
    E = fsmod.capi
    # the robot off the map: nothing is planned, nothing is sampled
    off_map = np.array([origin[0] - 0.5, origin[1] + 1.0, 0, 0, 0, 0, 1.0])
    got = sc.plan_paths_information(off_map, goals, want_waypoints=True)
    assert not got["achievable"].any() and (got["path_length"] == R.DBL_MAX).all()
    assert (got["n_waypoints"] == 0).all() and (got["info_mean"] == 0.0).all() and np.isposinf(got["info_min"]).all()
    assert (got["first_unsafe"] == -1).all() and (got["waypoint_offset"] == 0).all() and got["waypoint_info"].size == 0
    # an empty list
    got = sc.plan_paths_information(pose, np.zeros((0, 3)), want_waypoints=True)
    assert got["n_waypoints"].size == 0 and got["waypoint_offset"].tolist() == [0] and got["waypoint_pose7"].shape == (0, 7)
    # NULL parameters are the defaults
    full = sc.plan_paths_information(pose, goals, allow_unknown=True, want_waypoints=True)
    total = int(full["waypoint_offset"][-1])
    assert total > 10
    rc, n_total, off, cols = _raw_call(sc, pose, goals, total)
    assert rc == E.FS_OK and n_total == total and off.tobytes() == full["waypoint_offset"].tobytes()
    assert cols[4].tobytes() == full["n_waypoints"].tobytes() and cols[7].tobytes() == full["first_unsafe"].tobytes()
    # more way points than the dump has room for: FS_E_RANGE, the total reported
    rc, n_total, off, _ = _raw_call(sc, pose, goals, total - 1)
    assert rc == E.FS_E_RANGE and n_total == total
    rc, n_total, _, _ = _raw_call(sc, pose, goals, 0)
    assert rc == E.FS_E_RANGE and n_total == total
    # a dump with a pointer missing
    p = (C.c_double * 7)(*[float(v) for v in pose])
    z = np.zeros(64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cnt = C.c_int64()
    assert sc._L.fs_plan_paths_information(sc._h, C.byref(p), 1, 1, vp(goals), None, None, vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z),
                                           8, C.byref(cnt), None, None, None) == E.FS_E_INVALID
    # parameters
    for kw in (dict(sample_distance=float("nan")), dict(sample_distance=-0.1), dict(lookahead=-1), dict(fi_threshold=float("inf")),
               dict(fi_threshold=float("nan"))):
        with pytest.raises(fsmod.FsError) as e:
            sc.plan_paths_information(pose, goals, **kw)
        assert e.value.code == E.FS_E_INVALID, kw
    # a sample distance no path is as long as: no way point anywhere (inf / resolution is beyond the int range: the same)
    for sd in (1.0e6, float("inf")):
        got = sc.plan_paths_information(pose, goals, allow_unknown=True, sample_distance=sd, want_waypoints=True)
        assert got["achievable"].any() and (got["n_waypoints"] == 0).all() and got["waypoint_offset"].tolist() == [0] * 41
    with pytest.raises(ValueError):
        sc.plan_paths_information(pose, goals, achievable_in=[1, 1])
    # what fs_plan_paths and fs_score_fim refuse, with their codes
    bare = fsmod.FrontierScorer(device=0)
    try:
        with pytest.raises(fsmod.FsError) as e:
            bare.plan_paths_information(pose, goals)                                  # no grid
        assert e.value.code == E.FS_E_STATE
        bare.upload_grid(cells[None], origin, RES)
        with pytest.raises(fsmod.FsError) as e:
            bare.plan_paths_information(pose, goals)                                  # no landmarks
        assert e.value.code == E.FS_E_STATE
        bare.upload_landmarks(_map(name)[2])
        with pytest.raises(fsmod.FsError) as e:
            bare.plan_paths_information(pose, goals)                                  # no lookup table
        assert e.value.code == E.FS_E_STATE
        bare.lookup_generate()
        assert bare.plan_paths_information(pose, goals, allow_unknown=True)["n_waypoints"].tobytes() == full["n_waypoints"].tobytes()
        bare.upload_grid(np.zeros((2, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError) as e:
            bare.plan_paths_information(R.robot_pose((0, 0, 0), RES, 3, 3), np.zeros((1, 3)) + 0.3)   # a 3-D grid
        assert e.value.code == E.FS_E_INVALID
    finally:
        bare.close()
