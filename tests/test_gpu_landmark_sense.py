"""fs_upload_world_landmarks / fs_sense_landmarks / fs_world_landmarks_get on the GPU: every count, the discovered
list and the sighting counters against tests/landmark_sense_ref.py bit for bit; the set each pose sees against
fs_landmarks_in_view on a context that holds the whole world; the staged cloud against a twin that uploads the discovered
landmarks under "cloud.order" 2 (the staged arrays as bytes, the integers, lists and candidate records; the float sums); world clouds around the chunk
and device-order sizes; the interplay with fs_upload_landmarks, fs_upload_grid and a released world; the error paths; a first
call on a fresh context."""
import ctypes
import importlib

import numpy as np
import pytest

import landmark_sense_ref as LR
import occlusion_ref as OR

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
E = fsmod.capi
VOLUMES = [(14.0, 1.0), (6.0, 1.0), (6.0, 4.0)]                  # the last: cone off
C1_VOLUME = (1.2, 1.0)                                           # (C1's map is 3.2 m wide)
RAYS = dict(max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, n_rays=0, elev=(0.0,), obst=(240, 254), trace=(255, 255),
            polygon=(-1e300, -1e300, 1e300, 1e300), robot_radius=0.15)


def _sensor(vol, los=1, min_views=1):
    return dict(max_dist=vol[0], max_angle=vol[1], line_of_sight=los, min_views=min_views)


def _ctx(cells, origin, res, staged=None):
    """a context with table, fan and a staged grid of the world's shape (all free unless given) — the line of sight must come from
    the WORLD grid, so the staged one never holds the wall"""
    s = fsmod.FrontierScorer(device=0)
    s.lookup_generate()
    s.set_ray_params(**RAYS)
    s.upload_grid(np.zeros_like(cells) if staged is None else staged, origin, res)
    s.set_arrival_limits(4000.0, 0.0)
    return s


class Fixture:
    """the 64 x 64 map with a wall and two doors, 3 000 landmarks less the borderline ones, six poses; `sees` per (volume, los) once"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.cells = OR.fixture_cells()
        self.G = oracle.Grid(self.cells, origin=OR.FIX_ORIGIN, resolution=OR.FIX_RES)
        self.poses = OR.fixture_poses(oracle)
        self.world = LR.drop_borderline(oracle, self.poses, OR.fixture_landmarks(3000), VOLUMES)
        self._S = {}

    def S(self, vol, los):
        if (vol, los) not in self._S:
            self._S[(vol, los)] = LR.sees(self.oracle, self.G, self.poses, self.world, _sensor(vol, los))
        return self._S[(vol, los)]


@pytest.fixture(scope="module")
def fx(oracle):
    return Fixture(oracle)


@pytest.fixture(scope="module")
def sc(fx):
    s = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES)
    s.upload_world(fx.cells)
    yield s
    s.close()


def _check_state(s, wc, what=""):
    got = s.world_landmarks()
    assert got["m_world"] == wc.world.shape[0] and got["n_discovered"] == int(wc.flag.sum()), what
    np.testing.assert_array_equal(got["world_index"], wc.world_index, err_msg=f"world_index {what}")
    np.testing.assert_array_equal(got["views"], wc.views, err_msg=f"views {what}")


def _check_call(got, want, what=""):
    np.testing.assert_array_equal(got["n_in_view"], want["n_in_view"], err_msg=f"n_in_view {what}")
    assert (got["n_new"], got["n_discovered"]) == (want["n_new"], want["n_discovered"]), what


# ---- 1. against the restatement, bit for bit

@pytest.mark.parametrize("vol", VOLUMES)
@pytest.mark.parametrize("los", [0, 1])
@pytest.mark.parametrize("min_views", [1, 2])
def test_counts_lists_and_counters_equal_the_restatement(sc, fx, oracle, vol, los, min_views):
    S = fx.S(vol, los)
    sensor = _sensor(vol, los, min_views)
    what = f"{vol} los {los} min_views {min_views}"
    # the poses in one call
    sc.upload_world_landmarks(fx.world)
    wc = LR.WorldCloud(oracle, fx.world)
    _check_state(sc, wc, what + " (fresh)")
    _check_call(sc.sense_landmarks(fx.poses, sensor), wc.sense(fx.G, fx.poses, sensor, S=S), what)
    _check_state(sc, wc, what)
    assert 0 < wc.flag.sum() and (not los or wc.flag.sum() < fx.world.shape[0])   # (without the wall, six poses at 14 m see every landmark)
    one_call = wc.world_index.copy()
    # one call each: the same counters, the same set, and n_new adds up to it
    sc.upload_world_landmarks(fx.world)
    wc = LR.WorldCloud(oracle, fx.world)
    total = 0
    for k in range(fx.poses.shape[0]):
        got = sc.sense_landmarks(fx.poses[k:k + 1], sensor)
        _check_call(got, wc.sense(fx.G, fx.poses[k:k + 1], sensor, S=S[k:k + 1]), f"{what}, pose {k} alone")
        total += got["n_new"]
    _check_state(sc, wc, what + " (one call each)")
    np.testing.assert_array_equal(wc.world_index, one_call)
    assert total == one_call.shape[0]


def test_line_of_sight_in_three_dimensions(fs, oracle):
    w = fs.synth.make_workload("C1")                                # 64^3
    G = oracle.Grid(w.cells, origin=w.origin, resolution=w.resolution)
    poses = oracle.poses_from_yaw(w.goals[:4], np.array([0.3, -1.2, 2.5, 0.0]))
    world = LR.drop_borderline(oracle, poses, w.landmarks, [C1_VOLUME])
    sensor = _sensor(C1_VOLUME, 1, 1)
    S = LR.sees(oracle, G, poses, world, sensor)
    S0 = LR.sees(oracle, G, poses, world, _sensor(C1_VOLUME, 0, 1))
    assert 0 < S.sum() < S0.sum()                                   # the 3-D walk hides something and leaves something
    s = fs.FrontierScorer(device=0)
    try:
        s.upload_grid(np.zeros_like(w.cells), w.origin, w.resolution)
        s.upload_world(w.cells)
        s.upload_world_landmarks(world)
        wc = LR.WorldCloud(oracle, world)
        _check_call(s.sense_landmarks(poses, sensor), wc.sense(G, poses, sensor, S=S), "C1")
        _check_state(s, wc, "C1")
    finally:
        s.close()


# ---- 2. against fs_landmarks_in_view on a context that holds the whole world

@pytest.mark.parametrize("vol", [(14.0, 1.0), (6.0, 4.0)])
def test_each_pose_sees_what_landmarks_in_view_lists(sc, fx, vol):
    whole = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES, staged=fx.cells)
    try:
        whole.upload_landmarks(fx.world)
        whole.set_fim_params(*vol)
        whole.set_occlusion(True, occ=(254, 254), end_margin_m=0.3)
        off, ent = whole.landmarks_in_view(fx.poses)
        sc.upload_world_landmarks(fx.world)
        before = sc.world_landmarks()["views"]
        for k in range(fx.poses.shape[0]):
            got = sc.sense_landmarks(fx.poses[k:k + 1], dict(max_dist=vol[0], max_angle=vol[1], line_of_sight=1, min_views=1,
                                                              occ=(254, 254), end_margin_m=0.3))
            after = sc.world_landmarks()["views"]
            delta = after - before
            assert set(np.unique(delta).tolist()) <= {0, 1}
            np.testing.assert_array_equal(np.flatnonzero(delta), ent["index"][off[k]:off[k + 1]], err_msg=f"pose {k} {vol}")
            assert got["n_in_view"][0] == off[k + 1] - off[k] > 0
            before = after
    finally:
        whole.close()


# ---- 3. the staged cloud is what an upload would have staged

def _twin(fx, cloud, vol, occluded, staged=None):
    t = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES, staged=staged)
    t.set_option("cloud.order", 2)
    t.upload_landmarks(cloud)
    t.set_fim_params(*vol)
    t.set_occlusion(occluded)
    return t


FLOAT_COLUMNS = ("info_ref", "trace", "logdet")
# The Fisher float sums are not bit-stable from call to call in the scorer itself, whatever staged the cloud: on this fixture's map,
# six poses and a 4 097-landmark cloud sent through fs_upload_landmarks alone, 24 identical calls on 8 identical fresh contexts gave
# 2 distinct fs_score_fim outputs (one pose's info_ref, last bit) under each of "fim.learn" 0, "fim.split" 0, "fim.specialise" 0,
# "fim.hostfinish" 0 / 1 and "fim.bits1" 10; tests/test_gpu_frontier_search.py holds two such calls to rtol 1e-5 for the same reason.
# So the staging itself is compared byte for byte through fs_staged_cloud_get, every integer and every list exactly, and the float
# columns to that 1e-5 — except where the issue behind this feature asks for bytes (the last test of this section).
FLOAT_RTOL = 1.0e-5


def _same_staging(a, b, what):
    sa, sb = a.staged_cloud(), b.staged_cloud()
    assert (sa["m"], sa["n_chunks"]) == (sb["m"], sb["n_chunks"]), what
    for k in ("soa", "spheres", "perm"):
        assert sa[k].tobytes() == sb[k].tobytes(), f"staged {k} {what}"
    return sa


def _same_scores(a, b, poses, goals, what, float_bytes=False):
    _same_staging(a, b, what)
    fa, fb = a.score_fim(poses), b.score_fim(poses)
    for k in ("n_visible", "n_voxels"):
        np.testing.assert_array_equal(fa[k], fb[k], err_msg=f"{k} {what}")
    (oa, ea), (ob, eb) = a.landmarks_in_view(poses), b.landmarks_in_view(poses)
    np.testing.assert_array_equal(oa, ob, err_msg=f"offsets {what}")
    assert ea.tobytes() == eb.tobytes(), f"entries {what}"
    ra, rb = a.score_candidates(goals), b.score_candidates(goals)
    for f in ra.dtype.names:
        if f not in FLOAT_COLUMNS:
            assert ra[f].tobytes() == rb[f].tobytes(), f"records.{f} {what}"
    if float_bytes:
        for k in FLOAT_COLUMNS + ("fim21",):
            assert fa[k].tobytes() == fb[k].tobytes(), f"{k} {what}"
        assert ra.tobytes() == rb.tobytes(), f"records {what}"
    else:
        for k in FLOAT_COLUMNS:
            np.testing.assert_allclose(fa[k], fb[k], rtol=FLOAT_RTOL, err_msg=f"{k} {what}")
            np.testing.assert_allclose(ra[k], rb[k], rtol=FLOAT_RTOL, err_msg=f"records.{k} {what}")
        scale = np.maximum(np.abs(fb["fim21"]).max(axis=1, keepdims=True), 1e-6)
        assert np.max(np.abs(fa["fim21"] - fb["fim21"]) / scale, initial=0.0) <= FLOAT_RTOL, f"fim21 {what}"
    return fa, oa


def _two_sweeps_beside_a_twin(fx, occluded, float_bytes):
    vol = (6.0, 1.0)
    goals = np.array([[x, y, 0.0] for x, y in OR.FIX_XY])
    rng = np.random.default_rng(3)
    more = np.zeros((10, 7)); more[:, :2] = rng.uniform(-7.0, 7.0, size=(10, 2)); more[:, 2] = 0.3
    q = rng.normal(size=(10, 4)); more[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([fx.poses, more])
    a = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES, staged=fx.cells)
    t = None
    try:
        a.upload_world(fx.cells)
        a.set_fim_params(*vol)
        a.set_occlusion(occluded)
        a.upload_world_landmarks(fx.world)
        r1 = a.sense_landmarks(fx.poses[:2], _sensor(vol))
        idx1 = a.world_landmarks()["world_index"]
        assert r1["n_discovered"] == idx1.shape[0] > 64
        # one twin lives beside the context and serves the same calls in the same order
        t = _twin(fx, fx.world[idx1], vol, occluded, staged=fx.cells)
        f1, o1 = _same_scores(a, t, poses, goals, f"after the first sweep, occluded {occluded}", float_bytes)
        assert f1["n_visible"].max() > 0 and o1[-1] > 0
        # a second sweep adds landmarks: staged again, ranks shift
        r2 = a.sense_landmarks(fx.poses[2:], _sensor(vol))
        idx2 = a.world_landmarks()["world_index"]
        assert r2["n_new"] > 0 and r2["n_discovered"] == idx2.shape[0] == idx1.shape[0] + r2["n_new"]
        assert set(idx1.tolist()) < set(idx2.tolist())
        t.upload_landmarks(fx.world[idx2])
        f2, _ = _same_scores(a, t, poses, goals, f"after the second sweep, occluded {occluded}", float_bytes)
        assert f2["n_visible"].sum() > f1["n_visible"].sum()
    finally:
        a.close()
        if t is not None:
            t.close()


@pytest.mark.parametrize("occluded", [False, True])
def test_staged_cloud_equals_an_upload_of_the_discovered_landmarks(fx, occluded):
    """the staged arrays byte for byte, every integer, the lists and the records' integers exactly; the float sums to 1e-5"""
    _two_sweeps_beside_a_twin(fx, occluded, float_bytes=False)


@pytest.mark.parametrize("occluded", [False, True])
def test_fisher_sums_of_the_two_routes_compare_as_bytes(fx, occluded):
    """The same, with fim21, trace, logdet, info_ref and the whole records compared as BYTES, as the issue behind this feature sets it.
    The staged arrays ARE the same bytes (the test above), but the scorer's float sums are not bit-stable from call to call on ONE
    cloud (see FLOAT_COLUMNS above: 2 distinct outputs in 24 identical calls without any of this feature's code), so this test can
    fail through no fault of the staging: measured on an MI355X, 3 runs of these two cases gave 3 passes and 3 failures, each
    failure one pose's info_ref differing in its last bit (0x..d4 against 0x..d5 in its lowest byte, for instance)."""
    _two_sweeps_beside_a_twin(fx, occluded, float_bytes=True)


# ---- 4. sizes around the chunk (64) and the device-order threshold (4096)

@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 4095, 4097])
def test_sizes_with_a_known_mask(fx, oracle, m):
    world = OR.fixture_landmarks(m, seed=100 + m) if m else np.zeros((0, 3), dtype=np.float32)
    known = (np.arange(m) % 3 == 0)
    vol = (6.0, 1.0)
    goals = np.array([[x, y, 0.0] for x, y in OR.FIX_XY])
    a = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES)
    t = None
    try:
        a.set_fim_params(*vol)
        a.upload_world_landmarks(world, known)
        st = a.world_landmarks()
        assert (st["m_world"], st["n_discovered"]) == (m, int(known.sum()))
        np.testing.assert_array_equal(st["world_index"], np.flatnonzero(known))
        assert not st["views"].any()
        # a sweep that discovers nothing: a pose a kilometre away with half a metre of range
        far = np.array([[1000.0, 0.0, 0.3, 0.0, 0.0, 0.0, 1.0]])
        r = a.sense_landmarks(far, dict(max_dist=0.5, max_angle=1.0, line_of_sight=0))
        assert (r["n_in_view"][0], r["n_new"], r["n_discovered"]) == (0, 0, int(known.sum()))
        t = _twin(fx, world[known], vol, False)
        _same_scores(a, t, fx.poses, goals, f"m {m}, the known set")
        # a sweep that discovers everything: cone off, 100 m of range, no line of sight, from two poses
        r = a.sense_landmarks(fx.poses[:2], dict(max_dist=100.0, max_angle=4.0, line_of_sight=0))
        assert r["n_in_view"].tolist() == [m, m] and (r["n_new"], r["n_discovered"]) == (m - int(known.sum()), m)
        st = a.world_landmarks()
        np.testing.assert_array_equal(st["world_index"], np.arange(m))
        np.testing.assert_array_equal(st["views"], np.full(m, 2))
        t.upload_landmarks(world)
        _same_scores(a, t, fx.poses, goals, f"m {m}, the whole world")
    finally:
        a.close()
        if t is not None:
            t.close()


# ---- 5. interplay with the rest of the context

def test_upload_landmarks_in_between_is_undone_by_the_next_sweep(fx, oracle):
    vol = (6.0, 1.0)
    goals = np.array([[x, y, 0.0] for x, y in OR.FIX_XY])
    a = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES)
    t = None
    try:
        a.upload_world(fx.cells)
        a.set_fim_params(*vol)
        a.upload_world_landmarks(fx.world)
        r = a.sense_landmarks(fx.poses, _sensor(vol))
        idx = a.world_landmarks()["world_index"]
        other = OR.fixture_landmarks(500, seed=77)
        a.upload_landmarks(other)                                   # the caller's own cloud: the world cloud, counters and flags stay
        off, _ = a.landmarks_in_view(fx.poses)
        st = a.world_landmarks()
        np.testing.assert_array_equal(st["world_index"], idx)
        t = _twin(fx, other, vol, False)
        np.testing.assert_array_equal(off, t.landmarks_in_view(fx.poses)[0])
        r2 = a.sense_landmarks(fx.poses[:1], _sensor(vol))          # nothing new (all of pose 0's are discovered) — and yet staged again
        assert r2["n_new"] == 0 and r2["n_discovered"] == r["n_discovered"]
        t.upload_landmarks(fx.world[idx])
        _same_scores(a, t, fx.poses, goals, "restaged after fs_upload_landmarks")
    finally:
        a.close()
        if t is not None:
            t.close()


def test_another_grid_shape_drops_the_world_grid_and_release_leaves_the_staged_cloud(fx, oracle):
    vol = (6.0, 1.0)
    a = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES)
    try:
        a.upload_world(fx.cells)
        a.set_fim_params(*vol)
        a.upload_world_landmarks(fx.world)
        a.sense_landmarks(fx.poses[:1], _sensor(vol, los=1))
        before = a.world_landmarks()
        a.upload_grid(np.zeros((1, 32, 48), dtype=np.uint8), OR.FIX_ORIGIN, OR.FIX_RES)
        for sensor in (_sensor(vol, los=1), _sensor(vol, los=1, min_views=2)):
            with pytest.raises(E.FsError) as ei:
                a.sense_landmarks(fx.poses[1:2], sensor)
            assert ei.value.code == E.FS_E_STATE
        after = a.world_landmarks()
        np.testing.assert_array_equal(after["views"], before["views"])
        np.testing.assert_array_equal(after["world_index"], before["world_index"])
        wc = LR.WorldCloud(oracle, fx.world)
        wc.sense(fx.G, fx.poses[:1], _sensor(vol, 1), S=fx.S(vol, 1)[:1])
        # without a world grid: sensor NULL means line_of_sight 0 and the context's volume
        _check_call(a.sense_landmarks(fx.poses[1:2], None), wc.sense(None, fx.poses[1:2], _sensor(vol, 0), S=fx.S(vol, 0)[1:2]), "no world grid")
        _check_state(a, wc, "no world grid")
        # releasing the world cloud leaves the staged cloud alone
        off, ent = a.landmarks_in_view(fx.poses)
        a.upload_world_landmarks(None)
        with pytest.raises(E.FsError) as ei:
            a.sense_landmarks(fx.poses[:1], _sensor(vol, 0))
        assert ei.value.code == E.FS_E_STATE
        with pytest.raises(E.FsError) as ei:
            a.world_landmarks()
        assert ei.value.code == E.FS_E_STATE
        off2, ent2 = a.landmarks_in_view(fx.poses)
        np.testing.assert_array_equal(off, off2)
        assert ent.tobytes() == ent2.tobytes() and off[-1] > 0
    finally:
        a.close()


def test_unusable_world_landmarks_are_never_seen_and_keep_their_indices(fx, oracle):
    world = fx.world.copy()
    bad = [3, 64, 1000, world.shape[0] - 1]
    world[bad[0]] = (np.nan, 0.0, 0.0); world[bad[1]] = (0.0, np.inf, 0.0); world[bad[2]] = (1.0e30, 0.0, 0.0)
    world[bad[3]] = (0.0, 0.0, -np.inf)
    known = np.zeros(world.shape[0], dtype=np.uint8); known[[bad[1], 10]] = 1     # an unusable landmark may be known: it keeps its rank
    a = _ctx(fx.cells, OR.FIX_ORIGIN, OR.FIX_RES)
    t = None
    try:
        a.set_fim_params(6.0, 1.0)
        a.upload_world_landmarks(world, known)
        sensor = dict(max_dist=100.0, max_angle=4.0, line_of_sight=0)
        r = a.sense_landmarks(fx.poses, sensor)
        wc = LR.WorldCloud(oracle, world, known)
        _check_call(r, wc.sense(None, fx.poses, sensor), "unusable")
        _check_state(a, wc, "unusable")
        st = a.world_landmarks()
        assert st["views"][bad].tolist() == [0, 0, 0, 0]
        assert r["n_discovered"] == world.shape[0] - 3 and (r["n_in_view"] == world.shape[0] - 4).all()
        assert bad[1] in st["world_index"] and bad[0] not in st["world_index"]
        t = _twin(fx, world[st["world_index"]], (6.0, 1.0), False)
        _same_scores(a, t, fx.poses, np.array([[x, y, 0.0] for x, y in OR.FIX_XY]), "unusable landmarks in the discovered set")
    finally:
        a.close()
        if t is not None:
            t.close()


def test_error_paths_write_nothing(sc, fx):
    sc.upload_world_landmarks(fx.world)
    sc.sense_landmarks(fx.poses[:1], _sensor((6.0, 1.0)))
    before = sc.world_landmarks()
    L, h = sc._L, sc._h
    p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    poses = np.ascontiguousarray(fx.poses)
    bad_sensors = [E.LandmarkSensorC(0.0, 1.0, 1, 1, 254, 254, 0.3), E.LandmarkSensorC(6.0, -1.0, 1, 1, 254, 254, 0.3),
                   E.LandmarkSensorC(2.0e9, 1.0, 1, 1, 254, 254, 0.3), E.LandmarkSensorC(float("nan"), 1.0, 1, 1, 254, 254, 0.3),
                   E.LandmarkSensorC(6.0, 1.0, 2, 1, 254, 254, 0.3), E.LandmarkSensorC(6.0, 1.0, 1, 0, 254, 254, 0.3),
                   E.LandmarkSensorC(6.0, 1.0, 1, 1, 200, 100, 0.3), E.LandmarkSensorC(6.0, 1.0, 1, 1, 0, 256, 0.3),
                   E.LandmarkSensorC(6.0, 1.0, 1, 1, 254, 254, -1.0), E.LandmarkSensorC(6.0, 1.0, 1, 1, 254, 254, float("inf"))]
    niv = np.full(poses.shape[0], 77, dtype=np.int32)
    n_new, n_disc = ctypes.c_int32(77), ctypes.c_int32(77)
    for s in bad_sensors:
        assert L.fs_sense_landmarks(h, poses.shape[0], p(poses), ctypes.byref(s), p(niv), ctypes.byref(n_new), ctypes.byref(n_disc)) == E.FS_E_INVALID
    good = E.LandmarkSensorC(6.0, 1.0, 1, 1, 254, 254, 0.3)
    assert L.fs_sense_landmarks(h, -1, p(poses), ctypes.byref(good), p(niv), ctypes.byref(n_new), ctypes.byref(n_disc)) == E.FS_E_INVALID
    assert L.fs_sense_landmarks(h, 2, None, ctypes.byref(good), p(niv), ctypes.byref(n_new), ctypes.byref(n_disc)) == E.FS_E_INVALID
    assert (niv == 77).all() and n_new.value == 77 and n_disc.value == 77
    assert L.fs_upload_world_landmarks(h, None, 5, None) == E.FS_E_INVALID
    assert L.fs_upload_world_landmarks(h, p(fx.world), -1, None) == E.FS_E_INVALID
    assert L.fs_upload_world_landmarks(h, p(fx.world), 2000001, None) == E.FS_E_INVALID
    after = sc.world_landmarks()
    for k in ("world_index", "views"):
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    # n == 0: FS_OK, nothing changes
    r = sc.sense_landmarks(np.zeros((0, 7)), _sensor((6.0, 1.0)))
    assert (r["n_new"], r["n_discovered"]) == (0, before["n_discovered"])
    np.testing.assert_array_equal(sc.world_landmarks()["views"], before["views"])


# ---- 6. the first call on a fresh context: no earlier cloud, grid or table

def test_first_calls_on_a_fresh_context(fs, fx, oracle):
    s = fs.FrontierScorer(device=0)
    try:
        with pytest.raises(E.FsError) as ei:
            s.sense_landmarks(fx.poses, None)
        assert ei.value.code == E.FS_E_STATE
        s.upload_world_landmarks(fx.world)
        with pytest.raises(E.FsError) as ei:
            s.sense_landmarks(fx.poses, _sensor((14.0, 1.0), los=1))    # no world grid
        assert ei.value.code == E.FS_E_STATE
        wc = LR.WorldCloud(oracle, fx.world)
        # sensor NULL on a fresh context: fs_set_fim_params' defaults (14 m, 1.0 rad), min_views 1, no world grid -> no line of sight
        _check_call(s.sense_landmarks(fx.poses, None), wc.sense(None, fx.poses, _sensor((14.0, 1.0), 0), S=fx.S((14.0, 1.0), 0)), "fresh")
        _check_state(s, wc, "fresh")
        # the staged cloud is there for the calls that need a table once one is loaded
        s.lookup_generate()
        t = fs.FrontierScorer(device=0)
        try:
            t.lookup_generate(); t.set_option("cloud.order", 2); t.upload_landmarks(fx.world[wc.world_index])
            _same_staging(s, t, "fresh")
            fa, fb = s.score_fim(fx.poses), t.score_fim(fx.poses)
            for k in ("n_visible", "n_voxels"):
                np.testing.assert_array_equal(fa[k], fb[k], err_msg=k)
            for k in FLOAT_COLUMNS:
                np.testing.assert_allclose(fa[k], fb[k], rtol=FLOAT_RTOL, err_msg=k)
            assert fa["n_visible"].min() > 0
        finally:
            t.close()
    finally:
        s.close()
