"""fs_set_occlusion / fs_line_of_sight on the GPU: the primitive bit for bit against the numpy restatement
(tests/occlusion_ref.py), the scoring against the oracle over the landmarks the rule leaves, the invariants of the setting, and
every scoring route — fs_score_fim, the fused records, the way points of fs_plan_paths_information, the legs of fs_roadmap_routes,
fs_multi — honouring it."""
import importlib
import itertools

import numpy as np
import pytest

import occlusion_ref as OR

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
E = fsmod.capi
REL = 1e-4
COSTS = np.array([0, 100, 253, 254, 255], dtype=np.uint8)
MAX_DIST = 14.0


@pytest.fixture(scope="module")
def sc():
    """a context of this module's own: the setting must not leak into the session's shared scorer"""
    s = fsmod.FrontierScorer(device=0)
    s.lookup_generate()
    yield s
    s.close()


def _check_fim(got, want):
    """the rules of tests/test_gpu_parity.py::_check_fim (fit-slam_amd/parity.py)"""
    parity = importlib.import_module("fit-slam_amd.parity")
    np.testing.assert_array_equal(got["n_visible"], want["n_visible"])
    np.testing.assert_array_equal(got["n_voxels"], want["n_voxels"])
    scale = np.maximum(np.abs(want["info_f64"]), 1e-6)
    assert np.max(np.abs(got["info_ref"] - want["info_f64"]) / scale) <= REL
    drift = np.abs(want["info_ref"] - want["info_f64"]) / scale
    assert np.max(np.abs(got["info_ref"] - want["info_ref"]) / scale - drift) <= REL
    tr = np.maximum(np.abs(want["trace"]), 1e-6)
    assert np.max(np.abs(got["trace"] - want["trace"]) / tr) <= REL
    gate = parity.logdet_gate(got["logdet"], want["logdet"], want["fim"], n_visible=want["n_visible"])
    assert gate["ok"], gate
    if got.get("fim21") is not None:
        iu = np.triu_indices(6)
        wantF = want["fim"][:, iu[0], iu[1]]
        mag = np.maximum(np.abs(wantF).max(axis=1, keepdims=True), 1e-6)
        assert np.max(np.abs(got["fim21"] - wantF) / mag) <= REL


def _within_bar(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), 1e-6))) if want.size else 0.0


# ------------------------------------------------------------------------------------------------------------ 1. the primitive

def _pairs(rng, cells, origin, res, n):
    """n pairs: equal cells, axis-aligned and exactly diagonal lines in every sign combination, lines shorter than the margin,
    ends off the map, starts on an occluding cell, and random ones"""
    nz, ny, nx = cells.shape
    dims = np.array([nx, ny, nz])
    org = np.asarray(origin, dtype=np.float64)

    def centre(c):
        return org + (np.asarray(c, dtype=np.float64) + 0.5) * res

    a, b = [], []
    mid = dims // 2
    steps = [d for d in itertools.product((-1, 0, 1), repeat=3) if (nz > 1 or d[2] == 0)]
    for d in steps:                                                    # (0, 0, 0): equal cells
        for k in (1, 2, 3, 7):                                         # 1, 2: shorter than M; 7: longer (7 < nz or the axis is unused)
            e = mid + k * np.array(d)
            if (e >= 0).all() and (e < dims).all():
                a.append(centre(mid)); b.append(centre(e))
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0)):   # across the map
        k = int(min(dims[0], dims[1]) // 2 - 1)
        a.append(centre(mid)); b.append(centre(mid + k * np.array(d)))
    zc, yc, xc = np.nonzero(cells == 254)                              # a start on an occluding cell
    for i in rng.choice(zc.size, size=16, replace=False):
        a.append(centre((xc[i], yc[i], zc[i]))); b.append(centre(rng.integers(0, dims)))
    hi = dims * res
    for _ in range(24):                                                # one or both ends off the map
        p, q = rng.uniform(0, hi, size=3) + org, rng.uniform(0, hi, size=3) + org
        axis = int(rng.integers(0, 2))
        which = int(rng.integers(0, 3))
        off = org[axis] - res * 0.6 if rng.integers(0, 2) else org[axis] + hi[axis] + res * 0.1
        if which in (0, 2):
            p[axis] = off
        if which in (1, 2):
            q[axis] = off
        a.append(p); b.append(q)
    while len(a) < n:
        a.append(rng.uniform(0, hi, size=3) + org); b.append(rng.uniform(0, hi, size=3) + org)
    return np.array(a[:n]), np.array(b[:n])


@pytest.mark.parametrize("shape,res", [((1, 64, 64), 0.1), ((8, 32, 32), 0.25)])
def test_line_of_sight_equals_the_restatement(oracle, sc, shape, res):
    rng = np.random.default_rng(7 + shape[0])
    cells = rng.choice(COSTS, size=shape, p=[0.88, 0.03, 0.03, 0.03, 0.03])
    origin = (-3.2, 1.0, 0.0)
    G = oracle.Grid(cells, origin=origin, resolution=res)
    a, b = _pairs(rng, cells, origin, res, 512)
    assert a.shape == (512, 3)
    if shape[0] == 1:                                                  # z plays no part on a 2-D grid, whatever it is
        a[:, 2] = rng.uniform(-5, 5, size=512); b[:, 2] = rng.uniform(-5, 5, size=512)
    sc.upload_grid(cells, origin, res)
    try:
        for occ, margin in (((254, 254), 0.3), ((253, 254), 0.3), ((254, 254), 0.0)):
            sc.set_occlusion(False, occ, margin)                       # (`enabled` is not consulted)
            got = sc.line_of_sight(a, b)
            want = OR.lines_of_sight(oracle, G, a, b, occ, margin)
            for k in ("ok", "blocked", "tested_cells"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {occ} {margin}")
            assert 0 < want["blocked"].sum() < want["ok"].sum() and (want["ok"] == 0).sum() >= 16
            assert ((want["ok"] == 1) & (want["tested_cells"] == 0)).any()
    finally:
        sc.set_occlusion(False)


# -------------------------------------------------------------------------------------- 2. scoring against the filtered cloud

def _grid(oracle, cells=None):
    return oracle.Grid(OR.fixture_cells() if cells is None else cells, origin=OR.FIX_ORIGIN, resolution=OR.FIX_RES)


def _stage(sc, cells, lm, angle):
    sc.upload_grid(cells, OR.FIX_ORIGIN, OR.FIX_RES)
    sc.upload_landmarks(lm)
    sc.set_fim_params(MAX_DIST, angle)


@pytest.mark.parametrize("angle", [1.0, 4.0])
@pytest.mark.parametrize("m", [3000, 5000])
def test_scoring_equals_the_oracle_over_the_landmarks_in_line_of_sight(oracle, ref_table, sc, m, angle):
    """3 000 landmarks: the cloud ordered on the host; 5 000: on the device.  1.0: the cone; 4.0: the reference's own request."""
    G, lm, poses = _grid(oracle), OR.fixture_landmarks(m), OR.fixture_poses(oracle)
    off = oracle.pose_information(ref_table, lm, poses, MAX_DIST, angle)
    want = OR.occluded_pose_information(oracle, ref_table, G, lm, poses, MAX_DIST, angle)
    # not vacuous: the rule hides at least a fifth of what the predicate accepts, leaves at least ten, and — per cloud, over its
    # two visibility volumes (tests/test_occlusion_ref.py) — flips the 550 decision of a pose
    assert (want["n_visible"] <= 0.8 * off["n_visible"]).all() and (want["n_visible"] >= 10).all()
    flips = 0
    for ang in (1.0, 4.0):
        w_off = oracle.pose_information(ref_table, lm, poses, MAX_DIST, ang)
        w_on = OR.occluded_pose_information(oracle, ref_table, G, lm, poses, MAX_DIST, ang)
        flips += int(((w_on["info_ref"] > 550.0) != (w_off["info_ref"] > 550.0)).sum())
    assert flips >= 1
    _stage(sc, G.cells, lm, angle)
    try:
        sc.set_occlusion(True)
        assert sc.get_occlusion() == dict(enabled=True, occ=(254, 254), end_margin_m=0.3)
        got = sc.score_fim(poses)
        _check_fim(got, want)
        lean = sc.score_fim(poses, info_only=True)                     # NULL columns: what isPoseSafe reads
        np.testing.assert_array_equal(lean["n_voxels"], want["n_voxels"])
        assert _within_bar(lean["info_ref"], want["info_f64"]) <= REL
        one = sc.score_fim(poses[4:5], info_only=True)                 # the reference's call: one pose
        assert one["n_voxels"][0] == want["n_voxels"][4] and _within_bar(one["info_ref"], want["info_f64"][4:5]) <= REL
        sc.set_occlusion(False)
        np.testing.assert_array_equal(sc.score_fim(poses)["n_visible"], off["n_visible"])
    finally:
        sc.set_occlusion(False)


# -------------------------------------------------------------------------------------------------------------- 3. invariants

def test_invariants_of_the_setting(oracle, ref_table, sc):
    lm, poses = OR.fixture_landmarks(3000), OR.fixture_poses(oracle)
    cells = OR.fixture_cells()
    try:
        # no cost in the range: the integers of occlusion off, the floats within the parity rule
        soft = np.where(cells == 254, 100, cells).astype(np.uint8)
        _stage(sc, soft, lm, 1.0)
        off = sc.score_fim(poses)
        sc.set_occlusion(True)
        on = sc.score_fim(poses)
        want = oracle.pose_information(ref_table, lm, poses, MAX_DIST, 1.0)
        _check_fim(on, want)
        for k in ("n_visible", "n_voxels"):
            np.testing.assert_array_equal(on[k], off[k])
        # off again: the integers of a context that never had it on; on with no grid: FS_E_STATE
        sc.upload_grid(cells, OR.FIX_ORIGIN, OR.FIX_RES)
        hidden = sc.score_fim(poses)
        assert (hidden["n_visible"] < off["n_visible"]).all()
        sc.set_occlusion(False)
        back = sc.score_fim(poses)
        fresh = fsmod.FrontierScorer(device=0)
        try:
            fresh.lookup_generate()
            fresh.upload_landmarks(lm)
            fresh.set_fim_params(MAX_DIST, 1.0)
            never = fresh.score_fim(poses)
            for k in ("n_visible", "n_voxels"):
                np.testing.assert_array_equal(back[k], never[k])
            fresh.set_occlusion(True)
            with pytest.raises(fsmod.FsError) as e:
                fresh.score_fim(poses)
            assert e.value.code == E.FS_E_STATE
            fresh.set_occlusion(False)
            np.testing.assert_array_equal(fresh.score_fim(poses)["n_visible"], never["n_visible"])   # off: no grid needed
        finally:
            fresh.close()
        # invalid settings: FS_E_INVALID, nothing stored
        sc.set_occlusion(True, (200, 254), 0.5)
        kept = sc.get_occlusion()
        for occ, margin in (((255, 254), 0.3), ((-1, 254), 0.3), ((0, 256), 0.3), ((254, 254), float("nan")), ((254, 254), -0.1),
                            ((254, 254), 1.0e6), ((254, 254), float("inf"))):
            with pytest.raises(fsmod.FsError) as e:
                sc.set_occlusion(True, occ, margin)
            assert e.value.code == E.FS_E_INVALID
            assert sc.get_occlusion() == kept
        assert sc._L.fs_set_occlusion(sc._h, None) == E.FS_OK           # NULL: the defaults
        assert sc.get_occlusion() == dict(enabled=False, occ=(254, 254), end_margin_m=0.3)
    finally:
        sc.set_occlusion(False)


def test_keepout_zones_and_map_updates(oracle, ref_table, sc):
    lm, poses = OR.fixture_landmarks(3000), OR.fixture_poses(oracle)[4:5]          # the pose at (-1, 0.2) looking along +x
    try:
        # a keep-out disc (253) in front of the pose on an otherwise empty map: nothing by default, a screen under (253, 254)
        _stage(sc, np.zeros((64, 64), dtype=np.uint8), lm, 1.0)
        off = sc.score_fim(poses)
        _, n_cells = sc.keepout_add_disc(1.5, 0.2, 1.0)
        assert n_cells > 0
        painted = sc.read_grid_region()
        assert (painted == 253).any() and not (painted == 254).any()
        sc.set_occlusion(True)
        same = sc.score_fim(poses)
        for k in ("n_visible", "n_voxels"):
            np.testing.assert_array_equal(same[k], off[k])
        sc.set_occlusion(True, (253, 254))
        want = OR.occluded_pose_information(oracle, ref_table, _grid(oracle, painted), lm, poses, MAX_DIST, 1.0, occ=(253, 254))
        assert want["n_visible"][0] < off["n_visible"][0]
        _check_fim(sc.score_fim(poses), want)
        sc.keepout_clear()
        # fs_update_grid_region opens a third door in the wall: the result is the restatement's on the new map, at once
        cells = OR.fixture_cells()
        _stage(sc, cells, lm, 1.0)
        sc.set_occlusion(True)
        before = sc.score_fim(poses)
        _check_fim(before, OR.occluded_pose_information(oracle, ref_table, _grid(oracle, cells), lm, poses, MAX_DIST, 1.0))
        sc.update_grid_region(31, 29, 0, np.zeros((6, 2), dtype=np.uint8))
        opened = cells.copy()
        opened[29:35, 31:33] = 0
        want = OR.occluded_pose_information(oracle, ref_table, _grid(oracle, opened), lm, poses, MAX_DIST, 1.0)
        assert want["n_visible"][0] > before["n_visible"][0]
        _check_fim(sc.score_fim(poses), want)
    finally:
        sc.keepout_clear()
        sc.set_occlusion(False)


# ---------------------------------------------------------------------------------------------------------- 4. every route

def _goals():
    xy = list(OR.FIX_XY) + [(2.0, 3.0), (-6.5, 1.0)]
    return np.array([[x, y, 0.0] for x, y in xy], dtype=np.float64)     # 8 candidates; z = origin_z on a 2-D grid


def test_fused_records_carry_the_occluded_counts(oracle, ref_table, sc):
    G, lm = _grid(oracle), OR.fixture_landmarks(3000)
    goals = np.concatenate([_goals(), [[1.0, 1.0, 0.0], [9.0, 0.0, 0.0]]])          # + one blacklisted, one off the map
    black = np.zeros(goals.shape[0], dtype=np.uint8)
    black[8] = 1
    _stage(sc, G.cells, lm, 1.0)
    sc.set_ray_params(max_camera_depth=2.0, delta_theta=0.1, camera_fov=1.04, robot_radius=0.3)
    sc.set_arrival_limits(4000.0, sc.max_arrival()["min_gt"])
    try:
        arr = sc.score_arrival(goals, blacklisted=black, want_ray_counts=False)
        ok = arr["status"] == 0
        assert ok[:8].all() and not ok[8:].any()
        poses = oracle.poses_from_yaw(goals, arr["yaw"])
        plain = sc.score_candidates(goals, blacklisted=black)
        sc.set_occlusion(True)
        fim = sc.score_fim(poses)
        want = OR.occluded_pose_information(oracle, ref_table, G, lm, poses[ok], MAX_DIST, 1.0)
        np.testing.assert_array_equal(fim["n_visible"][ok], want["n_visible"])
        rec = sc.score_candidates(goals, blacklisted=black)
        np.testing.assert_array_equal(E.record_status(rec), arr["status"])
        np.testing.assert_array_equal(rec["arrival"], plain["arrival"])
        np.testing.assert_array_equal(rec["n_visible"][ok], fim["n_visible"][ok])
        np.testing.assert_array_equal(E.record_nvoxels(rec)[ok], np.minimum(fim["n_voxels"][ok], 65535))
        assert _within_bar(rec["info_ref"][ok], want["info_f64"]) <= REL
        assert (rec["n_visible"][ok] < plain["n_visible"][ok]).any()
        # a candidate whose status is not OK: zero Fisher information, as without occlusion
        assert (rec["n_visible"][~ok] == 0).all() and (rec["info_ref"][~ok] == 0).all() and (E.record_nvoxels(rec)[~ok] == 0).all()
        # the one-call cost assignment reads the same records
        costs = sc.get_frontier_costs(goals, np.linspace(1.0, 9.0, goals.shape[0]), np.zeros(goals.shape[0]), blacklisted=black, with_fim=True)
        np.testing.assert_array_equal(costs["records"]["n_visible"], rec["n_visible"])
    finally:
        sc.set_occlusion(False)


def _values_follow_the_setting(oracle, ref_table, sc, G, lm, pose7, info, what):
    """the dumped poses handed to fs_score_fim give the dumped values (the header's promise) — which are the occluded ones"""
    assert info.size >= 3, what
    again = sc.score_fim(pose7, info_only=True)["info_ref"]
    assert _within_bar(info, again) <= REL, what
    pick = np.unique(np.linspace(0, info.size - 1, 6).astype(int))
    want = OR.occluded_pose_information(oracle, ref_table, G, lm, pose7[pick], MAX_DIST, 1.0)
    assert _within_bar(info[pick], want["info_f64"]) <= REL, what
    sc.set_occlusion(False)
    plain = sc.score_fim(pose7, info_only=True)["info_ref"]
    sc.set_occlusion(True)
    assert (info < plain * (1 - 1e-3)).any(), what


def test_way_points_and_route_legs_are_scored_in_line_of_sight(oracle, ref_table, sc):
    G, lm = _grid(oracle), OR.fixture_landmarks(3000)
    _stage(sc, G.cells, lm, 1.0)
    robot = oracle.poses_from_yaw(np.array([[-5.0, -5.0, 0.0]]), np.array([0.3]))[0]
    goals = _goals()[1:]
    try:
        sc.set_occlusion(True)
        got = sc.plan_paths_information(robot, goals, allow_unknown=True, want_waypoints=True)
        assert got["achievable"].any()
        _values_follow_the_setting(oracle, ref_table, sc, G, lm, got["waypoint_pose7"], got["waypoint_info"], "way points")
        # a roadmap on the free cells of a 2 m lattice (the robot stands on one of its points) and the goals' own points
        pts = [(x, y) for x in np.arange(-7.0, 7.5, 2.0) for y in np.arange(-7.0, 7.5, 2.0)
               if G.cells[0, int((y + 8) / OR.FIX_RES), int((x + 8) / OR.FIX_RES)] == 0]
        sc.roadmap_add_nodes(np.array(pts + [tuple(g[:2]) for g in goals]))
        sc.roadmap_rebuild()
        r = sc.roadmap_routes(robot, goals, want_legs=True)
        _values_follow_the_setting(oracle, ref_table, sc, G, lm, r["leg_pose7"], r["leg_info"], "route legs")
    finally:
        sc.set_occlusion(False)


def test_multi_broadcasts_the_setting(oracle, sc):
    G, lm, poses = _grid(oracle), OR.fixture_landmarks(3000), OR.fixture_poses(oracle)
    _stage(sc, G.cells, lm, 1.0)
    m = fsmod.MultiScorer(devices=[0])
    try:
        m.lookup_generate()
        m.upload_grid(G.cells, OR.FIX_ORIGIN, OR.FIX_RES)
        m.upload_landmarks(lm)
        m.set_fim_params(MAX_DIST, 1.0)
        sc.set_occlusion(True, (254, 254), 0.3)
        m.set_occlusion(True, (254, 254), 0.3)
        assert m.get_occlusion() == sc.get_occlusion()
        a, b = sc.score_fim(poses), m.score_fim(poses)
        for k in ("n_visible", "n_voxels"):
            np.testing.assert_array_equal(a[k], b[k])
        assert _within_bar(b["info_ref"], a["info_ref"]) <= REL
        with pytest.raises(fsmod.FsError) as e:
            m.set_occlusion(True, (255, 0))
        assert e.value.code == E.FS_E_INVALID
    finally:
        m.close()
        sc.set_occlusion(False)
