"""fs_information_layer on the GPU against tests/information_layer_ref.py: anchors, counts and heading pairs exactly,
every per-heading value against the oracle and against fs_score_fim within the project's 1e-4 bar, and the field, the cost bytes
and the grid against the restatement fed the call's own per-heading values, bit for bit.  Maps are 96 x 80 and 130 x 70 with 3 000
landmarks: every stride leaves a cut last block, stride 3 on the whole map scores more than 256 blocks (the compaction crosses a
workgroup seam), the stride-1 window more than 64."""
import ctypes as C

import numpy as np
import pytest

import information_layer_ref as L
import inflation_ref as I
import occlusion_ref as OR

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
RES, ORIGIN, REL = L.RES, L.ORIGIN, L.REL
# Two calls on one cloud: the FIM worker's float sums are not bit-stable from call to call under any "fim.*" option,
# so a value is compared ACROSS calls to the bar tests/test_gpu_frontier_search.py holds two such calls to; bytes and grids across
# calls are compared where the cost steps are coarse (max_cost 8 over 200 .. 2500: 290 apart, a last bit moves no byte)
CALL_REL = 1e-5
COARSE = dict(info_lo=200.0, info_hi=2500.0, max_cost=8)
QUAT_ABS = 1e-12                 # host libm against numpy (sin, cos): a few ulp of a double
VIS = [(14.0, 1.0), (14.0, 4.0)]
LO, HI = 950.0, 1100.0           # about the spread of the maps' heading means under VIS[0]
# window (negative offsets: from the far corner), stride, K, reduce, yaw0, visibility
CASES = {
    "whole_s5_k8": (None, 5, 8, "mean", 0.0, 0),
    "whole_s3_k4": (None, 3, 4, "min", 0.3, 0),
    "whole_s7_k4": (None, 7, 4, "max", -1.1, 1),
    "odd_s5_k1": ((13, 7, 37, 21), 5, 1, "mean", 2.0, 1),
    "corner_s7_k8": ((0, -17, 29, 17), 7, 8, "mean", 0.0, 0),
    "far_corner_s5_k4": ((-23, -31, 23, 31), 5, 4, "min", 0.0, 1),
    "wide_s7_k1": ((3, 5, 71, 18), 7, 1, "max", 0.0, 0),
    "stride1_k4": ((31, 22, 24, 17), 1, 4, "mean", 0.0, 0),
    "s32_k8": ((5, 3, 80, 60), 32, 8, "mean", 0.0, 1),
}


def _window(w, cells):
    ny, nx = cells.shape
    return (0, 0, nx, ny) if w is None else (w[0] % nx, w[1] % ny, w[2], w[3])


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.Table.generate()


@pytest.fixture(scope="module")
def scorers(fs):
    """one staged context per map, kept for the module; get(m) stages the raw map again"""
    made = {}

    def get(m, vis=VIS[0]):
        cells, lm = L.layer_map(m)
        if m not in made:
            sc = fs.FrontierScorer(device=0)
            sc.upload_landmarks(lm)
            sc.lookup_generate()
            made[m] = sc
        made[m].upload_grid(cells, ORIGIN, RES)
        made[m].set_fim_params(*vis)
        return made[m]
    yield get
    for sc in made.values():
        sc.close()


def _grid_of(sc):
    return sc.read_grid_region()[0]


def _within_bar(got, want):
    scale = np.maximum(np.abs(want), 1e-6)
    return float(np.max(np.abs(got.astype(np.float64) - want) / scale)) if want.size else 0.0


def _same_values(a, b):
    """two calls' fields: the same blocks scored, every value within CALL_REL"""
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert _within_bar(a[ok], b[ok].astype(np.float64)) <= CALL_REL


def _check_geometry(res, cells, win, s, K, yaw0, pose_z=0.0):
    nx = cells.shape[1]
    anchor = L.anchors(cells, win, s)
    np.testing.assert_array_equal(res.anchor_cell, anchor)
    assert res.n_scored == int((anchor >= 0).sum())
    quat = L.quat_zw(K, yaw0)
    assert res.quat_zw.shape == (K, 2) and np.max(np.abs(res.quat_zw - quat)) <= QUAT_ABS
    want = L.poses(anchor, res.quat_zw, nx, ORIGIN, RES, pose_z)
    np.testing.assert_array_equal(res.pose7, want)                      # positions exactly; the pairs are the call's own
    return anchor


def _check_own_values(res, before, after, win, s, reduce, lo, hi, max_cost, write=True):
    """the field, the bytes and the grid from the call's own info_per_yaw, bit for bit"""
    ref = L.layer(before, win, s, res.info_per_yaw, reduce, lo, hi, max_cost)
    assert res.info.dtype == np.float32 and res.info_per_yaw.dtype == np.float32
    np.testing.assert_array_equal(res.info.view(np.uint32)[ref["anchor"] >= 0], ref["info"].view(np.uint32)[ref["anchor"] >= 0])
    assert np.isnan(res.info[ref["anchor"] < 0]).all() and np.isnan(res.info_per_yaw[:, ref["anchor"] < 0]).all()
    assert not np.isnan(res.info_per_yaw[:, ref["anchor"] >= 0]).any()
    if write:
        np.testing.assert_array_equal(after, ref["grid"])
        assert res.n_changed == ref["n_changed"]
    else:
        np.testing.assert_array_equal(after, before)
        assert res.n_changed == 0
    return ref


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("m", list(L.MAPS))
def test_cases(oracle, table, scorers, m, case):
    w, s, K, reduce, yaw0, v = CASES[case]
    cells, lm = L.layer_map(m)
    win = _window(w, cells)
    sc = scorers(m, VIS[v])
    # info_lo, info_hi: the quartiles of the field the oracle expects (parameters, not bounds), so the bytes of a case are many
    expect = L.anchors(cells, win, s)
    values = L.oracle_values(oracle, table, lm, L.poses(expect, L.quat_zw(K, yaw0), cells.shape[1], ORIGIN), VIS[v])
    field = L.reduce_field(L.per_yaw_field(expect, values, K), reduce)[expect >= 0]
    lo, hi = float(np.percentile(field, 25)), float(np.percentile(field, 75))
    assert hi > lo
    res = sc.information_layer(stride_cells=s, n_yaw=K, yaw0=yaw0, reduce=reduce, info_lo=lo, info_hi=hi, window=win, want_per_yaw=True)
    after = _grid_of(sc)
    anchor = _check_geometry(res, cells, win, s, K, yaw0)
    assert res.n_scored > 0 and res.pose7.shape == (res.n_scored * K, 7)
    ref = _check_own_values(res, cells, after, win, s, reduce, lo, hi, 252)
    assert res.n_changed > 0 and np.unique(ref["cost"][anchor >= 0]).size >= (3 if res.n_scored >= 8 else 1)
    # untouched: cells at 253 and above, unknown cells, cells outside the window
    changed = after != cells
    outside = np.ones_like(changed)
    outside[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = False
    assert not changed[cells >= 253].any() and not changed[outside].any()
    # every per-heading value: the oracle at the dumped poses, and fs_score_fim on this context
    got = res.info_per_yaw[:, anchor >= 0].T.reshape(-1)                 # [scored][K]: the order of pose7
    want = L.oracle_values(oracle, table, lm, res.pose7, VIS[v])
    err = _within_bar(got, want)
    print(f"{m} {case}: {res.n_scored} blocks, largest deviation from the oracle {err:.3e}")
    assert err <= REL
    fim = sc.score_fim(res.pose7, info_only=True)["info_ref"]
    assert _within_bar(got, fim.astype(np.float64)) <= REL
    assert sc.information_layer(stride_cells=s, n_yaw=K, yaw0=yaw0, reduce=reduce, info_lo=lo, info_hi=hi, window=win, write=False).info_per_yaw is None


@pytest.mark.parametrize("m", list(L.MAPS))
def test_reductions_and_the_field_only_form(scorers, m):
    cells, _ = L.layer_map(m)
    win = (7, 3, 83, 61)
    fields = {}
    for reduce in L.REDUCE:
        for write in (False, True):
            sc = scorers(m)
            res = sc.information_layer(stride_cells=5, n_yaw=8, reduce=reduce, info_lo=200.0, info_hi=2500.0, max_cost=200, window=win, write=write,
                                       want_per_yaw=True)
            _check_geometry(res, cells, win, 5, 8, 0.0)
            _check_own_values(res, cells, _grid_of(sc), win, 5, reduce, 200.0, 2500.0, 200, write)
            fields[reduce, write] = res
        _same_values(fields[reduce, False].info, fields[reduce, True].info)
        assert fields[reduce, True].n_changed > 0
        # a second writing call changes nothing (its values are another call's: COARSE steps)
        sc = scorers(m)
        first = sc.information_layer(stride_cells=5, n_yaw=8, reduce=reduce, window=win, **COARSE)
        after = _grid_of(sc)
        again = sc.information_layer(stride_cells=5, n_yaw=8, reduce=reduce, window=win, **COARSE)
        assert first.n_changed > 0 and again.n_changed == 0
        np.testing.assert_array_equal(_grid_of(sc), after)
    assert not np.array_equal(fields["min", True].info, fields["max", True].info)
    with np.errstate(invalid="ignore"):
        assert not (fields["min", True].info > fields["mean", True].info).any() and not (fields["mean", True].info > fields["max", True].info).any()


def test_pose_height_and_cost_range(scorers):
    m = "96x80"
    cells, _ = L.layer_map(m)
    win = (0, 0, 96, 80)
    for pose_z, max_cost, lo, hi in ((0.4, 1, LO, HI), (1.2, 252, 1e-3, 1e9), (0.0, 77, -5.0, 1.0)):
        sc = scorers(m)
        res = sc.information_layer(stride_cells=7, n_yaw=4, pose_z=pose_z, reduce="mean", info_lo=lo, info_hi=hi, max_cost=max_cost,
                                   window=win, want_per_yaw=True)
        _check_geometry(res, cells, win, 7, 4, 0.0, pose_z)
        ref = _check_own_values(res, cells, _grid_of(sc), win, 7, "mean", lo, hi, max_cost)
        assert ref["cost"].max() <= max_cost


@pytest.mark.parametrize("m", list(L.MAPS))
def test_after_inflate_the_result_is_the_max_of_both(scorers, m):
    cells, _ = L.layer_map(m)
    ny, nx = cells.shape
    win = (0, 0, nx, ny)
    inflated = I.inflate_exact(cells, I.LOCAL)[0]
    sc = scorers(m)
    sc.inflate(*I.LOCAL)
    np.testing.assert_array_equal(_grid_of(sc), inflated)
    res = sc.information_layer(stride_cells=5, n_yaw=4, info_lo=LO, info_hi=HI, window=win, want_per_yaw=True)
    after = _grid_of(sc)
    _check_geometry(res, inflated, win, 5, 4, 0.0)
    ref = _check_own_values(res, inflated, after, win, 5, "mean", LO, HI, 252)
    layer_alone = np.kron(ref["cost"], np.ones((5, 5), dtype=np.uint8))[:ny, :nx]
    writable = (inflated <= 252) & np.kron(ref["anchor"] >= 0, np.ones((5, 5), dtype=bool))[:ny, :nx]
    np.testing.assert_array_equal(after[writable], np.maximum(inflated, layer_alone)[writable])
    np.testing.assert_array_equal(after[~writable], inflated[~writable])
    assert (after[writable] > inflated[writable]).any() and (after[writable] == inflated[writable]).any()


@pytest.mark.parametrize("m", list(L.MAPS))
def test_cost_bytes_against_the_oracle(oracle, table, scorers, m):
    """equal, except on blocks whose oracle value lies within the 1e-4 bar of a quantisation edge: there at most 1 apart, and at
    most 1 % of the scored blocks (tests/test_information_layer_restatement.py holds the oracle alone to that)"""
    cells, lm = L.layer_map(m)
    ny, nx = cells.shape
    win = (0, 0, nx, ny)
    for s, K, vis in L.EDGE_CASES:
        anchor = L.anchors(cells, win, s)
        v = L.oracle_values(oracle, table, lm, L.poses(anchor, L.quat_zw(K), nx, ORIGIN), vis).reshape(-1, K)
        mean = v.sum(axis=1) / K
        lo, hi = L.edge_range(mean)
        sc = scorers(m, vis)
        res = sc.information_layer(stride_cells=s, n_yaw=K, reduce="mean", info_lo=lo, info_hi=hi, max_cost=L.EDGE_COST, window=win, want_per_yaw=True)
        got = _check_own_values(res, cells, _grid_of(sc), win, s, "mean", lo, hi, L.EDGE_COST)["cost"][anchor >= 0]
        want = L.cost_of(mean.astype(np.float32), lo, hi, L.EDGE_COST)
        near = L.near_edge(mean, lo, hi, L.EDGE_COST)
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"{m} stride {s}: {int((diff > 0).sum())} of {mean.size} bytes differ, {int(near.sum())} blocks near an edge")
        assert (diff[~near] == 0).all() and (diff <= 1).all() and near.sum() <= 0.01 * mean.size


def test_results_do_not_depend_on_the_batch_size(scorers):
    m = "130x70"
    cells, _ = L.layer_map(m)
    out = {}
    for batch in (None, 64, 1000):
        sc = scorers(m)
        if batch:
            sc.set_option("infolayer.batch", batch)
        try:
            res = sc.information_layer(stride_cells=3, n_yaw=4, reduce="mean", want_per_yaw=True, **COARSE)
            _check_own_values(res, cells, _grid_of(sc), (0, 0, cells.shape[1], cells.shape[0]), 3, "mean", COARSE["info_lo"], COARSE["info_hi"],
                              COARSE["max_cost"])
        finally:
            sc.set_option("infolayer.batch", 65536)
        out[batch] = (res, _grid_of(sc))
    assert out[None][0].n_scored * 4 > 1000
    for batch in (64, 1000):
        a, b = out[None], out[batch]
        _same_values(a[0].info_per_yaw, b[0].info_per_yaw)
        _same_values(a[0].info, b[0].info)
        np.testing.assert_array_equal(a[0].anchor_cell, b[0].anchor_cell)
        assert a[0].n_changed == b[0].n_changed > 0 and a[0].n_scored == b[0].n_scored
        np.testing.assert_array_equal(a[1], b[1])
    for bad in (0, -1, float(1 << 25)):
        with pytest.raises(Exception):
            sc.set_option("infolayer.batch", bad)


def test_occlusion(fs, oracle, table):
    cells, lm = L.layer_map("96x80")
    lm = lm[:600]
    win = (30, 20, 21, 14)
    G = oracle.Grid(np.array(cells), origin=ORIGIN, resolution=RES)
    sc = fs.FrontierScorer(device=0)
    try:
        sc.upload_grid(cells, ORIGIN, RES)
        sc.upload_landmarks(lm)
        sc.lookup_generate()
        sc.set_fim_params(*VIS[1])
        off = sc.information_layer(stride_cells=7, n_yaw=2, window=win, write=False, want_per_yaw=True)
        sc.set_occlusion(True)
        res = sc.information_layer(stride_cells=7, n_yaw=2, reduce="min", info_lo=100.0, info_hi=400.0, window=win, want_per_yaw=True)
        anchor = _check_geometry(res, cells, win, 7, 2, 0.0)
        _check_own_values(res, cells, _grid_of(sc), win, 7, "min", 100.0, 400.0, 252)
        want = OR.occluded_pose_information(oracle, table, G, lm, res.pose7, *VIS[1])
        got = res.info_per_yaw[:, anchor >= 0].T.reshape(-1)
        assert res.n_scored >= 4 and _within_bar(got, want["info_f64"]) <= REL
        assert (want["n_visible"] < 600).all() and not np.array_equal(off.info_per_yaw, res.info_per_yaw)      # the rule hid something
    finally:
        sc.close()


def _params(**kw):
    p = dict(stride_cells=5, n_yaw=8, yaw0=0.0, pose_z=0.0, reduce="mean", info_lo=550.0, info_hi=1100.0, max_cost=252)
    p.update(kw)
    return p


def test_refusals_leave_the_grid_alone(fs):
    cells, lm = L.layer_map("130x70")
    ny, nx = cells.shape
    nan, inf = float("nan"), float("inf")
    sc = fs.FrontierScorer(device=0)

    def refused(code, **kw):
        with pytest.raises(fs.capi.FsError) as e:
            sc.information_layer(**kw)
        assert e.value.code == code, kw
    try:
        sc._grid_shape, sc._grid_geom = (1, ny, nx), (ORIGIN, RES)       # (the binding's own check is not the one under test)
        refused(FS_E_STATE, **_params())
        sc.upload_grid(cells, ORIGIN, RES)
        refused(FS_E_STATE, **_params())                                 # no cloud
        sc.upload_landmarks(lm)
        refused(FS_E_STATE, **_params())                                 # no table
        sc.lookup_generate()
        for bad in (dict(stride_cells=0), dict(stride_cells=33), dict(stride_cells=-1), dict(n_yaw=0), dict(n_yaw=65), dict(yaw0=nan), dict(yaw0=inf),
                    dict(pose_z=nan), dict(pose_z=-inf), dict(info_lo=nan), dict(info_hi=nan), dict(info_lo=-inf), dict(info_hi=inf),
                    dict(info_lo=1100.0), dict(info_lo=1200.0), dict(info_lo=-1e308, info_hi=1e308), dict(max_cost=0), dict(max_cost=253),
                    dict(max_cost=-3)):
            refused(FS_E_INVALID, **_params(**bad))
        with pytest.raises(fs.capi.FsError):
            sc.information_layer(reduce="median")
        p = fs.capi.InfoLayerParamsC(5, 8, 0.0, 0.0, 3, 550.0, 1100.0, 252, 1)       # an unknown reduction past the binding
        assert sc._L.fs_information_layer(sc._h, C.byref(p), 0, 0, nx, ny, None, None, None, None, None, None) == FS_E_INVALID
        for win in ((-1, 0, 4, 4), (0, -1, 4, 4), (nx - 3, 0, 4, 4), (0, ny - 3, 4, 4), (nx, 0, 1, 1), (0, 0, nx + 1, ny), (0, 0, -1, 4), (0, 0, 4, -1),
                    (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
            refused(FS_E_INVALID, window=win, **_params())
        np.testing.assert_array_equal(_grid_of(sc), cells)
        vol = np.random.default_rng(1).integers(0, 256, size=(3, 40, 56), dtype=np.uint8)
        sc.upload_grid(vol, ORIGIN, RES)
        with pytest.raises(fs.capi.FsError) as e:
            sc.information_layer(window=(0, 0, 4, 4))
        assert e.value.code == FS_E_INVALID
        assert str(e.value) == f"fitslam_frontier error {FS_E_INVALID}: the information layer is defined on a 2-D costmap (nz == 1)"
        np.testing.assert_array_equal(sc.read_grid_region(), vol)
    finally:
        sc.close()


def test_empty_cases(scorers):
    m = "96x80"
    cells, _ = L.layer_map(m)
    sc = scorers(m)
    for win in ((9, 9, 0, 5), (9, 9, 5, 0), (0, 0, 0, 0)):
        res = sc.information_layer(window=win, want_per_yaw=True)
        assert (res.n_scored, res.n_changed) == (0, 0) and res.info.size == 0 and res.pose7.shape == (0, 7) and res.quat_zw.shape == (8, 2)
    assert (cells[0:7, 0:9] == 255).all()
    res = sc.information_layer(stride_cells=3, n_yaw=4, window=(0, 0, 9, 7), want_per_yaw=True)       # all unknown
    assert (res.n_scored, res.n_changed) == (0, 0) and res.info.shape == (3, 3) and np.isnan(res.info).all()
    assert (res.anchor_cell == -1).all() and np.isnan(res.info_per_yaw).all() and res.pose7.shape == (0, 7)
    lethal = np.full((20, 30), 254, dtype=np.uint8)
    lethal[3:6, 4:9] = 253
    sc.upload_grid(lethal, ORIGIN, RES)
    res = sc.information_layer(stride_cells=4, n_yaw=2)
    assert (res.n_scored, res.n_changed) == (0, 0) and np.isnan(res.info).all()
    np.testing.assert_array_equal(_grid_of(sc), lethal)


def _ray_kw(w):
    return dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=(-1e300, -1e300, 1e300, 1e300))


def _derived(sc, goals, robot, poses):
    out = {}
    a = sc.score_arrival(goals)
    for k in ("status", "arrival", "argmax", "achievable", "ray_counts"):
        out["arrival." + k] = a[k]
    pose = np.array([robot[0], robot[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    p = sc.plan_paths(pose, goals)
    for k in ("achievable", "path_length", "path_length_m"):
        out["plan." + k] = p[k]
    rec, every = sc.search_frontiers(robot)
    out["search.records"], out["search.every"] = rec, every
    f = sc.score_fim(poses, info_only=True)
    out["fim.info_ref"], out["fim.n_voxels"] = f["info_ref"], f["n_voxels"]
    return out


@pytest.mark.parametrize("layout", [1, 2])
def test_derived_state_equals_a_snapshot_of_the_resulting_map(fs, layout):
    """arrival scoring (byte walk and class image), the grid planner, the frontier search and fs_score_fim after the layer == on a
    fresh context given the resulting grid; the plan after the layer is not the plan before it (no stale field)"""
    w = fs.synth.make_small_2d(301, n=96, n_cand=8, n_landmarks=20)
    cells, lm = L.layer_map("130x70")
    rng = np.random.default_rng(11)
    free = np.argwhere(cells == 0)
    pick = free[rng.choice(free.shape[0], 40, replace=False)]
    goals = np.zeros((40, 3))
    goals[:, 0] = ORIGIN[0] + (pick[:, 1] + 0.5) * RES
    goals[:, 1] = ORIGIN[1] + (pick[:, 0] + 0.5) * RES
    robot = (float(goals[0, 0]), float(goals[0, 1]))
    poses = np.zeros((40, 7))
    poses[:, :3] = goals
    poses[:, 6] = 1.0
    dev, ref = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for sc in (dev, ref):
            sc.set_option("ray.layout", layout)
            sc.set_ray_params(**_ray_kw(w))
            sc.upload_landmarks(lm)
            sc.lookup_generate()
        dev.upload_grid(cells, ORIGIN, RES)
        mx = dev.max_arrival()
        before = _derived(dev, goals, robot, poses)                      # (every derived image exists before the cells change)
        dev.information_layer(stride_cells=5, n_yaw=4, info_lo=LO, info_hi=HI, max_cost=252)
        res = dev.information_layer(stride_cells=3, n_yaw=2, reduce="min", info_lo=LO, info_hi=HI, max_cost=200, window=(3, 5, 70, 40))
        assert res.n_changed > 0
        grid = _grid_of(dev)
        ref.upload_grid(grid, ORIGIN, RES)
        ref.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        got, want = _derived(dev, goals, robot, poses), _derived(ref, goals, robot, poses)
        assert got.keys() == want.keys()
        for k in want:
            if k == "fim.info_ref":                                      # (float sums of two calls: CALL_REL)
                assert _within_bar(got[k], want[k].astype(np.float64)) <= CALL_REL and _within_bar(before[k], want[k].astype(np.float64)) <= CALL_REL
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert not np.array_equal(before["plan.path_length_m"], want["plan.path_length_m"])
    finally:
        dev.close(); ref.close()


def test_multi_scorer_equals_the_single_context(fs):
    cells, lm = L.layer_map("96x80")
    one, multi = fs.FrontierScorer(device=0), fs.MultiScorer([0, 0])
    try:
        for sc in (one, multi):
            sc.upload_grid(cells, ORIGIN, RES)
            sc.upload_landmarks(lm)
            sc.lookup_generate()
            sc.set_fim_params(*VIS[0])
        kw = dict(stride_cells=5, n_yaw=4, reduce="mean", window=(3, 2, 90, 71), want_per_yaw=True, **COARSE)
        a, b = one.information_layer(**kw), multi.information_layer(**kw)
        for k in ("anchor_cell", "quat_zw", "pose7"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
        _same_values(a.info, b.info)
        _same_values(a.info_per_yaw, b.info_per_yaw)
        assert (a.n_scored, a.n_changed) == (b.n_scored, b.n_changed) and a.n_changed > 0
        grid = _grid_of(one)
        ny, nx = cells.shape
        for i in range(2):
            got = np.zeros((ny, nx), dtype=np.uint8)
            assert multi._L.fs_read_grid_region(multi.member(i), 0, 0, 0, nx, ny, 1, got.ctypes.data_as(C.c_void_p), nx, nx * ny) == 0
            np.testing.assert_array_equal(got, grid, err_msg=f"member {i}")
        with pytest.raises(fs.capi.FsError) as e:
            multi.information_layer(stride_cells=0)
        assert e.value.code == FS_E_INVALID
    finally:
        one.close(); multi.close()
