"""The inflation layer on the device against tests/inflation_ref.py, byte for byte: the reference's three parameter
sets, windows, unknown cells, the counters, the cost table, refusals, everything derived from the inflated grid, the multi scorer.
Maps are 96 x 96, 160 x 128 (not a multiple of 64 wide) and 200 x 72: with R = 100 the radius exceeds the 96-cell side and the
72-row map, every column tile has a partial wavefront, and every map has more rows than one LDS chunk of the column pass."""
import numpy as np
import pytest

import inflation_ref as I
import keepout_ref as K

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
RES = I.RES
ORIGIN = (-1.0, -2.0, 0.0)
SHAPES = {"96": (96, 96), "160x128": (128, 160), "200x72": (72, 200)}                       # (ny, nx)
PARAMS = {"global": I.GLOBAL, "local": I.LOCAL, "lethal": I.LETHAL_LAYER, "inscribed_beyond": (0.3, 0.6, 0.6), "zero": (0.0, 0.05, 0.6),
          "r500": (25.0, 0.05, 0.6)}


@pytest.fixture(scope="module")
def maps():
    return {name: I.grid(20 + k, ny, nx) for k, (name, (ny, nx)) in enumerate(SHAPES.items())}


@pytest.fixture(scope="module")
def whole(maps):
    """{(map, params): inflate_exact over the whole map}, computed once"""
    return {(m, p): I.inflate_exact(cells, PARAMS[p]) for m, cells in maps.items() for p in PARAMS}


@pytest.fixture(scope="module")
def s(fs):
    sc = fs.FrontierScorer(device=0)
    yield sc
    sc.close()


def _grid_of(s):
    return s.read_grid_region()[0]


@pytest.mark.parametrize("p", list(PARAMS))
@pytest.mark.parametrize("m", list(SHAPES))
def test_whole_map(s, maps, whole, m, p):
    cells = maps[m]
    want, n_seeds, n_changed = whole[m, p]
    s.upload_grid(cells, ORIGIN, RES)
    assert s.inflate(*PARAMS[p]) == (n_seeds, n_changed)
    np.testing.assert_array_equal(_grid_of(s), want)
    if p == "zero":
        assert (n_seeds, n_changed) == (0, 0)
    else:
        assert n_seeds == int((cells == 254).sum()) > 0 and n_changed > 0
        assert s.inflate(*PARAMS[p]) == (n_seeds, 0)                                          # idempotent
        np.testing.assert_array_equal(_grid_of(s), want)
    R, table = s.inflation_costs(*PARAMS[p])
    want_R, want_table = I.cost_table(PARAMS[p], RES)
    assert R == want_R
    np.testing.assert_array_equal(table, want_table)


def test_cost_table_at_other_resolutions(s, maps):
    for res in (0.05, 0.1, 0.025, 0.0731):
        s.upload_grid(maps["96"], ORIGIN, res)
        for params in (I.GLOBAL, I.LOCAL, (1.7, 0.33, 3.0), (0.5, 0.0, 10.0)):
            R, table = s.inflation_costs(*params)
            want_R, want_table = I.cost_table(params, res)
            assert R == want_R
            np.testing.assert_array_equal(table, want_table)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("p", ["global", "local"])
def test_unknown_cells(s, maps, p, flag):
    cells = maps["160x128"]
    want, n_seeds, n_changed = I.inflate_exact(cells, PARAMS[p], inflate_unknown=flag)
    was_unknown = cells == 255
    if flag:
        assert ((want < 253) & was_unknown).sum() > 100
    else:
        assert not ((want < 253) & was_unknown).any() and ((want == 253) & was_unknown).sum() >= 5
    s.upload_grid(cells, ORIGIN, RES)
    assert s.inflate(*PARAMS[p], inflate_unknown=flag) == (n_seeds, n_changed)
    np.testing.assert_array_equal(_grid_of(s), want)


def _windows(ny, nx):
    return {"one_cell": (nx // 2 + 1, ny // 2 - 3, 1, 1), "odd": (13, 7, 37, 21), "corner_lo": (0, 0, 29, 17), "corner_hi": (nx - 23, ny - 31, 23, 31),
            "tile_plus": (3, 5, 65, 17), "empty": (9, 9, 0, 5)}


@pytest.mark.parametrize("p", ["global", "local", "lethal"])
@pytest.mark.parametrize("m", list(SHAPES))
def test_windows(s, maps, whole, m, p):
    cells = maps[m]
    ny, nx = cells.shape
    full = whole[m, p][0]
    for name, win in _windows(ny, nx).items():
        x0, y0, sx, sy = win
        want, n_seeds, n_changed = I.inflate_exact(cells, PARAMS[p], window=win)
        inside = cells.copy()
        inside[y0:y0 + sy, x0:x0 + sx] = full[y0:y0 + sy, x0:x0 + sx]
        np.testing.assert_array_equal(want, inside)                                           # (a window is the whole map's result inside it)
        s.upload_grid(cells, ORIGIN, RES)
        assert s.inflate(*PARAMS[p], window=win) == (n_seeds, n_changed), name
        np.testing.assert_array_equal(_grid_of(s), want, err_msg=name)


@pytest.mark.parametrize("p", ["global", "local"])
def test_seeds_outside_the_window_only(s, p):
    cells = I.single_wall(128, 160)                                                           # the wall is row 64
    win = (21, 66, 101, 9)
    assert not (cells[66:75, 21:122] == 254).any()
    want, n_seeds, n_changed = I.inflate_exact(cells, PARAMS[p], window=win)
    assert n_seeds > 0 and n_changed == 101 * 9
    s.upload_grid(cells, ORIGIN, RES)
    assert s.inflate(*PARAMS[p], window=win) == (n_seeds, n_changed)
    np.testing.assert_array_equal(_grid_of(s), want)
    # ... and a window no seed reaches
    win = (100, 0, 40, 64 - I.cell_radius(PARAMS[p]) if p == "local" else 0)
    s.upload_grid(cells, ORIGIN, RES)
    got = s.inflate(*PARAMS[p], window=win)
    assert got == I.inflate_exact(cells, PARAMS[p], window=win)[1:] and got[1] == 0
    np.testing.assert_array_equal(_grid_of(s), cells)


def test_a_map_without_a_seed(s):
    for ny, nx in SHAPES.values():
        cells = I.no_seed(ny, nx)
        assert not (cells == 254).any() and (cells == 255).any() and (cells == 253).any()
        s.upload_grid(cells, ORIGIN, RES)
        for p in ("global", "lethal"):
            assert s.inflate(*PARAMS[p], inflate_unknown=True) == (0, 0)
        np.testing.assert_array_equal(_grid_of(s), cells)


def test_two_radii_compose_by_max(s, maps, whole):
    cells = maps["160x128"]
    a, b = whole["160x128", "global"][0], whole["160x128", "lethal"][0]
    both = I.inflate_exact(a, I.LETHAL_LAYER)[0]
    known = cells != 255
    np.testing.assert_array_equal(both[known], np.maximum(a, b)[known])
    s.upload_grid(cells, ORIGIN, RES)
    s.inflate(*I.GLOBAL)
    s.inflate(*I.LETHAL_LAYER)
    np.testing.assert_array_equal(_grid_of(s), both)
    s.upload_grid(cells, ORIGIN, RES)                                                         # the other order: the same known cells
    s.inflate(*I.LETHAL_LAYER)
    s.inflate(*I.GLOBAL)
    np.testing.assert_array_equal(_grid_of(s)[known], both[known])


def test_a_keepout_zone_stays_253(fs, maps):
    cells = maps["96"]
    origin = (0.0, 0.0, 0.0)
    zone = (K.FOV, 0.52, 2.42, 0.0, 3.5)
    mask, n_cells = K.zone_masks([zone], (96, 96, 0.0, 0.0, RES))
    marked = K.mark(cells, [zone], origin, RES)
    s = fs.FrontierScorer(device=0)
    try:
        s.upload_grid(cells, origin, RES)
        s.keepout_add_fov(*zone[1:])
        for params in (I.GLOBAL, I.LETHAL_LAYER):
            want, n_seeds, n_changed = I.inflate_exact(marked, params)
            s.upload_grid(cells, origin, RES)                                                 # (staged again: the zone is painted by the upload)
            assert s.inflate(*params) == (n_seeds, n_changed)
            got = _grid_of(s)
            np.testing.assert_array_equal(got, want)
            assert n_cells[0] > 1000 and (got[mask == 1] == 253).all()
        # a window rewritten afterwards: the zone is repainted by the update, the inflation on top leaves it
        s.update_grid_region(30, 30, 0, cells[30:60, 30:70])
        s.inflate(*I.LOCAL, window=(30, 30, 40, 30))
        assert (_grid_of(s)[mask == 1] == 253).all()
    finally:
        s.close()


def test_refusals_leave_the_grid_alone(fs, maps):
    cells = maps["160x128"]
    ny, nx = cells.shape
    nan, inf = float("nan"), float("inf")
    s = fs.FrontierScorer(device=0)
    try:
        for call in (lambda: s.inflate(*I.GLOBAL, window=(0, 0, 1, 1)), lambda: s.inflation_costs(*I.GLOBAL)):
            with pytest.raises(fs.capi.FsError) as e:
                call()
            assert e.value.code == FS_E_STATE
        s.upload_grid(cells, ORIGIN, RES)
        bad_params = [(nan, 0.05, 0.6), (5.0, nan, 0.6), (5.0, 0.05, nan), (inf, 0.05, 0.6), (5.0, inf, 0.6), (5.0, 0.05, inf),
                      (-0.1, 0.05, 0.6), (5.0, -0.05, 0.6), (5.0, 0.05, -0.6), (513 * RES, 0.05, 0.6), (1e300, 0.05, 0.6)]
        for params in bad_params:
            for call in (lambda: s.inflate(*params), lambda: s.inflation_costs(*params)):
                with pytest.raises(fs.capi.FsError) as e:
                    call()
                assert e.value.code == FS_E_INVALID, params
        for win in ((-1, 0, 4, 4), (0, -1, 4, 4), (nx - 3, 0, 4, 4), (0, ny - 3, 4, 4), (nx, 0, 1, 1), (0, 0, nx + 1, ny), (0, 0, -1, 4), (0, 0, 4, -1),
                    (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
            with pytest.raises(fs.capi.FsError) as e:
                s.inflate(*I.LOCAL, window=win)
            assert e.value.code == FS_E_INVALID, win
        np.testing.assert_array_equal(_grid_of(s), cells)
        assert s.inflate(512 * RES, 0.05, 0.6, window=(5, 5, 0, 0)) == (0, 0)                 # the largest radius is taken
        vol = np.random.default_rng(1).integers(0, 256, size=(3, 40, 56), dtype=np.uint8)
        s.upload_grid(vol, ORIGIN, RES)
        for call in (lambda: s.inflate(*I.LOCAL, window=(0, 0, 4, 4)), lambda: s.inflation_costs(*I.LOCAL)):
            with pytest.raises(fs.capi.FsError) as e:
                call()
            assert e.value.code == FS_E_INVALID
            assert str(e.value) == f"fitslam_frontier error {FS_E_INVALID}: the inflation layer is defined on a 2-D costmap (nz == 1)"
        np.testing.assert_array_equal(s.read_grid_region(), vol)
    finally:
        s.close()


def _ray_kw(w):
    return dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=(-1e300, -1e300, 1e300, 1e300))


def _derived(s, goals, robot):
    out = {}
    a = s.score_arrival(goals)
    for k in ("status", "arrival", "argmax", "achievable", "ray_counts"):
        out["arrival." + k] = a[k]
    pose = np.array([robot[0], robot[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    p = s.plan_paths(pose, goals)
    for k in ("achievable", "path_length", "path_length_m"):
        out["plan." + k] = p[k]
    r = s.refine_paths(np.tile(np.asarray(robot), (goals.shape[0], 1)), goals[:, :2])
    out["refine.status"], out["refine.cost"] = r["status"], r["cost"]
    out["refine.vertices"] = np.concatenate([v.reshape(-1, 2) for v in r["vertices"]] + [np.zeros((0, 2))])
    out["refine.poses"] = np.concatenate([v.reshape(-1, 2) for v in r["poses"]] + [np.zeros((0, 2))])
    rec, every = s.search_frontiers(robot)
    out["search.records"], out["search.every"] = rec, every
    return out


@pytest.mark.parametrize("layout", [1, 2])
def test_derived_state_equals_a_snapshot_of_the_host_inflated_map(fs, maps, layout):
    """arrival scoring (byte walk and class image, whose bricks are re-cut under the inflated window), the grid planner, the
    any-angle refinement and the frontier search after fs_inflate == on a fresh context given the host-inflated map"""
    w = fs.synth.make_small_2d(301, n=96, n_cand=8, n_landmarks=20)
    cells = maps["160x128"]
    rng = np.random.default_rng(11)
    inflated = I.inflate_exact(I.inflate_exact(cells, I.LOCAL)[0], I.LOCAL, window=(3, 5, 70, 40), inflate_unknown=True)[0]
    free = np.argwhere(inflated < 100)
    pick = free[rng.choice(free.shape[0], 40, replace=False)]
    goals = np.zeros((40, 3))
    goals[:, 0] = ORIGIN[0] + (pick[:, 1] + 0.5) * RES
    goals[:, 1] = ORIGIN[1] + (pick[:, 0] + 0.5) * RES
    robot = (float(goals[0, 0]), float(goals[0, 1]))
    dev, ref = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for sc in (dev, ref):
            sc.set_option("ray.layout", layout)
            sc.set_ray_params(**_ray_kw(w))
        dev.upload_grid(cells, ORIGIN, RES)
        mx = dev.max_arrival()
        before = _derived(dev, goals, robot)                              # (every derived image exists before the cells change)
        dev.inflate(*I.LOCAL)
        dev.inflate(*I.LOCAL, window=(3, 5, 70, 40), inflate_unknown=True)
        np.testing.assert_array_equal(dev.read_grid_region()[0], inflated)
        ref.upload_grid(inflated, ORIGIN, RES)
        ref.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        got, want = _derived(dev, goals, robot), _derived(ref, goals, robot)
        assert got.keys() == want.keys()
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        # ... and the inflation changed what is derived: the comparison is not vacuous
        assert not np.array_equal(before["arrival.ray_counts"], want["arrival.ray_counts"])
        assert not np.array_equal(before["refine.cost"], want["refine.cost"])
    finally:
        dev.close(); ref.close()


def test_multi_scorer_equals_the_single_context(fs, maps, whole):
    cells = maps["200x72"]
    w = fs.synth.make_small_2d(301, n=96, n_cand=8, n_landmarks=20)
    free = np.argwhere(cells == 0)
    pick = free[np.random.default_rng(5).choice(free.shape[0], 30, replace=False)]
    goals = np.zeros((30, 3))
    goals[:, 0] = ORIGIN[0] + (pick[:, 1] + 0.5) * RES
    goals[:, 1] = ORIGIN[1] + (pick[:, 0] + 0.5) * RES
    one, multi = fs.FrontierScorer(device=0), fs.MultiScorer([0, 0])
    try:
        for sc in (one, multi):
            sc.set_ray_params(**_ray_kw(w))
            sc.upload_grid(cells, ORIGIN, RES)
        mx = one.max_arrival()
        multi.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        want, n_seeds, n_changed = whole["200x72", "global"]
        assert one.inflate(*I.GLOBAL) == multi.inflate(*I.GLOBAL) == (n_seeds, n_changed)
        win = (17, 3, 90, 40)
        assert one.inflate(*I.LETHAL_LAYER, window=win, inflate_unknown=True) == multi.inflate(*I.LETHAL_LAYER, window=win, inflate_unknown=True)
        np.testing.assert_array_equal(_grid_of(one), I.inflate_exact(want, I.LETHAL_LAYER, window=win, inflate_unknown=True)[0])
        a, b = one.score_arrival(goals), multi.score_arrival(goals, n_rays_total=one.n_elev * one.n_yaw)
        for k in ("status", "arrival", "argmax", "achievable", "yaw"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a["ray_counts"].reshape(30, -1), b["ray_counts"])
        with pytest.raises(fs.capi.FsError) as e:
            multi.inflate(float("nan"), 0.05, 0.6)
        assert e.value.code == FS_E_INVALID
    finally:
        one.close(); multi.close()
