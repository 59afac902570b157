"""Keep-out zones on the staged grid: the reference's costmap layer LethalMarker and the behaviour-tree node
MarkLethalFOV on the device, against the line-cited restatement tests/keepout_ref.py — cell sets, the painted grid, everything
derived from it, persistence across staging calls, and the rules of the interface.  Grids are 96 x 96 and 160 x 128: the
smallest that hold a 70-cell fan both clear of and clipped by the border and span several 8 x 8 bricks and partial rows of
four cells."""
import math

import numpy as np
import pytest

import keepout_ref as K

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
RES = 0.05
ANCHOR = (K.FOV, 0.52, 2.42, 0.0, 3.5)               # on 96 x 96 at origin (0, 0): apex cell (10, 48), 1 188 distinct cells


def _grid(seed, ny, nx):
    """a costmap with a known interior, lethal blocks and unknown patches: frontiers, obstacles and plannable free space"""
    rng = np.random.default_rng(seed)
    cells = np.full((ny, nx), 255, np.uint8)
    cells[6:ny - 6, 6:nx - 6] = 0
    for _ in range(7):
        y, x = int(rng.integers(8, ny - 16)), int(rng.integers(8, nx - 16))
        cells[y:y + int(rng.integers(2, 7)), x:x + int(rng.integers(2, 9))] = int(rng.choice([254, 253, 200]))
    for _ in range(5):
        y, x = int(rng.integers(8, ny - 16)), int(rng.integers(8, nx - 16))
        cells[y:y + int(rng.integers(3, 10)), x:x + int(rng.integers(3, 10))] = 255
    return cells


def _geom(cells, origin):
    return (cells.shape[1], cells.shape[0], float(origin[0]), float(origin[1]), RES)


def _add(s, zone):
    if zone[0] == K.FOV:
        return s.keepout_add_fov(zone[1], zone[2], zone[3], zone[4])
    return s.keepout_add_disc(zone[1], zone[2], zone[4])


def _random_zones(rng, n, geom, margin=0.3):
    nx, ny, ox, oy, res = geom
    zones = []
    for _ in range(n):
        wx = float(rng.uniform(ox - margin, ox + nx * res + margin))
        wy = float(rng.uniform(oy - margin, oy + ny * res + margin))
        if rng.random() < 0.15:
            zones.append((K.DISC, wx, wy, 0.0, float(rng.choice([0.5, 1.0, 1.7]))))
        else:
            yaw = float(rng.integers(-4, 5)) * (math.pi / 2) if rng.random() < 0.2 else float(rng.uniform(-2 * math.pi, 2 * math.pi))
            zones.append((K.FOV, wx, wy, yaw, float(rng.choice([3.5, 3.5, 1.0]))))
    return zones


def _check_layer(s, zones, geom, returned=None):
    spec, n_cells, mask = s.keepout_get()
    want_mask, want_cells = K.zone_masks(zones, geom)
    assert spec.shape == (len(zones), 5)
    np.testing.assert_array_equal(spec, np.array(zones, dtype=np.float64).reshape(-1, 5))
    np.testing.assert_array_equal(n_cells, want_cells)
    np.testing.assert_array_equal(mask, want_mask)
    if returned is not None:
        assert [r[0] for r in returned] == list(range(len(zones)))
        np.testing.assert_array_equal([r[1] for r in returned], want_cells)
    return want_mask, want_cells


def _painted(cells, mask):
    """markCells with the restatement's union mask"""
    return np.where(mask == 1, K.COST, cells).astype(np.uint8)


CASES = {
    "anchor": ((96, 96), (0.0, 0.0, 0.0), [ANCHOR]),
    "clipped_corner": ((96, 96), (0.0, 0.0, 0.0), [(K.FOV, 4.3, 4.4, 0.6, 3.5), (K.FOV, 0.3, 0.2, -2.2, 3.5)]),
    "off_map": ((96, 96), (-1.0, -2.0, 0.0), [(K.FOV, float(np.nextafter(-1.0, -2.0)), 0.0, 0.0, 3.5), (K.FOV, 3.81, 0.0, 3.0, 3.5), (K.DISC, 0.0, 2.85, 0.0, 1.7)]),
    "disc": ((96, 96), (0.0, 0.0, 0.0), [(K.DISC, 2.4, 2.4, 0.0, 1.7)]),
    "disc_border": ((128, 160), (-3.0, -1.0, 0.0), [(K.DISC, -2.9, 2.0, 0.0, 1.7), (K.DISC, 4.9, 5.3, 0.0, 1.7)]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cell_sets(fs, case):
    (ny, nx), origin, zones = CASES[case]
    cells = _grid(1, ny, nx)
    s = fs.FrontierScorer(device=0)
    try:
        s.upload_grid(cells, origin, RES)
        returned = [_add(s, z) for z in zones]
        want_mask, want_cells = _check_layer(s, zones, _geom(cells, origin), returned)
        if case == "anchor":
            assert want_cells[0] == 1188
        if case == "off_map":
            assert want_cells.tolist() == [0, 0, 0]
        else:
            assert want_cells.min() > 0
        np.testing.assert_array_equal(s.read_grid_region(), K.mark(cells, zones, origin, RES)[None])
        np.testing.assert_array_equal(s.read_grid_region()[0], _painted(cells, want_mask))
    finally:
        s.close()


def test_cell_sets_of_200_random_zones_in_one_context(fs):
    cells = _grid(2, 128, 160)
    origin = (-3.0, -1.0, 0.0)
    geom = _geom(cells, origin)
    zones = _random_zones(np.random.default_rng(7), 200, geom)
    s = fs.FrontierScorer(device=0)
    try:
        s.upload_grid(cells, origin, RES)
        returned = [_add(s, z) for z in zones]
        want_mask, want_cells = _check_layer(s, zones, geom, returned)
        assert (want_cells == 0).sum() >= 5 and (want_cells > 500).sum() >= 50          # off-map apexes and whole fans
        np.testing.assert_array_equal(s.read_grid_region()[0], _painted(cells, want_mask))
    finally:
        s.close()


def test_read_grid_region_round_trip(fs):
    """without zones the staged grid reads back as it went in: whole map, windows at odd offsets, a strided window into a larger
    host array, a 3-D grid; a window that leaves the grid is refused"""
    rng = np.random.default_rng(3)
    s = fs.FrontierScorer(device=0)
    try:
        with pytest.raises(fs.capi.FsError) as e:
            s.read_grid_region(0, 0, 0, shape=(4, 4))
        assert e.value.code == FS_E_STATE
        cells = rng.integers(0, 256, size=(128, 160), dtype=np.uint8)
        s.upload_grid(cells, (0.0, 0.0, 0.0), RES)
        np.testing.assert_array_equal(s.read_grid_region(), cells[None])
        for x0, y0, sx, sy in ((0, 0, 1, 1), (3, 5, 61, 17), (159, 127, 1, 1), (37, 0, 123, 128), (8, 8, 64, 64)):
            np.testing.assert_array_equal(s.read_grid_region(x0, y0, 0, shape=(sy, sx)), cells[y0:y0 + sy, x0:x0 + sx])
        big = np.full((200, 300), 7, np.uint8)
        s.read_grid_region(11, 13, 0, out=big[50:50 + 40, 100:100 + 90])
        want = np.full((200, 300), 7, np.uint8)
        want[50:90, 100:190] = cells[13:53, 11:101]
        np.testing.assert_array_equal(big, want)
        for x0, y0, z0, shape in ((158, 0, 0, (1, 1, 3)), (0, 127, 0, (1, 2, 1)), (0, 0, 1, (1, 1, 1)), (-1, 0, 0, (1, 1, 1))):
            with pytest.raises(fs.capi.FsError) as e:
                s.read_grid_region(x0, y0, z0, shape=shape)
            assert e.value.code == FS_E_INVALID
        vol = rng.integers(0, 256, size=(5, 33, 47), dtype=np.uint8)
        s.upload_grid(vol, (0.0, 0.0, 0.0), RES)
        np.testing.assert_array_equal(s.read_grid_region(), vol)
        np.testing.assert_array_equal(s.read_grid_region(5, 7, 1, shape=(3, 20, 31)), vol[1:4, 7:27, 5:36])
        host = np.zeros((6, 40, 50), np.uint8)
        s.read_grid_region(0, 0, 0, out=host[1:6, 2:35, 3:50])
        np.testing.assert_array_equal(host[1:6, 2:35, 3:50], vol)
        assert host[0].sum() == 0 and host[:, :2].sum() == 0 and host[:, :, :3].sum() == 0
    finally:
        s.close()


def _ray_kw(w):
    return dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=(-1e300, -1e300, 1e300, 1e300))


def _derived(s, cells, origin, goals, robot):
    ny, nx = cells.shape
    out = {}
    a = s.score_arrival(goals)
    for k in ("status", "arrival", "argmax", "achievable", "ray_counts"):
        out["arrival." + k] = a[k]
    mask, count = s.frontier_cells((1, ny, nx), 160)
    out["frontier.mask"], out["frontier.count"] = mask, np.array([count])
    n = goals.shape[0]
    t = s.trace_segments(np.roll(goals, 1, axis=0), goals, 400.0)
    for k, v in t.items():
        out["trace." + k] = v
    pose = np.array([robot[0], robot[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    p = s.plan_paths(pose, goals)
    for k in ("achievable", "path_length", "path_length_m"):
        out["plan." + k] = p[k]
    rec, every = s.search_frontiers(robot)
    out["search.records"], out["search.every"] = rec, every
    assert n > 0
    return out


@pytest.mark.parametrize("layout", [1, 2])
def test_derived_images_equal_a_snapshot_of_the_host_marked_map(fs, layout):
    """frontier cells, the ray fan (byte walk and class image, whose bricks are re-cut under a new zone), segment traces, the
    grid planner and the frontier search on a device-marked context == on a fresh context given the host-marked map"""
    w = fs.synth.make_small_2d(301, n=96, n_cand=8, n_landmarks=20)
    cells = _grid(4, 128, 160)
    origin = (-3.0, -1.0, 0.0)
    geom = _geom(cells, origin)
    rng = np.random.default_rng(11)
    free = np.argwhere(cells == 0)
    pick = free[rng.choice(free.shape[0], 60, replace=False)]
    goals = np.zeros((60, 3))
    goals[:, 0] = origin[0] + (pick[:, 1] + 0.5) * RES
    goals[:, 1] = origin[1] + (pick[:, 0] + 0.5) * RES
    robot = (float(goals[0, 0]), float(goals[0, 1]))
    zones = [(K.FOV, 0.0, 2.0, 0.4, 3.5), (K.FOV, 1.0, 2.5, 2.9, 3.5), (K.DISC, 2.0, 1.0, 0.0, 1.7), (K.FOV, 4.6, 5.0, 1.0, 3.5)]
    dev, ref = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (dev, ref):
            s.set_option("ray.layout", layout)
            s.set_ray_params(**_ray_kw(w))
        dev.upload_grid(cells, origin, RES)
        mx = dev.max_arrival()
        dev.score_arrival(goals)                                   # (the class image exists before the zones arrive)
        for z in zones:
            _add(dev, z)
        marked = K.mark(cells, zones, origin, RES)
        assert (marked != cells).sum() > 1000
        ref.upload_grid(marked, origin, RES)
        ref.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        got, want = _derived(dev, cells, origin, goals, robot), _derived(ref, cells, origin, goals, robot)
        assert got.keys() == want.keys()
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        # ... and the zones changed what is derived: the comparison is not vacuous
        plain = fs.FrontierScorer(device=0)
        try:
            plain.set_option("ray.layout", layout)
            plain.set_ray_params(**_ray_kw(w))
            plain.upload_grid(cells, origin, RES)
            plain.set_arrival_limits(mx["max_gt"], mx["min_gt"])
            base = _derived(plain, cells, origin, goals, robot)
        finally:
            plain.close()
        assert not np.array_equal(base["arrival.ray_counts"], want["arrival.ray_counts"])
        assert not np.array_equal(base["trace.hit"], want["trace.hit"])
    finally:
        dev.close(); ref.close()


def test_zones_persist_across_staging_calls(fs):
    cells = _grid(5, 96, 96)
    origin = (0.0, 0.0, 0.0)
    geom = _geom(cells, origin)
    s = fs.FrontierScorer(device=0)
    try:
        s.upload_grid(cells, origin, RES)
        _add(s, ANCHOR)
        mask, _ = _check_layer(s, [ANCHOR], geom)
        # a window of zeros over half the zone (apex cell (10, 48), base at x = 80): zone cells 253, the rest of the window 0
        x0, y0, sx, sy = 43, 11, 50, 70
        s.update_grid_region(x0, y0, 0, np.zeros((sy, sx), np.uint8))
        want = K.mark(cells, [ANCHOR], origin, RES)
        want[y0:y0 + sy, x0:x0 + sx] = np.where(mask[y0:y0 + sy, x0:x0 + sx] == 1, 253, 0)
        got = s.read_grid_region()[0]
        np.testing.assert_array_equal(got, want)
        win = got[y0:y0 + sy, x0:x0 + sx]
        assert (win == 253).sum() == mask[y0:y0 + sy, x0:x0 + sx].sum() > 300 and set(np.unique(win)) == {0, 253}
        # a new snapshot comes back marked
        other = _grid(6, 96, 96)
        s.upload_grid(other, origin, RES)
        np.testing.assert_array_equal(s.read_grid_region()[0], K.mark(other, [ANCHOR], origin, RES))
        # the origin shifted by 1.0 m: the restatement's mask at the new geometry (matchSize)
        moved = (1.0, 0.0, 0.0)
        s.upload_grid(other, moved, RES)
        moved_mask, moved_cells = _check_layer(s, [ANCHOR], _geom(other, moved))
        assert moved_cells[0] == 0                                           # (0.52 < 1.0: the apex left the map)
        moved = (-1.0, 1.0, 0.0)
        s.upload_grid(other, moved, RES)
        moved_mask, moved_cells = _check_layer(s, [ANCHOR], _geom(other, moved))
        assert moved_cells[0] > 0 and not np.array_equal(moved_mask, mask)
        np.testing.assert_array_equal(s.read_grid_region()[0], K.mark(other, [ANCHOR], moved, RES))
        # an origin that puts the apex off the map: no cells, the zone is kept; restoring the origin brings them back
        s.upload_grid(other, (5.0, 5.0, 0.0), RES)
        spec, n_cells, m = s.keepout_get()
        assert spec.shape[0] == 1 and n_cells[0] == 0 and m.sum() == 0
        np.testing.assert_array_equal(s.read_grid_region()[0], other)
        s.upload_grid(other, origin, RES)
        _check_layer(s, [ANCHOR], geom)
        np.testing.assert_array_equal(s.read_grid_region()[0], K.mark(other, [ANCHOR], origin, RES))
        # another shape and resolution
        small = _grid(7, 40, 56)
        s.upload_grid(small, origin, 0.1)
        g2 = (56, 40, 0.0, 0.0, 0.1)
        m2, c2 = K.zone_masks([ANCHOR], g2)
        spec, n_cells, m = s.keepout_get()
        np.testing.assert_array_equal(m, m2)
        assert n_cells[0] == c2[0] > 0
        # a brick upload is a 3-D snapshot (its dimensions are multiples of 8): staged unmarked, the zone kept
        s.upload_grid_bricks((8, 96, 96), origin, RES, np.array([[2, 5, 0]], np.int32), np.zeros((1, 512), np.uint8), default_value=255)
        sparse = np.full((8, 96, 96), 255, np.uint8)
        sparse[:, 40:48, 16:24] = 0
        np.testing.assert_array_equal(s.read_grid_region(), sparse)
        spec, n_cells, m = s.keepout_get()
        assert spec.shape[0] == 1 and n_cells[0] == 0 and m.sum() == 0
        s.upload_grid(cells, origin, RES)
        _check_layer(s, [ANCHOR], geom)
    finally:
        s.close()


def test_a_zone_outside_the_window_is_on_the_grid(fs):
    """The gap this layer closes: LethalMarker::updateCosts ignores the cycle's bounds.  A zone is added, then a window that does
    not touch it is updated: the device grid equals the host master grid after the layer's cycle.  Without the zone call (what a
    caller who forwards windows only gets) it does not."""
    cells = _grid(8, 96, 96)
    origin = (0.0, 0.0, 0.0)
    window = np.full((10, 12), 254, np.uint8)
    x0, y0 = 4, 80                                                           # clear of the anchor fan (y 19 ... 76 from x = 10 on)
    host = cells.copy()
    host[y0:y0 + 10, x0:x0 + 12] = window
    host = K.mark(host, [ANCHOR], origin, RES)                               # the layer's cycle on the master grid
    mask, _ = K.zone_masks([ANCHOR], _geom(cells, origin))
    assert mask[y0:y0 + 10, x0:x0 + 12].sum() == 0
    with_zone, without = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (with_zone, without):
            s.upload_grid(cells, origin, RES)
        _add(with_zone, ANCHOR)
        for s in (with_zone, without):
            s.update_grid_region(x0, y0, 0, window)
        np.testing.assert_array_equal(with_zone.read_grid_region()[0], host)
        stale = without.read_grid_region()[0]
        assert (stale != host).sum() == ((mask == 1) & (cells != K.COST)).sum() > 1000
    finally:
        with_zone.close(); without.close()


def _poses(rng, n, geom):
    nx, ny, ox, oy, res = geom
    out = np.zeros((n, 7))
    out[:, 0] = rng.uniform(ox + 0.2, ox + nx * res - 0.2, n)
    out[:, 1] = rng.uniform(oy + 0.2, oy + ny * res - 0.2, n)
    out[:, 2] = rng.uniform(-0.1, 0.1, n)
    yaw = rng.uniform(-math.pi, math.pi, n)
    q = np.stack([rng.normal(0, 0.03, n), rng.normal(0, 0.03, n), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    q[: n // 2, :2] = 0.0                                                    # half of them yaw-only
    q[1] = [0.0, 0.0, 0.0, 1.0]
    q[2] = [0.0, 0.0, 1.0, 0.0]
    out[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    out[3, 3:] *= 2.5                                                        # (quatToEuler normalises)
    return out


def test_mark_lethal_fov(fs, oracle):
    w = fs.synth.make_small_2d(301, n=96, n_cand=8, n_landmarks=20)
    cells = _grid(9, 128, 160)
    origin = (-3.0, -1.0, 0.0)
    geom = _geom(cells, origin)
    rng = np.random.default_rng(13)
    poses = _poses(rng, 50, geom)
    free = np.argwhere(cells == 0)
    pick = free[rng.choice(free.shape[0], 40, replace=False)]
    goals = np.zeros((40, 3))
    goals[:, 0] = origin[0] + (pick[:, 1] + 0.5) * RES
    goals[:, 1] = origin[1] + (pick[:, 0] + 0.5) * RES
    one, multi = fs.FrontierScorer(device=0), fs.MultiScorer([0, 0])
    try:
        for s in (one, multi):
            s.set_ray_params(**_ray_kw(w))
            s.upload_grid(cells, origin, RES)
        mx = one.max_arrival()
        multi.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        zones = []
        for k in range(50):
            zone, black = K.mark_lethal_tick(poses[k], oracle.quat_to_yaw)
            got_black, zid, n_cells = one.mark_lethal_fov(poses[k])
            m_black, m_zid, m_cells = multi.mark_lethal_fov(poses[k])
            zones.append(zone)
            assert zid == m_zid == k
            np.testing.assert_array_equal(got_black, black)
            np.testing.assert_array_equal(m_black, black)
            assert n_cells == m_cells == K.zone_masks([zone], geom)[1][0]
            assert zone[1] == float(np.float32(zone[1])) and zone[2] == float(np.float32(zone[2]))
        want_mask, _ = _check_layer(one, zones, geom)                        # the stored requests are the float-rounded ones, exactly
        np.testing.assert_array_equal(one.read_grid_region()[0], _painted(cells, want_mask))
        a, b = one.score_arrival(goals), multi.score_arrival(goals, n_rays_total=one.n_elev * one.n_yaw)
        for k in ("status", "arrival", "argmax", "achievable", "yaw"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a["ray_counts"].reshape(40, -1), b["ray_counts"])
        for pose in (np.full(7, np.nan), np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])):
            with pytest.raises(fs.capi.FsError) as e:
                one.mark_lethal_fov(pose)
            assert e.value.code == FS_E_INVALID
        assert one.keepout_get()[0].shape[0] == 50
    finally:
        one.close(); multi.close()


def test_rules(fs):
    cells = _grid(10, 96, 96)
    origin = (0.0, 0.0, 0.0)
    geom = _geom(cells, origin)
    s = fs.FrontierScorer(device=0)
    try:
        # a zone added before any grid is stored, and applied at the first upload
        assert _add(s, ANCHOR) == (0, 0)
        spec, n_cells, mask = s.keepout_get()
        assert spec.shape[0] == 1 and n_cells[0] == 0 and mask is None
        s.upload_grid(cells, origin, RES)
        _check_layer(s, [ANCHOR], geom)
        np.testing.assert_array_equal(s.read_grid_region()[0], K.mark(cells, [ANCHOR], origin, RES))
        # non-finite arguments, negative and unconvertible sizes: refused, nothing stored
        for bad in ((K.FOV, 1.0, 1.0, float("nan"), 3.5), (K.FOV, float("inf"), 1.0, 0.0, 3.5), (K.FOV, 1.0, float("nan"), 0.0, 3.5),
                    (K.FOV, 1.0, 1.0, 0.0, float("inf")), (K.FOV, 1.0, 1.0, 0.0, -1.0), (K.FOV, 1.0, 1.0, 0.0, RES * 2.0 ** 31),
                    (K.DISC, 1.0, 1.0, 0.0, float("nan")), (K.DISC, 1.0, 1.0, 0.0, RES * 2.0 ** 31)):
            with pytest.raises(fs.capi.FsError) as e:
                _add(s, bad)
            assert e.value.code == FS_E_INVALID, bad
            text = ("the zone's size is 2^31 cells or more (the reference's conversion to unsigned int is undefined)" if bad[4] == RES * 2.0 ** 31
                    else "a keep-out zone needs a finite position and yaw and a finite size >= 0")
            assert str(e.value) == f"fitslam_frontier error {FS_E_INVALID}: {text}", bad
        assert s.keepout_get()[0].shape[0] == 1
        # a 3-D upload with zones stored is staged unmarked, and refuses a new zone; the zones are kept
        vol = np.random.default_rng(1).integers(0, 256, size=(3, 96, 96), dtype=np.uint8)
        s.upload_grid(vol, origin, RES)
        np.testing.assert_array_equal(s.read_grid_region(), vol)
        spec, n_cells, mask = s.keepout_get()
        assert spec.shape[0] == 1 and n_cells[0] == 0 and mask.sum() == 0
        not_2d = f"fitslam_frontier error {FS_E_INVALID}: keep-out zones are defined on a 2-D costmap (nz == 1)"
        with pytest.raises(fs.capi.FsError) as e:
            _add(s, (K.FOV, 1.0, 1.0, 0.0, 3.5))
        assert e.value.code == FS_E_INVALID and str(e.value) == not_2d
        with pytest.raises(fs.capi.FsError) as e:
            s.mark_lethal_fov([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        assert e.value.code == FS_E_INVALID and str(e.value) == not_2d
        assert s.keepout_get()[0].shape[0] == 1
        s.update_grid_region(0, 0, 1, np.zeros((1, 96, 96), np.uint8))          # (a window of a 3-D grid: no layer)
        assert s.read_grid_region(0, 0, 1, shape=(1, 96, 96)).sum() == 0
        s.upload_grid(cells, origin, RES)                                        # back to 2-D: the kept zone marks again
        _check_layer(s, [ANCHOR], geom)
        # clear, then an upload: no mark (the cells painted before the upload are not restored)
        s.keepout_clear()
        assert (s.read_grid_region()[0] == K.mark(cells, [ANCHOR], origin, RES)).all()
        s.upload_grid(cells, origin, RES)
        np.testing.assert_array_equal(s.read_grid_region()[0], cells)
        spec, n_cells, mask = s.keepout_get()
        assert spec.shape[0] == 0 and mask.sum() == 0
        s.update_grid_region(40, 40, 0, np.zeros((8, 8), np.uint8))
        assert s.read_grid_region(40, 40, 0, shape=(8, 8)).sum() == 0
    finally:
        s.close()


def test_zone_limit(fs):
    """FS_KEEPOUT_MAX_ZONES zones are taken (stored before any grid, all rasterised by the first upload), one more is refused"""
    limit = fs.capi.FS_KEEPOUT_MAX_ZONES
    assert limit >= 1024
    cells = _grid(12, 96, 96)
    origin = (0.0, 0.0, 0.0)
    geom = _geom(cells, origin)
    zones = _random_zones(np.random.default_rng(17), limit, geom, margin=0.1)
    zones = [z if z[0] == K.FOV else (K.FOV, z[1], z[2], 1.0, 1.0) for z in zones]
    s = fs.FrontierScorer(device=0)
    try:
        for z in zones:
            _add(s, z)
        for extra in ((K.FOV, 1.0, 1.0, 0.0, 3.5), (K.DISC, 1.0, 1.0, 0.0, 1.7)):
            with pytest.raises(fs.capi.FsError) as e:
                _add(s, extra)
            assert e.value.code == FS_E_INVALID
        s.upload_grid(cells, origin, RES)
        want_mask, _ = _check_layer(s, zones, geom)
        with pytest.raises(fs.capi.FsError) as e:
            _add(s, (K.FOV, 1.0, 1.0, 0.0, 3.5))
        assert e.value.code == FS_E_INVALID
        assert s.keepout_get(want_mask=False)[0].shape[0] == limit
        np.testing.assert_array_equal(s.read_grid_region()[0], _painted(cells, want_mask))
    finally:
        s.close()


def _snapshot(fs, s, route, cells, origin, res):
    if route == "bricks":
        xyz, bricks = fs.synth.dense_to_bricks(cells, 255)
        s.upload_grid_bricks(cells.shape, origin, res, xyz, bricks, default_value=255)
    else:
        s.upload_grid(cells, origin, res)


def test_the_two_snapshot_routes_are_one(fs):
    """fs_upload_grid and fs_upload_grid_bricks differ in how the cells reach the device and in nothing after that: the map read
    back, the arrival limits and the arrival records are equal, a stored zone is treated alike, a snapshot of the same shape keeps
    the world and one of another shape drops it.  A brick snapshot has whole 8 x 8 x 8 bricks, so the pair is compared on
    16 x 16 x 8; on 64 x 64 x 1 the brick route refuses the shape and changes nothing, and the dense route carries the zone."""
    no_world = f"fitslam_frontier error {FS_E_STATE}: fs_upload_world has not been called"
    w3 = fs.synth.make_workload("C1", n_cand=8, n_landmarks=8)
    kw3 = dict(max_camera_depth=w3.max_camera_depth, delta_theta=w3.delta_theta, camera_fov=w3.camera_fov, robot_radius=w3.robot_radius,
               n_rays=w3.n_yaw, elev=w3.elev, polygon=w3.polygon)
    rng = np.random.default_rng(23)
    res, origin = w3.resolution, (-1.0, -2.0, 0.5)
    values = np.array([0, 0, 0, 0, 254, 255, 255, 253, 100], np.uint8)
    vol, vol2, narrow = rng.choice(values, size=(8, 16, 16)), rng.choice(values, size=(8, 16, 16)), rng.choice(values, size=(8, 16, 8))
    vol[:, 8:, 8:] = 255                                                         # (a brick the list leaves out: the default value)
    goals = (rng.integers(0, (16, 16, 8), size=(12, 3)) + 0.5) * res + np.asarray(origin)
    zone = (K.DISC, origin[0] + 8 * res, origin[1] + 8 * res, 0.0, 3 * res)
    got = {}
    for route in ("dense", "bricks"):
        s = fs.FrontierScorer(device=0)
        try:
            s.set_ray_params(**kw3)
            assert _add(s, zone) == (0, 0)                                       # stored; a 3-D snapshot is staged unmarked
            _snapshot(fs, s, route, vol, origin, res)
            s.upload_world(vol2)
            spec, n_cells, mask = s.keepout_get()
            assert spec.shape[0] == 1 and n_cells[0] == 0 and mask.sum() == 0
            got[route] = dict(grid=s.read_grid_region(), limits=s.max_arrival(), arrival=s.score_arrival(goals))
            _snapshot(fs, s, route, vol2, origin, res)                               # the same shape: the world stays
            got[route]["sweep"] = s.sense(goals)
            got[route]["grid2"] = s.read_grid_region()
            _snapshot(fs, s, route, narrow, origin, res)                             # another shape: the world goes
            with pytest.raises(fs.capi.FsError) as e:
                s.sense(goals)
            assert str(e.value) == no_world
            np.testing.assert_array_equal(s.read_grid_region(), narrow)
        finally:
            s.close()
    a, b = got["dense"], got["bricks"]
    np.testing.assert_array_equal(a["grid"], vol)
    np.testing.assert_array_equal(b["grid"], vol)
    np.testing.assert_array_equal(a["grid2"], b["grid2"])
    assert a["limits"] == b["limits"]
    assert set(a["arrival"]) == set(b["arrival"])
    for k in a["arrival"]:
        np.testing.assert_array_equal(a["arrival"][k], b["arrival"][k], err_msg=k)
    for k in ("status", "seen_unknown"):
        np.testing.assert_array_equal(a["sweep"][k], b["sweep"][k], err_msg=k)
    assert (a["sweep"]["n_seen"], a["sweep"]["n_revealed"], a["sweep"]["window"]) == (b["sweep"]["n_seen"], b["sweep"]["n_revealed"], b["sweep"]["window"])

    w2 = fs.synth.make_small_2d(302, n=64, n_cand=12, n_landmarks=8)
    kw2 = dict(max_camera_depth=w2.max_camera_depth, delta_theta=w2.delta_theta, camera_fov=w2.camera_fov, robot_radius=w2.robot_radius,
               n_rays=w2.n_yaw, elev=w2.elev, polygon=w2.polygon)
    flat = np.array(w2.cells, dtype=np.uint8, copy=True)
    zone2 = (K.DISC, w2.origin[0] + 32 * w2.resolution, w2.origin[1] + 32 * w2.resolution, 0.0, 6 * w2.resolution)
    marked = K.mark(flat[0], [zone2], w2.origin, w2.resolution)
    assert (marked != flat[0]).any()
    s = fs.FrontierScorer(device=0)
    try:
        s.set_ray_params(**kw2)
        _add(s, zone2)
        s.upload_grid(flat, w2.origin, w2.resolution)
        s.upload_world(flat)
        np.testing.assert_array_equal(s.read_grid_region()[0], marked)
        limits, arrival = s.max_arrival(), s.score_arrival(w2.goals)
        with pytest.raises(fs.capi.FsError) as e:
            s.upload_grid_bricks(flat.shape, w2.origin, w2.resolution, np.zeros((0, 3), np.int32), np.zeros((0, 512), np.uint8))
        assert str(e.value) == f"fitslam_frontier error {FS_E_INVALID}: brick upload needs dimensions that are multiples of 8"
        np.testing.assert_array_equal(s.read_grid_region(shape=(64, 64)), marked)   # refused: the map, its limits and the world stay
        assert s.max_arrival() == limits
        again = s.score_arrival(w2.goals)
        for k in arrival:
            np.testing.assert_array_equal(again[k], arrival[k], err_msg=k)
        s.upload_grid(flat, w2.origin, w2.resolution)                            # the same shape: the world stays, the zone marks again
        np.testing.assert_array_equal(s.read_grid_region()[0], marked)
        assert s.sense(w2.goals[:4])["status"].shape == (4,)
        s.upload_grid(flat[:, :, :56], w2.origin, w2.resolution)                 # another shape: the world goes
        with pytest.raises(fs.capi.FsError) as e:
            s.sense(w2.goals[:4])
        assert str(e.value) == no_world
    finally:
        s.close()
