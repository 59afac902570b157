"""fs_sense, fs_upload_world, fs_goals_mapped and fs_grid_census on the GPU (fit-slam_amd/csrc/fs_sense.hip)
against tests/sense_ref.py, bit for bit: every output of the sweep and the whole staged map read back; scoring and the frontier
predicate after a sweep against a fresh snapshot of the merged map, through both ray walks, in 2-D and 3-D and with a keep-out
zone across the window; the error paths; the two small calls on maps with goals on every border and corner."""
import ctypes

import numpy as np
import pytest

import sense_ref as SR

pytestmark = pytest.mark.gpu

FS_E_INVALID, FS_E_STATE = -1, -4
N_POSES = 40
# what a refused sweep says, word for word
NO_GRID = "fs_upload_grid has not been called"
NO_WORLD = "fs_upload_world has not been called"
NO_SENSOR = "fs_set_ray_params has not been called and no sensor is given"


def _params(w, **over):
    p = dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov, n_rays=w.n_yaw,
             elev=tuple(w.elev), obst=(240, 254), trace=(255, 255), polygon=tuple(w.polygon))
    p.update(over)
    return p


def _case(fs, name):
    """(workload, world, staged, poses [40][3], first_ray [40]): the staged map is the world with a block set to unknown; the
    poses hold one off the map, one next to the border (its end points are clamped), one in the last row and column, one on a
    cell that is lethal in the world, two identical ones and one with the last admissible window"""
    if name == "C1":
        w = fs.synth.make_workload("C1", n_cand=N_POSES, n_landmarks=8)
    else:
        w = fs.synth.make_small_2d(401 + int(name), n=int(name), n_cand=N_POSES, n_landmarks=8)
    rng = np.random.default_rng(len(name) + 7)
    world = np.array(w.cells, dtype=np.uint8, copy=True)
    nz, ny, nx = world.shape
    staged = world.copy()
    z0 = 0 if nz == 1 else nz // 4
    staged[z0:z0 + max(1, nz // 2), ny // 5:ny // 5 + ny // 2, nx // 4:nx // 4 + nx // 2] = 255
    res, (ox, oy, oz) = w.resolution, w.origin
    centre = lambda x, y, z: ((x + 0.5) * res + ox, (y + 0.5) * res + oy, ((z + 0.5) * res + oz) if nz > 1 else oz)
    poses = np.array(w.goals[:N_POSES], dtype=np.float64, copy=True)
    zc = nz // 2
    poses[0] = (ox - 1.0, oy + 1.0, poses[0][2])                                 # off the map
    poses[1] = centre(2, ny // 2, zc)                                            # the fan's western end points are clamped
    poses[2] = centre(nx - 1, ny - 1, zc)                                        # last row and column
    lz, ly, lx = np.argwhere(world == 254)[len(np.argwhere(world == 254)) // 2]
    poses[3] = centre(lx, ly, lz)                                                # its own cell is lethal in the world
    poses[5] = poses[4]                                                          # two identical poses
    n_yaw, n_elev, k = SR.fan_shape(_params(w))
    first = rng.integers(-1, n_yaw - k + 1, size=N_POSES).astype(np.int32)
    first[5] = first[4]
    first[6] = n_yaw - k
    first[7] = -1
    first[3] = -1
    return w, world, staged, poses, first


_CASES, _REFS = {}, {}


def case(fs, name):
    if name not in _CASES:
        _CASES[name] = _case(fs, name)
    return _CASES[name]


def ref(fs, name, what, staged, world, params, poses, first):
    """sense_ref, computed once per (case, variant) and shared"""
    if (name, what) not in _REFS:
        w = case(fs, name)[0]
        _REFS[(name, what)] = SR.sense_ref(staged, world, w.origin, w.resolution, params, poses, first)
    return _REFS[(name, what)]


def _equal_sweep(got, want, grid):
    for k in ("status", "seen_unknown", "ray_unknown"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got["n_seen"], got["n_revealed"], got["window"]) == (want["n_seen"], want["n_revealed"], tuple(int(v) for v in want["window"]))
    np.testing.assert_array_equal(grid, want["grid"])


@pytest.mark.parametrize("name", ["61", "96", "C1"])
def test_sweep_equals_the_restatement(fs, name):
    w, world, staged, poses, first = case(fs, name)
    p = _params(w)
    s = fs.FrontierScorer(device=0)
    try:
        s.set_ray_params(**p)
        s.upload_grid(staged, w.origin, w.resolution)
        s.upload_world(world)
        before = s.grid_census()
        assert before == SR.census_ref(staged)
        got = s.sense(poses, first, rays=True)
        want = ref(fs, name, "window", staged, world, p, poses, first)
        assert want["status"][0] == SR.OFF_MAP and (want["status"][1:] == SR.OK).all()
        assert want["n_revealed"] > 0 and want["seen_unknown"][3] == 0 and (want["seen_unknown"] > 0).any()
        _equal_sweep(got, want, s.read_grid_region())
        after = s.grid_census()
        assert after == SR.census_ref(want["grid"]) and after["known"] == before["known"] + want["n_revealed"]
        # the same call again: every seen cell is known now (the world of these maps holds 255, which stays 255)
        again = s.sense(poses, first, rays=True)
        want2 = ref(fs, name, "window_again", want["grid"], world, p, poses, first)
        _equal_sweep(again, want2, s.read_grid_region())
        assert again["n_revealed"] == 0 and again["n_seen"] == got["n_seen"]
        # NULL first_ray: every pose sweeps the whole fan (the same shape: the world stays)
        s.upload_grid(staged, w.origin, w.resolution)
        got = s.sense(poses, None, rays=True)
        _equal_sweep(got, ref(fs, name, "lidar", staged, world, p, poses, None), s.read_grid_region())
        # a sensor of its own: twice the depth (in 3-D also four elevation rings), ranges of its own
        far = _params(w, max_camera_depth=2 * w.max_camera_depth, obst=(253, 254), trace=(200, 255))
        if name == "C1":
            far["elev"] = (-0.30, -0.10, 0.10, 0.30)
        s.upload_grid(staged, w.origin, w.resolution)
        got = s.sense(poses, first, sensor=far, rays=True)
        assert got["ray_unknown"].shape == (N_POSES,) + SR.fan_shape(far)[1::-1]
        _equal_sweep(got, ref(fs, name, "far", staged, world, far, poses, first), s.read_grid_region())
        got = s.sense(poses, first, sensor=far, rays=True)                       # (the cached table)
        _equal_sweep(got, ref(fs, name, "far_again", _REFS[(name, "far")]["grid"], world, far, poses, first), s.read_grid_region())
        # the context's own fan is still what NULL means
        s.upload_grid(staged, w.origin, w.resolution)
        _equal_sweep(s.sense(poses, first, rays=True), want, s.read_grid_region())
        if name == "61":
            # a polygon that clamps every end point beyond the map: every pose is off the map, nothing changes, a no-op
            s.upload_grid(staged, w.origin, w.resolution)
            gone = _params(w, polygon=(w.origin[0] + 100.0, -1e300, 1e300, 1e300))
            got = s.sense(poses, first, sensor=gone, rays=True)
            _equal_sweep(got, ref(fs, name, "gone", staged, world, gone, poses, first), s.read_grid_region())
            assert (got["status"] == SR.OFF_MAP).all() and got["n_seen"] == 0 and got["window"] == (0, 0, 0, 0, 0, 0)
            assert s.sense(np.zeros((0, 3)))["n_seen"] == 0
    finally:
        s.close()


def test_second_sweep_of_a_fully_known_world_reveals_nothing(fs):
    w, world, staged, poses, first = case(fs, "96")
    solid = world.copy()
    solid[solid == 255] = 0                                                      # a world free of 255
    p = _params(w)
    s = fs.FrontierScorer(device=0)
    try:
        s.set_ray_params(**p)
        s.upload_grid(np.full_like(solid, 255), w.origin, w.resolution)
        s.upload_world(solid)
        one = s.sense(poses, first, rays=True)
        assert one["n_revealed"] == one["n_seen"] > 0 and one["seen_unknown"].sum() > 0
        two = s.sense(poses, first, rays=True)
        assert two["n_revealed"] == 0 and two["n_seen"] == one["n_seen"] and two["window"] == one["window"]
        assert not two["seen_unknown"].any() and not two["ray_unknown"].any()
        np.testing.assert_array_equal(two["status"], one["status"])
        assert s.grid_census()["known"] == one["n_seen"]
    finally:
        s.close()


def _equal_arrival(a, b):
    for k in ("status", "arrival", "argmax", "achievable", "yaw", "ray_counts"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("name,keepout", [("96", False), ("96", True), ("C1", False)], ids=["2d", "2d_keepout", "3d"])
def test_scoring_after_a_sweep_equals_a_fresh_snapshot(fs, name, keepout, layout):
    w, world, staged, poses, first = case(fs, name)
    p = _params(w)
    a, b = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (a, b):
            s.set_option("ray.layout", layout)
            s.set_ray_params(**p)
            if keepout:                                                          # a stored zone across the sweep's window
                s.keepout_add_fov(float(poses[8][0]), float(poses[8][1]), 0.4, 2.0)
        a.upload_grid(staged, w.origin, w.resolution)
        mx = a.max_arrival()
        a.score_arrival(w.goals, w.frontier_size)                                # (the class image exists before the sweep)
        a.upload_world(world)
        got = a.sense(poses, first)
        want = ref(fs, name, "window", staged, world, p, poses, first)
        assert (got["n_seen"], got["window"]) == (want["n_seen"], tuple(int(v) for v in want["window"]))
        b.upload_grid(want["grid"], w.origin, w.resolution)
        b.set_arrival_limits(mx["max_gt"], mx["min_gt"])
        merged = a.read_grid_region()
        np.testing.assert_array_equal(merged, b.read_grid_region())
        if keepout:
            mask = a.keepout_get()[2].astype(bool)
            x0, y0, _, sx, sy, _ = got["window"]
            assert mask[y0:y0 + sy, x0:x0 + sx].any() and (merged[0][mask] == 253).all()
            np.testing.assert_array_equal(merged[0][~mask], want["grid"][0][~mask])
        else:
            np.testing.assert_array_equal(merged, want["grid"])
        _equal_arrival(a.score_arrival(w.goals, w.frontier_size), b.score_arrival(w.goals, w.frontier_size))
        ma, ca = a.frontier_cells(merged.shape, 160)
        mb, cb = b.frontier_cells(merged.shape, 160)
        assert ca == cb
        np.testing.assert_array_equal(ma, mb)
    finally:
        a.close(); b.close()


def test_error_paths(fs):
    w, world, staged, poses, first = case(fs, "61")
    p = _params(w)
    s = fs.FrontierScorer(device=0)
    try:
        def refused(code, f, *args, text=None, **kw):
            with pytest.raises(fs.capi.FsError) as e:
                f(*args, **kw)
            assert e.value.code == code
            assert text is None or str(e.value) == f"fitslam_frontier error {code}: {text}"
        refused(FS_E_STATE, s.upload_world, world, text=NO_GRID)                # no grid staged
        s.set_ray_params(**p)
        s.upload_grid(staged, w.origin, w.resolution)
        refused(FS_E_STATE, s.sense, poses, first, text=NO_WORLD)               # no world
        refused(FS_E_INVALID, s.upload_world, world[:, :60, :])                 # another shape: nothing changed
        refused(FS_E_STATE, s.sense, poses, first, text=NO_WORLD)
        s.upload_world(world)
        refused(FS_E_INVALID, s.upload_world, world[:, :, :60])                 # ... and the world staged before stays
        # first_ray out of range: nothing is written, the map stays
        n_yaw, n_elev, k = SR.fan_shape(p)
        ptr = lambda v: v.ctypes.data_as(ctypes.c_void_p)
        for bad in (n_yaw - k + 1, -2):
            fr = first.copy(); fr[17] = bad
            seen = np.full(N_POSES, 77, np.int32); status = np.full(N_POSES, 77, np.int32); win = np.full(6, 77, np.int32)
            rays = np.full((N_POSES, n_elev, n_yaw), 77, np.int32)
            n_seen, n_rev = ctypes.c_int64(77), ctypes.c_int64(77)
            rc = s._L.fs_sense(s._h, N_POSES, ptr(poses), ptr(fr), None, ptr(rays), ptr(seen), ptr(status), ctypes.byref(n_seen),
                               ctypes.byref(n_rev), ptr(win))
            assert rc == FS_E_INVALID
            assert s._L.fs_last_error(s._h).decode() == f"first_ray[17] = {bad} is outside [-1, {n_yaw - k}]"
            assert (seen == 77).all() and (status == 77).all() and (win == 77).all() and (rays == 77).all()
            assert n_seen.value == 77 and n_rev.value == 77
        np.testing.assert_array_equal(s.read_grid_region(), staged)
        refused(FS_E_INVALID, s.sense, poses, first, sensor=_params(w, elev=()))                    # validated as set_ray_params validates
        refused(FS_E_INVALID, s.sense, poses, first, sensor=_params(w, camera_fov=100.0))
        # a window update never touches the world; a snapshot of the same shape keeps it
        s.update_grid_region(3, 4, 0, np.full((5, 7), 255, np.uint8))
        s.upload_grid(staged, w.origin, w.resolution)
        got = s.sense(poses, first, rays=True)
        _equal_sweep(got, ref(fs, "61", "window", staged, world, p, poses, first), s.read_grid_region())
        # NULL releases it; a snapshot of another shape drops it
        s.upload_world(None)
        refused(FS_E_STATE, s.sense, poses, first, text=NO_WORLD)
        s.upload_world(world)
        s.upload_grid(staged[:, :60, :], w.origin, w.resolution)
        refused(FS_E_STATE, s.sense, poses, first, text=NO_WORLD)
        # a context without ray parameters needs a sensor
        t = fs.FrontierScorer(device=0)
        try:
            t.upload_grid(staged, w.origin, w.resolution)
            t.upload_world(world)
            refused(FS_E_STATE, t.sense, poses, first, text=NO_SENSOR)
            got = t.sense(poses, first, sensor=p, rays=True)
            _equal_sweep(got, _REFS[("61", "window")], t.read_grid_region())
        finally:
            t.close()
    finally:
        s.close()


def test_goals_mapped_and_census_equal_their_restatements(fs):
    s = fs.FrontierScorer(device=0)
    try:
        for seed, n in ((31, 61), (32, 96), (33, 24)):
            w = fs.synth.make_small_2d(seed, n=n, n_cand=4, n_landmarks=4)
            rng = np.random.default_rng(seed)
            cells = w.cells[0].copy()
            cells[rng.random(cells.shape) < 0.05] = 254
            if n == 24:
                cells = np.ascontiguousarray(cells[:7, :9])                      # a map smaller than the 5 x 5 block's reach
            ny, nx = cells.shape
            goals = SR.border_goals(nx, ny, w.origin, w.resolution, rng)
            s.upload_grid(cells, w.origin, w.resolution)
            want = SR.goals_mapped_ref(cells, w.origin, w.resolution, goals)
            np.testing.assert_array_equal(s.goals_mapped(goals), want)
            assert 0 < want.sum() < want.size
            assert s.grid_census() == SR.census_ref(cells)
            assert s.goals_mapped(np.zeros((0, 3))).shape == (0,)
        c1 = fs.synth.make_workload("C1", n_cand=4, n_landmarks=4)
        s.upload_grid(c1.cells, c1.origin, c1.resolution)
        assert s.grid_census() == SR.census_ref(c1.cells)                        # 3-D, 2^18 cells
        odd = np.ascontiguousarray(c1.cells[:3, :5, :7])                         # 105 cells: no whole 16-byte word but six
        s.upload_grid(odd, c1.origin, c1.resolution)
        assert s.grid_census() == SR.census_ref(odd)
        with pytest.raises(fs.capi.FsError) as e:
            s.goals_mapped(c1.goals)                                             # 2-D grids only
        assert e.value.code == FS_E_INVALID
    finally:
        s.close()
