"""The batched grid planner on the GPU: fs_navfn_potential and fs_plan_paths against the CPU restatement's
`converged` leg (tests/navfn_ref/navfn_ref.cpp) bit for bit, the per-context field cache, and fs_get_frontier_costs_planned
against fs_plan_paths + fs_get_frontier_costs."""
import importlib
import zlib

import numpy as np
import pytest

import planner_ref as R

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05


def _maps():
    """(name, cells [ny][nx], origin): REF2D's map, random floor plans up to 1024^2, a spiral corridor."""
    out = [("REF2D", fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0], None)]
    rng = np.random.Generator(np.random.PCG64(4242))
    for k, n in enumerate([64, 96, 100, 128, 160, 200, 256, 256, 300, 384, 512, 512, 640, 768, 1024, 1024, 72, 130, 257, 333]):
        out.append((f"plan{k}_{n}", fsmod.synth.make_grid(rng, n, 1)[0], None))
    out.append(("non_square", fsmod.synth.make_grid(rng, 192, 1)[0][:150, :], None))
    out.append(("spiral", R.spiral_map(512)[0], None))
    res = []
    for name, cells, _ in out:
        ny, nx = cells.shape
        res.append((name, np.ascontiguousarray(cells), (-nx * RES / 2, -ny * RES / 2, 0.0)))
    return res


MAPS = _maps()


def _scorer(cells, origin):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    return sc


def _robots(cells, seed, k=2):
    rng = np.random.default_rng(seed)
    xs, ys = R.free_cells(cells, rng, k)
    return list(zip(xs.tolist(), ys.tolist()))


def _goals(cells, origin, seed, n):
    """n goals: free and unknown cells (jittered inside the cell), a few off the map; achievable_in with some zeros"""
    rng = np.random.default_rng(seed)
    ny, nx = cells.shape
    xs, ys = R.free_cells(cells, rng, n)
    if (cells == 255).any() and n > 4:
        ux, uy = R.free_cells(cells, rng, n // 5, value=255)
        xs[: n // 5], ys[: n // 5] = ux, uy
    g = np.zeros((n, 3))
    g[:, 0] = origin[0] + (xs + rng.uniform(0.0, 1.0, n)) * RES
    g[:, 1] = origin[1] + (ys + rng.uniform(0.0, 1.0, n)) * RES
    if n >= 10:
        g[1, 0] = origin[0] - 1.0                        # off the map, left
        g[5, 1] = origin[1] + (ny + 3) * RES             # off the map, above
    ach = (rng.random(n) > 0.1).astype(np.uint8)
    return g, ach


@pytest.mark.parametrize("name,cells,origin", MAPS, ids=[m[0] for m in MAPS])
def test_potential_equals_converged_leg(name, cells, origin):
    sc = _scorer(cells, origin)
    try:
        for i, (rx, ry) in enumerate(_robots(cells, zlib.crc32(name.encode()))):
            for allow in (0, 1):
                pose = R.robot_pose(origin, RES, rx, ry, 0.4)
                got = sc.navfn_potential(pose, allow_unknown=allow)
                want, _ = R.converged_field(cells, rx, ry, allow_unknown=allow)
                assert got.tobytes() == want.tobytes(), (name, rx, ry, allow, int((got != want).sum()))
    finally:
        sc.close()


# REF2D, floor plans from 64^2 to 256^2, one of 512^2 and one of 1024^2 (where max_cycles and the path scratch's stride are largest),
# the non-square map and the spiral
COLUMN_MAPS = MAPS[:8] + [MAPS[11], MAPS[15]] + MAPS[-2:]
assert COLUMN_MAPS[0][0] == "REF2D" and COLUMN_MAPS[8][1].shape == (512, 512) and COLUMN_MAPS[9][1].shape == (1024, 1024)


@pytest.mark.parametrize("name,cells,origin", COLUMN_MAPS, ids=[m[0] for m in COLUMN_MAPS])
@pytest.mark.parametrize("n", [1, 50, 2000])
def test_plan_paths_equal_converged_leg(name, cells, origin, n):
    sc = _scorer(cells, origin)
    try:
        rx, ry = R.well_placed_robot(cells, np.random.default_rng(7 + n))
        pose = R.robot_pose(origin, RES, rx, ry, -2.0)
        goals, ach_in = _goals(cells, origin, 11 + n, n)
        for allow in (0, 1):
            got = sc.plan_paths(pose, goals, achievable_in=ach_in, allow_unknown=allow)
            want = R.plan(cells, origin, RES, pose, goals, achievable_in=ach_in, allow_unknown=allow)
            for k in ("path_length", "path_length_m", "path_heading", "achievable"):
                assert got[k].tobytes() == want[k].tobytes(), (name, n, allow, k, np.nonzero(got[k] != want[k])[0][:8])
            if n >= 50:
                assert got["achievable"].sum() > 0
    finally:
        sc.close()


def test_robot_or_goal_off_the_map():
    name, cells, origin = MAPS[1]
    sc = _scorer(cells, origin)
    try:
        goals, _ = _goals(cells, origin, 3, 20)
        off = np.array([origin[0] - 0.5, origin[1] + 1.0, 0, 0, 0, 0, 1.0])
        got = sc.plan_paths(off, goals)
        assert not got["achievable"].any() and (got["path_length"] == R.DBL_MAX).all() and (got["path_length_m"] == R.DBL_MAX).all()
        assert (got["path_heading"] == R.DBL_MAX).all()
        with pytest.raises(fsmod.FsError):
            sc.navfn_potential(off)
    finally:
        sc.close()


def test_three_d_grid_is_refused():
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(np.zeros((2, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError) as e:
            sc.plan_paths(R.robot_pose((0, 0, 0), RES, 3, 3), np.zeros((1, 3)) + 0.3)
        assert e.value.code == fsmod.capi.FS_E_INVALID
    finally:
        sc.close()


def test_field_cache():
    name, cells, origin = MAPS[7]
    cells = cells.copy()
    sc = _scorer(cells, origin)
    try:
        (rx, ry), = _robots(cells, 5, 1)
        pose = R.robot_pose(origin, RES, rx, ry)
        goals, _ = _goals(cells, origin, 6, 50)
        sc.get_counter(1002, reset=True)
        first = sc.plan_paths(pose, goals)
        assert sc.get_counter(1002) == 1
        second = sc.plan_paths(pose, goals)                 # same grid, robot cell and allow_unknown: the field is reused
        assert sc.get_counter(1002) == 1
        for k in first:
            assert first[k].tobytes() == second[k].tobytes()
        sc.navfn_potential(pose)
        assert sc.get_counter(1002) == 1
        sc.plan_paths(pose, goals, allow_unknown=True)       # another allow_unknown: a new field
        assert sc.get_counter(1002) == 2
        (qx, qy), = _robots(cells, 99, 1)
        if (qx, qy) == (rx, ry):
            qx, qy = _robots(cells, 100, 1)[0]
        sc.plan_paths(R.robot_pose(origin, RES, qx, qy), goals)   # another robot cell: a new field
        assert sc.get_counter(1002) == 3
        # the same cell from another point inside it: reused
        wx, wy = R.cell_centre(origin, RES, qx, qy)
        sc.plan_paths(np.array([wx + 0.01, wy - 0.01, 0, 0, 0, 0, 1.0]), goals)
        assert sc.get_counter(1002) == 3
        # a window of the map rewritten (a wall opened / closed): the field is dropped, the result is a fresh context's
        sc.plan_paths(pose, goals)
        builds = sc.get_counter(1002)
        y0, x0 = max(ry - 20, 1), max(rx - 20, 1)
        win = cells[y0:y0 + 40, x0:x0 + 40].copy()
        win[win >= 253] = 0
        win[18:22, :] = 254
        sc.update_grid_region(x0, y0, 0, win)
        cells[y0:y0 + 40, x0:x0 + 40] = win
        cells[ry, rx] = 0
        sc.update_grid_region(rx, ry, 0, np.zeros((1, 1), dtype=np.uint8))
        after = sc.plan_paths(pose, goals)
        assert sc.get_counter(1002) == builds + 1
        fresh = _scorer(cells, origin)
        try:
            want = fresh.plan_paths(pose, goals)
        finally:
            fresh.close()
        for k in want:
            assert after[k].tobytes() == want[k].tobytes(), k
        ref = R.plan(cells, origin, RES, pose, goals)
        for k in ("path_length", "path_length_m", "path_heading", "achievable"):
            assert after[k].tobytes() == ref[k].tobytes(), k
    finally:
        sc.close()


def _setup_scoring(sc, w, with_fim):
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    if with_fim:
        sc.set_option("fim.learn", 0)          # (the learnt pass prediction makes Fisher sums depend on the calls served before)
        sc.upload_landmarks(w.landmarks)
        sc.lookup_generate()
        sc.set_fim_params(14.0, 1.0)
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])


@pytest.mark.parametrize("with_fim", [False, True])
@pytest.mark.parametrize("which", ["small", "REF2D"])
def test_fused_equals_plan_then_costs(with_fim, which):
    w = fsmod.synth.make_small_2d(31, n=128, n_cand=80) if which == "small" else fsmod.synth.make_workload("REF2D", n_cand=300, n_landmarks=20_000)
    sc = fsmod.FrontierScorer(device=0)
    try:
        _setup_scoring(sc, w, with_fim)
        cells = w.cells[0]
        rx, ry = R.well_placed_robot(cells, np.random.default_rng(17))
        pose = R.robot_pose(w.origin, w.resolution, rx, ry, 1.0)
        for allow in (0, 1):
            plan = sc.plan_paths(pose, w.goals, allow_unknown=allow)
            want = sc.get_frontier_costs(w.goals, plan["path_length"], plan["path_heading"], frontier_size=w.frontier_size,
                                         blacklisted=w.blacklisted, achievable_in=plan["achievable"], with_fim=with_fim)
            got = sc.get_frontier_costs_planned(pose, w.goals, frontier_size=w.frontier_size, blacklisted=w.blacklisted,
                                                allow_unknown=allow, with_fim=with_fim)
            for k in ("weighted_cost", "arrival_utility", "distance_utility", "order"):
                assert got[k].tobytes() == want[k].tobytes(), (k, allow)
            # every record column bit for bit — except, with Fisher information, its float sums: which lane adds which term is
            # decided by the order of LDS atomics, so info_ref / trace / logdet are reproducible call to call only to the last
            # bits (tests/test_gpu_lifecycle.py); U1 reads the integers only
            floats = ("info_ref", "trace", "logdet") if with_fim else ()
            for k in got["records"].dtype.names:
                if k in floats:
                    np.testing.assert_allclose(got["records"][k], want["records"][k], rtol=5e-6, atol=1e-6, err_msg=k)
                else:
                    assert got["records"][k].tobytes() == want["records"][k].tobytes(), (k, allow)
            assert got["path_length_m"].tobytes() == plan["path_length_m"].tobytes()
            assert plan["achievable"].sum() > 0
    finally:
        sc.close()


def test_python_binding_sizes_its_buffers_from_the_staged_grid():
    sc = fsmod.FrontierScorer(device=0)
    try:
        pose = R.robot_pose((0.0, 0.0, 0.0), RES, 5, 5)
        with pytest.raises(fsmod.FsError):
            sc.navfn_potential(pose)                                  # nothing staged yet
        sc.upload_grid(np.zeros((40, 24), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        assert sc.navfn_potential(pose).shape == (40, 24)
        sc.upload_grid(np.zeros((16, 56), dtype=np.uint8), (0.0, 0.0, 0.0), RES)   # another shape: the buffer follows it
        assert sc.navfn_potential(pose).shape == (16, 56)
        with pytest.raises(ValueError):
            sc.plan_paths(pose, np.full((3, 3), 0.3), achievable_in=[1, 1])
    finally:
        sc.close()
