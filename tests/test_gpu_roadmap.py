"""The frontier roadmap on the GPU: fs_roadmap_rebuild's CSR and fs_roadmap_connect's insertions against the CPU
restatement (tests/roadmap_ref/roadmap_ref.cpp) bit for bit, fs_roadmap_plan against the restatement's `tree` leg bit for bit and
against its per-goal A* on achievability, the per-context tree cache, and fs_get_frontier_costs_roadmap against fs_roadmap_plan +
fs_get_frontier_costs."""
import importlib
import zlib

import numpy as np
import pytest

import planner_ref as P
import roadmap_ref as R

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05


def _maps():
    """(name, cells [ny][nx], origin): REF2D's map, floor plans up to 1024^2, a non-square map, the spiral corridor."""
    out = [("REF2D", fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])]
    rng = np.random.Generator(np.random.PCG64(5151))
    for k, n in enumerate([64, 96, 128, 160, 200, 256, 300, 384, 512, 640, 768, 1024]):
        out.append((f"plan{k}_{n}", fsmod.synth.make_grid(rng, n, 1)[0]))
    out.append(("non_square", fsmod.synth.make_grid(rng, 256, 1)[0][:170, :]))
    out.append(("spiral", P.spiral_map(512)[0]))
    return [(name, np.ascontiguousarray(c), (-c.shape[1] * RES / 2, -c.shape[0] * RES / 2, 0.0)) for name, c in out]


MAPS = _maps()


def _nodes(cells, origin, seed, k):
    """k node positions: free and unknown cells, jittered inside the cell"""
    rng = np.random.default_rng(seed)
    xs, ys = P.free_cells(cells, rng, k)
    if (cells == 255).any():
        ux, uy = P.free_cells(cells, rng, k // 5, value=255)
        xs[: k // 5], ys[: k // 5] = ux, uy
    return np.stack([origin[0] + (xs + rng.uniform(0, 1, k)) * RES, origin[1] + (ys + rng.uniform(0, 1, k)) * RES], axis=1)


def _pair(cells, origin):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    return sc, R.Roadmap(cells, origin, RES)


def _same_graph(got, want, what):
    for k in ("xy", "key", "row_ptr", "col"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("name,cells,origin", MAPS, ids=[m[0] for m in MAPS])
def test_rebuild_equals_restatement(name, cells, origin):
    sc, ref = _pair(cells, origin)
    try:
        area = cells.size * RES * RES
        pts = _nodes(cells, origin, zlib.crc32(name.encode()), int(min(1500, max(40, area / 2))))
        rc = ref.populate(pts)
        try:
            sc.roadmap_add_nodes(pts)
        except fsmod.FsError as e:
            assert e.code == R.FS_E_RANGE and rc == R.FS_E_RANGE
        ref.rebuild()
        sc.roadmap_rebuild()
        got, want = sc.roadmap_graph(), ref.graph()
        _same_graph(got, want, name)
        assert want["col"].size > 0
        # a second rebuild from the same nodes is the same CSR
        sc.roadmap_rebuild()
        _same_graph(sc.roadmap_graph(), want, name + " again")
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("name", ["REF2D", "plan5_256", "plan8_512", "plan11_1024"])
def test_connect_over_ticks_equals_restatement(name):
    cells, origin = next((c, o) for n, c, o in MAPS if n == name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    xs, ys = P.free_cells(cells, rng, 5)
    ticks = R.grow_ticks(fsmod, cells, origin, RES, list(zip(xs.tolist(), ys.tolist())))
    sc, ref = _pair(cells, origin)
    try:
        for t, (frontiers, robot) in enumerate(ticks):
            # UpdateRoadmapBT: addNodes(frontiers), addRobotPoseAsNode, constructNewEdges(frontiers), constructNewEdgeRobotPose
            for pts, robot_flag in ((frontiers, False), (robot[None], True)):
                if pts.shape[0]:
                    assert ref.populate(pts, robot_flag) == 0
                    sc.roadmap_add_nodes(pts, is_robot_pose=robot_flag)
            both = np.concatenate([frontiers, robot[None]])
            ref.connect(both)
            sc.roadmap_connect(both)
            _same_graph(sc.roadmap_graph(), ref.graph(), (name, t))
        # the rebuild of the grown roadmap as well, and a connect after it
        ref.rebuild(); sc.roadmap_rebuild()
        _same_graph(sc.roadmap_graph(), ref.graph(), (name, "rebuild"))
        ref.connect(ticks[0][0]); sc.roadmap_connect(ticks[0][0])
        _same_graph(sc.roadmap_graph(), ref.graph(), (name, "connect after rebuild"))
        assert ref.graph()["col"].size > 0
    finally:
        sc.close(); ref.close()


def _goals(cells, origin, seed, n, robot_xy):
    rng = np.random.default_rng(seed)
    ny, nx = cells.shape
    xs, ys = P.free_cells(cells, rng, n)
    g = np.zeros((n, 3))
    g[:, 0] = origin[0] + (xs + rng.uniform(0, 1, n)) * RES
    g[:, 1] = origin[1] + (ys + rng.uniform(0, 1, n)) * RES
    if n >= 10:
        g[1, 0] = origin[0] - 1.0                        # off the map, left
        g[5, 1] = origin[1] + (ny + 3) * RES             # off the map, above
        g[7, :2] = robot_xy                              # exactly at the robot
    ach = (rng.random(n) > 0.1).astype(np.uint8)
    return g, ach


@pytest.mark.parametrize("name,cells,origin", [m for m in MAPS if m[0] in ("REF2D", "plan5_256", "plan8_512", "plan11_1024", "non_square", "spiral")],
                         ids=["REF2D", "plan5_256", "plan8_512", "plan11_1024", "non_square", "spiral"])
def test_plan_equals_tree_leg_and_astar_achievability(name, cells, origin):
    sc, ref = _pair(cells, origin)
    try:
        seed = zlib.crc32(name.encode())
        pts = _nodes(cells, origin, seed, int(min(1500, max(40, cells.size * RES * RES / 2))))
        assert ref.populate(pts) == 0
        sc.roadmap_add_nodes(pts)
        ref.rebuild(); sc.roadmap_rebuild()
        rng = np.random.default_rng(seed + 7)
        for trial in range(2):
            rx, ry = pts[rng.integers(pts.shape[0])] + rng.uniform(-0.3, 0.3, 2)
            pose = R.pose7(rx, ry, 0.7 * trial + 0.2)
            for n in (1, 50, 2000):
                goals, ach = _goals(cells, origin, seed + n + trial, n, (rx, ry))
                got = sc.roadmap_plan(pose, goals, achievable_in=ach)
                want = ref.plan(pose, goals, achievable_in=ach)
                for k in ("path_length", "path_length_m", "path_heading", "achievable"):
                    assert got[k].tobytes() == want[k].tobytes(), (name, n, k)
                astar = ref.plan(pose, goals, achievable_in=ach, leg=R.REFERENCE_ASTAR)
                assert np.array_equal(astar["achievable"], got["achievable"]), (name, n)
                if n >= 10:
                    assert got["achievable"][7] == (1 if ach[7] else 0) and (not ach[7] or got["path_length_m"][7] == 0.0)
                    assert got["achievable"][~ach.astype(bool)].sum() == 0
            assert got["achievable"].sum() > 0
    finally:
        sc.close(); ref.close()


def test_plan_on_a_large_roadmap_takes_the_round_per_launch_tree():
    """Above RM_TREE_ONE_WG (16 384) nodes the tree is relaxed one round per launch, polled in batches; small cells and a short
    edge radius keep the restatement's rebuild short."""
    name, cells, origin = next(m for m in MAPS if m[0] == "plan11_1024")
    ny, nx = cells.shape
    rng = np.random.default_rng(16385)
    gx, gy = np.meshgrid(np.arange(0.1, nx * RES, 0.27), np.arange(0.1, ny * RES, 0.27))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-0.01, 0.01, (gx.size, 2))
    ix, iy = (pts[:, 0] / RES).astype(int), (pts[:, 1] / RES).astype(int)
    pts = pts[cells[iy, ix] == 0] + np.array(origin[:2])
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    sc.set_roadmap_params(grid_cell_size=0.5, radius_to_decide_edges=0.6)
    ref = R.Roadmap(cells, origin, RES, grid_cell_size=0.5, radius=0.6)
    try:
        assert ref.populate(pts) == 0
        sc.roadmap_add_nodes(pts)
        ref.rebuild(); sc.roadmap_rebuild()
        assert sc.roadmap_graph()["xy"].shape[0] > 16384
        rx, ry = pts[rng.integers(pts.shape[0])]
        pose = R.pose7(rx, ry, 0.4)
        goals, ach = _goals(cells, origin, 16386, 2000, (rx, ry))
        sc.get_counter(1006, reset=True)
        got = sc.roadmap_plan(pose, goals, achievable_in=ach)
        want = ref.plan(pose, goals, achievable_in=ach)
        for k in ("path_length", "path_length_m", "path_heading", "achievable"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert sc.get_counter(1006) > 0
        assert got["achievable"].sum() > 0
    finally:
        sc.close(); ref.close()


def test_plan_on_an_empty_and_a_keyless_roadmap():
    cells = np.zeros((80, 80), dtype=np.uint8)
    origin = (0.0, 0.0, 0.0)
    sc, ref = _pair(cells, origin)
    try:
        pose = R.pose7(1.0, 1.0)
        goals = np.array([[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [30.0, 1.0, 0.0]])
        for stage in ("empty", "keyless"):
            got, want = sc.roadmap_plan(pose, goals), ref.plan(pose, goals)
            for k in got:
                assert got[k].tobytes() == want[k].tobytes(), (stage, k)
            assert got["achievable"].tolist() == [1, 0, 0] and got["path_length_m"][0] == 0.0
            ref.populate([[1.5, 1.5], [2.5, 2.5]]); sc.roadmap_add_nodes([[1.5, 1.5], [2.5, 2.5]])   # nodes, but no key yet
        sc.roadmap_connect([[1.5, 1.5]]); ref.connect([[1.5, 1.5]])
        got, want = sc.roadmap_plan(pose, goals), ref.plan(pose, goals)
        for k in got:
            assert got[k].tobytes() == want[k].tobytes(), k
        assert got["achievable"].tolist() == [1, 1, 1]
    finally:
        sc.close(); ref.close()


def test_tree_cache_is_dropped_by_every_mutation():
    name, cells, origin = MAPS[0]
    sc, ref = _pair(cells, origin)
    try:
        pts = _nodes(cells, origin, 3, 300)
        sc.roadmap_add_nodes(pts); ref.populate(pts)
        sc.roadmap_rebuild(); ref.rebuild()
        goals, _ = _goals(cells, origin, 4, 50, (0.0, 0.0))
        pose = R.pose7(*pts[0])
        sc.get_counter(1005, reset=True)
        first = sc.roadmap_plan(pose, goals)
        sc.roadmap_plan(pose, goals)
        assert sc.get_counter(1005) == 1                             # the same roadmap and start node: reused
        assert sc.get_counter(1006) > 0
        sc.roadmap_plan(R.pose7(*pts[1]), goals)                     # another start node: a new tree
        assert sc.get_counter(1005) == 2
        builds = 2
        for what, mutate in (("add_nodes", lambda: (sc.roadmap_add_nodes([[0.123, 0.456]]), ref.populate([[0.123, 0.456]]))),
                             ("connect", lambda: (sc.roadmap_connect(pts[:5]), ref.connect(pts[:5]))),
                             ("rebuild", lambda: (sc.roadmap_rebuild(), ref.rebuild()))):
            mutate()
            got = sc.roadmap_plan(pose, goals)
            builds += 1
            assert sc.get_counter(1005) == builds, what
            want = ref.plan(pose, goals)
            for k in got:
                assert got[k].tobytes() == want[k].tobytes(), (what, k)
        assert first["achievable"].sum() > 0
        # new parameters start an empty roadmap
        sc.set_roadmap_params(radius_to_decide_edges=4.0)
        assert sc.roadmap_graph()["xy"].shape[0] == 0
        assert sc.roadmap_plan(pose, goals)["achievable"].sum() == 0
    finally:
        sc.close(); ref.close()


def test_roadmap_refuses_3d_grids_and_bad_input():
    sc = fsmod.FrontierScorer(device=0)
    try:
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_rebuild()                                      # no grid staged
        assert e.value.code == fsmod.capi.FS_E_STATE
        sc.upload_grid(np.zeros((4, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        sc.roadmap_add_nodes([[0.2, 0.2]])
        for call in (sc.roadmap_rebuild, lambda: sc.roadmap_connect([[0.2, 0.2]])):
            with pytest.raises(fsmod.FsError) as e:
                call()
            assert e.value.code == fsmod.capi.FS_E_INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_add_nodes([[np.nan, 0.0]])
        assert e.value.code == fsmod.capi.FS_E_INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.set_roadmap_params(grid_cell_size=0.0)
        assert e.value.code == fsmod.capi.FS_E_INVALID
    finally:
        sc.close()


@pytest.mark.parametrize("with_fim", [False, True])
@pytest.mark.parametrize("which", ["small", "REF2D"])
def test_fused_equals_plan_then_costs(with_fim, which):
    w = fsmod.synth.make_small_2d(31, n=128, n_cand=80) if which == "small" else fsmod.synth.make_workload("REF2D", n_cand=300, n_landmarks=20_000)
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                          robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
        sc.upload_grid(w.cells, w.origin, w.resolution)
        if with_fim:
            sc.set_option("fim.learn", 0)
            sc.upload_landmarks(w.landmarks)
            sc.lookup_generate()
            sc.set_fim_params(14.0, 1.0)
        mx = sc.max_arrival()
        sc.set_arrival_limits(4000.0, mx["min_gt"])
        sc.roadmap_add_nodes(w.goals[:, :2])
        sc.roadmap_rebuild()
        pose = R.pose7(*w.goals[0, :2], 1.0)
        plan = sc.roadmap_plan(pose, w.goals)
        want = sc.get_frontier_costs(w.goals, plan["path_length"], plan["path_heading"], frontier_size=w.frontier_size,
                                     blacklisted=w.blacklisted, achievable_in=plan["achievable"], with_fim=with_fim)
        got = sc.get_frontier_costs_roadmap(pose, w.goals, frontier_size=w.frontier_size, blacklisted=w.blacklisted, with_fim=with_fim)
        for k in ("weighted_cost", "arrival_utility", "distance_utility", "order"):
            assert got[k].tobytes() == want[k].tobytes(), k
        # (with Fisher information the float sums of a record are reproducible only to the last bits: tests/test_gpu_planner.py)
        floats = ("info_ref", "trace", "logdet") if with_fim else ()
        for k in got["records"].dtype.names:
            if k in floats:
                np.testing.assert_allclose(got["records"][k], want["records"][k], rtol=5e-6, atol=1e-6, err_msg=k)
            else:
                assert got["records"][k].tobytes() == want["records"][k].tobytes(), k
        assert got["path_length_m"].tobytes() == plan["path_length_m"].tobytes()
        assert plan["achievable"].sum() > 1
    finally:
        sc.close()
