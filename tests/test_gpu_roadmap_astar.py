"""The REFERENCE roadmap search on the GPU (fs_set_roadmap_search): fs_roadmap_plan, fs_get_frontier_costs_roadmap
and the pair lengths of fs_roadmap_next_goal answered by the reference's per-goal A*, against the CPU restatement
(tests/roadmap_ref/roadmap_ref.cpp, rr_plan(leg=REFERENCE_ASTAR)) bit for bit; the global route against the LDS route; the tree's
cache and counters left alone; the edge cases as the tree has them; the per-call search= keyword."""
import importlib
import zlib

import numpy as np
import pytest

import planner_ref as P
import roadmap_ref as R
import tour_ref as T

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05
COLS = ("path_length", "path_length_m", "path_heading", "achievable")


def _maps():
    """test_gpu_roadmap.py's maps: REF2D's map, floor plans up to 1024^2, a non-square map, the spiral corridor"""
    out = [("REF2D", fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])]
    rng = np.random.Generator(np.random.PCG64(5151))
    for k, n in enumerate([64, 96, 128, 160, 200, 256, 300, 384, 512, 640, 768, 1024]):
        out.append((f"plan{k}_{n}", fsmod.synth.make_grid(rng, n, 1)[0]))
    out.append(("non_square", fsmod.synth.make_grid(rng, 256, 1)[0][:170, :]))
    out.append(("spiral", P.spiral_map(512)[0]))
    return [(name, np.ascontiguousarray(c), (-c.shape[1] * RES / 2, -c.shape[0] * RES / 2, 0.0)) for name, c in out]


PLAN_MAPS = ("REF2D", "plan5_256", "plan8_512", "plan11_1024", "non_square", "spiral")
MAPS = [m for m in _maps() if m[0] in PLAN_MAPS + ("plan2_128",)]


def _map(name):
    return next((c, o) for n, c, o in MAPS if n == name)


def _nodes(cells, origin, seed, k):
    """test_gpu_roadmap.py's node sets: free and unknown cells, jittered inside the cell"""
    rng = np.random.default_rng(seed)
    xs, ys = P.free_cells(cells, rng, k)
    if (cells == 255).any():
        ux, uy = P.free_cells(cells, rng, k // 5, value=255)
        xs[: k // 5], ys[: k // 5] = ux, uy
    return np.stack([origin[0] + (xs + rng.uniform(0, 1, k)) * RES, origin[1] + (ys + rng.uniform(0, 1, k)) * RES], axis=1)


def _goals(cells, origin, seed, n, robot_xy):
    """test_gpu_roadmap.py's goal lists: free cells, two off the map, one at the robot, 10 % not achievable on input"""
    rng = np.random.default_rng(seed)
    ny, nx = cells.shape
    xs, ys = P.free_cells(cells, rng, n)
    g = np.zeros((n, 3))
    g[:, 0] = origin[0] + (xs + rng.uniform(0, 1, n)) * RES
    g[:, 1] = origin[1] + (ys + rng.uniform(0, 1, n)) * RES
    if n >= 10:
        g[1, 0] = origin[0] - 1.0
        g[5, 1] = origin[1] + (ny + 3) * RES
        g[7, :2] = robot_xy
    ach = (rng.random(n) > 0.1).astype(np.uint8)
    return g, ach


def _setup(name, cells=None, origin=None):
    if cells is None:
        cells, origin = _map(name)
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    ref = R.Roadmap(cells, origin, RES)
    pts = _nodes(cells, origin, zlib.crc32(name.encode()), int(min(1500, max(40, cells.size * RES * RES / 2))))
    assert ref.populate(pts) == 0
    sc.roadmap_add_nodes(pts)
    ref.rebuild(); sc.roadmap_rebuild()
    return sc, ref, pts


def _same(got, want, what):
    for k in COLS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _free(n):
    return np.zeros((n, n), dtype=np.uint8)


def test_four_node_graph_reference_gives_the_direct_edge():
    """S -> G directly (g = 4) against the g-shorter detour (3.12): the reference's A* pops G first and returns 2 m, the tree the
    3.06 m detour.  Fails without the REFERENCE search."""
    origin = (-1.0, -1.0, 0.0)
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(_free(160)[None], origin, RES)
        sc.set_roadmap_params(radius_to_decide_edges=3.0)
        sc.roadmap_add_nodes([[0.0, 0.0], [2.0, 0.0], [0.5, 0.9], [1.5, 0.9]])
        sc.roadmap_rebuild()
        goal = [[2.0, 0.0, 0.0]]
        sc.set_roadmap_search("reference")
        astar = sc.roadmap_plan(R.pose7(0.0, 0.0), goal)
        sc.set_roadmap_search("tree")
        tree = sc.roadmap_plan(R.pose7(0.0, 0.0), goal)
        assert astar["achievable"][0] == tree["achievable"][0] == 1
        assert astar["path_length_m"][0] == 2.0
        assert tree["path_length_m"][0] == pytest.approx(np.sqrt(0.25 + 0.81) * 2 + 1.0, abs=1e-12)
    finally:
        sc.close()


@pytest.mark.parametrize("name", PLAN_MAPS)
def test_plan_equals_reference_astar(name):
    cells, origin = _map(name)
    sc, ref, pts = _setup(name, cells, origin)
    try:
        sc.set_roadmap_search("reference")
        seed = zlib.crc32(name.encode())
        rng = np.random.default_rng(seed + 7)
        reached = 0
        for trial in range(2):
            rx, ry = pts[rng.integers(pts.shape[0])] + rng.uniform(-0.3, 0.3, 2)
            pose = R.pose7(rx, ry, 0.7 * trial + 0.2)
            for n in (1, 50, 2000):
                goals, ach = _goals(cells, origin, seed + n + trial, n, (rx, ry))
                got = sc.roadmap_plan(pose, goals, achievable_in=ach)
                want = ref.plan(pose, goals, achievable_in=ach, leg=R.REFERENCE_ASTAR)
                _same(got, want, (name, trial, n))
                reached += int(got["achievable"].sum())
        assert reached > 0
        assert sc.get_counter(1021) > 0 and sc.get_counter(1022) > 0
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("step,radius", [(0.5, 2.1), (1.0, 3.1)])
def test_plan_equals_reference_astar_on_lattices(step, radius):
    """nodes on a lattice over a free map: many records tie in f, and the heap's order of ties decides answers"""
    n = 220
    origin = (-1.0, -1.0, 0.0)
    cells = _free(n)
    side = np.arange(origin[0] + 0.25, origin[0] + n * RES - 0.25, step)
    gx, gy = np.meshgrid(side, side)
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
    sc = fsmod.FrontierScorer(device=0)
    ref = R.Roadmap(cells, origin, RES, radius=radius)
    try:
        sc.upload_grid(cells[None], origin, RES)
        sc.set_roadmap_params(radius_to_decide_edges=radius)
        assert ref.populate(pts) == 0
        sc.roadmap_add_nodes(pts)
        ref.rebuild(); sc.roadmap_rebuild()
        sc.set_roadmap_search("reference")
        rng = np.random.default_rng(int(step * 10))
        goals = np.zeros((100, 3))
        for i in rng.integers(0, pts.shape[0], 20):
            goals[:, :2] = pts[rng.integers(0, pts.shape[0], 100)]
            pose = R.pose7(*pts[i])
            _same(sc.roadmap_plan(pose, goals), ref.plan(pose, goals, leg=R.REFERENCE_ASTAR), (step, i))
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("with_fim", [False, True])
def test_fused_equals_plan_then_costs(with_fim):
    w = fsmod.synth.make_workload("REF2D", n_cand=300, n_landmarks=20_000)
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
        sc.set_roadmap_search("reference")
        pose = R.pose7(*w.goals[0, :2], 1.0)
        plan = sc.roadmap_plan(pose, w.goals)
        want = sc.get_frontier_costs(w.goals, plan["path_length"], plan["path_heading"], frontier_size=w.frontier_size,
                                     blacklisted=w.blacklisted, achievable_in=plan["achievable"], with_fim=with_fim)
        got = sc.get_frontier_costs_roadmap(pose, w.goals, frontier_size=w.frontier_size, blacklisted=w.blacklisted, with_fim=with_fim)
        for k in ("weighted_cost", "arrival_utility", "distance_utility", "order"):
            assert got[k].tobytes() == want[k].tobytes(), k
        floats = ("info_ref", "trace", "logdet") if with_fim else ()
        for k in got["records"].dtype.names:
            if k in floats:
                np.testing.assert_allclose(got["records"][k], want["records"][k], rtol=5e-6, atol=1e-6, err_msg=k)
            else:
                assert got["records"][k].tobytes() == want["records"][k].tobytes(), k
        assert got["path_length_m"].tobytes() == plan["path_length_m"].tobytes()
        assert plan["achievable"].sum() > 1
        tree = sc.roadmap_plan(pose, w.goals, search="tree")
        assert tree["achievable"].tobytes() == plan["achievable"].tobytes()
    finally:
        sc.close()


def _astar_matrix(ref, pts, radius):
    """the pair matrix of getNextGoal with getPlan as the reference's A*: rr_plan(leg=1) from point i (the robot) to point j"""
    m = pts.shape[0]
    M = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1, m):
            p = ref.plan(R.pose7(*pts[i]), np.array([[pts[j, 0], pts[j, 1], 0.0]]), leg=R.REFERENCE_ASTAR)
            M[i, j] = M[j, i] = p["path_length_m"][0] if p["achievable"][0] else radius * 100000
    return M


@pytest.mark.parametrize("name", ["REF2D", "plan2_128", "plan5_256"])
def test_next_goal_equals_reference_astar_pairs(name):
    radius = 12.0
    cells, origin = _map(name)
    sc, ref, pts = _setup(name, cells, origin)
    try:
        sc.set_roadmap_search("reference")
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 13)
        reached = 0
        for k in range(1, 9):
            robot = pts[rng.integers(pts.shape[0])] + rng.uniform(-0.3, 0.3, 2)
            n = k + 5
            goal = np.zeros((n, 3))
            xs, ys = P.free_cells(cells, rng, n)
            goal[:, 0] = origin[0] + (xs + rng.uniform(0, 1, n)) * RES
            goal[:, 1] = origin[1] + (ys + rng.uniform(0, 1, n)) * RES
            plm = np.concatenate([np.sort(rng.uniform(0.5, radius, k + 1)), rng.uniform(radius + 0.1, 60.0, 4)])
            if k >= 3:
                goal[1, :2] = robot
            ach = np.ones(n, np.uint8)
            got = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=k, local_radius=radius, want_matrix=True,
                                       want_selection=True)
            el = T.eligible(goal, ach)
            loc, glob, cg = T.select(plm, el, k, radius)
            assert got["n_locals"] == len(loc) == k
            pp = np.concatenate([robot.reshape(1, 2), goal[loc, :2], goal[[cg], :2]])
            M = _astar_matrix(ref, pp, radius)
            assert got["pair_length_m"].tobytes() == M.tobytes(), (name, k)
            L, cnt, perm, _ = T.tour(M)
            assert np.float64(got["tour_length"]).tobytes() == np.float64(L).tobytes() and got["n_tied"] == cnt, (name, k)
            if L < radius * 100000:
                tour = [loc[p] for p in perm] + [cg]
                assert got["tour"].tolist() == tour and got["next_index"] == tour[0], (name, k)
            else:
                assert got["next_index"] == -1
            reached += int((M < radius * 100000).sum() > k + 2)
        assert reached > 0
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("cap", [0, 24])
def test_global_route_equals_lds_route(cap):
    name = "plan8_512"
    cells, origin = _map(name)
    sc, ref, pts = _setup(name, cells, origin)
    try:
        sc.set_roadmap_search("reference")
        rng = np.random.default_rng(99)
        rx, ry = pts[rng.integers(pts.shape[0])]
        pose = R.pose7(rx, ry, 0.3)
        goals, ach = _goals(cells, origin, 100, 2000, (rx, ry))
        lds = sc.roadmap_plan(pose, goals, achievable_in=ach)
        assert sc.get_counter(1023, reset=True) == 0
        sc.set_option("roadmap.astar_lds_entries", cap)
        glob = sc.roadmap_plan(pose, goals, achievable_in=ach)
        _same(glob, lds, cap)
        assert sc.get_counter(1023) > 0
        if cap == 0:
            assert sc.get_counter(1023) == sc.get_counter(1021, reset=True) // 2
        robot = pts[3]
        k = 5
        goal = np.zeros((k + 3, 3))
        goal[:, :2] = pts[rng.integers(0, pts.shape[0], k + 3)]
        plm = np.concatenate([np.sort(rng.uniform(0.5, 12.0, k + 1)), [20.0, 30.0]])
        a = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, np.ones(k + 3, np.uint8), n_local=k, want_matrix=True)
        sc.set_option("roadmap.astar_lds_entries", 2048)
        b = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, np.ones(k + 3, np.uint8), n_local=k, want_matrix=True)
        assert a["pair_length_m"].tobytes() == b["pair_length_m"].tobytes()
        assert a["tour"].tolist() == b["tour"].tolist()
        _same(sc.roadmap_plan(pose, goals, achievable_in=ach), ref.plan(pose, goals, achievable_in=ach, leg=R.REFERENCE_ASTAR), name)
    finally:
        sc.close(); ref.close()


def test_reference_calls_leave_the_tree_cache_alone():
    sc, ref, pts = _setup("REF2D")
    try:
        cells, origin = _map("REF2D")
        goals, _ = _goals(cells, origin, 4, 50, (0.0, 0.0))
        pose = R.pose7(*pts[0])
        sc.get_counter(1005, reset=True)
        tree = sc.roadmap_plan(pose, goals)
        rounds = sc.get_counter(1006)
        assert sc.get_counter(1005) == 1 and rounds > 0
        sc.set_roadmap_search("reference")
        astar = sc.roadmap_plan(pose, goals)
        sc.roadmap_plan(R.pose7(*pts[1]), goals)
        assert sc.get_counter(1005) == 1 and sc.get_counter(1006) == rounds
        sc.set_roadmap_search("tree")
        again = sc.roadmap_plan(pose, goals)
        assert sc.get_counter(1005) == 1                              # the cached tree is still the one used
        _same(again, tree, "tree after reference")
        _same(astar, ref.plan(pose, goals, leg=R.REFERENCE_ASTAR), "reference")
        assert astar["achievable"].tobytes() == tree["achievable"].tobytes()
    finally:
        sc.close(); ref.close()


def test_edge_cases_as_the_tree_has_them():
    cells = np.zeros((80, 80), dtype=np.uint8)
    origin = (0.0, 0.0, 0.0)
    sc = fsmod.FrontierScorer(device=0)
    ref = R.Roadmap(cells, origin, RES)
    try:
        sc.upload_grid(cells[None], origin, RES)
        pose = R.pose7(1.0, 1.0)
        goals = np.array([[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [30.0, 1.0, 0.0]])
        for stage in ("empty", "keyless"):
            got = sc.roadmap_plan(pose, goals, search="reference")
            _same(got, sc.roadmap_plan(pose, goals, search="tree"), stage)
            _same(got, ref.plan(pose, goals, leg=R.REFERENCE_ASTAR), stage)
            assert got["achievable"].tolist() == [1, 0, 0] and got["path_length_m"][0] == 0.0
            ref.populate([[1.5, 1.5], [2.5, 2.5]]); sc.roadmap_add_nodes([[1.5, 1.5], [2.5, 2.5]])
        sc.roadmap_connect([[1.5, 1.5]]); ref.connect([[1.5, 1.5]])
        got = sc.roadmap_plan(pose, goals, search="reference")
        _same(got, ref.plan(pose, goals, leg=R.REFERENCE_ASTAR), "connected")
        assert got["achievable"].tolist() == [1, 1, 1]
        # a 3-D grid: the roadmap calls refuse it or plan on the roadmap alone, as under the tree
        sc.upload_grid(np.zeros((4, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        _same(sc.roadmap_plan(pose, goals, search="reference"), got, "3-D grid")
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_rebuild()
        assert e.value.code == fsmod.capi.FS_E_INVALID
    finally:
        sc.close(); ref.close()


def test_search_keyword_restores_the_setting():
    sc, ref, pts = _setup("REF2D")
    try:
        cells, origin = _map("REF2D")
        goals, _ = _goals(cells, origin, 5, 50, (0.0, 0.0))
        pose = R.pose7(*pts[2])
        tree = sc.roadmap_plan(pose, goals)
        astar = sc.roadmap_plan(pose, goals, search="reference")
        _same(astar, ref.plan(pose, goals, leg=R.REFERENCE_ASTAR), "keyword")
        _same(sc.roadmap_plan(pose, goals), tree, "restored to tree")
        assert sc._roadmap_search == "tree"
        sc.set_roadmap_search("reference")
        _same(sc.roadmap_plan(pose, goals, search="tree"), tree, "keyword tree")
        _same(sc.roadmap_plan(pose, goals), astar, "restored to reference")
        sc.set_roadmap_params(radius_to_decide_edges=6.1)               # keeps the setting (and empties the roadmap)
        assert sc._roadmap_search == "reference"
        with pytest.raises(fsmod.FsError) as e:
            sc.set_roadmap_search("dijkstra")
        assert e.value.code == fsmod.capi.FS_E_INVALID
        assert sc._L.fs_set_roadmap_search(sc._h, 2) == fsmod.capi.FS_E_INVALID
        assert sc._roadmap_search == "reference"
    finally:
        sc.close(); ref.close()
