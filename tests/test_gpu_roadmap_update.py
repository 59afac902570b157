"""fs_roadmap_update (UpdateRoadmapBT decided on the device) and fs_get_frontier_costs_searched_roadmap.  Every
roadmap is compared bit for bit — xy, key, row_ptr, col of roadmap_graph(), plus the pending count of roadmap_anchors() — against the
sequential CPU restatement (tests/roadmap_ref/roadmap_ref.cpp) and against a second context that runs the three-call sequence
fs_roadmap_add_nodes, fs_roadmap_add_nodes(robot), fs_roadmap_connect."""
import importlib

import numpy as np
import pytest

import frontier_search_maps as M
import planner_ref as P
import roadmap_ref as R

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05
DEFAULTS = (1.0, 6.1, 0.25, 0.25)


class Trio:
    """the context under test, the context of the three calls, the sequential restatement: one grid, one parameter set"""

    def __init__(self, cells, origin, params=DEFAULTS):
        self.cells, self.origin, self.params = np.ascontiguousarray(cells, dtype=np.uint8), origin, params
        self.new, self.old = fsmod.FrontierScorer(device=0), fsmod.FrontierScorer(device=0)
        for sc in (self.new, self.old):
            sc.upload_grid(self.cells[None], origin, RES)
            sc.set_roadmap_params(*params)
        self.ref = R.Roadmap(self.cells, origin, RES, *params)

    def close(self):
        self.new.close(); self.old.close(); self.ref.close()

    def seed(self, pts, rebuild=False):
        """existing nodes by the old calls on all three"""
        for sc in (self.new, self.old):
            sc.roadmap_add_nodes(pts)
            if rebuild:
                sc.roadmap_rebuild()
        assert self.ref.populate(pts) == 0
        if rebuild:
            self.ref.rebuild()

    def rebuild(self):
        self.new.roadmap_rebuild(); self.old.roadmap_rebuild(); self.ref.rebuild()

    def update(self, pts, robot, add_robot=True, what=""):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
        robot = np.asarray(robot, dtype=np.float64).reshape(2)
        # the restatement, sequentially
        rc = self.ref.populate(pts) if pts.shape[0] else 0
        if rc == 0 and add_robot:
            rc = self.ref.populate(robot[None], True)
        if rc == 0:
            self.ref.connect(np.concatenate([pts, robot[None]]))
        # the three calls
        rc_old = 0
        try:
            self.old.roadmap_add_nodes(pts)
            if add_robot:
                self.old.roadmap_add_nodes(robot[None], is_robot_pose=True)
            self.old.roadmap_connect(np.concatenate([pts, robot[None]]))
        except fsmod.FsError as e:
            rc_old = e.code
        # the one call
        rc_new, out = 0, None
        before = self.new.roadmap_graph()
        try:
            out = self.new.roadmap_update(pts, robot, add_robot_pose=add_robot)
        except fsmod.FsError as e:
            rc_new = e.code
        assert rc_new == rc_old == rc, (what, rc_new, rc_old, rc)
        got, want, seq = self.new.roadmap_graph(), self.ref.graph(), self.old.roadmap_graph()
        for k in ("xy", "key", "row_ptr", "col"):
            assert got[k].tobytes() == want[k].tobytes(), (what, k, "restatement")
            assert got[k].tobytes() == seq[k].tobytes(), (what, k, "three calls")
        assert self.new.roadmap_anchors()["n_pending"] == self.old.roadmap_anchors()["n_pending"], what
        if out is not None:
            assert out["n_nodes_added"] + int(out["robot_added"]) == got["xy"].shape[0] - before["xy"].shape[0], what
            assert 2 * out["n_edges_added"] == got["col"].size - before["col"].size, what
        return rc_new, out


def _free(ny, nx):
    return np.zeros((ny, nx), np.uint8)


def _tick_maps():
    ref2d = fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0]
    plan = fsmod.synth.make_grid(np.random.Generator(np.random.PCG64(5151)), 256, 1)[0]
    return [(name, np.ascontiguousarray(c), (-c.shape[1] * RES / 2, -c.shape[0] * RES / 2, 0.0)) for name, c in (("REF2D", ref2d), ("plan256", plan))]


TICK_MAPS = _tick_maps()


@pytest.mark.parametrize("name,cells,origin", TICK_MAPS, ids=[m[0] for m in TICK_MAPS])
def test_ticks_equal_the_sequence_and_the_restatement(name, cells, origin):
    rng = np.random.default_rng(77 + len(name))
    xs, ys = P.free_cells(cells, rng, 5)
    ticks = R.grow_ticks(fsmod, cells, origin, RES, list(zip(xs.tolist(), ys.tolist())))
    t = Trio(cells, origin)
    try:
        walks = 0
        for k, (frontiers, robot) in enumerate(ticks):
            rc, out = t.update(frontiers, robot, what=(name, k))
            assert rc == 0
            walks += out["n_walks"]
        assert t.ref.graph()["col"].size > 0 and walks > 0
        t.rebuild()
        rc, _ = t.update(ticks[0][0], ticks[1][1], what=(name, "after rebuild"))
        assert rc == 0
    finally:
        t.close()


def _directional_grid():
    cells = _free(64, 64)
    cells[23, 25] = 254
    centre = lambda x, y: [(x + 0.5) * RES, (y + 0.5) * RES]
    return cells, centre(20, 20), centre(30, 25), centre(22, 30)


def test_the_two_walk_directions_differ():
    cells, A, B, _ = _directional_grid()
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(cells[None], (0.0, 0.0, 0.0), RES)
        seg = sc.trace_segments(np.array([A + [0.0], B + [0.0]]), np.array([B + [0.0], A + [0.0]]), float(int(2.0 * 1.5 / RES)))
        assert bool(seg["hit"][0]) and not bool(seg["hit"][1])
    finally:
        sc.close()


@pytest.mark.parametrize("rebuilt", [False, True])
@pytest.mark.parametrize("order", ["ABC", "BAC", "CBA"])
def test_directional_pair(order, rebuilt):
    cells, A, B, Cn = _directional_grid()
    pts = [dict(A=A, B=B, C=Cn)[c] for c in order]
    t = Trio(cells, (0.0, 0.0, 0.0), (1.0, 2.0, 0.25, 0.25))
    try:
        if rebuilt:
            # the rebuild links A -> B one way only (its list of A walks B -> A, its list of B walks A -> B): the "linked either way
            # before the call" skip
            t.seed(pts, rebuild=True)
            g = t.ref.graph()
            ia, ib = order.index("A"), order.index("B")
            assert ib in g["col"][g["row_ptr"][ia]:g["row_ptr"][ia + 1]] and ia not in g["col"][g["row_ptr"][ib]:g["row_ptr"][ib + 1]]
        rc, out = t.update(pts, Cn, add_robot=False, what=(order, rebuilt))
        assert rc == 0
        if not rebuilt:
            g = t.new.roadmap_graph()
            ia, ib = order.index("A"), order.index("B")
            assert out["n_nodes_added"] == 3 and ib in g["col"][g["row_ptr"][ia]:g["row_ptr"][ia + 1]]
    finally:
        t.close()


CHAIN = np.stack([-19.9 + 0.2 * np.arange(200), np.full(200, 0.05)], axis=1)        # crosses x = 0 and 40 hash cells


@pytest.mark.parametrize("near_first", [False, True])
@pytest.mark.parametrize("how", ["in_order", "reversed", "shuffled"])
def test_conflict_chain(how, near_first):
    pts = dict(in_order=CHAIN, reversed=CHAIN[::-1], shuffled=CHAIN[np.random.default_rng(5).permutation(200)])[how]
    t = Trio(_free(40, 840), (-21.0, -1.0, 0.0))
    try:
        if near_first:
            # 0.1 m outside the chain's first point: only that point is rejected, and the parity of the whole chain flips
            t.seed([[float(pts[0, 0]) - (0.1 if how == "in_order" else -0.1), 0.05]])
        rc, out = t.update(pts, [0.0, 0.5], what=(how, near_first))
        assert rc == 0
        if how != "shuffled":
            assert near_first or out["n_nodes_added"] == 100     # every other point
            assert t.new.get_counter(1035) >= 100                # a chain settles one point per round
    finally:
        t.close()


def test_one_owner_many_points():
    rng = np.random.default_rng(11)
    t = Trio(_free(200, 200), (-5.0, -5.0, 0.0))
    try:
        t.seed([[0.3, 0.3], [2.0, 0.3], [0.3, 3.0], [-3.0, -3.0]])
        ang, rad = rng.uniform(0, 2 * np.pi, 300), rng.uniform(0, 0.05, 300)
        pts = np.stack([0.3 + rad * np.cos(ang), 0.3 + rad * np.sin(ang)], axis=1)
        rc, out = t.update(pts, [0.3, 0.3], add_robot=False, what="one owner")
        assert rc == 0 and out["n_nodes_added"] == 0 and t.new.get_counter(1034) == 1 and out["n_walks"] == 3
    finally:
        t.close()


def test_edges_of_the_domain():
    t = Trio(_free(200, 200), (-5.0, -5.0, 0.0))
    try:
        # nothing at all on an empty roadmap
        rc, out = t.update(np.zeros((0, 2)), [0.0, 0.0], add_robot=False, what="no-op")
        assert rc == 0 and out["n_nodes_added"] == 0 and not out["robot_added"] and t.new.roadmap_graph()["xy"].shape[0] == 0
        # the first update of an empty roadmap
        rc, out = t.update([[1.0, 1.0], [2.0, 1.0], [1.1, 1.0]], [0.0, 0.0], what="first")
        assert rc == 0 and out["n_nodes_added"] == 2 and out["robot_added"] and out["n_edges_added"] == 3
        # n = 0 with the robot only
        rc, out = t.update(np.zeros((0, 2)), [-2.0, -2.0], what="robot only")
        assert rc == 0 and out["robot_added"] and out["n_edges_added"] == 3
        # the robot pose within 0.25 m of a node: not added, still connected through its closest node
        rc, out = t.update([[3.5, 3.5]], [1.05, 1.1], what="robot near a node")
        assert rc == 0 and not out["robot_added"] and out["n_nodes_added"] == 1 and out["n_edges_added"] >= 1
        # add_robot_pose = False
        rc, out = t.update([[-3.0, 3.0]], [4.0, -4.0], add_robot=False, what="no robot node")
        assert rc == 0 and not out["robot_added"] and out["n_nodes_added"] == 1
        # a list of one
        rc, out = t.update([[0.5, -3.0]], [0.5, -3.1], what="one")
        assert rc == 0 and out["n_nodes_added"] == 1 and not out["robot_added"]
        # points off the map: added as nodes, their walks fail, no edge
        e0 = t.new.roadmap_graph()["col"].size
        rc, out = t.update([[7.0, 0.0], [0.0, -6.5], [-5.2, -5.2]], [6.0, 6.0], what="off the map")
        assert rc == 0 and out["n_nodes_added"] == 3 and out["robot_added"] and out["n_walks"] > 0
        assert out["n_edges_added"] == 0 and t.new.roadmap_graph()["col"].size == e0
    finally:
        t.close()


@pytest.mark.parametrize("robot_trips", [False, True])
def test_twenty_per_cell(robot_trips):
    t = Trio(_free(200, 200), (-5.0, -5.0, 0.0), (1.0, 6.1, 0.01, 0.01))
    try:
        lattice = np.array([[1.1 + 0.15 * i, 2.1 + 0.15 * j] for i in range(5) for j in range(5)])     # 25 points of hash cell (1, 2)
        t.seed(np.concatenate([lattice[:15], [[-2.0, -2.0], [3.5, 0.5]]]), rebuild=True)
        e0 = t.new.roadmap_graph()["col"].size
        if robot_trips:
            pts, robot = np.concatenate([lattice[15:20], [[0.5, 0.5]]]), lattice[20]
        else:
            pts, robot = np.concatenate([[[0.5, 0.5]], lattice[15:25]]), [0.0, 0.0]
        rc, out = t.update(pts, robot, what=("20 per cell", robot_trips))
        assert rc == fsmod.capi.FS_E_RANGE and out is None
        g = t.new.roadmap_graph()
        assert g["xy"].shape[0] == 17 + 7 and g["col"].size == e0          # 15 + 6 in the cell, the far point; no edge added
        assert t.new.roadmap_anchors()["n_pending"] == 17 + 7
        t.rebuild()                                                        # the roadmap is still usable
        for k in ("xy", "key", "row_ptr", "col"):
            assert t.new.roadmap_graph()[k].tobytes() == t.ref.graph()[k].tobytes(), k
    finally:
        t.close()


def test_invalid_input_changes_nothing():
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(_free(100, 100)[None], (0.0, 0.0, 0.0), RES)
        sc.roadmap_update([[1.0, 1.0], [2.0, 2.0]], [3.0, 3.0])
        before = sc.roadmap_graph()
        pending = sc.roadmap_anchors()["n_pending"]

        def unchanged():
            g = sc.roadmap_graph()
            return all(g[k].tobytes() == before[k].tobytes() for k in before) and sc.roadmap_anchors()["n_pending"] == pending
        for pts, robot in (([[4.0, 4.0], [np.nan, 1.0]], [1.0, 1.0]), ([[4.0, 4.0]], [np.inf, 0.0])):
            with pytest.raises(fsmod.FsError) as e:
                sc.roadmap_update(pts, robot)
            assert e.value.code == fsmod.capi.FS_E_INVALID and unchanged()
        sc.upload_grid(np.zeros((2, 100, 100), np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_update([[4.0, 4.0]], [1.0, 1.0])
        assert e.value.code == fsmod.capi.FS_E_INVALID and unchanged()
    finally:
        sc.close()


def _setup_scoring(sc, w):
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    sc.set_option("fim.learn", 0)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    sc.set_fim_params(14.0, 1.0)
    sc.set_arrival_limits(4000.0, sc.max_arrival()["min_gt"])


@pytest.mark.parametrize("search", ["tree", "reference"])
@pytest.mark.parametrize("which", ["REF2D", "plan256"])
def test_one_call_tick_equals_the_three_stages(fs, which, search):
    w = fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=2000) if which == "REF2D" else fs.synth.make_small_2d(7, n=256, n_cand=40)
    cells = w.cells[0]
    free = len(np.argwhere(cells == 0))
    one, three = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for sc in (one, three):
            _setup_scoring(sc, w)
            sc.set_roadmap_search(search)
        found = 0
        for tick, k in enumerate((free // 3, free // 3 + 40, free // 2)):
            pos = M._free_pos(cells, w.origin, w.resolution, k)
            pose = np.array([pos[0], pos[1], 0.0, 0.0, 0.0, np.sin(0.2 * tick), np.cos(0.2 * tick)])
            fim = tick == 2
            fr, _ = three.search_frontiers(pos, want_every=False)
            three.roadmap_update(np.stack([fr["goal_x"], fr["goal_y"]], axis=1), pos)
            got_fr, got = one.get_frontier_costs_searched_roadmap(pose, with_fim=fim)
            assert got_fr.tobytes() == fr.tobytes(), (which, tick)
            found += fr.shape[0]
            g1, g3 = one.roadmap_graph(), three.roadmap_graph()
            for key in ("xy", "key", "row_ptr", "col"):
                assert g1[key].tobytes() == g3[key].tobytes(), (which, tick, key)
            assert one.roadmap_anchors()["n_pending"] == three.roadmap_anchors()["n_pending"]
            if fr.shape[0] == 0:
                continue
            goal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], axis=1)
            want = three.get_frontier_costs_roadmap(pose, goal, frontier_size=fr["size"], with_fim=fim)
            for key in want:
                if key == "records":
                    for f in want[key].dtype.names:
                        if f in ("info_ref", "trace", "logdet"):          # the Fisher float sums: not run-to-run bit-stable
                            continue
                        assert got[key][f].tobytes() == want[key][f].tobytes(), (which, tick, f)
                else:
                    assert got[key].tobytes() == want[key].tobytes(), (which, tick, key)
        assert found > 3 and one.roadmap_graph()["col"].size > 0
    finally:
        one.close(); three.close()
