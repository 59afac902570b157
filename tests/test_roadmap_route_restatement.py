"""The CPU restatement of the roadmap routes (tests/roadmap_route_ref/roadmap_route_ref.cpp) against the roadmap
restatement it builds on: the node chains it returns sum, from the goal end, to rr_plan's lengths bit for bit under both legs, the
routes are numbered by distinct goal node, and refinePath does what FrontierRoadmap.cpp:657-714 does on a corridor made by hand."""
import numpy as np
import pytest

import roadmap_ref as R
import roadmap_route_maps as M
import roadmap_route_ref as RR

RES = M.RES
COLS = ("path_length", "path_length_m", "path_heading", "achievable")


@pytest.fixture(scope="module", params=["REF2D", "plan5_256"])
def world(request):
    ref, cells, origin, _ = M.restated_roadmap(request.param)
    yield request.param, ref, cells, origin
    ref.close()


@pytest.mark.parametrize("leg", [R.REFERENCE_ASTAR, R.TREE])
def test_chain_lengths_equal_the_plan(world, leg):
    name, ref, cells, origin = world
    xy = ref.graph()["xy"]
    pose = M.robot_pose(cells, origin)
    goals = M.goals_at_nodes(xy)
    goals = np.concatenate([goals, [[pose[0], pose[1], 0.0], [origin[0] - 1.0, origin[1], 0.0]]])
    ach = np.ones(goals.shape[0], np.uint8)
    ach[::9] = 0
    plan = ref.plan(pose, goals, achievable_in=ach, leg=leg)
    got = ref.routes(pose, goals, achievable_in=ach, leg=leg)
    root = ref.closest(pose[0], pose[1])
    planned = 0
    for i in range(goals.shape[0]):
        q = got["route_of"][i]
        is_robot = goals[i, 0] == pose[0] and goals[i, 1] == pose[1]
        assert (q >= 0) == (plan["achievable"][i] == 1 and not is_robot), i
        if q < 0:
            continue
        nodes = got["node"][got["node_offset"][q]:got["node_offset"][q + 1]]
        assert nodes[0] == root and nodes[-1] == got["goal_node"][q] == ref.closest(goals[i, 0], goals[i, 1])
        assert np.float64(RR.summed_from_goal_end(xy, nodes)).tobytes() == plan["path_length_m"][i].tobytes(), (name, leg, i)
        assert got["length_m"][q].tobytes() == plan["path_length_m"][i].tobytes()
        planned += 1
    assert planned > 30
    # one route per distinct goal node, ascending
    assert (np.diff(got["goal_node"]) > 0).all()
    assert set(got["route_of"][got["route_of"] >= 0].tolist()) == set(range(got["goal_node"].size))
    if leg == R.TREE:
        t = ref.tree(root)
        assert (np.diff(got["node_offset"]) == t["hops"][got["goal_node"]] + 1).all()


def test_the_tree_prefers_short_hops_and_refinement_undoes_them(world):
    """the measurement behind the feature: most tree routes get strictly shorter"""
    name, ref, cells, origin = world
    xy = ref.graph()["xy"]
    r = ref.routes(M.robot_pose(cells, origin), M.goals_at_nodes(xy), leg=R.TREE)
    f = ref.refine(r["node_offset"], r["node"])
    raw, new = np.diff(r["node_offset"]), np.diff(f["refined_offset"])
    assert (new <= raw).all() and (new < raw).sum() * 2 >= raw.size
    # a refined list is a subsequence of its route that starts at its start and, when complete, ends at its goal
    for q in range(raw.size):
        P = r["node"][r["node_offset"][q]:r["node_offset"][q + 1]].tolist()
        L = f["refined_node"][f["refined_offset"][q]:f["refined_offset"][q + 1]].tolist()
        it = iter(P)
        assert L[0] == P[0] and all(v in it for v in L)
        assert (L[-1] == P[-1]) == bool(f["complete"][q]) or len(P) == 1


def _corridor(wall=False):
    """five nodes on a free 200 x 80 grid: 0 -> 1 -> 2 along y = 1, then 3 and 4 round a corner.  With the wall (cells x = 60, y < 40,
    lethal) node 0 sees 1 only."""
    cells = np.zeros((80, 200), np.uint8)
    if wall:
        cells[:40, 60] = 254
    origin = (0.0, 0.0, 0.0)
    pts = np.array([[0.5, 1.0], [2.5, 1.0], [4.5, 1.0], [6.5, 1.5], [8.5, 3.0]])
    return cells, origin, pts


def test_corridor_with_a_known_shortcut():
    cells, origin, pts = _corridor()
    ref = RR.RouteRoadmap(cells, origin, RES, radius=2.6)
    try:
        assert ref.populate(pts) == 0
        ref.rebuild()
        g = ref.graph()
        # radius 2.6: only neighbours in the chain are linked (0-1, 1-2, 2-3, 3-4: 2.0, 2.0, 2.06, 2.5 m)
        assert [g["col"][g["row_ptr"][p]:g["row_ptr"][p + 1]].tolist() for p in range(5)] == [[1], [0, 2], [1, 3], [2, 4], [3]]
        for leg in (R.TREE, R.REFERENCE_ASTAR):
            r = ref.routes(R.pose7(0.5, 1.0), [[8.5, 3.0, 0.0]], leg=leg)
            assert r["node"].tolist() == [0, 1, 2, 3, 4] and r["route_of"].tolist() == [0]
        # isConnectable reaches (unsigned)(1.5 * 2.6 / 0.05) = 78 cells = 3.9 m: from 0 node 1 passes (2 m) and node 2 (4 m) passes too —
        # the walk is cut at max_length and nothing lies on it — so the scan runs on to the end: the free grid refines to [0, 4]
        f = ref.refine(r["node_offset"], r["node"])
        assert f["refined_node"].tolist() == [0, 4] and f["complete"].tolist() == [1] and f["walks"] == 4
        # a lethal wall between nodes 1 and 2 below y = 2 m: 0 -> 1 passes, 0 -> 2 hits it, so 1 is kept; 1 -> 2 hits it too: truncated
        ref.cells = _corridor(wall=True)[0]
        f = ref.refine(r["node_offset"], r["node"])
        assert f["refined_node"].tolist() == [0, 1] and f["complete"].tolist() == [0] and f["walks"] == 3
        # ... the wall moved so that only the far end is hidden from node 0: 0 sees 1, 2 (walks cut short of the wall) but not 3
        cells2 = np.zeros((80, 200), np.uint8)
        cells2[:25, 110] = 254                                   # x = 5.5 m, y < 1.25 m: crosses y = 1 between nodes 2 and 3
        ref.cells = cells2
        f = ref.refine(r["node_offset"], r["node"])
        # 0 -> 3 is cut at 3.9 m (before the wall) and passes, 0 -> 4 likewise: the wall is never seen from node 0
        assert f["refined_node"].tolist() == [0, 4] and f["complete"].tolist() == [1]
        poses = ref.leg_poses(f["refined_offset"], f["refined_node"])
        yaw = np.arctan2(3.0 - 1.0, 8.5 - 0.5)
        assert poses.shape == (1, 7) and poses[0, :3].tolist() == [0.5, 1.0, 0.0]
        assert poses[0, 3:].tolist() == [0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]
        # m = 1: the goal node is the root
        one = ref.routes(R.pose7(0.5, 1.0), [[0.6, 1.0, 0.0]], leg=R.TREE)
        assert one["node"].tolist() == [0]
        f1 = ref.refine(one["node_offset"], one["node"])
        assert f1["refined_node"].tolist() == [0] and f1["complete"].tolist() == [1] and f1["walks"] == 0
    finally:
        ref.close()
