"""The CPU restatement of the frontier roadmap (tests/roadmap_ref/roadmap_ref.cpp) on hand-built known answers:
edges, walls, the unknown-cell limit, the per-cell node limit, a graph on which the reference's squared-heuristic A* returns a
path that is longer under its own edge cost than the tree's, and the tree as a true fixed point."""
import numpy as np
import pytest

import roadmap_ref as R

RES = 0.05
ORIGIN = (-1.0, -1.0, 0.0)


def _free(n=160):
    return np.zeros((n, n), dtype=np.uint8)


def _cell(v):
    return int((v - ORIGIN[0]) / RES)


def test_three_node_chain():
    r = R.Roadmap(_free(), ORIGIN, RES, radius=3.0)
    assert r.populate([[0.0, 0.0], [2.5, 0.0], [5.0, 0.0]]) == 0
    r.rebuild()
    g = r.graph()
    assert g["key"].tolist() == [1, 1, 1]
    assert g["row_ptr"].tolist() == [0, 1, 3, 4] and g["col"].tolist() == [1, 0, 2, 1]
    p = r.plan(R.pose7(0.0, 0.0), [[5.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.4, 0.1, 0.0]])
    assert p["achievable"].tolist() == [1, 1, 1]
    assert p["path_length_m"].tolist() == [5.0, 0.0, 2.5]
    assert np.array_equal(p["path_length"], p["path_length_m"])


def test_wall_blocks_the_edge():
    cells = _free()
    cells[:, _cell(1.0)] = 254
    r = R.Roadmap(cells, ORIGIN, RES, radius=3.0)
    r.populate([[0.0, 0.0], [2.0, 0.0]])
    r.rebuild()
    g = r.graph()
    assert g["col"].size == 0 and g["key"].tolist() == [1, 1]
    p = r.plan(R.pose7(0.0, 0.0), [[2.0, 0.0, 0.0]])
    assert p["achievable"][0] == 0 and p["path_length_m"][0] == R.DBL_MAX and p["path_heading"][0] == R.DBL_MAX
    # 253 is in the obstacle range of isConnectable's visitor too
    cells[:, _cell(1.0)] = 253
    r2 = R.Roadmap(cells, ORIGIN, RES, radius=3.0)
    r2.populate([[0.0, 0.0], [2.0, 0.0]])
    r2.rebuild()
    assert r2.graph()["col"].size == 0


@pytest.mark.parametrize("width,linked", [(30, True), (36, True), (37, False), (45, False)])
def test_unknown_cell_limit(width, linked):
    """isConnectable rejects a segment with more than radius / res * 0.3 = 36.6 unknown cells (radius 6.1, res 0.05)."""
    cells = _free()
    x0 = _cell(0.5)
    cells[:, x0:x0 + width] = 255
    r = R.Roadmap(cells, ORIGIN, RES)
    r.populate([[0.0, 0.02], [5.0, 0.02]])
    r.rebuild()
    assert (r.graph()["col"].size == 2) == linked


def test_twenty_first_node_in_a_cell_raises_range_error():
    r = R.Roadmap(_free(), ORIGIN, RES, min_frontier=0.0)
    pts = [[0.05 + 0.04 * i, 0.5] for i in range(21)] + [[0.9, 0.9]]
    assert r.populate(pts) == R.FS_E_RANGE
    g = r.graph()
    assert g["xy"].shape[0] == 21                       # the 21st stays added, the point after it is not
    # the minimum distance drops a point near an existing node, in a neighbouring cell too
    r2 = R.Roadmap(_free(), ORIGIN, RES)
    assert r2.populate([[0.95, 0.5], [1.1, 0.5], [1.3, 0.5]]) == 0
    assert r2.graph()["xy"].tolist() == [[0.95, 0.5], [1.3, 0.5]]


def test_squared_heuristic_astar_returns_a_g_longer_path():
    """S -> G directly (g = 4) against the detour S -> Q1 -> Q2 -> G (g = 1.06 + 1 + 1.06 = 3.12): A* pops G at f = 4 before the
    detour's nodes (f = 4.12, the squared heuristic overestimates), so it returns 2 m; the tree follows the g-shortest detour."""
    r = R.Roadmap(_free(), ORIGIN, RES, radius=3.0)
    r.populate([[0.0, 0.0], [2.0, 0.0], [0.5, 0.9], [1.5, 0.9]])
    r.rebuild()
    goal = [[2.0, 0.0, 0.0]]
    astar = r.plan(R.pose7(0.0, 0.0), goal, leg=R.REFERENCE_ASTAR)
    tree = r.plan(R.pose7(0.0, 0.0), goal, leg=R.TREE)
    assert astar["achievable"][0] == tree["achievable"][0] == 1
    assert astar["path_length_m"][0] == 2.0
    detour = np.sqrt(0.25 + 0.81) + 1.0 + np.sqrt(0.25 + 0.81)
    assert tree["path_length_m"][0] == pytest.approx(detour, abs=1e-12)
    t = r.tree(0)
    assert t["pred"].tolist() == [-1, 3, 0, 2] and t["hops"][1] == 3


def _random_roadmap(seed, n_nodes=120, n=200):
    rng = np.random.default_rng(seed)
    cells = _free(n)
    for _ in range(12):                                  # a few wall segments
        x, y = rng.integers(0, n, 2)
        if rng.random() < 0.5:
            cells[y, x:x + rng.integers(10, 60)] = 254
        else:
            cells[y:y + rng.integers(10, 60), x] = 254
    r = R.Roadmap(cells, ORIGIN, RES, radius=3.0)
    pts = rng.uniform(ORIGIN[0], ORIGIN[0] + n * RES, size=(n_nodes, 2))
    r.populate(pts)
    r.rebuild()
    return r, rng


@pytest.mark.parametrize("seed", range(4))
def test_tree_is_a_fixed_point(seed):
    r, _ = _random_roadmap(seed)
    g = r.graph()
    t = r.tree(0)
    assert t["rounds"] > 0
    d, hops, pred = t["d"], t["hops"], t["pred"]
    xy = g["xy"]
    for u in range(xy.shape[0]):
        if not np.isfinite(d[u]):
            continue
        for v in g["col"][g["row_ptr"][u]:g["row_ptr"][u + 1]]:
            w = (xy[u, 0] - xy[v, 0]) ** 2 + (xy[u, 1] - xy[v, 1]) ** 2
            cand = (d[u] + w, hops[u] + 1, u)
            assert v == 0 or (d[v], hops[v], pred[v]) <= cand, (u, v)
    for v in range(1, xy.shape[0]):
        if np.isfinite(d[v]):
            u = pred[v]
            w = (xy[u, 0] - xy[v, 0]) ** 2 + (xy[u, 1] - xy[v, 1]) ** 2
            assert d[v] == d[u] + w and hops[v] == hops[u] + 1
        else:
            assert pred[v] == -1


@pytest.mark.parametrize("seed", range(4))
def test_legs_agree_on_achievability(seed):
    r, rng = _random_roadmap(seed)
    goals = np.zeros((60, 3))
    goals[:, :2] = rng.uniform(ORIGIN[0], ORIGIN[0] + 10.0, size=(60, 2))
    pose = R.pose7(*r.graph()["xy"][0])
    a = r.plan(pose, goals, leg=R.REFERENCE_ASTAR)
    t = r.plan(pose, goals, leg=R.TREE)
    assert np.array_equal(a["achievable"], t["achievable"])
    ok = t["achievable"] == 1
    assert np.array_equal(a["path_heading"], t["path_heading"])
    assert np.all(t["path_length_m"][ok] >= 0)


def test_connect_links_both_ways_and_marks_keys():
    r = R.Roadmap(_free(), ORIGIN, RES, radius=3.0)
    r.populate([[0.0, 0.0], [2.0, 0.0], [4.0, 0.0], [6.0, 5.5]])
    r.connect([[0.1, 0.1]])                               # closest node 0; its neighbours within 3 m: node 1
    g = r.graph()
    assert g["key"].tolist() == [1, 1, 0, 0]
    assert g["row_ptr"].tolist() == [0, 1, 2, 2, 2] and g["col"].tolist() == [1, 0]
    r.connect([[2.1, 0.0], [0.0, 0.0]])                   # node 1: links 1 <-> 2 (1 <-> 0 exists); node 0: nothing new
    g = r.graph()
    assert g["key"].tolist() == [1, 1, 1, 0]
    assert g["row_ptr"].tolist() == [0, 1, 3, 4, 4] and g["col"].tolist() == [1, 0, 2, 1]
    # a plan from a robot nearest a non-key node starts at the closest KEY node
    p = r.plan(R.pose7(6.0, 5.0), [[4.0, 0.0, 0.0]])
    assert p["achievable"][0] == 1 and p["path_length_m"][0] == 0.0
