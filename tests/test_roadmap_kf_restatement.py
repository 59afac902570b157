"""The CPU restatement of the roadmap's key-frame anchors (tests/roadmap_kf_ref/) on hand-built cases: mapDataCallback's
parents (own cell in message order, the square search's first cell in scan order, the radius truncation, orphans), optimizeSHM's
walk of keyframe_mapping_ in libstdc++'s iteration order, and populateNodes' de-duplication and 20-per-cell throw.  No GPU."""
import numpy as np
import pytest

import roadmap_kf_ref as K

f32 = np.float32


def ident(x, y):
    return K.pose(x, y)


def _pc(node, kf):
    """T^-1 * p for an identity rotation: float(p) - float(t), in float32"""
    return np.array([f32(node[0]) - f32(kf[0]), f32(node[1]) - f32(kf[1]), f32(0.0)], dtype=np.float32)


@pytest.fixture
def rm():
    r = K.KfRoadmap(1.0, 0.25, 0.25)
    yield r
    r.close()


def test_own_cell_parents_in_message_order_with_duplicates(rm):
    node = (0.5, 0.5)
    assert rm.add_nodes([node]) == 0
    ids = [7, 3, 7, 9]
    poses = [ident(0.1, 0.1), ident(0.2, 0.8), ident(0.3, 0.2), ident(5.5, 5.5)]
    assert rm.set_keyframes(ids, poses) == (1, 0)
    a = rm.anchors()
    assert a["n_pending"] == 0
    # keyframe_mapping_ got 7, 3 in that order; two keys in distinct buckets iterate newest first
    assert a["kf_id"].tolist() == [3, 7, 7]
    want7 = _pc(node, (0.3, 0.2))                      # an id named twice keeps its LAST pose, for both of its entries
    np.testing.assert_array_equal(a["point_c"][0], _pc(node, (0.2, 0.8)))
    np.testing.assert_array_equal(a["point_c"][1], want7)
    np.testing.assert_array_equal(a["point_c"][2], want7)


def test_square_search_takes_the_first_cell_in_scan_order(rm):
    rm.add_nodes([(0.5, 0.5)])
    # cell (1, 0) is nearer, but dx = -1 is scanned before dx = +1
    assert rm.set_keyframes([1, 2], [ident(1.05, 0.5), ident(-0.05, 1.95)]) == (1, 0)
    assert rm.anchors()["kf_id"].tolist() == [2]


@pytest.mark.parametrize("cell,offset,found", [
    (0.3, 1, True),      # radius (int)(0.3 m): 0, 0, 0 (the own cell again), then 1
    (0.3, 7, True), (0.3, 8, False),
    (2.5, 2, True), (2.5, 7, True),   # radii 2, 5, 7, then 10 > 7 stops
    (2.5, 8, False),
])
def test_search_radius_truncation(cell, offset, found):
    r = K.KfRoadmap(cell, 0.05, 0.05)
    try:
        x = 0.5 * cell
        r.add_nodes([(x, x)])
        kx = x + offset * cell
        assert r.set_keyframes([4], [ident(kx, x)]) == ((1, 0) if found else (0, 1))
        assert r.anchors()["kf_id"].size == (1 if found else 0)
    finally:
        r.close()


def test_orphan_is_gone_after_optimise(rm):
    rm.add_nodes([(0.5, 0.5), (20.5, 0.5)])
    assert rm.set_keyframes([1], [ident(0.4, 0.4)]) == (1, 1)
    assert rm.optimize() == 0
    nodes = rm.nodes()
    assert nodes.shape == (1, 2) and abs(nodes[0, 0] - 0.5) < 1e-6


def test_empty_message_orphans_every_pending_node(rm):
    rm.add_nodes([(0.5, 0.5), (2.5, 0.5)])
    assert rm.set_keyframes([], np.zeros((0, 7))) == (0, 2)
    assert rm.anchors()["n_pending"] == 0 and rm.anchors()["kf_id"].size == 0
    assert rm.optimize() == 0 and rm.nodes().shape[0] == 0


def test_absent_id_is_skipped_then_returns(rm):
    rm.add_nodes([(0.5, 0.5), (3.5, 0.5)])
    msg = ([1, 2], [ident(0.4, 0.4), ident(3.4, 0.4)])
    assert rm.set_keyframes(*msg) == (2, 0)
    assert rm.set_keyframes([1], [ident(0.4, 0.4)]) == (0, 0)
    assert rm.optimize() == 0
    assert rm.nodes().shape[0] == 1
    assert rm.anchors()["kf_id"].size == 2              # the absent id's anchor is kept
    rm.set_keyframes(*msg)
    assert rm.optimize() == 0 and rm.nodes().shape[0] == 2


def test_unchanged_poses_keep_the_nodes(rm):
    poses, fronts = K.trajectory(11, 20)
    for t, f in enumerate(fronts):
        rm.add_nodes(f)
        rm.add_nodes(poses[t, :2][None], is_robot_pose=True)
    before = rm.nodes()
    rm.set_keyframes(np.arange(len(poses)), poses)
    assert rm.optimize() == 0
    after = rm.nodes()
    assert after.shape == before.shape
    assert np.abs(np.sort(after, axis=0) - np.sort(before, axis=0)).max() < 1e-5


def test_rigid_correction_moves_the_nodes_rigidly(rm):
    poses, fronts = K.trajectory(12, 20)
    for f in fronts:
        rm.add_nodes(f)
    before = rm.nodes()
    rm.set_keyframes(np.arange(len(poses)), poses)
    dx, dy, th = 0.7, -0.4, 0.3
    rm.set_keyframes(np.arange(len(poses)), K.correct(poses, dx, dy, th))
    assert rm.optimize() == 0
    after = rm.nodes()
    c, s = np.cos(th), np.sin(th)
    moved = np.stack([c * before[:, 0] - s * before[:, 1] + dx, s * before[:, 0] + c * before[:, 1] + dy], axis=1)
    # each moved node has a match within 1e-5 m, and the counts agree
    assert after.shape == moved.shape
    d = np.sqrt(((after[:, None, :] - moved[None, :, :]) ** 2).sum(-1)).min(axis=1)
    assert d.max() < 1e-5


def test_two_parent_node_splits(rm):
    rm.add_nodes([(0.5, 0.5)])
    rm.set_keyframes([1, 2], [ident(0.2, 0.2), ident(0.8, 0.8)])
    rm.set_keyframes([1, 2], [ident(0.2, 0.2), ident(1.8, 0.8)])       # key frame 2 moved 1 m
    assert rm.optimize() == 0
    nodes = rm.nodes()
    assert nodes.shape[0] == 2
    assert sorted(np.round(nodes[:, 0], 4).tolist()) == [0.5, 1.5]


def test_iteration_order_decides_which_conflicting_point_survives(rm):
    """keyframe_mapping_ gets 1, 14, 3 (push order).  With libstdc++'s 13 buckets 14 joins 1's bucket in front of it and 3 opens
    a bucket of its own at the front: iteration 3, 14, 1 — neither id order nor insertion order.  Node B (key frame 3) is corrected
    onto node A (key frames 1 and 14): B is first in the sequence and survives, A is dropped."""
    A, B = (0.2, 0.2), (3.2, 0.2)
    rm.add_nodes([A, B])
    p1, p14, p3 = ident(0.5, 0.5), ident(0.5, 0.6), ident(3.5, 0.5)
    assert rm.set_keyframes([1, 14, 3], [p1, p14, p3]) == (2, 0)
    assert rm.anchors()["kf_id"].tolist() == [3, 14, 1]
    assert rm.set_keyframes([1, 14, 3], [p1, p14, ident(0.5, 0.55)]) == (0, 0)
    assert rm.optimize() == 0
    nodes = rm.nodes()
    assert nodes.shape[0] == 1
    assert abs(nodes[0, 0] - 0.2) < 1e-6 and abs(nodes[0, 1] - 0.25) < 1e-6      # B's corrected position, not A


def test_twenty_first_node_in_a_cell_throws():
    r = K.KfRoadmap(1.0, 0.1, 0.1)
    try:
        a = [(x, y) for x in (0.1, 0.3, 0.5, 0.7, 0.9) for y in (0.1, 0.4, 0.7)]           # 15 in cell (0, 0)
        b = [(x, y) for x in (1.1, 1.3, 1.5, 1.7, 1.9) for y in (0.25, 0.55)]              # 10 in cell (1, 0)
        assert r.add_nodes(a + b) == 0
        pa, pb = ident(0.5, 0.5), ident(1.5, 0.5)
        assert r.set_keyframes([1, 2], [pa, pb]) == (25, 0)
        assert r.set_keyframes([1, 2], [pa, ident(0.5, 0.5)]) == (0, 0)       # cell (1, 0)'s nodes shifted into cell (0, 0)
        assert r.optimize() == K.FS_E_RANGE
        assert r.nodes().shape[0] == 21
        # adding: the node that trips the throw is kept and queued
        r2 = K.KfRoadmap(1.0, 0.1, 0.1)
        assert r2.add_nodes(a + [(x - 1.0, y) for x, y in b]) == K.FS_E_RANGE
        assert r2.nodes().shape[0] == 21 and r2.anchors()["n_pending"] == 21
        r2.close()
    finally:
        r.close()
