"""The next goal on the GPU (fs_roadmap_next_goal) against the CPU restatement (tests/tour_ref/tour_ref.cpp and
tests/tour_ref.py over tests/roadmap_ref): the batched trees and the pair matrix bit for bit, every output for k = 1..10 locals,
the optimum for k = 11 and 12 against Held-Karp, the round-per-launch route against the one-workgroup route, the FI branch, the
refusals, and the single-tree cache of fs_roadmap_plan left alone."""
import importlib
import math
import zlib

import numpy as np
import pytest

import planner_ref as P
import roadmap_ref as R
import tour_ref as T

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05
RADIUS = 12.0
CHARGE = RADIUS * 100000


def _maps():
    """(name, cells [ny][nx], origin): REF2D's map, floor plans, a non-square map, the spiral corridor."""
    out = [("REF2D", fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])]
    rng = np.random.Generator(np.random.PCG64(6161))
    for n in (128, 256, 512):
        out.append((f"plan_{n}", fsmod.synth.make_grid(rng, n, 1)[0]))
    out.append(("non_square", fsmod.synth.make_grid(rng, 256, 1)[0][:170, :]))
    out.append(("spiral", P.spiral_map(512)[0]))
    return [(name, np.ascontiguousarray(c), (-c.shape[1] * RES / 2, -c.shape[0] * RES / 2, 0.0)) for name, c in out]


MAPS = _maps()
IDS = [m[0] for m in MAPS]


def _points(cells, origin, rng, k, res=RES):
    xs, ys = P.free_cells(cells, rng, k)
    return np.stack([origin[0] + (xs + rng.uniform(0, 1, k)) * res, origin[1] + (ys + rng.uniform(0, 1, k)) * res], axis=1)


def _setup(name, cells, origin):
    """the same roadmap on the device and in the restatement: nodes on free cells, rebuilt"""
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    ref = R.Roadmap(cells, origin, RES)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pts = _points(cells, origin, rng, int(min(1500, max(40, cells.size * RES * RES / 2))))
    assert ref.populate(pts) == 0
    sc.roadmap_add_nodes(pts)
    ref.rebuild(); sc.roadmap_rebuild()
    return sc, ref, pts


def _list(cells, origin, rng, k, robot_xy, n_global=4, res=RES):
    """k + 1 locals (the last one beyond n_local = k), n_global globals, two ineligible: path lengths chosen so that the selection
    has exactly k locals and the first global is the closest global"""
    n = k + 1 + n_global + 2
    goal = np.zeros((n, 3))
    goal[:, :2] = _points(cells, origin, rng, n, res)
    plm = np.concatenate([np.sort(rng.uniform(0.5, RADIUS, k + 1)), rng.uniform(RADIUS + 0.1, 60.0, n_global), [1.0, 2.0]])
    ach = np.ones(n, np.uint8)
    ach[-2] = 0
    bl = np.zeros(n, np.uint8)
    bl[-1] = 1
    if k >= 3:
        goal[1, :2] = robot_xy                                          # a local exactly at the robot: its pair length is 0
    perm = rng.permutation(n)
    return goal[perm], plm[perm], ach[perm], bl[perm]


def _same(got, want, what):
    for key in ("next_index", "status", "n_tied", "n_locals"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert got["tour"].tolist() == want["tour"].tolist(), what
    assert np.float64(got["tour_length"]).tobytes() == np.float64(want["tour_length"]).tobytes(), what
    assert got["selection"].tolist() == want["selection"].tolist(), what
    if want["pair_length_m"] is None:
        assert got["pair_length_m"] is None, what
    else:
        assert got["pair_length_m"].tobytes() == want["pair_length_m"].tobytes(), what


@pytest.mark.parametrize("name,cells,origin", MAPS, ids=IDS)
def test_outputs_equal_restatement_for_k_1_to_10(name, cells, origin):
    sc, ref, pts = _setup(name, cells, origin)
    try:
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 11)
        reached = 0
        for k in range(1, 11):
            robot = pts[rng.integers(pts.shape[0])] + rng.uniform(-0.3, 0.3, 2)
            goal, plm, ach, bl = _list(cells, origin, rng, k, robot)
            sc.get_counter(1010, reset=True)
            got = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, bl, n_local=k, local_radius=RADIUS, want_matrix=True,
                                       want_selection=True)
            want = T.next_goal(ref, robot, goal, plm, ach, bl, n_local=k, radius=RADIUS)
            _same(got, want, (name, k))
            assert got["n_locals"] == k
            assert sc.get_counter(1010) == math.factorial(k)
            assert sc.get_counter(1008) >= 1
            reached += int((got["pair_length_m"] < CHARGE).sum() > k + 2)
        assert reached > 0, name                                      # the lists were not all unreachable
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("name,cells,origin", [m for m in MAPS if m[0] in ("REF2D", "plan_256", "spiral")],
                         ids=["REF2D", "plan_256", "spiral"])
def test_batched_trees_reach_every_key_node_as_the_restatement(name, cells, origin):
    """Every key node of the roadmap as a local, the robot on a node: row 0 is the robot's tree read at every node, the other rows
    the locals' trees; all bit-equal to the pair lengths from rr_tree, and row 0 equal to fs_roadmap_plan's path_length_m."""
    sc, ref, pts = _setup(name, cells, origin)
    try:
        g = ref.graph()
        keys = np.flatnonzero(g["key"])
        robot = g["xy"][keys[0]]
        n_local = 8
        for c0 in range(0, keys.size, n_local + 1):
            sel = keys[c0:c0 + n_local + 1]
            if sel.size < 2:
                break
            goal = np.zeros((sel.size, 3))
            goal[:, :2] = g["xy"][sel]
            plm = np.arange(1.0, sel.size + 1.0)
            ach = np.ones(sel.size, np.uint8)
            got = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, n_local=n_local, want_matrix=True, want_selection=True)
            want = T.next_goal(ref, robot, goal, plm, ach, n_local=n_local)
            _same(got, want, (name, c0))
            plan = sc.roadmap_plan(R.pose7(*robot), goal)
            loc = np.flatnonzero((got["selection"] & 3) == 1)
            order = np.concatenate([loc[np.argsort(plm[loc], kind="stable")], np.flatnonzero(got["selection"] & 4)])
            row0 = got["pair_length_m"][0, 1:]
            ok = plan["achievable"][order].astype(bool)
            assert row0[ok].tobytes() == plan["path_length_m"][order][ok].tobytes(), (name, c0)
            assert (row0[~ok] == CHARGE).all(), (name, c0)
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("k", [11, 12])
def test_eleven_and_twelve_locals_reach_the_held_karp_optimum(k):
    name, cells, origin = MAPS[0]
    sc, ref, pts = _setup(name, cells, origin)
    try:
        rng = np.random.default_rng(400 + k)
        g = ref.graph()
        robot = pts[rng.integers(pts.shape[0])]
        # goals on nodes the robot's tree reaches (plus a jitter), so that a tour below the charge exists
        d = ref.tree(ref.closest(*robot))["d"]
        reach = np.flatnonzero(np.isfinite(d) & (g["key"] == 1))
        goal, plm, ach, bl = _list(cells, origin, rng, k, robot)
        on = (plm <= RADIUS) | (np.arange(plm.size) == np.flatnonzero(plm > RADIUS)[np.argmin(plm[plm > RADIUS])])
        goal[on, :2] = g["xy"][rng.choice(reach, int(on.sum()), replace=False)] + rng.uniform(-0.02, 0.02, (int(on.sum()), 2))
        sc.get_counter(1010, reset=True)
        got = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, bl, n_local=k, want_matrix=True, want_selection=True)
        assert sc.get_counter(1010) == math.factorial(k)
        M = got["pair_length_m"]
        loc = np.flatnonzero((got["selection"] & 3) == 1)
        loc = loc[np.argsort(plm[loc], kind="stable")].tolist()
        cg = int(np.flatnonzero(got["selection"] & 4)[0])
        assert M.tobytes() == T.pair_matrix(ref, np.concatenate([robot[None], goal[loc + [cg], :2]])).tobytes()
        assert len(loc) == k and got["n_tied"] >= 1
        hk = T.held_karp(M)
        assert abs(got["tour_length"] - hk) <= 1e-12 * abs(hk)
        assert hk < CHARGE
        t = got["tour"].tolist()
        assert len(t) == k + 1 and sorted(t[:k]) == sorted(loc) and t[k] == cg
        order = [loc.index(f) for f in t[:k]]
        L = T.tour_length(M, order)
        assert L == got["tour_length"]
        assert abs(L - hk) <= 1e-12 * abs(hk)
        assert got["next_index"] == t[0] and got["status"] == T.SAFE
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("name,cells,origin", [m for m in MAPS if m[0] in ("REF2D", "non_square")], ids=["REF2D", "non_square"])
def test_round_per_launch_route_equals_one_workgroup_route(name, cells, origin):
    sc, ref, pts = _setup(name, cells, origin)
    try:
        rng = np.random.default_rng(77)
        for k in (1, 5, 9):
            robot = pts[rng.integers(pts.shape[0])]
            goal, plm, ach, bl = _list(cells, origin, rng, k, robot)
            kw = dict(n_local=k, want_matrix=True, want_selection=True)
            sc.set_option("roadmap.tour_one_wg", 16384)
            a = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, bl, **kw)
            ra = sc.get_counter(1009)
            sc.set_option("roadmap.tour_one_wg", 0)
            b = sc.roadmap_next_goal(R.pose7(*robot), goal, plm, ach, bl, **kw)
            rb = sc.get_counter(1009)
            _same(b, a, (name, k))
            assert ra == rb and ra > 0
            _same(a, T.next_goal(ref, robot, goal, plm, ach, bl, n_local=k), (name, k, "restatement"))
    finally:
        sc.close(); ref.close()


def test_fisher_information_branch():
    w = fsmod.synth.make_workload("REF2D", n_cand=64, n_landmarks=20_000)
    cells = w.cells[0]
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(w.cells, w.origin, w.resolution)
        sc.upload_landmarks(w.landmarks)
        sc.lookup_generate()
        sc.set_fim_params(14.0, 1.0)
        rng = np.random.default_rng(9)
        pts = _points(cells, w.origin, rng, 200, w.resolution)
        sc.roadmap_add_nodes(pts)
        sc.roadmap_rebuild()
        robot = pts[0]
        fi_pose = R.pose7(*w.goals[0, :2], 0.3)
        info = float(sc.score_fim(fi_pose, info_only=True)["info_ref"][0])
        lo, hi = info - 1.0 - 1e-3 * abs(info), info + 1.0 + 1e-3 * abs(info)
        goal, plm, ach, bl = _list(cells, w.origin, rng, 4, robot, res=w.resolution)
        only_globals = plm + 2 * RADIUS
        for p in (plm, only_globals):
            plain = sc.roadmap_next_goal(R.pose7(*robot), goal, p, ach, bl, n_local=4)
            safe = sc.roadmap_next_goal(R.pose7(*robot), goal, p, ach, bl, n_local=4, fi_pose7=fi_pose, fi_threshold=lo)
            unsafe = sc.roadmap_next_goal(R.pose7(*robot), goal, p, ach, bl, n_local=4, fi_pose7=fi_pose, fi_threshold=hi)
            if plain["status"] == T.UNDETERMINED:                        # the zero frontier: the FI check is not reached
                assert safe["status"] == unsafe["status"] == T.UNDETERMINED
                continue
            assert plain["status"] == T.SAFE and safe["status"] == T.SAFE and unsafe["status"] == T.UNSAFE
            for o in (safe, unsafe):
                assert o["next_index"] == plain["next_index"] and o["tour"].tolist() == plain["tour"].tolist()
        assert sc.roadmap_next_goal(R.pose7(*robot), goal, only_globals, ach, bl, n_local=4)["n_locals"] == 0
    finally:
        sc.close()


def test_refusals():
    sc = fsmod.FrontierScorer(device=0)
    try:
        goal = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_next_goal(R.pose7(0.5, 0.5), goal, [1.0, 2.0], [1, 1])
        assert e.value.code == fsmod.capi.FS_E_STATE
        sc.roadmap_add_nodes([[0.0, 0.0], [1.0, 1.0]])
        for bad in (0, 13):
            with pytest.raises(fsmod.FsError) as e:
                sc.roadmap_next_goal(R.pose7(0.5, 0.5), goal, [1.0, 2.0], [1, 1], n_local=bad)
            assert e.value.code == fsmod.capi.FS_E_INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.set_option("roadmap.tour_one_wg", -1)
        assert e.value.code == fsmod.capi.FS_E_INVALID
        # a roadmap without key nodes: every pair is charged, the zero frontier
        out = sc.roadmap_next_goal(R.pose7(0.5, 0.5), goal, [1.0, 2.0], [1, 1], n_local=2)
        assert out["n_locals"] == 1 and out["status"] == T.UNDETERMINED and out["next_index"] == -1
        assert out["tour_length"] == 2 * CHARGE and out["n_tied"] == 1 and out["tour"].size == 0
        out = sc.roadmap_next_goal(R.pose7(0.5, 0.5), np.vstack([goal, [[3.0, 3.0, 0.0]]]), [1.0, 2.0, 3.0], [1, 1, 1], n_local=3)
        assert out["n_locals"] == 2 and out["status"] == T.UNDETERMINED and out["next_index"] == -1
        assert out["tour_length"] == 3 * CHARGE
    finally:
        sc.close()


def test_single_tree_cache_and_its_counters_are_left_alone():
    name, cells, origin = MAPS[0]
    sc, ref, pts = _setup(name, cells, origin)
    try:
        rng = np.random.default_rng(5)
        goal, plm, ach, bl = _list(cells, origin, rng, 6, pts[3])
        pose = R.pose7(*pts[3])
        sc.get_counter(1005, reset=True)
        first = sc.roadmap_plan(pose, goal)
        r1006 = sc.get_counter(1006)
        assert sc.get_counter(1005) == 1
        sc.roadmap_next_goal(R.pose7(*pts[7]), goal, plm, ach, bl, n_local=6)
        assert sc.get_counter(1005) == 1 and sc.get_counter(1006) == r1006
        again = sc.roadmap_plan(pose, goal)
        assert sc.get_counter(1005) == 1                                  # the cached tree was reused
        for k in first:
            assert again[k].tobytes() == first[k].tobytes(), k
    finally:
        sc.close(); ref.close()
