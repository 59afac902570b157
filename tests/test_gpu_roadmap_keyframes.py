"""The roadmap's key-frame anchors on the GPU: fs_roadmap_set_keyframes and fs_roadmap_optimize against the CPU
restatement (tests/roadmap_kf_ref/) bit for bit — anchors (ids and float bits, in keyframe_mapping_'s order), the optimised node list,
and the rebuilt CSR against tests/roadmap_ref —, fs_roadmap_plan on the optimised roadmap against roadmap_ref's tree leg, both
de-duplication schedules, a long de-duplication chain, a run of more than 50 k anchors, the refusals and the FS_E_RANGE state."""
import importlib

import numpy as np
import pytest

import roadmap_kf_ref as K
import roadmap_ref as R

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05
CELLS = np.ascontiguousarray(fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])
ORIGIN = (-CELLS.shape[1] * RES / 2, -CELLS.shape[0] * RES / 2, 0.0)
BOUNDS = (ORIGIN[0] + 1.5, -ORIGIN[0] - 1.5, ORIGIN[1] + 1.5, -ORIGIN[1] - 1.5)


def _pair(cell=1.0, radius=6.1, min_frontier=0.25, min_robot=0.25):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(CELLS[None], ORIGIN, RES)
    sc.set_roadmap_params(cell, radius, min_frontier, min_robot)
    return sc, K.KfRoadmap(cell, min_frontier, min_robot)


def _add(sc, ref, xy, robot=False):
    rc = ref.add_nodes(xy, robot)
    try:
        sc.roadmap_add_nodes(xy, robot)
        assert rc == 0
    except fsmod.FsError as e:
        assert e.code == fsmod.capi.FS_E_RANGE and rc == K.FS_E_RANGE


def _same_anchors(sc, ref, what):
    got, want = sc.roadmap_anchors(), ref.anchors()
    assert got["n_pending"] == want["n_pending"], what
    assert got["kf_id"].tobytes() == want["kf_id"].tobytes(), what
    assert got["point_c"].tobytes() == want["point_c"].tobytes(), what


def _optimise_both(sc, ref):
    rc = ref.optimize()
    try:
        sc.roadmap_optimize()
        assert rc == 0
    except fsmod.FsError as e:
        assert e.code == fsmod.capi.FS_E_RANGE and rc == K.FS_E_RANGE
    return rc


def _same_graph(sc, ref_nodes, params, what):
    got = sc.roadmap_graph()
    assert got["xy"].tobytes() == ref_nodes.tobytes(), what
    rr = K.graph_of(ref_nodes, CELLS, ORIGIN, RES, *params)
    want = rr.graph()
    for k in ("xy", "key", "row_ptr", "col"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    return rr


def _run(sc, ref, seed, n_ticks=60, every=4):
    """A robot walk: frontier and robot-pose nodes per tick, a map message every few ticks (all key frames so far), then a
    loop-closure correction that bends the second half of the trajectory."""
    poses, fronts = K.trajectory(seed, n_ticks, bounds=BOUNDS)
    rng = np.random.default_rng(seed + 1)
    for t in range(n_ticks):
        _add(sc, ref, fronts[t])
        _add(sc, ref, poses[t, :2][None], robot=True)
        if t % every == every - 1 or t == n_ticks - 1:
            ids = np.arange(t + 1, dtype=np.int32)
            if rng.uniform() < 0.3:
                ids = ids[rng.permutation(ids.size)]
            got = sc.roadmap_set_keyframes(ids, poses[ids])
            assert got == ref.set_keyframes(ids, poses[ids]), (seed, t)
            _same_anchors(sc, ref, (seed, t))
    half = n_ticks // 2
    fixed = poses.copy()
    fixed[half:] = K.correct(poses[half:], 0.35, -0.2, 0.08, about=tuple(poses[half, :2]))
    ids = np.arange(n_ticks, dtype=np.int32)
    assert sc.roadmap_set_keyframes(ids, fixed) == ref.set_keyframes(ids, fixed)
    return _optimise_both(sc, ref)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("cell", [1.0, 0.3, 2.5])
def test_seeded_runs_equal_restatement(seed, cell):
    params = (cell, 6.1, 0.25, 0.25)
    sc, ref = _pair(*params)
    try:
        rc = _run(sc, ref, seed * 100 + int(cell * 10))
        _same_anchors(sc, ref, "after optimise")
        if rc == 0:
            _same_graph(sc, ref.nodes(), params, (seed, cell))
        assert sc.get_counter(1016) == ref.anchors()["kf_id"].size
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("seed", [5, 6])
def test_plan_on_the_optimised_roadmap_equals_tree_leg(seed):
    params = (1.0, 6.1, 0.25, 0.25)
    sc, ref = _pair(*params)
    try:
        assert _run(sc, ref, seed, n_ticks=80) == 0
        rr = _same_graph(sc, ref.nodes(), params, seed)
        rng = np.random.default_rng(seed)
        goals = np.stack([rng.uniform(BOUNDS[0], BOUNDS[1], 40), rng.uniform(BOUNDS[2], BOUNDS[3], 40), np.zeros(40)], axis=1)
        robot = R.pose7(*ref.nodes()[0])
        got = sc.roadmap_plan(robot, goals)
        want = rr.plan(robot, goals, leg=R.TREE)
        for k in ("path_length", "path_length_m", "path_heading", "achievable"):
            assert got[k].tobytes() == want[k].tobytes(), k
        assert want["achievable"].any()
    finally:
        sc.close(); ref.close()


def test_both_dedup_schedules_agree():
    params = (1.0, 6.1, 0.25, 0.25)
    graphs, rounds = [], []
    for one_wg in (None, 0):
        sc, ref = _pair(*params)
        try:
            if one_wg is not None:
                sc.set_option("roadmap.dedup_one_wg", one_wg)      # every round a launch of its own
            assert _run(sc, ref, 77) == 0
            _same_graph(sc, ref.nodes(), params, one_wg)
            graphs.append(sc.roadmap_graph())
            rounds.append(sc.get_counter(1017))
        finally:
            sc.close(); ref.close()
    for k in graphs[0]:
        assert graphs[0][k].tobytes() == graphs[1][k].tobytes(), k
    assert rounds[0] == rounds[1] > 1


def _serpentine(m, row=100, step=0.2, gap=1.0, x0=0.0, y0=0.0):
    """m points `step` apart along a serpentine: rows of `row` points joined by vertical runs; only neighbours in the sequence
    are closer than 0.25"""
    pts, x, y, d = [], x0, y0, 1
    while len(pts) < m:
        for _ in range(row):
            pts.append((x, y)); x += d * step
        x -= d * step
        for _ in range(int(round(gap / step)) - 1):
            y += step; pts.append((x, y))
        y += step; d = -d
    return np.array(pts[:m])


@pytest.mark.parametrize("n,one_wg", [(17000, None), (3000, None), (3000, 0)])
def test_long_dedup_chain(n, one_wg):
    """n key frames, one node each; the correction puts the node of the key frame of rank r in keyframe_mapping_'s order on
    point r of a chain 0.2 m apart, so the greedy verdicts alternate along the whole sequence: ~n rounds.  17 000 is past the
    one-workgroup threshold (a round per launch); 3000 runs in one workgroup, or in batched launches with the knob at 0."""
    params = (1.0, 0.3, 0.25, 0.01)
    sc, ref = _pair(*params)
    try:
        if one_wg is not None:
            sc.set_option("roadmap.dedup_one_wg", one_wg)
        side = int(np.ceil(np.sqrt(n)))
        kx, ky = np.meshgrid(np.arange(side), np.arange(side))
        kf = np.stack([kx.ravel()[:n] + 0.5, ky.ravel()[:n] + 0.5], axis=1)
        poses = np.array([K.pose(x, y) for x, y in kf])
        _add(sc, ref, kf + 0.1, robot=True)
        ids = np.arange(n, dtype=np.int32)
        assert sc.roadmap_set_keyframes(ids, poses) == ref.set_keyframes(ids, poses) == (n, 0)
        order = ref.anchors()["kf_id"]
        chain = _serpentine(n)
        fixed = poses.copy()
        fixed[order, 0] = chain[:, 0] - 0.1
        fixed[order, 1] = chain[:, 1] - 0.1
        assert sc.roadmap_set_keyframes(ids, fixed) == ref.set_keyframes(ids, fixed) == (0, 0)
        assert _optimise_both(sc, ref) == 0
        nodes = ref.nodes()
        assert abs(nodes.shape[0] - n // 2) < 200
        assert sc.roadmap_graph()["xy"].tobytes() == nodes.tobytes()
        assert sc.get_counter(1017) > n // 2 and sc.get_counter(1018) == n
    finally:
        sc.close(); ref.close()


def test_fifty_thousand_anchors():
    """10 000 cells with a node and six key-frame entries each (one id named twice): about 60 000 anchors, a rigid correction."""
    side = 100
    params = (1.0, 0.6, 0.25, 0.25)
    sc, ref = _pair(*params)
    try:
        gx, gy = np.meshgrid(np.arange(side), np.arange(side))
        nodes = np.stack([ORIGIN[0] + gx.ravel() + 0.5, ORIGIN[1] + gy.ravel() + 0.5], axis=1)
        _add(sc, ref, nodes)
        rng = np.random.default_rng(9)
        ids, poses = [], []
        for k in range(side * side):
            x, y = nodes[k]
            for j in range(6):
                ids.append(6 * k + j if j < 5 else 6 * k)
                poses.append(K.pose(x + rng.uniform(-0.45, 0.45), y + rng.uniform(-0.45, 0.45), rng.uniform(-3, 3), scale=rng.uniform(0.9, 1.1)))
        ids = np.array(ids, np.int32); poses = np.array(poses)
        assert sc.roadmap_set_keyframes(ids, poses) == ref.set_keyframes(ids, poses)
        _same_anchors(sc, ref, "anchored")
        assert sc.get_counter(1016) >= 50000
        fixed = K.correct(poses, 0.12, 0.05, 0.01)
        assert sc.roadmap_set_keyframes(ids, fixed) == ref.set_keyframes(ids, fixed)
        assert _optimise_both(sc, ref) == 0
        _same_graph(sc, ref.nodes(), params, "50k")
    finally:
        sc.close(); ref.close()


def test_refusals_range_state_and_reset():
    E = fsmod.capi
    sc, ref = _pair(1.0, 6.1, 0.1, 0.1)
    try:
        a = [(x, y) for x in (0.1, 0.3, 0.5, 0.7, 0.9) for y in (0.1, 0.4, 0.7)]
        b = [(x, y) for x in (1.1, 1.3, 1.5, 1.7, 1.9) for y in (0.25, 0.55)]
        _add(sc, ref, np.array(a + b))
        pa, pb = K.pose(0.5, 0.5), K.pose(1.5, 0.5)
        assert sc.roadmap_set_keyframes([1, 2], [pa, pb]) == ref.set_keyframes([1, 2], [pa, pb]) == (25, 0)
        before = sc.roadmap_anchors()
        # refusals change nothing
        for bad in ([np.nan, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0.5, 0.5, 0.0, 0.0]):      # the second: a zero row in R
            with pytest.raises(fsmod.FsError) as e:
                sc.roadmap_set_keyframes([1, 2], [pa, bad])
            assert e.value.code == E.FS_E_INVALID
        after = sc.roadmap_anchors()
        assert after["kf_id"].tobytes() == before["kf_id"].tobytes() and after["n_pending"] == 0
        # optimise: node list up to the 21st node of the cell, no key, no edge
        assert sc.roadmap_set_keyframes([1, 2], [pa, K.pose(0.5, 0.5)]) == ref.set_keyframes([1, 2], [pa, K.pose(0.5, 0.5)])
        assert _optimise_both(sc, ref) == K.FS_E_RANGE
        g = sc.roadmap_graph()
        assert g["xy"].shape[0] == 21 and g["xy"].tobytes() == ref.nodes().tobytes()
        assert not g["key"].any() and g["col"].size == 0
        # a 3-D grid
        sc.upload_grid(np.zeros((2, 16, 16), np.uint8), ORIGIN, RES)
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_optimize()
        assert e.value.code == E.FS_E_INVALID
        # a new parameter set clears the queue, the key frames and the anchors
        sc.roadmap_add_nodes([(3.3, 3.3)])
        assert sc.roadmap_anchors()["n_pending"] == 1
        sc.set_roadmap_params(1.0, 6.1, 0.1, 0.1)
        an = sc.roadmap_anchors()
        assert an["n_pending"] == 0 and an["kf_id"].size == 0 and sc.get_counter(1016) == 0
        sc.upload_grid(CELLS[None], ORIGIN, RES)
        sc.roadmap_optimize()
        assert sc.roadmap_graph()["xy"].shape[0] == 0
    finally:
        sc.close(); ref.close()
