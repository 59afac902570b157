"""fs_roadmap_routes on the GPU: the plan against fs_roadmap_plan byte for byte under both roadmap searches; the
routes, their numbering and refinePath's lists against the CPU restatement (tests/roadmap_route_ref/roadmap_route_ref.cpp) exactly;
the leg poses against the node coordinates and host libm; every leg's value against the oracle within the project's 1e-4 relative
bar; the per-route columns against a recomputation from the call's own dump bit for bit and against the oracle's threshold
decision; the de-duplication against scoring every leg; the refusals; and the state the call leaves behind."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import roadmap_ref as R
import roadmap_route_maps as M
import roadmap_route_ref as RR
from test_gpu_roadmap_astar import _goals, _map

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
E = fsmod.capi
RES = M.RES
REL = 1e-4                       # info_ref against the oracle's fp64 sum
QUAT_ABS = 1e-12                 # device against host libm (atan2, sin, cos): test_gpu_pathinfo.py's bound
VIS = [(14.0, 1.0), (14.0, 4.0)]  # the build's cone and the request the reference itself makes (cone off)
N_LANDMARKS = 20_000
COLS = ("path_length", "path_length_m", "path_heading", "achievable")
SEARCHES = {"tree": R.TREE, "reference": R.REFERENCE_ASTAR}
NAMES = ("plan2_128", "plan5_256", "REF2D")


@functools.lru_cache(maxsize=None)
def _landmarks(name):
    """20 000 landmarks on obstacle cells, heights U(0, 2.5 m), as test_gpu_pathinfo.py's"""
    if name == "REF2D":
        return fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=N_LANDMARKS).landmarks
    cells, origin = _map(name)
    rng = np.random.Generator(np.random.PCG64(977))
    lm = fsmod.synth._landmarks(rng, cells[None], origin, RES, N_LANDMARKS)
    lm[:, 2] = rng.uniform(0.0, 2.5, size=lm.shape[0]).astype(np.float32)
    return lm


def _new_world(name, stage_fim=True):
    """(scorer, restatement, cells, origin) with _setup's roadmap of the map on both"""
    ref, cells, origin, pts = M.restated_roadmap(name)
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    sc.roadmap_add_nodes(pts)
    sc.roadmap_rebuild()
    if stage_fim:
        sc.upload_landmarks(_landmarks(name))
        sc.lookup_generate()
        sc.set_fim_params(*VIS[0])
    return sc, ref, cells, origin


@pytest.fixture(scope="module")
def worlds():
    """one staged context and one restatement per map, kept for the module (the tests leave grid, roadmap and options as found)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _new_world(name)
        return made[name]
    yield get
    for sc, ref, _, _ in made.values():
        sc.close(); ref.close()


def _csr(off, flat, q):
    return flat[off[q]:off[q + 1]]


def _same_routes(got, want, tag):
    assert got["route_of"].tobytes() == want["route_of"].tobytes(), tag
    assert got["goal_node"].tobytes() == want["goal_node"].tobytes(), tag
    assert got["node_offset"].tobytes() == want["node_offset"].tobytes(), tag
    assert got["node"].tobytes() == want["node"].tobytes(), tag


def _same_refined(got, want, tag):
    assert got["refined_offset"].tobytes() == want["refined_offset"].tobytes(), tag
    assert got["refined_node"].tobytes() == want["refined_node"].tobytes(), tag
    assert got["complete"].tobytes() == want["complete"].tobytes(), tag
    assert (got["n_legs"] == np.diff(want["refined_offset"]) - 1).all(), tag


def _columns_from_values(n_legs, values, threshold):
    """info_mean, info_min, first_unsafe as the header defines them, from a value dump: the fp64 sum of the positive values in leg
    order (a sequential loop: numpy's sum is pairwise) over the number of legs"""
    off = np.concatenate([[0], np.cumsum(n_legs)])
    n = n_legs.size
    mean, mn, unsafe = np.zeros(n), np.full(n, np.inf, dtype=np.float32), np.full(n, -1, dtype=np.int32)
    for f in range(n):
        v = values[off[f]:off[f + 1]]
        if v.size == 0:
            continue
        s = 0.0
        for x in v:
            if x > 0:
                s += float(x)
        mean[f] = s / v.size
        mn[f] = v.min()
        bad = np.nonzero(~(v.astype(np.float64) > threshold))[0]
        if bad.size:
            unsafe[f] = bad[0]
    return mean, mn, unsafe


def _oracle_values(oracle, table, landmarks, poses, vis):
    uniq, inverse = np.unique(poses, axis=0, return_inverse=True)
    want = oracle.pose_information(table, landmarks, uniq, vis[0], vis[1], n_threads=16)["info_f64"]
    return want[inverse.reshape(-1)]


def _within_bar(got, want):
    scale = np.maximum(np.abs(want), 1e-6)
    return float(np.max(np.abs(got.astype(np.float64) - want) / scale)) if want.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- 1. the routes

@pytest.mark.parametrize("n", [1, 50, 400])
@pytest.mark.parametrize("search", list(SEARCHES))
@pytest.mark.parametrize("name", NAMES)
def test_plan_and_routes_equal_the_restatement(worlds, name, search, n):
    sc, ref, cells, origin = worlds(name)
    pose = M.robot_pose(cells, origin)
    goals, ach = _goals(cells, origin, 31 + n, n, pose[:2])
    if n == 1:
        ach = None
    got = sc.roadmap_routes(pose, goals, achievable_in=ach, with_information=False, want_nodes=True, search=search)
    plan = sc.roadmap_plan(pose, goals, achievable_in=ach, search=search)
    tag = (name, search, n)
    for k in COLS:
        assert got[k].tobytes() == plan[k].tobytes(), (tag, k)
    want = ref.routes(pose, goals, achievable_in=ach, leg=SEARCHES[search])
    _same_routes(got, want, tag)
    assert sc.get_counter(1026) == want["goal_node"].size
    xy = ref.graph()["xy"]
    routed = got["route_of"] >= 0
    at_robot = (goals[:, 0] == pose[0]) & (goals[:, 1] == pose[1])
    assert (routed == ((got["achievable"] == 1) & ~at_robot)).all(), tag
    for i in np.nonzero(routed)[0]:
        nodes = _csr(got["node_offset"], got["node"], got["route_of"][i])
        assert np.float64(RR.summed_from_goal_end(xy, nodes)).tobytes() == got["path_length_m"][i].tobytes(), (tag, i)
    if n >= 50:
        assert routed.sum() > 5 and (got["achievable"] == 0).any() and (at_robot & (got["achievable"] == 1)).any()
    # refinePath on the same lists
    _same_refined(got, ref.refine(want["node_offset"], want["node"]), tag)
    # the lean call returns the same routes' columns
    lean = sc.roadmap_routes(pose, goals, achievable_in=ach, with_information=False, search=search)
    for k in COLS + ("route_of", "goal_node", "complete", "n_legs"):
        assert lean[k].tobytes() == got[k].tobytes(), (tag, k)


# ---------------------------------------------------------------------------------------------------------------- 2. four nodes

def test_four_node_graph_routes():
    """test_four_node_graph_reference_gives_the_direct_edge's graph: the REFERENCE route is [S, G], the tree's the 4-node detour"""
    origin = (-1.0, -1.0, 0.0)
    sc = fsmod.FrontierScorer(device=0)
    try:
        sc.upload_grid(np.zeros((1, 160, 160), dtype=np.uint8), origin, RES)
        sc.set_roadmap_params(radius_to_decide_edges=3.0)
        sc.roadmap_add_nodes([[0.0, 0.0], [2.0, 0.0], [0.5, 0.9], [1.5, 0.9]])
        sc.roadmap_rebuild()
        goal = [[2.0, 0.0, 0.0]]
        astar = sc.roadmap_routes(R.pose7(0.0, 0.0), goal, with_information=False, want_nodes=True, search="reference")
        tree = sc.roadmap_routes(R.pose7(0.0, 0.0), goal, with_information=False, want_nodes=True, search="tree")
        assert astar["node"].tolist() == [0, 1] and astar["path_length_m"][0] == 2.0
        assert tree["node"].tolist() == [0, 2, 3, 1]
        assert tree["path_length_m"][0] == pytest.approx(np.sqrt(0.25 + 0.81) * 2 + 1.0, abs=1e-12)
        for out in (astar, tree):
            assert out["route_of"].tolist() == [0] and out["goal_node"].tolist() == [1] and out["node_offset"].tolist() == [0, out["node"].size]
            # the free grid: the goal is visible from the start
            assert out["refined_node"].tolist() == [0, 1] and out["complete"].tolist() == [1] and out["n_legs"].tolist() == [1]
        raw = sc.roadmap_routes(R.pose7(0.0, 0.0), goal, refine=False, with_information=False, want_nodes=True, search="tree")
        assert raw["n_legs"].tolist() == [3] and "refined_node" not in raw and raw["complete"].tolist() == [1]
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------- 3. refinePath

def test_refinement_shortens_most_tree_routes_on_ref2d(worlds):
    sc, ref, cells, origin = worlds("REF2D")
    pose = M.robot_pose(cells, origin)
    xy = ref.graph()["xy"]
    goals = M.goals_at_nodes(xy)
    want = ref.routes(pose, goals, leg=R.TREE)
    wref = ref.refine(want["node_offset"], want["node"])
    raw, new = np.diff(want["node_offset"]), np.diff(wref["refined_offset"])
    assert raw.size >= 250 and (new < raw).sum() * 2 >= raw.size, "fixture: the restatement must shorten at least half of the routes"
    got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search="tree")
    _same_routes(got, want, "REF2D")
    _same_refined(got, wref, "REF2D")
    assert sc.get_counter(1027) >= wref["walks"] > 0          # (lanes behind a refusal have walked too)
    print(f"REF2D tree: {raw.size} routes, {(new < raw).sum()} shorter after refinePath, up to {int((raw - new).max())} nodes fewer; "
          f"isConnectable walks {wref['walks']} in sequence, {sc.get_counter(1027)} on the device")


def test_a_truncated_route_on_an_unchanged_grid(worlds):
    """plan5_256: an edge accepted when walked q -> p that refinePath, walking p -> q, refuses"""
    sc, ref, cells, origin = worlds("plan5_256")
    pose = M.robot_pose(cells, origin)
    xy = ref.graph()["xy"]
    goals = M.goals_at_nodes(xy)
    for search, leg in SEARCHES.items():
        want = ref.routes(pose, goals, leg=leg)
        wref = ref.refine(want["node_offset"], want["node"])
        assert (wref["complete"] == 0).any(), "fixture: the restatement must truncate a route here"
        got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search=search)
        _same_routes(got, want, search)
        _same_refined(got, wref, search)
        q = int(np.nonzero(got["complete"] == 0)[0][0])
        assert _csr(got["refined_offset"], got["refined_node"], q)[-1] != got["goal_node"][q]


def _line_world(spacing, min_d, unknown_from=None):
    """a line of 150 nodes along y = 1.6 m on a 1024 x 64 grid (free, or with a stretch of unknown cells across it)"""
    cells = np.zeros((64, 1024), dtype=np.uint8)
    if unknown_from is not None:
        cells[:, unknown_from:unknown_from + 40] = 255
    origin = (0.0, 0.0, 0.0)
    pts = np.stack([0.5 + spacing * np.arange(150), np.full(150, 1.6)], axis=1)
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    sc.set_roadmap_params(min_distance_between_two_frontier_nodes=min_d)
    ref = RR.RouteRoadmap(cells, origin, RES, min_frontier=min_d)
    assert ref.populate(pts) == 0
    sc.roadmap_add_nodes(pts)
    ref.rebuild(); sc.roadmap_rebuild()
    return sc, ref, pts


@pytest.mark.parametrize("spacing,min_d,unknown_from", [(0.3, 0.25, None), (0.12, 0.1, 150)])
def test_routes_longer_than_a_wave(spacing, min_d, unknown_from):
    """More than 64 raw nodes: the scan from a kept node takes more than one round of 64 lanes.  On the free grid every candidate
    passes (a walk is cut at max_length, not refused).  With nodes 0.12 m apart and 40 unknown cells across the line from 7.5 m on,
    the first refusal from the start comes after more than 64 acceptances: in the second round."""
    sc, ref, pts = _line_world(spacing, min_d, unknown_from)
    try:
        pose = R.pose7(*pts[0])
        goals = M.goals_at_nodes(pts[[149, 100, 70]])
        for search, leg in SEARCHES.items():
            want = ref.routes(pose, goals, leg=leg)
            wref = ref.refine(want["node_offset"], want["node"])
            raw = np.diff(want["node_offset"])
            if search == "tree":                      # (the A* takes the longest hops it can: a dozen nodes)
                assert raw.tolist() == [71, 101, 150], "fixture: routes of more than 64 nodes"
            if search == "tree" and unknown_from is not None:
                q = int(np.argmax(raw))
                P = _csr(want["node_offset"], want["node"], q).tolist()
                L = _csr(wref["refined_offset"], wref["refined_node"], q).tolist()
                pos = [P.index(v) for v in L]
                assert pos[1] - pos[0] > 64 and pos[1] != len(P) - 1, "fixture: a refusal behind more than 64 acceptances"
            got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search=search)
            _same_routes(got, want, (spacing, search))
            _same_refined(got, wref, (spacing, search))
            assert sc.get_counter(1027) >= wref["walks"]
    finally:
        sc.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a new wall

def test_a_wall_painted_after_the_build():
    """fs_update_grid_region paints a lethal block across the longest route: refinePath reads the grid staged now, the plan the
    roadmap's edges as they were built"""
    name = "REF2D"
    sc, ref, cells, origin = _new_world(name, stage_fim=False)
    try:
        pose = M.robot_pose(cells, origin)
        xy = ref.graph()["xy"]
        goals = M.goals_at_nodes(xy)
        for search, leg in SEARCHES.items():
            want = ref.routes(pose, goals, leg=leg)
            before = ref.refine(want["node_offset"], want["node"])
            plan = sc.roadmap_plan(pose, goals, search=search)
            q = int(np.argmax(np.diff(want["node_offset"])))
            P = _csr(want["node_offset"], want["node"], q)
            mid = 0.5 * (xy[P[len(P) // 2]] + xy[P[len(P) // 2 - 1]])
            cx, cy = int((mid[0] - origin[0]) / RES), int((mid[1] - origin[1]) / RES)
            x0, y0 = max(cx - 4, 0), max(cy - 4, 0)
            block = np.full((min(9, cells.shape[0] - y0), min(9, cells.shape[1] - x0)), 254, dtype=np.uint8)
            saved = cells[y0:y0 + block.shape[0], x0:x0 + block.shape[1]].copy()
            painted = cells.copy()
            painted[y0:y0 + block.shape[0], x0:x0 + block.shape[1]] = block
            sc.update_grid_region(x0, y0, 0, block)
            ref.cells = painted
            try:
                after = ref.refine(want["node_offset"], want["node"])
                assert (after["complete"] == 0).sum() > (before["complete"] == 0).sum(), "fixture: the block must truncate a route"
                got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search=search)
                _same_routes(got, want, search)
                _same_refined(got, after, search)
                for k in COLS:
                    assert got[k].tobytes() == plan[k].tobytes(), (search, k)
            finally:
                sc.update_grid_region(x0, y0, 0, saved)
                ref.cells = cells
            got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search=search)
            _same_refined(got, before, (search, "restored"))
    finally:
        sc.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 5. - 8., 10. the legs

@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("name,search,n", [("REF2D", "tree", 50), ("plan5_256", "reference", 400), ("plan2_128", "tree", 1)])
def test_leg_poses_values_and_columns(oracle, ref_table, worlds, name, search, n, refine):
    sc, ref, cells, origin = worlds(name)
    lm = _landmarks(name)
    pose = M.robot_pose(cells, origin)
    goals, ach = _goals(cells, origin, 57 + n, n, pose[:2])
    if n == 1:
        ach = None
    xy = ref.graph()["xy"]
    try:
        for vis in VIS:
            sc.set_fim_params(*vis)
            got = sc.roadmap_routes(pose, goals, achievable_in=ach, refine=refine, want_nodes=True, want_legs=True, search=search)
            tag = (name, search, n, refine, vis)
            off, flat = (got["refined_offset"], got["refined_node"]) if refine else (got["node_offset"], got["node"])
            assert (got["n_legs"] == np.diff(off) - 1).all()
            legs = int(got["n_legs"].sum())
            p7 = got["leg_pose7"]
            assert p7.shape == (legs, 7) and got["leg_info"].shape == (legs,)
            # 5. positions are the nodes', the quaternions host libm's
            frm = np.concatenate([_csr(off, flat, q)[:-1] for q in range(off.size - 1)]) if off.size > 1 else np.zeros(0, np.int64)
            assert p7[:, :2].tobytes() == np.ascontiguousarray(xy[frm]).tobytes(), tag
            assert (p7[:, 2] == 0.0).all() and (p7[:, 3:5] == 0.0).all()
            want_p7 = ref.leg_poses(off, flat)
            assert want_p7.shape == p7.shape
            if legs:
                assert np.max(np.abs(p7[:, 3:] - want_p7[:, 3:])) <= QUAT_ABS, tag
            # 6. the values: the oracle at the call's own dumped poses
            want = _oracle_values(oracle, ref_table, lm, p7, vis)
            err = _within_bar(got["leg_info"], want)
            print(f"{tag}: {off.size - 1} routes, {legs} legs, {sc.get_counter(1028)} distinct poses, max rel err {err:.3g}")
            assert err <= REL, (tag, err)
            assert 0 <= sc.get_counter(1028) <= legs
            # 7. the per-route columns: a pure function of the dumped values
            mean, mn, unsafe = _columns_from_values(got["n_legs"], got["leg_info"], 550.0)
            assert got["info_mean"].tobytes() == mean.tobytes(), tag
            assert got["info_min"].tobytes() == mn.tobytes(), tag
            assert got["first_unsafe"].tobytes() == unsafe.tobytes(), tag
            none = got["n_legs"] == 0
            assert (got["info_mean"][none] == 0.0).all() and np.isposinf(got["info_min"][none]).all() and (got["first_unsafe"][none] == -1).all()
            # 10. the dumped poses through fs_score_fim
            if legs:
                again = sc.score_fim(p7, info_only=True)["info_ref"]
                assert _within_bar(got["leg_info"], again.astype(np.float64)) <= REL, tag
            # the same call without the dumps
            lean = sc.roadmap_routes(pose, goals, achievable_in=ach, refine=refine, search=search)
            for k in ("n_legs", "complete", "goal_node", "route_of", "path_length_m"):
                assert lean[k].tobytes() == got[k].tobytes(), (tag, k)
            np.testing.assert_allclose(lean["info_mean"], got["info_mean"], rtol=5e-6, atol=1e-6)
        if n >= 50:
            assert legs > 20
    finally:
        sc.set_fim_params(*VIS[0])


@pytest.mark.parametrize("vis", VIS)
def test_first_unsafe_against_the_oracle(oracle, ref_table, worlds, vis):
    """The threshold sits in the widest gap of the central 40 % of the sorted oracle values (at least 1e-3 relative wide, ten
    times the bar, asserted): then first_unsafe is the oracle's decision on every route, none left out."""
    sc, ref, cells, origin = worlds("REF2D")
    lm = _landmarks("REF2D")
    pose = M.robot_pose(cells, origin)
    goals = M.goals_at_nodes(ref.graph()["xy"])
    sc.set_fim_params(*vis)
    try:
        for refine in (True, False):
            dump = sc.roadmap_routes(pose, goals, refine=refine, want_legs=True, search="tree")
            want = _oracle_values(oracle, ref_table, lm, dump["leg_pose7"], vis)
            assert want.size > 300
            v = np.sort(want)
            mid = v[int(0.3 * v.size):int(0.7 * v.size)]
            i = int(np.argmax(np.diff(mid)))
            threshold = 0.5 * (mid[i] + mid[i + 1])
            gap = (mid[i + 1] - mid[i]) / threshold
            print(f"REF2D refine={refine} vis {vis}: {want.size} legs, threshold {threshold:.6g}, gap {gap:.3g} relative")
            assert gap >= 1e-3, gap
            got = sc.roadmap_routes(pose, goals, refine=refine, fi_threshold=threshold, search="tree")
            _, _, unsafe = _columns_from_values(dump["n_legs"], want, threshold)
            assert got["first_unsafe"].tobytes() == unsafe.tobytes(), (refine, vis, np.nonzero(got["first_unsafe"] != unsafe)[0][:8])
            assert (unsafe >= 0).any() and (unsafe == -1).any()
    finally:
        sc.set_fim_params(*VIS[0])


# ---------------------------------------------------------------------------------------------------------------- 9. de-duplication

@pytest.mark.parametrize("search", list(SEARCHES))
def test_deduplication_changes_no_result(worlds, search):
    """"routes.dedup" 0 scores every leg, 1 one pose per distinct (from node, to node): identical integers and poses, values
    within the bar (bit-equality is recorded in DESIGN.md 4.16, not asserted).  Raw tree routes share their prefixes: at most
    n_nodes - 1 distinct legs, however many routes."""
    sc, ref, cells, origin = worlds("REF2D")
    pose = M.robot_pose(cells, origin)
    xy = ref.graph()["xy"]
    goals = M.goals_at_nodes(xy)
    out, poses = {}, {}
    try:
        for dedup in (1, 0):
            sc.set_option("routes.dedup", dedup)
            out[dedup] = sc.roadmap_routes(pose, goals, refine=False, want_nodes=True, want_legs=True, search=search)
            poses[dedup] = sc.get_counter(1028)
    finally:
        sc.set_option("routes.dedup", 1)
    for k in COLS + ("route_of", "goal_node", "complete", "n_legs", "first_unsafe", "node_offset", "node", "leg_pose7"):
        assert out[1][k].tobytes() == out[0][k].tobytes(), k
    assert _within_bar(out[1]["leg_info"], out[0]["leg_info"].astype(np.float64)) <= REL
    np.testing.assert_allclose(out[1]["info_mean"], out[0]["info_mean"], rtol=REL)
    np.testing.assert_allclose(out[1]["info_min"], out[0]["info_min"], rtol=REL, atol=1e-6)
    legs = int(out[1]["n_legs"].sum())
    same = out[1]["leg_info"].tobytes() == out[0]["leg_info"].tobytes()
    print(f"REF2D {search}: {legs} legs, poses scored with / without de-duplication {poses[1]} / {poses[0]}; values bit-equal: {same}")
    assert poses[0] == legs > 1000
    pairs = {(a, b) for q in range(out[1]["goal_node"].size) for a, b in zip(_csr(out[1]["node_offset"], out[1]["node"], q)[:-1].tolist(),
                                                                            _csr(out[1]["node_offset"], out[1]["node"], q)[1:].tolist())}
    assert poses[1] == len(pairs)
    if search == "tree":
        assert poses[1] <= xy.shape[0] - 1


# ---------------------------------------------------------------------------------------------------------------- 11. - 14.

def test_routes_only_on_a_context_without_landmarks_and_the_first_call():
    """with_information = 0 needs no landmarks and no table, and the call may be the first thing a fresh context does after the
    roadmap is built; with information, the first call of a fresh staged context scores its legs"""
    name = "plan5_256"
    bare, ref, cells, origin = _new_world(name, stage_fim=False)
    staged = _new_world(name)[0]
    try:
        pose = M.robot_pose(cells, origin)
        goals, ach = _goals(cells, origin, 5, 50, pose[:2])
        for search, leg in SEARCHES.items():
            want = ref.routes(pose, goals, achievable_in=ach, leg=leg)
            got = bare.roadmap_routes(pose, goals, achievable_in=ach, with_information=False, want_nodes=True, search=search)
            _same_routes(got, want, search)
            _same_refined(got, ref.refine(want["node_offset"], want["node"]), search)
            assert "info_mean" not in got
            with pytest.raises(fsmod.FsError) as e:
                bare.roadmap_routes(pose, goals, achievable_in=ach, search=search)
            assert e.value.code == E.FS_E_STATE
            full = staged.roadmap_routes(pose, goals, achievable_in=ach, want_nodes=True, want_legs=True, search=search)
            _same_routes(full, want, search)
            assert full["leg_info"].size == full["n_legs"].sum() > 10 and (full["leg_info"] > 0).any()
            mean, mn, unsafe = _columns_from_values(full["n_legs"], full["leg_info"], 550.0)
            assert full["info_mean"].tobytes() == mean.tobytes() and full["first_unsafe"].tobytes() == unsafe.tobytes()
    finally:
        bare.close(); staged.close(); ref.close()


def _raw_call(sc, pose, goals, max_routes, max_nodes, prm=None, groups=("raw", "refined", "legs"), info=True, drop=None):
    """the C entry point itself: (rc, n_routes, n_nodes_total, n_refined_total, arrays)"""
    n = goals.shape[0]
    p = (C.c_double * 7)(*[float(v) for v in pose])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rr, rn = max(max_routes, 1), max(max_nodes, 1)
    a = dict(pl=np.full(n, -7.0), plm=np.full(n, -7.0), ph=np.full(n, -7.0), ach=np.full(n, 7, np.uint8), route_of=np.full(n, -7, np.int32),
             goal_node=np.full(rr, -7, np.int32), complete=np.full(rr, 7, np.uint8), n_legs=np.full(rr, -7, np.int32),
             mean=np.full(rr, -7.0) if info else None, mn=np.full(rr, -7.0, np.float32) if info else None,
             unsafe=np.full(rr, -7, np.int32) if info else None,
             off=np.full(rr + 1, -7, np.int64) if "raw" in groups else None, node=np.full(rn, -7, np.int32) if "raw" in groups else None,
             roff=np.full(rr + 1, -7, np.int64) if "refined" in groups else None, rnode=np.full(rn, -7, np.int32) if "refined" in groups else None,
             p7=np.full((rn, 7), -7.0) if "legs" in groups else None, li=np.full(rn, -7.0, np.float32) if "legs" in groups else None)
    if drop:
        a[drop] = None
    nr, tot, rtot = C.c_int32(-7), C.c_int64(-7), C.c_int64(-7)
    rc = sc._L.fs_roadmap_routes(sc._h, C.byref(p), n, vp(goals), None, C.byref(prm) if prm is not None else None, vp(a["pl"]), vp(a["plm"]),
                                 vp(a["ph"]), vp(a["ach"]), vp(a["route_of"]), max_routes, C.byref(nr), vp(a["goal_node"]), vp(a["complete"]),
                                 vp(a["n_legs"]), vp(a["mean"]), vp(a["mn"]), vp(a["unsafe"]), max_nodes,
                                 C.byref(tot) if "raw" in groups else None, vp(a["off"]), vp(a["node"]),
                                 C.byref(rtot) if "refined" in groups else None, vp(a["roff"]), vp(a["rnode"]), vp(a["p7"]), vp(a["li"]))
    return rc, nr.value, tot.value, rtot.value, a


def test_edges_and_refusals(worlds):
    name = "plan2_128"
    sc, ref, cells, origin = worlds(name)
    pose = M.robot_pose(cells, origin)
    goals, _ = _goals(cells, origin, 3, 40, pose[:2])
    full = sc.roadmap_routes(pose, goals, want_nodes=True, want_legs=True)
    k, total = full["goal_node"].size, full["node"].size
    assert k > 3 and total > k
    # NULL parameters are the defaults; exact room is enough
    rc, nr, tot, rtot, a = _raw_call(sc, pose, goals, k, total)
    assert rc == E.FS_OK and (nr, tot, rtot) == (k, total, full["refined_node"].size)
    assert a["off"][:k + 1].tobytes() == full["node_offset"].tobytes() and a["node"][:total].tobytes() == full["node"].tobytes()
    assert a["roff"][:k + 1].tobytes() == full["refined_offset"].tobytes() and a["rnode"][:rtot].tobytes() == full["refined_node"].tobytes()
    assert a["n_legs"][:k].tobytes() == full["n_legs"].tobytes() and a["unsafe"][:k].tobytes() == full["first_unsafe"].tobytes()
    assert a["p7"][:full["leg_pose7"].shape[0]].tobytes() == full["leg_pose7"].tobytes()
    # too little room: FS_E_RANGE, the totals set, nothing else written
    for mr, mn in ((k - 1, total), (k, total - 1), (0, 0)):
        rc, nr, tot, rtot, a = _raw_call(sc, pose, goals, mr, mn)
        assert rc == E.FS_E_RANGE and nr == k and tot == total and rtot == total, (mr, mn)
        assert (a["pl"] == -7.0).all() and (a["ach"] == 7).all() and (a["route_of"] == -7).all() and (a["goal_node"] == -7).all()
        assert (a["off"] == -7).all() and (a["node"] == -7).all() and (a["li"] == -7.0).all() and (a["mean"] == -7.0).all()
    # without a dump max_nodes is not looked at
    rc, nr, _, _, a = _raw_call(sc, pose, goals, k, 0, groups=())
    assert rc == E.FS_OK and nr == k and a["n_legs"][:k].tobytes() == full["n_legs"].tobytes()
    # a dump group half given
    for drop in ("off", "node", "roff", "rnode", "p7", "li"):
        assert _raw_call(sc, pose, goals, k, total, drop=drop)[0] == E.FS_E_INVALID, drop
    # what the parameters switch off must not be asked for
    P = E.RouteParamsC
    assert _raw_call(sc, pose, goals, k, total, prm=P(0, 1, 550.0))[0] == E.FS_E_INVALID            # refined dump without refine
    assert _raw_call(sc, pose, goals, k, total, prm=P(1, 0, 550.0), groups=("raw", "refined"))[0] == E.FS_E_INVALID   # info columns
    assert _raw_call(sc, pose, goals, k, total, prm=P(1, 0, 550.0), groups=("legs",), info=False)[0] == E.FS_E_INVALID
    assert _raw_call(sc, pose, goals, k, total, prm=P(1, 0, 550.0), groups=("raw", "refined"), info=False)[0] == E.FS_OK
    assert _raw_call(sc, pose, goals, k, total, drop="mean")[0] == E.FS_E_INVALID
    assert _raw_call(sc, pose, goals, -1, total)[0] == E.FS_E_INVALID and _raw_call(sc, pose, goals, k, -1)[0] == E.FS_E_INVALID
    for thr in (float("inf"), float("nan")):
        with pytest.raises(fsmod.FsError) as e:
            sc.roadmap_routes(pose, goals, fi_threshold=thr)
        assert e.value.code == E.FS_E_INVALID
    with pytest.raises(ValueError):
        sc.roadmap_routes(pose, goals, achievable_in=[1, 1])
    with pytest.raises(fsmod.FsError) as e:
        sc.roadmap_routes(pose, goals, search="dijkstra")
    assert e.value.code == E.FS_E_INVALID
    # an empty list
    got = sc.roadmap_routes(pose, np.zeros((0, 3)), want_nodes=True, want_legs=True)
    assert got["goal_node"].size == 0 and got["node_offset"].tolist() == [0] and got["refined_offset"].tolist() == [0] and got["leg_pose7"].shape == (0, 7)
    # no frontier planned: no route
    got = sc.roadmap_routes(pose, goals, achievable_in=np.zeros(40, np.uint8), want_nodes=True, want_legs=True)
    assert got["goal_node"].size == 0 and (got["route_of"] == -1).all() and not got["achievable"].any() and got["node"].size == 0
    # what fs_roadmap_plan accepts and refinePath refuses: a 3-D grid; what fs_score_fim refuses: no table
    bare = fsmod.FrontierScorer(device=0)
    try:
        for search in SEARCHES:
            got = bare.roadmap_routes(pose, goals, refine=False, with_information=False, want_nodes=True, search=search)   # an empty roadmap
            assert got["goal_node"].size == 0 and got["achievable"].tolist() == bare.roadmap_plan(pose, goals, search=search)["achievable"].tolist()
        with pytest.raises(fsmod.FsError) as e:
            bare.roadmap_routes(pose, goals, with_information=False)                  # refinePath without a grid
        assert e.value.code == E.FS_E_STATE
        bare.upload_grid(np.zeros((2, 16, 16), dtype=np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError) as e:
            bare.roadmap_routes(pose, goals, with_information=False)                  # ... on a 3-D grid
        assert e.value.code == E.FS_E_INVALID
        bare.upload_grid(cells[None], origin, RES)
        bare.upload_landmarks(_landmarks(name))
        with pytest.raises(fsmod.FsError) as e:
            bare.roadmap_routes(pose, goals)                                          # no lookup table
        assert e.value.code == E.FS_E_STATE
    finally:
        bare.close()


def test_a_chain_pool_that_overflows_is_grown_and_the_call_retried():
    name = "plan5_256"
    sc, ref, cells, origin = _new_world(name, stage_fim=False)
    try:
        pose = M.robot_pose(cells, origin)
        goals = M.goals_at_nodes(ref.graph()["xy"])
        want = ref.routes(pose, goals, leg=R.REFERENCE_ASTAR)
        assert want["node"].size > 100
        sc.set_option("routes.pool_nodes", 16)
        got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search="reference")
        _same_routes(got, want, "grown pool")
        assert sc.get_counter(1029) == 1
        got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search="reference")
        _same_routes(got, want, "second call")
        assert sc.get_counter(1029, reset=True) == 1 and sc.get_counter(1029) == 0
        # the A*'s own record pool outgrown as well (the global route with a small LDS cap)
        sc.set_option("roadmap.astar_lds_entries", 24)
        got = sc.roadmap_routes(pose, goals, with_information=False, want_nodes=True, search="reference")
        _same_routes(got, want, "global route")
        assert sc.get_counter(1023) > 0
    finally:
        sc.close(); ref.close()


def test_the_call_leaves_the_planner_as_it_found_it():
    """fs_roadmap_plan, the tree cache and the A* counters after the call are what they are after fs_roadmap_plan in its place"""
    name = "REF2D"
    a, ref, cells, origin = _new_world(name, stage_fim=False)
    b = _new_world(name, stage_fim=False)[0]
    try:
        pose = M.robot_pose(cells, origin)
        goals, ach = _goals(cells, origin, 8, 50, pose[:2])
        for search in SEARCHES:
            a.roadmap_routes(pose, goals, achievable_in=ach, with_information=False, search=search)
            b.roadmap_plan(pose, goals, achievable_in=ach, search=search)
            for which in (1005, 1006, 1021, 1022, 1023):
                assert a.get_counter(which) == b.get_counter(which), (search, which)
            pa, pb = a.roadmap_plan(pose, goals, achievable_in=ach, search=search), b.roadmap_plan(pose, goals, achievable_in=ach, search=search)
            for k in COLS:
                assert pa[k].tobytes() == pb[k].tobytes(), (search, k)
            for which in (1005, 1006, 1021, 1022, 1023):
                assert a.get_counter(which) == b.get_counter(which), (search, which, "after the plan")
        assert a.get_counter(1005) == 1 and a._roadmap_search == "tree"
    finally:
        a.close(); b.close(); ref.close()
