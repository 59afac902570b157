"""The leg refinement on the GPU (fs_refine_paths / fs_refine_field) against the CPU restatement's `field` leg
(tests/thetastar_ref/thetastar_ref.cpp) bit for bit — every field, status, cost, vertex and pose —, achievability against the
`reference` leg apart from the flagged loop quirk, batches against single calls and the field grouping, refine_tour on a
roadmap_next_goal result, the field cache and its invalidation, and the refusals."""
import importlib
import zlib

import numpy as np
import pytest

import planner_ref as P
import thetastar_ref as T

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = 0.05


def _inflate(cells):
    """a floor plan whose walls carry a cost gradient: 252 next to a wall down to 1 twelve cells away (free cells only)"""
    c = cells.copy()
    wall = c == 254
    dist = np.full(c.shape, 99)
    cur = wall.copy()
    for d in range(1, 13):
        grown = cur.copy()
        grown[1:, :] |= cur[:-1, :]; grown[:-1, :] |= cur[1:, :]
        grown[:, 1:] |= cur[:, :-1]; grown[:, :-1] |= cur[:, 1:]
        dist[grown & ~cur & (dist == 99)] = d
        cur = grown
    band = (dist <= 12) & (c < 253)
    c[band] = np.clip(252 - (dist[band] - 1) * 23, 1, 252).astype(np.uint8)
    return c


def _maps():
    out = [("REF2D", fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16).cells[0])]
    rng = np.random.Generator(np.random.PCG64(7373))
    for n in (128, 256, 512, 1024):
        out.append((f"plan_{n}", fsmod.synth.make_grid(rng, n, 1)[0]))
    out.append(("non_square", fsmod.synth.make_grid(rng, 256, 1)[0][:170, :]))
    out.append(("spiral", P.spiral_map(256)[0]))
    out.append(("inflated", _inflate(fsmod.synth.make_grid(rng, 192, 1)[0])))
    return [(name, np.ascontiguousarray(c), (-c.shape[1] * RES / 2, -c.shape[0] * RES / 2, 0.0)) for name, c in out]


MAPS = _maps()
IDS = [m[0] for m in MAPS]


def _scorer(cells, origin):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    return sc


def _points(cells, origin, rng, k, value=None):
    ok = (cells < 254) if value is None else (cells == value)
    ys, xs = np.nonzero(ok)
    i = rng.choice(xs.size, k)
    return np.stack([origin[0] + (xs[i] + rng.uniform(0, 1, k)) * RES, origin[1] + (ys[i] + rng.uniform(0, 1, k)) * RES], axis=1)


def _legs(cells, origin, seed, n):
    """n legs from distinct starts; a few goals on unknown cells, one off the map, one on a wall"""
    rng = np.random.default_rng(seed)
    s = _points(cells, origin, rng, n)
    g = _points(cells, origin, rng, n)
    if (cells == 255).any():
        g[2] = _points(cells, origin, rng, 1, 255)[0]
    if (cells == 254).any():
        g[3] = _points(cells, origin, rng, 1, 254)[0]
    g[4] = (origin[0] - 1.0, origin[1])
    return s, g


def _cell(origin, xy):
    return int((xy[0] - origin[0]) / RES), int((xy[1] - origin[1]) / RES)


def _same_leg(got, i, want, what):
    assert got["status"][i] == want["status"], (what, i, got["status"][i], want["status"])
    assert got["cost"][i] == want["cost"], (what, i, got["cost"][i], want["cost"])
    assert got["vertices"][i].tobytes() == want["vertices"].tobytes(), (what, i, got["vertices"][i], want["vertices"])
    assert got["poses"][i].tobytes() == want["poses"].tobytes(), (what, i, len(got["poses"][i]), len(want["poses"]))


@pytest.mark.parametrize("name,cells,origin", MAPS, ids=IDS)
def test_fields_equal_restatement(name, cells, origin):
    sc = _scorer(cells, origin)
    try:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        for k, s in enumerate(_points(cells, origin, rng, 2)):
            sx, sy = _cell(origin, s)
            for allow, corners in ((1, 8), (0, 8), (1, 4)) if k == 0 else ((1, 8),):
                got = sc.refine_field(s, allow_unknown=allow, corners=corners)
                want = T.field(cells, sx, sy, allow_unknown=allow, corners=corners)
                assert got.tobytes() == want.tobytes(), (name, sx, sy, allow, corners, int((got != want).sum()))
    finally:
        sc.close()


@pytest.mark.parametrize("name,cells,origin", MAPS, ids=IDS)
def test_legs_equal_field_leg_and_reference_achievability(name, cells, origin):
    sc = _scorer(cells, origin)
    try:
        s, g = _legs(cells, origin, zlib.crc32(name.encode()) + 1, 13)
        got = sc.refine_paths(s, g)
        quirks = 0
        for i in range(13):
            want = T.leg(cells, origin, RES, s[i], g[i])
            _same_leg(got, i, want, name)
            if cells.size <= 300 * 300:
                ref = T.leg(cells, origin, RES, s[i], g[i], which=T.REFERENCE)
                if (ref["status"] == T.OK) != (want["status"] == T.OK):
                    assert want["status"] == T.OK and ref["quirk"], (name, i)
                    quirks += 1
                else:
                    assert ref["status"] == want["status"]
        assert got["status"][4] == T.GOAL_OFF_MAP
        assert quirks <= 4
    finally:
        sc.close()


@pytest.mark.parametrize("name,cells,origin", [MAPS[0], MAPS[2], MAPS[6]], ids=[MAPS[0][0], MAPS[2][0], MAPS[6][0]])
def test_batch_equals_single_calls_and_field_groups(name, cells, origin):
    sc = _scorer(cells, origin)
    try:
        s, g = _legs(cells, origin, zlib.crc32(name.encode()) + 2, 13)
        s[7] = s[1]                                    # a shared start: one field for two legs
        batch = sc.refine_paths(s, g)
        singles = [sc.refine_paths(s[i:i + 1], g[i:i + 1]) for i in range(13)]
        for i in range(13):
            one = {k: singles[i][k][0] for k in ("status", "cost", "vertices", "poses")}
            _same_leg(batch, i, one, (name, "single"))
        for m in (1, 3):
            sc.set_option("refine.max_fields", m)
            grouped = sc.refine_paths(s, g)
            for i in range(13):
                one = {k: batch[k][i] for k in ("status", "cost", "vertices", "poses")}
                _same_leg(grouped, i, one, (name, "max_fields", m))
        sc.set_option("refine.max_fields", 16)
    finally:
        sc.close()


def test_refine_tour_on_a_next_goal_result():
    name, cells, origin = MAPS[0]
    sc = _scorer(cells, origin)
    try:
        rng = np.random.default_rng(31)
        nodes = _points(cells, origin, rng, 400)
        sc.roadmap_add_nodes(nodes)
        sc.roadmap_rebuild()
        robot = _points(cells, origin, rng, 1)[0]
        pose = np.array([robot[0], robot[1], 0.0, 0.0, 0.0, 0.0, 1.0])
        goal = np.zeros((20, 3))
        goal[:, :2] = _points(cells, origin, rng, 20)
        plan = sc.roadmap_plan(pose, goal)
        ng = sc.roadmap_next_goal(pose, goal, plan["path_length_m"], plan["achievable"], n_local=5)
        tour = ng["tour"]
        assert len(tour) >= 1
        out = sc.refine_tour(pose, goal, ng)
        pts = np.vstack([robot[None], goal[tour, :2]])
        assert len(out["status"]) == len(tour)
        path = []
        for i in range(len(tour)):
            want = T.leg(cells, origin, RES, pts[i], pts[i + 1])
            _same_leg(out, i, want, "tour")
            if want["status"] == T.OK:
                path.append(want["poses"])
        assert out["path"].tobytes() == (np.vstack(path) if path else np.zeros((0, 2))).tobytes()
    finally:
        sc.close()


def test_field_cache_hits_and_invalidation():
    name, cells, origin = MAPS[1]
    sc = _scorer(cells, origin)
    try:
        s, g = _legs(cells, origin, 5, 13)
        sc.get_counter(1011, reset=True)
        first = sc.refine_paths(s, g)
        built = sc.get_counter(1011)
        n_starts = len({_cell(origin, p) for i, p in enumerate(s) if i != 4})    # (leg 4's goal is off the map: no field)
        assert built == n_starts and sc.get_counter(1012) > 0 and sc.get_counter(1013) > 0
        again = sc.refine_paths(s, g)
        assert sc.get_counter(1011) == built                      # every field from the cache
        for i in range(13):
            _same_leg(again, i, {k: first[k][i] for k in ("status", "cost", "vertices", "poses")}, "cached")
        # a window update drops the fields: the next call rebuilds them on the new grid
        sx, sy = _cell(origin, s[0])
        x0, y0 = max(0, sx - 6), max(0, sy - 6)
        win = cells[y0:y0 + 12, x0:x0 + 12].copy()
        win[win < 254] = 120
        sc.update_grid_region(x0, y0, 0, win)
        new = cells.copy()
        new[y0:y0 + 12, x0:x0 + 12] = win
        after = sc.refine_paths(s, g)
        assert sc.get_counter(1011) == 2 * built
        for i in range(13):
            _same_leg(after, i, T.leg(new, origin, RES, s[i], g[i]), "after update")
        assert sc.refine_field(s[0]).tobytes() == T.field(new, sx, sy).tobytes()
    finally:
        sc.close()


def test_refusals():
    c = np.zeros((40, 40), np.uint8)
    c[20, :] = 254
    c[5, 5] = 255
    origin = (0.0, 0.0, 0.0)
    sc = fsmod.FrontierScorer(device=0)
    try:
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths([[0.1, 0.1]], [[0.5, 0.5]])
        assert e.value.code == fsmod.capi.FS_E_STATE
        sc.upload_grid(np.zeros((2, 8, 8), np.uint8), origin, RES)
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths([[0.1, 0.1]], [[0.2, 0.2]])
        assert e.value.code == fsmod.capi.FS_E_INVALID
        sc.upload_grid(c[None], origin, RES)
        for kw in (dict(corners=6), dict(w_euc=0.0), dict(w_euc=float("nan")), dict(w_traversal=-1.0)):
            with pytest.raises(fsmod.FsError) as e:
                sc.refine_paths([[0.1, 0.1]], [[0.5, 0.5]], **kw)
            assert e.value.code == fsmod.capi.FS_E_INVALID, kw
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_field([-1.0, 0.5])
        assert e.value.code == fsmod.capi.FS_E_INVALID
        C = lambda x, y: ((x + 0.5) * RES, (y + 0.5) * RES)
        starts = [(-1.0, 0.5), C(2, 2), C(2, 20), C(2, 2), C(2, 2), C(2, 2), C(5, 5), C(2, 2)]
        goals = [C(3, 3), (0.5, 9.0), C(3, 3), C(2, 20), C(2, 30), C(5, 5), C(8, 8), C(2, 2)]
        out = sc.refine_paths(starts, goals, allow_unknown=False)
        assert out["status"].tolist() == [1, 2, 3, 4, 5, 4, 3, 0]
        assert out["cost"][:7].tolist() == [T.DBL_MAX] * 7 and (out["n_poses"][:7] == 0).all()
        assert out["n_vertices"][7] == 1 and out["n_poses"][7] == 1
        assert sc.refine_paths(starts, goals, allow_unknown=True)["status"].tolist() == [1, 2, 3, 4, 5, 0, 0, 0]
        assert (sc.refine_field(C(2, 20)) == T.DBL_MAX).all()
        empty = sc.refine_paths(np.zeros((0, 2)), np.zeros((0, 2)))
        assert empty["status"].shape == (0,)
    finally:
        sc.close()
