"""The REFERENCE refine search on the GPU (fs_set_refine_search): every leg's status, cost, vertices and poses against
the CPU run of the same header (thetastar_search_ref) bit for bit and, at the reference's weights, status class, raw vertices and
poses against the reference's compiled Theta* (reference_built); slot counts and batching, duplicate legs, the loop quirk against
the FIELD search, the untouched FIELD path and its cache, search= on a call, refine_tour, the sizing call and the refusals.

The maps are the small known maps of thetastar_search_ref plus three generated ones — 64 x 48, 48 x 64, 96 x 96: the smallest at
which a heap a few hundred entries deep, walks longer than 64 cells (a second lane round of the ordered fold) and a non-square
stride all occur.  Every map carries a one-cell lethal border, so no walk reads a cell off the map (where the device keeps the
restatement's "unsafe" and the reference reads outside its array)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import reference_built as B
import thetastar_ref as T
import thetastar_search_ref as S
from test_reference_built import theta_legs

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
RES = S.RES
_CLASS = {S.OK: "found", S.START_OFF_MAP: "off", S.GOAL_OFF_MAP: "off", S.START_UNSAFE: "unsafe", S.GOAL_UNSAFE: "unsafe", S.NO_PATH: "none"}
_REF_CLASS = {B.FOUND: "found", B.START_OFF_MAP: "off", B.GOAL_OFF_MAP: "off", B.UNSAFE: "unsafe", B.NO_PATH: "none"}


def _known():
    out = []
    for name, make in (("corridor", S.corridor_map), ("strip253", S.strip253_map), ("unknown", S.unknown_map), ("walled", S.walled_map),
                       ("open", S.open_map)):
        cells, a, b = make()
        pts = [(a, b), (b, a), (a, a), (a, (a[0] + 1, a[1]))]
        if name == "unknown":
            pts += [(a, (12, 7)), ((12, 8), b)]
        s = np.array([S.centre(S.ORIGIN, *p[0]) for p in pts])
        g = np.array([S.centre(S.ORIGIN, *p[1]) for p in pts])
        allow = np.array([True] * len(pts) + [False] * len(pts))
        out.append((name, cells, S.ORIGIN, np.vstack([s, s]), np.vstack([g, g]), allow))
    return out


def _generated():
    out = []
    for name, nx, ny, seed in S.GENERATED:
        cells = S.generated_map(nx, ny, seed)
        origin = S.map_origin(cells)
        s, g = theta_legs(cells, origin, seed)
        if nx >= 96:
            ls, lg = S.lane_legs(cells, origin)                    # four more, after the thirty
            s, g = np.vstack([s, ls]), np.vstack([g, lg])
        out.append((name, cells, origin, s, g, np.arange(len(s)) % 4 != 3))      # every fourth leg with allow_unknown off
    return out


CASES = _known() + _generated()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def expected():
    """per map: the header's CPU search of every leg at the reference's weights — computed once, read by every test, left unchanged"""
    return {name: [S.leg(cells, origin, RES, s[i], g[i], allow_unknown=bool(allow[i])) for i in range(len(s))]
            for name, cells, origin, s, g, allow in CASES}


def _scorer(cells, origin):
    sc = fsmod.FrontierScorer(device=0)
    sc.upload_grid(cells[None], origin, RES)
    return sc


def _run(sc, s, g, allow, **kw):
    """the legs in at most two calls (allow_unknown is per call): a dict of per-leg lists in input order"""
    out = dict(status=[None] * len(s), cost=[None] * len(s), vertices=[None] * len(s), poses=[None] * len(s))
    for value in (True, False):
        idx = np.nonzero(allow == value)[0]
        if idx.size == 0:
            continue
        r = sc.refine_paths(s[idx], g[idx], allow_unknown=value, **kw)
        for j, i in enumerate(idx):
            for key in out:
                out[key][i] = r[key][j]
    return out


def _same(out, i, want, what):
    assert int(out["status"][i]) == want["status"], (what, i, int(out["status"][i]), want["status"])
    assert np.float64(out["cost"][i]).tobytes() == np.float64(want["cost"]).tobytes(), (what, i, out["cost"][i], want["cost"])
    assert out["vertices"][i].tobytes() == want["vertices"].tobytes(), (what, i)
    assert out["poses"][i].tobytes() == want["poses"].tobytes(), (what, i)


def _blob(out):
    return (np.asarray(out["status"], dtype=np.int32).tobytes() + np.asarray(out["cost"], dtype=np.float64).tobytes()
            + b"".join(v.tobytes() for v in out["vertices"]) + b"".join(p.tobytes() for p in out["poses"]))


@pytest.mark.parametrize("name,cells,origin,s,g,allow", CASES, ids=IDS)
def test_legs_equal_the_header_and_the_compiled_reference(name, cells, origin, s, g, allow, expected):
    B.require()
    sc = _scorer(cells, origin)
    try:
        sc.set_refine_search("reference")
        out = _run(sc, s, g, allow)
        classes = []
        for i in range(len(s)):
            _same(out, i, expected[name][i], name)
            want = B.theta_leg(cells, origin, RES, s[i], g[i], allow_unknown=bool(allow[i]))
            classes.append(_REF_CLASS[want["status"]])
            assert _CLASS[int(out["status"][i])] == classes[-1], (name, i)
            if want["status"] == B.FOUND:
                assert out["poses"][i].tobytes() == want["poses"].tobytes(), (name, i)
                assert np.vstack([out["vertices"][i], out["vertices"][i][-1:]]).tobytes() == want["raw"].tobytes(), (name, i)
        if name.startswith("gen_"):
            assert classes.count("found") >= 8 and classes.count("unsafe") >= 3 and classes.count("off") == 1, (name, classes)
            deep = max(e["max_heap"] for e in expected[name])
            assert deep >= 100 and sc.get_counter(1046) <= deep, (name, deep)
        if name == "corridor":
            assert classes[0] == "none" and int(out["status"][0]) == S.NO_PATH
        # other weights and corners: only the header's CPU search is the yardstick
        for kw in (dict(corners=4), dict(w_euc=0.5), dict(w_euc=0.5, w_traversal=3.0, corners=4), dict(w_euc=2.0, w_traversal=0.0)):
            got = _run(sc, s[:12], g[:12], allow[:12], **kw)
            for i in range(min(12, len(s))):
                _same(got, i, S.leg(cells, origin, RES, s[i], g[i], allow_unknown=bool(allow[i]), **kw), (name, kw))
    finally:
        sc.close()


def test_long_walks_take_a_second_lane_round(expected):
    """the 96 x 96 map has legs whose vertices lie more than 64 cells apart: a walk of two chunks of the ordered fold was accepted"""
    name, cells, origin, s, g, allow = CASES[-1]
    longest = 0
    for e in expected[name]:
        if e["status"] == S.OK and len(e["vertices"]) > 1:
            d = np.abs(np.diff(e["vertices"], axis=0)) / RES
            longest = max(longest, int(np.round(d.max())))
    assert longest > 64, longest


def test_slot_counts_and_single_calls_give_the_same_bytes(expected):
    name, cells, origin, s, g, allow = CASES[-3]                  # 64 x 48
    sc = _scorer(cells, origin)
    try:
        sc.set_refine_search("reference")
        every = _run(sc, s, g, allow)
        on_map = sum(1 for i in np.nonzero(~allow)[0] if expected[name][i]["status"] not in (S.START_OFF_MAP, S.GOAL_OFF_MAP))
        assert sc.get_counter(1042) == on_map and sc.get_counter(1043) == 1          # (the last call: the allow_unknown-off legs)
        want = _blob(every)
        for slots in (1, 3):
            sc.set_option("refine.search_slots", slots)
            got = _run(sc, s, g, allow)
            assert _blob(got) == want, slots
            assert sc.get_counter(1043) == -(-on_map // slots), slots
        sc.set_option("refine.search_slots", 0)
        sc.set_option("refine.search_bytes", 1)                   # a budget below one slot still runs one at a time
        assert _blob(_run(sc, s, g, allow)) == want
        assert sc.get_counter(1043) == on_map
        sc.set_option("refine.search_bytes", float(1 << 30))
        single = dict(status=[], cost=[], vertices=[], poses=[])
        for i in range(len(s)):
            r = sc.refine_paths(s[i:i + 1], g[i:i + 1], allow_unknown=bool(allow[i]))
            for key in single:
                single[key].append(r[key][0])
        assert _blob(single) == want
    finally:
        sc.close()


def test_duplicate_legs_are_searched_once(expected):
    name, cells, origin, s, g, allow = CASES[-2]                  # 48 x 64
    sc = _scorer(cells, origin)
    try:
        idx = [i for i in range(len(s)) if allow[i] and expected[name][i]["status"] == S.OK][:4]
        rows = idx + idx[::-1] + idx[:2]
        # the same cells from other points inside them
        jitter = np.array([S.centre(origin, *[int(v) for v in ((s[i] - np.array(origin[:2])) / RES)]) for i in rows])
        out = sc.refine_paths(jitter, g[rows], search="reference")
        assert sc.get_counter(1042) == len(idx)
        assert sc.get_counter(1044) == sum(expected[name][i]["pops"] for i in idx)
        assert sc.get_counter(1045) == sum(expected[name][i]["los_walks"] for i in idx)
        assert sc.get_counter(1046) == max(expected[name][i]["max_heap"] for i in idx)
        for j, i in enumerate(rows):
            _same(out, j, expected[name][i], "duplicates")
    finally:
        sc.close()


def test_corridor_is_5_under_reference_and_0_under_field():
    cells, a, b = S.corridor_map()
    s, g = [S.centre(S.ORIGIN, *a)], [S.centre(S.ORIGIN, *b)]
    sc = _scorer(cells, S.ORIGIN)
    try:
        assert sc.refine_paths(s, g, search="reference")["status"].tolist() == [S.NO_PATH]
        assert sc.refine_paths(s, g)["status"].tolist() == [S.OK]
        sc.set_refine_search("reference")
        assert sc.refine_paths(s, g)["status"].tolist() == [S.NO_PATH]
        assert sc.refine_paths(s, g, search="field")["status"].tolist() == [S.OK]
    finally:
        sc.close()


def test_field_search_and_its_cache_are_untouched():
    name, cells, origin, s, g, allow = CASES[-3]
    s, g = s[:12], g[:12]                                         # at most 12 start cells: all their fields stay in the slab of 16
    sc = _scorer(cells, origin)
    try:
        before = sc.refine_paths(s, g)
        built = sc.get_counter(1011)
        assert built > 0 and sc.get_counter(1042) == 0
        field = sc.refine_field(s[0])
        sc.set_refine_search("reference")
        ref = sc.refine_paths(s, g)
        assert sc.refine_field(s[0]).tobytes() == field.tobytes()          # fs_refine_field does not look at the setting
        sc.set_refine_search("field")
        after = sc.refine_paths(s, g)
        assert sc.get_counter(1011) == built                                # every field still from the cache
        assert _blob(after) == _blob(before)
        assert _blob(ref) != _blob(before)
        for w in (before, after):
            for i in range(len(s)):
                _same(w, i, T.leg(cells, origin, RES, s[i], g[i]), "field")
    finally:
        sc.close()


def test_search_keyword_restores_the_setting_also_after_a_refused_call():
    cells, a, b = S.corridor_map()
    s, g = [S.centre(S.ORIGIN, *a)], [S.centre(S.ORIGIN, *b)]
    sc = _scorer(cells, S.ORIGIN)
    try:
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths(s, g, corners=6, search="reference")
        assert e.value.code == fsmod.capi.FS_E_INVALID
        assert sc._refine_search == "field" and sc.refine_paths(s, g)["status"].tolist() == [S.OK]
        sc.set_refine_search("reference")
        with pytest.raises(fsmod.FsError):
            sc.refine_paths(s, g, w_euc=0.0, search="field")
        assert sc._refine_search == "reference" and sc.refine_paths(s, g)["status"].tolist() == [S.NO_PATH]
        with pytest.raises(fsmod.FsError):
            sc.refine_paths(s, g, search="nonsense")
        assert sc.refine_paths(s, g)["status"].tolist() == [S.NO_PATH]
    finally:
        sc.close()


def test_refine_tour_equals_the_legs_one_by_one():
    name, cells, origin, _, _, _ = CASES[-1]                      # 96 x 96
    sc = _scorer(cells, origin)
    try:
        rng = np.random.default_rng(5)
        ys, xs = np.nonzero(cells < 200)

        def points(k):
            i = rng.choice(xs.size, k)
            return np.stack([origin[0] + (xs[i] + 0.5) * RES, origin[1] + (ys[i] + 0.5) * RES], axis=1)
        sc.roadmap_add_nodes(points(80))
        sc.roadmap_rebuild()
        robot = points(1)[0]
        pose = np.array([robot[0], robot[1], 0.0, 0.0, 0.0, 0.0, 1.0])
        goal = np.zeros((10, 3))
        goal[:, :2] = points(10)
        plan = sc.roadmap_plan(pose, goal)
        ng = sc.roadmap_next_goal(pose, goal, plan["path_length_m"], plan["achievable"], n_local=4)
        tour = ng["tour"]
        assert len(tour) >= 1
        out = sc.refine_tour(pose, goal, ng, search="reference")
        assert sc._refine_search == "field"
        pts = np.vstack([robot[None], goal[tour, :2]])
        path = []
        for i in range(len(tour)):
            one = sc.refine_paths(pts[i:i + 1], pts[i + 1:i + 2], search="reference")
            for key in ("status", "cost", "vertices", "poses"):
                assert np.asarray(out[key][i]).tobytes() == np.asarray(one[key][0]).tobytes(), (i, key)
            _same(out, i, S.leg(cells, origin, RES, pts[i], pts[i + 1]), "tour")
            if one["status"][0] == S.OK:
                path.append(one["poses"][0])
        assert out["path"].tobytes() == (np.vstack(path) if path else np.zeros((0, 2))).tobytes()
    finally:
        sc.close()


def test_a_parent_chain_longer_than_the_vertex_scratch():
    """618 vertices against a first scratch of 256 per search: the scratch grows and the searches run again, once"""
    cells, a, b = S.serpentine_map()
    origin = S.map_origin(cells)
    s, g = [S.centre(origin, *a)], [S.centre(origin, *b)]
    want = S.leg(cells, origin, RES, s[0], g[0])
    assert want["status"] == S.OK and len(want["vertices"]) > 256
    sc = _scorer(cells, origin)
    try:
        sc.set_refine_search("reference")
        for what in ("grown", "again"):
            out = sc.refine_paths(s, g)
            _same(out, 0, want, what)
            assert (sc.get_counter(1042), sc.get_counter(1044)) == (1, want["pops"]), what
        ref = B.theta_leg(cells, origin, RES, s[0], g[0])
        assert ref["status"] == B.FOUND and out["poses"][0].tobytes() == ref["poses"].tobytes()
    finally:
        sc.close()


def test_sizing_call_with_null_arrays(expected):
    name, cells, origin, s, g, allow = CASES[-3]
    sc = _scorer(cells, origin)
    try:
        sc.set_refine_search("reference")
        idx = np.nonzero(allow)[0]
        ss, gg = np.ascontiguousarray(s[idx]), np.ascontiguousarray(g[idx])
        n = len(idx)
        st = np.zeros(n, dtype=np.int32); cost = np.zeros(n); nv = np.zeros(n, dtype=np.int32); npz = np.zeros(n, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert sc._L.fs_refine_paths(sc._h, n, p(ss), p(gg), 1, 1.0, 2.0, 8, p(st), p(cost), p(nv), None, p(npz), None) == 0
        for j, i in enumerate(idx):
            e = expected[name][i]
            assert (st[j], nv[j], npz[j]) == (e["status"], len(e["vertices"]), len(e["poses"])), i
            assert cost[j].tobytes() == np.float64(e["cost"]).tobytes()
        assert sc._L.fs_refine_paths(sc._h, 0, None, None, 1, 1.0, 2.0, 8, None, None, None, None, None, None) == 0
    finally:
        sc.close()


def test_refusals():
    cells, a, b = S.open_map()
    s, g = [S.centre(S.ORIGIN, *a)], [S.centre(S.ORIGIN, *b)]
    sc = fsmod.FrontierScorer(device=0)
    try:
        for bad in (2, -1, 7):
            assert sc._L.fs_set_refine_search(sc._h, bad) == fsmod.capi.FS_E_INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths(s, g)                                  # no grid; and the setting is still FIELD: FS_E_STATE either way
        assert e.value.code == fsmod.capi.FS_E_STATE
        sc.set_refine_search("reference")
        for bad in (2, -1):
            assert sc._L.fs_set_refine_search(sc._h, bad) == fsmod.capi.FS_E_INVALID
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths(s, g)
        assert e.value.code == fsmod.capi.FS_E_STATE
        sc.upload_grid(np.zeros((2, 8, 8), np.uint8), (0.0, 0.0, 0.0), RES)
        with pytest.raises(fsmod.FsError) as e:
            sc.refine_paths([[0.1, 0.1]], [[0.2, 0.2]])
        assert e.value.code == fsmod.capi.FS_E_INVALID
        sc.upload_grid(cells[None], S.ORIGIN, RES)
        assert sc.refine_paths(s, g)["status"].tolist() == [S.OK]          # the refused values left REFERENCE in place ...
        assert sc.get_counter(1042) == 1
        for kw in (dict(corners=6), dict(w_euc=0.0), dict(w_traversal=-1.0)):
            with pytest.raises(fsmod.FsError) as e:
                sc.refine_paths(s, g, **kw)
            assert e.value.code == fsmod.capi.FS_E_INVALID, kw
        for key, value in (("refine.search_slots", -1), ("refine.search_slots", 65536), ("refine.search_bytes", 0), ("refine.search_bytes", 2.0 ** 41)):
            with pytest.raises(fsmod.FsError) as e:
                sc.set_option(key, value)
            assert e.value.code == fsmod.capi.FS_E_INVALID, (key, value)
        off = sc.refine_paths([(-9.0, 0.0), s[0]], [g[0], (0.0, 9.0)])
        assert off["status"].tolist() == [S.START_OFF_MAP, S.GOAL_OFF_MAP] and sc.get_counter(1042) == 0
    finally:
        sc.close()
