"""fs_search_frontiers (FrontierSearch::searchFrom on the device, pieces and goal points included) against the
oracle's restatement of the reference's search with the oracle's seeds, against the CPU restatement tests/frontier_ref with Nearest
seeds, bit for bit; fs_get_frontier_costs_searched against fs_search_frontiers -> fs_get_frontier_costs_planned (and, for a list
longer than the first fetch round, the roadmap form against its three stages); the refusals."""
import numpy as np
import pytest

import frontier_ref as FR
import frontier_search_maps as M

pytestmark = pytest.mark.gpu

MAPS = M.maps(large=True, spiral=True)


def _cells_of(every_xy, origin, res, nx):
    x = np.floor((every_xy[:, 0] - origin[0]) / res).astype(np.int64)
    y = np.floor((every_xy[:, 1] - origin[1]) / res).astype(np.int64)
    return (y * nx + x).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("prm", M.PARAMS)
def test_oracle_seeded_search_equals_the_reference_order(fs, oracle, scorer, prm):
    mx, mn, lethal, max_d = prm
    total = 0
    for name, cells, origin, res, pos in MAPS:
        ny, nx = cells.shape
        r = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=lethal, min_cluster=mn, max_cluster=mx, max_distance=max_d)
        seeds = FR.oracle_seeds(r)
        scorer.upload_grid(cells[None], origin, res)
        fr, every = scorer.search_frontiers(pos, lethal_threshold=lethal, max_frontier_distance=max_d, min_frontier_cluster_size=mn,
                                            max_frontier_cluster_size=mx, seeds=seeds)
        assert fr.shape[0] == r["goals"].shape[0], name
        np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(r["goals"][:, 0]), err_msg=name)
        np.testing.assert_array_equal(_bits(fr["goal_y"]), _bits(r["goals"][:, 1]), err_msg=name)
        np.testing.assert_array_equal(fr["size"], r["sizes"], err_msg=name)
        assert every.shape[0] == r["n_every"]
        labels = FR.oracle_labels(r)
        cp = M.pieces_from_every(_cells_of(every, origin, res, nx), seeds, labels, mx, (ny, nx))
        np.testing.assert_array_equal(cp, r["cell_piece"], err_msg=name)             # cell-to-piece membership
        np.testing.assert_array_equal(fr["label"], labels.ravel()[fr["goal_cell"]])
        total += fr.shape[0]
    assert total > 100


@pytest.mark.parametrize("prm", M.PARAMS)
def test_nearest_search_equals_the_restatement(fs, oracle, scorer, prm):
    mx, mn, lethal, max_d = prm
    levels = 0
    for name, cells, origin, res, pos in MAPS:
        ny, nx = cells.shape
        r = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=lethal, min_cluster=mn, max_cluster=mx, max_distance=max_d)
        labels = FR.oracle_labels(r)
        s = FR.search(labels, origin, res, M.robot_cell(cells, origin, res, pos), min_size=mn, max_size=mx)
        scorer.upload_grid(cells[None], origin, res)
        fr, every = scorer.search_frontiers(pos, lethal_threshold=lethal, max_frontier_distance=max_d, min_frontier_cluster_size=mn,
                                            max_frontier_cluster_size=mx)
        assert fr.shape[0] == s["goals"].shape[0], name
        np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(s["goals"][:, 0]), err_msg=name)
        np.testing.assert_array_equal(_bits(fr["goal_y"]), _bits(s["goals"][:, 1]), err_msg=name)
        for f in ("size", "label", "goal_cell", "seed_cell"):
            np.testing.assert_array_equal(fr[f], s[f if f != "size" else "sizes"], err_msg=f"{name} {f}")
        np.testing.assert_array_equal(_cells_of(every, origin, res, nx), s["every_cells"], err_msg=name)
        assert scorer.get_counter(1015) == s["guarded"]
        levels = max(levels, scorer.get_counter(1014))
    assert levels > 1


def _setup_scoring(sc, w):
    sc.set_ray_params(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov,
                      robot_radius=w.robot_radius, n_rays=w.n_yaw, elev=w.elev, polygon=w.polygon)
    sc.upload_grid(w.cells, w.origin, w.resolution)
    sc.set_option("fim.learn", 0)          # (the learnt pass prediction makes Fisher sums depend on the calls served before)
    sc.upload_landmarks(w.landmarks)
    sc.lookup_generate()
    sc.set_fim_params(14.0, 1.0)
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])


@pytest.mark.parametrize("which", ["small", "REF2D"])
def test_one_call_equals_search_then_planned(fs, which):
    w = fs.synth.make_small_2d(3, n=160, n_cand=40) if which == "small" else fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=20_000)
    cells = w.cells[0]
    pos = M._free_pos(cells, w.origin, w.resolution, len(np.argwhere(cells == 0)) // 3)
    pose = np.array([pos[0], pos[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    sc = fs.FrontierScorer(device=0)
    try:
        _setup_scoring(sc, w)
        fr, _ = sc.search_frontiers(pos, want_every=False)
        assert fr.shape[0] > 2
        goal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
        for black in (None, goal[::3, :2].copy()):
            bmask = None if black is None else np.array([any(g[0] == b[0] and g[1] == b[1] for b in black) for g in goal], np.uint8)
            for fim in (False, True):
                want = sc.get_frontier_costs_planned(pose, goal, frontier_size=fr["size"], blacklisted=bmask, with_fim=fim)
                got_fr, got = sc.get_frontier_costs_searched(pose, blacklist_xy=black, with_fim=fim)
                assert got_fr.tobytes() == fr.tobytes()
                for k in want:
                    if fim and k == "records":
                        # the Fisher float sums are not run-to-run bit-stable in the scorer itself (two get_frontier_costs_planned
                        # calls on the same columns differ in info_ref's last bits); every other field exactly
                        g, e = got[k], want[k]
                        for f in e.dtype.names:
                            if f in ("info_ref", "trace", "logdet"):
                                np.testing.assert_allclose(g[f], e[f], rtol=1e-5, err_msg=f"{which} {f}")
                            else:
                                assert g[f].tobytes() == e[f].tobytes(), (which, f)
                    else:                               # (the ranking reads only the records' integers)
                        assert got[k].tobytes() == want[k].tobytes(), (which, k, fim, black is None)
        # more records than the caller holds: refused, the count reported
        with pytest.raises(fs.FsError, match="no partial ranking"):
            sc.get_frontier_costs_searched(pose, max_records=fr.shape[0] - 1)
    finally:
        sc.close()


def test_refusals_and_staged_state(fs, oracle, scorer):
    name, cells, origin, res, pos = [m for m in MAPS if m[0] == "small9_512_0"][0]
    ny, nx = cells.shape
    scorer.upload_grid(cells[None], origin, res)
    labels0, cl0, n0, c0 = scorer.frontier_clusters((ny, nx), pos)
    fr_all, every = scorer.search_frontiers(pos)
    assert fr_all.shape[0] > 3
    # the clusters call is unchanged after a search
    labels1, cl1, n1, c1 = scorer.frontier_clusters((ny, nx), pos)
    np.testing.assert_array_equal(labels0, labels1)
    np.testing.assert_array_equal(cl0, cl1)
    assert (n0, c0) == (n1, c1) and c0 == every.shape[0]
    # capacity too small: the count is reported, the first records stored
    few, _ = scorer.search_frontiers(pos, max_records=3, want_every=False)
    np.testing.assert_array_equal(few, fr_all[:3])
    assert scorer.last_search_counts[0] == fr_all.shape[0]
    pose = np.array([pos[0], pos[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    with pytest.raises(fs.FsError):
        scorer.get_frontier_costs_searched(pose, max_records=3)
    # invalid seeds: not a frontier cell, two seeds in one component, off the map; the context stays usable
    non_frontier = int(np.flatnonzero(labels0.ravel() < 0)[0])
    s0 = int(fr_all["seed_cell"][0])
    same = int(np.flatnonzero(labels0.ravel() == labels0.ravel()[s0])[-1])
    for bad in ([non_frontier], [s0, same] if same != s0 else [s0, s0], [nx * ny]):
        with pytest.raises(fs.FsError):
            scorer.search_frontiers(pos, seeds=bad)
    again, _ = scorer.search_frontiers(pos)
    np.testing.assert_array_equal(again, fr_all)
    # robot off the map: no records
    fr, ev = scorer.search_frontiers((origin[0] - 1.0, origin[1]))
    assert fr.shape[0] == 0 and ev.shape[0] == 0
    # no frontier cells
    z = np.zeros((32, 32), np.uint8)
    scorer.upload_grid(z[None], (0.0, 0.0, 0.0), 0.05)
    fr, ev = scorer.search_frontiers((0.5, 0.5))
    assert fr.shape[0] == 0 and ev.shape[0] == 0
    # nz > 1
    c3 = fs.synth.make_workload("C1", n_cand=4)
    scorer.upload_grid(c3.cells, c3.origin, c3.resolution)
    with pytest.raises(fs.FsError):
        scorer.search_frontiers((0.0, 0.0))


def test_uncut_components_at_int32_max(fs, oracle, scorer):
    """max_frontier_cluster_size = INT32_MAX (no cutting) equals the reference's search, and nx * ny, record for record."""
    big = 2 ** 31 - 1
    for name, cells, origin, res, pos in [m for m in MAPS if m[0] in ("rooms", "small9_512_0", "REF2D")]:
        ny, nx = cells.shape
        r = oracle.frontier_search(cells, origin[:2], res, pos, max_cluster=big)
        scorer.upload_grid(cells[None], origin, res)
        fr, every = scorer.search_frontiers(pos, max_frontier_cluster_size=big, seeds=FR.oracle_seeds(r))
        assert fr.shape[0] == r["goals"].shape[0] > 0, name
        np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(r["goals"][:, 0]), err_msg=name)
        np.testing.assert_array_equal(_bits(fr["goal_y"]), _bits(r["goals"][:, 1]), err_msg=name)
        np.testing.assert_array_equal(fr["size"], r["sizes"], err_msg=name)
        assert every.shape[0] == r["n_every"]
        a, _ = scorer.search_frontiers(pos, max_frontier_cluster_size=big)
        b, _ = scorer.search_frontiers(pos, max_frontier_cluster_size=nx * ny)
        assert a.tobytes() == b.tobytes() and (a["size"] > 0).all()


def test_python_buffers_grow_to_the_search(fs, scorer):
    """The Python route starts with small buffers and searches again with exact sizes when the list is longer."""
    name, cells, origin, res, pos = [m for m in MAPS if m[0] == "small9_512_0"][0]
    scorer.upload_grid(cells[None], origin, res)
    full, every = scorer.search_frontiers(pos)
    sc = fs.FrontierScorer(device=0)
    try:
        sc.SEARCH_FIRST_RECORDS, sc.SEARCH_FIRST_CELLS = 2, 3
        sc.upload_grid(cells[None], origin, res)
        small, ev = sc.search_frontiers(pos)
        assert small.tobytes() == full.tobytes() and ev.tobytes() == every.tobytes() and full.shape[0] > 2
    finally:
        sc.close()


def _island_map(n=204, step=6):
    """Free space with a 2 x 2 unknown island every `step` cells — one frontier component per island, (n / step)^2 of them — and
    the robot in the middle.  0.3 m between islands: the roadmap update keeps every goal (closer than 0.25 m it drops them) and
    fills no 1 m cell beyond its 20 nodes."""
    cells = np.zeros((n, n), np.uint8)
    for a in range(2):
        for b in range(2):
            cells[2 + a::step, 2 + b::step] = 255
    origin = (-n * 0.05 / 2, -n * 0.05 / 2, 0.0)
    return cells, origin, 0.05, (origin[0] + (n // 2 + 0.3) * 0.05, origin[1] + (n // 2 + 0.6) * 0.05)


def _raw_searched(fs, sc, name, pose, max_size, cap):
    """fs_get_frontier_costs_searched / _searched_roadmap as C sees them, into arrays filled with a pattern: (rc, n_frontiers, arrays)"""
    import ctypes as C
    P = fs.capi
    out = dict(fr=np.full(cap, 0x5A, np.uint8).repeat(P.FRONTIER_RECORD_DTYPE.itemsize).view(P.FRONTIER_RECORD_DTYPE),
               rec=np.full(cap, 0x5A, np.uint8).repeat(P.RECORD_DTYPE.itemsize).view(P.RECORD_DTYPE),
               cost=np.full(cap, -7.0), order=np.full(cap, -7, np.int32))
    before = {k: v.tobytes() for k, v in out.items()}
    n = C.c_int32(-1)
    p7 = (C.c_double * 7)(*[float(v) for v in pose])
    rc = getattr(sc._L, name)(sc._h, C.byref(p7), 160, 50.0, 1, max_size, 0, 0, None, 0.25, 1.0, 0.5, 0.5, 0, cap, P._p(out["fr"]), C.byref(n),
                              P._p(out["rec"]), P._p(out["cost"]), None, None, P._p(out["order"]), None)
    return rc, n.value, all(out[k].tobytes() == before[k] for k in out)


def test_searched_list_longer_than_one_fetch_round(fs, oracle):
    """The one-call forms fetch the found records in a first round of at most 1 024 and the rest in a second: a list of 1 156
    equals search -> plan -> costs record for record, on the grid planner and on the roadmap; one record short of room, both
    refuse with the count and write nothing (the roadmap form before it touches the roadmap)."""
    import dataclasses
    cells, origin, res, pos = _island_map()
    mx = 2
    count = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=160, min_cluster=1, max_cluster=mx,
                                   max_distance=50.0)["goals"].shape[0]
    assert count == 34 * 34 > 1024
    w = dataclasses.replace(fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=2000), cells=cells[None], origin=origin, resolution=res)
    pose = np.array([pos[0], pos[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    one, three = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for sc in (one, three):
            _setup_scoring(sc, w)
        fr, _ = three.search_frontiers(pos, max_frontier_cluster_size=mx, want_every=False)
        assert fr.shape[0] == count
        goal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(count)], axis=1)

        def same(got_fr, got, want, what):
            assert got_fr.tobytes() == fr.tobytes(), what
            for k in want:                                   # (no Fisher information: every column is exact)
                assert got[k].tobytes() == want[k].tobytes(), (what, k)

        # refused first, on contexts that have planned nothing yet: nothing is written, the roadmap stays empty
        for name in ("fs_get_frontier_costs_searched", "fs_get_frontier_costs_searched_roadmap"):
            rc, n, untouched = _raw_searched(fs, one, name, pose, mx, count - 1)
            assert (rc, n, untouched) == (fs.capi.FS_E_INVALID, count, True), name
            assert f"{count} frontiers found, room for {count - 1}: no partial ranking" in one._L.fs_last_error(one._h).decode()
        assert one.roadmap_graph()["xy"].size == 0
        want = three.get_frontier_costs_planned(pose, goal, frontier_size=fr["size"])
        same(*one.get_frontier_costs_searched(pose, max_frontier_cluster_size=mx), want, "planned")
        three.roadmap_update(goal[:, :2].copy(), pos)
        got_fr, got = one.get_frontier_costs_searched_roadmap(pose, max_frontier_cluster_size=mx)
        g1, g3 = one.roadmap_graph(), three.roadmap_graph()
        for key in ("xy", "key", "row_ptr", "col"):
            assert g1[key].tobytes() == g3[key].tobytes(), key
        assert g1["xy"].size > 2 * 1024
        same(got_fr, got, three.get_frontier_costs_roadmap(pose, goal, frontier_size=fr["size"]), "roadmap")
    finally:
        one.close(); three.close()
