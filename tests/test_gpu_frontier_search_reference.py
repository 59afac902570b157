"""fs_search_frontiers with FS_SEEDS_REFERENCE (the reference's outer search on the device) against the oracle's
FrontierSearch::searchFrom bit for bit, without caller seeds: on the test maps, hand-built edge maps and random floor plans; the
one call under Reference against the two-call chain; the default, the override and the refusals; the outer-search counters."""
import numpy as np
import pytest

import frontier_outer_ref as R
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


def _check_against_oracle(oracle, sc, cells, origin, res, pos, prm, name):
    """Reference search (no seeds) = oracle.frontier_search; returns (records, oracle result)."""
    mx, mn, lethal, max_d = prm
    ny, nx = cells.shape
    r = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=lethal, min_cluster=mn, max_cluster=mx, max_distance=max_d)
    sc.upload_grid(cells[None], origin, res)
    kw = dict(lethal_threshold=lethal, max_frontier_distance=max_d, min_frontier_cluster_size=mn, max_frontier_cluster_size=mx)
    fr, every = sc.search_frontiers(pos, **kw)
    assert fr.shape[0] == r["goals"].shape[0], name
    np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(r["goals"][:, 0]), err_msg=name)
    np.testing.assert_array_equal(_bits(fr["goal_y"]), _bits(r["goals"][:, 1]), err_msg=name)
    np.testing.assert_array_equal(fr["size"], r["sizes"], err_msg=name)
    np.testing.assert_array_equal(fr["seed_cell"], r["cell_seed"].ravel()[fr["goal_cell"]], err_msg=name)
    assert every.shape[0] == r["n_every"], name
    seeds = FR.oracle_seeds(r)
    if r["n_every"]:
        cp = M.pieces_from_every(_cells_of(every, origin, res, nx), seeds, FR.oracle_labels(r), mx, (ny, nx))
        np.testing.assert_array_equal(cp, r["cell_piece"], err_msg=name)              # cell-to-piece membership
    # the same records as the caller-seeded call with the oracle's seeds, field for field
    fr_s, every_s = sc.search_frontiers(pos, seeds=seeds, **kw)
    assert fr.tobytes() == fr_s.tobytes(), name
    assert every.tobytes() == every_s.tobytes(), name
    return fr, r


@pytest.mark.parametrize("prm", M.PARAMS)
def test_reference_search_equals_the_oracle(fs, oracle, prm):
    sc = fs.FrontierScorer(device=0)
    try:
        sc.set_frontier_seed_order("reference")
        total = 0
        for name, cells, origin, res, pos in MAPS:
            fr, _ = _check_against_oracle(oracle, sc, cells, origin, res, pos, prm, name)
            total += fr.shape[0]
        assert total > 50
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
    mx = sc.max_arrival()
    sc.set_arrival_limits(4000.0, mx["min_gt"])


@pytest.mark.parametrize("which", ["small", "REF2D"])
def test_one_call_under_reference_equals_search_then_planned(fs, oracle, which):
    w = fs.synth.make_small_2d(3, n=160, n_cand=40) if which == "small" else fs.synth.make_workload("REF2D", n_cand=16, n_landmarks=20_000)
    cells = w.cells[0]
    pos = M._free_pos(cells, w.origin, w.resolution, len(np.argwhere(cells == 0)) // 3)
    pose = np.array([pos[0], pos[1], 0.0, 0.0, 0.0, 0.0, 1.0])
    sc = fs.FrontierScorer(device=0)
    try:
        _setup_scoring(sc, w)
        sc.set_frontier_seed_order("reference")
        fr, _ = sc.search_frontiers(pos, want_every=False)
        assert fr.shape[0] > 2
        r = oracle.frontier_search(cells, w.origin[:2], w.resolution, pos)
        np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(r["goals"][:, 0]))
        goal = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
        for black in (None, goal[::3, :2].copy()):
            bmask = None if black is None else np.array([any(g[0] == b[0] and g[1] == b[1] for b in black) for g in goal], np.uint8)
            for fim in (False, True):
                want = sc.get_frontier_costs_planned(pose, goal, frontier_size=fr["size"], blacklisted=bmask, with_fim=fim)
                got_fr, got = sc.get_frontier_costs_searched(pose, blacklist_xy=black, with_fim=fim)
                assert got_fr.tobytes() == fr.tobytes()
                for k in want:
                    if fim and k == "records":
                        # (the Fisher float sums are not run-to-run bit-stable in the scorer itself: test_gpu_frontier_search)
                        for f in want[k].dtype.names:
                            if f in ("info_ref", "trace", "logdet"):
                                np.testing.assert_allclose(got[k][f], want[k][f], rtol=1e-5, err_msg=f"{which} {f}")
                            else:
                                assert got[k][f].tobytes() == want[k][f].tobytes(), (which, f)
                    else:
                        assert got[k].tobytes() == want[k].tobytes(), (which, k, fim, black is None)
        # the per-call keyword gives the same one call on a context left at Nearest
        sc.set_frontier_seed_order("nearest")
        got_fr, got = sc.get_frontier_costs_searched(pose, seed_order="reference")
        want = sc.get_frontier_costs_planned(pose, goal, frontier_size=fr["size"])
        assert got_fr.tobytes() == fr.tobytes() and got["order"].tobytes() == want["order"].tobytes()
        near, _ = sc.search_frontiers(pos, want_every=False)
        near1, _ = sc.get_frontier_costs_searched(pose)
        assert near.tobytes() == near1.tobytes()
    finally:
        sc.close()


def test_default_override_and_refusals(fs, oracle):
    name, cells, origin, res, pos = [m for m in MAPS if m[0] == "small9_512_0"][0]
    r = oracle.frontier_search(cells, origin[:2], res, pos)
    labels = FR.oracle_labels(r)
    nearest = FR.search(labels, origin, res, M.robot_cell(cells, origin, res, pos))
    sc = fs.FrontierScorer(device=0)
    try:
        sc.upload_grid(cells[None], origin, res)

        def same_as_nearest(fr):
            assert fr.shape[0] == nearest["goals"].shape[0]
            np.testing.assert_array_equal(_bits(fr["goal_x"]), _bits(nearest["goals"][:, 0]))
            np.testing.assert_array_equal(_bits(fr["goal_y"]), _bits(nearest["goals"][:, 1]))
            np.testing.assert_array_equal(fr["seed_cell"], nearest["seed_cell"])

        fresh, _ = sc.search_frontiers(pos)                       # a fresh context: Nearest
        same_as_nearest(fresh)
        sc.set_frontier_seed_order("reference")
        ref, _ = sc.search_frontiers(pos)
        np.testing.assert_array_equal(_bits(ref["goal_x"]), _bits(r["goals"][:, 0]))
        assert ref.tobytes() != fresh.tobytes()                   # (this map's two orders differ)
        # caller seeds win over the setting
        seeds = nearest["seed_cell"][np.unique(nearest["label"], return_index=True)[1]]
        seeds = np.ascontiguousarray(seeds[::-1])
        under_ref, _ = sc.search_frontiers(pos, seeds=seeds)
        sc.set_frontier_seed_order("nearest")
        under_near, _ = sc.search_frontiers(pos, seeds=seeds)
        assert under_ref.tobytes() == under_near.tobytes()
        np.testing.assert_array_equal(np.unique(under_ref["seed_cell"]), np.unique(seeds))
        back, _ = sc.search_frontiers(pos)                        # set back to Nearest
        same_as_nearest(back)
        # an unknown value: FS_E_INVALID, the setting unchanged
        sc.set_frontier_seed_order("reference")
        for bad in (2, -1, 1 << 20):
            assert sc._L.fs_set_frontier_seed_order(sc._h, bad) == fs.capi.FS_E_INVALID
        assert sc._L.fs_set_frontier_seed_order(None, 1) == fs.capi.FS_E_INVALID
        again, _ = sc.search_frontiers(pos)
        assert again.tobytes() == ref.tobytes()
        with pytest.raises(fs.FsError):
            sc.set_frontier_seed_order("outer")
        # the per-call keyword applies to that call only
        one, _ = sc.search_frontiers(pos, seed_order="nearest")
        same_as_nearest(one)
        after, _ = sc.search_frontiers(pos)
        assert after.tobytes() == ref.tobytes()
        sc.set_frontier_seed_order("nearest")
        one, _ = sc.search_frontiers(pos, seed_order="reference")
        assert one.tobytes() == ref.tobytes()
        same_as_nearest(sc.search_frontiers(pos)[0])
    finally:
        sc.close()


def _edge_maps():
    """(name, cells, origin, res, robot_xy, params)"""
    out = []
    res, o = 0.05, (0.0, 0.0, 0.0)
    at = lambda x, y: (o[0] + (x + 0.5) * res, o[1] + (y + 0.5) * res)    # noqa: E731
    # two one-cell components met on the same level: the stub below the corridor is claimed first (slot order of the start's
    # left neighbour), so the component with the larger label and the larger cell index comes first
    a = np.full((20, 20), 255, np.uint8)
    a[9:12, :] = 254
    a[10, 9:12] = 0
    a[9, 11] = 0            # stub up from the right cell: frontier (11, 8)
    a[11, 9] = 0            # stub down from the left cell: frontier (9, 12)
    out.append(("same_level", a, o, res, at(10, 10), (20, 0, 160, 50.0)))
    # a free cell just outside the search radius next to a frontier: visited, never expanded
    b = np.full((24, 40), 254, np.uint8)
    b[12, 2:26] = 0                         # (25, 12) lies just outside the radius
    b[10:15, 26:29] = 255                   # frontier (26, 12): next to (25, 12) only
    b[9:12, 9:12] = 255                     # frontier (10, 11): next to an expanded cell
    out.append(("outside_reach", b, o, res, at(2, 12), (2, 0, 160, 1.0)))
    assert 22 < (1.0 + 2 * res * 1.414) / res < 23
    # the robot on an unknown cell: the search starts at nearestFreeCell's cell
    c = np.full((40, 40), 255, np.uint8)
    c[20:30, 20:32] = 0; c[24, 25] = 254
    out.append(("unknown_robot", c, o, res, at(12, 14), (5, 1, 160, 50.0)))
    # no free cell at all
    out.append(("no_free", np.full((16, 16), 255, np.uint8), o, res, at(3, 4), (20, 1, 160, 50.0)))
    out.append(("no_free_lethal", np.where(np.indices((16, 16)).sum(0) % 3 == 0, 254, 255).astype(np.uint8), o, res, at(3, 4), (20, 0, 160, 50.0)))
    # a region with no frontier (and a walled-off frontier region it never reaches)
    d = np.zeros((32, 32), np.uint8)
    d[:, 16] = 254; d[10:20, 24:30] = 255
    out.append(("no_frontier", d, o, res, at(4, 4), (20, 1, 160, 50.0)))
    return out


def test_edge_maps(fs, oracle):
    sc = fs.FrontierScorer(device=0)
    try:
        sc.set_frontier_seed_order("reference")
        for name, cells, origin, res, pos, prm in _edge_maps():
            fr, r = _check_against_oracle(oracle, sc, cells, origin, res, pos, prm, name)
            mx, mn, lethal, max_d = prm
            if name == "same_level":
                ny, nx = cells.shape
                assert list(fr["seed_cell"]) == [12 * nx + 9, 8 * nx + 11]
                near, _ = sc.search_frontiers(pos, lethal_threshold=lethal, max_frontier_distance=max_d, min_frontier_cluster_size=mn,
                                              max_frontier_cluster_size=mx, seed_order="nearest")
                assert near.shape[0] == 2 and not np.array_equal(_bits(near["goal_x"]), _bits(r["goals"][:, 0]))
                assert sc.get_counter(1019) == 3 and sc.get_counter(1020) == 5
            if name == "outside_reach":
                assert fr.shape[0] == 1 and r["cell_seed"][12, 26] < 0 and r["cell_seed"][11, 10] >= 0
            if name in ("no_free", "no_free_lethal", "no_frontier"):
                assert fr.shape[0] == 0
            if name == "unknown_robot":
                assert fr.shape[0] > 2
        # the robot off the map: no records, no levels
        cells = _edge_maps()[0][1]
        sc.upload_grid(cells[None], (0.0, 0.0, 0.0), 0.05)
        fr, ev = sc.search_frontiers((-1.0, 0.3))
        assert fr.shape[0] == 0 and ev.shape[0] == 0
        assert sc.get_counter(1019) == 0 and sc.get_counter(1020) == 0
    finally:
        sc.close()


def test_random_floor_plans(fs, oracle):
    rng = np.random.default_rng(20261016)
    sc = fs.FrontierScorer(device=0)
    try:
        sc.set_frontier_seed_order("reference")
        records = 0
        for k in range(56):
            n = int(rng.integers(64, 513))
            plan = fs.synth.make_grid(rng, n, 1)[0]
            ny, nx = int(rng.integers(64, n + 1)), int(rng.integers(64, n + 1))
            cells = np.ascontiguousarray(plan[:ny, :nx])
            res = float(rng.choice([0.05, 0.1]))
            origin = (float(rng.uniform(-20, 0)), float(rng.uniform(-20, 0)), 0.0)
            free = np.argwhere(cells < 254)
            y, x = free[int(rng.integers(len(free)))] if len(free) and k % 7 else (int(rng.integers(ny)), int(rng.integers(nx)))
            pos = (origin[0] + (x + float(rng.uniform(0.01, 0.99))) * res, origin[1] + (y + float(rng.uniform(0.01, 0.99))) * res)
            prm = (int(rng.choice([1, 3, 10, 20, 60, 400])), int(rng.integers(0, 4)), int(rng.choice([1, 100, 160, 250, 254])),
                   float(rng.choice([0.5, 2.0, 5.0, 50.0])))
            fr, _ = _check_against_oracle(oracle, sc, cells, origin, res, pos, prm, f"random {k} {nx}x{ny} {prm}")
            records += fr.shape[0]
        assert records > 200
    finally:
        sc.close()


def test_outer_counters(fs, oracle):
    """1019 = the level (from 1 at the start cell) whose popped cell first met the last component, 1020 = the cells of levels up to
    it; at most the whole search's depth, and less on some map: the walk ended early."""
    sc = fs.FrontierScorer(device=0)
    try:
        sc.set_frontier_seed_order("reference")
        early, spiral_levels = 0, 0
        for name, cells, origin, res, pos in [m for m in MAPS if m[0] != "plan_1024"]:
            for prm in M.PARAMS[:2] + M.PARAMS[2:3]:
                mx, mn, lethal, max_d = prm
                r = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=lethal, min_cluster=mn, max_cluster=mx,
                                           max_distance=max_d)
                o = R.outer_search(cells, origin, res, pos, r["cell_seed"], lethal, mx, max_d)
                np.testing.assert_array_equal(o["seeds"], FR.oracle_seeds(r), err_msg=name)
                sc.upload_grid(cells[None], origin, res)
                sc.search_frontiers(pos, lethal_threshold=lethal, max_frontier_distance=max_d, min_frontier_cluster_size=mn,
                                    max_frontier_cluster_size=mx, want_every=False)
                assert sc.get_counter(1019) == o["levels"], (name, prm)
                assert sc.get_counter(1020) == o["popped"], (name, prm)
                assert o["levels"] <= o["depth"]
                early += o["levels"] < o["depth"]
                if name == "spiral":
                    spiral_levels = max(spiral_levels, o["levels"])
        assert early > 0
        assert spiral_levels > 3000
    finally:
        sc.close()
