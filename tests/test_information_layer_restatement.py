"""The information layer's rule on the CPU: anchors against a brute-force search, the cost formula at its corners,
MEAN as a sequential fp64 loop, block geometry — the entry points' declarations, exports, bindings and NULL-context refusals — the
preconditions the GPU tests state about their maps, and the two-door planning scenario end to end with planner_ref, the oracle
and the restatement.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import information_layer_ref as L
import inflation_ref as I
import pathinfo_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fitslam_frontier.h")
WINDOWS = {"whole": None, "odd": (13, 7, 37, 21), "corner": (0, 0, 29, 17), "far_corner": (-23, -31, 23, 31), "wide": (3, 5, 71, 18),
           "stride1": (31, 22, 24, 17)}


def _window(name, cells):
    ny, nx = cells.shape
    w = WINDOWS[name]
    if w is None:
        return (0, 0, nx, ny)
    return (w[0] % nx, w[1] % ny, w[2], w[3])


@pytest.mark.parametrize("m", list(L.MAPS))
def test_anchors_against_brute_force(m):
    cells, _ = L.layer_map(m)
    for name in WINDOWS:
        for s in (1, 5, 7, 32):
            if s == 1 and name != "stride1":
                continue
            win = _window(name, cells)
            a = L.anchors(cells, win, s)
            np.testing.assert_array_equal(a, L.anchors_brute(cells, win, s), err_msg=f"{name} {s}")
            assert a.shape == L.blocks(win, s)[::-1]
            ok = a >= 0
            assert (cells.reshape(-1)[a[ok]] <= 252).all()


@pytest.mark.parametrize("m", list(L.MAPS))
def test_maps_have_an_unscored_block_and_an_off_centre_anchor(m):
    cells, lm = L.layer_map(m)
    ny, nx = cells.shape
    assert lm.shape == (L.N_LANDMARKS, 3) and (cells == 255).any() and (cells == 254).any() and (cells >= 253).sum() > 100
    for s in (5, 7):
        win = (0, 0, nx, ny)
        a = L.anchors(cells, win, s)
        nbx, nby = L.blocks(win, s)
        assert (a < 0).any() and (a >= 0).sum() > 64
        centre = np.array([[L.block_box(win, s, i, j)[5] * nx + L.block_box(win, s, i, j)[4] for i in range(nbx)] for j in range(nby)])
        assert ((a >= 0) & (a != centre)).any()
    assert (L.anchors(cells, (0, 0, nx, ny), 3) >= 0).sum() > 256                  # the compaction crosses a workgroup seam
    s1 = L.anchors(cells, _window("stride1", cells), 1)
    assert (s1 < 0).any() and (s1 >= 0).sum() > 64


def test_block_geometry():
    assert L.blocks((3, 4, 37, 21), 5) == (8, 5) and L.blocks((0, 0, 24, 17), 1) == (24, 17) and L.blocks((9, 9, 7, 3), 32) == (1, 1)
    assert L.blocks((0, 0, 0, 5), 5) == (0, 1)
    # the last block of a window that is no multiple of the stride is cut, its centre clamped into the window
    assert L.block_box((3, 4, 37, 21), 5, 7, 4) == (38, 24, 40, 25, 39, 24)
    assert L.block_box((3, 4, 37, 21), 5, 0, 0) == (3, 4, 8, 9, 5, 6)
    assert L.block_box((9, 9, 7, 3), 32, 0, 0) == (9, 9, 16, 12, 15, 11)              # a stride larger than the window
    assert L.block_box((0, 0, 24, 17), 1, 23, 16) == (23, 16, 24, 17, 23, 16)
    cells = np.zeros((12, 16), np.uint8)
    cells[9:12, 9:16] = 254
    cells[10, 9] = 7
    a = L.anchors(cells, (9, 9, 7, 3), 32)
    assert a.shape == (1, 1) and a[0, 0] == 10 * 16 + 9
    # ties: (d2, y, x) — the centre (2, 2) of a 5 x 5 block taken out, its four neighbours tie, the smaller y wins
    cells = np.zeros((5, 5), np.uint8)
    cells[2, 2] = 254
    assert L.anchors(cells, (0, 0, 5, 5), 5)[0, 0] == 1 * 5 + 2
    cells[1, 2] = 253
    assert L.anchors(cells, (0, 0, 5, 5), 5)[0, 0] == 2 * 5 + 1                       # same y: the smaller x


def test_cost_formula_at_its_corners():
    lo, hi = 550.0, 1100.0
    f = lambda v, mc=252: int(L.cost_of(np.float32(v), lo, hi, mc))
    assert f(lo) == 252 and f(hi) == 0 and f(100.0) == 252 and f(-5.0) == 252 and f(5000.0) == 0 and f(np.inf) == 0
    assert f(np.nan) == 0 and f(-np.inf) == 252
    assert f(825.0) == 126 and f(np.nextafter(np.float32(825.0), np.float32(2000.0))) == 125     # exactly on an integer edge, and just past
    assert f(1100.0 - 550.0 / 252.0 * 3) in (2, 3)
    assert f(hi - 1e-3) == 0 and f(lo + 1e-3) == 251 and f(lo, 1) == 1 and f(lo + 1e-3, 1) == 0
    # scalar python floats, operation by operation, give the same bytes as the array form
    v = np.random.default_rng(3).uniform(400, 1300, size=4000).astype(np.float32)
    want = []
    for x in v:
        t = (hi - float(x)) / (hi - lo)
        t = t if t > 0 else 0.0
        t = 1.0 if t > 1 else t
        want.append(int(252 * t))
    np.testing.assert_array_equal(L.cost_of(v, lo, hi, 252), np.array(want, dtype=np.uint8))


def test_mean_is_a_sequential_fp64_sum():
    rng = np.random.default_rng(5)
    per_yaw = (rng.uniform(0, 3000, size=(64, 9, 11)) * rng.choice([1e-3, 1.0, 1e3], size=(64, 9, 11))).astype(np.float32)
    got = L.reduce_field(per_yaw, "mean")
    for j in range(9):
        for i in range(11):
            s = 0.0
            for k in range(64):
                s += float(per_yaw[k, j, i])
            assert got[j, i] == np.float32(s / 64.0)
    np.testing.assert_array_equal(L.reduce_field(per_yaw, "min"), per_yaw.min(axis=0))
    np.testing.assert_array_equal(L.reduce_field(per_yaw, "max"), per_yaw.max(axis=0))
    assert L.reduce_field(per_yaw[:1], "mean").tobytes() == per_yaw[0].tobytes()


def test_store_writes_only_writable_cells_of_scored_blocks():
    cells, _ = L.layer_map("96x80")
    win = (13, 7, 37, 21)
    a = L.anchors(cells, win, 5)
    per_yaw = L.per_yaw_field(a, np.random.default_rng(1).uniform(300, 1300, size=int((a >= 0).sum()) * 4), 4)
    out = L.layer(cells, win, 5, per_yaw, "mean", 550.0, 1100.0, 252)
    grid = out["grid"]
    changed = grid != cells
    assert out["n_changed"] == changed.sum() > 0
    outside = np.ones_like(changed)
    outside[7:28, 13:50] = False
    assert not changed[outside].any() and not changed[cells > 252].any() and (grid >= cells).all()
    assert np.isnan(out["info"][a < 0]).all() and not np.isnan(out["info"][a >= 0]).any()
    again = L.layer(grid, win, 5, per_yaw, "mean", 550.0, 1100.0, 252)
    assert again["n_changed"] == 0                                                    # idempotent: anchors of writable cells stay writable


def test_quat_zw_and_poses():
    q = L.quat_zw(8, 0.3)
    assert q.shape == (8, 2) and np.allclose((q ** 2).sum(axis=1), 1.0)
    assert np.allclose(2 * np.arctan2(q[:, 0], q[:, 1]), 0.3 + np.arange(8) * np.pi / 4)
    a = np.array([[-1, 2 * 10 + 3], [5 * 10 + 9, -1]], dtype=np.int32)
    p = L.poses(a, q, 10, (1.0, -2.0, 0.0), 0.05, 0.4)
    assert p.shape == (16, 7)
    assert np.array_equal(p[0, :3], [1.0 + 3.5 * 0.05, -2.0 + 2.5 * 0.05, 0.4]) and np.array_equal(p[8, :3], [1.0 + 9.5 * 0.05, -2.0 + 5.5 * 0.05, 0.4])
    assert np.array_equal(p[:8, 5:], q) and not p[:, 3:5].any()


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: args.count(",") + 1 for name, args in re.findall(r"\bint\s+(fs_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}, text


def test_declared_exported_bound_and_refused_without_a_context(fs):
    decl, text = _declarations()
    lib = fs.load_library()
    for name in ("fs_information_layer", "fs_multi_information_layer"):
        assert decl[name] == 12 and name in fs.capi.EXPORTED_SYMBOLS
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == 12
    for macro, value in (("FS_INFO_LAYER_MAX_STRIDE", 32), ("FS_INFO_LAYER_MAX_YAW", 64), ("FS_INFO_REDUCE_MIN", 0), ("FS_INFO_REDUCE_MEAN", 1),
                         ("FS_INFO_REDUCE_MAX", 2)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, text)
        assert m and int(m.group(1)) == getattr(fs.capi, macro) == value
    fields = re.search(r"typedef struct fs_info_layer_params \{(.*?)\} fs_info_layer_params;", text, flags=re.S).group(1)
    names = re.findall(r"\b(stride_cells|n_yaw|yaw0|pose_z|reduce|info_lo|info_hi|max_cost|write)\b", fields)
    assert names == [n for n, _ in fs.capi.InfoLayerParamsC._fields_] and C.sizeof(fs.capi.InfoLayerParamsC) == 56
    assert callable(fs.FrontierScorer.information_layer) and callable(fs.MultiScorer.information_layer)
    blob = open(fs._build.LIB, "rb").read()
    for kernel in (b"infolayer_anchor_kernel", b"infolayer_scatter_kernel", b"infolayer_records_kernel", b"infolayer_store_kernel"):
        assert kernel in blob
    p = fs.capi.InfoLayerParamsC(5, 8, 0.0, 0.0, 1, 550.0, 1100.0, 252, 1)
    assert lib.fs_information_layer(None, C.byref(p), 0, 0, 1, 1, None, None, None, None, None, None) == fs.capi.FS_E_INVALID
    assert lib.fs_multi_information_layer(None, C.byref(p), 0, 0, 1, 1, None, None, None, None, None, None) == fs.capi.FS_E_INVALID


@pytest.fixture(scope="module")
def table(oracle):
    return oracle.Table.generate()


@pytest.mark.parametrize("m", list(L.MAPS))
def test_the_oracle_alone_stays_off_the_quantisation_edges(oracle, table, m):
    """the seeds of the GPU test's oracle-bytes comparison: at most 1 % of the scored blocks lie within the 1e-4 bar of an edge"""
    cells, lm = L.layer_map(m)
    ny, nx = cells.shape
    for s, K, vis in L.EDGE_CASES:
        win = (0, 0, nx, ny)
        a = L.anchors(cells, win, s)
        v = L.oracle_values(oracle, table, lm, L.poses(a, L.quat_zw(K), nx, L.ORIGIN), vis).reshape(-1, K)
        mean = v.sum(axis=1) / K
        lo, hi = L.edge_range(mean)
        near = L.near_edge(mean, lo, hi, L.EDGE_COST)
        assert near.sum() <= 0.01 * mean.size, (s, K, near.sum(), mean.size)
        assert np.unique(L.cost_of(mean.astype(np.float32), lo, hi, L.EDGE_COST)).size >= 4      # ... and the bytes are not all one


def _route(oracle, table, grid, lm):
    w = P.waypoints(grid, L.SCENE_ORIGIN, L.RES, L.scene_pose(L.SCENE_ROBOT), L.scene_goal(), sample_distance=L.SCENE_PATH["sample_distance_m"],
                    lookahead=L.SCENE_PATH["lookahead_points"])
    xyyaw = w["xyyaw"]
    p7 = np.zeros((xyyaw.shape[0], 7))
    p7[:, :2] = xyyaw[:, :2]
    p7[:, 3:] = P.yaw_to_quat(xyyaw[:, 2])
    return w, xyyaw, L.oracle_values(oracle, table, lm, p7, L.SCENE_VIS)


def test_the_planning_scenario_on_the_cpu(oracle, table):
    """what tests/test_gpu_information_layer_planning.py asserts of the GPU, with planner_ref's NavFn, the oracle's values and the
    restatement: door A and an unsafe way point before the layer, door B, safe and longer after; every way point's value at least
    5 % away from the threshold"""
    cells, lm = L.scene()
    thr = L.SCENE_THRESHOLD
    infl = I.inflate_exact(cells, L.SCENE_INFLATION)[0]
    w0, xy0, v0 = _route(oracle, table, infl, lm)
    assert L.door_of(xy0) == "A" and (v0 <= thr).any() and v0.size >= 8
    win = (0, 0, L.SCENE_NX, L.SCENE_NY)
    s, K = L.SCENE_LAYER["stride_cells"], L.SCENE_LAYER["n_yaw"]
    a = L.anchors(infl, win, s)
    vals = L.oracle_values(oracle, table, lm, L.poses(a, L.quat_zw(K), L.SCENE_NX, L.SCENE_ORIGIN), L.SCENE_VIS)
    out = L.layer(infl, win, s, L.per_yaw_field(a, vals, K), L.SCENE_LAYER["reduce"], thr, 2.0 * thr, L.SCENE_LAYER["max_cost"])
    w1, xy1, v1 = _route(oracle, table, out["grid"], lm)
    assert L.door_of(xy1) == "B" and (v1 > thr).all() and w1["path_length"][0] > w0["path_length"][0] * 1.5
    assert np.abs(np.concatenate([v0, v1]) / thr - 1.0).min() >= 0.05
    # the same decision one threshold step either way: the scenario does not sit on a knife's edge
    for other in (550.0, 650.0):
        o = L.layer(infl, win, s, L.per_yaw_field(a, vals, K), "mean", other, 2.0 * other, 252)
        assert L.door_of(_route(oracle, table, o["grid"], lm)[1]) == "B"
