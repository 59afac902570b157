"""The leg refinement's definition on the CPU: known answers of tests/thetastar_ref/thetastar_ref.cpp's `field`
leg, its field against an independent numpy relaxation bit for bit, the chain invariant G(goal) <= g(goal), agreement with the
`reference` leg (the reference's Theta* search) on achievability apart from the flagged loop quirk, the integer line-of-sight sums
against the reference's left fold, and the C ABI's new entry points (exported; no device, no result)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import thetastar_ref as T

fsmod = importlib.import_module("fit-slam_amd")
ORIGIN = (-1.0, -2.0)
RES = 0.05


def _c(x, y):
    return T.cell_centre(ORIGIN, RES, x, y)


def _cells(v):
    return np.round((np.asarray(v) - np.asarray(ORIGIN)) / RES - 0.5).astype(int)


def _corners(v):
    """the vertices with collinear runs merged: start, every real turn, goal"""
    v = _cells(v)
    out = [v[0]]
    for i in range(1, len(v) - 1):
        a, b = v[i] - out[-1], v[i + 1] - v[i]
        if a[0] * b[1] - a[1] * b[0] != 0:
            out.append(v[i])
    out.append(v[-1])
    return np.array(out)


def _trav(raw, w=2.0):
    c = 26 + 0.9 * raw
    return w * c * c / 254 / 254


def test_open_field_is_a_single_segment():
    c = np.zeros((30, 30), np.uint8)
    for s, g in (((5, 5), (5, 25)), ((1, 1), (28, 28)), ((3, 20), (25, 20)), ((27, 2), (2, 27))):
        leg = T.leg(c, ORIGIN, RES, _c(*s), _c(*g))
        assert leg["status"] == T.OK
        assert _corners(leg["vertices"]).tolist() == [list(s), list(g)], (s, g)


def test_l_corridor_turns_once_at_the_corner():
    c = np.full((30, 30), 254, np.uint8)
    c[3, 3:21] = 0                      # one cell wide: along y = 3, then up x = 20
    c[3:26, 20] = 0
    leg = T.leg(c, ORIGIN, RES, _c(3, 3), _c(20, 25))
    assert leg["status"] == T.OK
    k = _corners(leg["vertices"])
    assert k[0].tolist() == [3, 3] and k[-1].tolist() == [20, 25]
    inner = k[1:-1]
    assert len(inner) >= 1 and all(x >= 17 and y <= 5 for x, y in inner), inner.tolist()
    # the reference's loop drains its queue in a one-cell corridor: the quirk, flagged
    ref = T.leg(c, ORIGIN, RES, _c(3, 3), _c(20, 25), which=T.REFERENCE)
    assert ref["status"] == T.NO_PATH and ref["quirk"]


def test_walled_off_goal_is_unreachable():
    c = np.zeros((30, 30), np.uint8)
    c[10:20, 10] = c[10:20, 19] = 254
    c[10, 10:20] = c[19, 10:20] = 254
    for which in (T.FIELD, T.REFERENCE):
        leg = T.leg(c, ORIGIN, RES, _c(2, 2), _c(15, 15), which=which)
        assert leg["status"] == T.NO_PATH and leg["cost"] == T.DBL_MAX and len(leg["poses"]) == 0
    g = T.field(c, 2, 2)
    assert g[15, 15] == T.DBL_MAX and g[12:18, 12:18].max() == T.DBL_MAX


def test_start_equal_to_goal():
    c = np.zeros((20, 20), np.uint8)
    c[7, 7] = 40
    for which in (T.FIELD, T.REFERENCE):
        leg = T.leg(c, ORIGIN, RES, _c(7, 7), _c(7, 7), which=which)
        assert leg["status"] == T.OK
        assert leg["cost"] == _trav(40)
        assert len(leg["vertices"]) == 1 and len(leg["poses"]) == 1
        assert tuple(leg["poses"][0]) == _c(7, 7)


def test_unknown_cells_with_allow_unknown_on_and_off():
    c = np.zeros((20, 40), np.uint8)
    c[:, 15:25] = 255                  # an unknown band across the map
    on = T.leg(c, ORIGIN, RES, _c(3, 10), _c(35, 10), allow_unknown=True)
    off = T.leg(c, ORIGIN, RES, _c(3, 10), _c(35, 10), allow_unknown=False)
    assert on["status"] == T.OK and off["status"] == T.NO_PATH
    # a path-1 step into an unknown cell costs getCost(255) = 255.5; the field says so
    g = T.field(c, 3, 10, allow_unknown=True)
    assert g[10, 15] == (g[10, 14] + 1.0) + _trav(255)
    assert T.leg(c, ORIGIN, RES, _c(20, 10), _c(3, 10), allow_unknown=False)["status"] == T.START_UNSAFE
    assert T.leg(c, ORIGIN, RES, _c(3, 10), _c(20, 10), allow_unknown=False)["status"] == T.GOAL_UNSAFE
    # an unknown cell on a line of sight adds 25300^2 (the three-argument isSafe's OBS_COST - 1)
    s, _ = T.los(c, 14, 3, 16, 3)
    assert s == 2600 ** 2 + 25300 ** 2
    assert T.los(c, 14, 3, 16, 3, allow_unknown=False) == (None, None)


def test_four_against_eight_corners():
    c = np.zeros((16, 16), np.uint8)
    g8, g4 = T.field(c, 8, 8, corners=8), T.field(c, 8, 8, corners=4)
    t = _trav(0)
    assert g8[9, 9] == (g8[8, 8] + np.sqrt(2.0)) + t
    assert g4[9, 9] == (g4[8, 9] + 1.0) + t and g4[8, 9] == (g4[8, 8] + 1.0) + t
    assert (g4 >= g8).all() and (g4 > g8).any()
    l4 = T.leg(c, ORIGIN, RES, _c(1, 1), _c(12, 6), corners=4)
    l8 = T.leg(c, ORIGIN, RES, _c(1, 1), _c(12, 6), corners=8)
    assert l4["status"] == l8["status"] == T.OK
    assert l4["cost"] != l8["cost"]
    # the wall's corner: 8 moves cut it, 4 moves go round
    c[5, :10] = 254
    g8, g4 = T.field(c, 3, 3, corners=8), T.field(c, 3, 3, corners=4)
    assert g8[6, 10] < g4[6, 10] < T.DBL_MAX


def _min_wall_distance(poses, wall_cells):
    p = _cells(poses)
    d = np.abs(p[:, None, :] - wall_cells[None, :, :]).max(axis=2)
    return d.min(axis=1)


def test_inflation_gradient_bends_path_away_from_walls():
    ny, nx = 40, 60
    plain = np.zeros((ny, nx), np.uint8)
    plain[12:28, 25:35] = 254          # a block in the middle
    wall = np.argwhere(plain == 254)[:, ::-1]
    inflated = plain.copy()
    yy, xx = np.mgrid[0:ny, 0:nx]
    dist = np.full((ny, nx), 99)
    for x, y in wall:
        dist = np.minimum(dist, np.maximum(np.abs(xx - x), np.abs(yy - y)))
    band = (dist >= 1) & (dist <= 12)
    inflated[band] = np.clip(252 - (dist[band] - 1) * 23, 1, 252).astype(np.uint8)   # 252 next to the wall down to 1
    s, g = _c(5, 20), _c(55, 20)
    a = T.leg(plain, ORIGIN, RES, s, g)
    b = T.leg(inflated, ORIGIN, RES, s, g)
    assert a["status"] == b["status"] == T.OK
    da, db = _min_wall_distance(a["poses"], wall), _min_wall_distance(b["poses"], wall)
    assert db.min() > da.min(), (da.min(), db.min())
    assert np.median(db) > np.median(da)


def _maps():
    rng = np.random.Generator(np.random.PCG64(5150))
    out = [fsmod.synth.make_grid(rng, n, 1)[0] for n in (40, 64, 72)]
    out.append(fsmod.synth.make_grid(rng, 80, 1)[0][:50, :])
    return out


@pytest.mark.parametrize("k", range(4))
def test_field_equals_bellman_ford_bit_for_bit(k):
    c = _maps()[k]
    rng = np.random.default_rng(k)
    ys, xs = np.nonzero(c < 254)
    for j in rng.choice(xs.size, 3, replace=False):
        for allow in (True, False):
            for corners in (4, 8):
                for w in ((1.0, 2.0), (0.7, 5.0)):
                    a = T.field(c, xs[j], ys[j], allow_unknown=allow, w_euc=w[0], w_traversal=w[1], corners=corners)
                    b = T.bellman_ford(c, xs[j], ys[j], allow_unknown=allow, w_euc=w[0], w_traversal=w[1], corners=corners)
                    assert a.tobytes() == b.tobytes(), (k, j, allow, corners, w)


def _legs(c, rng, n):
    ys, xs = np.nonzero(c < 254)
    i = rng.choice(xs.size, 2 * n)
    ox, oy = ORIGIN
    p = np.stack([ox + (xs[i] + rng.uniform(0, 1, 2 * n)) * RES, oy + (ys[i] + rng.uniform(0, 1, 2 * n)) * RES], axis=1)
    return p[:n], p[n:]


def test_chain_cost_never_exceeds_field_and_agrees_with_reference_on_achievability():
    """G(goal) <= g(goal) on every leg; the field leg and the reference's search find a path on the same legs, apart from the
    reference's loop quirk (a goal, or the node that leads to it, popped as the last entry of the queue)."""
    quirks = legs = 0
    for k, c in enumerate(_maps()):
        rng = np.random.default_rng(100 + k)
        starts, goals = _legs(c, rng, 25)
        for s, g in zip(starts, goals):
            f = T.leg(c, ORIGIN, RES, s, g)
            r = T.leg(c, ORIGIN, RES, s, g, which=T.REFERENCE)
            legs += 1
            if f["status"] == T.OK:
                sx, sy = _cells(s)
                gx, gy = _cells(g)
                field = T.field(c, sx, sy)
                assert f["cost"] <= field[gy, gx]
                assert f["vertices"][0].tolist() == list(_c(sx, sy)) and f["vertices"][-1].tolist() == list(_c(gx, gy))
            if (f["status"] == T.OK) != (r["status"] == T.OK):
                assert f["status"] == T.OK and r["quirk"], (k, s, g, f["status"], r["status"])
                quirks += 1
            else:
                assert f["status"] == r["status"]
    assert legs == 100 and quirks < legs // 4


def _interp(vertices, res):
    """ThetaStar::backtrace (the goal pushed twice) + linearInterpolation, in numpy with the sqrt form of the distance"""
    raw = np.vstack([vertices, vertices[-1:]])
    out = []
    for j in range(len(raw) - 1):
        (x1, y1), (x2, y2) = raw[j], raw[j + 1]
        out.append((x1, y1))
        ex, ey = x2 - x1, y2 - y1
        dist = np.sqrt(ex * ex + ey * ey)
        loops = int(dist / res)
        with np.errstate(invalid="ignore"):
            sa, ca = ey / dist, ex / dist
        for k in range(1, loops):
            out.append((x1 + k * res * ca, y1 + k * res * sa))
    return np.array(out)


def test_backtrace_and_interpolation_known_answer():
    c = np.zeros((30, 30), np.uint8)
    leg = T.leg(c, ORIGIN, RES, _c(2, 4), _c(22, 4))
    v, p = leg["vertices"], leg["poses"]
    # the goal pushed twice by backtrace: its own segment has length 0 and contributes the goal once, last
    assert tuple(p[-1]) == _c(22, 4) and tuple(p[0]) == _c(2, 4)
    assert (np.abs(p[:-1] - p[-1]).max(axis=1) > 0).all()
    seg = np.diff(v, axis=0)
    loops = [int(np.sqrt(ex * ex + ey * ey) / RES) for ex, ey in seg]
    assert len(p) == sum(max(1, L) for L in loops) + 1
    assert p.tobytes() == _interp(v, RES).tobytes()
    # each segment's last point is dropped: no vertex but the start and the goal is a pose unless the step lands on it
    for c2 in (_maps()[1], _maps()[3]):
        rng = np.random.default_rng(9)
        for s, g in zip(*_legs(c2, rng, 6)):
            f = T.leg(c2, ORIGIN, RES, s, g)
            if f["status"] == T.OK:
                assert f["poses"].tobytes() == _interp(f["vertices"], RES).tobytes()


def test_integer_line_of_sight_sums_against_the_reference_fold():
    rng = np.random.default_rng(77)
    c = rng.integers(0, 253, size=(64, 64)).astype(np.uint8)
    c[rng.random((64, 64)) < 0.05] = 255
    worst = 0.0
    for _ in range(400):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(0, 64, 4))
        s, r = T.los(c, x0, y0, x1, y1)
        assert (s is None) == (r is None)
        if s is not None and s:
            v = 1.0 * s / (1e4 * 254 * 254)
            worst = max(worst, abs(v - r) / r)
    assert worst < 1e-13, worst


def test_library_exports_refine_and_refuses_without_device():
    """fs_refine_paths / fs_refine_field are exported and declared; with no context (and so with no device) they compute nothing."""
    lib = fsmod.load_library()
    assert "fs_refine_paths" in fsmod.capi.EXPORTED_SYMBOLS and "fs_refine_field" in fsmod.capi.EXPORTED_SYMBOLS
    assert hasattr(lib, "fs_refine_paths") and hasattr(lib, "fs_refine_field")
    st = np.zeros(1, np.int32)
    assert lib.fs_refine_paths(None, 1, None, None, 1, 1.0, 2.0, 8, None, None, None, None, None, None) == fsmod.capi.FS_E_INVALID
    start = (C.c_double * 2)(0.0, 0.0)
    assert lib.fs_refine_field(None, C.byref(start), 1, 1.0, 2.0, 8, st.ctypes.data_as(C.c_void_p)) == fsmod.capi.FS_E_INVALID
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(fsmod.FsError) as e:
            fsmod.FrontierScorer(device=0)
        assert e.value.code == fsmod.capi.FS_E_NO_DEVICE
