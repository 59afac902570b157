"""Loader of tests/thetastar_ref/thetastar_ref.cpp, the CPU restatement of the any-angle leg refinement: the
`field` leg (the definition the GPU is held to bit for bit) and the `reference` leg (the reference's Theta* search as it runs).
Compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use.

`vertices` lists every vertex of a leg once, start first.  The reference's generatePath returns one entry more: its backtrace pushes
the last vertex (the goal) twice, and linearInterpolation runs over that list — which is why the interpolated poses end with the goal
itself.  `poses` is computed from the list with the repeated goal, so it equals the reference's poses as they are; the reference's raw
path is `vertices` plus `vertices[-1]` once more (tests/test_reference_built.py holds both to the reference's compiled Theta*)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "thetastar_ref", "thetastar_ref.cpp")
DBL_MAX = np.finfo(np.float64).max
FIELD, REFERENCE = 0, 1
OK, START_OFF_MAP, GOAL_OFF_MAP, START_UNSAFE, GOAL_UNSAFE, NO_PATH = 0, 1, 2, 3, 4, 5
MOVES = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, -1), (-1, 1), (1, 1), (-1, -1))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="thetastar_ref_"), "libthetastar_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.tr_field.argtypes = [vp, ci, ci, ci, ci, ci, cd, cd, ci, vp]
        L.tr_leg.argtypes = [vp, ci, ci, cd, cd, cd, vp, vp, ci, cd, cd, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp]
        L.tr_los.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cells2d(cells):
    c = np.ascontiguousarray(cells, dtype=np.uint8)
    return c[0] if c.ndim == 3 else c


def field(cells, sx, sy, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8):
    """The fp64 field [ny][nx] from start cell (sx, sy); DBL_MAX where not reached."""
    c = _cells2d(cells)
    ny, nx = c.shape
    out = np.zeros((ny, nx))
    assert lib().tr_field(_p(c), nx, ny, int(sx), int(sy), 1 if allow_unknown else 0, float(w_euc), float(w_traversal), int(corners), _p(out)) == 0
    return out


def leg(cells, origin, resolution, start_xy, goal_xy, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8, which=FIELD):
    """One leg: dict(status, cost, vertices [V][2], poses [N][2], los_walks, chain, quirk)."""
    c = _cells2d(cells)
    ny, nx = c.shape
    s = np.ascontiguousarray(start_xy, dtype=np.float64)[:2].copy()
    g = np.ascontiguousarray(goal_xy, dtype=np.float64)[:2].copy()
    st, nv, npz = C.c_int(), C.c_int(), C.c_int()
    cost = C.c_double()
    stats = np.zeros(3, dtype=np.int64)
    vcap, pcap = 64, 1024
    while True:
        v = np.zeros((vcap, 2)); p = np.zeros((pcap, 2))
        lib().tr_leg(_p(c), nx, ny, float(origin[0]), float(origin[1]), float(resolution), _p(s), _p(g), 1 if allow_unknown else 0,
                     float(w_euc), float(w_traversal), int(corners), int(which), C.byref(st), C.byref(cost), C.byref(nv), _p(v), vcap,
                     C.byref(npz), _p(p), pcap, _p(stats))
        if nv.value <= vcap and npz.value <= pcap:
            break
        vcap, pcap = max(vcap, nv.value), max(pcap, npz.value)
    return dict(status=st.value, cost=cost.value, vertices=v[:nv.value].copy(), poses=p[:npz.value].copy(),
                los_walks=int(stats[0]), chain=int(stats[1]), quirk=bool(stats[2]))


def legs(cells, origin, resolution, starts, goals, which=FIELD, **kw):
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 2)
    return [leg(cells, origin, resolution, s, g, which=which, **kw) for s, g in zip(starts, goals)]


def los(cells, x0, y0, x1, y1, allow_unknown=True):
    """(integer sum or None, reference left-fold sum or None) of the line-of-sight walk from (x0, y0) to (x1, y1), w = 1."""
    c = _cells2d(cells)
    ny, nx = c.shape
    s = C.c_int64()
    r = C.c_double()
    bits = lib().tr_los(_p(c), nx, ny, 1 if allow_unknown else 0, int(x0), int(y0), int(x1), int(y1), C.byref(s), C.byref(r))
    return (s.value if bits & 1 else None), (r.value if bits & 2 else None)


def bellman_ford(cells, sx, sy, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8):
    """The field by synchronous numpy relaxation to the fixed point (an independent schedule)."""
    c = _cells2d(cells).astype(np.int64)
    ny, nx = c.shape
    safe = (c < 254) | ((c == 255) & bool(allow_unknown))
    cc = 26 + 0.9 * c.astype(np.float64)
    trav = w_traversal * cc * cc / 254 / 254
    g = np.full((ny, nx), DBL_MAX)
    if not safe[sy, sx]:
        return g
    g[sy, sx] = trav[sy, sx]
    fixed = np.zeros((ny, nx), dtype=bool)
    fixed[sy, sx] = True
    while True:
        best = g.copy()
        for dx, dy in MOVES[:corners]:
            e = w_euc * np.sqrt(float(dx * dx + dy * dy))
            # u = v + (dx, dy)
            sh = np.full((ny, nx), DBL_MAX)
            ys, ye = max(0, -dy), ny - max(0, dy)
            xs, xe = max(0, -dx), nx - max(0, dx)
            sh[ys:ye, xs:xe] = g[ys + dy:ye + dy, xs + dx:xe + dx]
            with np.errstate(over="ignore"):
                cand = (sh + e) + trav
            cand[sh >= DBL_MAX] = DBL_MAX
            best = np.minimum(best, cand)
        best[~safe | fixed] = g[~safe | fixed]
        if np.array_equal(best, g):
            return g
        g = best


def cell_centre(origin, resolution, x, y):
    return (origin[0] + (x + 0.5) * resolution, origin[1] + (y + 0.5) * resolution)
