"""Loader of tests/thetastar_search_ref/thetastar_search_ref.cpp, the host driver of fit-slam_amd/csrc/fs_thetastar.h (the REFERENCE
refine search), and the small known maps its CPU and GPU tests share.  Compiled by g++ -O2 -ffp-contract=off into a
temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "thetastar_search_ref", "thetastar_search_ref.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fit-slam_amd", "csrc")
OK, START_OFF_MAP, GOAL_OFF_MAP, START_UNSAFE, GOAL_UNSAFE, NO_PATH = 0, 1, 2, 3, 4, 5
RES = 0.05
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="thetastar_search_ref_"), "libthetastar_search_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.ts_leg.argtypes = [vp, ci, ci, cd, cd, cd, vp, vp, ci, cd, cd, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp]
        L.ts_heap_trace.argtypes = [ci, vp, vp, vp, vp, vp]
        L.ts_table_check.argtypes = [ci, ci]
        L.ts_table_check.restype = C.c_int64
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cells2d(cells):
    c = np.ascontiguousarray(cells, dtype=np.uint8)
    return c[0] if c.ndim == 3 else c


def leg(cells, origin, resolution, start_xy, goal_xy, allow_unknown=True, w_euc=1.0, w_traversal=2.0, corners=8):
    """One leg through the header's search: dict(status, cost, vertices [V][2] (each once, start first), poses [N][2], pops,
    los_walks, max_heap, records)."""
    c = _cells2d(cells)
    ny, nx = c.shape
    s = np.ascontiguousarray(start_xy, dtype=np.float64).reshape(-1)[:2].copy()
    g = np.ascontiguousarray(goal_xy, dtype=np.float64).reshape(-1)[:2].copy()
    st, nv, npz = C.c_int(), C.c_int(), C.c_int()
    cost = C.c_double()
    stats = np.zeros(4, dtype=np.int64)
    vcap, pcap = 64, 1024
    while True:
        v = np.zeros((vcap, 2)); p = np.zeros((pcap, 2))
        lib().ts_leg(_p(c), nx, ny, float(origin[0]), float(origin[1]), float(resolution), _p(s), _p(g), 1 if allow_unknown else 0,
                     float(w_euc), float(w_traversal), int(corners), C.byref(st), C.byref(cost), C.byref(nv), _p(v), vcap,
                     C.byref(npz), _p(p), pcap, _p(stats))
        if nv.value <= vcap and npz.value <= pcap:
            break
        vcap, pcap = max(vcap, nv.value), max(pcap, npz.value)
    return dict(status=st.value, cost=cost.value, vertices=v[:nv.value].copy(), poses=p[:npz.value].copy(), pops=int(stats[0]),
                los_walks=int(stats[1]), max_heap=int(stats[2]), records=int(stats[3]))


def heap_trace(ops, arg, val):
    """(pops, header's pop order, std::priority_queue's pop order) of one sequence; pops < 0: they parted at pop -pops"""
    ops = np.ascontiguousarray(ops, dtype=np.int32); arg = np.ascontiguousarray(arg, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    got = np.full(ops.size, -1, dtype=np.int32); want = np.full(ops.size, -2, dtype=np.int32)
    n = lib().ts_heap_trace(int(ops.size), _p(ops), _p(arg), _p(val), _p(got), _p(want))
    return n, got[:abs(n)], want[:abs(n)]


def table_mismatches(nx, ny):
    return int(lib().ts_table_check(int(nx), int(ny)))


def centre(origin, x, y):
    return (origin[0] + (x + 0.5) * RES, origin[1] + (y + 0.5) * RES)


# ------------------------------------------------------------------ the small known maps (a one-cell lethal border on each: no
# line-of-sight walk reads a cell off the map)
def _bordered(nx, ny, fill=0):
    c = np.full((ny, nx), fill, dtype=np.uint8)
    c[0, :] = c[-1, :] = 254
    c[:, 0] = c[:, -1] = 254
    return c


ORIGIN = (-0.6, -0.4, 0.0)


def corridor_map():
    """24 x 16, walls everywhere but a one-cell corridor along row 8 from x = 2 to x = 21: (cells, start cell, goal cell)"""
    c = _bordered(24, 16, 254)
    c[8, 2:22] = 0
    return c, (2, 8), (21, 8)


def strip253_map():
    """24 x 16 free floor with a column of cost 253 at x = 12 from wall to wall: a neighbour may step on it (raw < 254) and a
    line of sight may cross it as well (getCost = 26 + 0.9 * 253 = 253.7 < 254), at the price of (253.7 / 254)^2 w per cell"""
    c = _bordered(24, 16, 0)
    c[1:-1, 12] = 253
    return c, (3, 4), (20, 11)


def unknown_map():
    """24 x 16 with a wall at x = 12 whose only gap (rows 6-9) is unknown: passable with allow_unknown, closed without"""
    c = _bordered(24, 16, 0)
    c[1:-1, 12] = 254
    c[6:10, 11:14] = 255
    return c, (3, 3), (20, 12)


def walled_map():
    """24 x 16 with the goal inside a closed box"""
    c = _bordered(24, 16, 0)
    c[4:11, 14] = c[4:11, 20] = 254
    c[4, 14:21] = c[10, 14:21] = 254
    return c, (3, 8), (17, 7)


def open_map():
    c = _bordered(20, 12, 0)
    c[3:9, 9] = 254
    return c, (4, 6), (15, 5)


def serpentine_map(n=64):
    """n x n: lanes three cells wide that double back at alternate ends — a path of some hundred vertices (the reference's search
    rarely takes a long line of sight along a uniform lane): (cells, start cell, goal cell)"""
    c = _bordered(n, n, 0)
    for k, y in enumerate(range(4, n - 1, 4)):
        c[y, :] = 254
        if k % 2 == 0:
            c[y, n - 4:n - 1] = 0
        else:
            c[y, 1:4] = 0
    last = max(y for y in range(1, n - 1) if c[y, 2] == 0)
    return c, (2, 2), (n // 2, last)


def generated_map(nx, ny, seed):
    """random blocks, an inflation gradient around them, an unknown patch, a one-cell lethal border (and, from 96 cells a side on,
    a free lane along one wall)"""
    rng = np.random.default_rng(seed)
    wall = np.zeros((ny, nx), dtype=bool)
    for _ in range(max(6, nx * ny // 400)):
        w, h = rng.integers(2, 9), rng.integers(2, 9)
        x, y = rng.integers(1, nx - w), rng.integers(1, ny - h)
        wall[y:y + h, x:x + w] = True
    wall[0, :] = wall[-1, :] = wall[:, 0] = wall[:, -1] = True
    # distance to the nearest wall cell by growing the wall mask: cost 220 next to a wall, fading over four cells
    c = np.zeros((ny, nx), dtype=np.uint8)
    grown = wall.copy()
    for level in (220, 150, 80, 30):
        nxt = grown.copy()
        nxt[1:, :] |= grown[:-1, :]; nxt[:-1, :] |= grown[1:, :]
        nxt[:, 1:] |= grown[:, :-1]; nxt[:, :-1] |= grown[:, 1:]
        c[nxt & ~grown] = level
        grown = nxt
    c[wall] = 254
    if nx >= 96:
        c[2:5, 2:nx - 2] = 0               # a free lane three cells wide under the top wall: lines of sight longer than 64 cells
    ux, uy = rng.integers(2, nx - 12), rng.integers(2, ny - 12)
    patch = c[uy:uy + 9, ux:ux + 9]
    patch[patch < 254] = 255
    c[0, :] = c[-1, :] = 254
    c[:, 0] = c[:, -1] = 254
    return np.ascontiguousarray(c)


def map_origin(cells):
    return (-cells.shape[1] * RES / 2, -cells.shape[0] * RES / 2, 0.0)


def lane_legs(cells, origin):
    """legs along the free lane of a map 96 cells wide or wider: a straight walk, a shallow one each way, and one that leaves it"""
    nx = cells.shape[1]
    pairs = [((2, 3), (nx - 3, 3)), ((3, 2), (nx - 4, 4)), ((nx - 3, 4), (2, 2)), ((nx - 3, 2), (10, 3))]
    return np.array([centre(origin, *a) for a, _ in pairs]), np.array([centre(origin, *b) for _, b in pairs])


GENERATED = (("gen_64x48", 64, 48, 11), ("gen_48x64", 48, 64, 12), ("gen_96x96", 96, 96, 13))
