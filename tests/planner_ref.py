"""Loader of tests/navfn_ref/navfn_ref.cpp, the CPU restatement of the batched grid planner, and the maps its
tests share.  The restatement is compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "navfn_ref", "navfn_ref.cpp")
POT_HIGH = np.float32(1.0e10)
DBL_MAX = np.finfo(np.float64).max
CONVERGED, REFERENCE_ASTAR = 0, 1
NAVFN_TILE = 32
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="navfn_ref_"), "libnavfn_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.nr_converged_field.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]
        L.nr_costs.argtypes = [vp, ci, ci, ci, vp]
        L.nr_plan.argtypes = [vp, ci, ci, cd, cd, cd, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.nr_plan_points.argtypes = L.nr_plan.argtypes + [vp, vp, ci]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cells2d(cells):
    c = np.ascontiguousarray(cells, dtype=np.uint8)
    return c[0] if c.ndim == 3 else c


def converged_field(cells, rx, ry, allow_unknown=False):
    """(potential [ny][nx] float32, stats {rounds, tile_runs, sweeps, max_sweeps}) of the converged leg."""
    c = _cells2d(cells)
    ny, nx = c.shape
    pot = np.zeros((ny, nx), dtype=np.float32)
    st = np.zeros(4, dtype=np.int64)
    assert lib().nr_converged_field(_p(c), nx, ny, int(rx), int(ry), 1 if allow_unknown else 0, _p(pot), _p(st)) == 0
    return pot, dict(zip(("rounds", "tile_runs", "sweeps", "max_sweeps"), (int(v) for v in st)))


def costs(cells, allow_unknown=False):
    c = _cells2d(cells)
    ny, nx = c.shape
    out = np.zeros((ny, nx), dtype=np.uint8)
    lib().nr_costs(_p(c), nx, ny, 1 if allow_unknown else 0, _p(out))
    return out


def plan(cells, origin, resolution, robot_pose7, goal_xyz, achievable_in=None, allow_unknown=False, leg=CONVERGED, points=False):
    """The four columns of fs_plan_paths from one leg; leg REFERENCE_ASTAR also returns `limit` (bit 0 cycles, bit 1 buffer cap).
    points: also `pathx` / `pathy`, per goal the float32 path points as calcPath left them (empty where not achievable)."""
    c = _cells2d(cells)
    ny, nx = c.shape
    goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
    n = goal.shape[0]
    pose = np.ascontiguousarray(robot_pose7, dtype=np.float64).reshape(7)
    ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
    pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
    ach = np.zeros(n, dtype=np.uint8)
    lim = np.zeros(n, dtype=np.int32)
    args = (_p(c), nx, ny, float(origin[0]), float(origin[1]), float(resolution), _p(pose), 1 if allow_unknown else 0, int(leg), n,
            _p(goal), _p(ai), _p(pl), _p(plm), _p(ph), _p(ach), _p(lim))
    out = dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach, limit=lim)
    if not points:
        lib().nr_plan(*args)
        return out
    stride = 4 * max(nx, ny)
    px, py = np.zeros((n, stride), dtype=np.float32), np.zeros((n, stride), dtype=np.float32)
    assert lib().nr_plan_points(*args, _p(px), _p(py), stride) == 0
    lens = [int(pl[i]) if ach[i] else 0 for i in range(n)]
    out.update(pathx=[px[i, :k].copy() for i, k in enumerate(lens)], pathy=[py[i, :k].copy() for i, k in enumerate(lens)])
    return out


def cell_centre(origin, resolution, x, y):
    return (origin[0] + (x + 0.5) * resolution, origin[1] + (y + 0.5) * resolution)


def robot_pose(origin, resolution, x, y, yaw=0.0):
    wx, wy = cell_centre(origin, resolution, x, y)
    return np.array([wx, wy, 0.0, 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])


def spiral_map(n=256, gap=6, wall=2):
    """A square spiral corridor: free cells (0) between lethal walls (254); the wave from the centre crosses many tiles.
    Returns (cells [n][n], centre (x, y), outer end (x, y))."""
    c = np.zeros((n, n), dtype=np.uint8)
    lo, hi = 0, n - 1
    k = 0
    # concentric square rings of wall, each with one opening, alternating sides, so that the free space is one long corridor
    while hi - lo > 2 * (gap + wall):
        c[lo:lo + wall, lo:hi + 1] = 254
        c[hi - wall + 1:hi + 1, lo:hi + 1] = 254
        c[lo:hi + 1, lo:lo + wall] = 254
        c[lo:hi + 1, hi - wall + 1:hi + 1] = 254
        if k:                                       # the opening of this ring (the outermost ring stays closed)
            if k % 2:
                c[lo:lo + wall, lo + wall:lo + wall + gap] = 0
            else:
                c[hi - wall + 1:hi + 1, hi - wall - gap + 1:hi - wall + 1] = 0
        lo += wall + gap
        hi -= wall + gap
        k += 1
    mid = n // 2
    return c, (mid, mid), (wall + gap // 2, wall + gap // 2)


def free_cells(cells2d, rng, k, value=0):
    ys, xs = np.nonzero(_cells2d(cells2d) == value)
    idx = rng.choice(xs.size, size=k, replace=xs.size < k)
    return xs[idx], ys[idx]


def well_placed_robot(cells2d, rng, k=6):
    """Of k free cells drawn, the one whose field reaches the most cells (a robot that is not shut in a small room)."""
    c = _cells2d(cells2d)
    xs, ys = free_cells(c, rng, k)
    reach = [int((converged_field(c, x, y)[0] < POT_HIGH).sum()) for x, y in zip(xs, ys)]
    i = int(np.argmax(reach))
    return int(xs[i]), int(ys[i])
