"""Loader of tests/roadmap_ref/roadmap_ref.cpp, the CPU restatement of the frontier roadmap, and the roadmap its
tests grow.  The restatement is compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use and linked against the
oracle's libfso_oracle.so, whose single-ray trace is its isConnectable."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "roadmap_ref", "roadmap_ref.cpp")
DBL_MAX = np.finfo(np.float64).max
TREE, REFERENCE_ASTAR = 0, 1
FS_E_RANGE = -6
_lib = None


def lib():
    global _lib
    if _lib is None:
        if os.path.join(ROOT, "oracle") not in sys.path:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        so = O.build()
        out = os.path.join(tempfile.mkdtemp(prefix="roadmap_ref_"), "libroadmap_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC, so,
                        "-Wl,-rpath," + os.path.dirname(os.path.abspath(so))], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.rr_create.argtypes = [cd, cd, cd, cd]
        L.rr_create.restype = vp
        L.rr_destroy.argtypes = [vp]
        L.rr_destroy.restype = None
        L.rr_populate.argtypes = [vp, ci, vp, ci]
        L.rr_rebuild.argtypes = [vp, vp, ci, ci, cd, cd, cd, cd]
        L.rr_connect.argtypes = [vp, vp, ci, ci, cd, cd, cd, cd, ci, vp]
        L.rr_graph.argtypes = [vp, C.POINTER(ci), C.POINTER(C.c_longlong), vp, vp, vp, vp]
        L.rr_graph.restype = None
        L.rr_closest.argtypes = [vp, cd, cd, ci]
        L.rr_tree.argtypes = [vp, ci, vp, vp, vp]
        L.rr_plan.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _xy(a):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1])[:, :2])


class Roadmap:
    """One restated FrontierRoadMap over a 2-D grid (cells [ny][nx], origin (x, y, z), resolution)."""

    def __init__(self, cells, origin, resolution, grid_cell_size=1.0, radius=6.1, min_frontier=0.25, min_robot=0.25):
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        self.cells = c[0] if c.ndim == 3 else c
        self.origin = tuple(float(v) for v in origin) + (0.0,) * (3 - len(origin))
        self.res = float(resolution)
        self._h = lib().rr_create(grid_cell_size, radius, min_frontier, min_robot)

    def close(self):
        if self._h:
            lib().rr_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _grid(self):
        ny, nx = self.cells.shape
        return (_p(self.cells), nx, ny, self.origin[0], self.origin[1], self.origin[2], self.res)

    def populate(self, xy, is_robot_pose=False):
        p = _xy(xy)
        return lib().rr_populate(self._h, p.shape[0], _p(p), 1 if is_robot_pose else 0)

    def rebuild(self):
        lib().rr_rebuild(self._h, *self._grid())

    def connect(self, xy):
        p = _xy(xy)
        lib().rr_connect(self._h, *self._grid(), p.shape[0], _p(p))

    def graph(self):
        n, e = C.c_int(), C.c_longlong()
        lib().rr_graph(self._h, C.byref(n), C.byref(e), None, None, None, None)
        xy = np.zeros((n.value, 2)); key = np.zeros(n.value, np.uint8)
        row = np.zeros(n.value + 1, np.int32); col = np.zeros(max(e.value, 1), np.int32)
        lib().rr_graph(self._h, C.byref(n), C.byref(e), _p(xy), _p(key), _p(row), _p(col))
        return dict(xy=xy, key=key, row_ptr=row, col=col[:e.value])

    def closest(self, x, y, key_only=True):
        return lib().rr_closest(self._h, float(x), float(y), 1 if key_only else 0)

    def tree(self, root):
        n = self.graph()["xy"].shape[0]
        d = np.zeros(n); hops = np.zeros(n, np.int32); pred = np.zeros(n, np.int32)
        rounds = lib().rr_tree(self._h, int(root), _p(d), _p(hops), _p(pred))
        return dict(d=d, hops=hops, pred=pred, rounds=rounds)

    def plan(self, robot_pose7, goal_xyz, achievable_in=None, leg=TREE):
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        pose = np.ascontiguousarray(robot_pose7, dtype=np.float64).reshape(7)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        pl, plm, ph = np.zeros(n), np.zeros(n), np.zeros(n)
        ach = np.zeros(n, dtype=np.uint8)
        assert lib().rr_plan(self._h, _p(pose), n, _p(goal), _p(ai), int(leg), _p(pl), _p(plm), _p(ph), _p(ach)) == 0
        return dict(path_length=pl, path_length_m=plm, path_heading=ph, achievable=ach)


def pose7(x, y, yaw=0.0):
    return np.array([x, y, 0.0, 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])


def grow_ticks(fsmod, cells, origin, res, robot_cells, max_frontier_distance=25.1):
    """The node lists of a roadmap grown the way UpdateRoadmapBT grows it, one entry per simulated tick: (frontier goal points of
    fs_frontier_clusters' clusters from the robot, the robot pose xy).  Needs a GPU (the clusters come from the device)."""
    sc = fsmod.FrontierScorer(device=0)
    try:
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        sc.upload_grid(c[None] if c.ndim == 2 else c, origin, res)
        ticks = []
        for (rx, ry) in robot_cells:
            wx, wy = origin[0] + (rx + 0.5) * res, origin[1] + (ry + 0.5) * res
            _, cl, _, _ = sc.frontier_clusters(c.shape[-2:], (wx, wy), max_frontier_distance=max_frontier_distance, want_labels=False)
            pts = np.stack([cl["centroid_x"], cl["centroid_y"]], axis=1) if cl.size else np.zeros((0, 2))
            ticks.append((pts, np.array([wx, wy])))
        return ticks
    finally:
        sc.close()
