"""Loader of tests/roadmap_kf_ref/roadmap_kf_ref.cpp, the CPU restatement of the roadmap's key-frame anchors:
mapDataCallback, optimizeSHM and populateNodes.  Compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use.  The
edges of an optimised roadmap come from tests/roadmap_ref (`graph_of`)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "roadmap_kf_ref", "roadmap_kf_ref.cpp")
FS_E_RANGE = -6
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="roadmap_kf_ref_"), "libroadmap_kf_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.kr_create.argtypes = [cd, cd, cd]
        L.kr_create.restype = vp
        L.kr_destroy.argtypes = [vp]
        L.kr_destroy.restype = None
        L.kr_add_nodes.argtypes = [vp, ci, vp, ci]
        L.kr_set_keyframes.argtypes = [vp, ci, vp, vp, C.POINTER(ci), C.POINTER(ci)]
        L.kr_optimize.argtypes = [vp]
        L.kr_nodes.argtypes = [vp, vp]
        L.kr_anchors.argtypes = [vp, C.POINTER(ci), vp, vp]
        L.kr_anchors.restype = C.c_longlong
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class KfRoadmap:
    """One restated FrontierRoadMap's nodes, queue, key frames and anchors."""

    def __init__(self, grid_cell_size=1.0, min_frontier=0.25, min_robot=0.25):
        self.cell, self.min_frontier, self.min_robot = grid_cell_size, min_frontier, min_robot
        self._h = lib().kr_create(grid_cell_size, min_frontier, min_robot)

    def close(self):
        if self._h:
            lib().kr_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def add_nodes(self, xy, is_robot_pose=False):
        p = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
        return lib().kr_add_nodes(self._h, p.shape[0], _p(p), 1 if is_robot_pose else 0)

    def set_keyframes(self, ids, pose7):
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        poses = np.ascontiguousarray(np.asarray(pose7, dtype=np.float64).reshape(-1, 7))
        a, o = C.c_int(), C.c_int()
        rc = lib().kr_set_keyframes(self._h, ids.shape[0], _p(ids), _p(poses), C.byref(a), C.byref(o))
        if rc:
            raise ValueError("a pose without inverse")
        return a.value, o.value

    def optimize(self):
        return lib().kr_optimize(self._h)

    def nodes(self):
        n = lib().kr_nodes(self._h, None)
        xy = np.zeros((n, 2))
        lib().kr_nodes(self._h, _p(xy))
        return xy

    def anchors(self):
        k = C.c_int()
        r = lib().kr_anchors(self._h, C.byref(k), None, None)
        ids = np.zeros(r, np.int32); pts = np.zeros((r, 3), np.float32)
        lib().kr_anchors(self._h, C.byref(k), _p(ids), _p(pts))
        return dict(n_pending=k.value, kf_id=ids, point_c=pts)


def graph_of(nodes_xy, cells, origin, res, grid_cell_size=1.0, radius=6.1, min_frontier=0.25, min_robot=0.25):
    """roadmap_ref's rebuilt roadmap over an optimised node list (populated in order, then reConstructGraph)."""
    import roadmap_ref as R
    ref = R.Roadmap(cells, origin, res, grid_cell_size, radius, min_frontier, min_robot)
    rc = ref.populate(nodes_xy)
    assert rc == 0
    ref.rebuild()
    return ref


def pose(x, y, yaw=0.0, z=0.0, scale=1.0):
    """pose7 of a planar key frame; scale != 1 leaves the quaternion unnormalised"""
    return np.array([x, y, z, 0.0, 0.0, scale * np.sin(yaw / 2), scale * np.cos(yaw / 2)])


def correct(poses, dx, dy, dyaw, about=(0.0, 0.0)):
    """a rigid correction of planar poses: rotate by dyaw about `about`, then shift by (dx, dy)"""
    out = np.array(poses, dtype=np.float64, copy=True).reshape(-1, 7)
    c, s = np.cos(dyaw), np.sin(dyaw)
    px, py = out[:, 0] - about[0], out[:, 1] - about[1]
    out[:, 0] = about[0] + c * px - s * py + dx
    out[:, 1] = about[1] + s * px + c * py + dy
    yaw = 2 * np.arctan2(out[:, 5], out[:, 6]) + dyaw
    out[:, 5], out[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    return out


def trajectory(seed, n_ticks, step=0.5, start=(0.0, 0.0), bounds=None):
    """A seeded robot walk: one key frame per tick (~step metres apart), with frontier nodes scattered around each pose."""
    rng = np.random.default_rng(seed)
    x, y, yaw = float(start[0]), float(start[1]), 0.0
    poses, frontiers = [], []
    for t in range(n_ticks):
        yaw += rng.normal(0, 0.4)
        nx, ny = x + step * np.cos(yaw), y + step * np.sin(yaw)
        if bounds is not None and not (bounds[0] < nx < bounds[1] and bounds[2] < ny < bounds[3]):
            yaw += np.pi
            nx, ny = x + step * np.cos(yaw), y + step * np.sin(yaw)
        x, y = nx, ny
        poses.append(pose(x, y, yaw))
        k = int(rng.integers(2, 7))
        r = rng.uniform(0.3, 3.0, k); a = rng.uniform(-np.pi, np.pi, k)
        frontiers.append(np.stack([x + r * np.cos(a), y + r * np.sin(a)], axis=1))
    return np.array(poses), frontiers
