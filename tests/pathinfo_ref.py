"""Loader of tests/pathinfo_ref/pathinfo_ref.cpp, the CPU restatement of the way points of fs_plan_paths_information (DESIGN.md
4.15), and the closed form the GPU uses.  Compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pathinfo_ref", "pathinfo_ref.cpp")
DBL_MAX = np.finfo(np.float64).max
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="pathinfo_ref_"), "libpathinfo_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.pr_waypoints.argtypes = [vp, ci, ci, cd, cd, cd, vp, ci, ci, vp, vp, cd, ci, C.c_int64, vp, vp, vp, vp, vp]
        L.pr_waypoints.restype = C.c_int64
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def waypoints(cells, origin, resolution, robot_pose7, goal_xyz, achievable_in=None, allow_unknown=False, sample_distance=1.5, lookahead=10):
    """The reference's sampling loop on the converged leg's paths: dict(count [n], offset [n + 1], xyyaw [total][3], index [total]: the path point of each way point, path_length [n])."""
    c = np.ascontiguousarray(cells, dtype=np.uint8)
    c = c[0] if c.ndim == 3 else c
    ny, nx = c.shape
    goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
    n = goal.shape[0]
    pose = np.ascontiguousarray(robot_pose7, dtype=np.float64).reshape(7)
    ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
    count = np.zeros(n, dtype=np.int32)
    offset = np.zeros(n + 1, dtype=np.int32)
    pl = np.zeros(n)
    s = int(sample_distance / resolution)
    room = n * (4 * max(nx, ny) // (s + 1)) + 1          # a path has at most 4 max(nx, ny) points
    xyyaw = np.zeros((room, 3))
    idx = np.zeros(room, dtype=np.int32)
    total = lib().pr_waypoints(_p(c), nx, ny, float(origin[0]), float(origin[1]), float(resolution), _p(pose), 1 if allow_unknown else 0, n,
                               _p(goal), _p(ai), float(sample_distance), int(lookahead), room, _p(count), _p(offset), _p(xyyaw), _p(idx), _p(pl))
    assert total >= 0, total
    return dict(count=count, offset=offset, xyyaw=xyyaw[:total].copy(), index=idx[:total].copy(), path_length=pl)


def closed_form_counts(path_length, resolution, sample_distance=1.5):
    """len // (s + 1) way points for a planned path, 0 otherwise: what the GPU sizes its offsets with."""
    s = int(sample_distance / resolution)
    planned = path_length != DBL_MAX
    return np.where(planned, np.where(planned, path_length, 0).astype(np.int64) // (s + 1), 0).astype(np.int32)


def closed_form_indices(length, resolution, sample_distance=1.5, lookahead=10):
    """[(j, j_to)] of a path of `length` points: way point k at j = len - (k + 1)(s + 1), looking at max(j - lookahead, 0)."""
    s = int(sample_distance / resolution)
    return [(length - (k + 1) * (s + 1), max(length - (k + 1) * (s + 1) - lookahead, 0)) for k in range(length // (s + 1))]


def yaw_to_quat(yaw):
    """orientationAroundZAxis: (x, y, z, w) [n][4]"""
    yaw = np.asarray(yaw, dtype=np.float64)
    q = np.zeros(yaw.shape + (4,))
    q[..., 2] = np.sin(yaw * 0.5)
    q[..., 3] = np.cos(yaw * 0.5)
    return q
