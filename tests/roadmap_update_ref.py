"""Loader of tests/roadmap_update_ref/roadmap_update_ref.cpp: fs_roadmap_update's order-free rules (fit-slam_amd/csrc/
fs_roadmap_update.h) applied on the CPU to a roadmap held as arrays, with the oracle's single-ray trace as
isConnectable.  Compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "roadmap_update_ref", "roadmap_update_ref.cpp")
HEADER = os.path.join(ROOT, "fit-slam_amd", "csrc", "fs_roadmap_update.h")
FS_E_RANGE = -6
_lib = None


def lib():
    global _lib
    if _lib is None:
        if os.path.join(ROOT, "oracle") not in sys.path:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        so = O.build()
        out = os.path.join(tempfile.mkdtemp(prefix="roadmap_update_ref_"), "libroadmap_update_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out, SRC, so,
                        "-Wl,-rpath," + os.path.dirname(os.path.abspath(so))], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.ruref_update.argtypes = [cd, cd, cd, cd, vp, ci, ci, cd, cd, cd, cd, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                   C.POINTER(C.c_int32), vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp,
                                   C.c_int32, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class State:
    """A roadmap as arrays: xy [n][2], key [n], adjacency lists in append order."""

    def __init__(self, xy=None, key=None, row_ptr=None, col=None):
        self.xy = np.zeros((0, 2)) if xy is None else np.array(xy, dtype=np.float64).reshape(-1, 2)
        self.key = np.zeros(0, np.uint8) if key is None else np.array(key, dtype=np.uint8)
        n = self.xy.shape[0]
        self.adj = [[] for _ in range(n)]
        if row_ptr is not None:
            self.adj = [list(map(int, col[row_ptr[p]:row_ptr[p + 1]])) for p in range(n)]

    @classmethod
    def of_graph(cls, g):
        return cls(g["xy"], g["key"], g["row_ptr"], g["col"])

    def graph(self):
        row = np.zeros(len(self.adj) + 1, np.int32)
        row[1:] = np.cumsum([len(a) for a in self.adj])
        col = np.array([q for a in self.adj for q in a], dtype=np.int32)
        return dict(xy=self.xy.copy(), key=self.key.copy(), row_ptr=row, col=col)


def update(state, cells, origin, res, params, pts, robot, add_robot=True):
    """One fs_roadmap_update on `state` by the order-free rules.  params = (cell, radius, min_frontier, min_robot).  Returns
    dict(rc, n_nodes_added, robot_added, n_edges_added, n_walks, owners, rounds, directional)."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    ny, nx = cells.shape
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 2))
    robot = np.ascontiguousarray(robot, dtype=np.float64).reshape(2)
    g = state.graph()
    n_old, n = g["xy"].shape[0], pts.shape[0]
    xy_old = np.ascontiguousarray(g["xy"]) if n_old else np.zeros((1, 2))
    key_old = g["key"] if n_old else np.zeros(1, np.uint8)
    col = g["col"] if g["col"].size else np.zeros(1, np.int32)
    cap = n_old + n + 1
    xy_out, key_out = np.zeros((cap, 2)), np.zeros(cap, np.uint8)
    n_nodes, n_added, robot_added, n_pairs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    pairs_cap = cap * cap
    pairs = np.zeros((max(pairs_cap, 1), 2), np.int32)
    stats = np.zeros(4, np.int64)
    o = tuple(float(v) for v in origin) + (0.0,) * (3 - len(origin))
    rc = lib().ruref_update(*[float(v) for v in params], _p(cells), nx, ny, o[0], o[1], o[2], float(res), n_old, _p(xy_old), _p(key_old),
                            _p(g["row_ptr"]), _p(col), n, _p(pts if n else np.zeros((1, 2))), _p(robot), 1 if add_robot else 0,
                            C.byref(n_nodes), _p(xy_out), _p(key_out), C.byref(n_added), C.byref(robot_added), C.byref(n_pairs), _p(pairs),
                            pairs_cap, _p(stats))
    assert rc in (0, FS_E_RANGE), rc
    state.xy = xy_out[:n_nodes.value].copy()
    state.key = key_out[:n_nodes.value].copy()
    state.adj += [[] for _ in range(n_nodes.value - n_old)]
    for p, q in pairs[:n_pairs.value]:
        state.adj[p].append(int(q))
        state.adj[q].append(int(p))
    return dict(rc=rc, n_nodes_added=n_added.value, robot_added=robot_added.value, n_edges_added=n_pairs.value, n_walks=int(stats[0]),
                owners=int(stats[1]), rounds=int(stats[2]), directional=int(stats[3]))


def same_graph(a, b):
    """bit for bit: node list, key flags, row_ptr, col"""
    return (a["xy"].shape == b["xy"].shape and a["xy"].tobytes() == b["xy"].tobytes() and np.array_equal(a["key"], b["key"])
            and np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["col"], b["col"]))
