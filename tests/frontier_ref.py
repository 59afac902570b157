"""Loader of tests/frontier_ref/frontier_ref.cpp, the CPU restatement of the order-dependent tail of the frontier search (pieces and
goal points) and the check of fit-slam_amd/csrc/fs_median_sort.h against std::sort.  Compiled by g++ -O2
-ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "frontier_ref", "frontier_ref.cpp")
CSRC = os.path.join(ROOT, "fit-slam_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="frontier_ref_"), "libfrontier_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
        L.fr_search.argtypes = [vp, i32, i32, dbl, dbl, dbl, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                C.POINTER(C.c_int64), C.POINTER(i32)]
        L.fr_search.restype = i32
        L.fr_sort_check.argtypes = [vp, i32, i32, vp]
        L.fr_sort_check.restype = i32
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def oracle_labels(r):
    """Per cell the component label (smallest cell index) of the oracle's search, -1 elsewhere."""
    seed = r["cell_seed"]
    ny, nx = seed.shape
    idx = np.arange(ny * nx).reshape(ny, nx)
    out = np.full((ny, nx), -1, dtype=np.int32)
    for s in np.unique(seed[seed >= 0]):
        m = seed == s
        out[m] = idx[m].min()
    return out


def oracle_seeds(r):
    """The seed cells of the oracle's buildNewFrontier calls, in call order (ordered by the piece each seed opened)."""
    cs = r["cell_seed"].ravel()
    cp = r["cell_piece"].ravel()
    seeds = np.unique(cs[cs >= 0])
    return seeds[np.argsort(cp[seeds], kind="stable")].astype(np.int32)


def search(labels, origin, res, robot_cell, min_size=1, max_size=20, seeds=None):
    """dict(goals [k][2], sizes, label, goal_cell, seed_cell, cell_piece [ny][nx], every_cells, guarded); None for a refused seed."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    ny, nx = lab.shape
    n = nx * ny
    cap = n + 1
    goals = np.zeros((cap, 2)); size = np.zeros(cap, np.int32); label = np.zeros(cap, np.int32)
    goal_cell = np.zeros(cap, np.int32); seed_cell = np.zeros(cap, np.int32)
    cell_piece = np.zeros((ny, nx), np.int32); every = np.zeros(cap, np.int32)
    n_every, guarded = C.c_int64(), C.c_int32()
    sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32)
    k = lib().fr_search(_p(lab), nx, ny, float(origin[0]), float(origin[1]), float(res), int(robot_cell), int(min_size), int(max_size),
                        0 if sd is None else sd.shape[0], _p(sd), cap, _p(goals), _p(size), _p(label), _p(goal_cell), _p(seed_cell),
                        _p(cell_piece), _p(every), C.byref(n_every), C.byref(guarded))
    if k < 0:
        return None
    return dict(goals=goals[:k].copy(), sizes=size[:k].copy(), label=label[:k].copy(), goal_cell=goal_cell[:k].copy(),
                seed_cell=seed_cell[:k].copy(), cell_piece=cell_piece, every_cells=every[:n_every.value].copy(), guarded=guarded.value)


def search_call(labels, origin, res, robot_cell, min_size=1, max_size=20):
    """A zero-argument callable that runs only the restatement's Nearest search (its output buffers allocated beforehand): for
    timing the host tail without the wrapper's allocations."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    ny, nx = lab.shape
    cap = nx * ny + 1
    bufs = [np.zeros((cap, 2)), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32),
            np.zeros((ny, nx), np.int32), np.zeros(cap, np.int32)]
    n_every, guarded = C.c_int64(), C.c_int32()
    args = [_p(lab), nx, ny, float(origin[0]), float(origin[1]), float(res), int(robot_cell), int(min_size), int(max_size), 0, None, cap] + \
        [_p(b) for b in bufs] + [C.byref(n_every), C.byref(guarded)]
    f = lib().fr_search
    return lambda keep=(lab, bufs, n_every, guarded): f(*args)     # (keep: the buffers live as long as the callable)


def sort_check(values, mode):
    """fs_median_sort.h against std::sort: (1 equal / 0 different / -1 guard fired, the restatement's permutation)."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    ids = np.zeros(v.shape[0], np.int32)
    return lib().fr_sort_check(_p(v), v.shape[0], int(mode), _p(ids)), ids
