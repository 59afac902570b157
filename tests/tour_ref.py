"""Loader of tests/tour_ref/tour_ref.cpp, the CPU restatement of FullPathOptimizer::getNextGoal's selection and tour search
(DESIGN.md 4.11), and the restated next goal: the selection, the pair matrix from roadmap_ref's closest-node search and trees, the
reference's tour loop.  The restatement is compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tour_ref", "tour_ref.cpp")
SAFE, UNSAFE, UNDETERMINED = 0, 1, 2
SEL_LOCAL, SEL_GLOBAL, SEL_CLOSEST = 1, 2, 4
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="tour_ref_"), "libtour_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        L.tr_eligible.argtypes = [ci, vp, vp, vp, ci, vp, vp]
        L.tr_eligible.restype = None
        L.tr_select.argtypes = [ci, vp, vp, ci, cd, vp, C.POINTER(ci), vp, C.POINTER(ci)]
        L.tr_tour.argtypes = [ci, vp, C.POINTER(cd), C.POINTER(C.c_longlong), vp]
        L.tr_tour.restype = C.c_longlong
        L.tr_held_karp.argtypes = [ci, vp]
        L.tr_held_karp.restype = cd
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def eligible(goal_xyz, achievable, blacklisted=None, blacklist_xy=None):
    goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
    n = goal.shape[0]
    ach = np.ascontiguousarray(achievable, dtype=np.uint8)
    bl = None if blacklisted is None else np.ascontiguousarray(blacklisted, dtype=np.uint8)
    circ = np.zeros((0, 2)) if blacklist_xy is None else np.ascontiguousarray(blacklist_xy, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(n, dtype=np.uint8)
    lib().tr_eligible(n, _p(goal), _p(ach), _p(bl), circ.shape[0], _p(circ), _p(out))
    return out


def select(path_length_m, elig, n_local=5, radius=12.0):
    """(locals, globals, closest global or -1) of getFilteredFrontiersN"""
    plm = np.ascontiguousarray(path_length_m, dtype=np.float64)
    el = np.ascontiguousarray(elig, dtype=np.uint8)
    n = plm.shape[0]
    loc = np.zeros(max(n, 1), np.int32); glob = np.zeros(max(n, 1), np.int32)
    nl, ng = C.c_int(), C.c_int()
    cg = lib().tr_select(n, _p(plm), _p(el), int(n_local), float(radius), _p(loc), C.byref(nl), _p(glob), C.byref(ng))
    return loc[:nl.value].tolist(), glob[:ng.value].tolist(), cg


def selection_codes(n, loc, glob, cg):
    sel = np.zeros(n, np.uint8)
    sel[loc] = SEL_LOCAL
    sel[glob] = SEL_GLOBAL
    if cg >= 0:
        sel[cg] |= SEL_CLOSEST
    return sel


def tour(M):
    """getBestFullPath over M [(k+2)][(k+2)]: (min length, number of minimum tours, winning order of positions, tours tried)"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    k = M.shape[0] - 2
    L, cnt = C.c_double(), C.c_longlong()
    perm = np.zeros(max(k, 1), np.int32)
    tried = lib().tr_tour(k, _p(M), C.byref(L), C.byref(cnt), _p(perm))
    return L.value, cnt.value, perm[:k].tolist(), tried


def held_karp(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    return lib().tr_held_karp(M.shape[0] - 2, _p(M))


def tour_length(M, order):
    """calculatePathLength of robot -> locals in `order` (positions) -> global, summed left to right from 0.0"""
    path = [0] + [p + 1 for p in order] + [M.shape[0] - 1]
    s = 0.0
    for a, b in zip(path[:-1], path[1:]):
        s += M[a, b]
    return s


def pair_matrix(ref, pts, radius=12.0):
    """getPlan(i, true, j, true) for i < j over the points [m][2] on a roadmap_ref.Roadmap: equal points 0, else the tree from i's
    closest key node, the segment lengths summed from j's closest key node back along the predecessors; radius * 100000 where there
    is no path.  Symmetric, the lower index the direction."""
    pts = np.asarray(pts, dtype=np.float64)
    m = pts.shape[0]
    g = ref.graph()
    xy = g["xy"]
    start = [ref.closest(pts[i, 0], pts[i, 1], True) for i in range(m)]
    trees = {}
    M = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1, m):
            if pts[i, 0] == pts[j, 0] and pts[i, 1] == pts[j, 1]:
                v = 0.0
            else:
                v = radius * 100000
                s, e = start[i], start[j]
                if s >= 0 and e >= 0:
                    if s not in trees:
                        trees[s] = ref.tree(s)
                    t = trees[s]
                    if t["d"][e] < math.inf:
                        acc, w = 0.0, e
                        while w != s:
                            u = int(t["pred"][w])
                            ex, ey = xy[w, 0] - xy[u, 0], xy[w, 1] - xy[u, 1]
                            acc += math.sqrt(ex * ex + ey * ey)
                            w = u
                        v = acc
            M[i, j] = M[j, i] = v
    return M


def next_goal(ref, robot_xy, goal_xyz, path_length_m, achievable, blacklisted=None, blacklist_xy=None, n_local=5, radius=12.0):
    """getNextGoal without the FI check: dict like FrontierScorer.roadmap_next_goal's (status SAFE where the FI check would run)."""
    goal = np.asarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
    n = goal.shape[0]
    el = eligible(goal, achievable, blacklisted, blacklist_xy)
    loc, glob, cg = select(path_length_m, el, n_local, radius)
    out = dict(selection=selection_codes(n, loc, glob, cg), n_locals=len(loc), next_index=-1, status=UNDETERMINED,
               tour=np.zeros(0, np.int32), tour_length=0.0, n_tied=0, pair_length_m=None)
    if not loc:
        if glob:
            out.update(next_index=cg, status=SAFE, tour=np.array([cg], np.int32))
        return out
    pts = np.concatenate([np.asarray(robot_xy, dtype=np.float64).reshape(1, 2), goal[loc, :2], goal[[cg], :2]])
    M = pair_matrix(ref, pts, radius)
    L, cnt, perm, _ = tour(M)
    out.update(pair_length_m=M, tour_length=L, n_tied=cnt)
    if L >= radius * 100000:
        return out
    t = [loc[p] for p in perm] + [cg]
    out.update(tour=np.array(t, np.int32), next_index=t[0], status=SAFE)
    return out
