"""Loader of tests/alloc_ref/alloc_ref.cpp, the CPU restatement of the reference's task allocator: MinPos' rank
and modified matrices and Munkres as HungarianAlgorithm::Solve runs it, iterative; and the matrix families the allocator's tests
share.  The restatement is compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "alloc_ref", "alloc_ref.cpp")
GOLDEN = os.path.join(HERE, "golden", "alloc_reference_held.json")
DBL_MAX = float(np.finfo(np.float64).max)
FAMILIES = ("u1", "quantised", "equal", "dbl_max", "contested")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="alloc_ref_"), "liballoc_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci = C.c_void_p, C.c_int
        L.ar_minpos.argtypes = [ci, ci, vp, vp, vp, vp]
        L.ar_minpos.restype = None
        L.ar_solve.argtypes = [ci, ci, vp, vp, C.POINTER(C.c_double), vp]
        L.ar_solve.restype = ci
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def minpos(cost, distance):
    """(P [R][n] int32, modified cost [R][n]) of MinPosAlgo"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    dist = np.ascontiguousarray(distance, dtype=np.float64)
    R, n = cost.shape
    P = np.zeros((R, n), dtype=np.int32)
    mod = np.zeros((R, n))
    lib().ar_minpos(R, n, _p(cost), _p(dist), _p(P), _p(mod))
    return P, mod


def solve(cost):
    """HungarianAlgorithm::Solve: dict(assignment [R], total_cost, augmentations, step5, primes, capped)"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    R, n = cost.shape
    a = np.zeros(R, dtype=np.int32)
    total = C.c_double()
    stats = np.zeros(3, dtype=np.int64)
    rc = lib().ar_solve(R, n, _p(cost), _p(a), C.byref(total), _p(stats))
    return dict(assignment=a, total_cost=total.value, augmentations=int(stats[0]), step5=int(stats[1]), primes=int(stats[2]), capped=bool(rc))


def allocate(cost, distance=None, method="hungarian"):
    """TaskAllocator::solveAllocationHungarian / solveAllocationMinPos: solve()'s dict, plus rank and modified_cost under "minpos" """
    if method == "hungarian":
        return solve(cost)
    P, mod = minpos(cost, distance)
    out = solve(mod)
    out.update(rank=P, modified_cost=mod)
    return out


def step5_cap(R, n):
    return (R + 1) * (min(R, n) + 1)


def family(name, R, n, seed):
    """(cost, distance) [R][n] of one of the value families the allocator is tested on: "u1" continuous U1-like costs 1 / u with
    10 % dead entries and 20 % dead columns at DBL_MAX; "quantised" the same costs in quarter steps with integer distances (heavy
    ties); "equal" every entry equal; "dbl_max" every entry DBL_MAX; "contested" a column value in eighths plus a row offset in
    quarters (exact sums), so every robot wants the same frontiers in the same order and wide matrices do not end at the greedy stars"""
    rng = np.random.default_rng(seed)
    cost = 1.0 / rng.uniform(0.01, 1.0, (R, n))
    dist = rng.uniform(0.0, 30.0, (R, n))
    dead = (rng.random((R, n)) < 0.1) | (rng.random(n) < 0.2)[None, :]
    if name == "quantised":
        cost = np.floor(cost * 4.0) / 4.0
        dist = np.floor(dist)
    if name in ("u1", "quantised"):
        cost[dead] = DBL_MAX
    elif name == "equal":
        cost[:] = 3.5
        dist[:] = 2.0
    elif name == "dbl_max":
        cost[:] = DBL_MAX
    elif name == "contested":
        cost = (np.floor(rng.uniform(0.0, 64.0, n) * 8.0) / 8.0)[None, :] + (np.floor(rng.uniform(0.0, 16.0, R) * 4.0) / 4.0)[:, None]
        dist = np.floor(dist)
    else:
        assert name in FAMILIES, name
    return np.ascontiguousarray(cost), np.ascontiguousarray(dist)


def golden():
    """the reference's own held inputs and the answers its sources gave: list of dict(name, method, cost, distance, assignment, total_cost)"""
    import json
    cases = json.load(open(GOLDEN))["cases"]
    for c in cases:
        c["cost"] = np.array([[float(v) for v in row] for row in c["cost"]])
        c["distance"] = None if c["distance"] is None else np.array([[float(v) for v in row] for row in c["distance"]])
        c["total_cost"] = float(c["total_cost"])
    return cases
