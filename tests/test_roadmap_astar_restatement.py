"""fs_roadmap_astar.h, the per-goal A* of the REFERENCE roadmap search, compiled for the host by g++ through
tests/roadmap_astar_ref/: its heap against std::priority_queue with the reference's comparator, and its search against the
restatement's per-goal A* (tests/roadmap_ref/roadmap_ref.cpp, reference_astar) on walled maps and on lattice roadmaps, where equal
f values are frequent and their order decides answers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import roadmap_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "roadmap_astar_ref", "roadmap_astar_ref.cpp")
RES = 0.05
ORIGIN = (-1.0, -1.0, 0.0)
FOUND, NO_PATH, OVERFLOW = 0, 1, 2
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="roadmap_astar_ref_"), "libroadmap_astar_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci = C.c_void_p, C.c_int
        L.ra_heap_sequence.argtypes = [ci, vp, vp, ci, vp]
        L.ra_astar.argtypes = [ci, vp, vp, vp, ci, ci, ci, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def astar(graph, start, goal, cap=1 << 15):
    xy = np.ascontiguousarray(graph["xy"], dtype=np.float64)
    row = np.ascontiguousarray(graph["row_ptr"], dtype=np.int32)
    col = np.ascontiguousarray(graph["col"] if graph["col"].size else np.zeros(1, np.int32), dtype=np.int32)
    length, pops = np.zeros(1), np.zeros(1, np.int32)
    rc = lib().ra_astar(xy.shape[0], _p(xy), _p(row), _p(col), int(start), int(goal), int(cap), _p(length), _p(pops))
    return rc, float(length[0]), int(pops[0])


def _free(n):
    return np.zeros((n, n), dtype=np.uint8)


@pytest.mark.parametrize("seed", range(6))
def test_heap_pops_in_priority_queue_order(seed):
    rng = np.random.default_rng(seed)
    values = rng.choice([0.0, 0.5, 1.0, 1.25, 2.0, 3.5], size=rng.integers(2, 7), replace=False)
    n = 4000
    op = np.where(rng.random(n) < 0.58, rng.integers(0, values.size, n), -1).astype(np.int32)
    f = np.ascontiguousarray(values, dtype=np.float64)
    got, want = np.zeros(n, np.int32), np.zeros(n, np.int32)
    k_got = lib().ra_heap_sequence(n, _p(op), _p(f), 0, _p(got))
    k_want = lib().ra_heap_sequence(n, _p(op), _p(f), 1, _p(want))
    assert k_got == k_want > 1000
    assert np.array_equal(got[:k_got], want[:k_want])


def _compare(r, poses, goals):
    """every goal of every pose: the header's A* from closest(robot) to closest(goal) against rr_plan(leg=REFERENCE_ASTAR)"""
    g = r.graph()
    checked = found = 0
    for pose in poses:
        want = r.plan(pose, goals, leg=R.REFERENCE_ASTAR)
        s = r.closest(pose[0], pose[1])
        for i, (gx, gy, _) in enumerate(goals):
            if gx == pose[0] and gy == pose[1]:
                continue
            t = r.closest(gx, gy)
            if s < 0 or t < 0:
                assert want["achievable"][i] == 0
                continue
            rc, length, _ = astar(g, s, t)
            assert rc in (FOUND, NO_PATH)
            assert (rc == FOUND) == (want["achievable"][i] == 1), i
            if rc == FOUND:
                assert np.float64(length).tobytes() == want["path_length_m"][i].tobytes(), (i, length, want["path_length_m"][i])
                found += 1
            checked += 1
    return checked, found


@pytest.mark.parametrize("seed", range(4))
def test_search_equals_restatement_on_walled_maps(seed):
    rng = np.random.default_rng(seed)
    n = 200
    cells = _free(n)
    for _ in range(12):
        x, y = rng.integers(0, n, 2)
        if rng.random() < 0.5:
            cells[y, x:x + rng.integers(10, 60)] = 254
        else:
            cells[y:y + rng.integers(10, 60), x] = 254
    r = R.Roadmap(cells, ORIGIN, RES, radius=3.0)
    r.populate(rng.uniform(ORIGIN[0], ORIGIN[0] + n * RES, size=(150, 2)))
    r.rebuild()
    xy = r.graph()["xy"]
    poses = [R.pose7(*(xy[rng.integers(xy.shape[0])] + rng.uniform(-0.2, 0.2, 2))) for _ in range(5)]
    goals = np.zeros((80, 3))
    goals[:, :2] = rng.uniform(ORIGIN[0], ORIGIN[0] + n * RES, size=(80, 2))
    checked, found = _compare(r, poses, goals)
    assert checked == 400 and found > 100


@pytest.mark.parametrize("step,radius", [(0.5, 2.1), (1.0, 3.1)])
def test_search_equals_restatement_on_lattices(step, radius):
    """nodes on a lattice over a free map: squared segment lengths are exact, and many records tie in f"""
    n = 220
    r = R.Roadmap(_free(n), ORIGIN, RES, radius=radius)
    side = np.arange(ORIGIN[0] + 0.25, ORIGIN[0] + n * RES - 0.25, step)
    gx, gy = np.meshgrid(side, side)
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1)
    assert r.populate(pts) == 0
    r.rebuild()
    rng = np.random.default_rng(int(step * 10))
    poses = [R.pose7(*pts[i]) for i in rng.integers(0, pts.shape[0], 20)]
    goals = np.zeros((100, 3))
    goals[:, :2] = pts[rng.integers(0, pts.shape[0], 100)]
    checked, found = _compare(r, poses, goals)
    assert checked >= 1900 and found == checked


def test_four_node_graph_returns_the_direct_edge():
    """test_roadmap_restatement.py's graph: the squared heuristic pops the goal at f = 4 before the g-shorter detour"""
    r = R.Roadmap(_free(160), ORIGIN, RES, radius=3.0)
    r.populate([[0.0, 0.0], [2.0, 0.0], [0.5, 0.9], [1.5, 0.9]])
    r.rebuild()
    rc, length, pops = astar(r.graph(), 0, 1)
    assert rc == FOUND and length == 2.0 and pops == 2


def test_overflow_is_reported_not_truncated():
    r = R.Roadmap(_free(160), ORIGIN, RES, radius=3.0)
    r.populate([[0.0, 0.0], [2.0, 0.0], [0.5, 0.9], [1.5, 0.9]])
    r.rebuild()
    assert astar(r.graph(), 0, 1, cap=2)[0] == OVERFLOW
    assert astar(r.graph(), 0, 1, cap=4)[:2] == (FOUND, 2.0)
