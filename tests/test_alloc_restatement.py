"""The task allocator's CPU restatement (tests/alloc_ref/alloc_ref.cpp) against the answers the reference's own
sources gave on their held inputs (tests/golden/alloc_reference_held.json), against a brute-force optimum, and on the scan-order
properties the GPU kernel is held to; and the new entry points of the C ABI without a device."""
import itertools
import struct

import numpy as np
import pytest

import alloc_ref as A


def _bits(x):
    return struct.pack("<d", x)


@pytest.mark.parametrize("case", A.golden(), ids=lambda c: c["name"])
def test_reference_held_inputs(case):
    got = A.allocate(case["cost"], case["distance"], case["method"])
    assert got["assignment"].tolist() == case["assignment"]
    assert _bits(got["total_cost"]) == _bits(case["total_cost"])
    assert not got["capped"]


def test_minpos_matrices_of_the_held_input():
    """minPos_test.cpp: robots 2 and 3 tie in every column (strict <: neither counts the other), column 0 ties for all four"""
    case = next(c for c in A.golden() if c["method"] == "minpos")
    P, mod = A.minpos(case["cost"], case["distance"])
    assert P.tolist() == [[0, 3, 1, 3], [0, 2, 0, 2], [0, 0, 2, 0], [0, 0, 2, 0]]
    want = np.where(P == 0, case["cost"], A.DBL_MAX)
    assert mod.tobytes() == want.tobytes()


def _brute_force(cost):
    R, n = cost.shape
    best = np.inf
    if R <= n:
        for cols in itertools.permutations(range(n), R):
            best = min(best, sum(cost[r, c] for r, c in enumerate(cols)))
    else:
        for rows in itertools.permutations(range(R), n):
            best = min(best, sum(cost[r, c] for c, r in enumerate(rows)))
    return best


@pytest.mark.parametrize("R,n", [(1, 1), (1, 7), (2, 2), (3, 3), (2, 5), (5, 2), (4, 6), (5, 5), (5, 7), (3, 7), (5, 4)])
def test_total_is_the_brute_force_optimum(R, n):
    """finite matrices, R <= 5 and n <= 7: the total equals the optimum over every assignment to 1e-12 relative (a different
    optimal assignment may sum differently); the assignment is a matching of min(R, n) pairs"""
    rng = np.random.default_rng(100 * R + n)
    for trial in range(6):
        cost = rng.uniform(0.0, 50.0, (R, n))
        if trial % 2:
            cost = np.floor(cost / 5.0)                  # ties
        got = A.solve(cost)
        want = _brute_force(cost)
        assert got["total_cost"] == pytest.approx(want, rel=1e-12, abs=0.0 if want else 1e-300)
        a = got["assignment"]
        taken = a[a >= 0]
        assert len(taken) == min(R, n) and len(set(taken.tolist())) == len(taken)
        assert got["step5"] <= A.step5_cap(R, n)


def test_one_robot_takes_the_first_minimum():
    cost = np.array([[4.0, 2.0, 7.0, 2.0, 9.0, 2.0]])
    got = A.solve(cost)
    assert got["assignment"].tolist() == [1] and got["total_cost"] == 2.0
    rng = np.random.default_rng(3)
    for n in (1, 5, 64, 1025):
        row = np.floor(rng.uniform(0, 8, (1, n)))
        assert A.solve(row)["assignment"][0] == int(np.argmin(row[0]))


def test_two_dbl_max_entries_sum_to_infinity():
    """what the reference returns when two assigned entries are DBL_MAX"""
    got = A.solve(np.full((2, 2), A.DBL_MAX))
    assert got["assignment"].tolist() == [0, 1] and got["total_cost"] == np.inf


@pytest.mark.parametrize("family", A.FAMILIES)
def test_families_stay_within_the_step5_cap(family):
    for R, n in [(5, 2), (3, 8), (16, 17), (33, 64), (64, 3)]:
        cost, dist = A.family(family, R, n, 7 * R + n)
        for method in ("hungarian", "minpos"):
            got = A.allocate(cost, dist, method)
            assert not got["capped"] and got["step5"] <= A.step5_cap(R, n)
            taken = got["assignment"][got["assignment"] >= 0]
            assert len(taken) == min(R, n) and len(set(taken.tolist())) == len(taken)


def test_library_exports_the_allocator(fs):
    """the new entry points are exported and refuse a null context without a device"""
    lib = fs.load_library()
    for name in ("fs_allocate_tasks", "fs_allocate_tasks_dev", "fs_fleet_allocate_roadmap"):
        assert hasattr(lib, name) and name in fs.capi.EXPORTED_SYMBOLS
    assert lib.fs_allocate_tasks(None, 1, 1, None, None, 0, None, None, None, None) == fs.capi.FS_E_INVALID
    assert lib.fs_allocate_tasks_dev(None, 1, 1, None, None, 0, None, None, None, None, None) == fs.capi.FS_E_INVALID
    assert lib.fs_fleet_allocate_roadmap(None, 1, None, 1, None, None, None, 0.25, 1.0, 0.5, 0.5, 0, None, None, None, None, None,
                                         None, None) == fs.capi.FS_E_INVALID
