"""fs_allocate_tasks on the GPU (fit-slam_amd/csrc/fs_allocate.hip): the reference's held inputs, and random
matrices of every value family against the CPU restatement (tests/alloc_ref/alloc_ref.cpp) bit for bit — assignment, the bits of
the total, MinPos' P and modified matrix — over shapes that take both branches (R <= n, R > n), are no powers of two, have more
columns than the workgroup has threads and sit on the limits; the device form; the step-5 counter; every refusal."""
import importlib
import struct

import numpy as np
import pytest

import alloc_ref as A

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
SHAPES = [(1, 1), (1, 5), (2, 2), (5, 2), (64, 3), (3, 8), (8, 8), (16, 17), (33, 64), (64, 64), (64, 200), (5, 1025), (64, 4096)]
METHODS = ("hungarian", "minpos")


@pytest.fixture(scope="module")
def sc():
    s = fsmod.FrontierScorer(device=0)
    yield s
    s.close()


def _bits(x):
    return struct.pack("<d", x)


def _same(got, want, what):
    print(what, "assignment", got["assignment"].tolist()[:8], "total", got["total_cost"], "restated", want["total_cost"])
    assert got["assignment"].tolist() == want["assignment"].tolist(), what
    assert _bits(got["total_cost"]) == _bits(want["total_cost"]), what
    if "rank" in want:
        assert got["rank"].tobytes() == want["rank"].tobytes(), what
        assert got["modified_cost"].tobytes() == want["modified_cost"].tobytes(), what


@pytest.mark.parametrize("case", A.golden(), ids=lambda c: c["name"])
def test_reference_held_inputs(sc, case):
    got = sc.allocate_tasks(case["cost"], case["distance"], method=case["method"], want_rank=True)
    assert got["assignment"].tolist() == case["assignment"]
    assert _bits(got["total_cost"]) == _bits(case["total_cost"])


@pytest.mark.parametrize("R,n", SHAPES)
def test_equals_the_restatement_bit_for_bit(sc, R, n):
    """every family and both methods at one shape; counters 1030-1032 are the restatement's own counts, 1031 within the cap"""
    for k, family in enumerate(A.FAMILIES):
        cost, dist = A.family(family, R, n, 1000 * R + n + k)
        for method in METHODS:
            want = A.allocate(cost, dist, method)
            assert not want["capped"]
            got = sc.allocate_tasks(cost, dist if method == "minpos" else None, method=method, want_rank=True)
            _same(got, want, (R, n, family, method))
            counters = [sc.get_counter(1030), sc.get_counter(1031), sc.get_counter(1032)]
            print((R, n, family, method), "augmentations, step-5 runs, primes", counters, "cap", A.step5_cap(R, n))
            assert counters == [want["augmentations"], want["step5"], want["primes"]]
            assert counters[1] <= A.step5_cap(R, n)


def test_one_robot_takes_the_first_minimum(sc):
    row = np.array([[4.0, 2.0, 7.0, 2.0, 9.0, 2.0]])
    got = sc.allocate_tasks(row)
    assert got["assignment"].tolist() == [1] and got["total_cost"] == 2.0


def test_two_dbl_max_entries_sum_to_infinity(sc):
    got = sc.allocate_tasks(np.full((2, 2), A.DBL_MAX))
    assert got["assignment"].tolist() == [0, 1] and got["total_cost"] == np.inf


@pytest.mark.parametrize("R,n", [(5, 2), (16, 17), (33, 64), (5, 1025)])
def test_device_form_equals_host_form(sc, R, n):
    import torch
    dev = torch.device("cuda", 0)
    cost, dist = A.family("quantised", R, n, 31 * R + n)
    for method in METHODS:
        host = sc.allocate_tasks(cost, dist, method=method, want_rank=True)
        d_cost = torch.from_numpy(cost).to(dev); d_dist = torch.from_numpy(dist).to(dev)
        d_asg = torch.full((R,), -7, dtype=torch.int32, device=dev); d_total = torch.zeros(1, dtype=torch.float64, device=dev)
        d_rank = torch.zeros((R, n), dtype=torch.int32, device=dev); d_mod = torch.zeros((R, n), dtype=torch.float64, device=dev)
        d_status = torch.full((1,), 99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        sc.allocate_tasks_dev(R, n, d_cost.data_ptr(), d_dist.data_ptr() if method == "minpos" else 0, method, d_asg.data_ptr(),
                              d_total.data_ptr(), d_status.data_ptr(), d_rank=d_rank.data_ptr(), d_modified_cost=d_mod.data_ptr())
        sc.synchronize()
        assert int(d_status.cpu()[0]) == 0
        assert d_asg.cpu().numpy().tolist() == host["assignment"].tolist()
        assert _bits(float(d_total.cpu()[0])) == _bits(host["total_cost"])
        if method == "minpos":
            assert d_rank.cpu().numpy().tobytes() == host["rank"].tobytes()
            assert d_mod.cpu().numpy().tobytes() == host["modified_cost"].tobytes()
        # without the optional matrices (MinPos keeps its matrix in the context's scratch): the same answer
        d_asg.fill_(-7)
        torch.cuda.synchronize()
        sc.allocate_tasks_dev(R, n, d_cost.data_ptr(), d_dist.data_ptr() if method == "minpos" else 0, method, d_asg.data_ptr(),
                              d_total.data_ptr(), d_status.data_ptr())
        sc.synchronize()
        assert int(d_status.cpu()[0]) == 0 and d_asg.cpu().numpy().tolist() == host["assignment"].tolist()


def _refused(sc, code, cost, distance=None, method=0, R=None, n=None):
    """the raw call: its code, and nothing written"""
    import ctypes as C
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    R = cost.shape[0] if R is None else R
    n = cost.shape[1] if n is None else n
    asg = np.full(max(R, 1), -7, dtype=np.int32)
    total = C.c_double(-7.0)
    rank = np.full(cost.shape, -7, dtype=np.int32)
    mod = np.full(cost.shape, -7.0)
    dist = None if distance is None else np.ascontiguousarray(distance, dtype=np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = sc._L.fs_allocate_tasks(sc._h, R, n, p(cost), p(dist), method, p(asg), C.byref(total), p(rank), p(mod))
    assert rc == code, (rc, code)
    assert (asg == -7).all() and total.value == -7.0 and (rank == -7).all() and (mod == -7.0).all()


def test_refusals_return_their_code_and_write_nothing(sc):
    E = fsmod.capi.FS_E_INVALID
    good = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
        m = good.copy(); m[1, 2] = bad
        _refused(sc, E, m)                                   # an entry of cost
        _refused(sc, E, m, distance=good, method=1)
        _refused(sc, E, good, distance=m, method=1)          # an entry of distance
    _refused(sc, E, good, method=1)                          # MINPOS without distance
    _refused(sc, E, good, method=2)                          # unknown method
    _refused(sc, E, good, R=0)
    _refused(sc, E, good, n=0)
    _refused(sc, E, good, R=fsmod.capi.FS_ALLOC_MAX_ROBOTS + 1)
    _refused(sc, E, good, n=fsmod.capi.FS_ALLOC_MAX_TASKS + 1)
    # DBL_MAX and zero are entries like any other
    m = good.copy(); m[0, 0] = A.DBL_MAX; m[1, 1] = 0.0
    got = sc.allocate_tasks(m, m, method="minpos")
    assert got["assignment"].tolist() == A.allocate(m, m, "minpos")["assignment"].tolist()
    # the device form reports a refused entry through d_status and writes nothing else
    import torch
    dev = torch.device("cuda", 0)
    m = good.copy(); m[0, 1] = np.nan
    d_cost = torch.from_numpy(m).to(dev)
    d_asg = torch.full((2,), -7, dtype=torch.int32, device=dev); d_total = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sc.allocate_tasks_dev(2, 3, d_cost.data_ptr(), 0, "hungarian", d_asg.data_ptr(), d_total.data_ptr(), d_status.data_ptr())
    sc.synchronize()
    assert int(d_status.cpu()[0]) == E and d_asg.cpu().numpy().tolist() == [-7, -7] and float(d_total.cpu()[0]) == -7.0
    with pytest.raises(fsmod.FsError):
        sc.allocate_tasks_dev(2, 3, d_cost.data_ptr(), 0, "minpos", d_asg.data_ptr(), d_total.data_ptr(), d_status.data_ptr())
