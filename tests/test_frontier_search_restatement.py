"""CPU checks of the frontier search's order-dependent tail, no GPU:
- fit-slam_amd/csrc/fs_median_sort.h, compiled with g++, equals std::sort element for element (plain doubles with duplicates, the
  reference's angle comparator on random and cyclic angle sets, median-of-three killers up to n = 1024 that reach the heap sort);
- the restatement tests/frontier_ref/frontier_ref.cpp, fed the oracle's seeds, equals oracle.frontier_search record for record."""
import math

import numpy as np
import pytest

import frontier_ref as FR
import frontier_search_maps as M


def test_restated_sort_equals_std_sort_on_doubles_with_duplicates():
    rng = np.random.default_rng(5)
    for n in list(range(0, 40)) + [63, 64, 65, 100, 257, 1000, 4096]:
        for _ in range(4):
            v = rng.integers(0, max(1, n // 4 + 1), size=n).astype(np.float64)
            ok, ids = FR.sort_check(v, 0)
            assert ok == 1, n
            np.testing.assert_array_equal(v[ids], np.sort(v, kind="stable"))


def test_restated_sort_equals_std_sort_with_the_reference_comparator():
    rng = np.random.default_rng(6)
    guarded = exact = 0
    for n in list(range(1, 48)) + [64, 100, 201, 401, 1024]:
        for trial in range(30):
            kind = trial % 3
            if kind == 0:                        # anywhere in [0, 2 pi), quadrant boundaries included
                v = rng.uniform(0, 2 * math.pi, size=n)
                v[rng.random(n) < 0.1] = math.pi / 2
                v[rng.random(n) < 0.1] = 3 * math.pi / 2
            elif kind == 1:                      # lattice directions: many exact ties
                v = np.array([math.atan2(a, b) % (2 * math.pi) for a, b in rng.integers(-3, 4, size=(n, 2)) if (a, b) != (0, 0)] or [0.0])
            else:                                # three angle ranges: a cycle for the comparator
                v = rng.choice(np.array([0.3, 2.0, 3.5, 5.0, 6.0]), size=n) + rng.uniform(0, 0.2, size=n)
            ok, _ = FR.sort_check(v, 1)
            assert ok in (1, -1), (n, trial)
            guarded += ok == -1
            exact += ok == 1
    # (an input on which std::sort would leave the array is detected by the guard and not compared: guarded counts them)
    assert exact > 500 and exact + guarded == 30 * 52


def _median_of_three_killer(n):
    """Musser's sequence: every median-of-three pivot is the second smallest, so the depth limit is reached."""
    k = n // 2
    a = np.zeros(n)
    for i in range(1, k + 1):
        if i % 2:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


def test_restated_sort_reaches_the_heap_sort_like_std_sort():
    for n in (32, 64, 100, 256, 512, 1000, 1024):
        v = _median_of_three_killer(n)
        ok, ids = FR.sort_check(v, 0)
        assert ok == 1
        np.testing.assert_array_equal(v[ids], np.sort(v))
        # the same permutation under the angle comparator (values scaled into the first two quadrants: a strict weak order there)
        w = v / (2.1 * n) * math.pi
        ok, _ = FR.sort_check(w, 1)
        assert ok == 1


def _check_against_oracle(oracle, name, cells, origin, res, pos, prm):
    mx, mn, lethal, max_d = prm
    r = oracle.frontier_search(cells, origin[:2], res, pos, lethal_threshold=lethal, min_cluster=mn, max_cluster=mx, max_distance=max_d)
    labels = FR.oracle_labels(r)
    seeds = FR.oracle_seeds(r)
    s = FR.search(labels, origin, res, M.robot_cell(cells, origin, res, pos), min_size=mn, max_size=mx, seeds=seeds)
    assert s is not None
    assert s["goals"].shape == r["goals"].shape, name
    np.testing.assert_array_equal(s["goals"].view(np.uint64), r["goals"].view(np.uint64), err_msg=name)   # bit for bit
    np.testing.assert_array_equal(s["sizes"], r["sizes"])
    np.testing.assert_array_equal(s["cell_piece"], r["cell_piece"])
    assert s["every_cells"].shape[0] == r["n_every"]
    assert s["guarded"] == 0
    return r, s


@pytest.mark.parametrize("prm", M.PARAMS)
def test_restatement_with_the_oracles_seeds_equals_the_oracle(oracle, prm):
    total = 0
    for name, cells, origin, res, pos in M.maps(large=False):
        r, _ = _check_against_oracle(oracle, name, cells, origin, res, pos, prm)
        total += r["goals"].shape[0]
    assert total > 50


def test_nearest_seeds_give_the_same_pieces_sizes(oracle):
    """Nearest seeds change which cell a piece's goal is, never how many records of which sizes a component yields."""
    for name, cells, origin, res, pos in M.maps(large=False)[:6]:
        r = oracle.frontier_search(cells, origin[:2], res, pos)
        s = FR.search(FR.oracle_labels(r), origin, res, M.robot_cell(cells, origin, res, pos))
        assert sorted(s["sizes"].tolist()) == sorted(r["sizes"].tolist()), name
        assert s["every_cells"].shape[0] == r["n_every"]


def test_refused_seeds():
    lab = np.full((8, 8), -1, np.int32)
    lab[2, 2:6] = 18
    assert FR.search(lab, (0, 0), 0.05, 0, seeds=[0]) is None            # not a frontier cell
    assert FR.search(lab, (0, 0), 0.05, 0, seeds=[18, 19]) is None       # two seeds in one component
    assert FR.search(lab, (0, 0), 0.05, 0, seeds=[19])["sizes"].tolist() == [4]
