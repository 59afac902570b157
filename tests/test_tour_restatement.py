"""The CPU restatement of FullPathOptimizer::getNextGoal (tests/tour_ref/tour_ref.cpp) on hand-built known
answers: every branch of getFilteredFrontiersN, the blacklist circle's strict edge, stable ties in path length, a tour tie decided
by the robot leg, the all-penalty list, and the reference's tour loop against a Held-Karp optimum.  Also: the library exports the
new entry point, and it refuses a null context without a device."""
import numpy as np
import pytest

import roadmap_ref as R
import tour_ref as T

RES = 0.05
ORIGIN = (-1.0, -1.0, 0.0)


def _sel(plm, n_local=5, radius=12.0, elig=None):
    plm = np.asarray(plm, dtype=np.float64)
    el = np.ones(plm.shape[0], np.uint8) if elig is None else np.asarray(elig, np.uint8)
    return T.select(plm, el, n_local, radius)


def test_all_local_at_most_n_drops_the_last_local():
    loc, glob, cg = _sel([1.0, 2.0, 3.0])
    assert (loc, glob, cg) == ([0, 1], [], 2)
    assert T.selection_codes(3, loc, glob, cg).tolist() == [1, 1, 4]


def test_more_than_n_locals_and_no_global():
    # the closest global is overwritten by every local beyond n: the last one
    loc, glob, cg = _sel([7.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert (loc, glob, cg) == ([1, 2, 3, 4, 5], [], 0)


def test_locals_and_globals():
    loc, glob, cg = _sel([1.0, 13.0, 2.0, 20.0])
    assert (loc, glob, cg) == ([0, 2], [1, 3], 1)
    assert T.selection_codes(4, loc, glob, cg).tolist() == [1, 6, 1, 2]


def test_more_than_n_locals_then_a_global():
    loc, glob, cg = _sel([1.0, 2.0, 3.0, 30.0], n_local=2)
    assert (loc, glob, cg) == ([0, 1], [3], 3)


def test_only_globals():
    loc, glob, cg = _sel([15.0, 13.0])
    assert (loc, glob, cg) == ([], [1, 0], 1)


def test_one_frontier_becomes_the_global():
    loc, glob, cg = _sel([3.0])
    assert (loc, glob, cg) == ([], [0], 0)


def test_nothing_eligible():
    assert _sel([1.0, 2.0], elig=[0, 0]) == ([], [], -1)
    assert _sel([]) == ([], [], -1)


def test_blacklist_circle_edge_is_not_inside():
    goal = np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 0.0]])
    assert T.eligible(goal, [1, 1], None, [[1.7, 0.0]]).tolist() == [1, 1]
    assert T.eligible(goal, [1, 1], None, [[1.6999, 0.0]]).tolist() == [0, 1]
    assert T.eligible(goal, [1, 1], [0, 1], None).tolist() == [1, 0]
    assert T.eligible(goal, [0, 1], None, None).tolist() == [0, 1]


def test_ties_in_path_length_go_to_the_lower_index():
    loc, glob, cg = _sel([2.0, 1.0, 1.0, 2.0, 1.0], n_local=3)
    assert (loc, glob, cg) == ([1, 2, 4], [], 3)


def _sym(entries, m):
    M = np.zeros((m, m))
    for (i, j), v in entries.items():
        M[i, j] = M[j, i] = v
    return M


def test_tour_tie_decided_by_the_robot_leg():
    # nodes R=0, A=1, B=2, G=3: A,B = 2 + 1 + 1 = 4 and B,A = 1 + 1 + 2 = 4; the robot leg picks B first (the later order)
    M = _sym({(0, 1): 2.0, (1, 2): 1.0, (2, 3): 1.0, (0, 2): 1.0, (1, 3): 2.0}, 4)
    L, cnt, perm, tried = T.tour(M)
    assert (L, cnt, perm, tried) == (4.0, 2, [1, 0], 2)
    assert T.held_karp(M) == 4.0


def test_equal_robot_legs_keep_the_first_order():
    M = _sym({(0, 1): 1.0, (0, 2): 1.0, (1, 2): 1.0, (1, 3): 1.0, (2, 3): 1.0}, 4)
    assert T.tour(M)[:3] == (3.0, 2, [0, 1])


def test_all_penalty_list_is_undetermined():
    """No roadmap node: every pair is charged, so getBestFullPath fails and the zero frontier is returned."""
    ref = R.Roadmap(np.zeros((40, 40), np.uint8), ORIGIN, RES)
    goal = np.array([[0.5, 0.5, 0.0], [0.9, 0.2, 0.0], [30.0, 30.0, 0.0]])
    out = T.next_goal(ref, (0.0, 0.0), goal, [1.0, 2.0, 40.0], [1, 1, 1])
    assert out["n_locals"] == 2 and out["status"] == T.UNDETERMINED and out["next_index"] == -1
    assert out["tour_length"] == 3 * 12.0 * 100000 and out["n_tied"] == 2
    assert (out["pair_length_m"][~np.eye(4, dtype=bool)] == 1.2e6).all()


def test_next_goal_on_a_small_roadmap():
    ref = R.Roadmap(np.zeros((200, 200), np.uint8), ORIGIN, RES, radius=3.0)
    nodes = [[0.0, 0.0], [2.0, 0.0], [4.0, 0.0], [2.0, 2.0], [6.0, 0.0]]
    ref.populate(nodes)
    ref.rebuild()
    goal = np.array([[4.0, 0.0, 0.0], [2.0, 2.0, 0.0], [6.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    out = T.next_goal(ref, (0.0, 0.0), goal, [4.0, 2.8, 6.0, 2.0], [1, 1, 1, 1], n_local=3)
    # locals by path length: 3 (2.0), 1 (2.8), 0 (4.0); 2 (6.0) is local beyond n, so it becomes the closest global
    assert out["selection"].tolist() == [1, 1, 4, 1]
    M = out["pair_length_m"]
    assert M[0, 1] == 2.0 and M[0, 3] == 4.0 and M[0, 4] == 6.0 and M[1, 2] == 2.0 and M[2, 4] == M[0, 2] + 2.0
    # two tours of 8.83 m: robot -> (2, 0) -> (2, 2) -> (4, 0) -> (6, 0) and robot -> (2, 2) -> (2, 0) -> ...; the robot leg decides
    assert out["n_tied"] == 2
    assert out["tour"].tolist() == [3, 1, 0, 2] and out["next_index"] == 3 and out["status"] == T.SAFE
    assert out["tour_length"] == 2.0 + 2.0 + M[0, 2] + 2.0


@pytest.mark.parametrize("k", range(1, 10))
def test_held_karp_equals_the_reference_loop(k):
    rng = np.random.default_rng(100 + k)
    for trial in range(3):
        A = rng.uniform(0.5, 20.0, (k + 2, k + 2))
        if trial == 2:
            A = np.round(A)                                   # many ties
        M = np.triu(A, 1) + np.triu(A, 1).T
        if trial == 1:
            M[1, 2] = M[2, 1] = 12.0 * 100000                # a penalty pair
        L, cnt, perm, tried = T.tour(M)
        assert tried == np.prod(range(1, k + 1))
        assert sorted(perm) == list(range(k)) and cnt >= 1
        assert T.tour_length(M, perm) == L
        assert T.held_karp(M) == L


def test_library_exports_the_entry_point(fs):
    lib = fs.load_library()
    assert "fs_roadmap_next_goal" in fs.capi.EXPORTED_SYMBOLS
    assert hasattr(lib, "fs_roadmap_next_goal")
    assert lib.fs_roadmap_next_goal(None, None, 0, None, None, None, None, 0, None, 5, 12.0, None, 0.0,
                                    None, None, None, None, None, None, None, None) == fs.capi.FS_E_INVALID
