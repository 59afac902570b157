"""The numpy restatement of the line-of-sight rule (tests/occlusion_ref.py) against the pure-Python walk of oracle/pyref.py on
random 2-D and 3-D segments, and the properties of the occlusion fixture that keep the GPU tests from passing vacuously.  No GPU."""
import numpy as np
import pytest

import occlusion_ref as OR

COSTS = np.array([0, 100, 253, 254, 255], dtype=np.uint8)


def _rule_from_pyref(pyref, cells, origin, res, s, w, occ, margin_m):
    """the rule spelt out on pyref.walk_cells' (x, y, z) cell list"""
    cm = pyref.Costmap(cells, origin, res)
    s, w = list(s), list(w)
    if cm.nz == 1:
        s[2] = w[2] = cm.oz
    walk = pyref.walk_cells(cm, s, w, 1.0e9)            # a cap no walk reaches: scale = 1
    if walk is None:
        return False, False, 0
    end = len(walk) - 1
    m = 1 + int(margin_m / res)
    tested = [cm.cost(*c) for v, c in enumerate(walk) if v + m <= end]
    return True, any(occ[0] <= c <= occ[1] for c in tested), len(tested)


@pytest.mark.parametrize("shape,res", [((1, 48, 40), 0.25), ((6, 24, 20), 0.1)])
def test_restatement_equals_the_python_walk(oracle, pyref, shape, res):
    rng = np.random.default_rng(shape[0])
    cells = rng.choice(COSTS, size=shape, p=[0.84, 0.04, 0.04, 0.04, 0.04])
    origin = (-1.5, 2.0, 0.5)
    G = oracle.Grid(cells, origin=origin, resolution=res)
    nz, ny, nx = shape
    hi = np.array([nx, ny, nz]) * res
    a = rng.uniform(-0.1 * hi, 1.1 * hi, size=(300, 3)) + origin        # some ends off the map
    b = rng.uniform(-0.1 * hi, 1.1 * hi, size=(300, 3)) + origin
    b[:20] = a[:20] + rng.uniform(-2 * res, 2 * res, size=(20, 3))      # shorter than the margin, equal cells
    b[20:40, 1] = a[20:40, 1]                                           # axis-aligned
    seen = set()
    for occ, margin in (((254, 254), 0.3), ((253, 254), 0.3), ((254, 254), 0.0)):
        got = OR.lines_of_sight(oracle, G, a, b, occ, margin)
        for i in range(a.shape[0]):
            want = _rule_from_pyref(pyref, cells, origin, res, a[i], b[i], occ, margin)
            assert (bool(got["ok"][i]), bool(got["blocked"][i]), int(got["tested_cells"][i])) == want, (i, occ, margin)
            seen.add(want[:2] + (want[2] == 0,))
    # every outcome occurs: off the map, shorter than the margin, blocked, clear
    assert {(False, False, True), (True, False, True), (True, True, False), (True, False, False)} <= seen


def test_the_start_cell_is_tested_and_the_far_end_is_not(oracle):
    cells = np.zeros((1, 8, 16), dtype=np.uint8)
    G = oracle.Grid(cells, origin=(0.0, 0.0, 0.0), resolution=0.25)
    s, w = (0.1, 0.1, 5.0), (3.9, 0.1, -3.0)                            # cells (0, 0) -> (15, 0); z is ignored on a 2-D grid
    assert OR.line_of_sight(oracle, G, s, w) == (True, False, 14)       # M = 1 + int(0.3 / 0.25) = 2: visits 0 .. 13
    cells[0, 0, 0] = 254
    assert OR.line_of_sight(oracle, G, s, w) == (True, True, 14)
    cells[0, 0, 0] = 0
    cells[0, 0, 14:] = 254                                              # the last M cells: not tested
    assert OR.line_of_sight(oracle, G, s, w) == (True, False, 14)
    cells[0, 0, 13] = 253
    assert OR.line_of_sight(oracle, G, s, w) == (True, False, 14)       # 253 does not occlude by default
    assert OR.line_of_sight(oracle, G, s, w, occ=(253, 254)) == (True, True, 14)
    assert OR.line_of_sight(oracle, G, s, w, end_margin_m=0.0) == (True, True, 15)
    assert OR.line_of_sight(oracle, G, s, (4.1, 0.1, 0.0)) == (False, False, 0)


@pytest.mark.parametrize("m", [3000, 5000])
def test_fixture_properties(oracle, ref_table, m):
    """What tests/test_gpu_occlusion.py relies on: for every pose the rule hides at least 20 % of the landmarks the predicate
    accepts and leaves at least 10; for at least one pose the 550 decision differs between on and off."""
    G = oracle.Grid(OR.fixture_cells(), origin=OR.FIX_ORIGIN, resolution=OR.FIX_RES)
    lm = OR.fixture_landmarks(m)
    poses = OR.fixture_poses(oracle)
    flipped = 0
    for angle in (1.0, 4.0):
        off = oracle.pose_information(ref_table, lm, poses, 14.0, angle)
        on = OR.occluded_pose_information(oracle, ref_table, G, lm, poses, 14.0, angle)
        assert (on["n_visible"] <= 0.8 * off["n_visible"]).all(), (angle, on["n_visible"], off["n_visible"])
        assert (on["n_visible"] >= 10).all()
        flipped += int(((on["info_ref"] > 550.0) != (off["info_ref"] > 550.0)).sum())
    # (per cloud, over its two runs: with 5 000 landmarks and the cone off every pose stays above 550 even occluded — the lowest,
    # the pose facing the wall, drops from 5 860 to 821 — and the decision flips under the 1.0 rad cone)
    assert flipped >= 1
