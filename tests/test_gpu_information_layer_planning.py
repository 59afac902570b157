"""The information layer does its job: on a map whose short route leads through a door with few landmarks near it,
fs_plan_paths_information takes that door and reports an unsafe way point; after fs_information_layer on the inflated map it takes
the other door, every way point safe, on a longer path.  tests/test_information_layer_restatement.py holds the same scenario on
the CPU (planner_ref, the oracle, the restatement) and every way point's value at least 5 % away from the threshold."""
import numpy as np
import pytest

import information_layer_ref as L
import inflation_ref as I

pytestmark = pytest.mark.gpu


def _plan(sc):
    out = sc.plan_paths_information(L.scene_pose(L.SCENE_ROBOT), L.scene_goal(), sample_distance=L.SCENE_PATH["sample_distance_m"],
                                    lookahead=L.SCENE_PATH["lookahead_points"], fi_threshold=L.SCENE_THRESHOLD, want_waypoints=True)
    assert out["achievable"][0] == 1 and out["n_waypoints"][0] >= 8
    return out


def test_the_plan_moves_to_the_door_that_keeps_tracking(fs):
    cells, lm = L.scene()
    thr = L.SCENE_THRESHOLD
    sc = fs.FrontierScorer(device=0)
    try:
        sc.upload_grid(cells, L.SCENE_ORIGIN, L.RES)
        sc.upload_landmarks(lm)
        sc.lookup_generate()
        sc.set_fim_params(*L.SCENE_VIS)
        sc.inflate(*L.SCENE_INFLATION)
        inflated = sc.read_grid_region()[0]
        np.testing.assert_array_equal(inflated, I.inflate_exact(cells, L.SCENE_INFLATION)[0])
        before = _plan(sc)
        assert L.door_of(before["waypoint_pose7"][:, :2]) == "A" and before["first_unsafe"][0] >= 0 and before["info_min"][0] < thr
        res = sc.information_layer(info_lo=thr, info_hi=2.0 * thr, **L.SCENE_LAYER)
        assert res.n_changed > 0 and res.n_scored > 256
        after = _plan(sc)
        assert L.door_of(after["waypoint_pose7"][:, :2]) == "B" and after["first_unsafe"][0] == -1 and after["info_min"][0] > thr
        assert after["path_length_m"][0] > 1.5 * before["path_length_m"][0]
        # the layer only raised costs, and only of writable cells
        grid = sc.read_grid_region()[0]
        assert (grid >= inflated).all() and np.array_equal(grid[inflated > 252], inflated[inflated > 252])
    finally:
        sc.close()
