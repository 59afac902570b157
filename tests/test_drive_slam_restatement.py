"""The gated drive's restatement (tests/drive_slam_ref.py) on the episode test's 96 x 96 world, staged all unknown, with the 400
landmarks of `wall_cloud`: the table of DESIGN.md 4.25 (figures worked out once with a prototype and held here as numbers), what
every gated drive must hold, and the restatement's information against the CPU oracle's pose_information on the subset discovered
at that step.  No GPU.

Robot 0 of most cases drives east along row 22 under the north wall, looking at it: 260 landmarks sit in the wall's western half,
none in its eastern half, so the information of its stations falls 91.0, 82.7, 70.9, 51.4, 42.9, 28.0, 0, 0.  The threshold of
a case lies midway between two of those (`between`), taken from the UNGATED drive."""
import numpy as np
import pytest

import drive_ref as DR
import drive_slam_ref as DS
import occlusion_ref as OR
import sense_ref as SR
import test_drive_restatement as TR
import test_gpu_explore_episode as EP

CLOUD = DS.wall_cloud(EP.ORIGIN, EP.RES)
_RESULTS = {}


def cases():
    n_yaw, _, k = SR.fan_shape(EP.PARAMS)
    return DS.table_cases(EP.ORIGIN, EP.RES, (n_yaw, k))


def run(oracle, table, case, **over):
    c = dict(case, **over)
    return DS.drive_slam_ref(oracle, table, TR.STAGED, TR.WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, c["poses"], c["goals"], CLOUD, known=c["known"],
                             first_ray=c["first_ray"], lm_sensor=c["lm_sensor"], fim=DS.FIM, occlusion=c["occlusion"],
                             stop_when_mapped=c["stop_when_mapped"], threshold=c.get("threshold", DS.DEFAULT_THRESHOLD), gate=c["gate"],
                             gate_first_station=c["gate_first_station"])


def result(oracle, table, name):
    """(the case's threshold, drive_slam_ref of the case, the ungated drive), computed once and shared (read-only)"""
    if name not in _RESULTS:
        case = cases()[name]
        free = run(oracle, table, case, gate=False)
        r, hi, lo = case["between"]
        thr = DS.threshold_between(free["information"], free["information"][r][lo], free["information"][r][hi])
        _RESULTS[name] = (thr, run(oracle, table, case, threshold=thr), free)
    return _RESULTS[name]


# name: status, reached, voxels per robot, in_view per robot, n_new, n_discovered, n_seen, n_revealed
A_VOX, A_VIEW = [14, 13, 11, 8, 7, 5, 0, 0], [283, 277, 274, 270, 263, 260, 213, 156]
B_VOX, B_VIEW = [32, 31, 28, 22, 15], [296, 291, 286, 278, 203]
TABLE = {
    "unsafe": ([5, 0], [4, 4], [A_VOX[:5] + [0] * 3, B_VOX], [A_VIEW[:5] + [-1] * 3, B_VIEW], 296, 296, 8106, 2400),
    "gate_off": ([0, 0], [7, 4], [A_VOX, B_VOX], [A_VIEW, B_VIEW], 296, 296, 11922, 2696),
    "first_station_6": ([5, 0], [6, 4], [A_VOX, B_VOX], [A_VIEW[:7] + [-1], B_VIEW], 296, 296, 10651, 2543),
    "no_line_of_sight": ([5, 0], [4, 4], [A_VOX[:5] + [0] * 3, B_VOX], [A_VIEW[:5] + [-1] * 3, B_VIEW], 296, 296, 8106, 2400),
    "mapped_wins": ([4, 0], [5, 4], [A_VOX, B_VOX], [A_VIEW[:6] + [-1] * 2, B_VIEW], 296, 296, 2243, 1174),
    "min_views_2": ([5, 0], [3, 3], [[14, 13, 11, 8], [22, 26, 21, 16]], [[283, 277, 274, 270], [280, 276, 274, 267]], 280, 280, 6431, 2328),
    "discovered_by_the_other": ([0, 0], [4, 4], [[0, 0, 0, 6, 6], [0, 0, 0, 12, 16]], [[0, 1, 0, 155, 246], [7] * 5], 254, 254, 8071, 2285),
    "occluded_after_the_merge": ([0, 0], [2, 1], [[24, 22, 22], [32, 31]], [[80] * 3, [296, 291]], 376, 376, 794, 548),
    "known": ([5, 0], [4, 4], [A_VOX[:5] + [0] * 3, [29, 26, 24, 19, 13]], [[23, 9, 0, 0, 0, -1, -1, -1], [15, 6, 0, 0, 0]], 23, 157, 8106, 2400),
    "uneven_and_blocked": ([5, 0, 1], [4, 0, 0], [A_VOX[:5] + [0] * 3, [32], [0] * 4], [A_VIEW[:5] + [-1] * 3, [296], [51, -1, -1, -1]],
                           296, 296, 6752, 2423),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_table(oracle, ref_table, name):
    thr, r, free = result(oracle, ref_table, name)
    status, reached, voxels, in_view, n_new, n_disc, n_seen, n_revealed = TABLE[name]
    assert (list(r["status"]), list(r["reached"])) == (status, reached)
    assert [list(v) for v in r["voxels"]] == voxels and [list(v) for v in r["in_view"]] == in_view
    assert (r["n_new"], r["n_discovered"], r["n_seen"], r["n_revealed"]) == (n_new, n_disc, n_seen, n_revealed)


def test_what_the_cases_are_about(oracle, ref_table):
    thr, u, free = result(oracle, ref_table, "unsafe")
    np.testing.assert_allclose(free["information"][0], [91.00, 82.75, 70.86, 51.38, 42.92, 27.95, 0.0, 0.0], atol=0.01)
    assert 42.92 < thr < 51.38 and u["status"][0] == DS.UNSAFE and u["reached"][0] == 4
    # a stopped robot's later stations report 0, 0 and -1, and the stations before the stop what the ungated drive reports
    assert not u["information"][0][5:].any() and list(u["station_status"][0][5:]) == [-1] * 3
    np.testing.assert_array_equal(u["information"][0][:5], free["information"][0][:5])
    g = result(oracle, ref_table, "gate_off")[1]
    for k in ("information", "voxels", "in_view"):
        for x, y in zip(g[k], free[k]):
            np.testing.assert_array_equal(x, y)
    assert result(oracle, ref_table, "first_station_6")[1]["information"][0][5] < thr     # it passed stations 4 and 5 below the threshold
    # without line of sight the sensor also discovers the 40 landmarks behind the wall; nobody in row 22 has them in view
    nl = result(oracle, ref_table, "no_line_of_sight")[1]
    assert nl["n_discovered"] == u["n_discovered"] and (nl["views"][360:] == 0).all()
    m = result(oracle, ref_table, "mapped_wins")
    assert m[1]["information"][0][5] < m[0] < m[1]["information"][0][4] and m[1]["status"][0] == DR.MAPPED   # UNSAFE by the numbers, MAPPED by the rule
    assert SR.goals_mapped_ref(m[1]["grid_at"][5][0], EP.ORIGIN, EP.RES, np.asarray(cases()["mapped_wins"]["goals"])[:1])[0]
    assert not SR.goals_mapped_ref(m[1]["grid_at"][4][0], EP.ORIGIN, EP.RES, np.asarray(cases()["mapped_wins"]["goals"])[:1])[0]
    # min_views 2: nothing was known, and both robots are scored at step 0 against what their two sightings discovered
    mv = result(oracle, ref_table, "min_views_2")[1]
    assert mv["information"][0][0] > 90.0 and mv["information"][1][0] > 90.0 and mv["flags_at"][0].sum() > 200
    assert (mv["views"][mv["flags_at"][0]] >= 2).all()
    # robot 0 discovers the stretch at step 3; robot 1, parked, has it in its FIM volume from the start
    d = result(oracle, ref_table, "discovered_by_the_other")[1]
    assert list(d["information"][1][:3]) == [0.0, 0.0, 0.0] and d["information"][1][3] > 60.0 and (d["in_view"][1] == 7).all()
    assert d["flags_at"][2].sum() < 10 < 100 < d["flags_at"][3].sum()
    # parked, same pose, same discovered set at steps 0 .. 2: the drop at step 1 is the wall the merge of step 1 put on the map
    o = result(oracle, ref_table, "occluded_after_the_merge")[1]
    i0 = o["information"][0]
    assert i0[0] > i0[1] == i0[2] and (o["flags_at"][0] == o["flags_at"][2]).all()
    assert (o["grid_at"][0][0, :20, 47] == 255).all() and (o["grid_at"][1][0, :20, 47] == 254).sum() >= 3
    kn = result(oracle, ref_table, "known")
    assert kn[1]["n_discovered"] - kn[1]["n_new"] == 134 and kn[1]["information"][0][0] > 0.0
    ub = result(oracle, ref_table, "uneven_and_blocked")[1]
    assert ub["status"][2] == DR.BLOCKED and ub["views"].sum() == sum(int(v[v >= 0].sum()) for v in ub["in_view"])   # a stopped robot adds no sightings


@pytest.mark.parametrize("name", sorted(TABLE))
def test_information_equals_the_oracle_on_the_discovered_subset(oracle, ref_table, name):
    thr, r, free = result(oracle, ref_table, name)
    case = cases()[name]
    for rb, poses in enumerate(case["poses"]):
        for k in range(poses.shape[0]):
            if free["station_status"][rb][k] == -1:
                assert (free["information"][rb][k], free["voxels"][rb][k], free["in_view"][rb][k]) == (0.0, 0, -1)
                continue
            sub = CLOUD[free["flags_at"][k]]
            if case["occlusion"] is None:
                want = oracle.pose_information(ref_table, sub, poses[k:k + 1], DS.FIM[0], DS.FIM[1])
            else:
                G = oracle.Grid(free["grid_at"][k], origin=EP.ORIGIN, resolution=EP.RES)
                want = OR.occluded_pose_information(oracle, ref_table, G, sub, poses[k:k + 1], DS.FIM[0], DS.FIM[1], **case["occlusion"])
            assert free["voxels"][rb][k] == want["n_voxels"][0], (rb, k)
            np.testing.assert_allclose(free["information"][rb][k], want["info_f64"][0], rtol=1e-12, atol=0.0, err_msg=f"robot {rb} station {k}")
