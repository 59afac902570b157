"""tests/landmark_sense_ref.py — the numpy restatement of fs_sense_landmarks — on the occlusion fixture: a 64 x 64
map with a wall and two doors, 3 000 landmarks, six poses.  No GPU.  Non-vacuity (the sensor sees part of the cloud, the line of
sight removes part of that, min_views 2 is a strict subset), monotonicity over calls, independence of the order of poses, and the
library's entry points being present at all."""
import numpy as np
import pytest

import landmark_sense_ref as LR
import occlusion_ref as OR

VOLUMES = [(14.0, 1.0), (6.0, 1.0)]


@pytest.fixture(autouse=True)
def _the_call_exists(fs):
    # (the helper restates a library call: without the call there is nothing to restate)
    assert "fs_sense_landmarks" in fs.capi.EXPORTED_SYMBOLS and callable(fs.FrontierScorer.sense_landmarks)


@pytest.fixture(scope="module")
def fix(oracle):
    G =oracle.Grid(OR.fixture_cells(), origin=OR.FIX_ORIGIN, resolution=OR.FIX_RES)
    poses = OR.fixture_poses(oracle)
    raw = OR.fixture_landmarks(3000)
    world = LR.drop_borderline(oracle, poses, raw, VOLUMES + [(6.0, 4.0)])
    assert raw.shape[0] - world.shape[0] <= 30
    return G, poses, world


def _sensor(vol, los=1, min_views=1):
    return dict(max_dist=vol[0], max_angle=vol[1], line_of_sight=los, min_views=min_views)


def test_borderline_landmarks_are_few(oracle):
    poses, raw = OR.fixture_poses(oracle), OR.fixture_landmarks(3000)
    for vol in VOLUMES:
        assert LR.borderline(oracle, poses, raw, [vol]).sum() <= 1


@pytest.mark.parametrize("vol", VOLUMES)
def test_the_sensor_sees_part_of_the_cloud(fix, oracle, vol):
    G, poses, world = fix
    m = world.shape[0]
    in_volume = LR.sees(oracle, None, poses, world, _sensor(vol, los=0))
    in_sight = LR.sees(oracle, G, poses, world, _sensor(vol, los=1))
    assert not (in_sight & ~in_volume).any()
    assert (in_sight.sum(axis=1) < in_volume.sum(axis=1)).all()         # the wall hides something from every pose
    assert 0 < in_sight.sum(axis=1).min() and in_volume.sum(axis=1).max() < m
    if vol == (14.0, 1.0):
        assert 5 <= in_sight.sum(axis=1).min() <= 20 and 1000 <= in_sight.sum(axis=1).max() <= 1030
        assert 1150 <= in_volume.sum(axis=1).min() and in_volume.sum(axis=1).max() <= 2230
    one = LR.WorldCloud(oracle, world); one.sense(G, poses, _sensor(vol, min_views=1))
    two = LR.WorldCloud(oracle, world); two.sense(G, poses, _sensor(vol, min_views=2))
    d1, d2 = set(one.world_index.tolist()), set(two.world_index.tolist())
    assert 0 < len(d2) < len(d1) < m and d2 < d1
    want = {(14.0, 1.0): (2048, 930), (6.0, 1.0): (1206, 279)}[vol]
    # (the figures of the whole 3 000-landmark cloud; the borderline landmarks dropped here move them by a few at most)
    assert abs(len(d1) - want[0]) <= 30 and abs(len(d2) - want[1]) <= 30


def test_discovered_set_is_monotone_over_calls(fix, oracle):
    G, poses, world = fix
    wc = LR.WorldCloud(oracle, world)
    before, total_new = set(), 0
    for k in range(poses.shape[0]):
        r = wc.sense(G, poses[k:k + 1], _sensor((6.0, 1.0), min_views=2 if k % 2 else 1))
        now = set(wc.world_index.tolist())
        assert before <= now and len(now) - len(before) == r["n_new"] and r["n_discovered"] == len(now)
        before, total_new = now, total_new + r["n_new"]
    assert total_new == len(before) > 0
    r = wc.sense(G, poses[:0], _sensor((6.0, 1.0)))                      # no pose: nothing changes
    assert r["n_new"] == 0 and set(wc.world_index.tolist()) == before


def test_discovered_set_does_not_depend_on_the_order_of_poses(fix, oracle):
    G, poses, world = fix
    a = LR.WorldCloud(oracle, world); ra = a.sense(G, poses, _sensor((14.0, 1.0), min_views=2))
    perm = np.array([3, 0, 5, 1, 4, 2])
    b = LR.WorldCloud(oracle, world); rb = b.sense(G, poses[perm], _sensor((14.0, 1.0), min_views=2))
    np.testing.assert_array_equal(a.world_index, b.world_index)
    np.testing.assert_array_equal(a.views, b.views)
    np.testing.assert_array_equal(ra["n_in_view"][perm], rb["n_in_view"])
    assert (ra["n_new"], ra["n_discovered"]) == (rb["n_new"], rb["n_discovered"])


def test_unusable_landmarks_keep_their_index_and_are_never_seen(fix, oracle):
    G, poses, world = fix
    w = world.copy()
    w[5] = (np.nan, 0.0, 0.0); w[17] = (np.inf, 1.0, 1.0); w[40] = (1.0e30, 0.0, 0.0)
    wc = LR.WorldCloud(oracle, w)
    wc.sense(G, poses, _sensor((14.0, 4.0), los=0))
    assert wc.views[[5, 17, 40]].tolist() == [0, 0, 0] and not wc.flag[[5, 17, 40]].any()
    assert wc.flag.sum() > 0
