"""The closed loop of tests/test_gpu_explore_episode.py with the Fisher half switched on: the staged MAP grows
through fs_sense and the staged CLOUD through fs_sense_landmarks, both on the device, and each tick's choice — search, plan,
score with Fisher information, rank, prefer the poses SLAM could keep tracking at (isPoseSafe's question, asked here of
n_visible) — depends on both.

A twin context runs beside it on the host route: tests/sense_ref.py's merged window through fs_update_grid_region and the set
tests/landmark_sense_ref.py computes through fs_upload_landmarks ("cloud.order" 2).  After every tick the two agree on the
frontier records, the scored records (info columns included), costs, order, the chosen goal, the census and n_discovered.  A third
context gets the same maps but keeps the initial cloud: at least one tick must rank differently there, or the landmark half of
the loop shows nothing.

The device predicate is fp32; the poses of an episode are not known beforehand, so no borderline landmark can be dropped from the
world in advance.  Instead each tick holds the device's sightings (the counters' increments) against the restatement everywhere
outside the 1e-5 band, and the restatement takes the device's verdict inside it."""
import numpy as np
import pytest

import landmark_sense_ref as LR
import sense_ref as SR

pytestmark = pytest.mark.gpu

N, RES, MAX_TICKS = 96, 0.05, 40
ORIGIN = (-N * RES / 2, -N * RES / 2, 0.0)
PARAMS = dict(max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, n_rays=0, elev=(0.0,), obst=(240, 254), trace=(255, 255),
              polygon=(-1e300, -1e300, 1e300, 1e300))
VOLUME = (2.0, 1.0)                                                    # the landmark sensor's and the scoring volume
SENSOR = dict(max_dist=VOLUME[0], max_angle=VOLUME[1], line_of_sight=1, min_views=1, occ=(254, 254), end_margin_m=0.3)
MIN_VISIBLE = 15                                                       # a pose with fewer map points in view is not "safe"


def _world():
    """rooms behind walls with doors; the outer wall closes the map (tests/test_gpu_explore_episode.py's)"""
    w = np.zeros((N, N), dtype=np.uint8)
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 254
    w[:, 47:49] = 254
    w[20:27, 47:49] = 0
    w[70:76, 47:49] = 0
    w[44:46, :] = 254
    w[44:46, 12:18] = 0
    w[44:46, 60:67] = 0
    w[60:62, 49:80] = 254
    return w[None]


def _world_cloud(world):
    """three points on every lethal cell of the world, anywhere inside the cell, up to a metre above the floor"""
    ys, xs = np.nonzero(world[0] == 254)
    rng = np.random.default_rng(8)
    pts = []
    for _ in range(3):
        px = ORIGIN[0] + (xs + rng.uniform(0.05, 0.95, size=xs.shape[0])) * RES
        py = ORIGIN[1] + (ys + rng.uniform(0.05, 0.95, size=ys.shape[0])) * RES
        pts.append(np.stack([px, py, rng.uniform(0.0, 1.0, size=xs.shape[0])], 1))
    return np.concatenate(pts).astype(np.float32)


def _ranking(costs, black_mask):
    """achievable candidates in cost order, the safe ones (enough landmarks in view) first"""
    rec = costs["records"]
    ok = [int(c) for c in costs["order"]
          if not black_mask[c] and (rec["flags"][c] & 1) and ((rec["flags"][c] >> 8) & 0xFF) == 0 and costs["weighted_cost"][c] < 1e300]
    return [c for c in ok if rec["n_visible"][c] >= MIN_VISIBLE] + [c for c in ok if rec["n_visible"][c] < MIN_VISIBLE]


def test_episode_with_landmarks_equals_the_host_route(fs, oracle):
    world = _world()
    cloud = _world_cloud(world)
    assert 2000 <= cloud.shape[0] <= 6000
    G_world = oracle.Grid(world, origin=ORIGIN, resolution=RES)
    start = (-1.2 + RES / 2, -1.5 + RES / 2, 0.0)
    host = np.full_like(world, 255)
    ref = LR.WorldCloud(oracle, cloud)
    a, b, c = (fs.FrontierScorer(device=0) for _ in range(3))
    try:
        for s in (a, b, c):
            s.lookup_generate()
            s.set_ray_params(robot_radius=0.15, **PARAMS)
            s.set_fim_params(*VOLUME)
            s.upload_grid(host, ORIGIN, RES)
            mx = s.max_arrival()
            s.set_arrival_limits(mx["max_gt"], 0.0)
        for s in (b, c):
            s.set_option("cloud.order", 2)
        a.upload_world(world)
        a.upload_world_landmarks(cloud)
        assert a.world_landmarks()["n_discovered"] == 0

        def sweep(pose7, first, twins):
            """grid and cloud: the device route on a, the host route on `twins`"""
            origin = tuple(pose7[:3])
            got = a.sense([origin], None if first is None else [first], rays=False)
            want = SR.sense_ref(host, world, ORIGIN, RES, PARAMS, [origin], None if first is None else [first])
            np.testing.assert_array_equal(got["status"], want["status"])
            assert (got["n_seen"], got["n_revealed"], got["window"]) == (want["n_seen"], want["n_revealed"], tuple(int(v) for v in want["window"]))
            host[:] = want["grid"]
            x0, y0, z0, wx, wy, wz = want["window"]
            if wx:
                for t in twins:
                    t.update_grid_region(x0, y0, z0, host[z0:z0 + wz, y0:y0 + wy, x0:x0 + wx])
            before = a.world_landmarks()["views"]
            lm = a.sense_landmarks(pose7[None], SENSOR)
            seen_dev = (a.world_landmarks()["views"] - before) > 0
            S = LR.sees(oracle, G_world, pose7[None], cloud, SENSOR)
            border = LR.borderline(oracle, pose7[None], cloud, [VOLUME])
            np.testing.assert_array_equal(seen_dev[~border], S[0][~border])
            S[0][border] = seen_dev[border]
            wantl = ref.sense(G_world, pose7[None], SENSOR, S=S)
            np.testing.assert_array_equal(lm["n_in_view"], wantl["n_in_view"])
            assert (lm["n_new"], lm["n_discovered"]) == (wantl["n_new"], wantl["n_discovered"])
            np.testing.assert_array_equal(a.world_landmarks()["world_index"], ref.world_index)
            return got, lm

        pose0 = oracle.poses_from_yaw(np.array([start]), np.array([0.0]))[0]
        _, lm0 = sweep(pose0, None, (b, c))                            # tick 0: the whole fan, and what the camera sees of the cloud
        assert lm0["n_discovered"] > 0
        initial = ref.discovered.copy()
        b.upload_landmarks(initial); c.upload_landmarks(initial)
        robot, black, ticks, n_disc, differs = pose0.copy(), [], 0, [lm0["n_discovered"]], 0
        while ticks < MAX_TICKS:
            assert a.grid_census() == b.grid_census() == SR.census_ref(host)
            bl = np.array(black, dtype=np.float64).reshape(-1, 2) if black else None
            (fa, ca), (fb, cb), (fc, cc) = (s.get_frontier_costs_searched(robot, blacklist_xy=bl, allow_unknown=True, with_fim=True) for s in (a, b, c))
            assert fa.tobytes() == fb.tobytes() == fc.tobytes()
            if fa.shape[0] == 0:
                break
            for k in ("weighted_cost", "arrival_utility", "distance_utility", "order", "path_length_m"):
                assert ca[k].tobytes() == cb[k].tobytes(), f"{k}, tick {ticks}"
            # the records: every integer and the yaw exactly.  The fused call's Fisher float sums are not bit-stable from one call to
            # the next on ONE context (tests/test_gpu_frontier_search.py holds two such calls to rtol 1e-5 for that reason), so two
            # contexts are held to the same 1e-5; the staged bytes themselves are compared in tests/test_gpu_landmark_sense.py
            for f in ca["records"].dtype.names:
                if f in ("info_ref", "trace", "logdet"):
                    np.testing.assert_allclose(ca["records"][f], cb["records"][f], rtol=1e-5, err_msg=f"{f}, tick {ticks}")
                else:
                    assert ca["records"][f].tobytes() == cb["records"][f].tobytes(), f"{f}, tick {ticks}"
            bmask = np.array([any(g["goal_x"] == p[0] and g["goal_y"] == p[1] for p in black) for g in fa], dtype=bool)
            ra, rb, rc = _ranking(ca, bmask), _ranking(cb, bmask), _ranking(cc, bmask)
            assert ra == rb
            differs += ra != rc
            if not ra:
                break
            ticks += 1
            k = ra[0]
            goal = np.array([fa["goal_x"][k], fa["goal_y"][k], 0.0])
            rec = ca["records"][k]
            pose = oracle.poses_from_yaw(goal[None], np.array([float(rec["yaw"])]))[0]
            got, lm = sweep(pose, int(rec["argmax"]), (b, c))
            assert got["status"][0] == SR.OK
            n_disc.append(lm["n_discovered"])
            if lm["n_new"]:
                b.upload_landmarks(ref.discovered)
            mapped = a.goals_mapped([goal])
            np.testing.assert_array_equal(mapped, b.goals_mapped([goal]))
            if not mapped[0]:
                black.append((float(goal[0]), float(goal[1])))
            gx, gy = int((goal[0] - ORIGIN[0]) / RES), int((goal[1] - ORIGIN[1]) / RES)
            if world[0, gy, gx] == 0:                                  # (the robot does not stand inside a wall)
                robot = pose
        print(f"episode: {ticks} ticks, {len(black)} goals given up, discovered {n_disc[0]} -> {n_disc[-1]} of {cloud.shape[0]}, "
              f"{differs} ticks ranked differently with the initial cloud")
        assert ticks >= 5
        assert all(x <= y for x, y in zip(n_disc, n_disc[1:])) and n_disc[-1] > n_disc[0]
        assert differs >= 1
    finally:
        a.close(); b.close(); c.close()
