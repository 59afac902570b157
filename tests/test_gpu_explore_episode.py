"""A closed exploration loop on one device: search -> score and rank -> go to the best candidate -> SENSE there with the window its
argmax names -> the staged map has changed because of a decision the library took.

A twin context runs the same loop with the host route: tests/sense_ref.py's merged window sent through fs_update_grid_region.
After every tick the two staged grids, the rankings and the chosen goals are equal, and the explored-cell census never goes down
and equals numpy's count.

The tick's goal ends as the reference ends goals: CheckIfGoalMapped -> surroundingCellsMapped (fs_goals_mapped) says it is done;
a goal the sweep left unmapped is given up and blacklisted for the ticks after it.  The episode stops when no frontier, or no
achievable candidate, is left, or after 40 ticks."""
import numpy as np
import pytest

import sense_ref as SR

pytestmark = pytest.mark.gpu

N, RES, MAX_TICKS = 96, 0.05, 40
ORIGIN = (-N * RES / 2, -N * RES / 2, 0.0)
PARAMS = dict(max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, n_rays=0, elev=(0.0,), obst=(240, 254), trace=(255, 255),
              polygon=(-1e300, -1e300, 1e300, 1e300))


def _world():
    """rooms behind walls with doors; the outer wall closes the map"""
    w = np.zeros((N, N), dtype=np.uint8)
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = 254
    w[:, 47:49] = 254
    w[20:27, 47:49] = 0
    w[70:76, 47:49] = 0                                                # two doors in the north-south wall
    w[44:46, :] = 254
    w[44:46, 12:18] = 0
    w[44:46, 60:67] = 0                                                # one door in each half of the east-west wall
    w[60:62, 49:80] = 254                                              # a wall that ends in the open
    return w[None]


def _tick(s, robot, black):
    """one scoring tick: (frontier records, goals [n][3], costs dict, blacklist column) or None when no frontier is left"""
    fr, _ = s.search_frontiers(robot, want_every=False)
    if fr.shape[0] == 0:
        return None
    goals = np.stack([fr["goal_x"], fr["goal_y"], np.zeros(fr.shape[0])], 1)
    bl = np.array([(float(g[0]), float(g[1])) in black for g in goals], dtype=np.uint8)
    length = np.hypot(goals[:, 0] - robot[0], goals[:, 1] - robot[1])
    costs = s.get_frontier_costs(goals, length, np.zeros(fr.shape[0]), frontier_size=fr["size"], blacklisted=bl)
    return fr, goals, costs, bl


def _best(costs, bl):
    rec = costs["records"]
    for c in costs["order"]:
        if not bl[c] and (rec["flags"][c] & 1) and ((rec["flags"][c] >> 8) & 0xFF) == 0 and costs["weighted_cost"][c] < 1e300:
            return int(c)
    return -1


def test_episode_on_the_device_equals_the_host_route(fs):
    world = _world()
    start = (-1.2 + RES / 2, -1.5 + RES / 2, 0.0)
    sx, sy = int((start[0] - ORIGIN[0]) / RES), int((start[1] - ORIGIN[1]) / RES)
    assert world[0, sy, sx] == 0
    host = np.full_like(world, 255)                                    # the twin's master grid
    a, b = fs.FrontierScorer(device=0), fs.FrontierScorer(device=0)
    try:
        for s in (a, b):
            s.set_ray_params(robot_radius=0.15, **PARAMS)
            s.upload_grid(host, ORIGIN, RES)
            mx = s.max_arrival()
            s.set_arrival_limits(mx["max_gt"], 0.0)                    # (no lower limit: a fan half behind a wall is still a goal)
        a.upload_world(world)

        def sweep(pose, first):
            """the device route on a, the host route on b; returns a's result"""
            got = a.sense([pose], None if first is None else [first], rays=True)
            want = SR.sense_ref(host, world, ORIGIN, RES, PARAMS, [pose], None if first is None else [first])
            for k in ("status", "seen_unknown", "ray_unknown"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            assert (got["n_seen"], got["n_revealed"], got["window"]) == (want["n_seen"], want["n_revealed"], tuple(int(v) for v in want["window"]))
            host[:] = want["grid"]
            x0, y0, z0, wx, wy, wz = want["window"]
            if wx:
                b.update_grid_region(x0, y0, z0, host[z0:z0 + wz, y0:y0 + wy, x0:x0 + wx])
            return got

        known = a.grid_census()["known"]
        assert known == 0
        first = sweep(start, None)                                     # tick 0: the whole fan from the start cell
        assert first["n_revealed"] >= 1 and host[0, sy, sx] == world[0, sy, sx]
        robot, black, ticks, done, revealed = start[:2], set(), 0, 0, first["n_revealed"]
        while ticks < MAX_TICKS:
            ga, gb = a.read_grid_region(), b.read_grid_region()
            np.testing.assert_array_equal(ga, host)
            np.testing.assert_array_equal(gb, host)
            census = a.grid_census()
            assert census == SR.census_ref(host) == b.grid_census()
            assert census["known"] >= known and census["known"] == int((host != 255).sum())
            known = census["known"]
            ta, tb = _tick(a, robot, black), _tick(b, robot, black)
            assert (ta is None) == (tb is None)
            if ta is None:
                break
            np.testing.assert_array_equal(ta[0], tb[0])
            for k in ("records", "weighted_cost", "arrival_utility", "distance_utility", "order"):
                np.testing.assert_array_equal(ta[2][k], tb[2][k], err_msg=k)
            c = _best(ta[2], ta[3])
            assert c == _best(tb[2], tb[3])
            if c < 0:
                break
            ticks += 1
            goal = ta[1][c]
            rec = ta[2]["records"][c]
            got = sweep(tuple(goal), int(rec["argmax"]))
            assert got["status"][0] == SR.OK
            # the prediction against what was seen: nothing hid behind the staged map that the world does not hide too
            assert got["seen_unknown"][0] <= rec["arrival"]
            revealed += got["n_revealed"]
            mapped = a.goals_mapped([goal])
            np.testing.assert_array_equal(mapped, b.goals_mapped([goal]))
            np.testing.assert_array_equal(mapped, SR.goals_mapped_ref(host[0], ORIGIN, RES, [goal]))
            if mapped[0]:
                done += 1
            else:
                black.add((float(goal[0]), float(goal[1])))
            gx, gy = int((goal[0] - ORIGIN[0]) / RES), int((goal[1] - ORIGIN[1]) / RES)
            if world[0, gy, gx] == 0:                                  # (the robot does not stand inside a wall)
                robot = (float(goal[0]), float(goal[1]))
        print(f"episode: {ticks} ticks, {done} goals mapped, {len(black)} given up, {known} of {host.size} cells known")
        assert ticks >= 5 and done >= 1
        assert a.grid_census()["known"] == revealed == int((host != 255).sum()) > 1000
        assert (host == world)[host != 255].all()
    finally:
        a.close(); b.close()
