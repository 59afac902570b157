"""The sensor sweep's restatement (tests/sense_ref.py) held against what the reference PREDICTS for the same pose: arrival
information (oracle.arrival_information, the C restatement of setArrivalInformationForFrontier) on the staged map, with the
sweep looking where the prediction's best window looks.  No GPU.

The staged map equals the world except a region set to 255, so a staged obstacle is always a world obstacle: the world ray stops
no later than the staged ray, and every staged-unknown cell it counts the staged ray counts too —
    ray_unknown <= ray_counts inside the window,   seen_unknown <= arrival,
with equality when the world holds no obstacle cost under the staged-unknown region (both rays then stop at the same visit)."""
import numpy as np
import pytest

import sense_ref as SR


def _params(w):
    return dict(max_camera_depth=w.max_camera_depth, delta_theta=w.delta_theta, camera_fov=w.camera_fov, n_rays=w.n_yaw,
                elev=tuple(w.elev), obst=(240, 254), trace=(255, 255), polygon=tuple(w.polygon))


def _cases(fs):
    out = []
    for name, w in (("small61", fs.synth.make_small_2d(11, n=61, n_cand=24, n_landmarks=8)),
                    ("small96", fs.synth.make_small_2d(12, n=96, n_cand=24, n_landmarks=8)),
                    ("C1", fs.synth.make_workload("C1", n_cand=24, n_landmarks=8))):
        rng = np.random.Generator(np.random.PCG64(len(name) + w.cells.shape[1]))
        nz, ny, nx = w.cells.shape
        lo = [int(rng.integers(0, s // 2)) if s > 1 else 0 for s in (nz, ny, nx)]
        hi = [l + max(1, int(rng.integers(s // 4, s // 2 + 1))) for l, s in zip(lo, (nz, ny, nx))]
        region = np.zeros(w.cells.shape, dtype=bool)
        region[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        out.append((name, w, region))
    return out


@pytest.fixture(scope="module")
def cases(fs):
    return _cases(fs)


@pytest.mark.parametrize("clean", [False, True], ids=["walls_under_the_region", "no_obstacle_under_the_region"])
def test_sweep_never_sees_more_unknown_than_arrival_predicts(fs, oracle, cases, clean):
    for name, w, region in cases:
        world = w.cells.copy()
        if clean:
            world[region & (world >= 240) & (world <= 254)] = 0
        staged = world.copy()
        staged[region] = 255
        p = _params(w)
        rp = oracle.RayParams(max_camera_depth=p["max_camera_depth"], delta_theta=p["delta_theta"], camera_fov=p["camera_fov"],
                              n_rays=p["n_rays"], elev=p["elev"], obst=p["obst"], trace=p["trace"], polygon=p["polygon"])
        arr = oracle.arrival_information(oracle.Grid(staged, w.origin, w.resolution), rp, w.goals)
        n_yaw, n_elev, k = SR.fan_shape(p)
        assert arr["ray_counts"].shape == (w.goals.shape[0], n_elev, n_yaw)
        r = SR.sense_ref(staged, world, w.origin, w.resolution, p, w.goals, arr["argmax"])
        np.testing.assert_array_equal(r["status"], arr["status"])
        ok = np.nonzero(arr["status"] == 0)[0]
        assert ok.size >= 16, name
        for c in ok:
            f = int(arr["argmax"][c])
            inside, predicted = r["ray_unknown"][c][:, f:f + k], arr["ray_counts"][c][:, f:f + k]
            assert predicted.sum() == arr["arrival"][c]
            assert (r["ray_unknown"][c][:, :f] == 0).all() and (r["ray_unknown"][c][:, f + k:] == 0).all()
            assert r["seen_unknown"][c] == inside.sum()
            if clean:
                np.testing.assert_array_equal(inside, predicted, err_msg=f"{name} candidate {c}")
                assert r["seen_unknown"][c] == arr["arrival"][c]
            else:
                assert (inside <= predicted).all(), (name, c)
                assert r["seen_unknown"][c] <= arr["arrival"][c]
        # the merged map: world where seen, staged elsewhere; the counts and the window are those cells'
        seen = np.zeros(world.shape, dtype=bool)
        for (x, y, z) in r["seen"]:
            seen[z, y, x] = True
        np.testing.assert_array_equal(r["grid"], np.where(seen, world, staged))
        assert r["n_seen"] == int(seen.sum()) and r["n_revealed"] == int((seen & (staged == 255) & (world != 255)).sum())
        zz, yy, xx = np.nonzero(seen)
        assert r["window"] == (xx.min(), yy.min(), zz.min(), xx.max() - xx.min() + 1, yy.max() - yy.min() + 1, zz.max() - zz.min() + 1)
        # a second sweep of the merged map reveals nothing
        again = SR.sense_ref(r["grid"], world, w.origin, w.resolution, p, w.goals, arr["argmax"])
        assert again["n_revealed"] == 0 and again["n_seen"] == r["n_seen"]
        np.testing.assert_array_equal(again["grid"], r["grid"])


def _brute_mapped(cells, origin, res, goal):
    ny, nx = cells.shape
    if goal[0] < origin[0] or goal[1] < origin[1]:
        return 0
    cx, cy = int((goal[0] - origin[0]) / res), int((goal[1] - origin[1]) / res)
    if cx >= nx or cy >= ny:
        return 0
    if cells[cy, cx] == 254:
        return 1
    inside = lambda x, y: 0 <= x < nx and 0 <= y < ny
    ring = [(cx + dx, cy + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx or dy) and inside(cx + dx, cy + dy)]
    if sum(1 for (x, y) in ring if cells[y, x] == 254) >= 3:
        return 1
    # the up to 21 cells: the 5 x 5 block without its four corners, clipped at the map's edges
    block = {(cx + dx, cy + dy) for dx in range(-2, 3) for dy in range(-2, 3) if not (abs(dx) == 2 and abs(dy) == 2) and inside(cx + dx, cy + dy)}
    assert len(block) <= 21
    return 0 if any(cells[y, x] == 255 for (x, y) in block) else 1


def test_goals_mapped_ref_is_the_clipped_block_rule(fs):
    for seed, n in ((21, 61), (22, 96), (23, 7)):
        w = fs.synth.make_small_2d(seed, n=max(n, 24), n_cand=4, n_landmarks=4)
        cells = w.cells[0][:n, :n].copy()
        rng = np.random.default_rng(seed)
        cells[rng.random(cells.shape) < 0.05] = 254                     # enough lethal cells for the three-neighbour rule
        goals = SR.border_goals(n, n, w.origin, w.resolution, rng)
        got = SR.goals_mapped_ref(cells, w.origin, w.resolution, goals)
        want = np.array([_brute_mapped(cells, w.origin, w.resolution, g) for g in goals], dtype=np.uint8)
        np.testing.assert_array_equal(got, want)
        assert 0 < got.sum() < got.size
    c = SR.census_ref(cells)
    assert c["known"] + c["unknown"] == cells.size and c["lethal"] == int((cells == 254).sum()) and c["free"] == int((cells == 0).sum())


def test_first_ray_for_yaw_inverts_the_pose_yaw(fs):
    for dt, fov, n_rays in ((0.10, 1.04, 0), (2 * np.pi / 32, 1.04, 32), (0.05, 1.5, 0)):
        n_yaw = fs.capi.fan_n_yaw(dt, n_rays)
        assert n_yaw == SR.fan_shape(dict(delta_theta=dt, camera_fov=fov, n_rays=n_rays))[0]
        k = int(fov / dt)
        for i in range(n_yaw - k + 1):
            assert fs.capi.first_ray_for_yaw((i * dt) + (fov / 2), dt, fov, n_yaw) == i
        assert fs.capi.first_ray_for_yaw(-1.0, dt, fov, n_yaw) == 0
        assert fs.capi.first_ray_for_yaw(100.0, dt, fov, n_yaw) == n_yaw - k
