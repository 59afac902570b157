"""The robot-footprint disc of the arrival kernel (isRobotFootprintInLethal, DEP/src/Helpers.cpp:135-155; read only by
`if (lethal && frontier_size < 10) achievable = 0`, CostCalculator.cpp:77-82) against the oracle, bit for bit.

The kernel skips the scan when the frontier is too large for its result to be read and otherwise scans in groups of
independent loads, every lane loading in every pass (lanes without a disc cell read the start cell and discard it), so the
cases pin every one of those paths:

  grids       32 x 32 x 1 and 32 x 32 x 8
  walks       the byte walk and the class walk ("ray.layout" 1 and 2: FsRayArgs::layout 0 and 1), both on both grids
  discs       side 3 (one pass, most lanes without a cell), side 25 under a 4-ring fan (ten passes: several groups), side 33 under
              a 63-ray one-ring fan (eighteen passes, more than the fan has rounds; its last lane has no ray but its share of the
              disc; the disc hangs off the grid on every side)
  sizes       frontier_size 9, 10, 11 and absent (the kernel then scans, as with 0), each also with achievable_in = 0
  254 cells   inside the disc / exactly on the radius / just outside it (inside the scanned square) / only in another z slice (the
              8-slice grid; a one-slice grid has no other slice) / the start cell in the grid's corner with the 254 cell where a
              row-major read of the disc's off-grid part would wrap to / the same corner with a 254 cell inside the disc
  and         a blacklisted and an off-map candidate in every list (two workgroups per launch)

Every integer field — status, arrival, argmax, achievable, and the per-ray counts where the entry point returns them — must
equal oracle.arrival_information, from fs_score_candidates and from the arrival-only fs_score_arrival.
test_inputs_exercise_the_rule (no GPU) holds the inputs to their purpose: the oracle alone yields both achievable values in
every size class, and the lethal verdict each placement was built for.
"""
import functools

import numpy as np
import pytest

RES = 0.05
SIZES = (9, 10, 11, None)
# (side, rings, n_rays): n_rays 0 = the reference's accumulated 0.10 steps, 63 rays
DISCS = {3: ((-0.30, -0.10, 0.10, 0.30), 64), 25: ((-0.30, -0.10, 0.10, 0.30), 64), 33: ((0.0,), 0)}


def _just_outside(ri):
    """the cell of the scanned square nearest to the radius from outside: smallest dx^2 + dy^2 > ri^2 with |dx|, |dy| <= ri"""
    best = min((dx * dx + dy * dy, dx, dy) for dx in range(-ri, 1) for dy in range(0, ri + 1) if dx * dx + dy * dy > ri * ri)
    return best[1], best[2]


def _placements(nz, ri):
    """name -> (start cell (x, y, z), [254 cells], the verdict the placement was built for)"""
    cx, cy, cz = 16, 16, (3 if nz > 1 else 0)
    ox, oy = _just_outside(ri)
    p = {"inside": ((cx, cy, cz), [(cx + ri // 2, cy - ri // 3, cz)], True),
         "on_radius": ((cx, cy, cz), [(cx - ri, cy, cz)], True),
         "just_outside": ((cx, cy, cz), [(cx + ox, cy + oy, cz)], False),
         # start (0, 31): disc cell (-1, 31) read row-major without the off-grid rule is cell (31, 30)
         "corner_wrap_bait": ((0, 31, cz), [(31, 30, cz)], False),
         "corner_inside": ((0, 31, cz), [(min(ri, 1), 31 - ri // 2, cz)], True)}
    if nz > 1:
        p["other_slice"] = ((cx, cy, cz), [(cx, cy, cz + 1), (cx + ri // 2, cy, cz - 1)], False)
    return p


@functools.lru_cache(maxsize=None)
def _case(nz, side):
    """The inputs and the oracle's answers of one (grid, disc): computed once, shared by the walks and the CPU test."""
    import oracle as O
    O.build()
    ri = (side - 1) // 2
    elev, n_rays = DISCS[side]
    kw = dict(max_camera_depth=40 * RES, delta_theta=(2 * np.pi / n_rays) if n_rays else 0.10, camera_fov=1.04,
              robot_radius=(ri - 0.5) * RES, n_rays=n_rays, elev=elev)          # ceil(robot_radius / resolution) = ri
    rng = np.random.default_rng(1000 * nz + side)
    base = np.where(rng.random((nz, 32, 32)) < 0.8, 255, 0).astype(np.uint8)  # unknown / free: nothing lethal, no obstacle
    out = []
    for name, (start, lethal_cells, verdict) in _placements(nz, ri).items():
        cells = base.copy()
        for (x, y, z) in lethal_cells:
            cells[z, y, x] = 254
        g = [(start[0] + 0.5) * RES, (start[1] + 0.5) * RES, (start[2] + 0.5) * RES]
        goals = np.array([g] * 7 + [[-1.0, g[1], g[2]]], dtype=np.float64)       # ..., blacklisted, off the map
        black = np.array([0, 0, 0, 0, 0, 0, 1, 0], dtype=np.uint8)
        ach_in = np.array([1, 1, 1, 0, 0, 0, 1, 1], dtype=np.uint8)
        sized = np.array([9, 10, 11, 9, 10, 11, 9, 9], dtype=np.int32)
        G = O.Grid(cells, origin=(0.0, 0.0, 0.0), resolution=RES)
        P = O.RayParams(**kw)
        assert int(np.ceil(kw["robot_radius"] / RES)) == ri and 2 * ri + 1 == side
        assert O.footprint_in_lethal(G, start[0], start[1], start[2], float(ri)) == verdict, (nz, side, name)
        calls = []
        for fsize in (sized, None):
            want = O.arrival_information(G, P, goals, fsize, black, ach_in, min_gt=0.0, faithful=True)
            calls.append((fsize, want))
        out.append(dict(name=name, cells=cells, goals=goals, black=black, ach_in=ach_in, verdict=verdict, calls=calls))
    return kw, out


def test_inputs_exercise_the_rule():
    seen = {s: set() for s in SIZES}
    for nz in (1, 8):
        for side in DISCS:
            _, placements = _case(nz, side)
            assert {p["name"] for p in placements} >= {"inside", "on_radius", "just_outside", "corner_wrap_bait", "corner_inside"}
            assert (nz == 1) != any(p["name"] == "other_slice" for p in placements)
            for p in placements:
                for fsize, want in p["calls"]:
                    assert list(want["status"]) == [0] * 6 + [2, 1], (nz, side, p["name"])
                    sizes = [None] * 6 if fsize is None else list(fsize[:6])
                    for k, s in enumerate(sizes):
                        seen[s].add(int(want["achievable"][k]))
                        # the rule itself: the disc's verdict is read below 10 only, achievable_in passes through
                        scans = s is None or s < 10
                        assert want["achievable"][k] == (p["ach_in"][k] and not (scans and p["verdict"])), (nz, side, p["name"], k)
    assert all(v == {0, 1} for v in seen.values()), seen


@pytest.fixture(scope="module")
def disc_scorer(fs):
    s = fs.FrontierScorer(device=0)
    s.lookup_generate()
    s.upload_landmarks(np.random.default_rng(5).uniform(0.0, 1.6, (64, 3)).astype(np.float32))
    s.set_fim_params(14.0, 1.0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [1, 2], ids=["byte_walk", "class_walk"])
@pytest.mark.parametrize("side", sorted(DISCS))
@pytest.mark.parametrize("nz", [1, 8])
def test_footprint_disc_matches_oracle(disc_scorer, nz, side, walk):
    sc = disc_scorer
    kw, placements = _case(nz, side)
    sc.set_option("ray.layout", walk)
    sc.set_ray_params(**kw)
    assert sc.n_yaw * sc.n_elev == (63 if side == 33 else 256)
    for p in placements:
        sc.upload_grid(p["cells"], (0.0, 0.0, 0.0), RES)
        for fsize, want in p["calls"]:
            where = f"{p['name']}, frontier_size {'absent' if fsize is None else 'given'}"
            got = sc.score_arrival(p["goals"], fsize, p["black"], p["ach_in"])
            for k in ("status", "arrival", "argmax", "achievable", "ray_counts"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"fs_score_arrival {k}: {where}")
            got = sc.score_arrival(p["goals"], fsize, p["black"], p["ach_in"], want_ray_counts=False)
            for k in ("status", "arrival", "argmax", "achievable"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"fs_score_arrival without ray counts {k}: {where}")
            rec = sc.score_candidates(p["goals"], fsize, p["black"], p["ach_in"])
            np.testing.assert_array_equal((rec["flags"] >> 8) & 0xFF, want["status"], err_msg=f"fs_score_candidates status: {where}")
            np.testing.assert_array_equal(rec["flags"] & 1, want["achievable"], err_msg=f"fs_score_candidates achievable: {where}")
            np.testing.assert_array_equal(rec["arrival"], want["arrival"], err_msg=f"fs_score_candidates arrival: {where}")
            np.testing.assert_array_equal(rec["argmax"], want["argmax"], err_msg=f"fs_score_candidates argmax: {where}")
