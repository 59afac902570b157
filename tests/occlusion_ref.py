"""The line-of-sight rule of fs_set_occlusion (include/fitslam_frontier.h), restated in numpy from the oracle's
own cell walk — `oracle.trace_ray(...)["visited"]`, the linear offsets getTracedCells hands to its visitor — and the fixture
the occlusion tests share.  A helper, not a test module: tests/test_occlusion_ref.py checks it without a GPU,
tests/test_gpu_occlusion.py checks the library against it.

The rule: the UNCAPPED walk from s to w (scale 1: visits v = 0 .. end) is blocked when a visit with v + M <= end,
M = 1 + (unsigned)(end_margin_m / resolution), holds a cost in [occ_min, occ_max]; the start cell is tested; an end off the
map: nothing is tested, not blocked.  On a 2-D grid both z coordinates are origin_z.  tested_cells = the visits the rule
covers = max(0, end + 1 - M), whether or not an earlier one already blocked.
"""
import numpy as np

DEFAULT_OCC = (254, 254)
DEFAULT_MARGIN = 0.3


def margin_cells(resolution, end_margin_m=DEFAULT_MARGIN):
    return 1 + int(float(end_margin_m) / float(resolution))


def line_of_sight(oracle, G, s, w, occ=DEFAULT_OCC, end_margin_m=DEFAULT_MARGIN):
    """(ok, blocked, tested_cells) of one pair under the rule, on the oracle grid G."""
    nz, ny, nx = G.shape
    s = [float(v) for v in s]
    w = [float(v) for v in w]
    if nz == 1:
        s[2] = w[2] = float(G.origin[2])
    # any cap >= the walk's Euclidean length in cells gives scale = 1: hypot(d) <= sqrt(3) * max(n) < 2 * max(n)
    cap = 2 * max(nx, ny, nz)
    r = oracle.trace_ray(G, s, w, cap, obst=(256, 256), trace=(256, 256), faithful=False)
    if not r["ok"]:
        return False, False, 0
    visited = r["visited"]
    end = len(visited) - 1
    n = max(0, end + 1 - margin_cells(G.resolution, end_margin_m))
    costs = G.cells.reshape(-1)[visited[:n]]
    blocked = bool(np.any((costs >= occ[0]) & (costs <= occ[1])))
    return True, blocked, n


def lines_of_sight(oracle, G, from_xyz, to_xyz, occ=DEFAULT_OCC, end_margin_m=DEFAULT_MARGIN):
    a = np.asarray(from_xyz, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(to_xyz, dtype=np.float64).reshape(-1, 3)
    ok = np.zeros(a.shape[0], np.uint8)
    blocked = np.zeros(a.shape[0], np.uint8)
    tested = np.zeros(a.shape[0], np.int32)
    for i in range(a.shape[0]):
        ok[i], blocked[i], tested[i] = line_of_sight(oracle, G, a[i], b[i], occ, end_margin_m)
    return dict(ok=ok, blocked=blocked, tested_cells=tested)


_MASKS = {}


def unblocked_mask(oracle, G, pose7, landmarks, occ=DEFAULT_OCC, end_margin_m=DEFAULT_MARGIN):
    """[m] bool: landmarks whose line from the pose's float32 translation (the t of getTransformFromPose) to the landmark's
    float32 position is NOT blocked, both widened to double."""
    _, t = oracle.pose_to_rt(pose7)
    lm = np.ascontiguousarray(landmarks, dtype=np.float32).reshape(-1, 3)
    s = t.astype(np.float64)
    # (computed once per (map, position, cloud, settings): the tests ask for the same masks under several visibility volumes)
    key = (G.cells.tobytes(), tuple(G.origin), float(G.resolution), s.tobytes(), lm.tobytes(), tuple(occ), float(end_margin_m))
    if key not in _MASKS:
        keep = np.ones(lm.shape[0], dtype=bool)
        for k in range(lm.shape[0]):
            keep[k] = not line_of_sight(oracle, G, s, lm[k].astype(np.float64), occ, end_margin_m)[1]
        _MASKS[key] = keep
    return _MASKS[key].copy()


def occluded_pose_information(oracle, table, G, landmarks, pose7, max_dist, max_angle, occ=DEFAULT_OCC, end_margin_m=DEFAULT_MARGIN):
    """oracle.pose_information per pose over the landmarks the rule leaves: the columns stacked, plus `keep` [n][m]."""
    ps = np.asarray(pose7, dtype=np.float64).reshape(-1, 7)
    lm = np.ascontiguousarray(landmarks, dtype=np.float32).reshape(-1, 3)
    rows, keeps = [], []
    for p in ps:
        keep = unblocked_mask(oracle, G, p, lm, occ, end_margin_m)
        rows.append(oracle.pose_information(table, lm[keep], p[None], max_dist, max_angle))
        keeps.append(keep)
    out = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    out["keep"] = np.stack(keeps)
    return out


# ---- the fixture of the scoring tests: a 16 m x 16 m map with one wall and two doors
FIX_RES = 0.25
FIX_ORIGIN = (-8.0, -8.0, 0.0)
FIX_YAWS = (0.3, -0.7, 2.9, -2.4, 0.0, 1.5)
FIX_XY = ((-5.0, -5.0), (-4.1, 4.3), (3.7, -2.2), (5.5, 5.5), (-1.0, 0.2), (1.5, -6.0))


def fixture_cells():
    c = np.zeros((64, 64), dtype=np.uint8)           # [row = y][col = x]
    c[:, 31:33] = 254                                # the wall
    c[10:16, 31:33] = 0                              # two doors
    c[44:50, 31:33] = 0
    c[20:24, 8:20] = 254                             # two blocks
    c[40:44, 44:56] = 254
    c[0:6, 0:6] = 255                                # an unknown patch
    return c


def fixture_landmarks(m, seed=20):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-7.9, 7.9, size=(m, 2))
    z = rng.uniform(-1.0, 2.5, size=(m, 1))
    return np.concatenate([xy, z], axis=1).astype(np.float32)


def fixture_poses(oracle):
    goal = np.array([[x, y, 0.3] for x, y in FIX_XY], dtype=np.float64)
    return oracle.poses_from_yaw(goal, np.array(FIX_YAWS))
