"""The landmark sensor of fs_sense_landmarks (include/fitslam_frontier.h), restated in numpy.  A helper, not a test
module: tests/test_landmark_sense_restatement.py checks it without a GPU, tests/test_gpu_landmark_sense.py and
tests/test_gpu_explore_episode_landmarks.py check the library against it.

Pose p SEES world landmark i when the visibility predicate accepts it — here in float64 from `oracle.pose_to_rt`'s float32 R and
t — and, with line_of_sight, `occlusion_ref.unblocked_mask` on the WORLD grid keeps it.  Every sighting adds 1 to the landmark's
counter; a counter that reaches min_views sets the landmark's `discovered` flag for good; the discovered list is the flags'
ascending indices.

The device evaluates the predicate in fp32 with a fixed FMA order, so a landmark within relative 1e-5 of the range or the cone
boundary may fall either way there.  `borderline` reports those (pose, landmark) pairs; the tests drop such landmarks from the world
cloud before they upload it (`drop_borderline`, which fails when more than 1 % of the cloud would go).  The fp32 chain's error is
a few 1e-7 relative on |p| and absolute on cos, two orders of magnitude inside that band.
"""
import numpy as np

import occlusion_ref as OR

BAND = 1.0e-5
MAX_DROP = 0.01


def usable(world):
    """fs_upload_landmarks' usability test: finite and within 1e17 m (a NaN compares false)."""
    w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(w) <= np.float32(1.0e17)).all(axis=1)


def _camera(oracle, pose7, world):
    R, t = oracle.pose_to_rt(pose7)
    w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ok = usable(world)
    d = np.where(ok[:, None], w, 0.0) - t.astype(np.float64)[None, :]
    p = d @ R.astype(np.float64)                         # p = R^T (w - t): p_j = sum_i R[i][j] d_i
    return p, ok


def predicate(oracle, pose7, world, max_dist, max_angle):
    """(visible [m] bool, borderline [m] bool) of one pose in float64."""
    p, ok = _camera(oracle, pose7, world)
    n = np.sqrt((p * p).sum(axis=1))
    vis = n <= max_dist
    border = np.abs(n - max_dist) <= BAND * max_dist
    if max_angle < np.pi:
        c = float(np.float32(np.cos(max_angle)))
        with np.errstate(invalid="ignore", divide="ignore"):
            cosang = np.where(n > 0.0, p[:, 0] / np.where(n > 0.0, n, 1.0), 1.0)
        vis &= cosang >= c
        border |= (np.abs(cosang - c) <= BAND) & (n <= max_dist * (1.0 + BAND))
    return vis & ok, border & ok


def sees(oracle, G_world, pose7, world, sensor):
    """[n][m] bool: which world landmarks each pose sees.  sensor: dict(max_dist, max_angle, line_of_sight, occ, end_margin_m);
    G_world: the oracle Grid of the WORLD (None allowed without line_of_sight)."""
    ps = np.asarray(pose7, dtype=np.float64).reshape(-1, 7)
    w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((ps.shape[0], w.shape[0]), dtype=bool)
    ok = usable(w)
    w_safe = np.where(ok[:, None], w, np.float32(0.0))   # (an unusable landmark is never seen: its line is walked to nowhere in particular)
    for k, p in enumerate(ps):
        vis, _ = predicate(oracle, p, w, sensor["max_dist"], sensor["max_angle"])
        if sensor.get("line_of_sight", 1) and vis.any():
            # (the whole cloud's mask: occlusion_ref caches it per pose, whatever the volume)
            vis &= OR.unblocked_mask(oracle, G_world, p, w_safe, sensor.get("occ", OR.DEFAULT_OCC), sensor.get("end_margin_m", OR.DEFAULT_MARGIN))
        out[k] = vis & ok
    return out


def borderline(oracle, pose7, world, volumes):
    """[m] bool: landmarks within the band of the range or cone boundary of any pose under any of `volumes` [(max_dist, max_angle)]."""
    ps = np.asarray(pose7, dtype=np.float64).reshape(-1, 7)
    w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(w.shape[0], dtype=bool)
    for p in ps:
        for md, ma in volumes:
            out |= predicate(oracle, p, w, md, ma)[1]
    return out


def drop_borderline(oracle, pose7, world, volumes):
    """The world cloud without its borderline landmarks; at most 1 % may go."""
    w = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3)
    b = borderline(oracle, pose7, w, volumes)
    assert b.sum() <= MAX_DROP * max(w.shape[0], 1), f"{int(b.sum())} of {w.shape[0]} landmarks are borderline"
    return np.ascontiguousarray(w[~b])


class WorldCloud:
    """Counters, flags and the discovered list of a world cloud, as the context keeps them."""

    def __init__(self, oracle, world, known=None):
        self.oracle = oracle
        self.world = np.ascontiguousarray(world, dtype=np.float32).reshape(-1, 3)
        m = self.world.shape[0]
        self.views = np.zeros(m, dtype=np.int64)
        self.flag = np.zeros(m, dtype=bool) if known is None else (np.asarray(known).reshape(-1) != 0)
        assert self.flag.shape[0] == m

    def sense(self, G_world, pose7, sensor, S=None):
        """one fs_sense_landmarks call: dict(n_in_view, n_new, n_discovered).  S: `sees` of these poses, where the caller has it."""
        if S is None:
            S = sees(self.oracle, G_world, pose7, self.world, sensor)
        self.views += S.sum(axis=0)
        fresh = ~self.flag & (self.views >= int(sensor.get("min_views", 1)))
        if S.shape[0] == 0:
            fresh[:] = False
        self.flag |= fresh
        return dict(n_in_view=S.sum(axis=1).astype(np.int32), n_new=int(fresh.sum()), n_discovered=int(self.flag.sum()))

    @property
    def world_index(self):
        return np.flatnonzero(self.flag).astype(np.int32)

    @property
    def discovered(self):
        """what the staged cloud holds: the discovered landmarks' xyz in ascending world index"""
        return np.ascontiguousarray(self.world[self.flag])
