"""fs_landmarks_in_view on the GPU: the list of every pose against the oracle's own transform and predicate
(oracle/fso_fisher.c: fso_world_to_camera, fso_is_visible) looped over the uploaded array — indices exactly, p_camera and table_value
bit for bit —, against what fs_score_fim counts and sums, under fs_set_occlusion, with a capacity smaller than the list, in several
rounds, and across the context's life (first call, a second cloud, both ordering routes, the error returns)."""
import ctypes
import importlib

import numpy as np
import pytest

import occlusion_ref as OR

pytestmark = pytest.mark.gpu

fsmod = importlib.import_module("fit-slam_amd")
E = fsmod.capi
REL = importlib.import_module("fit-slam_amd.parity").REL          # 1e-4, as _check_fim uses it
# (max_dist, max_angle): the cone; the reference's own request (cone off); a cone wider than a half space (c < 0)
SETTINGS = [(14.0, 1.0), (14.0, 4.0), (6.0, 2.2)]
ON_LANDMARK = 11                     # pose 6 sits exactly on this landmark (n2 == 0)
# The reference table (gen_fi_lookup's bounds) spans x 0 .. 21 m and y, z -15 .. 14.7 m.  Inside the cone of (14, 1.0) a landmark has
# px >= 0 and |py|, |pz| <= 14 sin(1) = 11.8 m: none can miss that table, so under that setting a NaN table_value can only be
# provoked with a smaller table.  Every setting is therefore also run against a table of these bounds, where each of them lists misses.
SMALL_BOUNDS = (0.0, 9.0, -4.0, 4.0, -4.0, 4.0)


@pytest.fixture(scope="module")
def sc():
    """a context of this module's own: cloud, settings and options must not leak into the session's shared scorer"""
    s = fsmod.FrontierScorer(device=0)
    s.lookup_generate()
    yield s
    s.close()


def make_cloud(m, seed):
    """m landmarks in a 24 m x 24 m x 5 m slab; 5 of them unusable (NaN, +-inf, 1e30), 20 exact duplicates of others"""
    rng = np.random.default_rng(seed)
    lm = np.concatenate([rng.uniform(-12.0, 12.0, size=(m, 2)), rng.uniform(-2.0, 3.0, size=(m, 1))], axis=1).astype(np.float32)
    src = rng.choice(np.arange(40, m // 2), size=20, replace=False)
    dst = rng.choice(np.arange(m // 2, m - 8), size=20, replace=False)
    lm[dst] = lm[src]
    bad = [7, 100, m // 2 + 1, m - 3, m - 1]
    lm[bad[0], 0] = np.nan
    lm[bad[1], 1] = np.inf
    lm[bad[2], 2] = -np.inf
    lm[bad[3]] = (1.0e30, 0.0, 0.0)
    lm[bad[4]] = (np.nan, np.inf, 1.0e30)
    return lm


def make_poses(lm, extra=0):
    """8 poses (+ extra general ones): four general quaternions with roll and pitch, two yaw-only, one exactly on a landmark, one 1 km away"""
    rng = np.random.default_rng(5)
    ps = np.zeros((8 + extra, 7))
    ps[:, :2] = rng.uniform(-9.0, 9.0, size=(8 + extra, 2))
    ps[:, 2] = rng.uniform(-0.5, 1.5, size=8 + extra)
    q = rng.normal(size=(8 + extra, 4))
    ps[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    for i, yaw in ((4, 0.7), (5, -2.6)):
        ps[i, 3:] = (0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2))
    ps[6, :3] = lm[ON_LANDMARK].astype(np.float64)
    ps[7, :3] = (1000.0, -3.0, 0.5)
    return ps


class Restatement:
    """The CPU side for one (cloud, poses): oracle.world_to_camera / oracle.is_visible / oracle.voxel_coordinate / Table.find — the
    C functions behind them, called through ctypes with raw addresses — looped over the uploaded array.  p is computed once per
    (cloud, pose), keys and table values once per landmark that some setting lists."""

    def __init__(self, oracle, table, lm, poses):
        self.L, self.O, self.table = oracle.lib(), oracle, table
        self.lm = np.ascontiguousarray(lm, dtype=np.float32)
        self.poses = np.ascontiguousarray(poses, dtype=np.float64)
        n, m = self.poses.shape[0], self.lm.shape[0]
        self.P = np.zeros((n, m, 3), dtype=np.float32)
        for i in range(n):
            R, t = oracle.pose_to_rt(self.poses[i])
            R = np.ascontiguousarray(R.reshape(9), dtype=np.float32)
            ra, ta, la, pa = R.ctypes.data, t.ctypes.data, self.lm.ctypes.data, self.P[i].ctypes.data
            f = self.L.fso_world_to_camera
            for k in range(m):
                f(ra, ta, la + 12 * k, pa + 12 * k)
        self.vox = np.zeros((n, m, 3), dtype=np.int32)
        self.val = np.full((n, m), np.nan, dtype=np.float32)
        self.have = np.zeros((n, m), dtype=bool)
        self._vis = {}

    def visible(self, i, max_dist, max_angle):
        key = (i, max_dist, max_angle)
        if key not in self._vis:
            v = self.O._VisParams(max_dist, max_angle)
            pa, f, ref = self.P[i].ctypes.data, self.L.fso_is_visible, ctypes.byref(v)
            self._vis[key] = np.array([f(pa + 12 * k, ref) != 0 for k in range(self.lm.shape[0])], dtype=bool)
        return self._vis[key]

    def values(self, i, idx):
        """(voxel lattice index [k][3], table value [k]) of pose i's landmarks idx"""
        key = np.zeros(3, dtype=np.float32)
        for k in idx[~self.have[i, idx]]:
            p = self.P[i, k]
            self.L.fso_voxel_coordinate(float(p[0]), float(p[1]), float(p[2]), key.ctypes.data, self.vox[i, k].ctypes.data)
            self.val[i, k] = self.L.fso_table_find(self.table._h, key.ctypes.data)
            self.have[i, k] = True
        return self.vox[i, idx], self.val[i, idx]


_REFS = {}


def restatement(oracle, table, m, extra=0, tag="reference"):
    """computed once per (cloud, poses, table) and shared by the tests; `table` must be the one `tag` names"""
    if (m, extra, tag) not in _REFS:
        lm = make_cloud(m, seed=m)
        _REFS[(m, extra, tag)] = Restatement(oracle, table, lm, make_poses(lm, extra))
    return _REFS[(m, extra, tag)]


def check_lists(ref, off, ent, keep, setting, what=""):
    """the list of every pose against the restatement: keep[i] = the expected visibility mask of pose i"""
    n = ref.poses.shape[0]
    counts = np.array([int(k.sum()) for k in keep], dtype=np.int64)
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(counts)]), err_msg=f"offsets {setting} {what}")
    assert ent.shape[0] == off[n]
    for i in range(n):
        seg = ent[off[i]:off[i + 1]]
        want = np.flatnonzero(keep[i])
        np.testing.assert_array_equal(seg["index"], want, err_msg=f"index, pose {i} {setting} {what}")
        np.testing.assert_array_equal(seg["p_camera"].view(np.uint32), ref.P[i, want].view(np.uint32), err_msg=f"p_camera, pose {i} {setting} {what}")
        _, val = ref.values(i, want)
        miss = np.isnan(val)
        np.testing.assert_array_equal(np.isnan(seg["table_value"]), miss, err_msg=f"table misses, pose {i} {setting} {what}")
        np.testing.assert_array_equal(seg["table_value"][~miss].view(np.uint32), val[~miss].view(np.uint32), err_msg=f"table_value, pose {i} {setting} {what}")


def not_vacuous(ref, off, ent, misses_possible=True):
    n = ref.poses.shape[0]
    assert np.diff(off).max() >= 50
    if misses_possible:
        assert np.isnan(ent["table_value"]).any()
    assert not np.isnan(ent["table_value"]).all()
    shared = False
    for i in range(n):
        seg = ent[off[i]:off[i + 1]]
        vox, _ = ref.values(i, seg["index"])
        shared = shared or (seg.shape[0] > 0 and np.unique(vox, axis=0).shape[0] < seg.shape[0])
    assert shared


# ------------------------------------------------------------------------------------------------ 1. against the restatement

def _lists_against(ref, s, m, every_setting_misses):
    s.set_occlusion(False)
    s.upload_landmarks(ref.lm)
    for setting in SETTINGS:
        s.set_fim_params(*setting)
        off, ent = s.landmarks_in_view(ref.poses)
        keep = [ref.visible(i, *setting) for i in range(8)]
        check_lists(ref, off, ent, keep, setting)
        not_vacuous(ref, off, ent, misses_possible=every_setting_misses or setting != (14.0, 1.0))
        assert off[8] == off[7]                                         # the pose 1 km away sees nothing
        assert ON_LANDMARK in ent["index"][off[6]:off[7]]               # n2 == 0 is visible
        bad = [7, 100, m // 2 + 1, m - 3, m - 1]
        assert not np.isin(ent["index"], bad).any()


@pytest.mark.parametrize("m", [3000, 4200])
def test_lists_equal_the_restatement(oracle, ref_table, sc, m):
    """3 000 landmarks: the cloud ordered on the host; 4 200: on the device (from 4 096 on).  The reference's table."""
    _lists_against(restatement(oracle, ref_table, m), sc, m, every_setting_misses=False)


@pytest.mark.parametrize("m", [3000, 4200])
def test_lists_equal_the_restatement_with_a_small_table(oracle, m):
    """... and a table that every setting's visibility volume sticks out of: misses (NaN) under each of them"""
    small = oracle.Table.generate(SMALL_BOUNDS)
    s = fsmod.FrontierScorer(device=0)
    try:
        s.lookup_generate(SMALL_BOUNDS)
        _lists_against(restatement(oracle, small, m, tag="small"), s, m, every_setting_misses=True)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ 2. against the scoring call

@pytest.mark.parametrize("m", [3000, 4200])
def test_lists_are_what_fs_score_fim_counts_and_sums(oracle, ref_table, sc, m):
    ref = restatement(oracle, ref_table, m)
    sc.set_occlusion(False)
    sc.upload_landmarks(ref.lm)
    factor = np.array([0.0] + [oracle.factor_from_num(k) for k in range(1, 400)], dtype=np.float32)
    for setting in SETTINGS:
        sc.set_fim_params(*setting)
        off, ent = sc.landmarks_in_view(ref.poses)
        got = sc.score_fim(ref.poses)
        np.testing.assert_array_equal(np.diff(off), got["n_visible"], err_msg=str(setting))
        for i in range(8):
            seg = ent[off[i]:off[i + 1]]
            vox, _ = ref.values(i, seg["index"])
            # the reference's loop (FisherInfoManager.cpp:85-97) over the list in list order
            count, total = {}, np.float32(0.0)
            for v, value in zip(map(tuple, vox), seg["table_value"]):
                if np.isnan(value):
                    continue
                k = count[v] = count.get(v, 0) + 1
                total = np.float32(total + np.float32(np.float64(value) * np.float64(factor[min(k, 399)])))
            assert len(count) == got["n_voxels"][i], (setting, i)
            assert abs(float(total) - float(got["info_ref"][i])) <= REL * max(abs(float(total)), 1e-6), (setting, i, total, got["info_ref"][i])


# ------------------------------------------------------------------------------------------------------------ 3. occlusion

def _occlusion_case(oracle, ref_table, sc, cells, origin, res, lm, poses, settings):
    G = oracle.Grid(cells, origin=origin, resolution=res)
    ref = Restatement(oracle, ref_table, lm, poses)
    n = poses.shape[0]
    sc.upload_grid(cells, origin, res)
    sc.upload_landmarks(lm)
    try:
        for setting in settings:
            sc.set_fim_params(*setting)
            pred = [ref.visible(i, *setting) for i in range(n)]
            keep = [pred[i] & OR.unblocked_mask(oracle, G, poses[i], lm) for i in range(n)]
            assert any(0 < keep[i].sum() < pred[i].sum() for i in range(n))      # the rule removes some and leaves some
            sc.set_occlusion(True)
            off, ent = sc.landmarks_in_view(poses)
            check_lists(ref, off, ent, keep, setting, "occluded")
            np.testing.assert_array_equal(np.diff(off), sc.score_fim(poses)["n_visible"])
            sc.set_occlusion(False)
            off, ent = sc.landmarks_in_view(poses)
            check_lists(ref, off, ent, pred, setting, "occlusion off again")
    finally:
        sc.set_occlusion(False)


def test_occlusion_on_the_fixture_map(oracle, ref_table, sc):
    _occlusion_case(oracle, ref_table, sc, OR.fixture_cells(), OR.FIX_ORIGIN, OR.FIX_RES, OR.fixture_landmarks(3000), OR.fixture_poses(oracle),
                    [(14.0, 1.0), (14.0, 4.0)])


def test_occlusion_on_a_3d_grid(oracle, ref_table, sc):
    rng = np.random.default_rng(15)
    cells = rng.choice(np.array([0, 100, 253, 254, 255], dtype=np.uint8), size=(8, 32, 32), p=[0.88, 0.03, 0.03, 0.03, 0.03])
    origin, res = (-3.2, 1.0, 0.0), 0.25
    lm = (rng.uniform(0.05, 0.95, size=(600, 3)) * (8.0, 8.0, 2.0) + origin).astype(np.float32)
    poses = np.zeros((3, 7))
    poses[:, :3] = rng.uniform(0.2, 0.8, size=(3, 3)) * (8.0, 8.0, 2.0) + origin
    q = rng.normal(size=(3, 4))
    poses[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    _occlusion_case(oracle, ref_table, sc, cells, origin, res, lm, poses, [(14.0, 4.0)])


def test_occlusion_without_a_grid_is_a_state_error(oracle, ref_table):
    lm = make_cloud(3000, seed=3000)
    fresh = fsmod.FrontierScorer(device=0)
    try:
        fresh.lookup_generate()
        fresh.upload_landmarks(lm)
        fresh.set_fim_params(14.0, 1.0)
        fresh.set_occlusion(True)
        with pytest.raises(fsmod.FsError) as e:
            fresh.landmarks_in_view(make_poses(lm))
        assert e.value.code == E.FS_E_STATE
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------------------- 4. capacity

def _raw(sc, poses, max_total, out):
    L = fsmod.load_library()
    ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    off = np.full(ps.shape[0] + 1, -5, dtype=np.int64)
    rc = L.fs_landmarks_in_view(sc._h, ps.shape[0], E._p(ps), int(max_total), E._p(off), None if out is None else E._p(out))
    return rc, off


def test_capacity_smaller_than_the_list(oracle, ref_table, sc):
    ref = restatement(oracle, ref_table, 3000)
    sc.set_occlusion(False)
    sc.upload_landmarks(ref.lm)
    sc.set_fim_params(14.0, 4.0)
    off, ent = sc.landmarks_in_view(ref.poses)
    total = int(off[8])
    assert total >= 100
    half = total // 2
    assert any(off[i] < half < off[i + 1] for i in range(8))               # the capacity ends inside a pose's segment
    buf = np.full((half + 64) * 20, 0xA5, dtype=np.uint8)
    rc, off2 = _raw(sc, ref.poses, half, buf)
    assert rc == E.FS_OK
    np.testing.assert_array_equal(off2, off)
    assert buf[:half * 20].tobytes() == ent[:half].tobytes()
    assert (buf[half * 20:] == 0xA5).all()                                   # nothing at or beyond max_total is written
    rc, off3 = _raw(sc, ref.poses, 0, None)                                  # the count-only form
    assert rc == E.FS_OK
    np.testing.assert_array_equal(off3, off)
    off4, ent4 = sc.landmarks_in_view(ref.poses, max_total=half)             # the binding passes an integer straight through
    np.testing.assert_array_equal(off4, off)
    assert ent4.tobytes() == ent[:half].tobytes()
    off5, ent5 = sc.landmarks_in_view(ref.poses, max_total=total + 10)       # more room than entries
    assert ent5.tobytes() == ent.tobytes()


# --------------------------------------------------------------------------------------------------------------- 5. rounds

def test_rounds_of_three_poses_give_the_same_output(oracle, ref_table, sc):
    ref = restatement(oracle, ref_table, 3000, extra=2)
    assert ref.poses.shape[0] == 10
    sc.set_occlusion(False)
    sc.upload_landmarks(ref.lm)
    sc.set_fim_params(14.0, 1.0)
    off, ent = sc.landmarks_in_view(ref.poses)
    check_lists(ref, off, ent, [ref.visible(i, 14.0, 1.0) for i in range(10)], (14.0, 1.0))
    sc.set_option("view.round_poses", 3)
    try:
        off3, ent3 = sc.landmarks_in_view(ref.poses)
        half = int(off[10]) // 2
        off3h, ent3h = sc.landmarks_in_view(ref.poses, max_total=half)
    finally:
        sc.set_option("view.round_poses", 0)
    np.testing.assert_array_equal(off3, off)
    assert ent3.tobytes() == ent.tobytes()
    np.testing.assert_array_equal(off3h, off)
    assert ent3h.tobytes() == ent[:half].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 6. state

def test_first_call_of_a_fresh_context_and_a_second_shorter_cloud(oracle, ref_table):
    ref = restatement(oracle, ref_table, 4200)
    fresh = fsmod.FrontierScorer(device=0)
    try:
        fresh.lookup_generate()
        fresh.upload_landmarks(ref.lm)
        fresh.set_fim_params(14.0, 1.0)
        off, ent = fresh.landmarks_in_view(ref.poses)                       # the context's first call of any kind
        check_lists(ref, off, ent, [ref.visible(i, 14.0, 1.0) for i in range(8)], (14.0, 1.0), "first call")
        small = restatement(oracle, ref_table, 3000)
        fresh.upload_landmarks(small.lm)                                     # another, shorter cloud, by the other ordering route
        off, ent = fresh.landmarks_in_view(small.poses)
        assert ent.shape[0] > 0 and ent["index"].max() < 3000
        check_lists(small, off, ent, [small.visible(i, 14.0, 1.0) for i in range(8)], (14.0, 1.0), "second cloud")
    finally:
        fresh.close()


def test_both_ordering_routes_give_the_same_bytes(oracle, ref_table, sc):
    ref = restatement(oracle, ref_table, 4200)
    sc.set_occlusion(False)
    sc.set_fim_params(14.0, 4.0)
    got = {}
    try:
        for order in (0, 2):
            sc.set_option("cloud.order", order)
            sc.upload_landmarks(ref.lm)
            got[order] = sc.landmarks_in_view(ref.poses)
    finally:
        sc.set_option("cloud.order", 1)
    np.testing.assert_array_equal(got[0][0], got[2][0])
    assert got[0][1].shape[0] >= 100 and got[0][1].tobytes() == got[2][1].tobytes()


def test_error_returns(oracle, ref_table, sc):
    L = fsmod.load_library()
    ref = restatement(oracle, ref_table, 3000)
    fresh = fsmod.FrontierScorer(device=0)
    try:
        off = np.full(9, -5, dtype=np.int64)
        out = np.full(16 * 20, 0xA5, dtype=np.uint8)
        ps = ref.poses
        call = lambda h, n, p, cap, o, e: L.fs_landmarks_in_view(h, n, None if p is None else E._p(p), cap, None if o is None else E._p(o), None if e is None else E._p(e))
        assert call(None, 8, ps, 16, off, out) == E.FS_E_INVALID
        assert call(fresh._h, 8, ps, 16, off, out) == E.FS_E_STATE           # no table, no cloud
        fresh.lookup_generate()
        assert call(fresh._h, 8, ps, 16, off, out) == E.FS_E_STATE           # no cloud
        fresh.upload_landmarks(ref.lm)
        fresh.set_fim_params(14.0, 1.0)
        assert call(fresh._h, -1, ps, 16, off, out) == E.FS_E_INVALID
        assert call(fresh._h, 8, ps, 16, None, out) == E.FS_E_INVALID
        assert call(fresh._h, 8, None, 16, off, out) == E.FS_E_INVALID
        assert call(fresh._h, 8, ps, -1, off, out) == E.FS_E_INVALID
        assert call(fresh._h, 8, ps, 16, off, None) == E.FS_E_INVALID
        assert (off == -5).all() and (out == 0xA5).all()                     # every FS_E_INVALID case writes nothing
        assert call(fresh._h, 0, None, 0, off, None) == E.FS_OK
        assert off[0] == 0 and (off[1:] == -5).all()
        assert call(fresh._h, 8, ps, 16, off, out) == E.FS_OK                # offsets[n] > max_total is not an error
        assert off[0] == 0 and off[8] > 16
        noTable = fsmod.FrontierScorer(device=0)
        try:
            noTable.upload_landmarks(ref.lm)
            assert call(noTable._h, 8, ps, 16, off, out) == E.FS_E_STATE     # a cloud and no table
        finally:
            noTable.close()
    finally:
        fresh.close()
