"""fs_drive_slam at the boundary: declared in include/fitslam_frontier.h with fs_drive_slam_params and
FS_DRIVE_UNSAFE 5, exported by the library, listed in EXPORTED_SYMBOLS, bound with as many arguments as the header declares, the
parameter struct of the size the binding assumes, the kernels in the library, the ABI version unchanged, a NULL context refused,
and the host helper poses_along.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fitslam_frontier.h")

DECLARED = {
    "fs_drive_slam": ["fs_ctx *ctx", "int32_t n_robots", "const double *station_pose7", "const int32_t *n_stations", "const int32_t *first_ray",
                      "const double *goal_xyz", "const fs_ray_params *sensor", "const fs_landmark_sensor *lm_sensor",
                      "const fs_drive_slam_params *params", "int32_t *status", "int32_t *reached", "int32_t *station_status",
                      "int32_t *seen_unknown", "float *station_information", "int32_t *station_voxels", "int32_t *station_in_view",
                      "int64_t *n_seen", "int64_t *n_revealed", "int32_t window[6]", "int32_t *n_new", "int32_t *n_discovered"],
}


def _text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_call_its_params_and_the_new_status(fs):
    text = _text()
    for name, want in DECLARED.items():
        assert _args(text, name) == want, name
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+FS_DRIVE_UNSAFE\s+5\b", text) and fs.capi.FS_DRIVE_UNSAFE == 5
    assert re.search(r"#define\s+FS_DRIVE_MAPPED\s+4\b", text)           # (the codes before it stay)
    m = re.search(r"typedef\s+struct\s+fs_drive_slam_params\s*\{(.*?)\}\s*fs_drive_slam_params\s*;", text, flags=re.S)
    assert m
    fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t block_min, block_max", "int32_t stop_when_mapped", "int32_t gate", "double information_threshold",
                      "int32_t gate_first_station"]
    assert [n for n, _ in fs.capi.DriveSlamParamsC._fields_] == ["block_min", "block_max", "stop_when_mapped", "gate", "information_threshold",
                                                                 "gate_first_station"]
    assert ctypes.sizeof(fs.capi.DriveSlamParamsC) == 32 and fs.capi.DriveSlamParamsC.information_threshold.offset == 16


def test_library_exports_and_binds_the_call(fs):
    assert "fs_drive_slam" in fs.capi.EXPORTED_SYMBOLS
    L = fs.load_library()
    f = L.fs_drive_slam
    assert f.argtypes is not None and len(f.argtypes) == len(_args(_text(), "fs_drive_slam")) == 21
    assert f.restype is ctypes.c_int
    assert L.fs_abi_version() == 1
    assert callable(fs.FrontierScorer.drive_slam) and callable(fs.capi.poses_along)


def test_library_holds_the_new_kernels(fs):
    blob = open(fs._build.LIB, "rb").read()
    for kernel in (b"fs_drive_slam_sweep_kernel", b"fs_drive_slam_info_kernel", b"fs_drive_slam_gate_kernel", b"fs_drive_step_kernel",
                   b"fs_sense_landmarks_kernel"):
        assert kernel in blob, kernel
    assert "fs_drive_slam.hip" in fs._build.SOURCES and "fs_sense_landmarks_dev.h" in fs._build.HEADERS


def test_null_context_is_refused_and_nothing_is_written(fs):
    L = fs.load_library()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    poses = np.zeros((3, 7)); poses[:, 6] = 1.0
    n_st = np.array([2, 1], dtype=np.int32); goals = np.zeros((2, 3))
    ints = [np.full(n, 77, np.int32) for n in (2, 2, 3, 3, 3, 3, 6)]
    info = np.full(3, 77.0, np.float32)
    n_seen, n_rev = ctypes.c_int64(77), ctypes.c_int64(77)
    n_new, n_disc = ctypes.c_int32(77), ctypes.c_int32(77)
    rc = L.fs_drive_slam(None, 2, p(poses), p(n_st), None, p(goals), None, None, None, p(ints[0]), p(ints[1]), p(ints[2]), p(ints[3]), p(info),
                         p(ints[4]), p(ints[5]), ctypes.byref(n_seen), ctypes.byref(n_rev), p(ints[6]), ctypes.byref(n_new), ctypes.byref(n_disc))
    assert rc == fs.capi.FS_E_INVALID
    assert all((a == 77).all() for a in ints) and (info == 77.0).all()
    assert (n_seen.value, n_rev.value, n_new.value, n_disc.value) == (77, 77, 77, 77)


def test_poses_along_looks_where_stations_along_looks(fs):
    E = fs.capi
    xs = np.arange(0.0, 2.0001, 0.05)
    east = np.stack([xs, np.zeros_like(xs)], 1)
    st, first, idx = E.stations_along(east, 0.24)
    ps = E.poses_along(east, idx)
    assert ps.shape == (st.shape[0], 7)
    np.testing.assert_array_equal(ps[:, :3], st)
    np.testing.assert_allclose(ps[:, 3:], np.tile([0.0, 0.0, 0.0, 1.0], (st.shape[0], 1)), atol=1e-15)      # east: the identity
    n_yaw = E.fan_n_yaw(0.10)
    for path in (east[::-1], np.stack([np.zeros(9), np.arange(9) * 0.1], 1), np.stack([xs, 0.5 * xs], 1)):
        st, first, idx = E.stations_along(path, 0.2, look=3, z=0.25)
        ps = E.poses_along(path, idx, look=3, z=0.25)
        np.testing.assert_array_equal(ps[:, :3], st)
        yaw = 2.0 * np.arctan2(ps[:, 5], ps[:, 6])
        want = [E.first_ray_for_yaw(y if y >= 0.0 else y + 2 * np.pi, 0.10, 1.04, n_yaw) for y in yaw]
        assert list(first) == want                                       # the same direction, station by station (the last keeps its predecessor's)
        np.testing.assert_allclose(np.hypot(ps[:, 5], ps[:, 6]), 1.0, atol=1e-15)
        assert (ps[:, 3:5] == 0.0).all()
    assert E.poses_along(np.zeros((0, 2)), []).shape == (0, 7)
    lone = E.poses_along(east[:1], [0])
    np.testing.assert_array_equal(lone, [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
