"""fs_drive at the boundary: declared in include/fitslam_frontier.h, exported by the library, listed in
EXPORTED_SYMBOLS, bound with as many arguments as the header declares, fs_drive_params of the size the binding assumes, the kernels
in the library, the ABI version unchanged, a NULL context refused.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", "fitslam_frontier.h"), os.path.join(ROOT, "include", "fitslam_frontier_dev.h")]

DECLARED = {
    "fs_drive": ["fs_ctx *ctx", "int32_t n_robots", "const double *station_xyz", "const int32_t *n_stations", "const int32_t *first_ray",
                 "const double *goal_xyz", "const fs_ray_params *sensor", "const fs_drive_params *params", "int32_t *status",
                 "int32_t *reached", "int32_t *station_status", "int32_t *seen_unknown", "int64_t *n_seen", "int64_t *n_revealed",
                 "int32_t window[6]"],
}
CODES = {"FS_DRIVE_ARRIVED": 0, "FS_DRIVE_BLOCKED": 1, "FS_DRIVE_COLLIDED": 2, "FS_DRIVE_OFF_MAP": 3, "FS_DRIVE_MAPPED": 4,
         "FS_DRIVE_MAX_STATIONS": 2048, "FS_DRIVE_MAX_ROBOTS": 4096}


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_call_and_its_codes(fs):
    text = _text(HEADERS[0])
    for name, want in DECLARED.items():
        assert _args(text, name) == want, name
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", text)
    for name, value in CODES.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(fs.capi, name) == value


def test_exported_symbols_equal_the_declared_set(fs):
    declared = set()
    for h in HEADERS:
        declared |= set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", _text(h)))
    assert set(DECLARED) <= declared
    assert declared == set(fs.capi.EXPORTED_SYMBOLS)
    assert len(fs.capi.EXPORTED_SYMBOLS) == len(set(fs.capi.EXPORTED_SYMBOLS))


def test_drive_params_is_three_int32(fs):
    m = re.search(r"typedef\s+struct\s+fs_drive_params\s*\{(.*?)\}\s*fs_drive_params\s*;", _text(HEADERS[0]), flags=re.S)
    assert m
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert [re.sub(r"\s+", " ", f) for f in fields] == ["int32_t block_min, block_max", "int32_t stop_when_mapped"]
    assert ctypes.sizeof(fs.capi.DriveParamsC) == 12
    assert [n for n, _ in fs.capi.DriveParamsC._fields_] == ["block_min", "block_max", "stop_when_mapped"]


def test_library_exports_and_binds_the_call(fs):
    L = fs.load_library()
    text = _text(HEADERS[0])
    for name in DECLARED:
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == len(_args(text, name)), name
        assert f.restype is ctypes.c_int
    assert L.fs_abi_version() == 1
    assert callable(fs.FrontierScorer.drive) and callable(fs.capi.stations_along)


def test_library_holds_the_new_kernels(fs):
    blob = open(fs._build.LIB, "rb").read()
    for kernel in (b"fs_drive_step_kernel", b"fs_drive_merge_kernel", b"fs_drive_goal_kernel", b"fs_sense_kernel", b"fs_sense_merge_kernel"):
        assert kernel in blob, kernel
    assert "fs_drive.hip" in fs._build.SOURCES and "fs_sense_dev.h" in fs._build.HEADERS


def test_null_context_is_refused_and_nothing_is_written(fs):
    L = fs.load_library()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    stations = np.zeros((3, 3)); n_st = np.array([2, 1], dtype=np.int32); goals = np.zeros((2, 3))
    status = np.full(2, 77, np.int32); reached = np.full(2, 77, np.int32)
    sst = np.full(3, 77, np.int32); seen = np.full(3, 77, np.int32); win = np.full(6, 77, np.int32)
    n_seen, n_rev = ctypes.c_int64(77), ctypes.c_int64(77)
    rc = L.fs_drive(None, 2, p(stations), p(n_st), None, p(goals), None, None, p(status), p(reached), p(sst), p(seen),
                    ctypes.byref(n_seen), ctypes.byref(n_rev), p(win))
    assert rc == fs.capi.FS_E_INVALID
    for a in (status, reached, sst, seen, win):
        assert (a == 77).all()
    assert n_seen.value == 77 and n_rev.value == 77


def test_stations_along_cuts_by_distance_and_looks_ahead(fs):
    E = fs.capi
    xs = np.arange(0.0, 2.0001, 0.05)                                    # 41 poses, 0.05 m apart, heading east
    poses = np.stack([xs, np.zeros_like(xs)], 1)
    st, first, idx = E.stations_along(poses, 0.24)
    assert idx[0] == 0 and idx[-1] == 40 and (np.diff(idx) == 5).all() and st.shape == (9, 3)
    np.testing.assert_array_equal(st[:, :2], poses[idx])
    assert (first == 0).all()                                            # east is window 0
    st, first, idx = E.stations_along(poses[::-1], 0.28)                 # heading west; six steps a station and a remainder of four
    assert list(idx) == [0, 6, 12, 18, 24, 30, 36, 40] and (first == 26).all()
    st, first, idx = E.stations_along(poses[:1], 0.25)                   # a lone pose: one station, window 0
    assert st.shape == (1, 3) and list(first) == [0] and list(idx) == [0]
    st, first, idx = E.stations_along(poses[:3], 10.0, z=0.5)            # shorter than the spacing: first and last pose
    assert list(idx) == [0, 2] and (st[:, 2] == 0.5).all()
    north = np.stack([np.zeros(5), np.arange(5) * 0.1], 1)
    n_yaw = E.fan_n_yaw(0.10)
    assert (E.stations_along(north, 0.1, look=2)[1] == E.first_ray_for_yaw(np.pi / 2, 0.10, 1.04, n_yaw)).all()
    assert E.stations_along(np.zeros((0, 2)), 0.25)[0].shape == (0, 3)
