"""fs_upload_world_landmarks, fs_sense_landmarks and fs_world_landmarks_get at the boundary: declared in
include/fitslam_frontier.h, exported by the library, listed in EXPORTED_SYMBOLS, bound with as many arguments as the header
declares, the sensor struct's size, the ABI version unchanged, a NULL context refused.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", "fitslam_frontier.h"), os.path.join(ROOT, "include", "fitslam_frontier_dev.h")]

DECLARED = {
    "fs_upload_world_landmarks": ["fs_ctx *ctx", "const float *xyz", "int32_t m_world", "const uint8_t *known"],
    "fs_sense_landmarks": ["fs_ctx *ctx", "int32_t n", "const double *pose7", "const fs_landmark_sensor *sensor", "int32_t *n_in_view",
                           "int32_t *n_new", "int32_t *n_discovered"],
    "fs_world_landmarks_get": ["fs_ctx *ctx", "int32_t *m_world", "int32_t *n_discovered", "int32_t *world_index", "int32_t *views"],
}
SENSOR_FIELDS = ["double max_dist", "max_angle", "int32_t line_of_sight", "int32_t min_views", "int32_t occ_min", "occ_max",
                 "double end_margin_m"]


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_calls_and_the_sensor():
    text = _text(HEADERS[0])
    for name, want in DECLARED.items():
        assert _args(text, name) == want, name
    m = re.search(r"typedef\s+struct\s+fs_landmark_sensor\s*\{(.*?)\}\s*fs_landmark_sensor\s*;", text, flags=re.S)
    assert m, "fs_landmark_sensor is not declared"
    fields = [re.sub(r"\s+", " ", f).strip() for f in re.split(r"[;,]", m.group(1)) if f.strip()]
    assert fields == SENSOR_FIELDS
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", text)


def test_exported_symbols_equal_the_declared_set(fs):
    declared = set()
    for h in HEADERS:
        declared |= set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", _text(h)))
    assert set(DECLARED) <= declared
    assert declared == set(fs.capi.EXPORTED_SYMBOLS)
    assert len(fs.capi.EXPORTED_SYMBOLS) == len(set(fs.capi.EXPORTED_SYMBOLS))


def test_library_exports_and_binds_the_calls(fs):
    L = fs.load_library()
    text = _text(HEADERS[0])
    for name in DECLARED:
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == len(_args(text, name)), name
        assert f.restype is ctypes.c_int
    assert L.fs_abi_version() == 1
    for method in ("upload_world_landmarks", "sense_landmarks", "world_landmarks", "staged_cloud"):
        assert callable(getattr(fs.FrontierScorer, method)), method


def test_sensor_struct_size(fs):
    # two doubles, four int32, one double: no padding on any ABI this library is built for
    assert ctypes.sizeof(fs.capi.LandmarkSensorC) == 40
    assert [f[0] for f in fs.capi.LandmarkSensorC._fields_] == ["max_dist", "max_angle", "line_of_sight", "min_views", "occ_min", "occ_max",
                                                               "end_margin_m"]
    assert fs.capi.LandmarkSensorC.end_margin_m.offset == 32


def test_library_holds_the_new_kernels(fs):
    blob = open(fs._build.LIB, "rb").read()
    for kernel in (b"fs_sense_landmarks_kernel", b"fs_landmark_flags_kernel", b"fs_landmark_scan_kernel", b"fs_landmark_scatter_kernel"):
        assert kernel in blob, kernel
    assert "fs_sense_landmarks.hip" in fs._build.SOURCES


def test_null_context_is_refused_and_nothing_is_written(fs):
    L = fs.load_library()
    E = fs.capi
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    xyz = np.zeros((4, 3), dtype=np.float32)
    known = np.ones(4, dtype=np.uint8)
    assert L.fs_upload_world_landmarks(None, p(xyz), 4, p(known)) == E.FS_E_INVALID
    assert L.fs_upload_world_landmarks(None, None, 0, None) == E.FS_E_INVALID
    poses = np.zeros((2, 7)); poses[:, 6] = 1.0
    niv = np.full(2, 77, dtype=np.int32)
    n_new, n_disc = ctypes.c_int32(77), ctypes.c_int32(77)
    for los in (0, 1):
        sensor = E.LandmarkSensorC(14.0, 1.0, los, 1, 254, 254, 0.3)
        assert L.fs_sense_landmarks(None, 2, p(poses), ctypes.byref(sensor), p(niv), ctypes.byref(n_new), ctypes.byref(n_disc)) == E.FS_E_INVALID
    assert L.fs_sense_landmarks(None, 2, p(poses), None, p(niv), ctypes.byref(n_new), ctypes.byref(n_disc)) == E.FS_E_INVALID
    assert (niv == 77).all() and n_new.value == 77 and n_disc.value == 77
    m, nd = ctypes.c_int32(77), ctypes.c_int32(77)
    idx = np.full(4, 77, dtype=np.int32); views = np.full(4, 77, dtype=np.int32)
    assert L.fs_world_landmarks_get(None, ctypes.byref(m), ctypes.byref(nd), p(idx), p(views)) == E.FS_E_INVALID
    assert m.value == 77 and nd.value == 77 and (idx == 77).all() and (views == 77).all()
