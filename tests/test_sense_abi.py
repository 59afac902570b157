"""fs_upload_world, fs_sense, fs_goals_mapped and fs_grid_census at the boundary: declared in
include/fitslam_frontier.h, exported by the library, listed in EXPORTED_SYMBOLS, bound with as many arguments as the header
declares, the ABI version unchanged, a NULL context refused.  No GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", "fitslam_frontier.h"), os.path.join(ROOT, "include", "fitslam_frontier_dev.h")]

DECLARED = {
    "fs_upload_world": ["fs_ctx *ctx", "const uint8_t *cells", "int32_t nx", "int32_t ny", "int32_t nz"],
    "fs_sense": ["fs_ctx *ctx", "int32_t n", "const double *origin_xyz", "const int32_t *first_ray", "const fs_ray_params *sensor",
                 "int32_t *ray_unknown", "int32_t *seen_unknown", "int32_t *status", "int64_t *n_seen", "int64_t *n_revealed",
                 "int32_t window[6]"],
    "fs_goals_mapped": ["fs_ctx *ctx", "int32_t n", "const double *goal_xyz", "uint8_t *mapped"],
    "fs_grid_census": ["fs_ctx *ctx", "int64_t counts[4]"],
}


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_the_four_calls():
    text = _text(HEADERS[0])
    for name, want in DECLARED.items():
        assert _args(text, name) == want, name
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
    for method in ("upload_world", "sense", "goals_mapped", "grid_census", "first_ray_for_yaw"):
        assert callable(getattr(fs.FrontierScorer, method)), method


def test_library_holds_the_new_kernels(fs):
    blob = open(fs._build.LIB, "rb").read()
    for kernel in (b"fs_sense_kernel", b"fs_sense_merge_kernel", b"fs_goals_mapped_kernel", b"fs_grid_census_kernel"):
        assert kernel in blob, kernel
    assert "fs_sense.hip" in fs._build.SOURCES


def test_null_context_is_refused_and_nothing_is_written(fs):
    L = fs.load_library()
    E = fs.capi
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    cells = np.zeros((4, 4), dtype=np.uint8)
    assert L.fs_upload_world(None, p(cells), 4, 4, 1) == E.FS_E_INVALID
    origins = np.zeros((2, 3))
    seen = np.full(2, 77, dtype=np.int32); status = np.full(2, 77, dtype=np.int32); win = np.full(6, 77, dtype=np.int32)
    n_seen, n_rev = ctypes.c_int64(77), ctypes.c_int64(77)
    assert L.fs_sense(None, 2, p(origins), None, None, None, p(seen), p(status), ctypes.byref(n_seen), ctypes.byref(n_rev), p(win)) == E.FS_E_INVALID
    assert (seen == 77).all() and (status == 77).all() and (win == 77).all() and n_seen.value == 77 and n_rev.value == 77
    mapped = np.full(2, 0x5A, dtype=np.uint8)
    assert L.fs_goals_mapped(None, 2, p(origins), p(mapped)) == E.FS_E_INVALID
    assert (mapped == 0x5A).all()
    counts = np.full(4, 77, dtype=np.int64)
    assert L.fs_grid_census(None, p(counts)) == E.FS_E_INVALID
    assert (counts == 77).all()
