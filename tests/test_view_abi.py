"""fs_landmarks_in_view at the boundary: declared in include/fitslam_frontier.h with its 20-byte entry, exported by
the library, listed in EXPORTED_SYMBOLS, bound with the declared number of arguments, its entry mirrored by VIEW_DTYPE and
ViewLandmarkC, and the ABI version unchanged.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", "fitslam_frontier.h"), os.path.join(ROOT, "include", "fitslam_frontier_dev.h")]


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_header_declares_the_call_and_the_entry():
    text = _text(HEADERS[0])
    m = re.search(r"\bint\s+fs_landmarks_in_view\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "fs_landmarks_in_view is not declared"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["fs_ctx *ctx", "int32_t n", "const double *pose7", "int64_t max_total", "int64_t *offsets", "fs_view_landmark *out"]
    s = re.search(r"typedef\s+struct\s+fs_view_landmark\s*\{(.*?)\}\s*fs_view_landmark\s*;", text, flags=re.S)
    assert s, "fs_view_landmark is not declared"
    fields = [re.sub(r"\s+", " ", f).strip() for f in s.group(1).split(";") if f.strip()]
    assert fields == ["int32_t index", "float p_camera[3]", "float table_value"]
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", text)


def test_the_entry_is_twenty_bytes_for_a_c_compiler(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "view.c"
    src.write_text('#include <stddef.h>\n#include "fitslam_frontier.h"\n'
                   "typedef char size_is_20[sizeof(fs_view_landmark) == 20 ? 1 : -1];\n"
                   "typedef char index_at_0[offsetof(fs_view_landmark, index) == 0 ? 1 : -1];\n"
                   "typedef char p_at_4[offsetof(fs_view_landmark, p_camera) == 4 ? 1 : -1];\n"
                   "typedef char value_at_16[offsetof(fs_view_landmark, table_value) == 16 ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    res = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_exported_symbols_equal_the_declared_set(fs):
    declared = set()
    for h in HEADERS:
        declared |= set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", _text(h)))
    assert "fs_landmarks_in_view" in declared
    assert declared == set(fs.capi.EXPORTED_SYMBOLS)
    assert len(fs.capi.EXPORTED_SYMBOLS) == len(set(fs.capi.EXPORTED_SYMBOLS))


def test_library_exports_and_binds_the_call(fs):
    L = fs.load_library()
    f = getattr(L, "fs_landmarks_in_view")
    assert f.argtypes is not None and len(f.argtypes) == 6
    assert L.fs_abi_version() == 1
    assert callable(fs.FrontierScorer.landmarks_in_view)


def test_view_dtype_layout(fs):
    E = fs.capi
    assert E.VIEW_DTYPE.itemsize == 20 == ctypes.sizeof(E.ViewLandmarkC)
    assert E.VIEW_DTYPE.names == ("index", "p_camera", "table_value")
    assert [E.VIEW_DTYPE.fields[k][1] for k in E.VIEW_DTYPE.names] == [0, 4, 16]
    assert E.VIEW_DTYPE.fields["index"][0] == np.dtype("<i4") and E.VIEW_DTYPE.fields["table_value"][0] == np.dtype("<f4")
    assert E.VIEW_DTYPE.fields["p_camera"][0] == np.dtype(("<f4", (3,)))
    assert [(getattr(E.ViewLandmarkC, k).offset, getattr(E.ViewLandmarkC, k).size) for k in E.VIEW_DTYPE.names] == [(0, 4), (4, 12), (16, 4)]


def test_null_context_is_refused_and_nothing_is_written(fs):
    L = fs.load_library()
    off = np.full(3, 77, dtype=np.int64)
    out = np.full(4, 0x5A, dtype=np.uint8).repeat(20).view(fs.capi.VIEW_DTYPE)
    pose = np.zeros((2, 7))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.fs_landmarks_in_view(None, 2, p(pose), 4, p(off), p(out)) == fs.capi.FS_E_INVALID
    assert L.fs_landmarks_in_view(None, 0, None, 0, None, None) == fs.capi.FS_E_INVALID
    assert (off == 77).all() and (out.view(np.uint8) == 0x5A).all()
