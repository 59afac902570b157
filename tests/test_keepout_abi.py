"""The keep-out layer's entry points are declared in include/fitslam_frontier.h, exported by the library, bound with
the declared number of arguments, listed in EXPORTED_SYMBOLS and present on FrontierScorer / MultiScorer.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fitslam_frontier.h")

NEW = ["fs_keepout_add_fov", "fs_keepout_add_disc", "fs_keepout_clear", "fs_keepout_get", "fs_mark_lethal_fov", "fs_read_grid_region",
       "fs_multi_keepout_add_fov", "fs_multi_keepout_add_disc", "fs_multi_keepout_clear", "fs_multi_mark_lethal_fov"]


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(fs_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out, text


def test_declared_exported_and_bound(fs):
    decl, text = _declarations()
    L = fs.load_library()
    for name in NEW:
        assert name in decl, name
        assert name in fs.capi.EXPORTED_SYMBOLS, name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == decl[name], (name, decl[name])
    assert decl["fs_keepout_add_fov"] == 7 and decl["fs_keepout_add_disc"] == 6 and decl["fs_keepout_get"] == 5
    assert decl["fs_read_grid_region"] == decl["fs_update_grid_region"] == 10
    assert decl["fs_multi_mark_lethal_fov"] == decl["fs_mark_lethal_fov"] == 5
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", text) and L.fs_abi_version() == 1
    m = re.search(r"#define\s+FS_KEEPOUT_MAX_ZONES\s+(\d+)", text)
    assert m and int(m.group(1)) >= 1024 and int(m.group(1)) == fs.capi.FS_KEEPOUT_MAX_ZONES


def test_methods_of_the_binding(fs):
    for name in ("keepout_add_fov", "keepout_add_disc", "keepout_clear", "keepout_get", "mark_lethal_fov", "read_grid_region"):
        assert callable(getattr(fs.FrontierScorer, name)), name
    for name in ("keepout_add_fov", "keepout_add_disc", "keepout_clear", "mark_lethal_fov"):
        assert callable(getattr(fs.MultiScorer, name)), name


def test_null_context_is_refused(fs):
    L = fs.load_library()
    assert L.fs_keepout_add_fov(None, 0.0, 0.0, 0.0, 3.5, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_keepout_add_disc(None, 0.0, 0.0, 1.7, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_keepout_clear(None) == fs.capi.FS_E_INVALID
    assert L.fs_keepout_get(None, None, None, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_mark_lethal_fov(None, None, None, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_read_grid_region(None, 0, 0, 0, 1, 1, 1, None, 0, 0) == fs.capi.FS_E_INVALID
    assert L.fs_multi_keepout_clear(None) == fs.capi.FS_E_INVALID
