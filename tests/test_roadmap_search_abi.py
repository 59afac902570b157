"""The roadmap search setting (fs_set_roadmap_search) on the C ABI, without a GPU: the header declares it and its two
values, the library exports it, the binding carries the constants, and it refuses a missing context whatever the value."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_roadmap_search(fs):
    text = open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read()
    assert re.search(r"^#define FS_ROADMAP_SEARCH_TREE\s+0\b", text, re.M)
    assert re.search(r"^#define FS_ROADMAP_SEARCH_REFERENCE\s+1\b", text, re.M)
    assert re.search(r"\bint fs_set_roadmap_search\(fs_ctx \*ctx, int32_t search\);", text)


def test_binding_has_the_constants(fs):
    assert "fs_set_roadmap_search" in fs.capi.EXPORTED_SYMBOLS
    assert (fs.capi.FS_ROADMAP_SEARCH_TREE, fs.capi.FS_ROADMAP_SEARCH_REFERENCE) == (0, 1)
    assert fs.capi.ROADMAP_SEARCHES == {"tree": 0, "reference": 1}
    assert callable(getattr(fs.capi.FrontierScorer, "set_roadmap_search", None))


def test_library_exports_the_setter(fs):
    lib = fs.load_library()
    assert hasattr(lib, "fs_set_roadmap_search")
    for search in (0, 1, 2, -1):
        assert lib.fs_set_roadmap_search(None, search) == fs.capi.FS_E_INVALID
