"""The seed-order setting of the frontier search (fs_set_frontier_seed_order) on the C ABI, without a GPU: the
header declares it and its two values, the library exports it, and it refuses a missing context."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_seed_order(fs):
    text = open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read()
    assert re.search(r"^#define FS_SEEDS_NEAREST\s+0\b", text, re.M)
    assert re.search(r"^#define FS_SEEDS_REFERENCE\s+1\b", text, re.M)
    assert re.search(r"\bint fs_set_frontier_seed_order\(fs_ctx \*ctx, int32_t order\);", text)
    assert "fs_set_frontier_seed_order" in fs.capi.EXPORTED_SYMBOLS
    assert (fs.capi.FS_SEEDS_NEAREST, fs.capi.FS_SEEDS_REFERENCE) == (0, 1)
    assert fs.capi.SEED_ORDERS == {"nearest": 0, "reference": 1}


def test_library_exports_the_setter(fs):
    lib = fs.load_library()
    assert hasattr(lib, "fs_set_frontier_seed_order")
    for order in (0, 1, 2):
        assert lib.fs_set_frontier_seed_order(None, order) == fs.capi.FS_E_INVALID
