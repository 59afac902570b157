"""fs_roadmap_update and fs_get_frontier_costs_searched_roadmap in the public header and the ctypes binding (no GPU): both declared,
both bound with as many arguments as the header declares, FS_ABI_VERSION unchanged."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read()
NAMES = ("fs_roadmap_update", "fs_get_frontier_costs_searched_roadmap")


def _declared_args(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in fitslam_frontier.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [a.strip() for a in body.split(",")]


def test_header_declares_both():
    upd = _declared_args("fs_roadmap_update")
    assert len(upd) == 8 and "robot_xy[2]" in upd[3] and "add_robot_pose" in upd[4] and "int64_t" in upd[7]
    tick, searched = _declared_args("fs_get_frontier_costs_searched_roadmap"), _declared_args("fs_get_frontier_costs_searched")
    # fs_get_frontier_costs_searched's list without allow_unknown and with add_robot_pose
    assert len(tick) == len(searched)
    assert [a for a in tick if "add_robot_pose" not in a] == [a for a in searched if "allow_unknown" not in a]


def test_binding_matches_the_header():
    capi = importlib.import_module("fit-slam_amd.capi")
    L = capi.load_library()
    for name in NAMES:
        assert name in capi.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == len(_declared_args(name)), name
    assert hasattr(capi.FrontierScorer, "roadmap_update") and hasattr(capi.FrontierScorer, "get_frontier_costs_searched_roadmap")


def test_abi_version_stays_1():
    capi = importlib.import_module("fit-slam_amd.capi")
    assert capi.load_library().fs_abi_version() == 1
    assert re.search(r"#define\s+FS_ABI_VERSION\s+1\b", HEADER)
