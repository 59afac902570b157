"""fs_roadmap_routes on the C ABI, without a GPU: the header declares the call and its parameter struct after
fs_get_frontier_costs_roadmap, the library exports it, the binding lists it and lays the struct out as the header does, and it
refuses a missing context."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_call_after_the_fused_roadmap_call(fs):
    text = open(os.path.join(ROOT, "include", "fitslam_frontier.h")).read()
    m = re.search(r"typedef struct fs_route_params \{\s*int32_t refine;[^}]*int32_t with_information;[^}]*double\s+fi_threshold;[^}]*\} fs_route_params;", text)
    assert m
    call = re.search(r"^int fs_roadmap_routes\(fs_ctx \*ctx, const double robot_pose7\[7\], int32_t n, const double \*goal_xyz,", text, re.M)
    assert call
    assert text.index("int fs_get_frontier_costs_roadmap(") < m.start() < call.start() < text.index("Key-frame anchors")
    for counter in ("1026", "1027", "1028", "1029"):
        assert counter in text[m.start():text.index("Key-frame anchors")]


def test_binding_lists_the_symbol_and_the_struct(fs):
    assert "fs_roadmap_routes" in fs.capi.EXPORTED_SYMBOLS
    P = fs.capi.RouteParamsC
    assert [f[0] for f in P._fields_] == ["refine", "with_information", "fi_threshold"]
    assert C.sizeof(P) == 16 and P.fi_threshold.offset == 8 and P.with_information.offset == 4
    assert callable(getattr(fs.capi.FrontierScorer, "roadmap_routes", None))


def test_library_exports_the_call_and_refuses_a_null_context(fs):
    lib = fs.load_library()
    assert hasattr(lib, "fs_roadmap_routes")
    pose = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    n_routes = C.c_int32(-7)
    args = [None, C.byref(pose), 0, None, None, None] + [None] * 5 + [0, C.byref(n_routes)] + [None] * 6 + [0, None, None, None, None, None, None, None, None]
    assert len(args) == len(lib.fs_roadmap_routes.argtypes)
    assert lib.fs_roadmap_routes(*args) == fs.capi.FS_E_INVALID
    assert n_routes.value == -7
