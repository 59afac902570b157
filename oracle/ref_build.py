"""Builds oracle/_ref/libfitslam_ref.so: the units of the reference that compile without ROS 2 — its task allocator (Hungarian,
MinPos, TaskAllocator), its grid planner (NavFn) and its Theta* — from the reference's own source files, read where they lie
(FS_REFERENCE_DIR), behind the extern "C" wrappers of oracle/ref_wrap/ and the stand-in headers of oracle/ref_shim/.
TEST INFRASTRUCTURE ONLY: nothing of the reference is copied into this repository, and oracle/_ref/ stays out of git.

The scoring path, the roadmap and the roadmap's A* are not built: they need Eigen and the ROS message types (DESIGN.md "Oracle")."""
from __future__ import annotations

import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(_HERE, "_ref")
SO = os.path.join(OUT_DIR, "libfitslam_ref.so")
SYMBOLS = ("ref_hungarian", "ref_minpos", "ref_navfn_plan", "ref_navfn_path_on_field", "ref_navfn_fixed_point", "ref_theta_leg")
# no -march=native: the library travels to the GPU box like libfso_oracle.so does; no FMA contraction: bits are compared
FLAGS = ("-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared")
_PKG = os.path.join("dev_ws", "src", "DEPRECATED", "frontier_exploration")
_ALLOC = os.path.join(_PKG, "frontier_multirobot_allocator")
_EXPL = os.path.join(_PKG, "frontier_exploration")
# compiled as translation units of their own
_REF_SOURCES = (os.path.join(_ALLOC, "src", "hungarian", "Hungarian.cpp"), os.path.join(_ALLOC, "src", "minPos", "minPos.cpp"),
                os.path.join(_ALLOC, "src", "taskAllocator.cpp"), os.path.join(_EXPL, "src", "planners", "theta_star.cpp"))
# read through an #include (planner.cpp by oracle/ref_wrap/ref_navfn.cpp, see there)
_REF_INCLUDED = (os.path.join(_EXPL, "src", "planners", "planner.cpp"), os.path.join(_EXPL, "include", "frontier_exploration", "planners", "planner.hpp"),
                 os.path.join(_EXPL, "include", "frontier_exploration", "planners", "theta_star.hpp"),
                 os.path.join(_ALLOC, "include", "frontier_multirobot_allocator", "hungarian", "Hungarian.h"),
                 os.path.join(_ALLOC, "include", "frontier_multirobot_allocator", "minPos", "minPos.hpp"),
                 os.path.join(_ALLOC, "include", "frontier_multirobot_allocator", "taskAllocator.hpp"))
_REF_INCLUDE_DIRS = (os.path.join(_ALLOC, "include"), os.path.join(_EXPL, "include"), os.path.join(_EXPL, "src"))


def reference_dir() -> str:
    return os.environ.get("FS_REFERENCE_DIR") or "/root/reference"


def reference_present() -> bool:
    ref = reference_dir()
    return all(os.path.exists(os.path.join(ref, s)) for s in _REF_SOURCES + _REF_INCLUDED)


def available() -> bool:
    """the library exists (built here, or carried over from the machine that built it)"""
    return os.path.exists(SO)


def _own_files():
    out = [os.path.abspath(__file__)]
    for sub in ("ref_wrap", "ref_shim"):
        for d, _, names in os.walk(os.path.join(_HERE, sub)):
            out += [os.path.join(d, n) for n in names if n.endswith((".cpp", ".hpp", ".h"))]
    return sorted(out)


def build(force: bool = False) -> str:
    """Compile the library if it is missing or older than a wrapper, a stand-in header or a reference source.  With the reference
    tree present a failed compile raises; without it an existing library is left alone."""
    if not reference_present():
        return SO
    ref = reference_dir()
    deps = _own_files() + [os.path.join(ref, s) for s in _REF_SOURCES + _REF_INCLUDED]
    stale = (not os.path.exists(SO)) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps)
    if not (force or stale):
        return SO
    os.makedirs(OUT_DIR, exist_ok=True)
    wrappers = sorted(f for f in _own_files() if f.endswith(".cpp"))
    tmp = f"{SO}.tmp{os.getpid()}"
    cmd = [os.environ.get("CXX") or "g++", *FLAGS, "-I" + os.path.join(_HERE, "ref_shim"), "-I" + os.path.join(_HERE, "ref_wrap"),
           *("-I" + os.path.join(ref, d) for d in _REF_INCLUDE_DIRS), "-o", tmp, *wrappers, *(os.path.join(ref, s) for s in _REF_SOURCES)]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if done.returncode != 0:
            raise RuntimeError("oracle/_ref: the reference's sources did not compile\n" + " ".join(cmd) + "\n" + done.stdout[-4000:])
        os.replace(tmp, SO)          # (atomic: a test session that builds at the same time never loads half a file)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return SO


if __name__ == "__main__":
    print(build(force=True))
