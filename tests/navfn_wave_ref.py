"""Loader of tests/navfn_wave_ref/navfn_wave_ref.cpp, the host driver of fit-slam_amd/csrc/fs_navfn_wave.h (the REFERENCE grid
search's wave).  Compiled by g++ -O2 -ffp-contract=off into a temporary directory on first use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import planner_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "navfn_wave_ref", "navfn_wave_ref.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "fit-slam_amd", "csrc")
LIMIT_CYCLES, LIMIT_CAP = 1, 2
CAP = 10000
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="navfn_wave_ref_"), "libnavfn_wave_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", out, SRC], check=True)
        L = C.CDLL(out)
        vp, ci = C.c_void_p, C.c_int
        L.nw_wave.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]
        L.nw_heuristic_table.argtypes = [ci, vp]
        L.nw_hypot_table.argtypes = [ci, vp]
        L.nw_heuristic_table.restype = L.nw_hypot_table.restype = None
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def wave(cost, robot_cell, goal_cell, width=1, cap=CAP):
    """The wave from robot_cell that stops at goal_cell on the cost array `cost` (planner_ref.costs): dict(potarr [ny][nx],
    reached, limit, hash, replays).  width 1: the serial wave; 64: the device's chunked order."""
    cost = np.ascontiguousarray(cost, dtype=np.uint8)
    ny, nx = cost.shape
    pot = np.zeros((ny, nx), dtype=np.float32)
    out = np.zeros(4, dtype=np.int64)
    rc = lib().nw_wave(_p(cost), nx, ny, int(robot_cell[0]), int(robot_cell[1]), int(goal_cell[0]), int(goal_cell[1]), int(width), int(cap),
                       _p(pot), _p(out))
    assert rc == 0
    return dict(potarr=pot, reached=int(out[0]), limit=int(out[1]), hash=int(out[2]), replays=int(out[3]))


def wave_of_cells(cells, robot_cell, goal_cell, allow_unknown=False, width=1, cap=CAP):
    return wave(planner_ref.costs(cells, allow_unknown), robot_cell, goal_cell, width, cap)


def heuristic_tables(side):
    """(the header's float, the reference's with libm's hypot), each [side][side] over 0 <= dx, dy < side"""
    a, b = np.zeros((side, side), dtype=np.float32), np.zeros((side, side), dtype=np.float32)
    lib().nw_heuristic_table(side, _p(a))
    lib().nw_hypot_table(side, _p(b))
    return a, b
