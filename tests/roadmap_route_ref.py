"""Loader of tests/roadmap_route_ref/roadmap_route_ref.cpp, the CPU restatement of the roadmap routes: getPlan's node
lists under both roadmap searches, refinePath and the leg poses.  It includes tests/roadmap_ref/roadmap_ref.cpp unchanged.  Compiled by g++ -O2 -ffp-contract=off into a
temporary directory on first use and linked against the oracle's libfso_oracle.so."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

import roadmap_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "roadmap_route_ref", "roadmap_route_ref.cpp")
TREE, REFERENCE_ASTAR = R.TREE, R.REFERENCE_ASTAR
_lib = None


def lib():
    global _lib
    if _lib is None:
        if os.path.join(R.ROOT, "oracle") not in sys.path:
            sys.path.insert(0, os.path.join(R.ROOT, "oracle"))
        import oracle as O
        so = O.build()
        out = os.path.join(tempfile.mkdtemp(prefix="roadmap_route_ref_"), "libroadmap_route_ref.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC, so,
                        "-Wl,-rpath," + os.path.dirname(os.path.abspath(so))], check=True)
        L = C.CDLL(out)
        vp, ci, cd, ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong
        L.rrt_routes.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, C.POINTER(ci), vp, ll, C.POINTER(ll), vp, vp, vp]
        L.rrt_refine.argtypes = [vp, vp, ci, ci, cd, cd, cd, cd, ci, vp, vp, vp, vp, vp, C.POINTER(ll)]
        L.rrt_refine.restype = ll
        L.rrt_leg_poses.argtypes = [vp, ci, vp, vp, vp]
        L.rrt_leg_poses.restype = ll
        _lib = L
    return _lib


_p = R._p


class RouteRoadmap(R.Roadmap):
    """roadmap_ref.Roadmap with the route legs.  The roadmap itself is made and grown by roadmap_ref's library; this module's library
    compiles the same source (it includes roadmap_ref.cpp), so it reads the same object through the same handle."""

    def routes(self, robot_pose7, goal_xyz, achievable_in=None, leg=TREE):
        """route_of [n]; goal_node, length_m [routes]; node_offset [routes + 1], node [total]"""
        goal = np.ascontiguousarray(goal_xyz, dtype=np.float64).reshape(-1, 3)
        n = goal.shape[0]
        pose = np.ascontiguousarray(robot_pose7, dtype=np.float64).reshape(7)
        ai = None if achievable_in is None else np.ascontiguousarray(achievable_in, dtype=np.uint8)
        route_of = np.zeros(n, np.int32)
        nr, total = C.c_int(), C.c_longlong()
        rooms = (0, 0)
        for _ in range(2):
            gn = np.zeros(max(rooms[0], 1), np.int32); off = np.zeros(rooms[0] + 1, np.int64)
            node = np.zeros(max(rooms[1], 1), np.int32); length = np.zeros(max(rooms[0], 1))
            rc = lib().rrt_routes(self._h, _p(pose), n, _p(goal), _p(ai), int(leg), _p(route_of), rooms[0], C.byref(nr), _p(gn), rooms[1],
                                 C.byref(total), _p(off), _p(node), _p(length))
            if rc != R.FS_E_RANGE:
                break
            rooms = (nr.value, total.value)
        assert rc == 0
        return dict(route_of=route_of, goal_node=gn[:nr.value], node_offset=off[:nr.value + 1], node=node[:total.value],
                    length_m=length[:nr.value])

    def refine(self, node_offset, node):
        """refinePath of every list on the grid this roadmap holds NOW (self.cells): refined_offset, refined_node, complete, walks"""
        off = np.ascontiguousarray(node_offset, dtype=np.int64)
        nd = np.ascontiguousarray(node, dtype=np.int32)
        k = off.size - 1
        roff = np.zeros(k + 1, np.int64); ref = np.zeros(max(nd.size, 1), np.int32); comp = np.zeros(max(k, 1), np.uint8)
        walks = C.c_longlong()
        total = lib().rrt_refine(self._h, *self._grid(), k, _p(off), _p(nd), _p(roff), _p(ref), _p(comp), C.byref(walks))
        return dict(refined_offset=roff, refined_node=ref[:total], complete=comp[:k], walks=walks.value)

    def leg_poses(self, offset, nodes):
        off = np.ascontiguousarray(offset, dtype=np.int64)
        nd = np.ascontiguousarray(nodes, dtype=np.int32)
        k = off.size - 1
        legs = int(nd.size - k) if k else 0
        p7 = np.zeros((max(legs, 1), 7))
        got = lib().rrt_leg_poses(self._h, k, _p(off), _p(nd), _p(p7))
        assert got == legs
        return p7[:legs]


def summed_from_goal_end(xy, nodes):
    """the route's segment lengths summed from the goal end, as astar.cpp:57-63 does (a sequential fp64 loop)"""
    total = 0.0
    for k in range(len(nodes) - 1, 0, -1):
        e = xy[nodes[k]] - xy[nodes[k - 1]]
        total += float(np.sqrt(e[0] * e[0] + e[1] * e[1]))
    return total
