"""The roadmaps and robots the roadmap-route tests share: test_gpu_roadmap_astar.py's maps and its _setup recipe for
the restatement alone (no device), the robot on the free cell drawn by planner_ref.free_cells(cells, default_rng(3), 1), and the
goal list that asks for the route to every node."""
import zlib

import numpy as np

import planner_ref as P
import roadmap_ref as R
import roadmap_route_ref as RR
from test_gpu_roadmap_astar import RES, _map, _nodes


def node_points(name):
    cells, origin = _map(name)
    return _nodes(cells, origin, zlib.crc32(name.encode()), int(min(1500, max(40, cells.size * RES * RES / 2))))


def restated_roadmap(name):
    """(restatement with _setup's roadmap of the map, cells, origin, the node points handed to populate)"""
    cells, origin = _map(name)
    ref = RR.RouteRoadmap(cells, origin, RES)
    pts = node_points(name)
    assert ref.populate(pts) == 0
    ref.rebuild()
    return ref, cells, origin, pts


def robot_pose(cells, origin, yaw=0.3):
    xs, ys = P.free_cells(cells, np.random.default_rng(3), 1)
    return R.pose7(origin[0] + (xs[0] + 0.5) * RES, origin[1] + (ys[0] + 0.5) * RES, yaw)


def goals_at_nodes(xy):
    g = np.zeros((xy.shape[0], 3))
    g[:, :2] = xy
    return g
