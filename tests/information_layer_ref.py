"""CPU restatement of the information layer (include/fitslam_frontier.h) — this project's own extension, the
reference has no such layer: block geometry, anchors, heading pairs, poses, the three reductions, the cost formula and the store
in numpy, the values from oracle.pose_information; the test maps and the two-door planning scenario.  Checker only."""
import functools
import importlib

import numpy as np

RES = 0.05
REL = 1e-4                                   # info_ref against the oracle's fp64 sum
REDUCE = ("min", "mean", "max")


# ---- the rule

def blocks(window, s):
    """(nbx, nby) of the window (x0, y0, sx, sy) at stride s"""
    return -(-window[2] // s), -(-window[3] // s)


def block_box(window, s, i, j):
    """cells [bx0, bx1) x [by0, by1) of block (i, j) and its centre cell"""
    x0, y0, sx, sy = window
    bx0, by0 = x0 + i * s, y0 + j * s
    bx1, by1 = min(bx0 + s, x0 + sx), min(by0 + s, y0 + sy)
    return bx0, by0, bx1, by1, min(bx0 + s // 2, x0 + sx - 1), min(by0 + s // 2, y0 + sy - 1)


def anchors(cells, window, s):
    """anchor_cell [nby][nbx] int32: y * nx + x of the writable cell (<= 252) nearest the centre cell, ties to the smaller y, then
    the smaller x; -1 for a block without one"""
    ny, nx = cells.shape
    nbx, nby = blocks(window, s)
    out = np.full((nby, nbx), -1, dtype=np.int32)
    for j in range(nby):
        for i in range(nbx):
            bx0, by0, bx1, by1, cx, cy = block_box(window, s, i, j)
            yy, xx = np.nonzero(cells[by0:by1, bx0:bx1] <= 252)             # (row-major: y, then x, ascending)
            if yy.size == 0:
                continue
            d2 = (xx + bx0 - cx) ** 2 + (yy + by0 - cy) ** 2
            k = int(np.argmin(d2))                                           # (the first minimum: smallest y, then x)
            out[j, i] = (by0 + yy[k]) * nx + bx0 + xx[k]
    return out


def anchors_brute(cells, window, s):
    """the same, cell by cell with an explicit (d2, y, x) comparison"""
    ny, nx = cells.shape
    nbx, nby = blocks(window, s)
    out = np.full((nby, nbx), -1, dtype=np.int32)
    for j in range(nby):
        for i in range(nbx):
            bx0, by0, bx1, by1, cx, cy = block_box(window, s, i, j)
            best = None
            for y in range(by0, by1):
                for x in range(bx0, bx1):
                    if cells[y, x] <= 252:
                        key = ((x - cx) ** 2 + (y - cy) ** 2, y, x)
                        if best is None or key < best:
                            best = key
            if best is not None:
                out[j, i] = best[1] * nx + best[2]
    return out


def quat_zw(n_yaw, yaw0=0.0):
    """[K][2]: sin, cos of half of yaw0 + k * (2 pi / K)"""
    psi = np.array([yaw0 + k * (2.0 * np.pi / n_yaw) for k in range(n_yaw)], dtype=np.float64)
    return np.stack([np.sin(psi / 2.0), np.cos(psi / 2.0)], axis=1)


def poses(anchor, quat, nx, origin, res=RES, pose_z=0.0):
    """pose7 [n_scored * K][7]: scored blocks in block order, headings in order"""
    cells = anchor.reshape(-1)
    cells = cells[cells >= 0].astype(np.int64)
    K = quat.shape[0]
    p = np.zeros((cells.size, K, 7))
    p[:, :, 0] = (origin[0] + ((cells % nx).astype(np.float64) + 0.5) * res)[:, None]
    p[:, :, 1] = (origin[1] + ((cells // nx).astype(np.float64) + 0.5) * res)[:, None]
    p[:, :, 2] = pose_z
    p[:, :, 5] = quat[None, :, 0]
    p[:, :, 6] = quat[None, :, 1]
    return p.reshape(-1, 7)


def per_yaw_field(anchor, values, n_yaw):
    """info_per_yaw [K][nby][nbx] float32 from the values of poses(...) in their order; NaN where unscored"""
    out = np.full((n_yaw,) + anchor.shape, np.nan, dtype=np.float32)
    scored = anchor >= 0
    out[:, scored] = np.asarray(values, dtype=np.float32).reshape(-1, n_yaw).T
    return out


def reduce_field(per_yaw, reduce):
    """[nby][nbx] float32: min / max in float; mean = the fp64 sum in k order (a sequential loop: numpy's sum is pairwise), / K,
    rounded once"""
    K = per_yaw.shape[0]
    if reduce == "min":
        return per_yaw.min(axis=0)
    if reduce == "max":
        return per_yaw.max(axis=0)
    assert reduce == "mean"
    total = np.zeros(per_yaw.shape[1:], dtype=np.float64)
    for k in range(K):
        total = total + per_yaw[k].astype(np.float64)
    return (total / float(K)).astype(np.float32)


def cost_of(v, info_lo, info_hi, max_cost):
    """the header's step 6 on float32 values (NaN: 0): fp64 subtract, divide, clamp, one multiply, truncation"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = (np.float64(info_hi) - v.astype(np.float64)) / (np.float64(info_hi) - np.float64(info_lo))
        t = np.where(t > 0, t, 0.0)
        t = np.where(t > 1, 1.0, t)
    return (np.float64(max_cost) * t).astype(np.int64).astype(np.uint8)


def store(cells, window, s, anchor, cost):
    """(grid after the store, n_changed): every writable cell of a scored block becomes max(old, cost)"""
    out = cells.copy()
    nbx, nby = blocks(window, s)
    for j in range(nby):
        for i in range(nbx):
            if anchor[j, i] < 0:
                continue
            bx0, by0, bx1, by1, _, _ = block_box(window, s, i, j)
            blk = out[by0:by1, bx0:bx1]
            blk[...] = np.where(blk <= 252, np.maximum(blk, cost[j, i]), blk)
    return out, int((out != cells).sum())


def layer(cells, window, s, per_yaw, reduce, info_lo, info_hi, max_cost):
    """dict(info, cost [nby][nbx] (0 where unscored), grid, n_changed, anchor, n_scored) from a per-heading field"""
    anchor = anchors(cells, window, s)
    info = reduce_field(per_yaw, reduce)
    cost = np.where(anchor >= 0, cost_of(info, info_lo, info_hi, max_cost), 0).astype(np.uint8)
    grid, n_changed = store(cells, window, s, anchor, cost)
    return dict(info=info, cost=cost, grid=grid, n_changed=n_changed, anchor=anchor, n_scored=int((anchor >= 0).sum()))


def oracle_values(oracle, table, landmarks, pose7, vis):
    """the oracle's fp64 scalar of every pose; equal poses are scored once"""
    if pose7.shape[0] == 0:
        return np.zeros(0)
    uniq, inverse = np.unique(pose7, axis=0, return_inverse=True)
    want = oracle.pose_information(table, landmarks, uniq, vis[0], vis[1], n_threads=16)["info_f64"]
    return want[inverse.reshape(-1)]


# The comparison of cost bytes with bytes made from the oracle's values: a block within the 1e-4 bar of a quantisation edge may differ
# by one.  An edge every (hi - lo) / max_cost and a bar 2e-4 v wide put 2e-4 v max_cost / (hi - lo) of the blocks there: on the
# test maps (v about 1000, a spread of 100 .. 200 between the blocks) max_cost 8 over twice the spread keeps that near 0.5 %.
EDGE_COST = 8
EDGE_CASES = ((3, 4, (14.0, 1.0)), (7, 4, (14.0, 4.0)))      # (stride, K, visibility) on the whole map: the oracle alone has <= 1 % there


def edge_range(v64):
    """(info_lo, info_hi) of that comparison: the values' range grown by 0.45 of it on either side (half of it would put the
    smallest and the largest value exactly on edges 6 / 8 and 2 / 8)"""
    lo, hi = float(v64.min()), float(v64.max())
    return lo - 0.45 * (hi - lo), hi + 0.45 * (hi - lo)


def near_edge(v64, info_lo, info_hi, max_cost, rel=REL):
    """blocks whose value, moved by the bar either way, falls into another cost byte"""
    lo = cost_of((v64 * (1.0 - rel)).astype(np.float32), info_lo, info_hi, max_cost)
    hi = cost_of((v64 * (1.0 + rel)).astype(np.float32), info_lo, info_hi, max_cost)
    return lo != hi


# ---- the test maps: rooms in unknown space with walls on their borders (synth's floor plan), unknown patches, two long walls

MAPS = {"96x80": (41, 80, 96), "130x70": (42, 70, 130)}            # seed, ny, nx
ORIGIN = (-1.0, -2.0, 0.0)
N_LANDMARKS = 3000


@functools.lru_cache(maxsize=None)
def layer_map(name):
    """(cells [ny][nx], landmarks [3000][3] on obstacle cells, heights U(0, 2.5 m))"""
    synth = importlib.import_module("fit-slam_amd").synth
    seed, ny, nx = MAPS[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = np.ascontiguousarray(synth._floor_plan(rng, max(ny, nx))[:ny, :nx])
    cells[ny // 3:ny // 3 + 2, 8:nx - 8] = 254                       # walls across the rooms
    cells[ny // 3:ny // 3 + 2, nx // 2:nx // 2 + 6] = 0
    cells[10:ny - 10, 2 * nx // 3] = 254
    for _ in range(6):
        y, x = int(rng.integers(0, ny - 12)), int(rng.integers(0, nx - 12))
        cells[y:y + int(rng.integers(4, 12)), x:x + int(rng.integers(4, 12))] = 255
    cells[0:7, 0:9] = 255                                            # a corner no stride of the tests finds a writable cell in
    lm = synth._landmarks(rng, cells[None], ORIGIN, RES, N_LANDMARKS)
    lm[:, 2] = rng.uniform(0.0, 2.5, size=lm.shape[0]).astype(np.float32)
    cells.setflags(write=False)
    lm.setflags(write=False)
    return cells, lm


# ---- the planning scenario: a wall with two doors, few landmarks near the door of the short route, many near the other

SCENE_NX, SCENE_NY = 160, 120
SCENE_ORIGIN = (0.0, 0.0, 0.0)
SCENE_VIS = (2.5, 4.0)                                               # information is local on an 8 m map
SCENE_WALL = (58, 62)                                                # rows [58, 62)
SCENE_DOOR_A, SCENE_DOOR_B = (40, 52), (120, 132)                    # columns
SCENE_ROBOT, SCENE_GOAL = (46, 20), (46, 100)                        # cells (x, y)
SCENE_INFLATION = (0.30, 0.05, 3.0)
SCENE_LAYER = dict(stride_cells=4, n_yaw=8, reduce="mean", max_cost=252)
SCENE_THRESHOLD = 600.0                                              # fi_threshold and info_lo: between the two routes' minima (165 and 1079)
SCENE_PATH = dict(sample_distance_m=0.5, lookahead_points=10)


@functools.lru_cache(maxsize=None)
def scene():
    """(cells [120][160], landmarks): free space, a border wall, the wall with its two doors"""
    cells = np.zeros((SCENE_NY, SCENE_NX), dtype=np.uint8)
    cells[:2, :] = cells[-2:, :] = 254
    cells[:, :2] = cells[:, -2:] = 254
    cells[SCENE_WALL[0]:SCENE_WALL[1], :] = 254
    cells[SCENE_WALL[0]:SCENE_WALL[1], SCENE_DOOR_A[0]:SCENE_DOOR_A[1]] = 0
    cells[SCENE_WALL[0]:SCENE_WALL[1], SCENE_DOOR_B[0]:SCENE_DOOR_B[1]] = 0
    rng = np.random.Generator(np.random.PCG64(4270))
    w, h = SCENE_NX * RES, SCENE_NY * RES
    # a thin cloud left of x = 4.4 m (door A's side), a dense one right of it; a cluster behind the robot and one behind the goal,
    # so that both ends of either route are safe and the stretch through door A is not
    thin = rng.uniform((0.2, 0.2, 0.0), (4.4, h - 0.2, 2.0), size=(120, 3))
    dense = rng.uniform((4.6, 0.2, 0.0), (w - 0.2, h - 0.2, 2.0), size=(5200, 3))
    rx, ry = (SCENE_ROBOT[0] + 0.5) * RES, (SCENE_ROBOT[1] + 0.5) * RES
    gx, gy = (SCENE_GOAL[0] + 0.5) * RES, (SCENE_GOAL[1] + 0.5) * RES
    near_r = rng.uniform((rx - 1.6, 0.2, 0.0), (rx + 2.2, ry, 2.0), size=(1500, 3))
    near_g = rng.uniform((gx - 1.6, gy, 0.0), (gx + 2.2, h - 0.2, 2.0), size=(1500, 3))
    lm = np.concatenate([thin, dense, near_r, near_g]).astype(np.float32)
    cells.setflags(write=False)
    lm.setflags(write=False)
    return cells, lm


def scene_pose(cell):
    return np.array([(cell[0] + 0.5) * RES, (cell[1] + 0.5) * RES, 0.0, 0.0, 0.0, 0.0, 1.0])


def scene_goal():
    return np.array([[(SCENE_GOAL[0] + 0.5) * RES, (SCENE_GOAL[1] + 0.5) * RES, 0.0]])


def door_of(waypoint_xy):
    """'A' | 'B' | None: the door whose columns the way points cross the wall's rows in"""
    x = np.floor(waypoint_xy[:, 0] / RES).astype(int)
    y = np.floor(waypoint_xy[:, 1] / RES).astype(int)
    inside = (y >= SCENE_WALL[0] - 6) & (y < SCENE_WALL[1] + 6)        # (16 rows: a way point every 11 path points falls inside)
    for name, (lo, hi) in (("A", SCENE_DOOR_A), ("B", SCENE_DOOR_B)):
        if inside.any() and ((x[inside] >= lo - 8) & (x[inside] < hi + 8)).all():
            return name
    return None
