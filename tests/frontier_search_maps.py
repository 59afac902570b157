"""Maps and parameter sets of the frontier-search tests: the synthetic costmaps and hand-built maps of
test_gpu_frontier_clusters, REF2D, floor plans up to 1024^2 and the spiral corridor, each with a robot position on a free cell."""
import importlib

import numpy as np

import planner_ref

fsmod = importlib.import_module("fit-slam_amd")

# (max_frontier_cluster_size, min_frontier_cluster_size, lethal_threshold, max_frontier_distance)
PARAMS = [(20, 1, 160, 50.0), (5, 1, 250, 50.0), (40, 1, 1, 3.0), (200, 1, 160, 50.0)]


def _free_pos(cells, origin, res, k, fx=0.3, fy=0.6):
    free = np.argwhere(cells == 0)
    y, x = free[k % len(free)]
    return (origin[0] + (x + fx) * res, origin[1] + (y + fy) * res)


def maps(large=True, spiral=False):
    """[(name, cells [ny][nx], origin (x, y, z), res, robot_xy)]"""
    out = []
    for seed, n in ((3, 160), (4, 200), (9, 512)):
        w = fsmod.synth.make_small_2d(seed, n=n, n_cand=40)
        c = np.ascontiguousarray(w.cells[0])
        rng = np.random.default_rng(seed)
        for j in range(2):
            out.append((f"small{seed}_{n}_{j}", c, tuple(w.origin), w.resolution, _free_pos(c, w.origin, w.resolution, int(rng.integers(1 << 30)))))
    m = np.full((40, 60), 255, np.uint8)
    m[5:15, 5:25] = 0; m[5:15, 35:55] = 0; m[25:35, 5:25] = 0; m[15:25, 10:12] = 0
    m[14:26, 9] = 254; m[14:26, 12] = 254; m[4, 5:25] = 254
    out.append(("rooms", m, (0.0, 0.0, 0.0), 0.05, (0.5, 0.5)))
    b = np.full((30, 30), 255, np.uint8); b[5:25, 5:25] = 0; b[14:17, 14:17] = 254
    out.append(("blob", b, (0.0, 0.0, 0.0), 0.05, (15.5 * 0.05, 15.5 * 0.05)))
    u = np.full((64, 64), 255, np.uint8); u[40:50, 30:45] = 0; u[45, 44] = 200
    out.append(("unknown_start", u, (-1.0, -2.0, 0.0), 0.05, (-1.0 + 3.2 * 0.05, -2.0 + 2.7 * 0.05)))
    w = fsmod.synth.make_workload("REF2D", n_cand=16, n_landmarks=16)
    c = np.ascontiguousarray(w.cells[0])
    out.append(("REF2D", c, tuple(w.origin), w.resolution, _free_pos(c, w.origin, w.resolution, len(np.argwhere(c == 0)) // 2)))
    rng = np.random.Generator(np.random.PCG64(777))
    for n in ([128, 256, 512, 1024] if large else [128, 256]):
        c = np.ascontiguousarray(fsmod.synth.make_grid(rng, n, 1)[0])
        origin = (-n * 0.05 / 2, -n * 0.05 / 2, 0.0)
        out.append((f"plan_{n}", c, origin, 0.05, _free_pos(c, origin, 0.05, int(rng.integers(1 << 30)))))
    if spiral:
        s = planner_ref.spiral_map(256)[0].copy()
        s[100:156, 100:156] = np.where(s[100:156, 100:156] == 0, 255, s[100:156, 100:156])      # an unknown core: frontiers
        origin = (-6.4, -6.4, 0.0)
        out.append(("spiral", np.ascontiguousarray(s), origin, 0.05, _free_pos(s, origin, 0.05, 0)))
    return out


def robot_cell(cells, origin, res, pos):
    ny, nx = cells.shape
    mx, my = int((pos[0] - origin[0]) / res), int((pos[1] - origin[1]) / res)
    return my * nx + mx


def pieces_from_every(every_cells, seed_order, labels, max_size, shape):
    """cell_piece [ny][nx] in the oracle's numbering from an emission-ordered cell list: per seed the component's cells come
    contiguously, full pieces of max + 1 cells, then the remainder, and one more number after every component."""
    ny, nx = shape
    lab = labels.ravel()
    out = np.full(ny * nx, -1, np.int32)
    t, seq = 0, 0
    for s in seed_order:
        size = int((lab == lab[s]).sum())
        for q in range(size):
            out[every_cells[t + q]] = seq + q // (max_size + 1)
        seq += size // (max_size + 1) + 1
        t += size
    return out.reshape(ny, nx)
