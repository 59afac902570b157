"""A Python restatement of the outer search of FrontierSearch::searchFrom (DEP/src/FrontierSearch.cpp:44-94) that records depths:
the start cell (nearestFreeCell's result, or the robot's cell), the FIFO over cells below 254 inside the search radius in nhood4
order, and per component (the oracle's cell_seed) the first frontier neighbour of a popped cell.  Levels are counted from 1 at the
start cell, as the device's counters 1019 / 1020 count them."""
from collections import deque

import numpy as np


def _world_to_map(origin, res, nx, ny, pos):
    if pos[0] < origin[0] or pos[1] < origin[1]:
        return None
    mx, my = int((pos[0] - origin[0]) / res), int((pos[1] - origin[1]) / res)
    return (mx, my) if mx < nx and my < ny else None


def _nearest_free(m, nx, ny, start, val):
    seen = bytearray(nx * ny)
    q = deque([start])
    seen[start] = 1
    while q:
        i = q.popleft()
        if m[i] < val:
            return i
        y, x = divmod(i, nx)
        l, r, u, d = x > 0, x < nx - 1, y > 0, y < ny - 1
        for ok, j in ((l, i - 1), (r, i + 1), (u, i - nx), (d, i + nx), (l and u, i - 1 - nx), (l and d, i - 1 + nx),
                      (r and u, i + 1 - nx), (r and d, i + 1 + nx)):
            if ok and not seen[j]:
                seen[j] = 1
                q.append(j)
    return None


def outer_search(cells, origin, res, pos, cell_seed, lethal_threshold=160, max_cluster=20, max_distance=50.0):
    """dict(seeds: the seed cells in output order, first_level: per seed the level of the popped cell that met it, levels: the
    level of the last first meeting (0: no component), popped: cells of levels 1..levels, depth: the deepest level of the whole
    search); None when the robot is off the map.  cell_seed [ny][nx]: the oracle's, which names each found component."""
    ny, nx = cells.shape
    mp = _world_to_map(origin, res, nx, ny, pos)
    if mp is None:
        return None
    m = cells.ravel().tolist()
    comp = np.asarray(cell_seed).ravel().tolist()
    start = mp[1] * nx + mp[0]
    s = _nearest_free(m, nx, ny, start, lethal_threshold & 0xFF)
    if s is not None:
        start = s
    reach = max_distance + (max_cluster * res * 1.414)
    visited = bytearray(nx * ny)
    visited[start] = 1
    level = {start: 1}
    q = deque([start])
    met, seeds, first_level = set(), [], []
    popped_at = [0]                                   # popped_at[L]: cells of levels 1..L
    while q:
        i = q.popleft()
        li = level[i]
        while len(popped_at) <= li:
            popped_at.append(popped_at[-1])
        popped_at[li] += 1
        y, x = divmod(i, nx)
        for ok, j in ((x > 0, i - 1), (x < nx - 1, i + 1), (y > 0, i - nx), (y < ny - 1, i + nx)):
            if not ok:
                continue
            if m[j] < 254 and not visited[j]:
                visited[j] = 1
                jy, jx = divmod(j, nx)
                wx, wy = origin[0] + (jx + 0.5) * res, origin[1] + (jy + 0.5) * res
                if np.sqrt((pos[0] - wx) ** 2 + (pos[1] - wy) ** 2) < reach:
                    level[j] = li + 1
                    q.append(j)
            elif comp[j] >= 0 and comp[j] not in met:
                met.add(comp[j])
                seeds.append(j)
                first_level.append(li)
    levels = max(first_level) if first_level else 0
    return dict(seeds=np.array(seeds, np.int32), first_level=np.array(first_level, np.int32), levels=levels,
                popped=popped_at[levels] if levels else 0, depth=len(popped_at) - 1)
