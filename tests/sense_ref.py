"""Pure-Python restatement of the sensor sweep (fs_sense), of surroundingCellsMapped for a batch (fs_goals_mapped) and of the
explored-cell census (fs_grid_census) — what fit-slam_amd/csrc/fs_sense.hip is compared with, bit for bit.

The sweep is this project's own extension; what it walks is the reference's arrival fan, taken from oracle/pyref.py: `Costmap`
(worldToMap), `walk_cells` (getTracedCells + bresenham2D, DEP/src/Helpers.cpp:7-96) and `theta_fan` (DEP/src/CostCalculator.cpp:36),
with the end point and its clamp formed as pyref.arrival_information forms them (:42-48).

  H = DEP/src/Helpers.cpp

`params` is a dict of FrontierScorer.set_ray_params' keyword arguments (max_camera_depth, delta_theta, camera_fov, n_rays, elev,
obst, trace, polygon; anything missing takes that call's default)."""
import math

import numpy as np

from pyref import Costmap, theta_fan, walk_cells

OK, OFF_MAP = 0, 1
DEFAULTS = dict(max_camera_depth=2.0, delta_theta=0.10, camera_fov=1.04, n_rays=0, elev=(0.0,), obst=(240, 254), trace=(255, 255),
                polygon=(-1e300, -1e300, 1e300, 1e300))


def fan_shape(params):
    """(n_yaw, n_elev, window) of the fan"""
    p = {**DEFAULTS, **params}
    return len(theta_fan(p["delta_theta"], p["n_rays"])), len(p["elev"]), int(p["camera_fov"] / p["delta_theta"])


def sense_ref(staged, world, origin, resolution, params, origins, first_ray=None):
    """Returns dict(grid, status, seen_unknown, ray_unknown, n_seen, n_revealed, window): grid = the staged map after the call
    ([nz][ny][nx]), the rest as fs_sense's outputs (window = (x0, y0, z0, sx, sy, sz), sizes 0 when nothing was seen)."""
    p = {**DEFAULTS, **params}
    st, wd = Costmap(staged, origin, resolution), Costmap(world, origin, resolution)
    assert st.cells.shape == wd.cells.shape
    depth, elev, poly = p["max_camera_depth"], tuple(p["elev"]), p["polygon"]
    obst, trace = p["obst"], p["trace"]
    thetas = theta_fan(p["delta_theta"], p["n_rays"])
    n_yaw, k = len(thetas), int(p["camera_fov"] / p["delta_theta"])
    max_length = int(depth / wd.res)                                     # CostCalculator.cpp:28
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    n = origins.shape[0]
    first = np.full(n, -1, dtype=np.int64) if first_ray is None else np.asarray(first_ray, dtype=np.int64).reshape(-1)
    if np.any(first < -1) or np.any(first > n_yaw - k):
        raise ValueError("first_ray outside [-1, n_yaw - window]")
    status = np.zeros(n, dtype=np.int32)
    seen_unknown = np.zeros(n, dtype=np.int32)
    ray_unknown = np.zeros((n, len(elev), n_yaw), dtype=np.int32)
    seen = set()
    for q in range(n):
        sx, sy, sz = (float(v) for v in origins[q])
        used = range(n_yaw) if first[q] < 0 else range(int(first[q]), int(first[q]) + k)
        walks = {}
        ok = wd.world_to_map(sx, sy, sz) is not None
        for e, el in enumerate(elev):
            if not ok:
                break
            dh, dz = depth * math.cos(el), depth * math.sin(el)
            for i in used:
                wx = sx + (dh * math.cos(thetas[i]))                     # :42-43
                wy = sy + (dh * math.sin(thetas[i]))
                wz = sz + dz
                wx = max(poly[0], max(wd.ox, min(poly[2], min(wd.ox + wd.size_in_meters(wd.nx), wx))))   # :47-48
                wy = max(poly[1], max(wd.oy, min(poly[3], min(wd.oy + wd.size_in_meters(wd.ny), wy))))
                wz = max(wd.oz, min(wd.oz + wd.size_in_meters(wd.nz), wz))
                cells = walk_cells(wd, (sx, sy, sz), (wx, wy, wz), float(max_length))
                if cells is None:                                        # :50-55 — the fan aborts: the pose sees nothing
                    ok = False
                    break
                walks[(e, i)] = cells
        if not ok:
            status[q] = OFF_MAP
            continue
        for (e, i), cells in walks.items():
            count = 0
            for c in cells:
                seen.add(c)
                if obst[0] <= wd.cost(*c) <= obst[1]:                    # the wall's face is seen and ends the ray
                    break
                if trace[0] <= st.cost(*c) <= trace[1]:
                    count += 1
            ray_unknown[q, e, i] = count
        seen_unknown[q] = int(ray_unknown[q].sum())
    grid = st.cells.copy()
    n_revealed = 0
    for (x, y, z) in seen:
        if st.cells[z, y, x] == 255 and wd.cells[z, y, x] != 255:
            n_revealed += 1
        grid[z, y, x] = wd.cells[z, y, x]
    if seen:
        lo = [min(c[a] for c in seen) for a in range(3)]
        hi = [max(c[a] for c in seen) for a in range(3)]
        window = (lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1)
    else:
        window = (0, 0, 0, 0, 0, 0)
    return dict(grid=grid, status=status, seen_unknown=seen_unknown, ray_unknown=ray_unknown, n_seen=len(seen), n_revealed=n_revealed,
                window=window, seen=seen)


def nhood4(idx, nx, ny):
    """H:185-216"""
    out = []
    if idx > nx * ny - 1:
        return out
    if idx % nx > 0:
        out.append(idx - 1)
    if idx % nx < nx - 1:
        out.append(idx + 1)
    if idx >= nx:
        out.append(idx - nx)
    if idx < nx * (ny - 1):
        out.append(idx + nx)
    return out


def nhood8(idx, nx, ny):
    """H:224-255"""
    out = nhood4(idx, nx, ny)
    if idx > nx * ny - 1:
        return out
    if idx % nx > 0 and idx >= nx:
        out.append(idx - 1 - nx)
    if idx % nx > 0 and idx < nx * (ny - 1):
        out.append(idx - 1 + nx)
    if idx % nx < nx - 1 and idx >= nx:
        out.append(idx + 1 - nx)
    if idx % nx < nx - 1 and idx < nx * (ny - 1):
        out.append(idx + 1 + nx)
    return out


def nhood20(idx, nx, ny):
    """H:263-275: nhood4 plus the nhood8 of each of those (duplicates kept, as there)"""
    out = nhood4(idx, nx, ny)
    for val in list(out):
        out.extend(nhood8(val, nx, ny))
    return out


def goals_mapped_ref(cells2d, origin, resolution, goals):
    """surroundingCellsMapped (H:98-133) for goals [n][3] -> uint8 [n]"""
    cm = Costmap(cells2d, origin, resolution)
    assert cm.nz == 1
    flat = cm.cells[0].reshape(-1)
    nx, ny = cm.nx, cm.ny
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(goals.shape[0], dtype=np.uint8)
    for g in range(goals.shape[0]):
        m = cm.world_to_map(float(goals[g, 0]), float(goals[g, 1]), cm.oz)
        if m is None:                                                    # H:101-104
            continue
        idx = m[1] * nx + m[0]
        if flat[idx] == 254:                                             # H:106-107
            out[g] = 1
            continue
        if sum(1 for c in nhood8(idx, nx, ny) if flat[c] == 254) >= 3:   # H:110-120
            out[g] = 1
            continue
        out[g] = 0 if any(flat[c] == 255 for c in nhood20(idx, nx, ny)) else 1   # H:121-132
    return out


def border_goals(nx, ny, origin, res, rng, n_random=200):
    """goals [n][3] for goals_mapped: cell centres on every border and corner and one cell inside them, random points, and
    points off the map on every side"""
    cells = [(x, y) for x in range(nx) for y in (0, 1, ny - 2, ny - 1)] + [(x, y) for y in range(ny) for x in (0, 1, nx - 2, nx - 1)]
    g = [((x + 0.5) * res + origin[0], (y + 0.5) * res + origin[1], 0.0) for (x, y) in cells]
    g += [(origin[0] + rng.uniform(0, nx * res), origin[1] + rng.uniform(0, ny * res), 0.0) for _ in range(n_random)]
    g += [(origin[0] - 0.01, origin[1] + 1.0, 0.0), (origin[0] + 1.0, origin[1] - 0.01, 0.0), (origin[0] + nx * res, origin[1] + 1.0, 0.0),
          (origin[0] + 1.0, origin[1] + ny * res + 3.0, 0.0)]
    return np.asarray(g, dtype=np.float64)


def census_ref(cells):
    """the explored-cell counter's figures: known (!= 255), unknown (== 255), lethal (== 254), free (== 0)"""
    c = np.asarray(cells, dtype=np.uint8)
    return dict(known=int((c != 255).sum()), unknown=int((c == 255).sum()), lethal=int((c == 254).sum()), free=int((c == 0).sum()))
