"""The inflation layer of DESIGN.md 4.26 restated on the CPU — a helper, not a test.

`cost_table` is InflationLayer::computeCost (nav2 Humble) for every squared cell distance; `inflate_exact` is the library's rule
(the exact nearest lethal cell) in two independent forms, brute force over offsets and scipy's Euclidean feature transform turned
into integer d2; `inflate_brushfire` is Humble's own ordered propagation (InflationLayer::updateCosts: bins by distance, first
come first served inside a bin, 4-neighbours, every cell carries its source) in plain Python; `grid` builds the test maps."""
import math

import numpy as np

LETHAL, INSCRIBED, UNKNOWN = 254, 253, 255
RES = 0.05
# (inflation_radius, inscribed_radius, cost_scaling_factor): fit_slam2/params/active_slam_nav2_params.yaml — the global costmap's
# inflation_layer :162-163, the local costmap's :137-138, the global lethal_inflation_layer :169-170; robot_radius 0.05
GLOBAL = (5.0, 0.05, 0.6)
LOCAL = (0.60, 0.05, 0.6)
LETHAL_LAYER = (0.3, 0.05, 0.6)
FAR = np.int64(1) << 40


def cell_radius(params, res=RES):
    """Costmap2D::cellDistance"""
    return int(max(0.0, math.ceil(params[0] / res)))


def cost_table(params, res=RES):
    """(R, cost_by_d2 [R * R + 1]); libm through `math`, as the library's host code goes through <cmath>"""
    _, inscribed, scaling = params
    R = cell_radius(params, res)
    table = np.zeros(R * R + 1, dtype=np.uint8)
    for d2 in range(R * R + 1):
        if d2 == 0:
            table[d2] = LETHAL
            continue
        d = math.sqrt(float(d2)) * res
        table[d2] = INSCRIBED if d <= inscribed else int(252 * math.exp(-1.0 * scaling * (d - inscribed)))
    return R, table


def d2_brute(seeds, R):
    """smallest dx^2 + dy^2 <= R^2 to a seed by trying every offset; FAR where there is none"""
    ny, nx = seeds.shape
    out = np.full((ny, nx), FAR, dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 > R * R or abs(dy) >= ny or abs(dx) >= nx:
                continue
            # cell (y, x) sees the seed at (y + dy, x + dx)
            ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
            xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
            view = out[yd, xd]
            np.minimum(view, np.where(seeds[ys, xs], d2, FAR), out=view)
    return out


def d2_edt(seeds, R):
    """the same from scipy's feature transform: the nearest seed's indices, the distance recomputed in integers"""
    from scipy import ndimage
    ny, nx = seeds.shape
    if not seeds.any():
        return np.full((ny, nx), FAR, dtype=np.int64)
    iy, ix = ndimage.distance_transform_edt(~seeds, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:ny, 0:nx]
    d2 = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
    return np.where(d2 <= R * R, d2, FAR)


def write_rule(old, cost, inflate_unknown):
    """InflationLayer::updateCosts' store for arrays of old values and new costs"""
    takes = (old == UNKNOWN) & ((cost > 0) if inflate_unknown else (cost >= INSCRIBED))
    return np.where(takes, cost, np.maximum(old, cost)).astype(np.uint8)


def inflate_exact(cells, params, res=RES, window=None, inflate_unknown=False, method="auto"):
    """(inflated copy of cells [ny][nx], n_seeds, n_changed) for window = (x0, y0, sx, sy), None = the whole map"""
    cells = np.asarray(cells, dtype=np.uint8)
    ny, nx = cells.shape
    x0, y0, sx, sy = (0, 0, nx, ny) if window is None else window
    R, table = cost_table(params, res)
    out = cells.copy()
    if sx == 0 or sy == 0 or R == 0:
        return out, 0, 0
    gx0, gy0, gx1, gy1 = max(0, x0 - R), max(0, y0 - R), min(nx, x0 + sx + R), min(ny, y0 + sy + R)
    seeds = np.zeros((ny, nx), dtype=bool)
    seeds[gy0:gy1, gx0:gx1] = cells[gy0:gy1, gx0:gx1] == LETHAL
    if method == "auto":
        method = "brute" if R <= 20 else "edt"
    d2 = (d2_brute if method == "brute" else d2_edt)(seeds, R)
    win = (slice(y0, y0 + sy), slice(x0, x0 + sx))
    d2w, old = d2[win], cells[win]
    reached = d2w <= R * R
    cost = table[np.where(reached, d2w, 0)]
    out[win] = np.where(reached, write_rule(old, cost, inflate_unknown), old)
    return out, int(seeds.sum()), int((out != cells).sum())


def inflate_brushfire(cells, params, res=RES, inflate_unknown=False):
    """Humble's InflationLayer::updateCosts over the whole map; returns the inflated copy"""
    cells = np.asarray(cells, dtype=np.uint8)
    ny, nx = cells.shape
    R, table = cost_table(params, res)
    out = cells.copy()
    if R == 0:
        return out
    master = out.reshape(-1)
    seen = np.zeros(ny * nx, dtype=bool)
    bins = [[] for _ in range(R * R + 1)]               # inflation_cells_: one bin per distinct distance, nearest first
    for j in range(ny):
        for i in range(nx):
            if cells[j, i] == LETHAL:
                bins[0].append((j * nx + i, i, j, i, j))

    def enqueue(index, mx, my, sx_, sy_):
        if seen[index]:
            return
        d2 = (mx - sx_) ** 2 + (my - sy_) ** 2
        if d2 > R * R:                                  # distanceLookup(...) > cell_inflation_radius_
            return
        bins[d2].append((index, mx, my, sx_, sy_))

    for d2_bin in bins:
        k = 0
        while k < len(d2_bin):                          # (a bin may grow while it is walked)
            index, mx, my, sx_, sy_ = d2_bin[k]
            k += 1
            if seen[index]:
                continue
            seen[index] = True
            cost = int(table[(mx - sx_) ** 2 + (my - sy_) ** 2])
            old = int(master[index])
            if old == UNKNOWN and ((cost > 0) if inflate_unknown else (cost >= INSCRIBED)):
                master[index] = cost
            else:
                master[index] = max(old, cost)
            if mx > 0:
                enqueue(index - 1, mx - 1, my, sx_, sy_)
            if my > 0:
                enqueue(index - nx, mx, my - 1, sx_, sy_)
            if mx < nx - 1:
                enqueue(index + 1, mx + 1, my, sx_, sy_)
            if my < ny - 1:
                enqueue(index + nx, mx, my + 1, sx_, sy_)
    return out


def grid(seed, ny, nx):
    """a costmap with a known interior, lethal blocks, blocks of 253 and 200, unknown patches (some of them against lethal
    cells) and one long wall"""
    rng = np.random.default_rng(seed)
    cells = np.full((ny, nx), UNKNOWN, np.uint8)
    cells[6:ny - 6, 6:nx - 6] = 0
    for k in range(7):
        y, x = int(rng.integers(8, ny - 16)), int(rng.integers(8, nx - 16))
        cells[y:y + int(rng.integers(2, 7)), x:x + int(rng.integers(2, 9))] = (254, 253, 200, 254, 254, 253, 254)[k]
    wy = int(rng.integers(ny // 3, 2 * ny // 3))
    cells[wy:wy + 2, 10:nx - 14] = LETHAL                                  # the long wall, with a door
    cells[wy:wy + 2, nx // 2:nx // 2 + 5] = 0
    for _ in range(5):
        y, x = int(rng.integers(8, ny - 16)), int(rng.integers(8, nx - 16))
        cells[y:y + int(rng.integers(3, 10)), x:x + int(rng.integers(3, 10))] = UNKNOWN
    cells[wy + 2:wy + 6, 20:30] = UNKNOWN                                  # unknown against the wall
    return cells


def single_seed(ny, nx):
    cells = np.zeros((ny, nx), np.uint8)
    cells[ny // 2 + 3, nx // 3] = LETHAL
    return cells


def single_wall(ny, nx):
    cells = np.zeros((ny, nx), np.uint8)
    cells[ny // 2, 7:nx - 9] = LETHAL
    return cells


def no_seed(ny, nx):
    cells = grid(99, ny, nx)
    cells[cells == LETHAL] = 252
    return cells
