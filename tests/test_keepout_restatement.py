"""The host side of the keep-out layer (fit-slam_amd/csrc/fs_keepout.h, DESIGN.md 4.19: the end cells of a zone's rays and the
walk the kernel runs) against the line-cited restatement of the reference (tests/keepout_ref.py) — end cells and walked index
lists, bit for bit.  The header's functions are compiled by g++ into a small shared object (tests/keepout_ref/keepout_host.cpp).
No GPU."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import keepout_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "keepout_ref", "keepout_host.cpp")
INC = os.path.join(ROOT, "fit-slam_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="keepout_host_"), "libkeepout_host.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", INC, "-o", out, SRC], check=True)
        L = C.CDLL(out)
        L.kohost_zone_rays.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double, C.c_void_p]
        L.kohost_walk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
        L.kohost_walk.restype = C.c_longlong
        _lib = L
    return _lib


def host_zone(zone, geom):
    """(rays [n][4], walked indices) as the library's host code computes them"""
    L = lib()
    rays = np.zeros((360, 4), np.int32)
    n = L.kohost_zone_rays(int(zone[0]), zone[1], zone[2], zone[3], zone[4], geom[0], geom[1], geom[2], geom[3], geom[4], rays.ctypes.data)
    assert n >= 0
    idx = np.zeros(360 * (geom[0] + geom[1]) + 8, np.int64)
    m = L.kohost_walk(rays.ctypes.data, n, geom[0], idx.ctypes.data, idx.size)
    assert m <= idx.size
    return rays[:n], idx[:m]


def check(zone, geom):
    rays, idx = host_zone(zone, geom)
    want = K.zone_rays(zone, geom)
    if want is None:
        assert rays.shape[0] == 0 and idx.size == 0
        return 0
    (ax, ay), ends = want
    assert rays.shape[0] == len(ends)
    assert np.array_equal(rays, np.array([[ax, ay, ex, ey] for ex, ey in ends], dtype=np.int32)), (zone, geom)
    assert idx.tolist() == K.zone_indices(zone, geom), (zone, geom)
    return idx.size


ANCHOR_GEOM = (96, 96, 0.0, 0.0, 0.05)
ANCHOR_ZONE = (K.FOV, 0.52, 2.42, 0.0, 3.5)


def test_anchor_by_hand():
    """96 x 96, origin (0, 0), resolution 0.05, apex world (0.52, 2.42), yaw 0, height 3.5: apex cell (10, 48), h = 70, base end
    points (80, 76) and (80, 19); every ray has dx = 70 >= dy, so 71 cells each = 1 420 pushed indices."""
    rays, idx = host_zone(ANCHOR_ZONE, ANCHOR_GEOM)
    assert rays.shape == (20, 4)
    assert np.all(rays[:, 0] == 10) and np.all(rays[:, 1] == 48)
    assert tuple(rays[0, 2:]) == (80, 76) and tuple(rays[-1, 2:]) == (80, 19)
    assert np.all(rays[:, 2] == 80)
    assert idx.size == 20 * 71 == 1420
    assert check(ANCHOR_ZONE, ANCHOR_GEOM) == 1420
    distinct = np.unique(idx).size
    assert distinct == np.unique(K.zone_indices(ANCHOR_ZONE, ANCHOR_GEOM)).size
    assert distinct == 1188
    # a fan of lines, not a filled triangle: cells strictly inside the triangle stay unmarked
    mask, counts = K.zone_masks([ANCHOR_ZONE], ANCHOR_GEOM)
    assert counts[0] == distinct and mask.sum() == distinct
    assert mask[48, 10] == 1 and distinct < 70 * 57 // 2                      # (the triangle's area in cells)


def test_walk_visits_both_ends_and_steps_diagonally():
    L = lib()
    idx = np.zeros(64, np.int64)
    rays = np.array([[2, 3, 6, 5]], np.int32)
    n = L.kohost_walk(rays.ctypes.data, 1, 10, idx.ctypes.data, idx.size)
    got = [(int(i) % 10, int(i) // 10) for i in idx[:n]]
    assert got[0] == (2, 3) and got[-1] == (6, 5) and n == 5                  # max(dx, dy) + 1 cells: diagonal steps, unlike bresenham2D
    assert idx[:n].tolist() == K.ray_trace(10, 10, 2, 3, 6, 5)
    rays = np.array([[4, 4, 4, 4]], np.int32)                                 # a ray of one cell
    assert L.kohost_walk(rays.ctypes.data, 1, 10, idx.ctypes.data, idx.size) == 1 and idx[0] == 44


def test_every_end_point_clamps_on_a_small_map():
    geom = (16, 16, 0.0, 0.0, 0.05)
    for yaw in (0.0, 0.7, math.pi / 2, 2.3, math.pi, -2.0, -math.pi / 2):
        zone = (K.FOV, 0.4, 0.4, yaw, 3.5)
        rays, _ = host_zone(zone, geom)
        assert rays.shape[0] == 20
        assert np.all((rays[:, 2] == 0) | (rays[:, 2] == 15) | (rays[:, 3] == 0) | (rays[:, 3] == 15))
        check(zone, geom)
        check((K.DISC, 0.4, 0.4, 0.0, 1.7), geom)


def test_apex_just_below_the_origin_marks_nothing():
    geom = (96, 96, -1.0, -1.0, 0.05)
    for wx, wy in ((np.nextafter(-1.0, -2.0), 0.0), (0.0, np.nextafter(-1.0, -2.0)), (-1.0 + 96 * 0.05, 0.0), (0.0, 5.0)):
        rays, idx = host_zone((K.FOV, float(wx), float(wy), 0.3, 3.5), geom)
        assert rays.shape[0] == 0 and idx.size == 0
        assert K.zone_rays((K.FOV, float(wx), float(wy), 0.3, 3.5), geom) is None
    assert check((K.FOV, -1.0, -1.0, 0.3, 3.5), geom) > 0                     # the origin itself is cell (0, 0)


def test_height_truncates_at_resolution_003():
    geom = (160, 160, 0.0, 0.0, 0.03)
    zone = (K.FOV, 0.6, 2.4, 0.0, 3.5)                                        # 3.5 / 0.03 = 116.67 -> 116
    rays, _ = host_zone(zone, geom)
    assert int(3.5 / 0.03) == 116
    assert tuple(rays[0, :2]) == (20, 80)
    assert np.all(rays[:, 2] == 20 + 116)
    check(zone, geom)


def test_sizes_the_reference_cannot_convert_are_refused():
    L = lib()
    rays = np.zeros((360, 4), np.int32)
    for size in (float("nan"), float("inf"), -1.0, 0.05 * 2.0 ** 31):
        assert L.kohost_zone_rays(K.FOV, 1.0, 1.0, 0.0, size, 96, 96, 0.0, 0.0, 0.05, rays.ctypes.data) == -1
    assert L.kohost_zone_rays(K.FOV, 1.0, 1.0, 0.0, 0.05 * (2.0 ** 31 - 1024), 96, 96, 0.0, 0.0, 0.05, rays.ctypes.data) == 20


def test_random_zones():
    """2 400 seeded zones: maps 16 ... 160 cells a side, resolutions 0.03 / 0.05 / 0.1, origins negative and positive, the apex
    anywhere including a margin off the map, yaw in [-2 pi, 2 pi] with exact multiples of pi / 2 among them."""
    rng = np.random.default_rng(20240607)
    seen = dict(zones=0, off_map=0, fov=0, disc=0, clamped=0, quarter=0, pushed=0)
    for _ in range(2400):
        nx, ny = int(rng.integers(16, 161)), int(rng.integers(16, 161))
        res = float(rng.choice([0.03, 0.05, 0.1]))
        ox, oy = float(rng.uniform(-6.0, 3.0)), float(rng.uniform(-6.0, 3.0))
        geom = (nx, ny, ox, oy, res)
        margin = 0.4
        wx = float(rng.uniform(ox - margin, ox + nx * res + margin))
        wy = float(rng.uniform(oy - margin, oy + ny * res + margin))
        if rng.random() < 0.2:
            yaw = float(rng.integers(-4, 5)) * (math.pi / 2)
            seen["quarter"] += 1
        else:
            yaw = float(rng.uniform(-2 * math.pi, 2 * math.pi))
        if rng.random() < 0.12:
            zone = (K.DISC, wx, wy, 0.0, float(rng.choice([0.5, 1.0, 1.7])))
            seen["disc"] += 1
        else:
            zone = (K.FOV, wx, wy, yaw, float(rng.choice([3.5, 3.5, 1.0, 0.04, 6.0])))
            seen["fov"] += 1
        pushed = check(zone, geom)
        seen["zones"] += 1
        seen["pushed"] += pushed
        if pushed == 0:
            seen["off_map"] += 1
        else:
            ends = np.array(K.zone_rays(zone, geom)[1])
            if np.any((ends[:, 0] == 0) | (ends[:, 0] == nx - 1) | (ends[:, 1] == 0) | (ends[:, 1] == ny - 1)):
                seen["clamped"] += 1
    assert seen["zones"] >= 2000 and seen["off_map"] >= 50 and seen["disc"] >= 100 and seen["clamped"] >= 200 and seen["quarter"] >= 200, seen


def test_the_disc_has_gaps():
    """getPointsInSemiCircle marks 360 lines, not a disc: at 34 cells radius cells inside the circle stay unmarked."""
    geom = (96, 96, 0.0, 0.0, 0.05)
    zone = (K.DISC, 2.4, 2.4, 0.0, 1.7)
    check(zone, geom)
    mask, counts = K.zone_masks([zone], geom)
    yy, xx = np.mgrid[0:96, 0:96]
    r = int(1.7 / 0.05)
    assert r in (33, 34)
    inside = (xx - 48) ** 2 + (yy - 48) ** 2 <= (r - 2) ** 2
    assert np.count_nonzero(inside & (mask == 0)) > 0
    assert counts[0] == mask.sum()
