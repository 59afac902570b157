"""The inflation layer's rule on the CPU: the cost table at the reference's parameters, the two forms of the exact
transform against each other, the exact transform against Humble's ordered brushfire (never below it, equal where one seed or one
straight wall leaves the brushfire no choice), windows, idempotence, the write rule on unknown cells — and the entry points'
declarations, exports, bindings and NULL-context refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

import inflation_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fitslam_frontier.h")

R12, R20 = (0.60, 0.05, 0.6), (1.0, 0.05, 0.6)
TWO_COSTS = (0.3, 0.6, 0.6)                                  # inscribed beyond the radius: only 254 and 253 occur
MAPS = {"grid64": lambda: I.grid(1, 64, 64), "grid96": lambda: I.grid(2, 96, 96), "grid_72x80": lambda: I.grid(3, 72, 80),
        "seed": lambda: I.single_seed(64, 64), "wall": lambda: I.single_wall(64, 64), "none": lambda: I.no_seed(64, 64)}


@pytest.fixture(scope="module")
def fires():
    """{(map, params): (exact, brushfire)}, computed once"""
    out = {}
    for name, make in MAPS.items():
        cells = make()
        for params in (R12, R20, TWO_COSTS):
            out[name, params] = (cells, I.inflate_exact(cells, params)[0], I.inflate_brushfire(cells, params))
    return out


def test_table_at_the_reference_parameters():
    R, table = I.cost_table(I.GLOBAL, 0.05)
    assert R == 100 and table.shape == (10001,)
    # 252 * exp(-0.6 * (0.05 * sqrt(2) - 0.05)) = 248.8..., 252 * exp(-0.6 * 4.95) = 12.9...
    assert [int(table[d2]) for d2 in (0, 1, 2, 10000)] == [254, 253, 248, 12]
    assert (np.diff(table.astype(int)) <= 0).all() and table[1:].max() == 253
    assert I.cost_table(I.LOCAL, 0.05)[0] == 12 and I.cost_table(I.LETHAL_LAYER, 0.05)[0] == 6
    R, table = I.cost_table(TWO_COSTS, 0.05)
    assert R == 6 and set(table.tolist()) == {254, 253}
    assert I.cost_table((0.0, 0.05, 0.6), 0.05)[0] == 0
    assert I.cost_table((0.6, 0.05, 0.0), 0.05)[1][2:].tolist() == [252] * 143          # no decay


@pytest.mark.parametrize("name", list(MAPS))
def test_brute_force_and_scipy_agree(name):
    cells = MAPS[name]()
    seeds = cells == I.LETHAL
    for R in (1, 6, 12, 20):
        np.testing.assert_array_equal(I.d2_brute(seeds, R), I.d2_edt(seeds, R))
    for params in (R12, I.LETHAL_LAYER):
        a, b = I.inflate_exact(cells, params, method="brute"), I.inflate_exact(cells, params, method="edt")
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1:] == b[1:]
    win = (5, 9, 37, 21)
    a, b = I.inflate_exact(cells, R20, window=win, method="brute"), I.inflate_exact(cells, R20, window=win, method="edt")
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:]


def test_exact_is_never_below_the_brushfire(fires):
    differ, total = 0, 0
    for (name, params), (cells, exact, fire) in fires.items():
        assert (exact >= fire).all(), (name, params)
        n = int((exact != fire).sum())
        if params == TWO_COSTS:
            assert n == 0, name
        else:
            differ, total = differ + n, total + exact.size
    print(f"exact != brushfire on {differ} of {total} cells (R = 12 and 20)")              # a record, not a gate


@pytest.mark.parametrize("name", ["seed", "wall", "none"])
def test_exact_equals_the_brushfire_where_it_has_no_choice(fires, name):
    for params in (R12, R20, TWO_COSTS):
        cells, exact, fire = fires[name, params]
        np.testing.assert_array_equal(exact, fire)
        if name == "none":
            np.testing.assert_array_equal(exact, cells)
        else:
            assert (exact != cells).sum() > 100


@pytest.mark.parametrize("window", [(0, 0, 96, 96), (11, 7, 37, 21), (40, 40, 1, 1), (0, 75, 30, 21), (70, 3, 26, 10), (5, 5, 0, 9)])
def test_a_window_equals_the_whole_map_inside_and_the_input_outside(window):
    cells = I.grid(2, 96, 96)
    x0, y0, sx, sy = window
    for params in (R12, I.GLOBAL):
        whole = I.inflate_exact(cells, params)[0]
        got, n_seeds, n_changed = I.inflate_exact(cells, params, window=window)
        want = cells.copy()
        want[y0:y0 + sy, x0:x0 + sx] = whole[y0:y0 + sy, x0:x0 + sx]
        np.testing.assert_array_equal(got, want)
        assert n_changed == int((want != cells).sum())
        R = I.cell_radius(params)
        grown = cells[max(0, y0 - R):y0 + sy + R, max(0, x0 - R):x0 + sx + R]
        assert n_seeds == (int((grown == 254).sum()) if sx and sy else 0)


def test_idempotent_and_composes_by_max(fires):
    for (name, params), (cells, exact, _) in fires.items():
        again, n_seeds, n_changed = I.inflate_exact(exact, params)
        np.testing.assert_array_equal(again, exact)
        assert n_changed == 0 and n_seeds == int((cells == 254).sum())
    cells = I.grid(2, 96, 96)
    a, b = I.inflate_exact(cells, R20)[0], I.inflate_exact(cells, I.LETHAL_LAYER)[0]
    both = I.inflate_exact(a, I.LETHAL_LAYER)[0]
    known = cells != 255
    np.testing.assert_array_equal(both[known], np.maximum(a, b)[known])
    assert (both[cells == 253] == 253).all() and (both[cells == 254] == 254).all()


def test_the_two_branches_on_unknown_cells():
    cells = np.full((40, 40), 255, np.uint8)
    cells[20, 20] = 254
    R, table = I.cost_table(R12)
    off = I.inflate_exact(cells, R12)[0]
    on = I.inflate_exact(cells, R12, inflate_unknown=True)[0]
    yy, xx = np.mgrid[0:40, 0:40]
    d2 = (yy - 20) ** 2 + (xx - 20) ** 2
    cost = np.where(d2 <= R * R, table[np.minimum(d2, R * R)], 0)
    np.testing.assert_array_equal(off, np.where(cost >= 253, cost, 255))
    np.testing.assert_array_equal(on, np.where(cost > 0, cost, 255))
    assert (off == 253).sum() == 4 and (on < 253).sum() > 300 and on.min() > 0
    # a known cell next to it takes max(old, cost) in both
    cells[20, 22] = 200
    cells[20, 25] = 250
    for flag in (False, True):
        got = I.inflate_exact(cells, R12, inflate_unknown=flag)[0]
        assert got[20, 22] == max(200, int(table[4])) == int(table[4]) and got[20, 25] == 250 > table[25]


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: args.count(",") + 1 for name, args in re.findall(r"\bint\s+(fs_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}, text


def test_declared_exported_bound_and_refused_without_a_context(fs):
    decl, text = _declarations()
    L = fs.load_library()
    for name, n_args in (("fs_inflate", 8), ("fs_inflation_costs", 4), ("fs_multi_inflate", 8)):
        assert decl[name] == n_args and name in fs.capi.EXPORTED_SYMBOLS
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == n_args
    m = re.search(r"#define\s+FS_INFLATE_MAX_CELLS\s+(\d+)", text)
    assert m and int(m.group(1)) == fs.capi.FS_INFLATE_MAX_CELLS == 512
    assert re.search(r"double inflation_radius, inscribed_radius, cost_scaling_factor;.*\n\s*int32_t inflate_unknown, reserved;", text)
    assert callable(fs.FrontierScorer.inflate) and callable(fs.FrontierScorer.inflation_costs) and callable(fs.MultiScorer.inflate)
    blob = open(fs._build.LIB, "rb").read()
    assert b"fs_inflate_rows_kernel" in blob and b"fs_inflate_cols_kernel" in blob
    import ctypes as C
    p = fs.capi.InflationParamsC(5.0, 0.05, 0.6, 0, 0)
    r = C.c_int32()
    assert L.fs_inflate(None, C.byref(p), 0, 0, 1, 1, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_inflate(None, None, 0, 0, 1, 1, None, None) == fs.capi.FS_E_INVALID
    assert L.fs_inflation_costs(None, C.byref(p), C.byref(r), None) == fs.capi.FS_E_INVALID
    assert L.fs_multi_inflate(None, C.byref(p), 0, 0, 1, 1, None, None) == fs.capi.FS_E_INVALID
