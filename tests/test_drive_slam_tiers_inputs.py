"""The inputs of tests/drive_slam_tiers.py against the CPU oracle alone: every precondition tests/test_gpu_drive_slam_tiers.py relies
on, so that an input which drifts out of its regime fails here and not on the GPU machine.  No GPU.

Per-slab occupied voxels, that holes were hit, that the last x plane of a cut-down box was hit, that occlusion removes some voxels
and not all, that no (pose, landmark) pair is borderline, the threshold's clearance."""
import numpy as np
import pytest

import drive_ref as DR
import drive_slam_ref as DS
import drive_slam_tiers as T
import landmark_sense_ref as LR


def _range(f):
    return int(f["slabs"].min()), int(f["slabs"].max())


@pytest.mark.parametrize("name", sorted(T.INPUTS))
def test_no_pair_is_borderline_and_the_census_counts_what_the_oracle_counts(oracle, ref_table, name):
    inp = T.inputs(oracle, name)
    assert not LR.borderline(oracle, inp["poses"], inp["cloud"], [inp["fim"]]).any()
    if name.startswith("crowd_") and name.endswith("_beside"):
        return                                                           # (the same ball as load_4000 and the crowd of crowd_k)
    box = name.split("_")[0] if name.split("_")[0] in T.BOXES else "generated"
    f = T.facts(oracle, ref_table, name, box)
    np.testing.assert_array_equal([len(c) for c in f["census"]], f["want"]["n_voxels"])
    np.testing.assert_array_equal(f["slabs"].sum(axis=1), f["want"]["n_voxels"])


def test_tier_1_under_load(oracle, ref_table):
    """three loads of the hash table, none over its 2 048 slots; the heaviest slab of the largest holds at least 1 500"""
    ranges = {}
    for name in ("load_4000", "load_24000", "load_29000"):
        f = T.facts(oracle, ref_table, name)
        ranges[name] = _range(f)
        assert f["slabs"].max() <= T.SLOTS and f["n_over"] == 0, (name, f["slabs"])
    print("voxels per slab:", ranges)
    assert ranges["load_4000"][1] < 400 and 1200 < ranges["load_24000"][0] and ranges["load_29000"][1] >= 1500


def test_mixed_tiers_in_one_pose(oracle, ref_table):
    """slab 3 alone cannot fit its table, at both stations; no other slab is more than half full"""
    for name in ("mixed", "mixed_crowd"):
        f = T.facts(oracle, ref_table, name)
        print(name, "voxels per slab:", f["slabs"].tolist())
        assert (f["slabs"][:, 3] > T.SLOTS).all() and (np.delete(f["slabs"], 3, axis=1) <= 1024).all()
        assert (f["n_over"], f["n_loaded"]) == (2, 16)
    # the crowded voxel of mixed_crowd lies in the slab that falls back, beyond the factor table
    cen = T.facts(oracle, ref_table, "mixed_crowd")["census"][0]
    big = [k for k, n in cen.items() if n >= 500]
    assert len(big) == 1 and big[0][0] & 7 == 3


def test_the_existing_overflow_input_is_over_in_every_slab(oracle, ref_table):
    f = T.facts(oracle, ref_table, "overflow")
    assert (f["slabs"] > T.SLOTS).all() and f["want"]["n_voxels"].min() > 20000


@pytest.mark.parametrize("name", ["load_29000", "mixed", "overflow"])
def test_holes_were_hit(oracle, ref_table, name):
    full, holed = T.facts(oracle, ref_table, name), T.facts(oracle, ref_table, name, "holes")
    tab, rec, dims = T.table(oracle, ref_table, "holes")
    assert dims == T.table(oracle, ref_table, "generated")[2]            # the box is what it was
    assert 0.68 * ref_table.records.shape[0] < rec.shape[0] < 0.72 * ref_table.records.shape[0]
    print(name, "voxels:", full["want"]["n_voxels"], "with holes:", holed["want"]["n_voxels"], "per slab:", _range(holed))
    assert (holed["want"]["n_voxels"] < 0.8 * full["want"]["n_voxels"]).all() and (holed["want"]["n_voxels"] > 0).all()
    np.testing.assert_array_equal(holed["want"]["n_visible"], full["want"]["n_visible"])
    # the tiers the holed table leaves: tier 1 alone, one slab over, every slab over
    assert {"load_29000": holed["n_over"] == 0, "mixed": (holed["slabs"][:, 3] > T.SLOTS).all() and holed["n_over"] == 2,
            "overflow": (holed["slabs"] > T.SLOTS).all()}[name]


@pytest.mark.parametrize("box, dims, cells", [("tx5", (0, 5, 100, 100), 10000), ("tx64", (0, 64, 100, 100), 80000), ("short", (0, 16, 40, 40), 3200)])
def test_other_lattice_boxes(oracle, ref_table, box, dims, cells):
    """the box, its slab_cells, a ball that stays in tier 1 and a block that overflows; every pose counts a voxel of the last x plane"""
    assert T.table(oracle, ref_table, box)[2] == dims
    jx0, tx, ty, tz = dims
    assert (tx + 7) // 8 * ty * tz == cells
    assert {"tx5": tx < 8, "tx64": tx % 8 == 0, "short": cells < 4096 and cells % 4096 != 0}[box]
    small, large = T.facts(oracle, ref_table, f"{box}_ball", box), T.facts(oracle, ref_table, f"{box}_block", box)
    print(box, "ball per slab:", small["slabs"].tolist(), "block per slab:", large["slabs"].tolist())
    assert small["n_over"] == 0 and small["slabs"].max() < 1024
    owning = min(tx, 8)
    assert (large["slabs"][:, :owning] > T.SLOTS).all() and (large["slabs"][:, owning:] == 0).all() and (small["slabs"][:, owning:] == 0).all()
    for f in (small, large):
        for cen in f["census"]:
            assert max(k[0] for k in cen) - jx0 == tx - 1
        # landmarks outside the box were there to be refused
        assert (f["want"]["n_visible"] > sum(cen.values())).all()


def test_crowded_voxels(oracle, ref_table):
    """one voxel at the first station; 336 landmarks and 500 give the same information: the series is 0 from rank 337 on"""
    info = {}
    for k in T.CROWDS:
        f = T.facts(oracle, ref_table, f"crowd_{k}")
        assert f["want"]["n_voxels"][0] == 1 and list(f["census"][0].values()) == [k]
        info[k] = f["want"]["info_f64"][0]
    print("information:", info)
    assert info[1] < info[2] < info[336] == info[337] == info[351] == info[352] == info[500]
    assert info[500] == pytest.approx(T.CROWD_INFORMATION, rel=1e-8)
    assert sum(oracle.factor_from_num(j) for j in range(337, 600)) == 0.0 and T.FACTOR_N - 1 > 337
    beside = T.facts(oracle, ref_table, "crowd_500_beside")
    assert max(beside["census"][0].values()) == 500 and beside["n_over"] == 0


@pytest.mark.parametrize("name", ["mixed_rim", "overflow_rim"])
def test_discovery_fills_the_tiers(oracle, ref_table, name):
    """nothing known: the second station discovers landmarks in the step in which it counts them, and the tiers are those of the
    known cloud"""
    d = T.discovery(oracle, name)
    f = T.facts(oracle, ref_table, name, flags=d["flags"])
    fresh = d["flags"][1] & ~d["flags"][0]
    print(name, "discovered per step:", d["flags"].sum(axis=1), "voxels per slab:", f["slabs"].tolist())
    assert fresh.sum() > 50 and d["n_new"] == d["n_discovered"] == d["flags"][1].sum()
    np.testing.assert_array_equal(f["want"]["n_visible"], d["n_in_view"])
    over = f["slabs"] > T.SLOTS
    assert over[:, 3].all() and over.sum() == (2 if name == "mixed_rim" else 16)
    # station 1 counts freshly discovered landmarks in a slab that falls back: voxels that hold nothing else
    inp = T.inputs(oracle, name)
    new = T.slabs(T.census(oracle, ref_table, inp["cloud"][fresh], inp["poses"][1], inp["fim"]), 0)
    without = oracle.pose_information(ref_table, inp["cloud"][d["flags"][0]], inp["poses"][1:], *inp["fim"])
    assert new[3] > 0 and without["n_voxels"][0] < f["want"]["n_voxels"][1]


def test_occlusion_removes_some_voxels_but_not_all(oracle, ref_table):
    d = T.discovery(oracle, "mixed_rim")
    o = T.occluded_facts(oracle, ref_table, "mixed_rim", d["flags"])
    print("voxels:", o["open"], "occluded:", o["want"]["n_voxels"], "per slab:", o["slabs"].tolist())
    assert (o["want"]["n_voxels"] < o["open"]).all() and (o["want"]["n_voxels"] > 0).all()
    np.testing.assert_array_equal(o["slabs"].sum(axis=1), o["want"]["n_voxels"])
    assert (o["slabs"][:, 3] > T.SLOTS).all()                            # the line of sight runs inside tier 2


def test_the_fleet(oracle, ref_table):
    """64 ragged station lists, no borderline pair, a threshold with clearance, three statuses, stops at three different steps"""
    case = T.fleet(oracle)
    assert [p.shape[0] for p in case["poses"]] == [1 + r % 6 for r in range(64)]
    assert not LR.borderline(oracle, np.concatenate(case["poses"]), case["cloud"], [(2.0, 1.0), DS.FIM]).any()
    free = T.fleet_ref(oracle, ref_table, case, gate=False)
    r, hi, lo = case["between"]
    thr = DS.threshold_between(free["information"], free["information"][r][lo], free["information"][r][hi])
    got = T.fleet_ref(oracle, ref_table, case, threshold=thr)
    print("threshold", thr, "status", got["status"].tolist(), "reached", got["reached"].tolist())
    assert {DR.ARRIVED, DR.MAPPED, DS.UNSAFE} <= set(got["status"].tolist())
    assert len(set(got["reached"][got["status"] == DS.UNSAFE].tolist())) >= 3
    assert (got["status"][1::4] == DR.MAPPED).all() and (got["reached"][1::4] == 0).all()


def test_equality_at_the_gate(oracle, ref_table):
    """all visible landmarks in one voxel at both stations: the information is one product, table value x series"""
    f = T.facts(oracle, ref_table, "one_voxel")
    assert list(f["want"]["n_voxels"]) == [1, 1] and list(f["want"]["n_visible"]) == [3, 3]
    free = T.one_voxel_ref(oracle, ref_table, gate=False)
    t = np.float32(free["information"][0][1])
    assert t > 0.0 and free["information"][0][1] == f["want"]["info_f64"][1]
    assert list(T.one_voxel_ref(oracle, ref_table, threshold=float(t))["status"]) == [DS.UNSAFE]
    assert list(T.one_voxel_ref(oracle, ref_table, threshold=float(np.nextafter(t, np.float32(-np.inf), dtype=np.float32)))["status"]) == [DR.ARRIVED]
