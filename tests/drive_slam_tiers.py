"""Inputs that hold fs_drive_slam's information kernel (fit-slam_amd/csrc/fs_drive_slam.hip) at loaded hash tables and
at table edges.  A helper, not a test module: tests/test_drive_slam_tiers_inputs.py checks every input against the CPU oracle alone,
tests/test_gpu_drive_slam_tiers.py runs them on the device.

The kernel splits a pose's voxels over eight slab workgroups by `ix & 7`, ix the voxel's x index inside the table's box, and counts
a slab's landmarks per voxel in an LDS hash table of 2 048 slots (tier 1; a lane gives up after 128 probes) or, when that fails, in
direct-indexed passes over ranges of 4 096 slab-local voxel indices (tier 2).  What decides the tier is therefore the number of
occupied voxels PER SLAB, which `census` / `slabs` work out here from oracle.world_to_camera, oracle.voxel_coordinate and the oracle
table's own find — nothing the library returns.

Clouds are built in the camera frame of the first station (x ahead) and turned into the world by the station's yaw.  Every cloud goes
through landmark_sense_ref.drop_borderline for its poses and volumes before anybody sees it."""
import numpy as np

import drive_ref as DR
import drive_slam_ref as DS
import landmark_sense_ref as LR
import occlusion_ref as OR
import sense_ref as SR
import test_drive_restatement as TR
import test_gpu_explore_episode as EP

STEP = float(np.float32(0.3))                                            # the voxel lattice (step_max as the reference widens it)
SLABS, SLOTS, MAX_PROBE, FACTOR_N = 8, 2048, 128, 352                    # FS_GATE_SLABS, FS_GATE_SLOTS, FS_GATE_MAX_PROBE, FS_FACTOR_N
FIM = (14.0, 4.0)                                                        # the volume of isPoseSafe's own request: 14 m, cone off
CENTRE = np.array(DR.cell_centre(20, 20, EP.ORIGIN, EP.RES))
EAST = np.array(DR.cell_centre(25, 20, EP.ORIGIN, EP.RES))               # the second station of the yaw-0.3 inputs
NORTH = np.array(DR.cell_centre(20, 25, EP.ORIGIN, EP.RES))              # ... of the yaw-0 inputs: camera x stays what it was
FAR = DR.cell_centre(90, 90, EP.ORIGIN, EP.RES)                          # a goal nobody maps
CROWDS = (1, 2, 336, 337, 351, 352, 500)
CROWD_INFORMATION = 4.49440763                                           # 336 or more landmarks in the voxel (3.0, 0, 0.3): 2.22002220 x 2.02448769
OCCLUSION = DS.OCCLUSION


def sensor(fim):
    """a landmark sensor with the FIM volume and no line of sight: whatever a pose scores it has discovered by then"""
    return dict(max_dist=fim[0], max_angle=fim[1], line_of_sight=0, min_views=1)


def to_world(cam, yaw, at=CENTRE):
    c, s = np.cos(yaw), np.sin(yaw)
    cam = np.asarray(cam, dtype=np.float64).reshape(-1, 3)
    return np.stack([at[0] + c * cam[:, 0] - s * cam[:, 1], at[1] + s * cam[:, 0] + c * cam[:, 1], at[2] + cam[:, 2]], 1).astype(np.float32)


def ball(n, seed=17, radius=14.0):
    """n landmarks uniform in a ball around CENTRE (tests/test_gpu_drive_slam.py's 60 000-landmark input is ball(60000))"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (CENTRE + v / np.linalg.norm(v, axis=1)[:, None] * (radius * rng.uniform(0.0, 1.0, size=(n, 1)) ** (1.0 / 3.0))).astype(np.float32)


def shell(n, seed=37, r0=14.0, r1=14.25):
    """n landmarks between r0 and r1 from CENTRE: out of the first station's reach, a part of them within the second's"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return (CENTRE + v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(r0, r1, size=(n, 1))).astype(np.float32)


def planes(n_per_plane, half, seed=23, slab=3, reach=13.0):
    """landmarks ON the camera-frame x planes ix = slab, slab + 8, .. (x = 0.3 ix, the middle of the voxel), y and z uniform in
    +-half: at yaw 0 they all fall to one slab"""
    rng = np.random.default_rng(seed)
    out = []
    for ix in range(slab, int(reach / STEP), SLABS):
        yz = rng.uniform(-half, half, size=(n_per_plane, 2))
        out.append(np.concatenate([np.full((n_per_plane, 1), ix * STEP), yz], axis=1))
    return to_world(np.concatenate(out), 0.0)


def block(n, lo, hi, yaw, seed=29):
    """n landmarks uniform in the camera-frame box lo .. hi [3]"""
    rng = np.random.default_rng(seed)
    return to_world(rng.uniform(lo, hi, size=(n, 3)), yaw)


def crowd(k, yaw, ix=10, seed=31):
    """k landmarks inside ONE voxel: +-0.1 m around the lattice point (0.3 ix, 0, 0.3) of the first station's camera frame"""
    rng = np.random.default_rng(seed)
    return to_world(np.array([ix * STEP, 0.0, STEP]) + rng.uniform(-0.1, 0.1, size=(k, 3)), yaw)


# ---- lookup tables: the generated one cut down by record selection

BOXES = {
    # name: (lattice index ranges kept (x, y, z; None = all), share of the records removed at random)
    "generated": ((None, None, None), 0.0),
    "holes": ((None, None, None), 0.3),
    "tx5": (((0, 4), None, None), 0.0),                                  # slabs 5..7 own nothing; 10 000 cells per slab: ranges 4096, 4096, 1808
    "tx64": (((0, 63), None, None), 0.0),                                # tx a multiple of 8: every slab owns 8 planes
    "short": (((0, 15), (-20, 19), (-20, 19)), 0.0),                     # 2 x 40 x 40 = 3 200 cells per slab: ONE range, shorter than 4 096
}
_TABLES = {}


def lattice(records):
    return np.round(np.asarray(records, dtype=np.float32)[:, :3].astype(np.float64) / STEP).astype(np.int64)


def records(ref_table, box):
    """the records [n][4] of a box of BOXES, cut out of the generated table's"""
    keep_ranges, holes = BOXES[box]
    rec = ref_table.records
    lat = lattice(rec)
    keep = np.ones(rec.shape[0], dtype=bool)
    for a, rng_a in enumerate(keep_ranges):
        if rng_a is not None:
            keep &= (lat[:, a] >= rng_a[0]) & (lat[:, a] <= rng_a[1])
    if holes > 0.0:
        lo, hi = lat[keep].min(axis=0), lat[keep].max(axis=0)
        corner = (lat == lo).all(axis=1) | (lat == hi).all(axis=1)      # (the box stays what it was)
        keep &= (np.random.default_rng(41).random(rec.shape[0]) >= holes) | corner
    return np.ascontiguousarray(rec[keep])


def table(oracle, ref_table, box):
    """(oracle Table, records or None for the generated table, (jx0, tx, ty, tz)), made once per box"""
    if box not in _TABLES:
        rec = None if box == "generated" else records(ref_table, box)
        lat = lattice(ref_table.records if rec is None else rec)
        ext = lat.max(axis=0) - lat.min(axis=0) + 1
        _TABLES[box] = (ref_table if rec is None else oracle.Table.from_records(rec), rec, (int(lat[:, 0].min()), int(ext[0]), int(ext[1]), int(ext[2])))
    return _TABLES[box]


# ---- the inputs

def _mixed():
    return np.concatenate([ball(12000), planes(900, 7.0)])


INPUTS = {
    # name: (cloud, yaw, second station, FIM volume)
    "load_4000": (lambda: ball(4000), 0.3, EAST, FIM),
    "load_24000": (lambda: ball(24000), 0.3, EAST, FIM),
    "load_29000": (lambda: ball(29000), 0.3, EAST, FIM),
    "overflow": (lambda: ball(60000), 0.3, EAST, FIM),                   # the existing test's input: all eight slabs over
    "mixed": (_mixed, 0.0, NORTH, FIM),
    "mixed_crowd": (lambda: np.concatenate([_mixed(), crowd(500, 0.0, ix=11)]), 0.0, NORTH, FIM),
    "mixed_rim": (lambda: np.concatenate([_mixed(), shell(3000)]), 0.0, NORTH, FIM),          # for discovery: something new at station 1
    "overflow_rim": (lambda: np.concatenate([ball(60000), shell(3000)]), 0.3, EAST, FIM),
    "tx5_ball": (lambda: ball(6000, radius=4.0), 0.3, EAST, FIM),
    "tx5_block": (lambda: block(27000, (-0.3, -10.0, -10.0), (1.5, 10.0, 10.0), 0.3), 0.3, EAST, FIM),
    "tx64_ball": (lambda: ball(6000, radius=20.0), 0.3, EAST, (20.0, 4.0)),
    "tx64_block": (lambda: block(36000, (-0.3, -3.3, -3.3), (19.4, 3.3, 3.3), 0.3), 0.3, EAST, (20.0, 4.0)),
    "short_ball": (lambda: ball(4000, radius=7.0), 0.3, EAST, FIM),
    "short_block": (lambda: block(46000, (-0.45, -6.6, -6.6), (4.95, 6.3, 6.3), 0.3), 0.3, EAST, FIM),
    "one_voxel": (lambda: crowd(3, 0.0), 0.0, NORTH, FIM),
}
for _k in CROWDS:
    INPUTS[f"crowd_{_k}"] = (lambda k=_k: crowd(k, 0.3), 0.3, EAST, FIM)
    INPUTS[f"crowd_{_k}_beside"] = (lambda k=_k: np.concatenate([ball(4000), crowd(k, 0.3)]), 0.3, EAST, FIM)
_INPUTS = {}


def inputs(oracle, name):
    """dict(cloud [m][3] float32 without borderline landmarks, poses [2][7], fim, sensor), made once per name (read-only)"""
    if name not in _INPUTS:
        make, yaw, second, fim = INPUTS[name]
        poses = DS.pose_rows([CENTRE, second], yaw)
        cloud = LR.drop_borderline(oracle, poses, make(), [fim])
        cloud.setflags(write=False)
        _INPUTS[name] = dict(cloud=cloud, poses=poses, fim=fim, sensor=sensor(fim))
    return _INPUTS[name]


# ---- what the oracle says about an input

def census(oracle, tab, cloud, pose7, fim, keep=None):
    """{lattice index (jx, jy, jz): landmarks} of the voxels the pose counts: the landmarks of `cloud` (those of the mask `keep`)
    the predicate accepts, their camera-frame points by oracle.world_to_camera, their voxels by oracle.voxel_coordinate, and only
    voxels the table `tab` knows"""
    lm = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
    vis, _ = LR.predicate(oracle, pose7, lm, fim[0], fim[1])
    if keep is not None:
        vis &= keep
    R, t = oracle.pose_to_rt(pose7)
    count, key_of = {}, {}
    for w in lm[vis]:
        p = oracle.world_to_camera(R, t, w)
        key, idx = oracle.voxel_coordinate(p[0], p[1], p[2])
        k = (int(idx[0]), int(idx[1]), int(idx[2]))
        if k not in count:
            count[k], key_of[k] = 0, key
        count[k] += 1
    return {k: n for k, n in count.items() if not np.isnan(tab.find(key_of[k]))}


def slabs(cen, jx0):
    """occupied voxels per slab [8]: slab ownership is (jx - jx0) & 7"""
    return np.bincount([(k[0] - jx0) & (SLABS - 1) for k in cen], minlength=SLABS)


_FACTS = {}


def facts(oracle, ref_table, name, box="generated", flags=None):
    """per station of the input under the box's table: dict(want = oracle.pose_information's columns stacked over the stations,
    census [2], slabs [2][8], n_over, n_loaded), made once.  flags: per station the mask of the landmarks discovered by then (None:
    all known)."""
    key = (name, box, None if flags is None else flags.tobytes())
    if key not in _FACTS:
        inp = inputs(oracle, name)
        tab, _, (jx0, _, _, _) = table(oracle, ref_table, box)
        rows, cens = [], []
        for k, p in enumerate(inp["poses"]):
            sub = inp["cloud"] if flags is None else inp["cloud"][flags[k]]
            rows.append(oracle.pose_information(tab, sub, p[None], inp["fim"][0], inp["fim"][1]))
            cens.append(census(oracle, tab, sub, p, inp["fim"]))
        want = {c: np.concatenate([r[c] for r in rows]) for c in ("info_f64", "n_voxels", "n_visible")}
        per = np.stack([slabs(c, jx0) for c in cens])
        _FACTS[key] = dict(want=want, census=cens, slabs=per, n_over=int((per > SLOTS).sum()), n_loaded=int((per >= MAX_PROBE).sum()))
    return _FACTS[key]


def discovery(oracle, name):
    """the landmark sensor's restatement over the input's two stations, nothing known before: dict(flags [2][m] after step k,
    n_in_view [2], n_new, n_discovered, world_index, views)"""
    inp = inputs(oracle, name)
    wc = LR.WorldCloud(oracle, inp["cloud"])
    flags, in_view = [], []
    for p in inp["poses"]:
        in_view.append(int(wc.sense(None, p[None], inp["sensor"])["n_in_view"][0]))
        flags.append(wc.flag.copy())
    return dict(flags=np.stack(flags), n_in_view=in_view, n_new=int(wc.flag.sum()), n_discovered=int(wc.flag.sum()),
                world_index=wc.world_index, views=wc.views.copy())


_GRIDS = {}


def staged_after(name, oracle):
    """the staged grid after the merge of step 0 and of step 1 of the input's two-station drive on the episode world, all unknown
    before (tests/sense_ref.py, as drive_slam_ref's steps 2 and 3)"""
    if name not in _GRIDS:
        grid, out = np.array(TR.STAGED, dtype=np.uint8, copy=True), []
        for p in inputs(oracle, name)["poses"]:
            grid = SR.sense_ref(grid, TR.WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, [p[:3]], [-1])["grid"]
            out.append(grid)
        _GRIDS[name] = out
    return _GRIDS[name]


_OCCLUDED = {}


def occluded_facts(oracle, ref_table, name, flags):
    """`facts` with the line of sight on the staged grid after each step's merge (occlusion_ref.occluded_pose_information), plus
    `open` = the voxels the same stations count without occlusion"""
    if name not in _OCCLUDED:
        inp = inputs(oracle, name)
        rows, per = [], []
        for k, (p, grid) in enumerate(zip(inp["poses"], staged_after(name, oracle))):
            G = oracle.Grid(grid, origin=EP.ORIGIN, resolution=EP.RES)
            sub = inp["cloud"][flags[k]]
            r = OR.occluded_pose_information(oracle, ref_table, G, sub, p[None], inp["fim"][0], inp["fim"][1], **OCCLUSION)
            rows.append(r)
            per.append(slabs(census(oracle, ref_table, sub, p, inp["fim"], keep=r["keep"][0]), 0))
        want = {c: np.concatenate([r[c] for r in rows]) for c in ("info_f64", "n_voxels", "n_visible")}
        _OCCLUDED[name] = dict(want=want, slabs=np.stack(per), open=facts(oracle, ref_table, name, flags=flags)["want"]["n_voxels"])
    return _OCCLUDED[name]


# ---- sixty-four robots on the wall cloud of the table cases

_FLEET = {}


def fleet(oracle):
    """A case of drive_slam_ref.table_cases' shape plus `cloud`: 64 robots in the south-west room of the episode world, looking north
    at the landmark-rich wall; 1 .. 6 stations (cycling) five cells apart along a row, rows and first columns spread over the room.
    Every fourth robot's goal lies one cell from its first station — mapped by its first sweep.  The cloud is wall_cloud without
    the landmarks that are borderline for one of the 224 poses.  `between`: robot 35 drives along row 10 out of the rich stretch's
    view; the threshold lies midway between its stations 3 and 4."""
    if not _FLEET:
        poses, goals = [], []
        for r in range(64):
            n, y, x0 = 1 + r % 6, 5 + (r * 11) % 38, 3 + (r * 7) % 24
            poses.append(DS.pose_rows(DR.line_stations(x0, x0 + 5 * (n - 1), y, 5, EP.ORIGIN, EP.RES), np.pi / 2))
            goals.append(DR.cell_centre(x0 + 1, y + 1, EP.ORIGIN, EP.RES) if r % 4 == 1 else FAR)
        cloud = LR.drop_borderline(oracle, np.concatenate(poses), DS.wall_cloud(EP.ORIGIN, EP.RES), [(DS.SENSOR["max_dist"], DS.SENSOR["max_angle"]), DS.FIM])
        _FLEET.update(poses=poses, goals=goals, cloud=cloud, first_ray=None, lm_sensor=DS.SENSOR, known=None, occlusion=None,
                      stop_when_mapped=True, gate=True, gate_first_station=1, between=(35, 3, 4))
    return _FLEET


def fleet_ref(oracle, ref_table, case, **over):
    """drive_slam_ref of the fleet's case on the episode world, staged all unknown"""
    c = dict(case, **over)
    return DS.drive_slam_ref(oracle, ref_table, TR.STAGED, TR.WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, c["poses"], c["goals"], c["cloud"], known=c["known"],
                             first_ray=c["first_ray"], lm_sensor=c["lm_sensor"], fim=DS.FIM, occlusion=c["occlusion"],
                             stop_when_mapped=c["stop_when_mapped"], threshold=c.get("threshold", DS.DEFAULT_THRESHOLD), gate=c["gate"],
                             gate_first_station=c["gate_first_station"])


def one_voxel_ref(oracle, ref_table, **over):
    """drive_slam_ref of one robot over the two stations of `one_voxel`, nothing known before"""
    inp = inputs(oracle, "one_voxel")
    return DS.drive_slam_ref(oracle, ref_table, TR.STAGED, TR.WORLD, EP.ORIGIN, EP.RES, EP.PARAMS, [inp["poses"]], [FAR], inp["cloud"],
                             lm_sensor=inp["sensor"], fim=inp["fim"], **over)
