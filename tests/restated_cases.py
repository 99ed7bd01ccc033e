"""Inputs of the stage-by-stage restatement tests (tests only), shared by the GPU file
(test_gpu_restated.py, HIP Detector) and the CPU file (test_oracle_restated.py, Oracle).

Each builder returns an np_pipeline.Case plus the constructor parameters of a backend; the tests
assert, from np_pipeline.run's report, that the route or edge a case is for was reached.
"""
from __future__ import annotations

import numpy as np

import np_pipeline as npp
import np_reference as ref
from conftest import scene_params
from agile_grasp2_amd import scene
from agile_grasp2_amd.weights import make_lenet_weights

# k_sweep_orient.hip stages a cropped list in LDS chunks of kOStage points; a longer list is worked
# through in several chunks (the multi-chunk route), and one of more than kOMaskChunks chunks does
# not keep its membership ballots between passes C and D
SWEEP_STAGE_POINTS = 2432
SWEEP_MASK_CHUNKS = 8


def fuzz_case(seed):
    """test_gpu_fuzz.draw_case's configuration `seed`, on the same scene, samples and weights."""
    from test_gpu_fuzz import draw_case
    prm, kind, n, n_samples = draw_case(seed)
    xyz, ws = scene.make_scene(seed=50 + seed, n_target=n, kind=kind)
    idx = scene.draw_samples(seed, xyz.shape[0], n_samples)
    full = scene_params(ws, num_threads=4, **prm)
    return npp.Case(f"fuzz{seed}", xyz, full, sample_idx=idx, seed=seed, weights=make_lenet_weights(seed)), full


def small_case(name, seed=5, n_samples=120, **kw):
    """The conftest small scene (6 000 points, one camera) under other parameters."""
    xyz, ws = scene.make_scene(seed=3, n_target=6000)
    idx = scene.draw_samples(3, xyz.shape[0], n_samples)
    full = scene_params(ws, num_threads=4, **dict(dict(min_score_diff=-1e30, num_selected=100000), **kw))
    return npp.Case(name, xyz, full, sample_idx=idx, seed=seed, weights=make_lenet_weights(seed)), full


def given_normals_case():
    """Normals supplied with the cloud (cloud_camera.cpp:4-32): the float64 plane fit of every point
    (NaN where it has fewer than 3 neighbours), turned by a seeded jitter so that they are not the
    ones compute_normals would produce."""
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    nb = npp.Neighbours(xyz, 0.01)
    rng = np.random.default_rng(12)
    nrm = np.full((3, len(xyz)), np.nan)
    for i in range(len(xyz)):
        k = nb.radius(xyz[i], 0.01)
        if len(k) >= 3:
            n, _ = ref.pca_normal(xyz[k], xyz[i])
            n = n + rng.normal(scale=0.05, size=3)
            nrm[:, i] = n / np.linalg.norm(n)
    idx = scene.draw_samples(12, len(xyz), 100)
    full = scene_params(ws, num_threads=4, min_score_diff=-1e30, num_selected=100000)
    return npp.Case("given_normals", xyz, full, sample_idx=idx, seed=4, normals=nrm,
                    weights=make_lenet_weights(4)), full


def xyz_samples_case(slot_base=1000):
    """Samples given as coordinates (jittered cloud points, one far outside the cloud, one NaN) and
    numbered from slot_base."""
    xyz, ws = scene.make_scene(seed=3, n_target=6000)
    idx = scene.draw_samples(3, xyz.shape[0], 60)
    rng = np.random.default_rng(8)
    sx = (xyz[idx].astype(np.float64) + rng.normal(scale=0.004, size=(len(idx), 3))).T
    sx[:, 3] = [10.0, 10.0, 10.0]   # no neighbours: no frame
    sx[:, 4] = np.nan               # invalid sample: no frame
    full = scene_params(ws, num_threads=4, min_score_diff=-1e30, num_selected=100000)
    return npp.Case("xyz_samples", xyz, full, sample_xyz=sx, slot_base=slot_base, seed=6,
                    weights=make_lenet_weights(6)), full


def dense_case(n_orient=8, n_samples=12):
    """Un-voxelised dense clutter at 0.5 mm spacing: cropped neighbourhoods of tens of thousands of
    points leave the LDS stage of the sweep (long-list route) and span many staging chunks."""
    xyz, ws = scene.make_scene(seed=5, n_target=200000, kind="objects", voxel=None, spacing=0.0005)
    idx = scene.draw_samples(5, xyz.shape[0], n_samples)
    full = scene_params(ws, num_threads=4, num_orientations=n_orient, min_score_diff=-1e30,
                        num_selected=100000)
    return npp.Case("dense", xyz, full, sample_idx=idx, seed=7, weights=make_lenet_weights(7),
                    normals_subset=3000), full


# camera_source columns of the two-camera case, by band of x: seen by one camera, by the other, by
# both (a tie of the vote), "not seen" (2, cloud_camera.cpp:151) beside a 1, and by neither
CAM_BANDS = [(1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (2, 2), (1, 1)]


def two_camera_case(seed=1):
    """Two cameras with distinct origins on opposite sides of the objects and a per-point
    camera_source in bands of x (CAM_BANDS): samples inside a (1, 1) or (2, 2) band draw an exact tie,
    samples inside a (2, 1) band vote for camera 1 only."""
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    n = len(xyz)
    q = np.quantile(xyz[:, 0], np.linspace(0, 1, len(CAM_BANDS) + 1)[1:-1])
    band = np.searchsorted(q, xyz[:, 0])
    cam = np.array(CAM_BANDS, dtype=np.int32)[band].T.copy()
    assert cam.shape == (2, n)
    cams = [scene.CAMERA, np.array([1.3, 0.45, -0.05])]
    idx = scene.draw_samples(20 + seed, n, 160)
    full = scene_params(ws, num_threads=4, n_cams=2, cam_origin=cams, min_score_diff=-1e30,
                        num_selected=100000)
    return npp.Case("two_cameras", xyz, full, sample_idx=idx, seed=seed, cam_source=cam,
                    weights=make_lenet_weights(seed)), full


def assert_reached(rep, records=True):
    """Every case: frames were compared, and (unless stated) records were swept, listed and imaged."""
    assert rep["frames"]["compared"] > 0, rep["name"]
    if records:
        assert len(rep["sweep"]["hyps"]) > 0, rep["name"]
        assert rep["images"].max() > 0, rep["name"]


# ---- prune on its bounds ------------------------------------------------------------------------

def f32_around(v):
    """(largest float32 <= v, smallest float32 > v) for a float64 v."""
    f = np.float32(v)
    if float(f) > v:
        f = np.nextafter(f, np.float32(-np.inf))
    return float(f), float(np.nextafter(f, np.float32(np.inf)))


def prune_scene():
    """Tabletop scene, every prune test open (wide workspace, apertures 0..1, no half filter)."""
    xyz, ws = scene.make_scene(seed=3, n_target=6000)
    idx = scene.draw_samples(3, xyz.shape[0], 120)
    prm = scene_params([-10.0, 10.0, -10.0, 10.0, -10.0, 10.0], num_threads=4, min_aperture=0.0,
                       max_aperture=1.0, filter_half_grasps=0, min_score_diff=-1e30, num_selected=100000)
    return xyz, idx, prm


def with_extra_point(xyz, z):
    """xyz plus one point far beside the cloud (0.5 m beyond its x extent: outside every hand radius
    of every sample) at height z: it sets the cloud's min_z when z is below the cloud."""
    e = np.array([[float(xyz[:, 0].max()) + 0.5, float(xyz[:, 1].mean()), z]], dtype=np.float32)
    return np.concatenate([xyz, e])


def same_canonical_order(a, b):
    n = min(len(a), len(b))
    oa, ob = ref.canonical_order(a), ref.canonical_order(b)
    return np.array_equal(oa[oa < n], ob[ob < n])


def prune_on_bounds(make, seed=5):
    """Prune with its parameters sitting exactly on recorded values (grasp_detector.cpp:363-395).

    One run of prune_scene picks a record; detectors built by make(params) then run the same cloud,
    samples and seed with min_aperture / max_aperture at the record's width and its float64
    neighbours, the x / y workspace bounds at the float32 values on either side of the record's corner
    extremes, and one extra isolated point whose z puts the cloud's min_z on either side of the
    record's lowest corner.  Every variant: records byte-identical to its reference run (so only the
    prune decision moves), flags equal to prune_keep on that variant's records, the chosen record's
    flag where prune_keep puts it, and detect's scored set the kept set.  Returns the flips seen."""
    xyz, idx, prm = prune_scene()
    w = make_lenet_weights(seed)
    resolved = {}

    def run(p, cloud):
        b = make(p)
        b.set_cloud(cloud)
        b.compute_normals()
        h = b.generate_hypotheses(sample_idx=idx, seed=seed)
        keep = b.prune(len(h))
        bp = npp.params_of(b)
        resolved.setdefault("prm", bp)
        mz = ref.cloud_min_z(cloud)
        want = np.array([ref.prune_keep(x, bp, mz) for x in h], dtype=np.uint8)
        assert np.array_equal(keep, want), ("prune flags differ from prune_keep", np.flatnonzero(keep != want)[:5])
        b.lenet_load(w)
        _, allh = b.detect(sample_idx=idx, seed=seed)
        kk = [(int(x["sample_slot"]), int(x["orientation"])) for x in h[keep == 1]]
        assert [(int(x["sample_slot"]), int(x["orientation"])) for x in allh] == kk, "detect scored another set"
        if hasattr(b, "close"):
            b.close()
        return h, keep

    base_h, base_keep = run(prm, xyz)
    assert len(base_h) > 20 and 0 < base_keep.sum() < len(base_h)
    k = int(np.flatnonzero((base_keep == 1) & (base_h["width"] > 0))[0])
    flips = []

    def variant(p, cloud, expect, what, ref_h=base_h):
        h, keep = run(p, cloud)
        assert h.tobytes() == ref_h.tobytes(), (what, "records moved: the variant is not a pure prune change")
        assert keep[k] == expect, (what, "record", k, "flag", int(keep[k]), "expected", expect)
        flips.append((what, expect))
        return keep

    wd = float(base_h[k]["width"])
    dn, up = float(np.nextafter(wd, -np.inf)), float(np.nextafter(wd, np.inf))
    for field, v, expect in (("min_aperture", wd, 1), ("min_aperture", up, 0), ("min_aperture", dn, 1),
                             ("max_aperture", wd, 1), ("max_aperture", dn, 0), ("max_aperture", up, 1)):
        variant(dict(prm, **{field: v}), xyz, expect, (field, v))
    P = ref.prune_corners(base_h[k], resolved["prm"])
    for a in (0, 1):
        lo_in, lo_out = f32_around(P[:, a].min())          # min bound: <= the corner keeps
        hi_below, hi_above = f32_around(P[:, a].max())
        hi_in, hi_out = (hi_below, float(np.nextafter(np.float32(hi_below), np.float32(-np.inf)))) \
            if hi_below == P[:, a].max() else (hi_above, hi_below)
        for i_bound, v, expect in ((2 * a, lo_in, 1), (2 * a, lo_out, 0), (2 * a + 1, hi_in, 1), (2 * a + 1, hi_out, 0)):
            ws = list(prm["workspace"])
            ws[i_bound] = v
            variant(dict(prm, workspace=ws), xyz, expect, ("workspace", i_bound, v))
    # min_z: the extra point sits below the cloud; a record whose lowest corner lies below the cloud is
    # chosen where moving the point from z0 to the corner keeps every point's grid cell (same
    # canonical order: same neighbour order, same frames and records)
    zc = float(ref.cloud_min_z(xyz))
    z0 = float(np.float32(zc - 0.03))
    x0 = with_extra_point(xyz, z0)
    h0, keep0 = run(prm, x0)
    mnz = np.array([ref.prune_corners(x, resolved["prm"])[:, 2].min() for x in h0])
    order = np.argsort(np.abs(mnz - z0))
    pick = None
    for j in order[:80]:
        if not mnz[j] < zc - 0.001:
            continue
        z1, z2 = f32_around(mnz[j])
        if same_canonical_order(x0, with_extra_point(xyz, z1)) and same_canonical_order(x0, with_extra_point(xyz, z2)):
            pick = int(j)
            break
    assert pick is not None, "no record whose lowest corner can carry the cloud's min_z"
    k = pick
    z1, z2 = f32_around(mnz[k])
    variant(prm, with_extra_point(xyz, z1), 1, ("min_z", z1), ref_h=h0)
    variant(prm, with_extra_point(xyz, z2), 0, ("min_z", z2), ref_h=h0)
    return flips


# ---- what each case must reach --------------------------------------------------------------------

def expect_filter_half(rep):
    """filter_half_grasps=1 (grasp_detector.cpp:369): the gate drops records that are not half
    antipodal, and keeps half-but-not-fully antipodal ones (a gate on full_antipodal would not)."""
    h, keep = rep["sweep"]["hyps"], rep["keep"]
    assert (h["half_antipodal"] == 0).any(), "no record for the gate to drop"
    assert not keep[h["half_antipodal"] == 0].any()
    assert (keep[(h["half_antipodal"] == 1) & (h["full_antipodal"] == 0)] == 1).any(), \
        "no half-only record passed the gate"


def expect_two_cameras(rep, case):
    """Both cameras won votes; exact ties (first camera wins) and camera-1 majorities occurred on
    frames whose flip the two origins decide differently; and "not seen" (2) entries were drawn."""
    f = rep["frames"]
    assert f["majority"][0] > 0 and f["majority"][1] > 0, f["majority"]
    assert f["ties"] > 0 and f["tie_flip_differs"] > 0, f
    assert f["maj1_flip_differs"] > 0, f
    assert (np.asarray(case.cam_source) == 2).any()


def expect_dense(rep):
    """The restated cropped lists span more than kOMaskChunks staging chunks of the sweep."""
    kc = rep["sweep"]["kcrop"]
    assert kc.max() > SWEEP_STAGE_POINTS * SWEEP_MASK_CHUNKS, kc.max()
    assert (kc > SWEEP_STAGE_POINTS).sum() >= 3, kc


def expect_xyz_samples(rep, case):
    """Coordinate samples: the far and the NaN sample have no frame; slots start at slot_base."""
    assert rep["frames"]["invalid"] >= 2
    assert rep["sweep"]["hyps"]["sample_slot"].min() >= case.slot_base > 0
