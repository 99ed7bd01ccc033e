"""Threshold scenes on the CPU: the fixtures' own claims, and the oracle against the explicit-order
numpy restatement on them.

tests/threshold_scenes.py places one probe point per sample exactly on, one float32 lattice step
beside, or across the margin of each decision threshold of the hand sweep.  These tests state what
the fixtures contain (so the GPU parity tests on them mean something) and pin the oracle, the
checker of those GPU tests, to np_reference.sweep_sample_ordered at exactly these points.
"""
import numpy as np
import pytest

import np_reference as npr
import threshold_scenes as ts

GEOMETRIES = ("exact", "general")
MARGIN_CLASSES = ("top", "bottom", "fs", "fsr", "fsr_right", "crop_hi", "crop_lo")


@pytest.fixture(scope="module", params=GEOMETRIES)
def scene(request):
    sc = ts.build_scene(request.param, R=8)
    return sc, ts.restate(sc)


def by_class(sc):
    out = {}
    for p in sc.probes:
        out.setdefault(p["name"], []).append(p)
    return out


def test_exact_geometry_preconditions():
    from oracle import api
    sc = ts.build_scene("exact", R=8, classes=("top",))
    for row in sc.frames:
        F = ts.frame_matrix(row)
        assert set(np.abs(F).ravel().tolist()) <= {0.0, 1.0}, F
    for R in (8, 16, 32):
        p = api.default_params(**ts.base_params("exact", R))
        fs, ang, dep = api.hand_constants(p)
        assert ang[R // 2] == 0.0            # cos = 1, sin = 0 exactly: Fr = frame
        t = ts.hand_tables(ts.base_params("exact", R))
        assert np.array_equal(fs, t[0]) and np.array_equal(dep, t[4])
        assert t[2][R // 2] == 1.0 and t[3][R // 2] == 0.0
        assert fs[0] == 2.0 ** -7 - 2.0 ** -4 and fs[10] == 0.0   # slot bounds exact at k = 0
        sp = fs[11] - fs[10]
        assert 1.0 < 2.0 ** -7 / sp < 2.0      # the kernels' fast path applies (fast_ok)


def test_probe_placement(scene):
    """Each threshold has probes on both sides within one float32 lattice step, spread across the
    margin band, and (exact geometry) exactly on it."""
    sc, _ = scene
    cl = by_class(sc)
    assert set(cl) == set(MARGIN_CLASSES) | {"deepen", "radius"}
    for name, ps in cl.items():
        kinds = {p["kind"] for p in ps}
        assert {"lo1", "hi1", "lo2", "hi2"} <= kinds, name
        for p in ps:
            v, t = p["value"], p["threshold"]
            if p["kind"] == "eq":
                assert v == t
            elif p["kind"].startswith("lo"):
                assert v < t
            elif p["kind"].startswith("hi"):
                assert v > t
        near = [abs(p["value"] - p["threshold"]) for p in ps if p["kind"] in ("lo1", "hi1")]
        # exact geometry: one step of the centred lattice (<= 1.2e-7 m at these coordinates);
        # general geometry: the 3-D lattice search lands far closer
        assert max(near) <= (1.2e-7 if sc.geometry == "exact" else 2e-9), (name, near)
        if name in MARGIN_CLASSES:
            band = [p["value"] - p["threshold"] for p in ps if p["kind"] == "band"]
            m = ps[0]["margin"]
            assert sum(1 for b in band if -m < b < 0) >= 2 and sum(1 for b in band if 0 < b < m) >= 2
            assert min(band) < -m and max(band) > m
    eq = {p["name"] for p in sc.probes if p["kind"] == "eq"}
    if sc.geometry == "exact":
        assert set(MARGIN_CLASSES) <= eq           # equality really occurs
    assert "radius" in eq                          # d2 == (float)(r * r) in float32


def deciding(sc, rs):
    """Probe classes whose probe (on, or one lattice step beside, its threshold) decides a record:
    removing it changes its sample's restated records (a slot it alone occupies, the orientation it
    retires, the crop, the deepen step)."""
    out = set()
    for p in sc.probes:
        if p["kind"] not in ("lo1", "hi1", "eq"):
            continue
        s = p["sample"]
        sub = ts.Scene(sc.geometry, sc.R, sc.oi, sc.params, sc.xyz, sc.normals,
                       sc.sample_idx[s:s + 1], [], sc.frames[s:s + 1])
        without = ts.restate(sub, exclude=[p["index"]])[0]
        if ts.records_key(without["records"]) != ts.records_key(rs[s]["records"]):
            out.add(p["name"])
    return out


def test_probes_decide(scene):
    sc, rs = scene
    assert deciding(sc, rs) == set(by_class(sc))


@pytest.mark.parametrize("fw,od", [(0.005, 0.09), (0.01, 0.03)])
def test_probes_decide_slot_table_params(fw, od):
    """The scenes of the GPU slot-table tests (finger width outside (1, 2) spacings) keep threshold
    content: all but one class still decide (the outermost slot bounds move with the hand)."""
    sc = ts.build_scene("general", R=16, finger_width=fw, hand_outer_diameter=od)
    got = deciding(sc, ts.restate(sc))
    assert {"top", "fsr", "fsr_right", "crop_hi", "crop_lo", "deepen", "radius"} <= got, got


def test_patch_hand(scene):
    """Without its probe, every sample has a record at the probed orientation, with the hand
    ts.PATCH_HAND (the 'deepen' probes are placed in that hand's finger)."""
    sc, _ = scene
    rs = ts.restate(sc, exclude=[p["index"] for p in sc.probes])
    for r in rs:
        rec = [x for x in r["records"] if x["orientation"] == sc.oi]
        assert len(rec) == 1 and rec[0]["hand"] == ts.PATCH_HAND[sc.geometry]


def check_oracle(sc, rs):
    o = sc.oracle()
    got = o.generate_hypotheses(sample_idx=sc.sample_idx)
    c = o.counters()
    assert c.sum_k2 == sum(r["k2"] for r in rs)
    assert c.sum_kcrop == sum(r["kcrop"] for r in rs)
    want = [(s, rec) for s, r in enumerate(rs) for rec in r["records"]]
    assert len(got) == len(want)
    for h, (s, rec) in zip(got, want):
        assert h["sample_slot"] == s and h["orientation"] == rec["orientation"]
        for f in ("binormal", "approach", "axis", "surface", "bottom", "top"):
            assert np.array_equal(h[f], rec[f]), f
        assert h["width"] == rec["width"] and h["n_points"] == rec["n_points"]
        assert (h["half_antipodal"], h["full_antipodal"]) == (rec["half_antipodal"], rec["full_antipodal"])
    for k, (s, rec) in enumerate(want):
        pts, nrm = o.hyp_points(k, rec["n_points"])
        assert np.array_equal(pts.T, rec["pts"]) and np.array_equal(nrm.T, rec["nrm"]), k
    return got


@pytest.mark.parametrize("side", ["hi", "lo"])
@pytest.mark.parametrize("seed", range(6))
def test_slab_corner_scene(seed, side):
    """The row-culling case: the probe is inside the crop slab within 1e-8 m of its face and on the
    three cell edges where tighten_row's slab bound is tight; it decides its sample's record, and
    the oracle agrees with the restatement."""
    sc = ts.slab_corner_scene(seed, side)
    p = sc.probes[0]
    assert 0 < (p["threshold"] - p["value"]) * (1 if side == "hi" else -1) < 1e-8
    P = sc.xyz[p["index"]]
    o = sc.xyz.min(axis=0)
    assert np.array_equal(o, sc.xyz[-1])                 # the anchor is the grid origin
    inv = np.float32(1.0) / np.float32(0.01)
    for a, edge in enumerate(p["edges"]):
        nb = np.nextafter(P[a], np.float32(-np.inf) if edge == "low" else np.float32(np.inf))
        step = np.floor((nb - o[a]) * inv) - np.floor((P[a] - o[a]) * inv)
        assert step == (-1 if edge == "low" else 1), (a, edge)
    rs = ts.restate(sc)
    assert deciding(sc, rs) == {p["name"]}
    assert len(check_oracle(sc, rs)) >= 1


def test_deepen_step_exact():
    """Exact geometry with init_bite = ts.DEEPEN_BITE: a probe sits at y == depths[1] == 2^-6 in the
    left finger of the selected hand, where pass B's first estimate (y - depths[0]) * 200 floors to
    the wrong step; the probe decides the deepen step, and the oracle agrees with the restatement."""
    from oracle import api
    sc = ts.build_scene("exact", R=8, classes=("deepen",), init_bite=ts.DEEPEN_BITE)
    _, _, dep = api.hand_constants(api.default_params(**sc.params))
    assert dep[1] == 2.0 ** -6 and np.array_equal(dep, ts.hand_tables(sc.params)[4])
    assert (dep[1] - dep[0]) * 200.0 < 1.0               # the estimate says step 0, y fails step 1
    eq = [p for p in sc.probes if p["kind"] == "eq"]
    assert len(eq) == 1 and eq[0]["value"] == dep[1]
    rs = ts.restate(sc)
    assert deciding(sc, rs) == {"deepen"}
    check_oracle(sc, rs)


def test_estimate_wrong_side(scene):
    """General geometry: for every margin class some probe's float32 estimate lies on the wrong
    side of the threshold -- only the exact path can decide it.  (Exact geometry: the estimates
    are exact at the probed orientation.)"""
    sc, _ = scene
    wrong = {}
    for p in sc.probes:
        side = ts.estimate_side(sc, p)
        if side is None:
            continue
        truth = p["value"] < p["threshold"]
        wrong[p["name"]] = wrong.get(p["name"], 0) + int(side != truth)
    if sc.geometry == "general":
        assert all(wrong[c] >= 1 for c in MARGIN_CLASSES), wrong
    else:
        assert not any(wrong.values()), wrong


def test_oracle_matches_restatement(scene):
    """Records bit for bit, K2 / Kcrop counts and closing-region points of the oracle equal the
    restatement's on the threshold scenes."""
    sc, rs = scene
    got = check_oracle(sc, rs)
    assert len(got) > 5 * len(sc.sample_idx)


def test_oracle_radius_search_at_r(scene):
    """Points at d2 == (float)(r*r) and one lattice step either side: the strict < of the reference."""
    sc, _ = scene
    o = sc.oracle()
    rank = np.empty(len(sc.xyz), dtype=np.int64)
    rank[npr.canonical_order(sc.xyz)] = np.arange(len(sc.xyz))
    ps = [p for p in sc.probes if p["name"] == "radius"]
    for p in ps:
        q = sc.xyz[sc.sample_idx[p["sample"]]]
        got = o.radius_search(q, 0.1)
        want = npr.brute_radius(sc.xyz, q, 0.1, rank)
        assert np.array_equal(got, want)
        assert (p["index"] in got) == (p["value"] < p["threshold"])


def test_radius_shell_scene_oracle():
    """The normals scene of the GPU tests: the oracle's radius search at the normals radius keeps
    exactly the shell points with d2 < (float)(r*r), as the brute-force restatement does."""
    from oracle import api
    xyz, queries = ts.radius_shell_scene()
    o = api.Oracle(**dict(ts.base_params("general", 8), num_threads=2))
    o.set_cloud(xyz)
    rank = np.empty(len(xyz), dtype=np.int64)
    rank[npr.canonical_order(xyz)] = np.arange(len(xyz))
    r2f = np.float32(0.01 * 0.01)
    n_eq = 0
    for qi, shell in queries:
        got = o.radius_search(xyz[qi], 0.01)
        assert np.array_equal(got, npr.brute_radius(xyz, xyz[qi], 0.01, rank))
        for j, d2 in shell:
            assert (j in got) == (d2 < r2f)
            n_eq += d2 == r2f
        assert any(d2 < r2f for _, d2 in shell) and any(d2 > r2f for _, d2 in shell)
    assert n_eq >= 5
