"""Threshold scenes: clouds whose points sit ON the hand sweep's decision thresholds (tests only).

The sweep kernels decide most points from a float32 estimate of their rotated coordinates, or cull
them from a float32 bound, and redo the reference's float64 test only inside a margin around each
threshold (k_sweep.hip: classify, pass A, exact_A; k_sweep_common.h: tighten_row; k_sweep_orient.hip:
pass B).  Random clouds almost never put a point within float32 rounding of a threshold, so this
module builds scenes that do.

A scene is a set of isolated SAMPLES, each the centre of a small planar patch (given normals, so no
added point moves a normal) plus ONE probe point placed for a single threshold of one orientation of
that sample (`oi`).  The probe's centred coordinates are computed exactly as the oracle and the
kernels compute them: d = f32(p) - f32(q) in float32, widened, then
X[k] = (Fr[0][k] d0 + Fr[1][k] d1) + Fr[2][k] d2 with Fr = frame * rot formed as in
oracle/ag2_oracle.cpp (sweep_sample).  The probe position is found by a search over the float32
lattice around the ideal position, so a probe lands exactly on the threshold (where the arithmetic
allows it), on the nearest lattice values on either side, or at chosen offsets across the margin.
Patches are 0.3 m apart, so a probe is outside every other sample's hand radius (0.1 m).

Two geometries:
  exact    dyadic hand parameters and axis-aligned patch normals: the frame entries are 0 / +-1 and
           orientation R/2 has angle 0, so the rotated coordinates are plain components of d and
           equality with top, bottom, +-hand_height, the slot bounds and r^2 really occurs.
  general  the default (launch-file) hand parameters, tilted patches whose normals fan out across
           the patch (a well-conditioned frame), and an orientation with a non-trivial angle.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32

# margins of the kernels' fast paths (k_sweep.hip classify / pass A), in metres or slot spacings
CROP_BAND = 2.0e-6
Y_MARGIN = 1.0e-6
X_MARGIN_SPACINGS = 1.0e-4

EXACT_PARAMS = dict(finger_width=2.0 ** -7, hand_outer_diameter=2.0 ** -4, hand_depth=2.0 ** -4,
                    hand_height=2.0 ** -6, init_bite=2.0 ** -7)
GENERAL_PARAMS = dict(finger_width=0.01, hand_outer_diameter=0.09, hand_depth=0.06,
                      hand_height=0.02, init_bite=0.01)
CAMERA = np.array([0.0, 0.0, 3.0])


# ---- explicit-order arithmetic (the oracle's association order; no BLAS) ----------------------

def hand_tables(prm):
    """fs, fsr, cos_t, sin_t, depths as ag2_oracle.cpp computes them (libm cos/sin via math)."""
    od, fw, R = prm["hand_outer_diameter"], prm["finger_width"], int(prm["num_orientations"])
    step = ((od - fw) - 0.0) / 9.0
    fs = np.zeros(20)
    for i in range(10):
        h = 0.0 + float(i) * step
        fs[i] = (h - od) + fw
        fs[10 + i] = h
    fsr = fs + fw
    low = -1.0 * math.pi / 2.0
    astep = (math.pi / 2.0 - low) / float(R)
    ang = [low + float(i) * astep for i in range(R)]
    cos_t = np.array([math.cos(a) for a in ang])
    sin_t = np.array([math.sin(a) for a in ang])
    depths = []
    d = prm["init_bite"] + 0.005
    while d <= prm["hand_depth"]:
        depths.append(d)
        d += 0.005
    return fs, fsr, cos_t, sin_t, np.array(depths)


def frame_matrix(fr_row):
    """F[a][k]: column k = normal, binormal, curv of a local_frames row [sample, n, b, c]."""
    return np.stack([fr_row[3:6], fr_row[6:9], fr_row[9:12]], axis=1)


def rot_frame(F, cs, sn):
    """Fr = frame * rot (hand_search.cpp:356-357), element by element in the oracle's order."""
    rot = [[cs, -1.0 * sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]
    Fr = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            Fr[a, b] = (F[a, 0] * rot[0][b] + F[a, 1] * rot[1][b]) + F[a, 2] * rot[2][b]
    return Fr


def centred(p, q):
    """d = f32(p) - f32(q) in float32, widened (hand_search.cpp:209-210)."""
    return (np.asarray(p, dtype=F32) - np.asarray(q, dtype=F32)).astype(np.float64)


def rotated(M, d, k):
    """(M[0][k] d0 + M[1][k] d1) + M[2][k] d2 for rows of d (N x 3 float64)."""
    return (M[0, k] * d[..., 0] + M[1, k] * d[..., 1]) + M[2, k] * d[..., 2]


def dist2_f32(p, q):
    """float32 squared distance, (dx^2 + dy^2) + dz^2 (the grid's radius test)."""
    d = np.asarray(p, dtype=F32) - np.asarray(q, dtype=F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fma32(a, b, c):
    """float32 fma with one rounding (a*b is exact in float64 for float32 inputs; the sum is
    rounded once through exact rational arithmetic)."""
    from fractions import Fraction
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    out = np.empty(np.broadcast(a, b, c).shape, dtype=F32)
    for i, (x, y, z) in enumerate(np.broadcast(a, b, c)):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        f = F32(float(v))  # nearest f64, then f32: correct unless the f64 value is a f32 tie
        e = Fraction(float(f)) - v
        if e != 0:  # settle a double-rounding tie by the exact value
            other = np.nextafter(f, F32(np.inf) if e < 0 else F32(-np.inf))
            eo = Fraction(float(other)) - v
            if abs(eo) < abs(e) or (abs(eo) == abs(e) and (other.view(np.uint32) & 1) == 0):
                f = other
        out.reshape(-1)[i] = f
    return out


def pass_a_estimate(F, cs, sn, d):
    """The float32 estimates (x, y) of pass A (k_sweep.hip): u = n.d, v = b.d in f32,
    y ~ fma(c, v, -(s u)), x ~ fma(c, u, s v)."""
    d32 = np.asarray(d, dtype=np.float64).astype(F32)
    n = [F32(F[a, 0]) for a in range(3)]
    b = [F32(F[a, 1]) for a in range(3)]
    u = (n[0] * d32[..., 0] + n[1] * d32[..., 1]) + n[2] * d32[..., 2]
    v = (b[0] * d32[..., 0] + b[1] * d32[..., 1]) + b[2] * d32[..., 2]
    cf, sf = F32(cs), F32(sn)
    ya = fma32(cf, v, -(sf * u))
    xa = fma32(cf, u, sf * v)
    return xa, ya


def crop_estimate(F, d):
    """|curv . d| in float32 (k_sweep.hip classify)."""
    d32 = np.asarray(d, dtype=np.float64).astype(F32)
    c = [F32(F[a, 2]) for a in range(3)]
    return np.abs((c[0] * d32[..., 0] + c[1] * d32[..., 1]) + c[2] * d32[..., 2])


# ---- float32 lattice search ----------------------------------------------------------------------

def lattice(p, k):
    """All float32 points within +-k ulps of p in each coordinate: (2k+1)^3 x 3."""
    p = np.asarray(p, dtype=F32)
    axes = []
    for a in range(3):
        lo, hi, v = [], [], p[a]
        x = v
        for _ in range(k):
            x = np.nextafter(x, F32(-np.inf))
            lo.append(x)
        x = v
        for _ in range(k):
            x = np.nextafter(x, F32(np.inf))
            hi.append(x)
        axes.append(np.array(lo[::-1] + [v] + hi, dtype=F32))
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([x.reshape(-1) for x in g], axis=1)


def pick(cands, vals, thr, kind, off=0.0):
    """Choose one candidate: 'eq' value == thr; 'lo<n>' / 'hi<n>' the n-th distinct value strictly
    below / above thr; 'band' the value nearest thr + off.  Returns (index, value) or None."""
    if kind == "eq":
        hit = np.nonzero(vals == thr)[0]
        return (int(hit[0]), vals[hit[0]]) if len(hit) else None
    if kind == "band":
        i = int(np.argmin(np.abs(vals - (thr + off))))
        return i, vals[i]
    n = int(kind[2:])
    side = vals < thr if kind.startswith("lo") else vals > thr
    u = np.unique(vals[side])
    if len(u) < n:
        return None
    want = u[-n] if kind.startswith("lo") else u[n - 1]
    i = int(np.nonzero(vals == want)[0][0])
    return i, vals[i]


# ---- scenes -----------------------------------------------------------------------------------

def patch(center, normal, tilt, rng_step=0.0025, radius=0.0101):
    """Planar disc of points around `center` perpendicular to `normal`; normals fan by `tilt`
    radians across the disc about one in-plane axis (0: all equal to `normal`)."""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    t = np.cross(n, [0.0, 1.0, 0.0] if abs(n[1]) < 0.9 else [1.0, 0.0, 0.0])
    t /= np.linalg.norm(t)
    w = np.cross(n, t)
    m = int(radius / rng_step)
    pts, nrm = [], []
    for i in range(-m, m + 1):
        for j in range(-m, m + 1):
            a, b = i * rng_step, j * rng_step
            if a * a + b * b > radius * radius:
                continue
            pts.append(center + a * t + b * w)
            ang = tilt * a / radius
            nrm.append(math.cos(ang) * n + math.sin(ang) * t)
    return np.array(pts), np.array(nrm)


class Scene:
    """xyz (N x 3 float32), normals (3 x N float64), sample_idx, params and per-sample probe info."""

    def __init__(self, geometry, R, oi, params, xyz, normals, sample_idx, probes, frames):
        self.geometry, self.R, self.oi = geometry, R, oi
        self.params, self.xyz, self.normals, self.sample_idx = params, xyz, normals, sample_idx
        self.probes, self.frames = probes, frames

    def oracle(self, **kw):
        from oracle import api
        o = api.Oracle(**dict(self.params, num_threads=4, **kw))
        o.set_cloud(self.xyz, normals=self.normals)
        return o


def base_params(geometry, R, **kw):
    prm = dict(EXACT_PARAMS if geometry == "exact" else GENERAL_PARAMS)
    prm.update(num_orientations=R, min_score_diff=-1e30, num_selected=1000, filter_half_grasps=0,
               min_aperture=0.0, max_aperture=1.0, cam_origin=[CAMERA, CAMERA],
               workspace=[-10.0, 10.0, -10.0, 10.0, -10.0, 10.0])
    prm.update(kw)
    return prm


KINDS = ["eq", "lo1", "hi1", "lo2", "hi2", "lo3", "hi3"]
BANDS = [-2.0, -1.0, -0.5, -0.1, 0.1, 0.5, 1.0, 2.0]   # x margin


def threshold_classes(prm, fs, fsr, depths, geometry):
    """(name, coordinate, threshold, margin, frame-coordinate target of the probe).  The free
    coordinates place the probe where its side decides the record of a patch-only sample."""
    top, hh = prm["init_bite"], prm["hand_height"]
    bottom = prm["init_bite"] - prm["hand_depth"]
    sp = fs[11] - fs[10]
    k = 0 if geometry == "exact" else 1            # a slot whose hand is open on the bare patch
    only_k = 0.5 * (fs[k] + fs[k + 1])             # inside slot k and no other slot
    outside = fs[0] - 0.006                        # outside every slot
    ymid = top - 0.002
    xm = X_MARGIN_SPACINGS * sp
    return [
        ("top", 1, top, Y_MARGIN, (only_k, top, 0.0)),
        ("bottom", 1, bottom, Y_MARGIN, (outside, bottom, 0.0)),
        ("fs", 0, fs[k], xm, (fs[k], ymid, 0.0)),
        ("fsr", 0, fsr[k], xm, (fsr[k], ymid, 0.0)),
        ("fsr_right", 0, fsr[10 + k], xm, (fsr[10 + k], ymid, 0.0)),
        ("crop_hi", 2, hh, CROP_BAND, (only_k, ymid, hh)),
        ("crop_lo", 2, -hh, CROP_BAND, (only_k, ymid, -hh)),
        ("deepen", 1, depths[1], Y_MARGIN, (None, depths[1], 0.0)),   # x: the hand's left finger
        ("radius", 3, None, 0.0, (outside, None, 0.0)),                # behind the hand at r
    ]


def build_scene(geometry="exact", R=8, kinds=KINDS, bands=BANDS, classes=None, ulps=6,
                background=None, **kw):
    """Build a threshold scene (see the module docstring).  `background(q, Fr)` may return extra
    points for a sample (given the patch normal); `classes` limits the threshold classes."""
    from oracle import api
    prm = base_params(geometry, R, **kw)
    oi = R // 2 if geometry == "exact" else R // 2 + 1
    fs, fsr, cos_t, sin_t, depths = hand_tables(prm)
    cls = threshold_classes(prm, fs, fsr, depths, geometry)
    if classes is not None:
        cls = [c for c in cls if c[0] in classes]
    specs = []
    for c in cls:
        for kd in kinds:
            specs.append((c, kd, 0.0))
        if c[3] > 0:
            for b in bands:
                specs.append((c, "band", b * c[3]))
    rng = np.random.default_rng(17 if geometry == "exact" else 29)
    # patch centres on a 0.3 m lattice (dyadic 0.25 m + 0.0625 spacing in the exact geometry)
    n = len(specs)
    side = int(math.ceil(n ** (1.0 / 3.0)))
    step = 0.3125 if geometry == "exact" else 0.3
    pts, nrms, sidx, normals0 = [], [], [], []
    for i in range(n):
        g = np.array([i % side, (i // side) % side, i // (side * side)], dtype=np.float64)
        c = 0.25 + step * g
        if geometry == "exact":
            nn = np.array([0.0, 0.0, 1.0])
            tilt = 0.0
        else:
            c = c + rng.uniform(-0.01, 0.01, 3)
            nn = rng.normal(size=3)
            nn[2] = abs(nn[2]) + 0.5
            nn /= np.linalg.norm(nn)
            tilt = 0.25
        c = c.astype(F32).astype(np.float64)
        p, q = patch(c, nn, tilt)
        sidx.append(sum(len(x) for x in pts) + int(np.argmin(np.abs(p - c).sum(axis=1))))
        pts.append(p)
        nrms.append(q)
        normals0.append(nn)
    # an anchor at the origin pins the grid origin (the cloud's minimum), so the probes added below
    # cannot reorder any sample's neighbours and move its frame
    pts.append(np.zeros((1, 3)))
    nrms.append(np.array([[0.0, 0.0, 1.0]]))
    xyz = np.concatenate(pts).astype(F32)
    normals = np.concatenate(nrms).T.copy()
    sidx = np.array(sidx, dtype=np.int32)
    o = api.Oracle(**dict(prm, num_threads=4))
    o.set_cloud(xyz, normals=normals)
    fr, valid = o.local_frames(sample_idx=sidx)
    assert valid.all()
    r2f = F32(prm.get("nn_radius_hands", 0.1) * prm.get("nn_radius_hands", 0.1))
    probes, extra_xyz, extra_n = [], [], []
    for s, (c, kd, off) in enumerate(specs):
        name, coord, thr, margin, tgt = c
        F = frame_matrix(fr[s])
        Fr = rot_frame(F, cos_t[oi], sin_t[oi])
        q = xyz[sidx[s]]
        tgt = list(tgt)
        if name == "deepen":   # in the left finger of the hand the bare patch selects
            tgt[0] = 0.5 * (fsr[PATCH_HAND[geometry] - 1] + fs[PATCH_HAND[geometry] + 1]) \
                if PATCH_HAND[geometry] > 0 else 0.5 * (fs[0] + fs[1])
        if name == "radius":
            r = math.sqrt(float(r2f))   # behind the hand, outside every slot, two coordinates
            tgt = [tgt[0], -math.sqrt(r * r - tgt[0] * tgt[0]), 0.0]
        if kd == "band":
            tgt[coord] += off
        ideal = q.astype(np.float64) + Fr @ np.array(tgt, dtype=np.float64)
        cands = lattice(ideal, ulps)
        if name == "radius":
            vals = dist2_f32(cands, q)
            thr_v = r2f
        else:
            vals = rotated(Fr, centred(cands, q), coord)
            thr_v = thr
        got = pick(cands, vals, thr_v, kd, off)
        if got is None:   # (no lattice value of that kind: the sample keeps its bare patch)
            continue
        j, v = got
        probes.append(dict(sample=s, name=name, kind=kd, offset=off, threshold=thr_v, margin=margin,
                           coord=coord, value=v, index=len(xyz) + len(extra_xyz)))
        extra_xyz.append(cands[j])
        extra_n.append(normals0[s])
        if background is not None:
            bx = background(q, Fr, prm, fs, fsr)
            extra_xyz.extend(list(bx))
            extra_n.extend([normals0[s]] * len(bx))
    xyz = np.concatenate([xyz, np.array(extra_xyz, dtype=F32)])
    normals = np.concatenate([normals, np.array(extra_n).T], axis=1)
    sc = Scene(geometry, R, oi, prm, xyz, normals, sidx, probes, fr)
    fr2, valid2 = sc.oracle().local_frames(sample_idx=sidx)
    assert valid2.all() and np.array_equal(fr2, fr), "an added point moved a frame"
    return sc


# hand index the bare patch selects at the probed orientation (all ten hands open in the exact
# geometry: valid[ceil(10/2) - 1] = 4; asserted by test_threshold_scenes.test_patch_hand)
PATCH_HAND = {"exact": 4, "general": 4}


def restate(sc, exclude=None):
    """Per-sample records of the scene by the explicit-order restatement (np_reference), the radius
    neighbour count K2 and the cropped count K.  `exclude`: point indices to leave out."""
    import np_reference as npr
    prm = sc.params
    tables = hand_tables(prm)
    xyz = sc.xyz
    rank = np.empty(len(xyz), dtype=np.int64)
    rank[npr.canonical_order(xyz, prm.get("grid_cell", 0.01))] = np.arange(len(xyz))
    nrm = sc.normals.T.astype(F32).astype(np.float64)
    r = prm.get("nn_radius_hands", 0.1)
    out = []
    for s, si in enumerate(sc.sample_idx):
        q = xyz[si]
        nb = npr.brute_radius(xyz, q, r, rank)
        if exclude is not None:
            nb = nb[~np.isin(nb, exclude)]
        D = centred(xyz[nb], q)
        F = frame_matrix(sc.frames[s])
        recs, kc = npr.sweep_sample_ordered(D, nrm[nb], F, q.astype(np.float64), prm, tables)
        out.append(dict(records=recs, k2=len(nb), kcrop=kc, neighbours=nb))
    return out


def estimate_side(sc, p):
    """Side of the threshold the kernels' float32 estimate puts probe p on (True: below), or None
    where no estimate decides (radius: exact f32 test; deepen: f64 search)."""
    fs, fsr, cos_t, sin_t, depths = hand_tables(sc.params)
    s = p["sample"]
    F = frame_matrix(sc.frames[s])
    d = centred(sc.xyz[p["index"]][None], sc.xyz[sc.sample_idx[s]])
    if p["coord"] in (0, 1) and p["name"] != "deepen":
        xa, ya = pass_a_estimate(F, cos_t[sc.oi], sin_t[sc.oi], d)
        est = (xa if p["coord"] == 0 else ya)[0]
        return bool(est < F32(p["threshold"]))
    if p["coord"] == 2:
        ze = crop_estimate(F, d)[0]
        return bool((-ze if p["threshold"] < 0 else ze) < F32(p["threshold"]))
    return None


def records_key(recs):
    """Bytes that identify a sample's restated records (for 'does this point decide' checks)."""
    return b"".join(np.array([r["orientation"], r["n_points"], r["half_antipodal"], r["full_antipodal"]]
                             ).tobytes() + r["top"].tobytes() + r["bottom"].tobytes() +
                    r["surface"].tobytes() + np.float64(r["width"]).tobytes() for r in recs)


def blob(n, seed):
    """Background for the sweep's long-list routes: `n` points in front of the fingertips of the
    probed orientation (y beyond hand_depth, so no deepen step reaches them), inside the crop slab
    and the hand radius.  Returns a function for build_scene(background=...)."""
    rng = np.random.default_rng(seed)

    def make(q, Fr, prm, fs, fsr):
        hh = prm["hand_height"]
        X = np.stack([rng.uniform(-0.03, 0.03, n), rng.uniform(prm["hand_depth"] + 0.008, 0.09, n),
                      rng.uniform(-0.5 * hh, 0.5 * hh, n)], axis=1)
        return (q.astype(np.float64)[None, :] + X @ Fr.T).astype(F32)
    return make


def radius_shell_scene(r=0.01, seed=5):
    """Normals scene: query points at grid-cell corners, edges and faces, each with neighbours at
    d2 == (float)(r*r) and one float32 lattice step either side, in several directions, plus a few
    random points inside the radius.  Returns (xyz, list of (query index, [(point index, d2)]))."""
    rng = np.random.default_rng(seed)
    r2f = F32(r * r)
    pts = [np.zeros(3)]          # anchor: grid origin (0, 0, 0), cells at multiples of grid_cell
    queries = []
    dirs = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, 0, 1), (1, -1, 1), (-1, -1, -1), (0, 1, 1)]
    # near the origin, where the float32 lattice is fine enough for d2 to hit (float)(r*r) exactly
    centres = [(0.03, 0.03, 0.03), (0.06, 0.03, 0.035), (0.09, 0.035, 0.035), (0.12, 0.03, 0.03),
               (0.15, 0.033, 0.037)]
    for ci, c in enumerate(centres):
        q = np.array(c, dtype=F32)
        qi = len(pts)
        pts.append(q.astype(np.float64))
        for _ in range(12):
            v = rng.normal(size=3)
            pts.append(q + rng.uniform(0.2, 0.8) * r * v / np.linalg.norm(v))
        shell = []
        for di, dv in enumerate(dirs):
            u = np.array(dv, dtype=np.float64)
            cands = lattice(q.astype(np.float64) + r * u / np.linalg.norm(u), 5)
            vals = dist2_f32(cands, q)
            for kd in ("eq", "lo1", "hi1"):
                got = pick(cands, vals, r2f, kd)
                if got is not None:
                    shell.append((len(pts), float(got[1])))
                    pts.append(cands[got[0]].astype(np.float64))
        queries.append((qi, shell))
    return np.array(pts, dtype=F32), queries


# init_bite for a deepen-step scene in the exact geometry: depths[1], accumulated in float64 as the
# reference does, is then the dyadic 2^-6 (a float32 value that y reaches exactly), and pass B's
# first estimate (y - depths[0]) * 200 of a point at y == depths[1] rounds to just below 1: only
# the exact compares after it find the right step (k_sweep_orient.hip, pass B).
DEEPEN_BITE = 0.005625000000000001


def cell_edge_origin(p, edge, k=60, cell=0.01):
    """A float32 grid origin o below p such that p lies on the `edge` ('low' or 'high') of its grid
    cell in that coordinate: floor((p - o) * inv) is K and the neighbouring float32 value of p
    (below for 'low', above for 'high') lies in the neighbouring cell.  Arithmetic of cell_of
    (ag2_device.h) and of the oracle's grid."""
    inv = F32(1.0) / F32(cell)
    p = F32(p)
    nb = np.nextafter(p, F32(-np.inf) if edge == "low" else F32(np.inf))
    o = F32(float(p) - k * cell)
    step = np.float32(-np.inf)
    cand = [o]
    for direction in (F32(np.inf), F32(-np.inf)):
        x = o
        for _ in range(4000):
            x = np.nextafter(x, direction)
            cand.append(x)
    for o in sorted(cand, key=lambda v: abs(float(v) - float(cand[0]))):
        kp = np.floor((p - o) * inv)
        kn = np.floor((nb - o) * inv)
        if kn == kp + (-1 if edge == "low" else 1):
            return o
    raise AssertionError("no grid origin puts the point on a cell edge")


def slab_corner_scene(seed, side="hi", kind=None, R=8):
    """One sample whose probe is inside the crop slab, within a float32 step of its face, and at the
    corner of its grid cell where the row culling's slab bound is tight (k_sweep_common.h,
    tighten_row): on the y and z edges that give the row's extreme of curv_y dy + curv_z dz, and on
    the x edge the slab bound cuts.  The grid origin (pinned by an anchor point at the cloud's
    minimum) is chosen to put the cell edges there.  The patch normals are all equal, so the frame
    does not depend on the neighbours' order and the origin cannot move it."""
    from oracle import api
    prm = base_params("general", R)
    oi = R // 2 + 1
    fs, fsr, cos_t, sin_t, _ = hand_tables(prm)
    rng = np.random.default_rng(seed)
    nn = rng.normal(size=3)
    nn[2] = abs(nn[2]) + 0.5
    nn /= np.linalg.norm(nn)
    c = (0.6 + rng.uniform(-0.05, 0.05, 3)).astype(F32).astype(np.float64)
    pts, _ = patch(c, nn, 0.0)
    xyz = np.concatenate([pts, np.zeros((1, 3))]).astype(F32)
    si = int(np.argmin(np.abs(pts - c).sum(axis=1)))
    normals = np.tile(nn[:, None], (1, len(xyz) + 1))
    o = api.Oracle(**dict(prm, num_threads=1))
    o.set_cloud(xyz, normals=normals[:, :-1])
    fr, valid = o.local_frames(sample_idx=np.array([si], dtype=np.int32))
    assert valid.all()
    F = frame_matrix(fr[0])
    Fr = rot_frame(F, cos_t[oi], sin_t[oi])
    q = xyz[si]
    hh = prm["hand_height"]
    thr = hh if side == "hi" else -hh
    kind = kind or ("lo1" if side == "hi" else "hi1")    # the inside neighbour of the face
    ideal = q.astype(np.float64) + Fr @ np.array([0.5 * (fs[1] + fs[2]), prm["init_bite"] - 0.002, thr])
    cands = lattice(ideal, 6)
    vals = rotated(F, centred(cands, q), 2)
    j, v = pick(cands, vals, thr, kind)
    P = cands[j]
    cn = [F32(F[a, 2]) for a in range(3)]
    sg = 1.0 if side == "hi" else -1.0          # inside: sg * (cx dx + cy dy + cz dz) < hh
    edges = ["low" if sg * cn[0] > 0 else "high"]
    edges += ["low" if sg * cn[a] >= 0 else "high" for a in (1, 2)]
    origin = np.array([cell_edge_origin(P[a], edges[a]) for a in range(3)], dtype=F32)
    xyz = np.concatenate([pts.astype(F32), P[None, :], origin[None, :]]).astype(F32)
    sc = Scene("general", R, oi, prm, xyz, normals, np.array([si], dtype=np.int32),
               [dict(sample=0, name="crop_corner_" + side, kind=kind, offset=0.0, threshold=thr,
                     margin=CROP_BAND, coord=2, value=v, index=len(pts), edges=edges)], fr)
    fr2, valid2 = sc.oracle().local_frames(sample_idx=sc.sample_idx)
    assert valid2.all() and np.array_equal(fr2, fr), "the grid origin moved the frame"
    return sc
