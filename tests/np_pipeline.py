"""Stage-by-stage check of a detection backend against the numpy restatements (tests only).

A backend is anything with the C-ABI's calls: the HIP `capi.Detector` or the CPU `oracle.api.Oracle`.
Each stage is checked on the backend's OWN inputs (its normals feed the frame check, its frames feed
the sweep check, its point lists feed the image check), so a failure names one stage and not the
stages after it.  Nothing here reads the other backend: the truth is np_reference.

  1 normals  pca_normal (float64, LAPACK), within the Davis-Kahan bound of normal_bound
  2 frames   np_reference.local_frame on the backend's normals, majority camera of the draws
  3 sweep    sweep_sample_ordered on the backend's frames: records, point lists bit-equal
  4 prune    prune_keep on every record
  5 images   render_image on the backend's own point lists, bit-equal
  6 scores   lenet_f64.forward_f64 within lenet_f64.bound; the selection by selection_check

`run` returns a report of what each stage saw (counts, routes reached) so that a test can assert it
was not checked vacuously.
"""
from __future__ import annotations

import numpy as np

import np_reference as ref

U32 = 2.0 ** -24          # float32 unit roundoff
EPS64 = 2.0 ** -53        # float64 unit roundoff

PARAM_FIELDS = ("finger_width", "hand_outer_diameter", "hand_depth", "hand_height", "init_bite",
                "nn_radius_taubin", "nn_radius_hands", "normals_radius", "grid_cell", "num_orientations",
                "n_cams", "filter_half_grasps", "min_aperture", "max_aperture", "min_score_diff",
                "num_selected")


def params_of(backend) -> dict:
    """The backend's own parameter block as a dict (the restatements read these, not the test's)."""
    p = backend.params
    d = {k: getattr(p, k) for k in PARAM_FIELDS}
    d["cam_origin"] = np.array([[p.cam_origin[i][j] for j in range(3)] for i in range(2)])
    d["workspace"] = [float(p.workspace[i]) for i in range(6)]
    return d


class Case:
    """One input: cloud, parameters, samples (indices or coordinates), seeds, optional camera
    sources, given normals and LeNet weights.  `normals_subset`: check the normals of this many
    random points (the NaN pattern is always checked on every point)."""

    def __init__(self, name, xyz, prm, sample_idx=None, sample_xyz=None, slot_base=0, seed=0,
                 cam_source=None, normals=None, weights=None, normals_subset=None):
        self.name, self.xyz, self.prm = name, np.ascontiguousarray(xyz, dtype=np.float32), dict(prm)
        self.sample_idx, self.sample_xyz = sample_idx, sample_xyz
        self.slot_base, self.seed = slot_base, seed
        self.cam_source, self.normals, self.weights = cam_source, normals, weights
        self.normals_subset = normals_subset

    def samples(self) -> dict:
        if self.sample_idx is not None:
            return dict(sample_idx=self.sample_idx)
        return dict(sample_xyz=self.sample_xyz)

    def sample_points(self) -> np.ndarray:
        """The samples as the backends see them: float32 (hand_search.cpp:115, a PointXYZRGBA)."""
        if self.sample_idx is not None:
            return self.xyz[self.sample_idx]
        return np.asarray(self.sample_xyz, dtype=np.float64).T.astype(np.float32)


class Neighbours:
    """brute_radius semantics (float32 squared distance strictly below (float)(r*r), canonical
    order) with a k-d tree only to find candidates: the test itself is brute_radius's."""

    def __init__(self, xyz, cell):
        from scipy.spatial import cKDTree
        self.xyz = np.asarray(xyz, dtype=np.float32)
        assert np.isfinite(self.xyz).all()
        self.rank = np.empty(len(self.xyz), dtype=np.int64)
        self.rank[ref.canonical_order(self.xyz, cell)] = np.arange(len(self.xyz))
        self.tree = cKDTree(self.xyz.astype(np.float64))

    def candidates(self, q, r):
        pad = r * (1.0 + 1e-5) + 1e-6   # float32 rounding of the distance cannot reach this far
        return self.tree.query_ball_point(np.asarray(q, dtype=np.float64), pad, workers=-1)

    def exact(self, q, r, cand):
        cand = np.asarray(cand, dtype=np.int64)
        if not np.isfinite(q).all() or len(cand) == 0:
            return np.zeros(0, dtype=np.int32)
        got = ref.brute_radius(self.xyz[cand], q, r, self.rank[cand])
        return cand[got].astype(np.int32)

    def radius(self, q, r):
        q = np.asarray(q, dtype=np.float32)
        if not np.isfinite(q).all():
            return np.zeros(0, dtype=np.int32)
        return self.exact(q, r, self.candidates(q, r))


# ---- 1. normals ---------------------------------------------------------------------------------

def normal_bound(nb_xyz: np.ndarray, w: np.ndarray) -> float:
    """Bound on sin(angle) between a float32 plane-fit normal and the float64 one.

    The backends follow PCL 1.7 (hand_search.cpp:85-92): raw moments S = sum p p^T and s = sum p
    accumulated in float32 over the K neighbours, divided by K, then C = S/K - (s/K)(s/K)^T, then the
    smallest eigenvector.  With P = max |coordinate| over the neighbours and u = 2^-24:
      S/K   each of the K products and K-1 additions rounds once, in any summation order, and the
            division once more: |err| <= ((K + 1) u + O(u^2)) P^2;
      s/K   likewise |err| <= (K u + O(u^2)) P;
      m m^T the product of two perturbed means: 2 K u P^2, plus its own rounding u P^2;
      C     the final subtraction rounds a value of size <= 2 P^2: 2 u P^2.
    Per entry |E_ij| <= (3K + 4) u P^2 to first order; (3K + 6) u P^2 covers the second-order terms,
    and ||E||_2 <= 3 max |E_ij| for a 3 x 3 matrix.  By Davis-Kahan's sin-theta theorem the computed
    eigenvector is within sin(angle) <= ||E||_2 / delta of the exact one, delta the distance from
    the computed smallest eigenvalue to the exact middle one, and by Weyl delta >= (w1 - w0) - ||E||_2.
    The f64 eigen-solver (~1e-15 / gap) and the float32 store of the result (~sqrt(3) u) add 1e-6.
    Where the gap closes the bound grows past 1 and the angle is unconstrained: no case is skipped, the
    bound simply says nothing there."""
    K = nb_xyz.shape[0]
    P = float(np.abs(nb_xyz.astype(np.float64)).max())
    E2 = 3.0 * (3 * K + 6) * U32 * P * P
    delta = (w[1] - w[0]) - E2
    if delta <= 0:
        return np.inf
    return E2 / delta + 1e-6


def check_normals(backend, case, nb, prm, rng_seed=0) -> dict:
    got = backend.get_normals()
    xyz = case.xyz
    n = len(xyz)
    assert got.shape == (3, n)
    if case.normals is not None:
        # given normals (cloud_camera.cpp:27-31): float PointNormal fields, widened on use
        want = np.asarray(case.normals, dtype=np.float64).astype(np.float32).astype(np.float64)
        assert np.array_equal(got, want, equal_nan=True), "given normals were not kept as float32"
        return dict(given=True, checked=0, nan=int(np.isnan(got).any(axis=0).sum()))
    r = prm["normals_radius"]
    isnan = np.isnan(got)
    # NaN exactly where fewer than 3 neighbours (self included) are within the radius: the third
    # nearest point decides, by brute_radius's float32 test wherever float64 distances leave doubt
    d3 = nb.tree.query(xyz.astype(np.float64), k=min(3, n), workers=-1)[0].reshape(n, -1)[:, -1]
    few = (d3 > r * (1.0 + 1e-5) + 1e-6) if n >= 3 else np.ones(n, dtype=bool)
    doubt = np.flatnonzero((np.abs(d3 - r) <= r * 1e-5 + 1e-6) & (n >= 3))
    for i in doubt:
        few[i] = len(nb.radius(xyz[i], r)) < 3
    assert (few == isnan.any(axis=0)).all(), (
        "NaN pattern of the normals differs from the < 3 neighbour rule", np.flatnonzero(few != isnan.any(axis=0))[:10])
    assert (isnan.all(axis=0) == isnan.any(axis=0)).all()
    idx = np.flatnonzero(~few)
    if case.normals_subset is not None and len(idx) > case.normals_subset:
        idx = np.sort(np.random.default_rng(rng_seed).choice(idx, case.normals_subset, replace=False))
    checked = determined = 0
    worst = 0.0
    for i in idx:
        nbi = nb.radius(xyz[i], r)
        p = xyz[i].astype(np.float64)
        g = got[:, i]
        assert abs(np.linalg.norm(g) - 1.0) < 1e-6, (i, "normal is not unit length")
        # the flip towards the viewpoint (0,0,0), hand_search.cpp:88, decided by a float32 dot product
        assert -(p @ g) >= -4.0 * U32 * np.abs(p).sum(), (i, "normal faces away from the viewpoint")
        want, w = ref.pca_normal(xyz[nbi], xyz[i])
        bnd = normal_bound(xyz[nbi], w)
        s = np.linalg.norm(np.cross(g / np.linalg.norm(g), want))
        if bnd < 1.0:
            checked += 1
            worst = max(worst, s / bnd)
            assert s <= bnd, (i, "normal outside its Davis-Kahan bound", s, bnd, w)
            # where the bound leaves no doubt about the side, the sign must be the reference's
            if abs(want @ p) > (bnd + 1e-6) * np.linalg.norm(p):
                determined += 1
                assert g @ want > 0, (i, "viewpoint sign differs from the reference's")
    return dict(given=False, checked=checked, determined=determined, worst_ratio=worst,
                nan=int(few.sum()), points=n, doubtful=len(doubt))


# ---- 2. frames ----------------------------------------------------------------------------------

def frame_tolerance(m: int, w: np.ndarray) -> float:
    """Components of a frame from M = N^T N (m unit normals, f64): M's entries carry ~m eps of
    rounding, the eigenvector of its smallest eigenvalue moves by that over the gap w1 - w0, and the
    normal / binormal / curvature axis are linear in it."""
    gap = w[1] - w[0]
    return 1e-12 + 64.0 * m * EPS64 / max(gap, 1e-300)


def _aligned(got, want, v, tol):
    """want with the sign of got where the camera-facing flip of want is within tol of ambiguous."""
    if abs(want @ v) <= 4.0 * tol * np.linalg.norm(v) and got @ want < 0:
        return -want
    return want


def check_frames(backend, case, nb, prm, nrm) -> dict:
    fr, valid = backend.local_frames(slot_base=case.slot_base, seed=case.seed, **case.samples())
    Q = case.sample_points()
    assert fr.shape[0] == len(Q)
    finite_n = np.isfinite(nrm).all(axis=0)
    cs = None if case.cam_source is None else np.asarray(case.cam_source)
    ncam = 1 if cs is None else cs.shape[0]
    origins = np.asarray(prm["cam_origin"], dtype=np.float64)[:ncam]
    st = dict(valid=0, invalid=0, ties=0, majority=[0, 0], tie_flip_differs=0, maj1_flip_differs=0,
              compared=0)
    for t, q in enumerate(Q):
        nbt = nb.radius(q, prm["nn_radius_taubin"])
        nbt = nbt[finite_n[nbt]]   # NaN-normal neighbours are not drawn (ag2_oracle.cpp local_frame)
        assert valid[t] == (1 if len(nbt) else 0), (t, "frame validity differs from the neighbour rule")
        if not valid[t]:
            st["invalid"] += 1
            continue
        st["valid"] += 1
        s, n, b, c = fr[t, 0:3], fr[t, 3:6], fr[t, 6:9], fr[t, 9:12]
        assert np.array_equal(s, q.astype(np.float64)), t
        F = np.stack([n, b, c], axis=1)
        assert np.allclose(F.T @ F, np.eye(3), atol=1e-12), (t, "frame not orthonormal")
        assert np.linalg.det(F) > 0.999999, (t, "frame not right-handed")
        info = {}
        slot = case.slot_base + t
        args = dict(cam_source_nb=cs[:, nbt]) if cs is not None else {}
        org = origins if cs is not None else origins[0]
        rn, rb, rc, w = ref.local_frame(nrm[:, nbt].T, q, org, case.seed, slot, info=info, **args)
        maj = info["majority"]
        st["majority"][maj] += 1
        v = s - info["origin"]
        # local_frame.cpp:51-55: both axes face the majority camera (exact comparisons in f64)
        assert n @ v <= 1e-15 and b @ v <= 1e-15, (t, "frame does not face the majority camera", maj)
        if ncam == 2:
            votes = info["votes"]
            v0, v1 = s - origins[0], s - origins[1]
            differs = ((rn @ v0 > 0) != (rn @ v1 > 0)) or ((rb @ v0 > 0) != (rb @ v1 > 0))
            if votes[0] == votes[1]:
                st["ties"] += 1
                st["tie_flip_differs"] += int(differs)
            elif maj == 1:
                st["maj1_flip_differs"] += int(differs)
        tol = frame_tolerance(info["m"], w)
        # :42 argmax of the column sums: a sum within rounding of the maximum may win on either side
        gs = info["gsum"]
        cand = np.flatnonzero(gs >= gs.max() * (1.0 - 1e-12))
        errs = []
        for j in cand:
            rn, rb, rc, w = ref.local_frame(nrm[:, nbt].T, q, org, case.seed, slot, jmax=int(j), **args)
            an, ab = _aligned(n, rn, v, tol), _aligned(b, rb, v, tol)
            ac = np.cross(an, ab)
            errs.append(max(np.abs(n - an).max(), np.abs(b - ab).max(), np.abs(c - ac).max()))
        assert min(errs) <= tol, (t, "frame differs from the restatement", min(errs), tol, w)
        st["compared"] += 1
    return dict(st, frames=fr, valid_mask=valid)


# ---- 3. sweep -----------------------------------------------------------------------------------

def record_array(recs, dtype) -> np.ndarray:
    """Restated records (dicts of sweep_sample_ordered, plus 'slot') as the C-ABI's record type."""
    out = np.zeros(len(recs), dtype=dtype)
    for k, r in enumerate(recs):
        for f in ("axis", "approach", "binormal", "surface", "bottom", "top", "width", "half_antipodal",
                  "full_antipodal", "n_points", "orientation"):
            out[k][f] = r[f]
        out[k]["sample_slot"] = r["slot"]
    return out


def check_sweep(backend, case, nb, prm, nrm, frames, valid) -> dict:
    from oracle.api import HYP_DTYPE
    hyps = backend.generate_hypotheses(slot_base=case.slot_base, seed=case.seed, **case.samples())
    counters = backend.counters()
    tables = ref.hand_constants(prm)
    Q = case.sample_points()
    recs, kcrop, k2 = [], [], []
    for t, q in enumerate(Q):
        if not valid[t]:
            continue
        nb2 = nb.radius(q, prm["nn_radius_hands"])
        D = (case.xyz[nb2] - q[None, :]).astype(np.float64)   # float32 subtraction, then widened
        F = np.stack([frames[t, 3:6], frames[t, 6:9], frames[t, 9:12]], axis=1)
        out, kc = ref.sweep_sample_ordered(D, nrm[:, nb2].T, F, frames[t, 0:3], prm, tables)
        for r in out:
            r["slot"] = case.slot_base + t
        recs.extend(out)
        kcrop.append(kc)
        k2.append(len(nb2))
    want = record_array(recs, HYP_DTYPE)
    gk = {(int(h["sample_slot"]), int(h["orientation"])) for h in hyps}
    wk = {(int(h["sample_slot"]), int(h["orientation"])) for h in want}
    assert gk == wk, ("(sample_slot, orientation) sets differ", sorted(gk - wk)[:5], sorted(wk - gk)[:5])
    assert len(hyps) == len(want)
    for k in range(len(want)):
        assert hyps[k].tobytes() == want[k].tobytes(), (k, "record bytes differ", hyps[k], want[k])
    lists = []
    for k, r in enumerate(recs):
        p, q = backend.hyp_points(k, int(r["n_points"]))
        assert p.tobytes() == np.ascontiguousarray(r["pts"].T).tobytes(), (k, "hyp_points points differ")
        assert np.array_equal(q, r["nrm"].T, equal_nan=True), (k, "hyp_points normals differ")
        lists.append((p, q))
    assert counters.sum_kcrop == sum(kcrop), "the backend counted other cropped lists"
    return dict(hyps=hyps, lists=lists, kcrop=np.array(kcrop, dtype=np.int64), k2=np.array(k2, dtype=np.int64),
                counters=counters)


# ---- 4. prune, 5. images, 6. scores ---------------------------------------------------------------

def check_prune(backend, case, prm, hyps) -> np.ndarray:
    keep = backend.prune(len(hyps))
    mz = ref.cloud_min_z(case.xyz)
    want = np.array([ref.prune_keep(h, prm, mz) for h in hyps], dtype=np.uint8)
    bad = np.flatnonzero(keep != want)
    assert len(bad) == 0, ("prune flags differ from prune_keep", bad[:10], keep[bad[:10]])
    return keep


def check_images(backend, lists) -> np.ndarray:
    imgs = backend.render_images(0, len(lists))
    for k, (p, q) in enumerate(lists):
        assert np.array_equal(imgs[k], ref.render_image(p.T, q.T)), (k, "image bytes differ")
    return imgs


def _key(h):
    return int(h["sample_slot"]), int(h["orientation"])


def check_scores(backend, case, prm, hyps, keep, imgs) -> dict:
    import lenet_f64
    from agile_grasp2_amd.selection_check import check_selection
    sel, allh = backend.detect(slot_base=case.slot_base, seed=case.seed, do_prune=True, **case.samples())
    kept = np.flatnonzero(keep)
    # the scored set is exactly the records prune(n) keeps, in record order
    assert [_key(h) for h in allh] == [_key(h) for h in hyps[kept]], "detect scored another set than prune kept"
    for f in hyps.dtype.names:
        if f != "score":
            assert np.array_equal(allh[f], hyps[kept][f]), f
    if len(kept) == 0:
        return dict(scored=0, selected=len(sel))
    w = {k: np.asarray(v, dtype=np.float32) for k, v in case.weights.items()}
    logits = lenet_f64.forward_f64(w, imgs[kept])
    bnd = lenet_f64.bound(w, imgs[kept])
    truth = logits[:, 1] - logits[:, 0]
    eb = bnd[:, 0] + bnd[:, 1]
    tol = eb + U32 * (np.abs(truth) + eb) + 1e-30     # + the float32 subtraction of the two logits
    err = np.abs(allh["score"] - truth)
    assert (err <= tol).all(), ("score outside the float64 bound", np.flatnonzero(err > tol)[:5])
    true_all = allh.copy()
    true_all["score"] = truth
    chk = check_selection(sel, true_all, float(prm["min_score_diff"]), int(prm["num_selected"]),
                          float(tol.max()), tag=case.name)
    return dict(scored=len(kept), selected=len(sel), selection=chk)


def run(backend, case, scores=True) -> dict:
    """Load `case` into `backend` and check every stage; returns the report."""
    prm = params_of(backend)
    backend.set_cloud(case.xyz, cam_source=case.cam_source, normals=case.normals)
    if case.normals is None:
        backend.compute_normals()
    nb = Neighbours(case.xyz, prm["grid_cell"])
    rep = dict(name=case.name)
    rep["normals"] = check_normals(backend, case, nb, prm)
    nrm = backend.get_normals()
    fr = check_frames(backend, case, nb, prm, nrm)
    rep["frames"] = fr
    sw = check_sweep(backend, case, nb, prm, nrm, fr["frames"], fr["valid_mask"])
    rep["sweep"] = sw
    hyps = sw["hyps"]
    rep["keep"] = check_prune(backend, case, prm, hyps)
    rep["images"] = check_images(backend, sw["lists"])
    if scores and case.weights is not None:
        backend.lenet_load(case.weights)
        rep["scores"] = check_scores(backend, case, prm, hyps, rep["keep"], rep["images"])
    return rep
