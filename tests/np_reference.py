"""Independent numpy/scipy re-derivations used to pin the C++ oracle (tests only).

Each function recomputes one stage of the reference algorithm a second way (brute force, LAPACK
eigh, scipy.ndimage, torch-CPU conv) so that a mistake in oracle/ag2_oracle.cpp does not silently
become the definition of "correct".  Citations are to files of the reference tree (gwding/agile_grasp2).
"""
from __future__ import annotations

import numpy as np

MASK64 = (1 << 64) - 1


def draw_u64(seed: int, slot: int, j: int) -> int:
    """The counter RNG that replaces rand() (hand_search.cpp:130), in Python integers."""
    x = (seed ^ ((0x9E3779B97F4A7C15 * (slot + 1)) & MASK64)) & MASK64
    x = (x + ((0xD1B54A32D192ED03 * (j + 1)) & MASK64)) & MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def grid_keys(xyz: np.ndarray, cell: float = 0.01):
    """Cell key of every point: float32 arithmetic, x fastest."""
    xyz = xyz.astype(np.float32)
    o = xyz.min(axis=0)
    inv = np.float32(1.0) / np.float32(cell)
    c = np.floor((xyz - o) * inv).astype(np.int64)
    dims = c.max(axis=0) + 1
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def canonical_order(xyz: np.ndarray, cell: float = 0.01) -> np.ndarray:
    """sorted position -> original index, ascending (cell key, index)."""
    k = grid_keys(xyz, cell)
    return np.lexsort((np.arange(len(k)), k)).astype(np.int32)


def brute_radius(xyz: np.ndarray, q: np.ndarray, r: float, rank: np.ndarray) -> np.ndarray:
    """Exact radius search semantics of pcl::KdTreeFLANN::radiusSearch (hand_search.cpp:122,:201):
    float squared distance strictly below (float)(r*r); returned in canonical order."""
    xyz = xyz.astype(np.float32)
    d = xyz - q.astype(np.float32)[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = np.nonzero(d2 < np.float32(r * r))[0]
    return idx[np.argsort(rank[idx], kind="stable")].astype(np.int32)


def pca_normal(nb_xyz: np.ndarray, p: np.ndarray) -> np.ndarray:
    """Plane-fit normal (pcl::NormalEstimationOMP, hand_search.cpp:85-92) in float64 with LAPACK,
    flipped towards the viewpoint (0,0,0)."""
    a = nb_xyz.astype(np.float64)
    c = np.cov(a.T, bias=True)
    w, v = np.linalg.eigh(c)
    n = v[:, 0]
    if np.dot(-p.astype(np.float64), n) < 0:
        n = -n
    return n, w


def majority_camera(cam_source_cols: np.ndarray) -> int:
    """HandSearch::calculateLocalFrames' camera vote (hand_search.cpp:133-146): per camera, count the
    drawn neighbours whose camera_source entry is exactly 1 (:139; a 2 marks "not seen",
    cloud_camera.cpp:151, and does not count); VectorXi::maxCoeff(&i) returns the FIRST maximum, so
    a tie goes to the lower camera index.  cam_source_cols: n_cams x m, one column per draw."""
    votes = (np.asarray(cam_source_cols) == 1).sum(axis=1)
    return int(np.argmax(votes))  # argmax: first maximum


def local_frame(normals_nb: np.ndarray, sample: np.ndarray, cam_origin: np.ndarray,
                seed: int, slot: int, cam_source_nb: np.ndarray | None = None, jmax: int | None = None,
                info: dict | None = None):
    """LocalFrame::findAverageNormalAxis (local_frame.cpp:26-59) on the drawn normals.
    normals_nb: K x 3 finite neighbour normals in canonical order.

    cam_origin: one origin (3,), or with cam_source_nb (n_cams x K, the neighbours' camera_source
    columns) the origins of every camera (n_cams x 3): the frame then faces the majority camera of
    the draws (hand_search.cpp:133-146, local_frame.cpp:51-55).  jmax overrides the argmax of
    :42 (for callers that resolve a near-tie of the column sums); info, if given, receives the
    draws, the majority camera, the column sums and the eigenvalues of M."""
    k = normals_nb.shape[0]
    m = min(50, k)
    picks = [draw_u64(seed, slot, j) % k for j in range(m)]
    origin = np.asarray(cam_origin, dtype=np.float64)
    majority = 0
    if cam_source_nb is not None:
        drawn = np.asarray(cam_source_nb)[:, picks]
        majority = majority_camera(drawn)
        origin = origin.reshape(-1, 3)[majority]
        if info is not None:
            info["votes"] = (drawn == 1).sum(axis=1)
    N = normals_nb[picks].astype(np.float64)
    N = N / np.linalg.norm(N, axis=1, keepdims=True)
    M = N.T @ N
    w, v = np.linalg.eigh(M)
    c = v[:, 0]
    G = (N @ N.T) ** 6
    gsum = G.sum(axis=0)
    if jmax is None:
        jmax = int(np.argmax(gsum))
    npart = (np.eye(3) - np.outer(c, c)) @ N[jmax]
    normal = npart / np.linalg.norm(npart)
    binormal = np.cross(c, normal)
    v2 = sample.astype(np.float64) - origin
    if normal @ v2 > 0:
        normal = -normal
    if binormal @ v2 > 0:
        binormal = -binormal
    curv = np.cross(normal, binormal)
    if info is not None:
        info.update(picks=picks, majority=majority, origin=origin, gsum=gsum, jmax=jmax, m=m)
    return normal, binormal, curv, w


def hand_constants(prm):
    """(fs, fsr, cos_t, sin_t, depths) of the hand sweep, derived from the reference in its own
    operation order:
      fs      FingerHand ctor, finger_hand.cpp:9-12: fs_half = VectorXd::LinSpaced(10, 0.0, od - fw),
              finger_spacing_ << (fs_half - od + fw), fs_half.  LinSpaced as Eigen 3.2 (ROS Indigo)
              evaluates it: low + i * ((high - low) / (n - 1)) for every i (Eigen >= 3.3 returns `high`
              itself for the last entry: fs[9], fs[19] could then differ by one ulp).
      fsr     the slot's right edge, finger_spacing_(i) + finger_width_ (finger_hand.cpp:61).
      angles  hand_search.cpp:179-180: LinSpaced(R + 1, -pi/2, pi/2), first R entries; rot's
              cos / sin (:357) by libm.
      depths  FingerHand::deepenHand, finger_hand.cpp:118-122: depth = min_depth + 0.005, then
              += 0.005 while depth <= max_depth, accumulated in double (min_depth = init_bite,
              max_depth = hand_depth: hand_search.cpp:373)."""
    import math
    od, fw, R = float(prm["hand_outer_diameter"]), float(prm["finger_width"]), int(prm["num_orientations"])
    n = 10
    low, high = 0.0, od - fw
    step = (high - low) / float(n - 1)
    fs_half = [low + float(i) * step for i in range(n)]
    fs = np.array([(h - od) + fw for h in fs_half] + fs_half)
    fsr = np.array([f + fw for f in fs])
    alow, ahigh = -1.0 * math.pi / 2.0, math.pi / 2.0
    astep = (ahigh - alow) / float(R)
    ang = [alow + float(i) * astep for i in range(R)]
    cos_t = np.array([math.cos(a) for a in ang])
    sin_t = np.array([math.sin(a) for a in ang])
    depths = []
    d = float(prm["init_bite"]) + 0.005
    while d <= float(prm["hand_depth"]):
        depths.append(d)
        d += 0.005
    return fs, fsr, cos_t, sin_t, np.array(depths)


def cloud_min_z(xyz: np.ndarray) -> np.float32:
    """pcl::getMinMax3D's min_bound(2) over the processed cloud (grasp_detector.cpp:152-153): the float
    minimum z of the finite points."""
    xyz = np.asarray(xyz, dtype=np.float32)
    ok = np.isfinite(xyz[:, :3]).all(axis=1)
    return np.float32(xyz[ok, 2].min()) if ok.any() else np.float32(np.inf)


def prune_corners(rec, prm):
    """The five points of GraspDetector::pruneGraspsOnHandParameters (grasp_detector.cpp:372-380), in
    float64: left / right bottom, left / right top (bottom or top +- half_width * binormal), and
    bottom - 0.10 * approach.  Returns 5 x 3."""
    hw = 0.5 * float(prm["hand_outer_diameter"])
    b, t = np.asarray(rec["bottom"], dtype=np.float64), np.asarray(rec["top"], dtype=np.float64)
    bn, ap = np.asarray(rec["binormal"], dtype=np.float64), np.asarray(rec["approach"], dtype=np.float64)
    return np.stack([b + hw * bn, b - hw * bn, t + hw * bn, t - hw * bn, b - 0.10 * ap])


def prune_keep(rec, prm, min_z) -> bool:
    """GraspDetector::pruneGraspsOnHandParameters (grasp_detector.cpp:363-395) for one record.
    :369 a record that is not half antipodal is dropped when filter_half_grasps is set; :383-387 the
    aperture bounds are inclusive (>= min_aperture, <= max_aperture, doubles); the workspace bounds
    and min_z are `float` parameters (:363-364: the double workspace_ narrows at the call, :154), the
    corner coordinates stay double and are compared against the widened floats, inclusively.
    min_z: cloud_min_z of the processed cloud (:152-154)."""
    if int(prm.get("filter_half_grasps", 0)) and not int(rec["half_antipodal"]):
        return False
    ws = prm["workspace"]
    min_x, max_x, min_y, max_y = (float(np.float32(ws[i])) for i in range(4))
    P = prune_corners(rec, prm)
    ap = float(rec["width"])
    return bool(ap >= float(prm["min_aperture"]) and ap <= float(prm["max_aperture"])
                and P[:, 2].min() >= float(np.float32(min_z))
                and P[:, 1].min() >= min_y and P[:, 1].max() <= max_y
                and P[:, 0].min() >= min_x and P[:, 0].max() <= max_x)


def finger_tables(od=0.09, fw=0.01):
    """FingerHand ctor, finger_hand.cpp:7-12."""
    fs_half = np.array([0.0 + i * ((od - fw) / 9.0) for i in range(10)])
    fs = np.concatenate([(fs_half - od) + fw, fs_half])
    return fs, fs + fw


def sweep_sample(P, Q, frame, sample, prm):
    """HandSearch::calculateHand (hand_search.cpp:319-426) for one sample, vectorised numpy.
    P, Q: K2 x 3 float64 centred points / normals (canonical order); frame: 3x3 [n b c] columns.
    Returns a list of dicts."""
    fw, od, depth, hh, bite, R = (prm["finger_width"], prm["hand_outer_diameter"], prm["hand_depth"],
                                  prm["hand_height"], prm["init_bite"], prm["num_orientations"])
    fs, fsr = finger_tables(od, fw)
    z = P @ frame[:, 2]
    keep = (z > -hh) & (z < hh)
    Pc, Qc = P[keep], Q[keep]
    out = []
    if Pc.shape[0] == 0:
        return out
    depths = []
    d = bite + 0.005
    while d <= depth:
        depths.append(d)
        d += 0.005
    for oi in range(R):
        a = -np.pi / 2 + oi * (np.pi / R)
        rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0, 0, 1.0]])
        Fr = frame @ rot
        X = Pc @ Fr
        Y = Qc @ Fr
        top, bottom = bite, bite - depth
        cset = X[:, 1] < top
        if not cset.any() or (X[cset, 1] < bottom).any():
            continue
        xc = X[cset, 0]
        free = np.array([not ((xc > fs[k]) & (xc < fsr[k])).any() for k in range(20)])
        if free.sum() <= 2:
            continue
        hand = free[:10] & free[10:]
        if hand.sum() == 0:
            continue
        valid = np.nonzero(hand)[0]
        idx = int(valid[int(np.ceil(len(valid) / 2.0)) - 1])
        for dd in depths:
            cs = X[:, 1] < dd
            if (X[cs, 1] < dd - depth).any():
                break
            xs = X[cs, 0]
            if ((xs > fs[idx]) & (xs < fsr[idx])).any() or ((xs > fs[10 + idx]) & (xs < fsr[10 + idx])).any():
                break
            top, bottom = dd, dd - depth
        left, right = fs[idx] + fw, fs[10 + idx]
        center = 0.5 * (left + right)
        surface = X[:, 1].min()
        box = (X[:, 1] < top) & (X[:, 0] > left) & (X[:, 0] < right)
        if not box.any():
            continue
        XB, YB = X[box], Y[box]
        width = XB[:, 0].max() - XB[:, 0].min()
        lc = left - 0.5 * (0.1 - (right - left))
        U = np.stack([(1.0 / 0.1) * (XB[:, 0] - lc), (1.0 / (top - bottom)) * (XB[:, 1] - bottom),
                      (1.0 / (2.0 * hh)) * (XB[:, 2] + hh)], axis=1)
        cosf = np.cos(30.0 * np.pi / 180.0)
        le = U[:, 0] < U[:, 0].min() + 0.003
        re = U[:, 0] > U[:, 0].max() - 0.003
        lv = le & (-YB[:, 0] > cosf)
        rv = re & (YB[:, 0] > cosf)
        label = 0
        if lv.any() or rv.any():
            label = 1
        if lv.any() and rv.any():
            ty = min(U[lv, 1].max(), U[rv, 1].max())
            by = max(U[lv, 1].min(), U[rv, 1].min())
            tz = min(U[lv, 2].max(), U[rv, 2].max())
            bz = max(U[lv, 2].min(), U[rv, 2].min())
            if ty > by and tz > bz:
                label = 2
        out.append(dict(
            orientation=oi, binormal=Fr[:, 0], approach=Fr[:, 1], axis=Fr[:, 2],
            surface=Fr @ np.array([center, surface, 0.0]) + sample,
            bottom=Fr @ np.array([center, bottom, 0.0]) + sample,
            top=Fr @ np.array([center, top, 0.0]) + sample,
            width=width, label=label, U=U, Y=YB))
    return out


def render_image(U: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """Learning::convertToImageRGB + convertTo(CV_8UC3,255) (learning.cpp:143-209, :16) with
    scipy's maximum_filter as the 3x3 dilate.  U, Y: P x 3."""
    from scipy.ndimage import maximum_filter
    S = 60
    y = U[:, 1] - U[:, 1].min()
    cs = 1.0 / S
    cell = np.floor(U[:, 0] / cs).astype(np.int64) + np.floor(y / cs).astype(np.int64) * S
    ok = (cell >= 0) & (cell < S * S)
    acc = np.zeros((S * S, 3))
    np.add.at(acc, cell[ok], Y[ok])  # sequential, in order
    cnt = np.bincount(cell[ok], minlength=S * S)
    img = np.zeros((S, S, 3), dtype=np.float32)
    c = np.nonzero(cnt)[0]
    a = acc[c]
    with np.errstate(all="ignore"):  # per cell, elementwise: the same operations as a loop over cells
        v = np.abs((1.0 / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]))[:, None] * a)
    v = np.where(np.isnan(v), 0.0, v)
    img[S - 1 - c // S, c % S] = v.astype(np.float32)
    dil = maximum_filter(img, size=(3, 3, 1), mode="constant", cval=0.0)
    rgb = dil[:, :, ::-1]
    t = rgb.astype(np.float32) * np.float32(255.0)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def lenet_torch(w: dict, images_hwc: np.ndarray) -> np.ndarray:
    """Caffe LeNet of caffe/test_1batch2.prototxt via torch CPU ops (fp32)."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(images_hwc.astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}
    with torch.no_grad():
        x = F.max_pool2d(F.conv2d(x, t["conv1_w"], t["conv1_b"]), 2)
        x = F.max_pool2d(F.conv2d(x, t["conv2_w"], t["conv2_b"]), 2)
        x = F.relu(F.linear(x.flatten(1), t["ip1_w"], t["ip1_b"]))
        x = F.linear(x, t["ip2_w"], t["ip2_b"])
    return x.numpy()


def _rot3(M, D, k):
    """(M[0][k] D0 + M[1][k] D1) + M[2][k] D2 over the rows of D: the oracle's association order
    (BLAS / @ would sum in another order and differ in the last bit)."""
    return (M[0, k] * D[:, 0] + M[1, k] * D[:, 1]) + M[2, k] * D[:, 2]


def antipodal_label(pts, nrm, thresh=0.003):
    """Antipodal::evaluateGrasp (antipodal.cpp:8-84) on unit-box points / rotated normals (P x 3)."""
    cos_fc = np.cos(30.0 * np.pi / 180.0)
    lt, rt = pts[:, 0].min() + thresh, pts[:, 0].max() - thresh
    lv = (((-1.0 * nrm[:, 0] + 0.0 * nrm[:, 1]) + 0.0 * nrm[:, 2]) > cos_fc) & (pts[:, 0] < lt)
    rv = (((1.0 * nrm[:, 0] + 0.0 * nrm[:, 1]) + 0.0 * nrm[:, 2]) > cos_fc) & (pts[:, 0] > rt)
    label = 1 if (lv.any() or rv.any()) else 0
    if lv.any() and rv.any():
        ty = min(pts[lv, 1].max(), pts[rv, 1].max())
        by = max(pts[lv, 1].min(), pts[rv, 1].min())
        tz = min(pts[lv, 2].max(), pts[rv, 2].max())
        bz = max(pts[lv, 2].min(), pts[rv, 2].min())
        if ty > by and tz > bz:
            label = 2
    return label


def sweep_sample_ordered(D, Q, F, sample, prm, tables):
    """sweep_sample restated with the oracle's operation order, so that its records are bit-equal
    to oracle/ag2_oracle.cpp's (sweep_sample) rather than close.
    D: K2 x 3 float64 centred radius neighbours, widened from float32 (canonical order); Q: their
    normals; F: 3x3 frame, columns [normal binormal curv]; sample: float64[3];
    tables: (fs, fsr, cos_t, sin_t, depths) as the oracle derives them.
    Returns (records, kcrop): each record a dict of the hypothesis fields plus pts / nrm (P x 3)."""
    fs, fsr, cos_t, sin_t, depths = tables
    fw, hh = prm["finger_width"], prm["hand_height"]
    zf = _rot3(F, D, 2)
    keep = (zf > -1.0 * hh) & (zf < hh)
    P, Qc = D[keep], Q[keep]
    out = []
    if P.shape[0] == 0:
        return out, 0
    for oi in range(len(cos_t)):
        cs, sn = cos_t[oi], sin_t[oi]
        rot = [[cs, -1.0 * sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]
        Fr = np.array([[(F[a, 0] * rot[0][b] + F[a, 1] * rot[1][b]) + F[a, 2] * rot[2][b]
                        for b in range(3)] for a in range(3)])
        X = np.stack([_rot3(Fr, P, k) for k in range(3)], axis=1)
        top, bottom = prm["init_bite"], prm["init_bite"] - prm["hand_depth"]
        below = X[:, 1] < top
        if not below.any() or (X[below, 1] < bottom).any():
            continue
        xb = X[below, 0]
        free = np.array([not ((xb > fs[k]) & (xb < fsr[k])).any() for k in range(20)])
        if not free.sum() > 2:
            continue
        valid = np.nonzero(free[:10] & free[10:])[0]
        if len(valid) == 0:
            continue
        idx = int(valid[int(np.ceil(len(valid) / 2.0)) - 1])
        for d in depths:
            t_, b_ = d, d - prm["hand_depth"]
            cs_ = X[:, 1] < t_
            xx = X[cs_, 0]
            if (X[cs_, 1] < b_).any() or (((xx > fs[idx]) & (xx < fsr[idx])) |
                                          ((xx > fs[10 + idx]) & (xx < fsr[10 + idx]))).any():
                break
            top, bottom = t_, b_
        left, right = fs[idx] + fw, fs[10 + idx]
        center = 0.5 * (left + right)
        surface = X[:, 1].min()
        box = np.nonzero((X[:, 1] < top) & (X[:, 0] > left) & (X[:, 0] < right))[0]
        if len(box) == 0:
            continue
        rec = dict(orientation=oi, binormal=Fr[:, 0].copy(), approach=Fr[:, 1].copy(),
                   axis=Fr[:, 2].copy())
        for name, yv in (("surface", surface), ("bottom", bottom), ("top", top)):
            rec[name] = np.array([((Fr[a, 0] * center + Fr[a, 1] * yv) + Fr[a, 2] * 0.0) + sample[a]
                                  for a in range(3)])
        XB = X[box]
        nrm = np.stack([_rot3(Fr, Qc[box], k) for k in range(3)], axis=1)
        rec["width"] = XB[:, 0].max() - XB[:, 0].min()
        lower = (left - 0.5 * (0.1 - (right - left)), bottom, -1.0 * hh)
        scales = (1.0 / 0.1, 1.0 / (top - bottom), 1.0 / (2.0 * hh))
        pts = np.stack([scales[a] * (XB[:, a] - lower[a]) for a in range(3)], axis=1)
        label = antipodal_label(pts, nrm)
        rec.update(half_antipodal=int(label >= 1), full_antipodal=int(label == 2),
                   n_points=len(box), pts=pts, nrm=nrm, hand=idx)
        out.append(rec)
    return out, int(P.shape[0])
