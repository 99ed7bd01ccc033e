"""ImportanceSampling::detectGraspPoses on the device (ag2_detect_importance, importance_sampling.cpp:30-118).

1. the sampler equals a restatement of the host loop's draw (integers through np_reference.draw_u64, glibc
   log / cos / sqrt / exp through math): picks, decisions, tried counts and random indices equal, Gaussian
   samples within 4 ulp (the device's math library is the only allowed difference);
2. the whole call equals, byte for byte, ag2_detect(indices) ++ ag2_detect(round k's samples) ... then
   ag2_find_clusters when min_inliers > 0, in both of its forms (step by step, one trip);
3. the oracle, fed the device's rounds, returns the same hands per round;
4. from the second call on a context the call waits for the device once;
5. edge cases: no hand from the initial detect, a short output buffer, the 10^6-candidate guard;
6. the C++ mirror's opt-in (ImportanceSampling::setSampleOnDevice).
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import scene_params
from np_reference import draw_u64
from agile_grasp2_amd import capi
from agile_grasp2_amd.weights import make_lenet_weights, save_ag2w

STREAM0 = 0xFFFFFFFFFFFF0000
U53 = 1.0 / 9007199254740992.0
ROUNDS, SAMPLES = 3, 40


def restate_round(surf, cloud, seed, it, num_samples, prob_rand, radius, method, max_tried=1000000):
    """The host loop of one round (ag2_host.cpp, ImportanceSampling::detectGraspPoses) in Python.
    surf: h x 3 hand surfaces, cloud: n x 3 float32.  Returns (3 x S samples, tried, accepted, random indices)."""
    stream = STREAM0 + it
    num_rand = int(prob_rand * num_samples)
    ng = num_samples - num_rand
    sigma = radius
    term = 1.0 / math.sqrt(math.pow(2.0 * math.pi, 3.0) * math.pow(sigma, 3.0))
    coef = -1.0 / (2.0 * sigma)
    out = np.zeros((3, num_samples))
    sl = [tuple(float(v) for v in s) for s in surf]

    def dens(x, s):
        d0, d1, d2 = x[0] - s[0], x[1] - s[1], x[2] - s[2]
        return term * math.exp(coef * ((d0 * d0 + d1 * d1) + d2 * d2))

    j = tried = 0
    while j < ng and tried < max_tried:
        ctr = 7 * tried
        tried += 1
        idx = draw_u64(seed, stream, ctr) % len(sl)
        x = []
        for k in range(3):
            u1 = ((draw_u64(seed, stream, ctr + 1 + 2 * k) >> 11) + 1) * U53
            u2 = (draw_u64(seed, stream, ctr + 2 + 2 * k) >> 11) * U53
            g = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
            x.append(sl[idx][k] + g * sigma)
        accept = True
        if method == capi.IS_MAX:
            maxp = 0.0
            for s in sl:
                p = dens(x, s)
                maxp = p if maxp < p else maxp
            accept = dens(x, sl[idx]) >= maxp
        if accept:
            out[:, j] = x
            j += 1
    ridx = [draw_u64(seed, stream, 7 * tried + (q - ng)) % len(cloud) for q in range(ng, num_samples)]
    for q, r in zip(range(ng, num_samples), ridx):
        out[:, q] = cloud[r].astype(np.float64)
    return out, tried, j, ridx


def assert_ulp(got, want, ulps=4):
    scale = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert np.all(np.abs(got - want) <= ulps * scale), np.abs(got - want).max()


def make_detector(ws, xyz, **kw):
    d = capi.Detector(**scene_params(ws, **dict(dict(min_score_diff=-1e30, num_selected=50), **kw)))
    d.set_cloud(xyz)
    d.compute_normals()
    d.lenet_load(make_lenet_weights(7))
    return d


def composition(d, idx, rounds, seed, do_prune, min_inliers, n_resident=None):
    """ag2_detect(indices) ++ ag2_detect(round k) ... [ag2_find_clusters]: (hands, per-detect lists)"""
    d.set_min_inliers(0)
    parts = [d.detect(sample_idx=idx, seed=seed, do_prune=do_prune, want_all=False, n_resident=n_resident)[0]]
    if len(parts[0]):
        parts += [d.detect(sample_xyz=r, seed=seed, do_prune=do_prune, want_all=False)[0] for r in rounds]
    hands = np.concatenate(parts)
    if min_inliers > 0 and len(hands):
        hands = d.find_clusters(hands, min_inliers)
    d.set_min_inliers(min_inliers)
    return hands, parts


def with_nonfinite(xyz):
    x = xyz.copy()
    x[::97] = np.nan
    x[5::211, 1] = np.inf
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("min_inliers,do_prune,nonfinite", [(0, True, False), (5, True, False), (0, False, False),
                                                            (5, False, True)])
def test_importance_equals_composition(small_scene, min_inliers, do_prune, nonfinite):
    xyz, ws, idx = small_scene
    cloud = with_nonfinite(xyz) if nonfinite else xyz
    d = make_detector(ws, cloud)
    d.set_min_inliers(min_inliers)
    for call in range(2):  # the first call runs step by step, the second in one trip
        seed = 11 + call
        hands, rounds = d.detect_importance(sample_idx=idx, seed=seed, do_prune=do_prune, num_iterations=ROUNDS,
                                            num_samples=SAMPLES)
        info = d.importance_info()
        cnt, times = d.counters(), d.times()
        assert info.one_trip == call and info.redone == 0
        assert len(rounds) == ROUNDS and info.rounds == ROUNDS and info.n_initial > 0
        want, parts = composition(d, idx, rounds, seed, do_prune, min_inliers)
        assert info.n_initial == len(parts[0]) and info.n_hands == sum(len(p) for p in parts)
        assert hands.tobytes() == want.tobytes()
        assert sum(len(p) for p in parts[1:]) > 0
        # counters and stage times describe the call's last detect, in both forms
        assert cnt.n_samples == SAMPLES and cnt.n_selected == len(parts[-1]) and times.total_ms > 0.0


@pytest.mark.gpu
def test_importance_on_resident_indices(small_scene):
    """sample_idx == NULL: the indices ag2_subsample_uniformly left on the device, in both forms (the queued form
    must fetch them for the initial detect, not take the query points a previous call left)."""
    xyz, ws, _ = small_scene
    d = make_detector(ws, xyz)
    n = d.subsample_uniformly(100, seed=5, want_indices=False)
    for call in range(3):
        seed = 21 + call
        hands, rounds = d.detect_importance(n_resident=n, seed=seed, num_iterations=ROUNDS, num_samples=SAMPLES)
        info = d.importance_info()
        assert info.one_trip == (call > 0) and info.redone == 0 and info.n_initial > 0
        want, parts = composition(d, None, rounds, seed, True, 0, n_resident=n)
        assert info.n_initial == len(parts[0])
        assert hands.tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [capi.IS_MAX, capi.IS_SUM])
@pytest.mark.parametrize("radius", [0.02, 0.002])
def test_sampler_matches_host_loop(small_scene, method, radius):
    """Every round of the call, restated from the hands the composition found before it."""
    xyz, ws, idx = small_scene
    d = make_detector(ws, xyz)
    for seed in (3, 8):
        for call in range(2):
            hands, rounds = d.detect_importance(sample_idx=idx, seed=seed, num_iterations=ROUNDS, num_samples=SAMPLES,
                                                radius=radius, method=method)
            info = d.importance_info()
            _, parts = composition(d, idx, rounds, seed, True, 0)
            for it, r in enumerate(rounds):
                surf = np.concatenate(parts[: it + 1])["surface"]
                want, tried, acc, ridx = restate_round(surf, xyz, seed, it, SAMPLES, 0.3, radius, method)
                assert info.tried[it] == tried and info.accepted[it] == acc, (it, info.tried[it], tried)
                ng = SAMPLES - int(0.3 * SAMPLES)
                assert_ulp(r[:, :ng], want[:, :ng])
                assert np.array_equal(r[:, ng:], want[:, ng:])  # the same cloud points, exactly


@pytest.mark.gpu
def test_sampler_where_max_rejects_most(small_scene):
    """Many hands packed within a few millimetres: MAX keeps a small share of the candidates."""
    xyz, ws, _ = small_scene
    d = make_detector(ws, xyz)
    rng = np.random.default_rng(4)
    surf = (xyz[rng.choice(len(xyz), 1, replace=False)][0] + rng.normal(0, 0.003, size=(120, 3))).T
    for seed, it in ((1, 0), (2, 4)):
        got, tried, acc = d.importance_sample(surf, it, seed=seed, num_samples=30, method=capi.IS_MAX)
        want, t2, a2, _ = restate_round(surf.T, xyz, seed, it, 30, 0.3, 0.02, capi.IS_MAX)
        assert (tried, acc) == (t2, a2) and tried > 5 * acc
        assert_ulp(got[:, :21], want[:, :21])
        assert np.array_equal(got[:, 21:], want[:, 21:])


@pytest.mark.gpu
def test_sampler_guard(small_scene):
    """More Gaussian samples than the 10^6-candidate guard admits (SUM keeps every candidate): 10^6 tried, the
    slots left unfilled are (0, 0, 0), the random samples read the counters after the last candidate."""
    xyz, ws, _ = small_scene
    d = make_detector(ws, xyz)
    surf = xyz[:3].T.astype(np.float64)
    S, prob = 1000005, 2.5e-6
    ng = S - int(prob * S)
    got, tried, acc = d.importance_sample(surf, 2, seed=7, num_samples=S, prob_rand_samples=prob, method=capi.IS_SUM)
    assert (tried, acc) == (1000000, 1000000) and ng == 1000003
    assert np.all(got[:, 1000000:ng] == 0.0)
    head, _, _, _ = restate_round(surf.T, xyz, 7, 2, 50, 0.0, 0.02, capi.IS_SUM)  # candidates 0 .. 49
    assert_ulp(got[:, :50], head)
    stream = STREAM0 + 2
    for q in range(ng, S):
        r = draw_u64(7, stream, 7 * 1000000 + (q - ng)) % len(xyz)
        assert np.array_equal(got[:, q], xyz[r].astype(np.float64))


@pytest.mark.gpu
def test_importance_matches_oracle(small_scene):
    from oracle import api
    xyz, ws, idx = small_scene
    seed = 9
    d = make_detector(ws, xyz, num_selected=1000)
    for _ in range(2):
        hands, rounds = d.detect_importance(sample_idx=idx, seed=seed, num_iterations=ROUNDS, num_samples=SAMPLES)
    o = api.Oracle(**scene_params(ws, min_score_diff=-1e30, num_selected=1000, num_threads=4))
    o.set_cloud(xyz)
    o.compute_normals()
    o.lenet_load(make_lenet_weights(7))
    want = [o.detect(sample_idx=idx, seed=seed)[0]] + [o.detect(sample_xyz=m, seed=seed)[0] for m in rounds]
    assert sum(len(x) for x in want) == len(hands) and sum(len(x) for x in want[1:]) > 0
    tol = 1e-4 * max(np.abs(x["score"]).max() for x in want if len(x)) + 2e-3
    pos = 0
    for x in want:  # per round: the same hands, bit-equal poses, scores within the fp32 tolerance
        got = hands[pos: pos + len(x)]
        pos += len(x)
        kg = np.lexsort((got["orientation"], got["sample_slot"]))
        kw = np.lexsort((x["orientation"], x["sample_slot"]))
        for f in ("sample_slot", "orientation", "bottom", "surface", "axis", "width"):
            assert np.array_equal(got[f][kg], x[f][kw]), f
        assert np.abs(got["score"][kg] - x["score"][kw]).max() <= tol


@pytest.mark.gpu
def test_one_trip_at_launch_file_setting(small_scene):
    """launch/file_importance_sampling.launch: 100 initial samples, 5 x 50, MAX, min_inliers 5."""
    xyz, ws, idx = small_scene
    d = make_detector(ws, xyz)
    d.set_min_inliers(5)
    first, r1 = d.detect_importance(sample_idx=idx[:100], seed=4)
    i1 = d.importance_info()
    assert i1.one_trip == 0 and i1.host_syncs > 1
    second, r2 = d.detect_importance(sample_idx=idx[:100], seed=4)
    i2 = d.importance_info()
    assert i2.host_syncs == 1 and i2.one_trip == 1 and i2.redone == 0
    assert first.tobytes() == second.tobytes() and len(r2) == 5
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2))
    assert list(i1.tried)[:5] == list(i2.tried)[:5] and list(i1.accepted)[:5] == list(i2.accepted)[:5]


@pytest.mark.gpu
def test_no_initial_hand(small_scene):
    xyz, ws, idx = small_scene
    d = make_detector(ws, xyz, min_score_diff=1e30)
    for call in range(2):
        hands, rounds = d.detect_importance(sample_idx=idx, seed=2)
        info = d.importance_info()
        assert len(hands) == 0 and rounds == [] and info.n_initial == 0 and info.rounds == 0
    assert info.one_trip == 1 and info.host_syncs == 1
    assert d.counters().n_frames == 0   # the queued rounds had no valid query point


@pytest.mark.gpu
def test_max_hand_bound(small_scene):
    """MAX evaluates every hand per candidate: more than AG2_IMPORTANCE_MAX_HANDS are refused; SUM takes them."""
    xyz, ws, _ = small_scene
    d = make_detector(ws, xyz)
    surf = np.repeat(xyz[:1].T.astype(np.float64), capi.IMPORTANCE_MAX_HANDS + 1, axis=1)
    with pytest.raises(RuntimeError, match="rc=-3"):
        d.importance_sample(surf, 0, seed=1, num_samples=10, method=capi.IS_MAX)
    got, tried, acc = d.importance_sample(surf, 0, seed=1, num_samples=10, method=capi.IS_SUM)
    assert (tried, acc) == (7, 7)
    got, tried, acc = d.importance_sample(surf[:, :capi.IMPORTANCE_MAX_HANDS], 0, seed=1, num_samples=10,
                                          method=capi.IS_MAX)
    assert acc == 7   # (identical surfaces tie: every candidate is kept)


@pytest.mark.gpu
def test_short_output_buffer(small_scene):
    xyz, ws, idx = small_scene
    d = make_detector(ws, xyz)
    ip = capi.default_importance_params(num_iterations=2, num_samples=30)
    out = np.zeros(1, dtype=capi.HYP_DTYPE)
    n = C.c_size_t(0)
    si = np.ascontiguousarray(idx, dtype=np.int32)
    rc = d.L.ag2_detect_importance(d.h, si.ctypes.data_as(C.c_void_p), C.c_size_t(len(si)), C.c_uint64(6), C.c_int(1),
                                   C.byref(ip), out.ctypes.data_as(C.c_void_p), C.c_size_t(1), C.byref(n))
    assert rc == -3 and n.value > 1   # AG2_ERR_CAPACITY, with the size needed
    hands, rounds = d.detect_importance(sample_idx=idx, seed=6, params=ip, cap=n.value)
    assert len(hands) == n.value
    want, _ = composition(d, idx, rounds, 6, True, 0)
    assert hands.tobytes() == want.tobytes()


def _read_driver_out(path):
    buf = open(path, "rb").read()
    n0, nr = struct.unpack_from("<qq", buf, 0)
    off = 16
    rounds = []
    for _ in range(nr):
        (s,) = struct.unpack_from("<q", buf, off)
        off += 8
        rounds.append(np.frombuffer(buf, dtype="<f8", count=3 * s, offset=off).reshape(s, 3).T.copy())
        off += 24 * s
    (nh,) = struct.unpack_from("<q", buf, off)
    off += 8
    rec = np.frombuffer(buf, dtype=np.dtype([("slot", "<i4"), ("orient", "<i4"), ("v", "<f8", 11)]), count=nh,
                        offset=off)
    return n0, rounds, rec


@pytest.mark.gpu
@pytest.mark.parametrize("min_inliers", [0, 5])
def test_cpp_sample_on_device(tmp_path, small_scene, min_inliers):
    from test_cpp_host import params_text
    from test_importance_abi import build_importance_driver
    tmp = str(tmp_path)
    exe = build_importance_driver(tmp)
    xyz, ws, idx = small_scene
    w = make_lenet_weights(7)
    wpath, lpath = os.path.join(tmp, "w.ag2w"), os.path.join(tmp, "labels.txt")
    save_ag2w(wpath, w)
    open(lpath, "w").write("0\n1\n")
    xyz.astype("<f4").tofile(os.path.join(tmp, "cloud.f32"))
    idx.astype("<i4").tofile(os.path.join(tmp, "idx.i32"))
    seed = 9
    open(os.path.join(tmp, "params.txt"), "w").write(params_text(ws, wpath, lpath, seed))
    outs = {}
    for dev in ("0", "1"):
        outp = os.path.join(tmp, f"out{dev}.bin")
        r = subprocess.run([exe, os.path.join(tmp, "cloud.f32"), os.path.join(tmp, "idx.i32"),
                            os.path.join(tmp, "params.txt"), dev, str(min_inliers), outp],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[dev] = _read_driver_out(outp)
    n0, rounds, rec = outs["1"]
    assert n0 > 0 and len(rounds) == ROUNDS
    # the same hands as the composition run on its own lastSampleRounds()
    d = capi.Detector(**scene_params(ws, min_score_diff=-1e30, num_selected=1000))
    d.set_cloud(xyz)
    d.compute_normals()
    d.lenet_load(w)
    want, parts = composition(d, idx, rounds, seed, True, min_inliers)
    assert len(parts[0]) == n0 and len(rec) == len(want)
    assert np.array_equal(rec["slot"], want["sample_slot"]) and np.array_equal(rec["orient"], want["orientation"])
    v = np.concatenate([want["score"][:, None], want["bottom"], want["surface"], want["axis"], want["width"][:, None]],
                       axis=1)
    assert rec["v"].tobytes() == np.ascontiguousarray(v).tobytes()
    # the host loop (default) draws the same rounds up to the last ulp of the device's math library
    n0h, rounds_h, rec_h = outs["0"]
    assert n0h == n0 and len(rounds_h) == ROUNDS
    assert_ulp(rounds_h[0], rounds[0])
