"""Two-camera clouds (CloudCamera(cloud, size_left), cloud_camera.cpp:34-51) and clouds that bring their normals
(cloud_camera.cpp:4-31) on the device and frame paths: ag2_set_cloud_desc, ag2_detect_frame_desc,
ag2_submit_frame_desc / ag2_wait_frame, ag2_pipe_submit_desc.

Bars (the project's own): the context state equals what ag2_set_cloud leaves for the explicit camera matrix, as bytes;
records equal the oracle's bit for bit apart from the score, scores within 1e-4 max|score| + 1e-3, the selection through
selection_check; a frame equals the step-by-step composition as bytes."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_params
from agile_grasp2_amd import scene
from agile_grasp2_amd.selection_check import check_selection
from agile_grasp2_amd.weights import make_lenet_weights

pytestmark = pytest.mark.gpu

CAMS = [scene.CAMERA, scene.CAMERA + np.array([0.0, 0.6, 0.1])]
REC_FIELDS = ("sample_slot", "orientation", "half_antipodal", "full_antipodal", "n_points", "axis",
              "approach", "binormal", "surface", "bottom", "top", "width")


def cam_matrix(n, size_left):
    """cloud_camera.cpp:34-51"""
    cam = np.zeros((2, n), dtype=np.int32)
    cam[0, :size_left] = 1
    cam[1, size_left:] = 1
    return cam


def records(xyz, nrm, floats):
    """n records of `floats` float32 each: xyz at 0, normals (when they fit) at float 4 -- floats = 12 is the 48-byte
    PointXYZRGBNormal; everything else is filled with a pattern no kernel may read as data"""
    rec = np.full((xyz.shape[0], floats), 1.0e30, dtype=np.float32)
    rec[:, :3] = xyz
    if nrm is not None and floats >= 7:
        rec[:, 4:7] = nrm
    return rec


class DeviceCopy:
    """host arrays copied into device memory for the length of a test"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptrs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        self.ptrs.append(p)
        return p.value

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def small_case():
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    n = xyz.shape[0]
    return xyz, ws, n, n // 3, scene.draw_samples(2, n, 100)


def flipped_normals(o):
    """the oracle's normals with the sign flipped on every third point, as the float32 a sensor record holds"""
    nrm = o.get_normals().T.astype(np.float32)
    nrm[::3] = -nrm[::3]
    return np.ascontiguousarray(nrm)


def oracle_for(ws, xyz, cam=None, normals=None, **kw):
    from oracle import api
    prm = dict(n_cams=2, cam_origin=CAMS) if cam is not None else {}
    prm.update(kw)
    o = api.Oracle(**scene_params(ws, num_threads=4, **prm))
    o.set_cloud(xyz, cam_source=cam, normals=None if normals is None else normals.T.astype(np.float64))
    if normals is None:
        o.compute_normals()
    return o


def desc_args(xyz, nrm, stride, nrm_mode, on_device, dev):
    """keyword arguments of capi.cloud_desc for one layout of the same cloud"""
    rec = records(xyz, nrm if nrm_mode == "interleaved" else None, stride // 4)
    sep = None
    if nrm_mode == "separate12":
        sep = np.ascontiguousarray(nrm)
    elif nrm_mode == "separate16":
        sep = records(nrm, None, 4)
    if not on_device:
        kw = dict(xyz=rec[:, :3])
        if nrm_mode == "interleaved":
            kw["normals"] = rec[:, 4:7]
        elif sep is not None:
            kw["normals"] = sep[:, :3]
        return kw
    dptr = dev.put(rec)
    kw = dict(dptr=dptr, n=xyz.shape[0], stride=stride)
    if nrm_mode == "interleaved":
        kw.update(normals_dptr=dptr + 16, normals_stride=stride)
    elif sep is not None:
        kw.update(normals_dptr=dev.put(sep), normals_stride=sep.strides[0])
    return kw


LAYOUTS = [(12, "none"), (16, "none"), (32, "none"), (48, "none"), (12, "separate12"), (16, "separate16"),
           (32, "separate12"), (32, "interleaved"), (48, "interleaved"), (48, "separate16")]


@pytest.mark.parametrize("on_device", [False, True])
def test_state_equals_set_cloud_with_the_explicit_matrix(on_device):
    from agile_grasp2_amd import capi
    xyz, ws, n, sl, idx = small_case()
    cam = cam_matrix(n, sl)
    nrm = flipped_normals(oracle_for(ws, xyz, cam))
    prm = scene_params(ws, n_cams=2, cam_origin=CAMS)
    dev = DeviceCopy()
    for stride, mode in LAYOUTS:
        d, r = capi.Detector(**prm), capi.Detector(**prm)
        given = None if mode == "none" else nrm
        d.set_cloud_desc(size_left=sl, **desc_args(xyz, given, stride, mode, on_device, dev))
        r.set_cloud(xyz, cam_source=cam, normals=None if given is None else given.T.astype(np.float64))
        tag = (stride, mode)
        gx, gc = d.get_cloud()
        rx, rc = r.get_cloud()
        assert gx.tobytes() == xyz.tobytes() == rx.tobytes(), tag
        assert gc.tobytes() == rc.tobytes() and np.array_equal(gc, cam), tag
        assert d.get_grid_perm().tobytes() == r.get_grid_perm().tobytes(), tag
        if given is None:
            d.compute_normals()
            r.compute_normals()
        assert d.get_normals().tobytes() == r.get_normals().tobytes(), tag
        if given is not None:
            assert np.array_equal(d.get_normals().T.astype(np.float32).view(np.uint32), given.view(np.uint32)), tag
        # ... and what is made from that state
        assert d.generate_hypotheses(sample_idx=idx, seed=1).tobytes() == \
            r.generate_hypotheses(sample_idx=idx, seed=1).tobytes(), tag
        d.close()
        r.close()
    dev.free()


def test_size_left_at_both_ends_and_an_empty_cloud():
    from agile_grasp2_amd import capi
    xyz, ws, n, _, idx = small_case()
    prm = scene_params(ws, n_cams=2, cam_origin=CAMS)
    d, r = capi.Detector(**prm), capi.Detector(**prm)
    for sl in (0, n, 1, n - 1):
        d.set_cloud_desc(xyz, size_left=sl)
        r.set_cloud(xyz, cam_source=cam_matrix(n, sl))
        assert d.get_cloud()[1].tobytes() == r.get_cloud()[1].tobytes(), sl
        for x in (d, r):
            x.compute_normals()
        assert d.generate_hypotheses(sample_idx=idx[:40], seed=2).tobytes() == \
            r.generate_hypotheses(sample_idx=idx[:40], seed=2).tobytes(), sl
    d.set_cloud_desc(np.zeros((0, 3), dtype=np.float32), size_left=0)
    assert d.counters().n_points == 0
    d.set_cloud_desc(xyz, size_left=5)   # the context is usable afterwards
    assert d.counters().n_points == n
    d.close()
    r.close()


def assert_records_equal_oracle(got, want, tag=""):
    assert len(got) == len(want) and len(want) > 0, (tag, len(got), len(want))
    for f in REC_FIELDS:
        assert np.array_equal(got[f], want[f]), (tag, f)
    # all 20 doubles of every record (axis ... width = 19, the score apart)
    assert got.view(np.uint8).reshape(len(got), -1)[:, :152].tobytes() == \
        want.view(np.uint8).reshape(len(want), -1)[:, :152].tobytes(), tag


def test_against_the_oracle_and_the_vote_and_the_normals_matter():
    from agile_grasp2_amd import capi
    xyz, ws, n, sl, idx = small_case()
    cam = cam_matrix(n, sl)
    # -- preconditions on the CPU: the camera vote and the given normals change the oracle's records --
    o_one = oracle_for(ws, xyz)
    o_two = oracle_for(ws, xyz, cam)
    h_one = o_one.generate_hypotheses(sample_idx=idx, seed=1)
    h_two = o_two.generate_hypotheses(sample_idx=idx, seed=1)
    assert h_one.tobytes() != h_two.tobytes(), "two cameras must change a record: pick another origin"
    nrm = flipped_normals(o_two)
    sel_prm = dict(min_score_diff=0.0, num_selected=10)
    o_nrm = oracle_for(ws, xyz, cam, normals=nrm, **sel_prm)
    h_nrm = o_nrm.generate_hypotheses(sample_idx=idx, seed=1)
    assert h_nrm.tobytes() != h_two.tobytes(), "the given normals must change a record"
    w = make_lenet_weights(7)
    o_nrm.lenet_load(w)
    o_sel, o_all = o_nrm.detect(sample_idx=idx, seed=1, do_prune=True)
    assert 0 < len(o_sel) < len(o_all), "the selection must be neither empty nor everything"
    assert int((o_all["score"] >= 0.0).sum()) > len(o_sel), "the top-k must cut as well"
    # -- two cameras, normals computed --
    prm = scene_params(ws, n_cams=2, cam_origin=CAMS, **sel_prm)
    d = capi.Detector(**prm)
    d.lenet_load(w)
    d.set_cloud_desc(records(xyz, None, 8)[:, :3], size_left=sl)
    d.compute_normals()
    assert_records_equal_oracle(d.generate_hypotheses(sample_idx=idx, seed=1), h_two, "two cameras")
    # -- two cameras, normals given (48-byte records, interleaved) --
    rec = records(xyz, nrm, 12)
    d.set_cloud_desc(rec[:, :3], size_left=sl, normals=rec[:, 4:7])
    assert_records_equal_oracle(d.generate_hypotheses(sample_idx=idx, seed=1), h_nrm, "given normals")
    g_sel, g_all = d.detect(sample_idx=idx, seed=1, do_prune=True)
    assert len(g_all) == len(o_all)
    for f in REC_FIELDS:
        assert np.array_equal(g_all[f], o_all[f]), f
    tol = 1e-4 * np.abs(o_all["score"]).max() + 1e-3
    err = np.abs(g_all["score"] - o_all["score"]).max()
    print(f"score error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    chk = check_selection(g_sel, o_all, 0.0, 10, tol, tag="sized cloud with normals")
    assert chk["selected"] > 0
    # -- and the same through a frame --
    f_sel, f_n = d.detect_frame_desc(rec[:, :3], idx, seed=1, size_left=sl, normals=rec[:, 4:7])
    assert f_n == len(o_all) and f_sel.tobytes() == g_sel.tobytes()
    d.close()


# ---- frames --------------------------------------------------------------------------------------------------

def _clouds(n_frames, n_target, n_samples):
    out = []
    for k in range(n_frames):
        xyz, ws = scene.make_scene(seed=10 + k, n_target=n_target + 137 * (k % 3))
        out.append((xyz, ws, scene.draw_samples(20 + k, xyz.shape[0], n_samples)))
    return out


def _size_left(k, n):
    return [n // 3, n, 0, n // 2, n // 4, 17, n - 1][k % 7]


def _pair(ws, n_cams=2, **kw):
    from agile_grasp2_amd import capi
    prm = scene_params(ws, **(dict(n_cams=2, cam_origin=CAMS) if n_cams == 2 else {}), **kw)
    w = make_lenet_weights(7)
    df, ds = capi.Detector(**prm), capi.Detector(**prm)
    for d in (df, ds):
        d.lenet_load(w)
    return df, ds


def _frame_normals(ds, xyz, cam):
    """normals for a frame: the computed ones, every third flipped (NaN where a point has too few neighbours)"""
    ds.set_cloud(xyz, cam_source=cam)
    ds.compute_normals()
    nrm = ds.get_normals().T.astype(np.float32)
    nrm[::3] = -nrm[::3]
    return np.ascontiguousarray(nrm)


def _compose(ds, xyz, sl, nrm, idx, seed, two=True, do_prune=True):
    """the composition a frame has to equal, through the host entry with the explicit matrix:
    ag2_set_cloud [+ ag2_compute_normals without given normals] + ag2_detect"""
    ds.set_cloud(xyz, cam_source=cam_matrix(len(xyz), sl) if two else None,
                 normals=None if nrm is None else nrm.T.astype(np.float64))
    if nrm is None:
        ds.compute_normals()
    return ds.detect(sample_idx=idx, seed=seed, do_prune=do_prune, want_all=False)


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("use_graph", [True, False])
def test_sized_frames_equal_the_composition(use_graph, given):
    frames = _clouds(7, 20000, 300)
    ws = frames[0][1]
    df, ds = _pair(ws, min_score_diff=-50.0, num_selected=40)
    df.stream_configure(0, 0, use_graph)
    total = 0
    for k, (xyz, _, idx) in enumerate(frames):
        n = len(xyz)
        sl = _size_left(k, n)
        nrm = _frame_normals(ds, xyz, cam_matrix(n, sl)) if given else None
        got, gn = df.detect_frame_desc(xyz, idx, seed=k, size_left=sl, normals=nrm)
        want, wn = _compose(ds, xyz, sl, nrm, idx, k)
        assert gn == wn and got.tobytes() == want.tobytes(), k
        total += len(want)
    assert total > 50
    assert df.get_cloud()[1].tobytes() == ds.get_cloud()[1].tobytes()
    assert df.get_normals().tobytes() == ds.get_normals().tobytes()
    fi = df.frame_info()
    assert fi.frames == 7 and fi.stepwise_runs >= 1
    if use_graph:
        assert fi.graph_replays > 0 and fi.captures >= 1 and fi.capture_failed == 0
    else:
        assert fi.captures == 0 and fi.graph_replays == 0 and fi.plain_runs > 0
    df.close()
    ds.close()


def test_the_camera_split_reaches_a_replayed_frame():
    """size_left is not frozen into the graph: the same cloud replayed with another split gives the other split's
    records (and they differ)."""
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    n = len(xyz)
    idx = scene.draw_samples(2, n, 100)
    df, ds = _pair(ws, min_score_diff=-1e30, num_selected=-1)
    outs = []
    for k, sl in enumerate([n // 3, n // 3, n, n // 3, 0]):
        got, gn = df.detect_frame_desc(xyz, idx, seed=1, size_left=sl, do_prune=False)
        want, wn = _compose(ds, xyz, sl, None, idx, 1, do_prune=False)
        assert gn == wn and got.tobytes() == want.tobytes(), k
        outs.append(got.tobytes())
    assert outs[2] != outs[1] and outs[3] == outs[1]
    assert df.frame_info().graph_replays >= 2
    df.close()
    ds.close()


def test_a_frame_that_outgrows_the_shapes_and_a_flavour_switch():
    small = _clouds(3, 8000, 100)
    big_xyz, _ = scene.make_scene(seed=77, n_target=30000)
    big = (big_xyz, None, scene.draw_samples(5, len(big_xyz), 250))
    ws = small[0][1]
    df, ds = _pair(ws, min_score_diff=-1e30, num_selected=25)
    df.stream_configure(max_points=len(small[0][0]) + 2000, max_samples=0, use_graph=True)

    def run(seq, given, k0):
        for k, (xyz, _, idx) in enumerate(seq):
            n = len(xyz)
            sl = _size_left(k0 + k, n)
            nrm = _frame_normals(ds, xyz, cam_matrix(n, sl)) if given else None
            got, gn = df.detect_frame_desc(xyz, idx, seed=k0 + k, size_left=sl, normals=nrm)
            want, wn = _compose(ds, xyz, sl, nrm, idx, k0 + k)
            assert gn == wn and got.tobytes() == want.tobytes(), (given, k)

    run([small[0], small[1], small[2], big, small[0], big, small[1]], True, 0)
    fi = df.frame_info()
    assert fi.stepwise_runs == 2          # the first frame and the first big one (more points than max_points)
    assert fi.captures == 2 and fi.graph_replays >= 2
    assert fi.max_points >= len(big_xyz) and fi.max_samples == 250
    # the frames stop bringing normals: shapes learned again, ONE more capture, replays again; and back
    before = fi
    run([small[0], small[1], small[2], small[0]], False, 7)
    fi = df.frame_info()
    assert fi.captures == before.captures + 1 and fi.stepwise_runs == before.stepwise_runs + 1
    assert fi.graph_replays >= before.graph_replays + 2
    before = fi
    run([small[1], small[2], small[0]], True, 11)
    fi = df.frame_info()
    assert fi.captures == before.captures + 1 and fi.graph_replays >= before.graph_replays + 1
    df.close()
    ds.close()


def test_sized_frames_with_grasp_clusters():
    frames = _clouds(5, 20000, 300)
    ws = frames[0][1]
    df, ds = _pair(ws, min_score_diff=-1e30, num_selected=40)
    for d in (df, ds):
        d.set_min_inliers(3)
    total = 0
    for k, (xyz, _, idx) in enumerate(frames):
        n = len(xyz)
        sl = _size_left(k, n)
        nrm = _frame_normals(ds, xyz, cam_matrix(n, sl))
        got, gn = df.detect_frame_desc(xyz, idx, seed=k, size_left=sl, normals=nrm)
        want, wn = _compose(ds, xyz, sl, nrm, idx, k)
        assert gn == wn and got.tobytes() == want.tobytes(), k
        total += len(want)
    assert total > 0
    assert df.frame_info().graph_replays > 0
    df.close()
    ds.close()


def test_device_resident_records_with_interleaved_normals_submit_and_wait():
    """48-byte PointXYZRGBNormal records in device memory through ag2_submit_frame_desc / ag2_wait_frame; a second
    submit before the wait is refused (AG2_ERR_STATE) and harms nothing."""
    frames = _clouds(7, 15000, 200)
    ws = frames[0][1]
    df, ds = _pair(ws, min_score_diff=-1e30, num_selected=30)
    dev = DeviceCopy()
    for k, (xyz, _, idx) in enumerate(frames):
        n = len(xyz)
        sl = _size_left(k, n)
        nrm = _frame_normals(ds, xyz, cam_matrix(n, sl))
        dptr = dev.put(records(xyz, nrm, 12))
        kw = dict(dptr=dptr, n=n, stride=48, normals_dptr=dptr + 16, normals_stride=48)
        df.submit_frame_desc(sample_idx=idx, seed=k, size_left=sl, **kw)
        if k == 3:
            with pytest.raises(RuntimeError, match="in flight"):
                df.submit_frame_desc(sample_idx=idx, seed=k, size_left=sl, **kw)
        want, wn = _compose(ds, xyz, sl, nrm, idx, k)   # (while the frame runs)
        got, gn = df.wait_frame()
        assert gn == wn and got.tobytes() == want.tobytes(), k
    assert df.frame_info().graph_replays > 0
    dev.free()
    df.close()
    ds.close()


def test_a_depth_two_pipe_returns_sized_frames_in_submission_order():
    from agile_grasp2_amd import capi
    frames = _clouds(8, 15000, 200)
    ws = frames[0][1]
    prm = scene_params(ws, n_cams=2, cam_origin=CAMS, min_score_diff=-1e30, num_selected=30)
    w = make_lenet_weights(7)
    pipe = capi.Pipe(depth=2, **prm)
    pipe.lenet_load(w)
    ds = capi.Detector(**prm)
    ds.lenet_load(w)
    wants, jobs = [], []
    for k, (xyz, _, idx) in enumerate(frames):
        n = len(xyz)
        sl = _size_left(k, n)
        nrm = _frame_normals(ds, xyz, cam_matrix(n, sl)) if k % 2 == 0 or k > 4 else None
        jobs.append((xyz, idx, sl, nrm))
        wants.append(_compose(ds, xyz, sl, nrm, idx, k))
    got = []
    for k, (xyz, idx, sl, nrm) in enumerate(jobs):
        if k >= 2:
            got.append(pipe.wait())
        pipe.submit_desc(xyz, idx, seed=k, size_left=sl, normals=nrm)
    got.append(pipe.wait())
    got.append(pipe.wait())
    for k, ((sel, n_scored, _), (want, wn)) in enumerate(zip(got, wants)):
        assert n_scored == wn and sel.tobytes() == want.tobytes(), k
    pipe.close()
    ds.close()


def test_one_camera_frames_without_normals_take_todays_path():
    """The same stream through ag2_detect_frame_desc and through ag2_detect_frame: identical bytes, identical
    ag2_frame_info."""
    from agile_grasp2_amd import capi
    frames = _clouds(7, 20000, 300)
    ws = frames[0][1]
    df, d0 = _pair(ws, n_cams=1, min_score_diff=-50.0, num_selected=40)
    for k, (xyz, _, idx) in enumerate(frames):
        got, gn = df.detect_frame_desc(xyz, idx, seed=k)
        want, wn = d0.detect_frame(xyz, idx, seed=k)
        assert gn == wn and got.tobytes() == want.tobytes(), k
    fa, fb = df.frame_info(), d0.frame_info()
    for name, _ in capi.FrameInfo._fields_:
        assert getattr(fa, name) == getattr(fb, name), name
    assert fa.graph_replays == 5 and fa.captures == 1
    df.close()
    d0.close()


def test_the_older_entries_still_refuse_a_two_camera_context():
    frames = _clouds(1, 8000, 50)
    xyz, ws, idx = frames[0]
    df, ds = _pair(ws)
    with pytest.raises(RuntimeError, match="single-camera"):
        df.detect_frame(xyz, idx, seed=0)
    with pytest.raises(RuntimeError, match="single-camera"):
        df.detect_frame_raw(xyz, num_samples=50)
    got, gn = df.detect_frame_desc(xyz, idx, seed=0, size_left=100)
    want, wn = _compose(ds, xyz, 100, None, idx, 0)
    assert gn == wn and got.tobytes() == want.tobytes()
    df.close()
    ds.close()
