"""Argument checks of the cloud-description entries (ag2_set_cloud_desc, ag2_detect_frame_desc,
ag2_submit_frame_desc, ag2_pipe_submit_desc): every error returns AG2_ERR_ARG with a message and leaves the context
usable.  What needs no context runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import scene_params
from agile_grasp2_amd import capi, scene

ERR_ARG = -1
NEW = ["ag2_set_cloud_desc", "ag2_detect_frame_desc", "ag2_submit_frame_desc", "ag2_pipe_submit_desc"]


def test_the_new_entries_are_declared_exported_and_bound():
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    exported = entry.exported_symbols(capi.LIB_PATH)
    for s in NEW:
        assert s in declared and s in exported and s in capi.SYMBOLS, s
    text = open(os.path.join(entry.ROOT, "include", "ag2_c.h")).read()
    assert "#define AG2_ABI_VERSION 1" in text and "typedef struct ag2_cloud_desc" in text


def test_the_binding_lays_the_description_out_as_the_header_does():
    # const void*, size_t, size_t, int (+ padding), size_t, const void*, size_t on an LP64 target
    assert C.sizeof(capi.CloudDesc) == 56
    assert [getattr(capi.CloudDesc, f).offset for f, _ in capi.CloudDesc._fields_] == [0, 8, 16, 24, 32, 40, 48]


def test_a_null_context_or_pipe_is_an_argument_error():
    L = capi.load()
    d, _ = capi.cloud_desc(np.zeros((4, 3), dtype=np.float32))
    ns, na = C.c_size_t(0), C.c_size_t(0)
    assert L.ag2_set_cloud_desc(None, C.byref(d)) == ERR_ARG
    assert L.ag2_detect_frame_desc(None, C.byref(d), None, C.c_size_t(0), C.c_uint64(0), C.c_int(1), None,
                                   C.c_size_t(0), C.byref(ns), C.byref(na)) == ERR_ARG
    assert L.ag2_submit_frame_desc(None, C.byref(d), None, C.c_size_t(0), C.c_uint64(0), C.c_int(1)) == ERR_ARG
    assert L.ag2_pipe_submit_desc(None, C.byref(d), None, C.c_size_t(0), C.c_uint64(0), C.c_int(1)) == ERR_ARG


def _calls(det, idx):
    """the three context entries as functions of a description: each returns the C return code"""
    L = det.L
    si = np.ascontiguousarray(idx, dtype=np.int32)
    sel = np.zeros(len(si) * 8, dtype=capi.HYP_DTYPE)
    ns, na = C.c_size_t(0), C.c_size_t(0)
    p = lambda d: None if d is None else C.byref(d)  # noqa: E731
    return {
        "set_cloud_desc": lambda d: L.ag2_set_cloud_desc(det.h, p(d)),
        "detect_frame_desc": lambda d: L.ag2_detect_frame_desc(
            det.h, p(d), si.ctypes.data_as(C.c_void_p), C.c_size_t(len(si)), C.c_uint64(1), C.c_int(1),
            sel.ctypes.data_as(C.c_void_p), C.c_size_t(len(sel)), C.byref(ns), C.byref(na)),
        "submit_frame_desc": lambda d: L.ag2_submit_frame_desc(
            det.h, p(d), si.ctypes.data_as(C.c_void_p), C.c_size_t(len(si)), C.c_uint64(1), C.c_int(1)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("n_cams", [1, 2])
def test_every_argument_error_is_reported_and_the_context_stays_usable(n_cams):
    from agile_grasp2_amd.weights import make_lenet_weights
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    n = len(xyz)
    idx = scene.draw_samples(2, n, 40)
    nrm = np.zeros((n, 3), dtype=np.float32)
    nrm[:, 2] = 1.0
    cams = [scene.CAMERA, scene.CAMERA + np.array([0.0, 0.6, 0.1])]
    prm = scene_params(ws, min_score_diff=-1e30, **(dict(n_cams=2, cam_origin=cams) if n_cams == 2 else {}))
    det = capi.Detector(**prm)
    det.lenet_load(make_lenet_weights(7))
    good_sl = n // 3 if n_cams == 2 else n

    def desc(**kw):
        d, keep = capi.cloud_desc(xyz, good_sl, nrm)
        for k, v in kw.items():
            setattr(d, k, v)
        return d, keep

    bad = {
        "size_left > n": desc(size_left=n + 1),
        "normals stride under 12": desc(normals_stride_bytes=8),
        "normals stride not a multiple of 4": desc(normals_stride_bytes=14),
        "xyz NULL with n > 0": desc(xyz=None),
        "xyz stride under 12": desc(stride_bytes=8),
        "NULL description": (None, None),
    }
    if n_cams == 1:
        bad["size_left != n on a one-camera context"] = desc(size_left=n - 1)
    for name, call in _calls(det, idx).items():
        for what, (d, _) in bad.items():
            assert call(d) == ERR_ARG, (name, what)
            assert len(det.L.ag2_last_error(det.h)) > 0, (name, what)
        # ... and the context goes on working
        want = None
        for rep in range(2):
            got, _ = det.detect_frame_desc(xyz, idx, seed=1, size_left=good_sl, normals=nrm)
            assert len(got) > 0
            want = got if want is None else want
            assert got.tobytes() == want.tobytes(), name
    det.close()
