"""C++ host mirror: GraspDetector::detectGraspPosesInFrame(cloud, size_left_cloud) for PointXYZRGBA and
PointXYZRGBNormal clouds (tests/cpp/sized_frames.cpp) equals CloudCamera(cloud, size_left) + setSampleIndices +
detectGraspPoses, record for record as bytes.

not-gpu: the driver compiles and links against the headers and reports its usage.
gpu: it runs on the small two-camera scene."""
import os
import subprocess

import numpy as np
import pytest

from agile_grasp2_amd import scene
from agile_grasp2_amd.weights import make_lenet_weights, save_ag2w
from test_cpp_host import CSRC_DIR, HOST_DIR, ROOT, params_text


def build_driver(tmp):
    subprocess.check_call(["make", "-C", CSRC_DIR, "-s", "-j", "8"])
    subprocess.check_call(["make", "-C", HOST_DIR, "-s"])
    exe = os.path.join(tmp, "sized_frames")
    subprocess.check_call([
        "g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "sized_frames.cpp"), "-o", exe,
        "-L", HOST_DIR, "-lag2host", "-L", CSRC_DIR, "-lag2hip",
        f"-Wl,-rpath,{HOST_DIR}", f"-Wl,-rpath,{CSRC_DIR}"])
    return exe


def test_the_driver_builds_against_the_mirror(tmp_path):
    exe = build_driver(str(tmp_path))
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(HOST_DIR, "libag2host.so")], text=True)
    assert out.count("GraspDetector::detectGraspPosesInFrame(") == 3   # the raw overload and the two sized ones
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr   # nothing touched the GPU


@pytest.mark.gpu
def test_the_sized_overloads_equal_the_three_calls(tmp_path):
    from conftest import scene_params
    from oracle import api
    tmp = str(tmp_path)
    exe = build_driver(tmp)
    xyz, ws = scene.make_scene(seed=12, n_target=5000, kind="objects")
    n = len(xyz)
    idx = scene.draw_samples(2, n, 100)
    o = api.Oracle(**scene_params(ws, num_threads=4))
    o.set_cloud(xyz)
    o.compute_normals()
    nrm = o.get_normals().T.astype(np.float32)
    nrm[::3] = -nrm[::3]
    wpath, lpath = os.path.join(tmp, "w.ag2w"), os.path.join(tmp, "labels.txt")
    save_ag2w(wpath, make_lenet_weights(7))
    open(lpath, "w").write("0\n1\n")
    xyz.astype("<f4").tofile(os.path.join(tmp, "cloud.f32"))
    np.ascontiguousarray(nrm).astype("<f4").tofile(os.path.join(tmp, "normals.f32"))
    idx.astype("<i4").tofile(os.path.join(tmp, "idx.i32"))
    # (camera_pose is the first camera; the second sits at the origin: the vote between them matters)
    text = params_text(ws, wpath, lpath, 5).replace("min_score_diff = -1e30", "min_score_diff = 0.0") \
        .replace("num_selected = 1000", "num_selected = 10")
    open(os.path.join(tmp, "params.txt"), "w").write(text)
    r = subprocess.run([exe, os.path.join(tmp, "cloud.f32"), os.path.join(tmp, "normals.f32"),
                        os.path.join(tmp, "idx.i32"), os.path.join(tmp, "params.txt"), str(n // 3)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "sized frames ok" in r.stdout, r.stdout
