"""Host time per ImportanceSampling::detectGraspPoses call of the C++ mirror, the host loop (default) against
ONE ag2_detect_importance call (setSampleOnDevice(true)), at the launch-file setting
(launch/file_importance_sampling.launch: 100 initial samples, 5 rounds of 50, MAX, min_inliers 5).
Median over --reps calls after two warm-up calls; prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from agile_grasp2_amd import scene  # noqa: E402
from agile_grasp2_amd.weights import make_lenet_weights, save_ag2w  # noqa: E402


def build_driver(tmp):
    """tests/cpp/importance_device.cpp against the host mirror and the HIP library."""
    host, csrc = os.path.join(ROOT, "agile_grasp2_amd", "host"), os.path.join(ROOT, "agile_grasp2_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "-j", "8"])
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = os.path.join(tmp, "importance_device")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "importance_device.cpp"), "-o", exe,
                           "-L", host, "-lag2host", "-L", csrc, "-lag2hip",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}"])
    return exe


def params_text(ws, wpath, lpath, seed):
    """launch/file_importance_sampling.launch hand geometry (key = value text of GraspDetector::Params).  The
    launch file keeps num_selected 50; min_score_diff is opened up because the synthetic weights score below 500."""
    cam = [float(v) for v in scene.CAMERA]
    pose = [1.0, 0.0, 0.0, cam[0], 0.0, 1.0, 0.0, cam[1], 0.0, 0.0, 1.0, cam[2], 0.0, 0.0, 0.0, 1.0]
    return "\n".join([
        f"workspace = {list(map(float, ws))}", f"camera_pose = {pose}",
        "num_orientations = 8", "nn_radius_taubin = 0.01", "nn_radius_hands = 0.1",
        "finger_width = 0.01", "hand_outer_diameter = 0.09", "hand_depth = 0.06", "hand_height = 0.02",
        "init_bite = 0.01", "filter_half_grasps = false", "gripper_width_range = [0.03, 0.08]",
        "antipodal_mode = 1", f"trained_file = {wpath}", f"label_file = {lpath}", "model_file =",
        "min_score_diff = -1e30", "num_selected = 50", "plot_mode = 0", f"seed = {seed}", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        xyz, ws = scene.make_scene(seed=3, n_target=a.points)
        idx = scene.draw_samples(3, xyz.shape[0], 100)
        wpath, lpath = os.path.join(tmp, "w.ag2w"), os.path.join(tmp, "labels.txt")
        save_ag2w(wpath, make_lenet_weights(7))
        open(lpath, "w").write("0\n1\n")
        xyz.astype("<f4").tofile(os.path.join(tmp, "cloud.f32"))
        idx.astype("<i4").tofile(os.path.join(tmp, "idx.i32"))
        open(os.path.join(tmp, "params.txt"), "w").write(params_text(ws, wpath, lpath, 9))
        res = {"points": int(xyz.shape[0]), "initial_samples": 100, "rounds": 5, "samples": 50, "min_inliers": 5}
        for name, dev in (("host_loop_ms", "0"), ("device_ms", "1")):
            r = subprocess.run([exe, os.path.join(tmp, "cloud.f32"), os.path.join(tmp, "idx.i32"),
                                os.path.join(tmp, "params.txt"), dev, "5", os.path.join(tmp, "out.bin"),
                                str(a.reps), "5", "50"], capture_output=True, text=True, timeout=600)
            if r.returncode:
                raise SystemExit(r.stderr)
            res[name] = float(re.search(r"median_ms ([0-9.]+)", r.stdout).group(1))
        res["note"] = f"host time per ImportanceSampling::detectGraspPoses call of the C++ mirror, median of {a.reps}"
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
