#!/usr/bin/env python3
"""Generate tests/golden/reference_constants.json from a checkout of the reference (gwding/agile_grasp2).

The reference holds no tests or golden vectors for the hot path, only structural constants (SURVEY.md
section 8c).  This script reads them out of its files as text and stores the VALUES (numbers, names,
shapes; no source text) so that tests/test_reference_constants.py and tests/test_cpp_host.py can check
them without the reference tree.  Regenerate with

    python tests/golden/make_reference_constants.py <path to the reference checkout>

Sources: src/agile_grasp2/grasp_detector.cpp (base_tf, sqrt_tf), src/agile_grasp2/finger_hand.cpp
(finger slots per side), caffe/test_1batch2.prototxt (LeNet input and layers),
include/agile_grasp2/hand_search.h (default neighbour radii), launch/file_detect_grasps.launch
(parameters in file order, comments removed).
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_constants.json")


def read(ref, rel):
    with open(os.path.join(ref, rel)) as f:
        return f.read()


def extract(ref):
    out = {}
    txt = read(ref, "src/agile_grasp2/grasp_detector.cpp")
    for name in ("base_tf", "sqrt_tf"):
        m = re.search(name + r"\s*<<([^;]*);", txt)
        vals = [float(v) for v in m.group(1).replace("\n", " ").split(",")]
        assert len(vals) == 16, name
        out[name] = vals

    fh = read(ref, "src/agile_grasp2/finger_hand.cpp")
    m = re.search(r"int n = (\d+);", fh)
    # the slots: LinSpaced(n, 0, od - fw) and the same shifted by -(od - fw) (what the tests' formula assumes)
    assert m and "setLinSpaced(n, 0.0, hand_outer_diameter - finger_width)" in fh
    assert "(fs_half.array() - hand_outer_diameter_ + finger_width_).matrix(), fs_half" in fh
    out["finger_slots_per_side"] = int(m.group(1))

    proto = read(ref, "caffe/test_1batch2.prototxt")
    out["lenet_input"] = [int(v) for v in re.findall(r"dim:\s*(\d+)", proto)]
    layers = re.findall(r'layer\s*\{\s*name:\s*"(\w+)"\s*type:\s*"(\w+)"(.*?)(?=layer\s*\{|\Z)', proto, flags=re.S)
    out["lenet_layers"] = []
    for name, typ, body in layers:
        prm = {}
        for key in ("num_output", "kernel_size", "stride", "pool"):
            m = re.search(key + r":\s*(\w+)", body)
            if m:
                prm[key] = int(m.group(1)) if m.group(1).isdigit() else m.group(1)
        out["lenet_layers"].append([name, typ, prm])

    hs = read(ref, "include/agile_grasp2/hand_search.h")
    for key in ("nn_radius_taubin", "nn_radius_hands"):
        m = re.search(key + r"_\(([0-9.]+)\)", hs)
        out["hand_search_default_" + key] = float(m.group(1))

    launch = re.sub(r"<!--.*?-->", "", read(ref, "launch/file_detect_grasps.launch"), flags=re.S)
    out["launch_rosparams"] = [[k, v.strip()] for k, v in
                               re.findall(r'<rosparam\s+param="(\w+)">([^<]*)</rosparam>', launch)]
    out["launch_params"] = [[k, v] for k, v in re.findall(r'<param\s+name="(\w+)"\s+value="([^"]*)"', launch)]
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with open(OUT, "w") as f:
        json.dump(extract(sys.argv[1]), f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
