#!/usr/bin/env python3
"""Per-frame time of the cfg5-sized stream (about 300 k points, 2 000 samples, clouds resident in HBM) through the
frame entries, one process, alternating blocks:

  a   ag2_detect_frame on a one-camera context (the path before the description entries) -- timed TWICE (a1, a2),
      so that its spread against itself in this run is known
  b   the same clouds on a two-camera context through ag2_detect_frame_desc (differs from a by the pack's mask)
  c   b with the normals given (k_gather_normals in place of k_normals)

Every way is warmed up until its graph replays.  Latency = host time of one call (it ends with the wait for the
results).  Writes one JSON record; nothing is asserted.

    python tools/time_frames_sized.py [--frames 1000] [--block 50] [--out profiles/frames_sized.json]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from agile_grasp2_amd import capi, scene  # noqa: E402
from agile_grasp2_amd.weights import make_lenet_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1000, help="timed frames per way")
ap.add_argument("--block", type=int, default=50, help="frames of one way before the next takes over")
ap.add_argument("--clouds", type=int, default=4)
ap.add_argument("--out", default="")
args = ap.parse_args()

n_points, S, R, _, _ = bench.CONFIGS["cfg5"]
clouds, ws = scene.make_stream(40, n_points, args.clouds, voxel=scene.VOXEL)
idxs = [scene.draw_samples(20 + k, len(c), S) for k, c in enumerate(clouds)]
cams = [scene.CAMERA, scene.CAMERA + np.array([0.0, 0.6, 0.1])]
prm1 = bench.launch_params(ws, R)
prm2 = dict(prm1, n_cams=2, cam_origin=cams)
w = make_lenet_weights(7)


def make(prm):
    d = capi.Detector(**prm)
    d.lenet_load(w)
    d.set_stage_timing(0)
    d.stream_configure(0, 0, True)
    return d


ctx = {"a": make(prm1), "b": make(prm2), "c": make(prm2)}
dev = [torch.from_numpy(c).cuda() for c in clouds]
# the normals c brings: the computed ones of each cloud, as float32 records of their own
nrm = []
for c in clouds:
    ctx["c"].set_cloud_desc(c, size_left=len(c) // 2)
    ctx["c"].compute_normals()
    nrm.append(torch.from_numpy(np.ascontiguousarray(ctx["c"].get_normals().T.astype(np.float32))).cuda())
torch.cuda.synchronize()


def frame(way, k):
    j = k % len(clouds)
    n = len(clouds[j])
    if way == "a":
        return ctx["a"].detect_frame(sample_idx=idxs[j], seed=k, dptr=dev[j].data_ptr(), n=n, stride=12)[1]
    kw = dict(dptr=dev[j].data_ptr(), n=n, stride=12, size_left=n // 2)
    if way == "c":
        kw.update(normals_dptr=nrm[j].data_ptr(), normals_stride=12)
    return ctx[way].detect_frame_desc(sample_idx=idxs[j], seed=k, **kw)[1]


for way in ctx:   # warm-up: until the graph replays (a frame that outgrows the learned shapes runs step by step)
    for k in range(200):
        frame(way, k)
        if k >= 2 * len(clouds) and ctx[way].frame_info().graph_replays >= 2 * len(clouds):
            break
    else:
        raise SystemExit(f"way {way}: the graph never replayed: {ctx[way].frame_info().graph_replays}")

legs = [("a1", "a"), ("b", "b"), ("c", "c"), ("a2", "a")]
lat = {name: [] for name, _ in legs}
scored = {name: 0 for name, _ in legs}
before = {way: ctx[way].frame_info() for way in ctx}
gc.collect()
gc.disable()
k0 = {name: 0 for name, _ in legs}
while min(len(v) for v in lat.values()) < args.frames:
    for name, way in legs:
        for _ in range(args.block):
            t0 = time.perf_counter()
            scored[name] += frame(way, k0[name])
            lat[name].append((time.perf_counter() - t0) * 1e3)
            k0[name] += 1
gc.enable()

out = {"workload": f"cfg5-sized stream: {len(clouds)} voxelised clouds of about {n_points} points in HBM, {S} samples, "
                   f"{R} orientations, host time of one synchronous frame call",
       "block": args.block, "ways": {}}
for name, way in legs:
    v = np.asarray(lat[name])
    out["ways"][name] = {"frames": int(len(v)), "window_s": float(v.sum() / 1e3), "p50_ms": float(np.percentile(v, 50)),
                         "p99_ms": float(np.percentile(v, 99)), "mean_ms": float(v.mean()),
                         "scored_per_frame": scored[name] / len(v)}
for way in ctx:
    fi, f0 = ctx[way].frame_info(), before[way]
    # (frames of the timed window that were not graph replays, and why: ag2_frame_info; for a: a1 and a2 together)
    out["ways"]["a1" if way == "a" else way]["frame_info_in_window"] = {
        f: int(getattr(fi, f) - getattr(f0, f))
        for f in ("frames", "graph_replays", "plain_runs", "stepwise_runs", "captures", "fallbacks")}
a1, a2 = out["ways"]["a1"], out["ways"]["a2"]
out["a_against_itself_p50_ms"] = abs(a1["p50_ms"] - a2["p50_ms"])
out["b_minus_a_p50_ms"] = out["ways"]["b"]["p50_ms"] - 0.5 * (a1["p50_ms"] + a2["p50_ms"])
out["c_minus_a_p50_ms"] = out["ways"]["c"]["p50_ms"] - 0.5 * (a1["p50_ms"] + a2["p50_ms"])
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
for d in ctx.values():
    d.close()
