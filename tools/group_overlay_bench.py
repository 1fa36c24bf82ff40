#!/usr/bin/env python3
"""What one launch for all slots buys the overlay of a live group ("Live group"), at the level of the ops:
  grouped   ops.group_points_source + ops.group_gaze_overlay over N jobs: two table uploads, two launches, one allocation;
  per_job   N times (infer.points_to_source, infer.marker_centers, ops.gaze_overlay or ops.gaze_overlay_yuv with the params row
            given on the host): what GazeLiveGroup._slot_rows did per slot and round before.
N = 1, 4, 16 jobs of one frame each (a tick of a frame per stream) and of 8 frames each, frames of 1088 x 1080 (H x W) in packed
RGB and in nv12 (drawn in nv12), a 64 x 64 map, S 256, alpha 0.4, radius 5, one marker a frame.  The frames are synthesised from a
seed.  The two variants are checked to give the same bytes, warmed up, and then timed in alternating rounds: a round is `--steps`
calls and one device synchronise under a host clock, so it sees what a caller sees -- the host chain and the kernels, whichever
is longer.  Reported per configuration: the median over the rounds in microseconds a call, every round, the spread of the rounds
and the ratio of the medians.  No threshold: this is a record.

    python tools/group_overlay_bench.py                            # -> profiles/group_overlay_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                                  # noqa: E402
from csts_amd import inputs, marker_centers, ops, points_to_source  # noqa: E402

H, W, S, M, ALPHA, RADIUS = 1088, 1080, 256, 64, 0.4, 5
NV12 = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}


def make_case(n, k, fmt, dev, g):
    shape = (k, H * 3 // 2, W) if fmt else (k, H, W, 3)
    frames = [torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8) for _ in range(n)]
    p = torch.softmax(torch.randn(n * k, M * M, generator=g, device=dev) / 2, dim=-1)
    mn, mx = p.amin(dim=-1, keepdim=True), p.amax(dim=-1, keepdim=True)
    maps = ((p - mn) / (mx - mn + 1e-6)).reshape(n * k, M, M).contiguous()
    points = torch.rand(n * k, 2, generator=g, device=dev)
    row = inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
    return frames, maps, points, row


def variants(frames, maps, points, row, fmt):
    n, k = len(frames), frames[0].shape[0]

    def grouped():
        src = ops.group_points_source(points, [(k, row, H, W)] * n, S)
        return ops.group_gaze_overlay([(f, row) for f in frames], maps, src["centers"], S, alpha=ALPHA, radius=RADIUS, **fmt)

    def per_job():
        outs = []
        for j, f in enumerate(frames):
            sel = slice(j * k, (j + 1) * k)
            centers = marker_centers(points_to_source(points[sel], row, S), H, W)
            if fmt:
                outs.append(ops.gaze_overlay_yuv(f, maps[sel], row, S, centers=centers, alpha=ALPHA, radius=RADIUS, **fmt))
            else:
                outs.append(ops.gaze_overlay(f, maps[sel], row, S, centers=centers, alpha=ALPHA, radius=RADIUS))
        return outs

    return {"grouped": grouped, "per_job": per_job}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps               # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50, help="calls between two synchronisations: one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--jobs", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_overlay_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/group_overlay_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    res = {"tool": "group_overlay_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "calls_per_round": args.steps, "warmup": args.warmup, "build": build_stamp.current(), "shape": [H, W], "map": [M, M],
           "crop": S, "cases": []}
    for name, fmt in (("rgb24", {}), ("nv12", NV12)):
        for k in args.frames:
            for n in args.jobs:
                g = torch.Generator(device=dev).manual_seed(1000 * n + k)
                run = variants(*make_case(n, k, fmt, dev, g), fmt)
                a, b = run["grouped"](), run["per_job"]()
                differing = sum(int((x != y).sum()) for x, y in zip(a, b))
                del a, b
                for fn in run.values():
                    for _ in range(args.warmup):
                        fn()
                times = {v: [] for v in run}
                for _ in range(args.rounds):
                    for v, fn in run.items():
                        times[v].append(timed(fn, args.steps))
                case = {"format": name, "jobs": n, "frames_per_job": k, "bytes_differing": differing}
                for v, ts in times.items():
                    case[v] = {"median_us": round(statistics.median(ts), 1), "round_us": [round(t, 1) for t in ts],
                               "round_spread_us": round(max(ts) - min(ts), 1)}
                case["per_job_over_grouped"] = round(case["per_job"]["median_us"] / case["grouped"]["median_us"], 2)
                case["grouped_faster_beyond_spread"] = bool(max(times["grouped"]) < min(times["per_job"]))
                res["cases"].append(case)
                print(f"{name} {n} jobs x {k} frames: grouped {case['grouped']['median_us']} us, per job "
                      f"{case['per_job']['median_us']} us, ratio {case['per_job_over_grouped']}, bytes differing {differing}", flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
