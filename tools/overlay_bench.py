#!/usr/bin/env python3
"""Time of the gaze overlay (ops.gaze_overlay, csts_gaze_overlay) on the GPU against
  (a) torch       the same rule composed from torch ops on the GPU: index the map bilinearly, quantise, gather the JET table, blend
                  in fp32, select by the crop mask, paint the disc -- several full-size fp32 intermediates;
  (b) copy        out.copy_(frames) of the same uint8 tensor: the streaming floor of 3 bytes in + 3 bytes out per pixel.
16 frames of 1080 x 1440 and of 256 x 256 with a 64 x 64 map, S 256, alpha 0.4, radius 5, one marker per frame.  Every variant is
captured in a HIP graph of its own and replayed; rounds alternate the variants, one event pair around `--steps` replays each.
GB/s counts 6 bytes per pixel for every variant.

    python tools/overlay_bench.py                                  # -> profiles/overlay_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from csts_amd import inputs, ops                    # noqa: E402


def axis(E, ne, o, S, m, dev):
    p = torch.arange(E, device=dev, dtype=torch.float64)
    c = (2 * p + 1) * ne
    inside = (c >= o * 2 * E) & (c < (o + S) * 2 * E)
    src = ((((p + 0.5) * ne / E - 0.5 - o) + 0.5) * m / S - 0.5).clamp(min=0)
    i0 = src.floor().clamp(max=m - 1)
    return inside, i0.long(), (i0 + 1).clamp(max=m - 1).long(), (src - i0).float()


def overlay_torch(frames, maps, centers, row, S, alpha, radius, jet, green):
    """The rule of include/csts_hip.h from torch ops (the quantisation may differ from the kernel's on pixels next to a step)."""
    N, H, W, _ = frames.shape
    dev = frames.device
    nh, nw, y0, x0 = row[:4]
    iny, i0, i1, ly = axis(H, nh, y0, S, maps.shape[1], dev)
    inx, j0, j1, lx = axis(W, nw, x0, S, maps.shape[2], dev)
    r0, r1 = maps[:, i0], maps[:, i1]
    top = torch.lerp(r0[:, :, j0], r0[:, :, j1], lx)
    bot = torch.lerp(r1[:, :, j0], r1[:, :, j1], lx)
    v = torch.lerp(top, bot, ly[None, :, None])
    q = (v * 255.0).long().clamp(0, 255)
    f = frames.float()
    blend = torch.round((1.0 - alpha) * f + alpha * jet[q])
    active = centers[:, 0] >= 0
    out = torch.where((iny[:, None] & inx[None, :])[None, :, :, None] & active[:, None, None, None], blend, f)
    Y, X = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
    disc = ((X - centers[:, 0, None, None]) ** 2 + (Y - centers[:, 1, None, None]) ** 2 <= radius * radius) & active[:, None, None]
    return torch.where(disc[..., None], green, out).to(torch.uint8)


def graphed(fn, warmup):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def time_replays(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n              # us per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="replays between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/overlay_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    N, S, M, alpha, radius = 16, 256, 64, 0.4, 5
    jet = torch.from_numpy(ops.jet_table()).float().to(dev)
    green = torch.tensor([0.0, 255.0, 0.0], device=dev)             # made here: a capture admits no copy from the host
    res = {"tool": "overlay_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "replays_per_round": args.steps,
           "warmup": args.warmup, "build": build_stamp.current(), "frames": N, "map": [M, M], "shapes": {}}
    for H, W in ((1080, 1440), (256, 256)):
        g = torch.Generator(device=dev).manual_seed(H)
        frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        p = torch.softmax(torch.randn(N, M * M, generator=g, device=dev) / 2, dim=-1)
        mn, mx = p.amin(dim=-1, keepdim=True), p.amax(dim=-1, keepdim=True)
        maps = ((p - mn) / (mx - mn + 1e-6)).reshape(N, M, M).contiguous()
        row = [S, S, 0, 0, 0] if (H, W) == (S, S) else \
            inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
        params = torch.tensor(row, dtype=torch.int32, device=dev)
        centers = torch.stack([torch.randint(0, W, (N,), generator=g, device=dev), torch.randint(0, H, (N,), generator=g, device=dev)],
                              dim=-1).to(torch.int32)
        out_k, out_c = torch.empty_like(frames), torch.empty_like(frames)
        variants = {"gaze_overlay": lambda: ops.gaze_overlay(frames, maps, params, S, centers=centers, alpha=alpha, radius=radius, out=out_k),
                    "torch": lambda: overlay_torch(frames, maps, centers, row, S, alpha, radius, jet, green),
                    "copy": lambda: out_c.copy_(frames)}
        differ = (variants["gaze_overlay"]().int() - variants["torch"]().int()).abs().amax(dim=-1)
        graphs = {k: graphed(fn, args.warmup) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, gr in graphs.items():
                times[k].append(time_replays(gr, args.steps))
        nbytes = 6 * N * H * W
        shape = {"params": row, "bytes_in_plus_out": nbytes,
                 "pixels_differing_from_torch": int((differ > 0).sum()), "max_channel_difference": int(differ.max())}
        for k, v in times.items():
            med = statistics.median(v)
            shape[k] = {"median_us": round(med, 2), "round_us": [round(x, 2) for x in v], "round_spread_us": round(max(v) - min(v), 2),
                        "gb_per_s": round(nbytes / med / 1e3, 1)}
        shape["torch_over_fused"] = round(shape["torch"]["median_us"] / shape["gaze_overlay"]["median_us"], 2)
        shape["fused_over_copy"] = round(shape["gaze_overlay"]["median_us"] / shape["copy"]["median_us"], 2)
        shape["fused_beats_torch_beyond_spread"] = bool(max(times["gaze_overlay"]) < min(times["torch"]))
        res["shapes"][f"{H}x{W}"] = shape
        print(f"{H}x{W}: " + ", ".join(f"{k} {shape[k]['median_us']} us ({shape[k]['gb_per_s']} GB/s)" for k in variants) +
              f", torch / fused {shape['torch_over_fused']}, fused / copy {shape['fused_over_copy']}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
