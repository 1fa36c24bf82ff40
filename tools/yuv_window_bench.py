#!/usr/bin/env python3
"""Decoder surfaces read in place against the repack a caller did before ("Decoder surfaces"): 16 nv12
surfaces of Hs x Ws = 1088 x 2048 holding 1080 x 1920 pictures, window (0, 0, 1080, 1920) -- what a hardware decoder hands over for
a 1080p stream.  For each of
  clip_sample        2 clips of T 8 out of the 16 frames, S 256, the test-mode centre crop;
  yuv_to_rgb         the 16 frames into one RGB tensor;
  gaze_overlay_yuv   the 16 frames drawn out of place (64 x 64 maps, one marker a frame), and in place;
  stream_push        one GazeStream.push of 8 frames with their audio at stride 8 (random weights; eager, a push works on the host
                     too): a fresh stream is fed 88 frames untimed, so that every timed push completes a window, then `--pushes`
                     pushes run between two events
the windowed call on the surfaces is timed against inputs.yuv_window of the surfaces followed by the tight call: "window" and
"repack_then_tight", plus "repack" alone.  The two give the same bits (checked first; the overlay through yuv_window).  All but
the push are captured in a HIP graph each and replayed; rounds alternate the variants, one event pair around `--steps` replays
each; medians over the rounds and the per-round spread are reported, whatever comes out.

    python tools/yuv_window_bench.py                              # -> profiles/yuv_window_bench.json

--merge NAME=FILE ... : also record the JSON files of other benches (tools/yuv_bench.py and tools/overlay_yuv_bench.py of this
tree and of its parent, run in the same visit, alternated) under "tight_path" in the output; with --merge-only nothing is measured
and the files are added to the JSON --out already holds (no GPU needed)."""
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
from csts_amd import GazePredictor, inputs, ops     # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402
from overlay_bench import graphed, time_replays     # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, HS, WS, WINDOW, S, M = 16, 1088, 2048, (0, 0, 1080, 1920), 256, 64
FMT = {"pixel_format": "nv12", "matrix": "bt709", "full_range": False}


def summary(times):
    return {k: {"median_us": round(statistics.median(v), 2), "round_us": [round(x, 2) for x in v],
                "round_spread_us": round(max(v) - min(v), 2)} for k, v in times.items()}


def verdict(res):
    """window against repack_then_tight: the ratio of the medians, and whether the rounds of one lie wholly below the other's."""
    w, r = res["window"], res["repack_then_tight"]
    res["repack_then_tight_over_window"] = round(r["median_us"] / w["median_us"], 3)
    res["window_faster_beyond_spread"] = bool(max(w["round_us"]) < min(r["round_us"]))
    res["window_slower_beyond_spread"] = bool(min(w["round_us"]) > max(r["round_us"]))
    return res


def time_graphs(variants, args):
    graphs = {k: graphed(fn, args.warmup) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, gr in graphs.items():
            times[k].append(time_replays(gr, args.steps))
    return verdict(summary(times))


def time_pushes(predictor, surf, wav, window, pushes, rounds):
    """us per GazeStream.push of 8 frames: `pushes` pushes between two events on a stream that was fed 88 frames before (untimed)."""
    per = wav.numel() // surf.shape[0]

    def run(frames, **kw):
        stream = predictor.stream(stride=8, batch=1, **FMT, **kw)
        got = []

        def push(i):
            a = (8 * i) % surf.shape[0]
            got.extend(stream.push(frames(a), wav[a * per:(a + 8) * per]))

        for i in range(11):
            push(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(11, 11 + pushes):
            push(i)
        e1.record()
        e1.synchronize()
        stream.close()
        return e0.elapsed_time(e1) * 1e3 / pushes, got

    variants = {"window": lambda: run(lambda a: surf[a:a + 8], window=window),
                "repack_then_tight": lambda: run(lambda a: inputs.yuv_window(surf[a:a + 8], "nv12", window))}
    first = {k: fn()[1] for k, fn in variants.items()}                                   # warm-up, and the same windows
    same = len(first["window"]) == len(first["repack_then_tight"]) and all(
        torch.equal(a["heatmaps"], b["heatmaps"]) for a, b in zip(first["window"], first["repack_then_tight"]))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(fn()[0])
    res = verdict(summary(times))
    res.update({"pushes_per_round": pushes, "frames_per_push": 8, "windows_per_run": len(first["window"]), "same_bits": bool(same)})
    return res


def merged(items):
    """{NAME: the JSON of FILE} for the NAME=FILE items of --merge."""
    out = {}
    for item in items:
        name, path = item.split("=", 1)
        with open(path) as f:
            out[name] = json.load(f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="replays between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pushes", type=int, default=8, help="pushes of 8 frames between the two events of one stream round")
    ap.add_argument("--merge", nargs="*", default=[], metavar="NAME=FILE", help="JSON files to record under tight_path")
    ap.add_argument("--merge-only", action="store_true", help="measure nothing: add the --merge files to the JSON in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_window_bench.json"))
    args = ap.parse_args()
    if args.merge_only:
        with open(args.out) as f:
            res = json.load(f)
        res.setdefault("tight_path", {}).update(merged(args.merge))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(f"wrote {args.out}")
        return
    if not torch.cuda.is_available():
        raise SystemExit("tools/yuv_window_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    H, W = WINDOW[2:]
    g = torch.Generator(device=dev).manual_seed(HS)
    surf = torch.randint(0, 256, (N, HS * 3 // 2, WS), generator=g, device=dev, dtype=torch.uint8)
    p = torch.softmax(torch.randn(N, M * M, generator=g, device=dev) / 2, dim=-1)
    mn, mx = p.amin(dim=-1, keepdim=True), p.amax(dim=-1, keepdim=True)
    maps = ((p - mn) / (mx - mn + 1e-6)).reshape(N, M, M).contiguous()
    row = inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
    params = torch.tensor(row, dtype=torch.int32, device=dev)
    centers = torch.stack([torch.randint(0, W, (N,), generator=g, device=dev), torch.randint(0, H, (N,), generator=g, device=dev)],
                          dim=-1).to(torch.int32)
    idx = torch.arange(N, dtype=torch.int32, device=dev).view(2, 8)
    par2 = params[None].repeat(2, 1)
    kw = dict(centers=centers, alpha=0.4, radius=5)
    rgb = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    out_s, work = torch.empty_like(surf), surf.clone()
    out_t = torch.empty(N, H * 3 // 2, W, dtype=torch.uint8, device=dev)

    def repack():
        return inputs.yuv_window(surf, "nv12", WINDOW)

    def in_place_tight():                                    # the repack is the working copy a caller draws on
        t = repack()
        return ops.gaze_overlay_yuv(t, maps, params, S, out=t, **kw, **FMT)

    cases = {
        "clip_sample": {"window": lambda: inputs.clip_sample(surf, idx, par2, S, window=WINDOW, **FMT),
                        "repack_then_tight": lambda: inputs.clip_sample(repack(), idx, par2, S, **FMT)},
        "yuv_to_rgb": {"window": lambda: inputs.yuv_to_rgb(surf, out=rgb, window=WINDOW, **FMT),
                       "repack_then_tight": lambda: inputs.yuv_to_rgb(repack(), out=rgb, **FMT)},
        "gaze_overlay_yuv": {"window": lambda: ops.gaze_overlay_yuv(surf, maps, params, S, out=out_s, window=WINDOW, **kw, **FMT),
                             "repack_then_tight": lambda: ops.gaze_overlay_yuv(repack(), maps, params, S, out=out_t, **kw, **FMT)},
        "gaze_overlay_yuv_in_place": {"window": lambda: ops.gaze_overlay_yuv(work, maps, params, S, out=work, window=WINDOW, **kw,
                                                                             **FMT),
                                      "repack_then_tight": in_place_tight},
    }
    same = {"clip_sample": torch.equal(cases["clip_sample"]["window"](), cases["clip_sample"]["repack_then_tight"]()),
            "yuv_to_rgb": torch.equal(cases["yuv_to_rgb"]["window"]().clone(), cases["yuv_to_rgb"]["repack_then_tight"]()),
            "gaze_overlay_yuv": torch.equal(inputs.yuv_window(cases["gaze_overlay_yuv"]["window"](), "nv12", WINDOW),
                                            cases["gaze_overlay_yuv"]["repack_then_tight"]())}
    res = {"tool": "yuv_window_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "replays_per_round": args.steps, "warmup": args.warmup, "build": build_stamp.current(), "frames": N,
           "surface": [HS, WS], "window": list(WINDOW), "format": FMT, "params": row,
           "surface_bytes_per_frame": HS * WS * 3 // 2, "window_bytes_per_frame": H * W * 3 // 2, "same_bits": same}
    for name, variants in cases.items():
        res[name] = time_graphs(dict(variants, repack=repack), args)
        work.copy_(surf)
        print(f"{name}: window {res[name]['window']['median_us']} us, repack + tight {res[name]['repack_then_tight']['median_us']} us "
              f"(repack alone {res[name]['repack']['median_us']} us)", flush=True)
    cfg = load_yaml(YAML, ["NUM_GPUS", 1])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    wav = 0.1 * torch.randn(N * 24000 // 30, device=dev)
    res["stream_push"] = time_pushes(predictor, surf, wav, WINDOW, args.pushes, args.rounds)
    print(f"stream_push: window {res['stream_push']['window']['median_us']} us, repack + tight "
          f"{res['stream_push']['repack_then_tight']['median_us']} us a push of 8 frames", flush=True)
    if args.merge:
        res["tight_path"] = merged(args.merge)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
