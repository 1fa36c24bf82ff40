#!/usr/bin/env python3
"""What the whole-recording attention track costs on the GPU ("Whole-recording attention"): one MI355X, b = 8 windows,
8 x 256^2, bf16, a 900-frame 360 x 480 recording with a 30 s waveform at stride 16, as tools/video_bench.py lays it out.  Two
comparisons in ONE process:

  1. video   GazePredictor.predict_video with and without attention_track=True: wall-clock seconds per call (a host clock around
             the call and a device synchronise), rounds alternated; the figure of merit is what the flag adds to one call.
  2. op      ops.attention_track alone on the audio_attention of every window of that recording, against the composition a user
             had before it: the per-window attention=True result (column, head mean), the time mix by torch indexing, index_add_
             of the mixed maps per video frame, division by the count, F.interpolate(bilinear) to S x S per frame and head,
             amin / amax, rescale.  Both captured into a HIP graph and replayed; rounds alternate; one event pair spans --steps
             replays.

Medians and the spread over rounds go to --out.

    python tools/attention_track_bench.py                          # -> profiles/attention_track_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from attention_bench import compare, graphed        # noqa: E402
from csts_amd import ops                            # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402
from csts_amd.infer import GazePredictor          # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


def time_axis(T, Tp, dev):
    """(t0, t1, lambda) of every input frame on the axis of T' coarse maps (align_corners=False), as torch tensors."""
    u = ((torch.arange(T, device=dev, dtype=torch.float32) + 0.5) * Tp / T - 0.5).clamp(min=0)
    t0 = u.floor().long().clamp(max=Tp - 1)
    return t0, (t0 + 1).clamp(max=Tp - 1), u - t0


def parent_track(column, frames_idx, n_frames, T, S):
    """The composition attention_track replaces, from torch ops alone (no host read: it is captured like the op)."""
    Wn, Hh, Tp, h, w = column.shape
    cols = torch.cat([column, column.mean(dim=1, keepdim=True)], dim=1)                  # (Wn, Hh + 1, T', h, w)
    t0, t1, lam = time_axis(T, Tp, column.device)
    lam = lam[None, None, :, None, None]
    mixed = (1 - lam) * cols[:, :, t0] + lam * cols[:, :, t1]                            # (Wn, Hh + 1, T, h, w)
    rows = mixed.permute(0, 2, 1, 3, 4).reshape(Wn * T, Hh + 1, h, w)
    target = frames_idx.reshape(-1).long()
    inside = (target >= 0) & (target < n_frames)
    bucket = torch.where(inside, target, torch.full_like(target, n_frames))              # n_frames: the discard row
    total = torch.zeros(n_frames + 1, Hh + 1, h, w, device=column.device).index_add_(0, bucket, rows)[:n_frames]
    count = torch.zeros(n_frames + 1, device=column.device).index_add_(0, bucket, torch.ones_like(bucket, dtype=torch.float32))
    count = count[:n_frames]
    mean = total / count.clamp(min=1)[:, None, None, None]
    up = torch.nn.functional.interpolate(mean, size=(S, S), mode="bilinear", align_corners=False)
    lo, hi = up.amin(dim=(-2, -1), keepdim=True), up.amax(dim=(-2, -1), keepdim=True)
    return {"mixed": mean, "maps": (mean - lo) / (hi - lo + 1e-6), "range": torch.cat([lo, hi], dim=-1).flatten(2), "count": count}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="replays between the two events of one round of the op comparison")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--video-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_track_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attention_track_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", args.compute])
    N, H, W, B, stride = 900, 360, 480, 8, 16
    S, T = int(cfg.DATA.TEST_CROP_SIZE), int(cfg.DATA.NUM_FRAMES)
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 24000 // 30, generator=g, device=dev)
    res = {"tool": "attention_track_bench", "device": torch.cuda.get_device_name(0), "compute": args.compute, "frames": N, "H": H,
           "W": W, "stride": stride, "batch": B, "rounds": args.rounds, "replays_per_round": args.steps, "warmup": args.warmup,
           "video_rounds": args.video_rounds, "build": build_stamp.current()}
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev, graph=True)

    # ---- 1. the whole recording, with and without the track
    calls = {"plain": lambda: predictor.predict_video(frames, wav, stride=stride, batch=B),
             "attention_track": lambda: predictor.predict_video(frames, wav, stride=stride, batch=B, attention_track=True)}
    kept = {}
    for k, fn in calls.items():                                   # captures both graphs, warms every shape
        for _ in range(2):
            kept[k] = fn()
        torch.cuda.synchronize()
    secs = {k: [] for k in calls}
    for _ in range(args.video_rounds):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in secs.items()}
    track = kept["attention_track"]
    res["video"] = {"windows": track["windows"],
                    **{k: {"median_s": round(med[k], 4), "round_s": [round(x, 4) for x in v], "round_spread_s": round(max(v) - min(v), 4)}
                       for k, v in secs.items()},
                    "attention_track_adds_ms": round((med["attention_track"] - med["plain"]) * 1e3, 2),
                    "attention_track_adds_percent": round((med["attention_track"] / med["plain"] - 1) * 100, 2),
                    "gaze_bit_equal": all(bool(torch.equal(track[k].nan_to_num(-1.0), kept["plain"][k].nan_to_num(-1.0)))
                                          for k in ("points", "peak", "count", "heatmaps", "rescaled")),
                    "attention_frames": int((track["attention_count"] > 0).sum())}
    print("video: " + json.dumps(res["video"]), flush=True)

    # ---- 2. the op alone, on the column of that recording's windows
    with torch.no_grad():
        # the column of every window, as predict_video hands it to the op
        grabbed = {}
        real = ops.attention_track

        def grab(column, frames_idx, n_frames, n_input_frames, crop_size):
            grabbed.update(column=column.clone(), frames_idx=frames_idx.clone())
            return real(column, frames_idx, n_frames, n_input_frames, crop_size)

        ops.attention_track = grab
        try:
            calls["attention_track"]()
        finally:
            ops.attention_track = real
        column, frames_idx = grabbed["column"], grabbed["frames_idx"]
        nwin, heads = column.shape[0], column.shape[1]
        h, w = column.shape[3:]
        Tp = column.shape[2]
        g_new, o_new = graphed(lambda: ops.attention_track(column, frames_idx, N, T, S), args.warmup)
        g_old, o_old = graphed(lambda: parent_track(column, frames_idx, N, T, S), args.warmup)
        torch.cuda.synchronize()
        hit = o_new["count"] > 0
        r2 = compare({"attention_track": g_new.replay, "parent": g_old.replay}, args.rounds, args.steps)
        r2["parent_over_new"] = round(r2["parent"]["median_us"] / r2["attention_track"]["median_us"], 2)
        r2["new_is_faster"] = bool(r2["attention_track"]["median_us"] < r2["parent"]["median_us"])
        r2["shape"] = {"windows": nwin, "heads": heads, "Tp": Tp, "grid": [h, w], "T": T, "S": S, "frames": N,
                       "hit_frames": int(hit.sum()), "pairs_per_hit_frame_max": int(o_new["count"].max())}
        r2["agreement"] = {"count_equal": bool(torch.equal(o_new["count"].float(), o_old["count"])),
                           "mixed_max_abs": float((o_new["mixed"] - o_old["mixed"]).abs().max()),
                           "maps_max_abs_on_hit": float((o_new["maps"][hit] - o_old["maps"][hit]).abs().max()),
                           "range_max_abs_on_hit": float((o_new["range"][hit] - o_old["range"][hit]).abs().max())}
        r2["bytes_parent_upsampled"] = N * (heads + 1) * S * S * 4
        r2["bytes_written_new"] = sum(v.numel() * 4 for v in o_new.values())
        res["op"] = r2
        print("op: " + json.dumps({k: (v["median_us"] if isinstance(v, dict) and "median_us" in v else v) for k, v in r2.items()}),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
