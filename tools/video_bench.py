"""Whole-video prediction, measured in ONE process ("Whole-video prediction"):

  (a) sampler  inputs.clip_sample straight out of a resident video against the gather it removes, frames[idx] into a
               (B, T, H, W, 3) tensor followed by inputs.spatial_sample, both from this build: B 8, T 8, a 360 x 480 source, S 256,
               windows 16 frames apart as predict_video lays them out;
  (b) track    ops.gaze_track against its torch composition (index_add_ + divide + min / max / arg-max) at 64 x 64 on the maps
               of a 900-frame video (stride 16: 51 windows of 8 maps);
  (c) video    GazePredictor.predict_video on 900 synthetic frames (360 x 480) with a 30 s waveform at stride 16: clips per second;
  (d) fill     ops.gaze_track_fill in both modes against its torch composition (neighbour search with cummax / a reversed cummin: no host read, a
               gather and blend, then min / max / arg-max) on the sparse track of the DEFAULT Ego4D plan at 900 frames, 64 x 64
               (13 windows, 102 predicted frames); also, from plan_video on the host, how many windows a track made dense by a
               small stride would need instead.

After a warm-up the variants of (a) and of (b) are alternated over several rounds (clock and thermal drift hit both alike); a
round times `--steps` calls between two device events.  Reports the median of the per-round times and their spread, checks
that the variants agree, writes the JSON (with the build stamp) to --out and prints it on one line.

    python tools/video_bench.py                                    # -> profiles/video_bench.json
    python tools/video_bench.py --skip-video                       # (a), (b) and (d) only: no model is built
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
import build_stamp                                  # noqa: E402
from csts_amd import GazePredictor, default_max_gap, inputs, ops, plan_video     # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


def time_calls(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n              # us per call


def alternate(variants, warmup, steps, rounds):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(time_calls(fn, steps))
    return {k: {"median_us": round(statistics.median(v), 2), "round_us": [round(x, 2) for x in v],
                "round_spread_us": round(max(v) - min(v), 2)} for k, v in times.items()}


def track_torch(preds, target_idx, n_frames):
    """The torch composition gaze_track replaces."""
    P, H, W = preds.shape
    keep = (target_idx >= 0) & (target_idx < n_frames)
    t = torch.where(keep, target_idx, torch.full_like(target_idx, n_frames))
    heat = torch.zeros(n_frames + 1, H * W, dtype=torch.float32, device=preds.device).index_add_(0, t, preds.reshape(P, -1))[:-1]
    count = torch.zeros(n_frames + 1, dtype=torch.float32, device=preds.device).index_add_(0, t, torch.ones_like(t, dtype=torch.float32))[:-1]
    heat = heat / count.clamp(min=1)[:, None]
    mn, (mx, idx) = heat.amin(dim=-1, keepdim=True), heat.max(dim=-1, keepdim=True)
    resc = (heat - mn) / (mx - mn + 1e-6)
    points = torch.cat([(idx % W).float() / W, torch.div(idx, W, rounding_mode="floor").float() / H], dim=-1)
    return heat, resc, points, mx[:, 0], count


def fill_torch(heatmaps, count, mode, max_gap):
    """The torch composition gaze_track_fill replaces."""
    N, H, W = heatmaps.shape
    idx = torch.arange(N, device=heatmaps.device)
    pred = count > 0
    a = torch.cummax(torch.where(pred, idx, torch.full_like(idx, -1)), dim=0).values            # last predicted frame <= n, -1: none
    b = torch.flip(torch.cummin(torch.flip(torch.where(pred, idx, torch.full_like(idx, N)), [0]), dim=0).values, [0])   # first predicted frame >= n, N: none
    ok = pred | ((a >= 0) & (b < N) & (b - a <= max_gap))
    ac, bc = a.clamp(min=0), b.clamp(max=N - 1)
    flat = heatmaps.reshape(N, -1)
    if mode == "hold":
        heat = flat[ac]
    else:
        span = (bc - ac).clamp(min=1).float()
        wa = torch.where(bc > ac, (bc - idx).float() / span, torch.ones_like(span))
        wb = torch.where(bc > ac, (idx - ac).float() / span, torch.zeros_like(span))
        heat = wa[:, None] * flat[ac] + wb[:, None] * flat[bc]
    heat = torch.where(ok[:, None], heat, torch.zeros_like(heat))
    mn, (mx, am) = heat.amin(dim=-1, keepdim=True), heat.max(dim=-1, keepdim=True)
    resc = (heat - mn) / (mx - mn + 1e-6)
    points = torch.cat([(am % W).float() / W, torch.div(am, W, rounding_mode="floor").float() / H], dim=-1)
    nb = torch.where(ok[:, None], torch.stack([a, b], dim=-1), torch.full_like(idx, -1)[:, None])
    return heat, resc, points, mx[:, 0], nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50, help="calls between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--video-rounds", type=int, default=3)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/video_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", args.compute])
    N, H, W, S, B, T, stride = 900, 360, 480, 256, 8, 8, 16
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 24000 // 30, generator=g, device=dev)
    plan = plan_video(cfg, N, stride=stride)
    out = {"tool": "video_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.steps,
           "warmup": args.warmup, "build": build_stamp.current()}

    # ---- (a) the sampler
    idx = torch.from_numpy(plan["frames_idx"][:B]).to(dev)
    row = inputs.spatial_rule_host(torch.zeros(1, T, 2).numpy(), H, W, S, train=False, spatial_idx=1)[0]
    params = torch.from_numpy(row).to(dev).repeat(B, 1)
    lidx = idx.long()
    variants = {"clip_sample": lambda: inputs.clip_sample(frames, idx, params, S),
                "gather_then_sample": lambda: inputs.spatial_sample(frames[lidx], params, S)}
    same = bool(torch.equal(variants["clip_sample"](), variants["gather_then_sample"]()))
    res = alternate(variants, args.warmup, args.steps, args.rounds)
    gather_bytes = 2 * B * T * H * W * 3
    out["sampler"] = {"B": B, "T": T, "H": H, "W": W, "S": S, "params": row.tolist()[0], "bit_equal": same, **res,
                      "gather_minus_fused_us": round(res["gather_then_sample"]["median_us"] - res["clip_sample"]["median_us"], 2),
                      "model_MB_per_frame": {"gather_read_write": round(2 * H * W * 3 / 1e6, 3),
                                             "sample_read": round(H * W * 3 / 1e6, 3), "sample_write": round(3 * S * S * 4 / 1e6, 3)},
                      "gather_MB_per_call": round(gather_bytes / 1e6, 2)}

    # ---- (b) the track
    P = plan["windows"] * T
    preds = torch.softmax(torch.randn(P, 64 * 64, generator=g, device=dev) / 2, dim=-1).reshape(P, 64, 64)
    target = torch.from_numpy(plan["target_idx"].reshape(-1)).to(dev)
    variants = {"gaze_track": lambda: ops.gaze_track(preds, target, N), "torch": lambda: track_torch(preds, target, N)}
    a, b = variants["gaze_track"](), variants["torch"]()
    covered = a["count"] > 0
    agree = {"heatmaps_max_abs": float((a["heatmaps"].reshape(N, -1) - b[0]).abs().max()),
             "points_equal_on_covered": bool(torch.equal(a["points"][covered], b[2][covered])),
             "count_equal": bool(torch.equal(a["count"].float(), b[4]))}
    res = alternate(variants, args.warmup, args.steps, args.rounds)
    out["track"] = {"maps": P, "frames": N, "grid": [64, 64], "covered_frames": int(covered.sum()), "agreement": agree, **res,
                    "torch_over_fused": round(res["torch"]["median_us"] / res["gaze_track"]["median_us"], 2)}

    # ---- (c) the whole video
    if not args.skip_video:
        torch.manual_seed(cfg.RNG_SEED)
        predictor = GazePredictor(cfg, device=dev, graph=True)
        predictor.predict_video(frames, wav, stride=stride)          # captures the graph
        torch.cuda.synchronize()
        secs = []
        for _ in range(args.video_rounds):
            t0 = time.perf_counter()
            r = predictor.predict_video(frames, wav, stride=stride)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        med = statistics.median(secs)
        out["video"] = {"frames": N, "H": H, "W": W, "stride": stride, "windows": r["windows"], "compute": args.compute,
                        "batch": min(int(cfg.TEST.BATCH_SIZE), 8), "round_s": [round(v, 4) for v in secs], "median_s": round(med, 4),
                        "round_spread_s": round(max(secs) - min(secs), 4), "clips_per_s": round(r["windows"] / med, 1),
                        "video_frames_per_s": round(N / med, 1), "covered_frames": int((r["count"] > 0).sum())}
    # ---- (d) the fill, on the sparse track of the default plan
    dplan = plan_video(cfg, N)
    gap = default_max_gap(dplan)
    Pd = dplan["windows"] * T
    dpreds = torch.softmax(torch.randn(Pd, 64 * 64, generator=g, device=dev) / 2, dim=-1).reshape(Pd, 64, 64)
    sparse = ops.gaze_track(dpreds, torch.from_numpy(dplan["target_idx"].reshape(-1)).to(dev), N, want=("heatmaps", "count"))
    heat, count = sparse["heatmaps"], sparse["count"]
    predicted = int((count > 0).sum())
    out["fill"] = {"frames": N, "grid": [64, 64], "stride": dplan["stride"], "windows": dplan["windows"], "max_gap": gap,
                   "predicted_frames": predicted}
    for mode in ("hold", "linear"):
        variants = {"gaze_track_fill": lambda m=mode: ops.gaze_track_fill(heat, count, mode=m, max_gap=gap),
                    "torch": lambda m=mode: fill_torch(heat, count, m, gap)}
        a, b = variants["gaze_track_fill"](), variants["torch"]()
        covered = a["neighbours"][:, 0] >= 0
        agree = {"heatmaps_max_abs": float((a["heatmaps"].reshape(N, -1) - b[0]).abs().max()),
                 "points_equal_on_covered": bool(torch.equal(a["points"][covered], b[2][covered])),
                 "neighbours_equal": bool(torch.equal(a["neighbours"].long(), b[4]))}
        res = alternate(variants, args.warmup, args.steps, args.rounds)
        nfilled = int(covered.sum()) - predicted
        maps_moved = predicted + (2 if mode == "linear" else 1) * nfilled + 2 * N      # maps read + heatmaps and rescaled written
        out["fill"][mode] = {"covered_frames": int(covered.sum()), "filled_frames": nfilled, "agreement": agree,
                             "model_MB": round(maps_moved * 64 * 64 * 4 / 1e6, 1),
                             **res, "torch_over_fused": round(res["torch"]["median_us"] / res["gaze_track_fill"]["median_us"], 2)}
    # what a track made dense by stride alone costs in forward passes (host arithmetic, nothing is run)
    dense = plan_video(cfg, N, stride=7)
    dt = dense["target_idx"].reshape(-1)
    dcount = np.bincount(dt[dt < N], minlength=N)
    span = np.nonzero(dcount)[0]
    out["fill"]["dense_by_stride"] = {"stride": 7, "windows": int(dense["windows"]), "windows_with_fill": int(dplan["windows"]),
                                      "empty_frames_in_span": int((dcount[span[0]:span[-1] + 1] == 0).sum())}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
