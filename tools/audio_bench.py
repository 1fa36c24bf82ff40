#!/usr/bin/env python3
"""Time of the audio resampling (inputs.resample_audio, csts_resample_wav) on the GPU against
  (a) torch   the textbook composition of the same rule from torch ops: zero-stuff the waveform by `up`, pad `half` zeros at both
              ends, F.conv1d with the flipped filter at stride `down` -- for 44.1 kHz (80/147) the stuffed signal is 80 times the
              input;
and of GazePredictor.predict_video on one recording with its 48 kHz waveform (sample_rate=48000) against the same call on the
waveform already at 24 kHz.  Mono fp32 waveforms of 10 s and 300 s at 48 kHz and 44.1 kHz.  Every variant is warmed up on its own
shape; rounds alternate the variants, one event pair around `--steps` calls each (the torch composition of the 300 s waveforms
runs `--long-steps` calls a round, and those cases `--long-rounds` rounds).  The file is rewritten after every case, so a case
that fails leaves the earlier ones.

    python tools/audio_bench.py                                    # -> profiles/audio_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from csts_amd import GazePredictor, inputs          # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402


def resample_torch(x, taps, up, down, half):
    """The rule of include/csts_hip.h from torch ops: x (n,) -> (ceil(n up / down),)."""
    n = x.shape[0]
    n_out = -(-n * up // down)
    need = (n_out - 1) * down + 2 * half + 1                    # stuffed samples the last output reaches, with the left pad
    z = torch.zeros(max(need, half + n * up), dtype=torch.float32, device=x.device)
    z[half:half + n * up:up] = x
    return F.conv1d(z[None, None, :need], taps.flip(0)[None, None], stride=down)[0, 0]


def time_calls(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n              # us per call


def summary(v):
    med = statistics.median(v)
    return {"median_us": round(med, 2), "round_us": [round(x, 2) for x in v], "round_spread_us": round(max(v) - min(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="calls between the two events of one round")
    ap.add_argument("--long-steps", type=int, default=1, help="the same for the torch composition of the 300 s waveforms")
    ap.add_argument("--long-rounds", type=int, default=3, help="rounds of the 300 s cases")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--video-frames", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/audio_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    res = {"tool": "audio_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.steps,
           "calls_per_round_torch_300s": args.long_steps, "rounds_300s": args.long_rounds, "warmup": args.warmup,
           "build": build_stamp.current(), "resample": {}}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    for seconds in (10, 300):
        for rate in (48000, 44100):
            taps, up, down, half = inputs.resample_filter(rate, device=dev)
            n = rate * seconds
            x = 0.1 * torch.randn(n, generator=torch.Generator(device=dev).manual_seed(rate + seconds), device=dev)
            variants = {"resample_audio": lambda: inputs.resample_audio(x, rate),
                        "torch": lambda: resample_torch(x, taps, up, down, half)}
            steps = {"resample_audio": args.steps, "torch": args.steps if seconds <= 10 else args.long_steps}
            case = {"samples": n, "ratio": [up, down], "taps": 2 * half + 1, "stuffed_samples": n * up,
                    "multiply_adds_polyphase": int(-(-n * up // down) * (2 * half // up + 1))}
            got, want = variants["resample_audio"](), variants["torch"]()
            case["max_abs_difference_from_torch"] = float((got - want).abs().max())
            del got, want
            for k, fn in variants.items():
                for _ in range(args.warmup if steps[k] > args.long_steps else 1):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds if seconds <= 10 else args.long_rounds):
                for k, fn in variants.items():
                    times[k].append(time_calls(fn, steps[k]))
            for k, v in times.items():
                case[k] = summary(v)
            case["torch_over_kernel"] = round(case["torch"]["median_us"] / case["resample_audio"]["median_us"], 2)
            case["kernel_beats_torch_beyond_spread"] = bool(max(times["resample_audio"]) < min(times["torch"]))
            case["input_gb_per_s"] = round(4 * n / case["resample_audio"]["median_us"] / 1e3, 1)
            res["resample"][f"{rate}Hz_{seconds}s"] = case
            write()
            print(f"{rate} Hz, {seconds} s: resample_audio {case['resample_audio']['median_us']} us, torch "
                  f"{case['torch']['median_us']} us, torch / kernel {case['torch_over_kernel']}", flush=True)
            del x
            torch.cuda.empty_cache()

    # the whole path: one recording, its waveform at 48 kHz with the rate against the waveform already at 24 kHz
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"), ["NUM_GPUS", 1])
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev)
    N = args.video_frames
    g = torch.Generator(device=dev).manual_seed(3)
    frames = torch.randint(0, 256, (N, 360, 480, 3), generator=g, device=dev, dtype=torch.uint8)
    wav48 = 0.1 * torch.randn(N * 48000 // 30, generator=g, device=dev)
    wav24 = inputs.resample_audio(wav48, 48000)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    variants = {"at_24khz": lambda: predictor.predict_video(frames, wav24, return_heatmaps=False),
                "sample_rate_48000": lambda: predictor.predict_video(frames, wav48, return_heatmaps=False, sample_rate=48000)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(wall(fn))
    video = {"frames": N, "frame_size": [360, 480], "samples_48khz": int(wav48.shape[0]), "clock": "host, around a synchronised call"}
    for k, v in times.items():
        video[k] = summary(v)
    video["added_us"] = round(video["sample_rate_48000"]["median_us"] - video["at_24khz"]["median_us"], 2)
    video["added_beyond_spread"] = bool(min(times["sample_rate_48000"]) > max(times["at_24khz"]))
    res["predict_video"] = video
    write()
    print(f"predict_video, {N} frames: at 24 kHz {video['at_24khz']['median_us']} us, with sample_rate=48000 "
          f"{video['sample_rate_48000']['median_us']} us", flush=True)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
