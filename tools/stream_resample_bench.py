"""Resampling on a live stream, measured in ONE process ("Live stream", "Audio at any rate"):

  push      inputs.StreamResampler.push of the audio of 8 frames at 30 fps -- 12 800 samples at 48 kHz, 11 760 at 44.1 kHz, mono
            fp32 -- next to inputs.resample_audio of a piece of the same size (stateless: zero edges, one launch, no tail to
            carry).  The two alternate piece by piece; every call is timed on the host with the device drained before and after,
            as a caller that reads the samples would see it.  `--pushes` timed pieces (default 256) after `--warmup` of each.
  stream    GazePredictor.stream on tools/stream_bench.py's recording (360 x 480 frames, Ego4D forecast plan, bf16, stride 9,
            pushes of 8 frames): the audio pushed at 48 kHz with input_rate=48000 against the same recording's audio at 24 kHz
            (resampled beforehand).  The two replays alternate over `--rounds` rounds after one warm-up replay each; per-push
            times are pooled over the rounds.

Reports the median, the 10th / 90th percentile and the extremes of every series.  --merge KEY=FILE adds the JSON of FILE under
"other_tools"[KEY]: the figures of tools measured beside this one (tools/audio_bench.py on two builds, bench.py).  Writes the
JSON (with the build stamp) to --out and prints it on one line.

    python tools/stream_resample_bench.py                          # -> profiles/stream_resample_bench.json
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
from csts_amd import GazePredictor, inputs          # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
CHUNK, FPS = 8, 30


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, r


def series(v):
    """Per-call microseconds -> the median and the spread."""
    s = sorted(v)
    return {"calls": len(s), "median_us": round(statistics.median(s), 2), "p10_us": round(s[len(s) // 10], 2),
            "p90_us": round(s[len(s) * 9 // 10], 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2)}


def bench_push(rate, pushes, warmup, dev):
    piece = rate * CHUNK // FPS
    x = 0.1 * torch.randn((pushes + warmup) * piece, generator=torch.Generator(device=dev).manual_seed(rate), device=dev)
    r = inputs.StreamResampler(rate)
    times = {"stream_push": [], "resample_audio": []}
    for i in range(pushes + warmup):
        p = x[i * piece:(i + 1) * piece]
        a, y = wall(lambda: r.push(p))
        b, z = wall(lambda: inputs.resample_audio(p, rate))
        assert y.numel() == (piece * r.up // r.down if i else inputs.resample_ready(piece, r.up, r.down, r.half))
        if i >= warmup:
            times["stream_push"].append(a)
            times["resample_audio"].append(b)
    res = {k: series(v) for k, v in times.items()}
    res.update({"piece_samples": piece, "ratio": [r.up, r.down], "tail_samples": int(r._tail.shape[1]),
                "push_over_stateless": round(res["stream_push"]["median_us"] / res["resample_audio"]["median_us"], 3)})
    return res


def replay(predictor, frames, wav, per, rate):
    s = predictor.stream(stride=9, input_rate=rate)
    secs, windows = [], 0
    for a in range(0, frames.shape[0], CHUNK):
        b = min(a + CHUNK, frames.shape[0])
        t, r = wall(lambda: s.push(frames[a:b], wav[a * per:b * per]))
        secs.append(t)
        windows += len(r)
    return secs, windows


def bench_stream(frames_n, rounds, dev):
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "bf16"])
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (frames_n, 360, 480, 3), generator=g, device=dev, dtype=torch.uint8)
    wav48 = 0.1 * torch.randn(frames_n * 1600, generator=g, device=dev)
    wav24 = inputs.resample_audio(wav48, 48000)
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    variants = {"at_24khz": (wav24, 800, None), "input_rate_48000": (wav48, 1600, 48000)}
    windows = {k: replay(predictor, frames, *v)[1] for k, v in variants.items()}       # warm-up: captures the graph
    times = {k: [] for k in variants}
    totals = {k: [] for k in variants}
    for _ in range(rounds):
        for k, v in variants.items():
            secs, w = replay(predictor, frames, *v)
            assert w == windows[k]
            times[k] += secs
            totals[k].append(round(sum(secs) / 1e3, 3))
    res = {k: dict(series(v), total_round_ms=totals[k], windows=windows[k]) for k, v in times.items()}
    res.update({"frames": frames_n, "chunk": CHUNK, "stride": 9, "rounds": rounds,
                "added_median_us_per_push": round(res["input_rate_48000"]["median_us"] - res["at_24khz"]["median_us"], 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--frames", type=int, default=450)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--merge", action="append", default=[], metavar="KEY=FILE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_resample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/stream_resample_bench.py measures on an MI355X: no GPU found")
    if args.pushes < 200:
        raise SystemExit("--pushes: at least 200 timed pushes")
    dev = torch.device("cuda:0")
    out = {"tool": "stream_resample_bench", "device": torch.cuda.get_device_name(0), "build": build_stamp.current(),
           "clock": "host, around one call with the device drained before and after", "warmup": args.warmup, "push": {}}
    for rate in (48000, 44100):
        out["push"][f"{rate}Hz"] = bench_push(rate, args.pushes, args.warmup, dev)
    out["stream"] = bench_stream(args.frames, args.rounds, dev)
    for item in args.merge:
        key, path = item.split("=", 1)
        out.setdefault("other_tools", {})[key] = json.load(open(path))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
