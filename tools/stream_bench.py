"""Live-stream prediction, measured in ONE process ("Live stream"):

  stream    GazePredictor.stream on the Ego4D forecast plan, bf16: a synthetic recording (360 x 480, 24 kHz audio) is replayed in
            pushes of `chunk` frames with the matching audio; the wall time of every push is taken with the device drained, as a
            caller that reads the points would see it;
  compose   what a user would otherwise write to predict while recording: for every window a push completes, inputs.clip_sample
            out of a resident copy of the frames, a fresh inputs.stft_logpower of the observed waveform, inputs.audio_windows_at
            and predict_batch; pushes that complete no window cost nothing.  It needs the frames resident.

at chunk 1 and chunk 8, at stride 9 and at the default stride.  Both replay the same recording and emit the same windows; they are
alternated over several rounds (clock and thermal drift hit both alike).  Reports, per configuration and variant, the median over
the rounds of the per-round total and of the per-round mean / median / worst push, with the spread between rounds, and the ring
bytes against the bytes of the resident recording.  Writes the JSON (with the build stamp) to --out and prints it on one line.

    python tools/stream_bench.py                                   # -> profiles/stream_bench.json
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
from csts_amd import GazePredictor, inputs, stream_schedule, stream_window     # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
PER = 800                                           # samples per frame: 24 kHz at 30 fps


def pushes_of(n_frames, chunk):
    return [(min(chunk, n_frames - a), min(chunk, n_frames - a) * PER) for a in range(0, n_frames, chunk)]


def run_stream(predictor, frames, wav, stride, chunk):
    """One replay through GazeStream -> (seconds per push, windows emitted)."""
    s = predictor.stream(stride=stride)
    secs, windows, a = [], 0, 0
    for k, m in pushes_of(frames.shape[0], chunk):
        t0 = time.perf_counter()
        r = s.push(frames[a:a + k], wav[a * PER:a * PER + m])
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        windows += len(r)
        a += k
    return secs, windows, s


def run_compose(predictor, frames, wav, plan, params, schedule):
    """The same windows from a resident recording, one at a time, in the pushes that complete them."""
    observed, inp = int(plan["observed"]), np.asarray(plan["inputs"])
    secs, windows = [], 0
    for ready in schedule:
        t0 = time.perf_counter()
        for w in ready:
            win = stream_window(plan, w)
            o = win["origin"]
            idx = torch.from_numpy(win["frames_idx"].astype(np.int32)).to(frames.device)[None]
            video = inputs.clip_sample(frames, idx, params, 256)
            spec = inputs.stft_logpower(wav[None, o * PER:(o + observed) * PER])[0]
            cols = spec.shape[1]
            cen = np.clip(np.rint(inp / observed * cols), 128, cols - 1 - 128).astype(np.int32)
            audio = inputs.audio_windows_at(spec, torch.from_numpy(cen).to(frames.device)[None])
            predictor.predict_batch({"video": video, "audio": audio})
            windows += 1
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return secs, windows


def summary(rounds):
    """rounds: one list of per-push seconds per round -> medians over the rounds, in ms, and the spread between rounds."""
    def ms(v):
        return round(v * 1e3, 3)
    total = [sum(r) for r in rounds]
    return {"total_ms": ms(statistics.median(total)), "total_round_ms": [ms(v) for v in total],
            "total_round_spread_ms": ms(max(total) - min(total)),
            "push_mean_ms": ms(statistics.median([statistics.mean(r) for r in rounds])),
            "push_median_ms": ms(statistics.median([statistics.median(r) for r in rounds])),
            "push_worst_ms": ms(statistics.median([max(r) for r in rounds])),
            "push_worst_round_spread_ms": ms(max(max(r) for r in rounds) - min(max(r) for r in rounds))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=450)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/stream_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", args.compute])
    N, H, W = args.frames, 360, 480
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * PER, generator=g, device=dev)
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    params = torch.tensor([predictor._video_params_row(H, W)], dtype=torch.int32, device=dev)
    out = {"tool": "stream_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "compute": args.compute,
           "frames": N, "H": H, "W": W, "build": build_stamp.current(), "configs": []}
    for stride in (9, None):
        for chunk in (1, 8):
            secs, windows, s = run_stream(predictor, frames, wav, stride, chunk)          # warm-up: captures the graph
            pushes = pushes_of(N, chunk)
            schedule = stream_schedule(s.plan, pushes)
            run_compose(predictor, frames, wav, s.plan, params, schedule)
            times = {"stream": [], "compose": []}
            for _ in range(args.rounds):
                a, wa, _ = run_stream(predictor, frames, wav, stride, chunk)
                b, wb = run_compose(predictor, frames, wav, s.plan, params, schedule)
                assert wa == wb == windows == sum(len(x) for x in schedule)
                times["stream"].append(a)
                times["compose"].append(b)
            res = {k: summary(v) for k, v in times.items()}
            out["configs"].append({"stride": int(s.plan["stride"]), "chunk": chunk, "pushes": len(pushes), "windows": windows,
                                   **res, "compose_over_stream_total": round(res["compose"]["total_ms"] / res["stream"]["total_ms"], 3)})
            out["memory"] = {**s.capacity, "ring_bytes": s.capacity["crop_bytes"] + s.capacity["spec_bytes"],
                             "resident_recording_bytes": N * H * W * 3 + N * PER * 4,
                             "resident_bytes_per_frame": H * W * 3 + PER * 4}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
