"""The live gaze track, measured in ONE process ("Live overlay"):

  push        GazeStream.push on the Ego4D forecast plan, bf16, stride 9: a synthetic recording (360 x 480, 24 kHz audio) replayed
              in pushes of 30 frames with the matching audio;
  live        push_live on a stream opened with live="linear": the same windows, plus the rows of the push's 30 frames
              (ops.live_track_add per step, ops.live_track_rows per step);
  live+draw   the same with overlay=True: the 30 frames drawn over as well (render_track on the push's frames);
  recompose   what showing the forecast took before: track_from_windows over ALL windows emitted so far, fill_track, and
              render_track, timed when 10, 100 and 1000 windows have been emitted.  It needs the frames resident and their number.
              Two renders are timed: the whole recording so far, and only the frames of the last push (the least a caller who
              wants the newest frames has to draw; the fold and the fill still run over everything).

The three streams replay the same recording in lockstep, push by push, each push timed with the device drained, in an order that
rotates from push to push (clock and thermal drift hit all alike).  Reports the per-push median / mean / worst over the replay and
over the pushes that completed a window, the cost of live over push, the recomposition at the three lengths, and the ring bytes.
--train-bench PARENT_TREE: also runs `python bench.py` in this tree and in a built checkout of the parent commit, alternating, and
stores their JSON lines as evidence that the training path is untouched.  Writes the JSON (with the build stamp) to --out.

    python tools/live_bench.py                                     # -> profiles/live_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                  # noqa: E402
from csts_amd import GazePredictor, fill_track, track_from_windows     # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
PER, CHUNK, STRIDE = 800, 30, 9                     # samples per frame (24 kHz at 30 fps), frames per push, frames between windows
VARIANTS = ("push", "live", "live_draw")


def ms(v):
    return round(v * 1e3, 3)


def stats(secs):
    return {"pushes": len(secs), "median_ms": ms(statistics.median(secs)), "mean_ms": ms(statistics.mean(secs)),
            "worst_ms": ms(max(secs)), "total_ms": ms(sum(secs))}


def timed(fn, repeats=3):
    """Median seconds of fn() with the device drained before and after."""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def replay(predictor, base, wav, n_pushes, marks, resident):
    """One lockstep replay of the three variants -> (per-variant per-push seconds, per-push window counts, the recomposition
    timings at the marks).  base: the frames the recording cycles through; resident: the recording as the recomposition needs it."""
    streams = {"push": predictor.stream(stride=STRIDE), "live": predictor.stream(stride=STRIDE, live="linear"),
               "live_draw": predictor.stream(stride=STRIDE, live="linear", overlay=True)}
    secs = {k: [] for k in VARIANTS}
    emitted, results, recompose = [], [], {}
    period = base.shape[0] // CHUNK
    for i in range(n_pushes):
        a = (i % period) * CHUNK
        frames, audio = base[a:a + CHUNK], wav[a * PER:(a + CHUNK) * PER]
        got = {}
        for j in range(3):
            name = VARIANTS[(i + j) % 3]
            s = streams[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = s.push(frames, audio) if name == "push" else s.push_live(frames, audio)[0]
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
        assert [r["window"] for r in got["push"]] == [r["window"] for r in got["live"]] == [r["window"] for r in got["live_draw"]]
        emitted.append(len(got["push"]))
        before = len(results)
        results += got["push"]
        for mark in marks:
            if before < mark <= len(results) and resident is not None:
                n = (i + 1) * CHUNK
                known, plan = results[:mark], streams["push"].plan
                track = {}

                def fold():
                    track["t"] = fill_track(track_from_windows(known, n), mode="linear", plan=plan)

                fold_s, _ = timed(fold)
                all_s, _ = timed(lambda: predictor.render_track(resident[:n], track["t"]))
                last = {k: track["t"][k][n - CHUNK:n] for k in ("rescaled", "points")}
                last_s, _ = timed(lambda: predictor.render_track(resident[n - CHUNK:n], last))
                recompose[str(mark)] = {"windows": mark, "frames": n, "fold_and_fill_ms": ms(fold_s), "render_all_ms": ms(all_s),
                                        "render_last_push_ms": ms(last_s), "whole_recording_ms": ms(fold_s + all_s),
                                        "newest_push_only_ms": ms(fold_s + last_s),
                                        "resident_frame_bytes": int(resident[:n].numel())}
    return secs, emitted, recompose, streams


def train_bench(parent, rounds):
    """`python bench.py` here and in the parent's tree, alternating, each in a fresh child process -> their JSON lines."""
    out = {"branch": [], "parent": []}
    for _ in range(rounds):
        for name, tree in (("branch", ROOT), ("parent", parent)):
            p = subprocess.run([sys.executable, "bench.py"], cwd=tree, capture_output=True, text=True, timeout=1500)
            if p.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}:\n{p.stderr[-2000:]}")
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            out[name].append(json.loads(lines[-1]))
            print(f"bench.py in the {name} tree done", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1000, help="emitted windows the replay runs to (the last recomposition mark)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--train-bench", default=None, metavar="PARENT_TREE", help="a built checkout of the parent commit")
    ap.add_argument("--train-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/live_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", args.compute])
    H, W = 360, 480
    marks = sorted({m for m in (10, 100, 1000) if m <= args.windows} | {args.windows})
    n_pushes = -(-(86 + STRIDE * (args.windows - 1)) // CHUNK)           # window w is ready once 86 + 9 w frames are in
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randint(0, 256, (10 * CHUNK, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    wav = 0.1 * torch.randn(10 * CHUNK * PER, generator=g, device=dev)
    resident = base.repeat(-(-n_pushes // 10), 1, 1, 1)[:n_pushes * CHUNK]     # the recording the recomposition keeps
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    replay(predictor, base, wav, 6, (), None)                             # warm-up: the graph, every kernel of the three paths
    out = {"tool": "live_bench", "device": torch.cuda.get_device_name(0), "compute": args.compute, "H": H, "W": W,
           "stride": STRIDE, "chunk": CHUNK, "pushes": n_pushes, "frames": n_pushes * CHUNK, "rounds": args.rounds,
           "build": build_stamp.current(), "rounds_detail": []}
    per_round = {k: [] for k in VARIANTS}
    for r in range(args.rounds):
        secs, emitted, recompose, streams = replay(predictor, base, wav, n_pushes, marks, resident if r == 0 else None)
        busy = [i for i, e in enumerate(emitted) if e]
        detail = {"windows": sum(emitted), "pushes_with_windows": len(busy)}
        for k in VARIANTS:
            detail[k] = {"all": stats(secs[k]), "with_windows": stats([secs[k][i] for i in busy])}
            per_round[k].append(secs[k])
        if r == 0:
            out["recompose"] = recompose
            cap = streams["live"].capacity
            out["memory"] = {**cap, "ring_bytes_without_live": cap["crop_bytes"] + cap["spec_bytes"],
                             "ring_bytes_with_live": cap["crop_bytes"] + cap["spec_bytes"] + cap["track_bytes"],
                             "resident_bytes_per_frame": H * W * 3 + PER * 4}
        out["rounds_detail"].append(detail)
        print(f"replay {r + 1} of {args.rounds} done", file=sys.stderr, flush=True)
    med = {k: statistics.median([statistics.median(r) for r in per_round[k]]) for k in VARIANTS}
    mean = {k: statistics.median([statistics.mean(r) for r in per_round[k]]) for k in VARIANTS}
    out["per_push"] = {k: {"median_ms": ms(med[k]), "mean_ms": ms(mean[k]),
                           "median_round_ms": [ms(statistics.median(r)) for r in per_round[k]],
                           "mean_round_ms": [ms(statistics.mean(r)) for r in per_round[k]]} for k in VARIANTS}
    out["live_over_push_mean_ms"] = ms(mean["live"] - mean["push"])
    out["live_draw_over_push_mean_ms"] = ms(mean["live_draw"] - mean["push"])
    if args.train_bench is not None:
        del predictor
        torch.cuda.empty_cache()
        out["train_bench"] = train_bench(os.path.abspath(args.train_bench), args.train_rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
