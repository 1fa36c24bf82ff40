"""The live attention ring, measured in ONE process ("Live attention"):

  live / live+att            GazeStream.push_live on the Ego4D forecast plan, bf16, stride 9, opened with live="hold" and with
                             live="hold", attention=True: a synthetic 1088 x 1080 recording pushed FRAME BY FRAME with its 800
                             samples, as a camera delivers it;
  draw / draw+att            the same with overlay=True, and with attention_overlay="mean" on top (a second drawn frame per push);
  ops alone                  ops.live_attention_add of one window plus ops.live_attention_rows of one frame on a ring of the
                             stream's size, against the composition the rule is stated by -- ops.attention_track over ALL windows
                             emitted so far, the pick, ops.attention_rescale of the picked map -- with 10, 100 and 1000 windows
                             emitted.  The composition needs every window's audio_attention resident.
  launches                   device kernels of one push that runs no window and of one that runs one, per variant (torch.profiler).

The four streams replay the same recording in lockstep, push by push, each push timed with the device drained, in an order that
rotates from push to push (clock and thermal drift hit all alike); the spread over pushes and over rounds is written down with
every median.  These paths are bound by launch cost and latency: no bandwidth figure is claimed.  Writes the JSON (with the build
stamp) to --out.

    python tools/live_attention_bench.py                           # -> profiles/live_attention_bench.json
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
from csts_amd import GazePredictor, ops, stream_window     # noqa: E402
from csts_amd.config import load_yaml               # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
PER, STRIDE, H, W = 800, 9, 1080, 1088
VARIANTS = {"live": {}, "live_att": {"attention": True}, "draw": {"overlay": True},
            "draw_att": {"overlay": True, "attention": True, "attention_overlay": "mean"}}


def ms(v):
    return round(v * 1e3, 4)


def spread(secs):
    q = sorted(secs)
    return {"n": len(q), "median_ms": ms(statistics.median(q)), "mean_ms": ms(statistics.mean(q)), "min_ms": ms(q[0]),
            "p10_ms": ms(q[len(q) // 10]), "p90_ms": ms(q[(len(q) * 9) // 10]), "max_ms": ms(q[-1])}


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def replay(predictor, base, wav, n_pushes):
    """One lockstep replay of the four variants, frame by frame -> (per-variant per-push seconds, windows per push, streams)."""
    names = list(VARIANTS)
    streams = {k: predictor.stream(stride=STRIDE, live="hold", **kw) for k, kw in VARIANTS.items()}
    secs, emitted = {k: [] for k in names}, []
    for i in range(n_pushes):
        a = i % base.shape[0]
        frame, audio = base[a:a + 1], wav[a * PER:(a + 1) * PER]
        ran = {}
        for j in range(len(names)):
            name = names[(i + j) % len(names)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ran[name] = len(streams[name].push_live(frame, audio)[0])
            torch.cuda.synchronize()
            secs[name].append(time.perf_counter() - t0)
        assert len(set(ran.values())) == 1
        emitted.append(ran["live"])
    return secs, emitted, streams


def count_kernels(fn):
    """Device kernels fn() launches, by torch.profiler; None (and why) where the profiler does not report them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")), None
    except Exception as e:                          # the figure is optional; the timings are not
        return None, f"{type(e).__name__}: {e}"


def launches(predictor, base, wav):
    """Kernels of the push that takes frame 93 (no window ready) and of the one that takes frame 94 (window 1 runs), per variant."""
    out = {}
    for name, kw in VARIANTS.items():
        s = predictor.stream(stride=STRIDE, live="hold", **kw)
        s.push_live(base[:93], wav[:93 * PER])
        quiet, why = count_kernels(lambda: s.push_live(base[93:94], wav[93 * PER:94 * PER]))
        done = []
        busy, why2 = count_kernels(lambda: done.extend(s.push_live(base[94:95], wav[94 * PER:95 * PER])[0]))
        out[name] = {"push_without_window": quiet, "push_with_one_window": busy, "windows_run": len(done), "note": why or why2}
    return out


def ops_alone(plan, marks, repeats, dev):
    """One add + one row on the ring against the re-folding composition with `mark` windows emitted, random audio_attention."""
    heads, Tp, h, w, S, T = 8, 4, 8, 8, 256, 8
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for mark in marks:
        more = repeats + 3                                        # the ring side folds a NEW window per repeat, as a stream does
        every = torch.rand(mark + more, heads, Tp, h, w, generator=g, device=dev)
        later = np.stack([stream_window(plan, i)["frames_idx"] for i in range(mark + more)]).astype(np.int64)
        later_dev = torch.from_numpy(later).to(dev)
        frames, frames_dev = later[:mark], later_dev[:mark].contiguous()
        n = int(frames[-1, -1])                                   # the frame whose step ran the newest window
        ring = ops.live_attention_ring(55, heads, h, w, dev)
        lo = max(0, mark - 8)                                      # the windows whose frames the ring still holds
        ops.live_attention_add(every[lo:mark], later_dev[lo:mark], later[lo:mark], ring, live_from=max(0, n - 8))
        nxt = [mark]

        def ring_ops():
            i = nxt[0]
            nxt[0] += 1
            at = int(later[i, -1])
            ops.live_attention_add(every[i:i + 1], later_dev[i:i + 1], later[i:i + 1], ring, live_from=at - 8)
            return ops.live_attention_rows(ring, at, 1, S, 8)

        column = every[:mark].contiguous()                        # what the composition folds: the windows emitted so far

        def recompose():
            A = ops.attention_track(column, frames_dev, n + 1, T, S)
            count = A["count"][max(0, n - 8):n + 1]
            at = max(0, n - 8) + int(torch.nonzero(count > 0).max())          # the pick reads the counts back
            return ops.attention_rescale(A["mixed"][at:at + 1], S)

        for fn in (ring_ops, recompose):
            timed(fn, 3)
        a, b = timed(ring_ops, repeats), timed(recompose, repeats)
        out[str(mark)] = {"windows": mark, "frames": n + 1, "ring_add_plus_row": spread(a), "refold_pick_rescale": spread(b),
                          "resident_attention_bytes": int(column.numel() * 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=176, help="frames a replay pushes (window w runs with frame 85 + 9 w)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=30, help="timed repeats of the ops-alone measurements")
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_attention_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/live_attention_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", args.compute])
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randint(0, 256, (args.pushes, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    wav = 0.1 * torch.randn(args.pushes * PER, generator=g, device=dev)
    torch.manual_seed(cfg.RNG_SEED)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    replay(predictor, base, wav, 96)                              # warm-up: both graphs, every kernel of the four paths
    out = {"tool": "live_attention_bench", "device": torch.cuda.get_device_name(0), "compute": args.compute, "H": H, "W": W,
           "stride": STRIDE, "frames_per_push": 1, "pushes": args.pushes, "rounds": args.rounds, "build": build_stamp.current(),
           "rounds_detail": []}
    per_round = {k: [] for k in VARIANTS}
    for r in range(args.rounds):
        secs, emitted, streams = replay(predictor, base, wav, args.pushes)
        busy = [i for i, e in enumerate(emitted) if e]
        quiet = [i for i, e in enumerate(emitted) if not e]
        detail = {"windows": sum(emitted)}
        for k in VARIANTS:
            detail[k] = {"without_window": spread([secs[k][i] for i in quiet]), "with_window": spread([secs[k][i] for i in busy])}
            per_round[k].append(secs[k])
        out["rounds_detail"].append(detail)
        if r == 0:
            out["memory"] = streams["live_att"].capacity
        print(f"replay {r + 1} of {args.rounds} done", file=sys.stderr, flush=True)
    med = {k: [statistics.median(r) for r in per_round[k]] for k in VARIANTS}
    mean = {k: [statistics.mean(r) for r in per_round[k]] for k in VARIANTS}
    out["per_push"] = {k: {"median_ms": ms(statistics.median(med[k])), "mean_ms": ms(statistics.median(mean[k])),
                           "median_round_ms": [ms(v) for v in med[k]], "mean_round_ms": [ms(v) for v in mean[k]]} for k in VARIANTS}
    out["attention_over_live_median_ms"] = ms(statistics.median(med["live_att"]) - statistics.median(med["live"]))
    out["attention_over_live_mean_ms"] = ms(statistics.median(mean["live_att"]) - statistics.median(mean["live"]))
    out["attention_overlay_over_draw_median_ms"] = ms(statistics.median(med["draw_att"]) - statistics.median(med["draw"]))
    out["attention_overlay_over_draw_mean_ms"] = ms(statistics.median(mean["draw_att"]) - statistics.median(mean["draw"]))
    out["launches"] = launches(predictor, base, wav)
    out["ops_alone"] = ops_alone(streams["live"].plan, (10, 100, 1000), args.repeats, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
