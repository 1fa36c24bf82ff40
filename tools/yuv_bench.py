"""4:2:0 frames against packed RGB, measured in ONE process at Ego4D's picture size ("YUV frames"):
1088 x 1080 pictures, 86 observed frames per clip, T 8, S 256, batches of 4 and 8 clips.

  (a) batch_sample   the pixel pass of one batch out of a resident arena: on RGB recordings, on nv12 recordings (sampled in
                     place), and as the composition a caller without the nv12 pass would run: gather the B * T frames, yuv_to_rgb,
                     spatial_sample.  The three give the same bits (checked).  Bytes per call are computed from the shapes: the
                     bytes the kernel stages (two source rows of the crop's span per output row, 3 bytes a pixel; or two luma and two
                     chroma spans, 2 bytes a pixel) and the resident bytes of the arena.
  (b) predict_video  clips/s of GazePredictor.predict_video over one recording, RGB and nv12 (random weights, graphed).
  (c) bench          `python bench.py --gpus 1` in child processes, alternating this tree and (with --parent-tree DIR, a built tree
                     of the parent commit) the parent: the default path is untouched, so the two should agree within their spread.

(a) and (b) alternate their variants over several rounds after a warm-up; a round of (a) times `--steps` calls between two device
events.  Writes the JSON (with the build stamp) to --out and prints it on one line.

    python tools/yuv_bench.py [--parent-tree DIR] [--bench-runs 3]         # -> profiles/yuv_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                                   # noqa: E402
from video_bench import alternate                    # noqa: E402
from csts_amd import GazePredictor, inputs           # noqa: E402
from csts_amd.config import load_yaml                # noqa: E402

YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
H, W, OBSERVED, T, S = 1088, 1080, 86, 8, 256


def note(msg):
    print(f"yuv_bench: {msg}", file=sys.stderr, flush=True)


def bench_runs(trees, runs, steps, warmup):
    """bench.py in child processes, the trees alternating -> per tree the clips/s of every run, their median and spread."""
    res = {k: [] for k in trees}
    for r in range(runs):
        for name, tree in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}:\n{p.stderr[-2000:]}")
            rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append(float(rec.get("clips_per_s", rec.get("value"))))
            note(f"bench.py run {r} in the {name} tree: {res[name][-1]}")
    return {k: {"clips_per_s": v, "median": statistics.median(v), "spread": max(v) - min(v)} for k, v in res.items()}


def span_pixels(row, width):
    """Pixels of a source row the pass stages for one output row under the params row (fp32, as the kernel computes them)."""
    nh, nw, y0, x0, flip = row
    sx = np.float32(width) / np.float32(nw)
    lo = min(int(max((np.float32(x0) + np.float32(0.5)) * sx - np.float32(0.5), np.float32(0))), width - 1)
    hi = min(int(max((np.float32(x0 + S - 1) + np.float32(0.5)) * sx - np.float32(0.5), np.float32(0))) + 1, width - 1)
    return hi - lo + 1


def batch_case(b, dev, args):
    g = torch.Generator(device=dev).manual_seed(b)
    yuv = torch.randint(0, 256, (b, OBSERVED, H * 3 // 2, W), generator=g, device=dev, dtype=torch.uint8)
    rgb = torch.empty(b, OBSERVED, H, W, 3, dtype=torch.uint8, device=dev)
    for i in range(b):
        inputs.yuv_to_rgb(yuv[i], "nv12", out=rgb[i])
    row = inputs.spatial_rule_host(np.zeros((1, T, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
    params = torch.tensor([row] * b, dtype=torch.int32, device=dev)
    idx = torch.from_numpy(np.stack([np.linspace(i, OBSERVED - 1 - i, T).astype(np.int32) for i in range(b)])).to(dev)
    tabs = {}
    for name, per in (("rgb", H * W * 3), ("nv12", H * W * 3 // 2)):
        host = np.array([[i * OBSERVED * per, OBSERVED, H, W] for i in range(b)], dtype=np.int64)
        tabs[name] = (host, torch.from_numpy(host).to(dev))
    out = torch.empty(b, 3, T, S, S, dtype=torch.float32, device=dev)
    gather = (torch.arange(b, device=dev)[:, None] * OBSERVED + idx.long())

    def on_rgb():
        return inputs.batch_sample(rgb.view(-1), tabs["rgb"][1], idx, params, S, tabs["rgb"][0], out=out)

    def on_nv12():
        return inputs.batch_sample(yuv.view(-1), tabs["nv12"][1], idx, params, S, tabs["nv12"][0], out=out, pixel_format="nv12")

    def convert_then_sample():
        frames = yuv.view(b * OBSERVED, H * 3 // 2, W)[gather]                # (b, T, H * 3 / 2, W)
        return inputs.spatial_sample(inputs.yuv_to_rgb(frames, "nv12"), params, S)

    a = on_rgb().clone()
    same = {"nv12_vs_rgb": bool(torch.equal(on_nv12(), a)), "convert_then_sample_vs_rgb": bool(torch.equal(convert_then_sample(), a))}
    res = alternate({"rgb": on_rgb, "nv12": on_nv12, "convert_then_sample": convert_then_sample}, args.warmup, args.steps, args.rounds)
    span = span_pixels(row, W)
    rows = b * T * S
    res["bit_equal"] = same
    res["bytes_per_call"] = {
        "rgb_staged": rows * 2 * span * 3, "nv12_staged": rows * (2 * span + 2 * (2 * (span // 2 + 1))),
        "convert_then_sample": b * T * (H * W * 3 // 2 + H * W * 3) + rows * 2 * span * 3,
        "written": b * 3 * T * S * S * 4, "span_pixels": span,
        "arena_rgb": int(rgb.numel()), "arena_nv12": int(yuv.numel())}
    res["nv12_over_rgb"] = round(res["nv12"]["median_us"] / res["rgb"]["median_us"], 3)
    res["convert_then_sample_over_nv12"] = round(res["convert_then_sample"]["median_us"] / res["nv12"]["median_us"], 3)
    return res


def video_case(dev, args):
    cfg = load_yaml(YAML, ["NUM_GPUS", 1])
    torch.manual_seed(0)
    predictor = GazePredictor(cfg, device=dev, graph=True)
    n = args.video_frames
    g = torch.Generator(device=dev).manual_seed(1)
    yuv = torch.randint(0, 256, (n, H * 3 // 2, W), generator=g, device=dev, dtype=torch.uint8)
    rgb = inputs.yuv_to_rgb(yuv, "nv12")
    wav = 0.1 * torch.randn(n * 800, generator=g, device=dev)
    runs = {"rgb": lambda: predictor.predict_video(rgb, wav, batch=4, return_heatmaps=False),
            "nv12": lambda: predictor.predict_video(yuv, wav, batch=4, return_heatmaps=False, pixel_format="nv12")}
    tracks = {k: fn() for k, fn in runs.items()}                              # warm-up: the graph is captured here
    windows = tracks["rgb"]["windows"]
    same = all(torch.equal(tracks["rgb"][k].nan_to_num(-1.0), tracks["nv12"][k].nan_to_num(-1.0)) for k in ("points", "peak"))
    times = {k: [] for k in runs}
    for _ in range(args.video_rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / 1e3)
    res = {"frames": n, "windows": windows, "bit_equal": bool(same), "recording_bytes": {"rgb": int(rgb.numel()), "nv12": int(yuv.numel())}}
    for k, v in times.items():
        res[k] = {"clips_per_s": [round(windows / t, 2) for t in v], "median_clips_per_s": round(windows / statistics.median(v), 2),
                  "spread_clips_per_s": round(windows / min(v) - windows / max(v), 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50, help="calls between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--video-frames", type=int, default=278, help="frames of the recording of (b): 4 windows at the default stride")
    ap.add_argument("--video-rounds", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built tree of the parent commit: bench.py runs there too")
    ap.add_argument("--bench-runs", type=int, default=3, help="bench.py runs per tree (0: skip)")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/yuv_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    out = {"tool": "yuv_bench", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_round": args.steps,
           "warmup": args.warmup, "build": build_stamp.current(), "picture": [H, W], "observed_frames": OBSERVED, "T": T, "S": S,
           "batch_sample": {}}
    for b in (4, 8):
        out["batch_sample"][f"b{b}"] = batch_case(b, dev, args)
        note(f"batch_sample b {b} done")
        torch.cuda.empty_cache()
    if args.video_rounds > 0:
        out["predict_video"] = video_case(dev, args)
        note("predict_video done")
        torch.cuda.empty_cache()
    if args.bench_runs > 0:
        trees = {"this": ROOT}
        if args.parent_tree:
            trees["parent"] = os.path.abspath(args.parent_tree)
        out["bench"] = bench_runs(trees, args.bench_runs, args.bench_steps, args.bench_warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
