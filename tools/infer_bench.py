"""Forward-only (inference) pass of the benchmark configuration (b = 4, 16 x 256^2, bf16, one GPU), timed both ways in ONE
process ("Inference"):

  (a) eager    model([video], audio) from Python, then losses.frame_softmax, then the per-frame min-max rescale as torch ops:
               the forward-only path as it ran before GraphedEvalStep existed;
  (b) graphed  csts_amd.infer.GraphedEvalStep.run: the same forward and the fused gaze head (csts_gaze_decode) replayed as one
               HIP graph.

After a warm-up the two are alternated over several rounds (clock and thermal drift hit both alike); a round times `--steps`
calls between two device events.  Reports the median of the per-round times per call of each variant and their spread, checks
that both produce the same heat maps, writes the JSON (with the build stamp) to --out and prints it on one line.

    python tools/infer_bench.py                                    # -> profiles/infer_bench.json
    python tools/infer_bench.py --mode head --steps 50             # the head kernels alone on one batch of logits, for
                                                                   #   rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py ...
    python tools/infer_bench.py --merge-kernel-stats <kernel_stats.csv>   # adds that trace's head-kernel rows to --out as "head_kernels"
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import build_stamp                              # noqa: E402
from csts_amd.config import load_yaml           # noqa: E402
from csts_amd.build import build_model          # noqa: E402
from csts_amd import losses, ops, train as T    # noqa: E402
from csts_amd.infer import GraphedEvalStep      # noqa: E402


def rescale_torch(p):
    """tools/test_avgaze_net.py:68-70 as torch ops."""
    mn = p.amin(dim=(-2, -1), keepdim=True)
    mx = p.amax(dim=(-2, -1), keepdim=True)
    return (p - mn) / (mx - mn + 1e-6)


def eager_pass(model, batch):
    p = losses.frame_softmax(model([batch["video"]], batch["audio"]), temperature=2)
    return p, rescale_torch(p)


def time_calls(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def merge_kernel_stats(path, out_path, min_calls):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if int(r["Calls"]) < min_calls:          # the one forward that made the logits, the batch's input kernels
                continue
            rows.append({"kernel": r["Name"], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                         "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {"tool": "infer_bench"}
    doc["head_kernels"] = {"source": "rocprofv3 --kernel-trace --stats, tools/infer_bench.py --mode head (a run of its own)",
                           "rows": rows}
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["head_kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="pass", choices=["pass", "head"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30, help="calls between the two events of one round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_bench.json"))
    ap.add_argument("--merge-kernel-stats", default=None)
    ap.add_argument("--min-calls", type=int, default=50, help="--merge-kernel-stats keeps kernels launched at least this often (= --steps of the traced run)")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out, args.min_calls)
    if not torch.cuda.is_available():
        raise SystemExit("tools/infer_bench.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", args.frames, "CSTS_AMD.COMPUTE", args.compute])
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    model.eval()
    batch = T.synthetic_batch(args.batch, args.frames, 256, 2000, dev)
    with torch.no_grad():
        if args.mode == "head":
            logits = model([batch["video"]], batch["audio"])
            for _ in range(args.steps):
                rescale_torch(losses.frame_softmax(logits, temperature=2))
                ops.gaze_decode(logits, 2.0)
            torch.cuda.synchronize()
            print(json.dumps({"tool": "infer_bench", "mode": "head", "calls": args.steps, "logits": list(logits.shape)}))
            return
        step = GraphedEvalStep(cfg, model, batch)
        variants = {"eager": lambda: eager_pass(model, batch), "graphed": lambda: step.run(batch["video"], batch["audio"])}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        p_e, r_e = eager_pass(model, batch)
        g = step.run(batch["video"], batch["audio"])
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        same = {"preds_rel_l2": rel(g["preds"], p_e), "rescaled_rel_l2": rel(g["rescaled"], r_e)}
        rounds = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                rounds[name].append(time_calls(fn, args.steps))
    out = {"tool": "infer_bench", "batch": args.batch, "frames": args.frames, "compute": args.compute, "rounds": args.rounds,
           "calls_per_round": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "graphed_vs_eager_outputs": same, "build": build_stamp.current()}
    for name, ms in rounds.items():
        out[name] = {"median_ms": round(statistics.median(ms), 4), "round_ms": [round(v, 4) for v in ms],
                     "round_spread_ms": round(max(ms) - min(ms), 4)}
    out["graphed_minus_eager_ms"] = round(out["graphed"]["median_ms"] - out["eager"]["median_ms"], 4)
    if os.path.exists(args.out):            # keep a kernel trace merged earlier
        try:
            old = json.load(open(args.out))
            if "head_kernels" in old:
                out["head_kernels"] = old["head_kernels"]
        except Exception:
            pass
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
