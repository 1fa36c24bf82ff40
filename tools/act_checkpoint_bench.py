"""Cost and benefit of MODEL.ACT_CHECKPOINT ("Activation checkpointing"): for the benchmark configuration (b = 4,
16 x 256^2, bf16, the whole iteration as one HIP graph) and for 32 x 256^2 (Aria YAML, b = 1), the graph-replayed step time and
torch.cuda.max_memory_allocated() of one step with the key off and on.  Every configuration runs in a fresh child process under
its own time limit; the first failure ends the run.  bench.py takes no config overrides, so this tool builds the same model and
step itself.  Writes profiles/act_checkpoint_bench.json and prints it.

    python tools/act_checkpoint_bench.py                 # the four configurations
    python tools/act_checkpoint_bench.py --max-batch     # + the largest batch (16 x 256^2) that completes a step, key off and on

--max-batch doubles the batch from a size known to fit and never runs into an out-of-memory fault on purpose: the peak is
predicted linearly in the batch from the last two measured sizes, and the search stops at the first size whose prediction
exceeds 80 % of the card.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"bench": ("configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml", 16, 4),
           "T32": ("configs/Aria/CSTS_Aria_Gaze_Forecast.yaml", 32, 1)}


def child(args):
    import torch
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    from csts_amd import train as T
    yaml, frames, batch = CONFIGS[args.config]
    batch = args.batch or batch
    dev = torch.device("cuda:0")
    cfg = load_yaml(os.path.join(ROOT, yaml), ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", frames,
                                               "CSTS_AMD.COMPUTE", "bf16", "MODEL.ACT_CHECKPOINT", bool(args.on)])
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    model.train()
    data = T.synthetic_batch(batch, frames, 256, 1000, dev)
    opt = T.construct_optimizer(model, cfg, capturable=True)
    torch.cuda.reset_peak_memory_stats()
    step = T.GraphedTrainStep(cfg, model, opt, data)
    lr = T.get_lr_at_epoch(cfg, 0.0)
    for _ in range(args.warmup):
        step.run(lr=lr)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step.run(lr=lr)[0]
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    # the graph's private pool holds the step's activations: the peak over warm-up, capture and replays is the step's footprint
    print(json.dumps({"config": args.config, "act_checkpoint": bool(args.on), "batch": batch, "frames": frames, "steps": args.steps,
                      "median_step_ms": round(statistics.median(times), 3), "min_step_ms": round(times[0], 3),
                      "p90_step_ms": round(times[int(0.9 * (len(times) - 1))], 3),
                      "max_memory_allocated": int(torch.cuda.max_memory_allocated()),
                      "total_memory": int(torch.cuda.get_device_properties(0).total_memory),
                      "loss": float(loss), "finite": bool(torch.isfinite(loss))}))


def run_child(config, on, batch, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", config, "--on", str(int(on)), "--batch", str(batch or 0),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
    if p.returncode != 0:
        raise SystemExit(f"{config} act_checkpoint={on} batch={batch}: exit code {p.returncode}\n{p.stderr[-3000:]}")
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    if not rec["finite"]:
        raise SystemExit(f"{config} act_checkpoint={on}: loss is not finite")
    return rec


def max_batch(on, args):
    """Doubling from the benchmark's own batch; stops before a size whose predicted peak exceeds 80 % of the card."""
    sizes = []
    b = CONFIGS["bench"][2]
    while True:
        rec = run_child("bench", on, b, args)
        sizes.append((b, rec["max_memory_allocated"], rec["median_step_ms"]))
        limit = 0.8 * rec["total_memory"]
        if len(sizes) < 2:
            (b0, m0) = (0, 0)
        else:
            b0, m0 = sizes[-2][:2]
        slope = (sizes[-1][1] - m0) / (sizes[-1][0] - b0)
        predicted = sizes[-1][1] + slope * b          # peak at 2 b
        if predicted > limit:
            return {"act_checkpoint": on, "largest_batch_run": b, "sizes": sizes, "predicted_peak_at_next": int(predicted), "limit": int(limit)}
        b *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--config", default="bench", choices=sorted(CONFIGS))
    ap.add_argument("--on", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    ap.add_argument("--max-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_checkpoint_bench.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"tool": "act_checkpoint_bench", "runs": []}
    for config in ("bench", "T32"):
        for on in (False, True):
            result["runs"].append(run_child(config, on, 0, args))
        off, on_ = result["runs"][-2:]
        result[config] = {"step_ms_off": off["median_step_ms"], "step_ms_on": on_["median_step_ms"],
                          "step_ratio": round(on_["median_step_ms"] / off["median_step_ms"], 4),
                          "peak_gib_off": round(off["max_memory_allocated"] / 2 ** 30, 3),
                          "peak_gib_on": round(on_["max_memory_allocated"] / 2 ** 30, 3),
                          "peak_ratio": round(on_["max_memory_allocated"] / off["max_memory_allocated"], 4)}
    if args.max_batch:
        result["max_batch"] = [max_batch(False, args), max_batch(True, args)]
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


if __name__ == "__main__":
    main()
