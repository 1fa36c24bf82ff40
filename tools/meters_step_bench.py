"""Step time of the benchmark configuration (b = 4, 16 x 256^2, bf16, one GPU, the whole iteration as one HIP graph) with and
without the device-resident gaze meter in the captured step ("Gaze meters"): two GraphedTrainSteps in ONE process,
alternated over several rounds, so that clock and thermal drift hit both alike.  Reports the median step time of each variant,
the spread of the per-round medians of the same variant, and the on-minus-off difference.  Prints one JSON line.

    python tools/meters_step_bench.py                      # both variants, alternated
    python tools/meters_step_bench.py --variant off        # one variant alone (for a kernel trace: tools/step_kernel_counts.py)
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd.config import load_yaml           # noqa: E402
from csts_amd.build import build_model          # noqa: E402
from csts_amd import metrics, train as T        # noqa: E402


def timed(step, batch, lr, n):
    times = []
    for _ in range(n):                      # one event pair per step: the per-step distribution, not only the mean
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step.run(batch, lr=lr)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="both", choices=["both", "on", "off"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant per round")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", args.frames, "CSTS_AMD.COMPUTE", args.compute])
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    model.train()
    batch = T.synthetic_batch(args.batch, args.frames, 256, 1000, dev)
    lr = T.get_lr_at_epoch(cfg, 0.0)
    steps, meter = {}, None
    for name in (["off", "on"] if args.variant == "both" else [args.variant]):
        m = copy.deepcopy(model) if args.variant == "both" else model
        if name == "on":
            meter = metrics.GazeMeter(cfg.TRAIN.DATASET, cfg.LOG_PERIOD, dev, "train")
        steps[name] = T.GraphedTrainStep(cfg, m, T.construct_optimizer(m, cfg, capturable=True), batch,
                                         meter=meter if name == "on" else None)
    for s in steps.values():
        for _ in range(args.warmup):
            s.run(batch, lr=lr)
    torch.cuda.synchronize()
    rounds = {k: [] for k in steps}
    for _ in range(args.rounds):
        for name, s in steps.items():
            rounds[name].append(timed(s, batch, lr, args.steps))
    out = {"tool": "meters_step_bench", "batch": args.batch, "frames": args.frames, "compute": args.compute,
           "rounds": args.rounds, "steps_per_round": args.steps}
    for name, rs in rounds.items():
        meds = [statistics.median(r) for r in rs]
        out[name] = {"median_step_ms": round(statistics.median([t for r in rs for t in r]), 4),
                     "round_medians_ms": [round(v, 4) for v in meds], "round_spread_ms": round(max(meds) - min(meds), 4)}
    if len(rounds) == 2:
        out["on_minus_off_ms"] = round(out["on"]["median_step_ms"] - out["off"]["median_step_ms"], 4)
    if meter is not None:
        out["meter_iterations"] = meter.iterations()
        out["meter_window_median"] = meter.window_median()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
