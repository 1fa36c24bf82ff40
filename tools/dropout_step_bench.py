"""Step time of the benchmark configuration (b = 4, 16 x 256^2, bf16, one GPU, the whole iteration as one HIP graph) at a given
MVIT.DROPOUT_RATE: the cost of the unfused dropout passes ("Element dropout").  bench.py takes no config overrides,
so this tool builds the same model and step itself.  One rate per process; prints one JSON line.

    python tools/dropout_step_bench.py --rate 0.0
    python tools/dropout_step_bench.py --rate 0.1
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd.config import load_yaml           # noqa: E402
from csts_amd.build import build_model          # noqa: E402
from csts_amd import train as T                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "fp32", "fp16"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", args.frames,
                     "CSTS_AMD.COMPUTE", args.compute, "MVIT.DROPOUT_RATE", args.rate])
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg)
    model.train()
    batch = T.synthetic_batch(args.batch, args.frames, 256, 1000, dev)
    opt = T.construct_optimizer(model, cfg, capturable=True)
    step = T.GraphedTrainStep(cfg, model, opt, batch)
    lr = T.get_lr_at_epoch(cfg, 0.0)
    for _ in range(args.warmup):
        step.run(lr=lr)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):             # one event pair per step: the per-step distribution, not only the mean
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step.run(lr=lr)[0]
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    print(json.dumps({"tool": "dropout_step_bench", "rate": args.rate, "batch": args.batch, "frames": args.frames,
                      "compute": args.compute, "steps": args.steps, "median_step_ms": round(statistics.median(times), 3),
                      "min_step_ms": round(times[0], 3), "p90_step_ms": round(times[int(0.9 * (len(times) - 1))], 3),
                      "loss": float(loss), "finite": bool(torch.isfinite(loss))}))


if __name__ == "__main__":
    main()
