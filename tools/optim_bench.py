"""Time of ONE device-fused optimizer step (clip norm + update + bf16 shadow refresh, with the three fusion-conv weights updated
from their rank-(B T') factors) on the real CSTS parameter set, for each SOLVER.OPTIMIZING_METHOD: the step is captured into a HIP
graph and replayed.  Gradients are synthetic (the optimizer streams them the same whatever their values).  Prints one JSON line
per method with the step time and the bytes per parameter of the update (optim.hip row).  Under
`rocprofv3 --kernel-trace --stats -- python tools/optim_bench.py` the per-kernel times and launch counts of one step follow.

    python tools/optim_bench.py [--methods adamw,adam,sgd,sgd0] [--steps 50]
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
from csts_amd import lib as L, train as T       # noqa: E402

# bytes per parameter of the update pass (fp32 p / g / buffers, 16-bit shadow): DESIGN.md, optim.hip row
BYTES = {"adamw": 30, "adam": 30, "sgd": 22, "sgd0": 14}
METHOD = {"adamw": ("adamw", []), "adam": ("adam", []), "sgd": ("sgd", ["SOLVER.MOMENTUM", 0.9]), "sgd0": ("sgd", ["SOLVER.MOMENTUM", 0.0])}


def run(name, model, cfg0, rows, steps, warmup):
    method, extra = METHOD[name]
    cfg = cfg0.clone()
    cfg.merge_from_list(["SOLVER.OPTIMIZING_METHOD", method, "SOLVER.NESTEROV", False] + extra)
    opt = T.construct_optimizer(model, cfg, capturable=True)
    dev = opt.device
    fac = []
    for n in ("vision_pool", "audio_pool", "audio_pool2"):
        w = getattr(model, n).weight
        N, K = w.shape[0], w.numel() // w.shape[0]
        fac.append((w, torch.randn(rows, N, device=dev) * 1e-3, torch.randn(rows, K, device=dev).to(L.half_dtype())))
    fid = {id(w) for w, _, _ in fac}
    for p in opt.params:
        p.grad = None if id(p) in fid else torch.randn_like(p) * 1e-3
    opt.set_factored(fac)
    snap = [p.detach().clone() for p in opt.params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    opt.refill_capture_pool()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    for _ in range(warmup):
        g.replay()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    with torch.no_grad():
        for p, s in zip(opt.params, snap):
            p.copy_(s)
    n = opt.n_total
    ms = statistics.median(times)
    print(json.dumps({"method": name, "optimizer": type(opt).__name__, "params": n, "factored_rows": rows, "step_ms_median": round(ms, 4),
                      "step_ms_min": round(min(times), 4), "update_bytes_per_param": BYTES[name],
                      "update_bytes_GB": round(n * BYTES[name] / 1e9, 3)}), flush=True)
    opt.set_factored(None)
    for p in opt.params:
        p.grad = None
    del g, opt
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--methods", default="adamw,adam,sgd,sgd0")
    ap.add_argument("--rows", type=int, default=32, help="factored token rows B * T' (32: b = 4 at 16 frames)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 16, "CSTS_AMD.COMPUTE", "bf16"])
    model = build_model(cfg)
    for name in args.methods.split(","):
        run(name, model, cfg, args.rows, args.steps, args.warmup)


if __name__ == "__main__":
    main()
