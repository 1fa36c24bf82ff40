"""Child process of tests/test_gpu_optim_model.py (not a test module): CSTS_AMD.COMPUTE fp16 (libcsts_hip_f16.so + dynamic loss
scaling inside the optimizer kernels) with SOLVER.OPTIMIZING_METHOD sgd / adam and SOLVER.CLIP_GRAD_VAL -- a configuration the
stock torch optimizers cannot train (no GradScaler) -- builds the fused optimizer and takes finite steps, eager and as a HIP
graph.  Writes a JSON document of measured quantities to argv[1]."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd.config import load_yaml           # noqa: E402
from csts_amd.build import build_model          # noqa: E402
from csts_amd import train as T                 # noqa: E402
from csts_amd import optim as OPT               # noqa: E402
from oracle import csts_oracle as O             # noqa: E402  (test infrastructure)

DEV = torch.device("cuda:0")


def case(method, extra):
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", "fp16",
                     "SOLVER.OPTIMIZING_METHOD", method, "SOLVER.BASE_LR", 0.01 if method == "sgd" else 1e-4] + list(extra))
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(8, 256), strict=True)
    m.eval()
    opt = T.construct_optimizer(m, cfg, capturable=True)
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 8, 256, seed=99).items()}
    w = m.blocks[5].mlp.fc1.weight
    w0 = w.detach().clone()
    # the loss scale starts at 65536 (GradScaler's default): the first steps may overflow in fp16 and be skipped on the device
    losses = [float(T.train_step(cfg, m, batch, opt, lr=cfg.SOLVER.BASE_LR)[0]) for _ in range(4)]
    g = T.GraphedTrainStep(cfg, m, opt, batch, warmup=1)
    losses += [float(g.run(batch, lr=cfg.SOLVER.BASE_LR)[0]) for _ in range(2)]
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
    r = {"type": type(opt).__name__, "fused": isinstance(opt, OPT.FusedOptimizer), "clip_value": opt.clip_value,
         "max_grad_norm": opt.max_grad_norm, "loss_scale": float(opt.loss_scale), "losses": losses, "params_finite": finite,
         "steps": opt.step_count(), "moved": float((w.detach() - w0).abs().max())}
    del g, opt, m
    torch.cuda.empty_cache()
    return r


def main():
    res = {"sgd_value_clip": case("sgd", ["SOLVER.MOMENTUM", 0.9, "SOLVER.CLIP_GRAD_VAL", 0.5]),
           "adam": case("adam", [])}
    json.dump(res, open(sys.argv[1], "w"))


if __name__ == "__main__":
    main()
