"""Child process of tests/test_gpu_dropout.py: one training forward + backward of the fp16 compute mode (libcsts_hip_f16.so) at
MVIT.DROPOUT_RATE 0.1 under torch.manual_seed(21).  One process runs one 16-bit type, so this cannot share pytest's process
with the bf16 checks.  Saves {loss, finite, grads (unscaled, fp64 on the CPU)} to argv[1]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd.config import load_yaml           # noqa: E402
from csts_amd.build import build_model          # noqa: E402
from csts_amd import train as T                 # noqa: E402
from oracle import csts_oracle as O             # noqa: E402  (test infrastructure)

DEV = torch.device("cuda:0")


def main(out_path):
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", "fp16",
                     "MVIT.DROPOUT_RATE", 0.1])
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(8, 256), strict=True)
    m.train()
    batch = {k: v.to(DEV) for k, v in O.synthetic_batch(2, 8, 256, seed=1000).items()}
    scale, finite = 65536.0, False
    for _ in range(8):          # GradScaler semantics by hand: halve the loss scale on overflow (same seed: same masks)
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(21)
        loss, *_ = T.compute_loss(cfg, m, batch["video"], batch["audio"], batch["labels_hm"])
        (loss * scale).backward()
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
        if finite:
            break
        scale *= 0.5
    grads = {n: (p.grad.double() / scale).flatten().cpu() for n, p in m.named_parameters() if p.grad is not None}
    torch.save({"loss": float(loss), "finite": bool(finite) and bool(torch.isfinite(loss)), "grads": grads}, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
