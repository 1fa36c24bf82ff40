"""One rank of the data-parallel sgd test (tests/test_gpu_dist_sgd.py starts it as a FRESH child process; it is not a test
module).  WORLD 2: the rank joins a gloo group on cuda:0 (like tests/dp_worker.py) and runs csts_amd.train.SegmentedTrainStep
with SOLVER.OPTIMIZING_METHOD sgd (FusedSGD: momentum 0.9, dampening 0.1) on ITS OWN clip of the seed-1000 B=2 batch.  WORLD 1:
the same chain in one process on the whole B=2 batch, the reference the two ranks must equal.  Two real steps (the second
continues the momentum buffers); per-parameter update heads, momentum-buffer heads, checksums and losses go to OUT.npz.

    python tests/dp_sgd_worker.py RANK WORLD PORT OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    from csts_amd import train as T, ops, optim as OPT, distributed as du
    from oracle import csts_oracle as O               # test infrastructure: seeded weights + the fixture's batch

    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", "fp32",
                     "CSTS_AMD.TRUNK_CUT", 3, "SOLVER.OPTIMIZING_METHOD", "sgd", "SOLVER.BASE_LR", 0.01, "SOLVER.MOMENTUM", 0.9,
                     "SOLVER.DAMPENING", 0.1, "SOLVER.NESTEROV", False])
    core = build_model(cfg)
    core.load_state_dict(O.seeded_params(8, 256), strict=True)
    core.eval()                                        # drop-path off
    model = du.GradAllReduce(core, bucket_mb=cfg.CSTS_AMD.GRAD_BUCKET_MB) if world > 1 else core
    full = O.synthetic_batch(2, 8, 256, seed=1000)
    sl = slice(rank, rank + 1) if world > 1 else slice(0, 2)
    batch = {k: v[sl].contiguous().to(dev) for k, v in full.items() if k in ("video", "audio", "labels_hm")}
    opt = T.construct_optimizer(model, cfg, capturable=True)
    assert type(opt) is OPT.FusedSGD and opt.max_grad_norm == 1.0 and opt.momentum == 0.9
    step = T.SegmentedTrainStep(cfg, model, opt, batch, warmup=1)
    assert step.dist == (world > 1) and step.use_graphs
    p0 = [p.detach().clone() for p in core.parameters()]
    losses = []
    for _ in range(2):
        loss, kld, nce = step.run(batch, lr=0.01)
        losses.append([float(loss), float(kld), float(nce)])
    torch.cuda.synchronize()
    params = list(core.parameters())
    idx = {id(p): i for i, p in enumerate(opt.params)}
    res = {"losses": np.array(losses), "steps": opt.step_count(), "clip_norm": float(opt.grad_norm),
           "delta_heads": torch.cat([(p.detach() - q).reshape(-1)[:256] for p, q in zip(params, p0)]).cpu().numpy(),
           "buf_heads": torch.cat([opt._m[idx[id(p)]][:256] for p in params]).cpu().numpy(),
           "buf_set": opt.buf_step_t.cpu().numpy(),
           "param_sum": np.array([float(p.detach().double().sum()) for p in params])}
    np.savez(out, **res)
    ops.reset_deferred()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
