"""One rank of the two-process data-parallel test with MODEL.ACT_CHECKPOINT True (tests/test_gpu_cli_act_checkpoint.py starts it
as a FRESH child process; it is not a test module).  Like tests/dp_worker.py: the real CSTS model on cuda:0, a gloo group,
csts_amd.train.SegmentedTrainStep on this rank's clip of the seed-1000 B=2 batch of tests/golden/model_T8_B2.npz -- here with
every encoder block recomputed inside the captured backward graphs, its gradients produced straight into the flat buckets by
the per-block nested passes.  Writes what the optimizer graph reads (norms, leading slices, losses) and, after one real update,
checksums of every parameter.

    python tests/act_checkpoint_dp_worker.py RANK WORLD PORT TRUNK_CUT COMPUTE OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, trunk_cut, compute, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6]
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    from csts_amd import train as T, ops, distributed as du
    from oracle import csts_oracle as O

    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", compute,
                     "CSTS_AMD.TRUNK_CUT", trunk_cut, "MODEL.ACT_CHECKPOINT", True])
    core = build_model(cfg)
    assert len(core.checkpointed_blocks()) == 20
    core.load_state_dict(O.seeded_params(8, 256), strict=True)
    core.eval()                                        # drop-path off: the fixture is an eval-mode forward + backward
    model = du.GradAllReduce(core, bucket_mb=cfg.CSTS_AMD.GRAD_BUCKET_MB)
    full = O.synthetic_batch(world, 8, 256, seed=1000)
    batch = {k: v[rank:rank + 1].contiguous().to(dev) for k, v in full.items() if k in ("video", "audio", "labels_hm")}
    opt = T.construct_optimizer(model, cfg, capturable=True)
    step = T.SegmentedTrainStep(cfg, model, opt, batch, warmup=1)
    assert step.dist and step.use_graphs and step.trunk_cut == trunk_cut

    loss, kld, nce = step.run(batch, lr=0.0)
    torch.cuda.synchronize()
    res = {"loss": float(loss), "kld": float(kld), "nce": float(nce), "n_buckets": len(step.flat)}
    ptrs = [(f.data_ptr(), f.data_ptr() + f.numel() * 4) for f, _ in step.flat]
    avg = step.averaged_grads()
    names, norms, total = [], [], 0.0
    for n, p in core.named_parameters():
        assert p.grad is not None and any(lo <= p.grad.data_ptr() < hi for lo, hi in ptrs), n      # views of the flat buckets
        g = avg[p].double()
        names.append(n)
        norms.append(float(g.norm()))
        total += float((g * g).sum())
        res["g__" + n] = avg[p].flatten()[:64].float().cpu().numpy()
    res["grad_names"], res["grad_norms"], res["grad_total_norm"] = np.array(names), np.array(norms), total ** 0.5
    res["clip_norm_seen"] = float(opt.grad_norm)
    opt.reset_state()
    loss_b, _, _ = step.run(batch, lr=1e-4)
    torch.cuda.synchronize()
    res["loss_b"] = float(loss_b)
    res["param_sum"] = np.array([float(p.detach().double().sum()) for p in core.parameters()])
    res["param_heads"] = torch.cat([p.detach().reshape(-1)[:256].float() for p in core.parameters()]).cpu().numpy()
    np.savez(out, **res)
    ops.reset_deferred()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
