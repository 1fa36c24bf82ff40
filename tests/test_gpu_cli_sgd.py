"""tools/run_net.py with SOLVER.OPTIMIZING_METHOD sgd (the reference's default method, slowfast/models/optimizer.py:83-91) in
fresh child processes: one epoch from a HIP graph with FusedSGD, a checkpoint whose "optimizer_state" is torch.optim.SGD's
(momentum buffers; slowfast/utils/checkpoint.py:131) and loads into a torch.optim.SGD over the same parameters, then a second
invocation that auto-resumes from it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
STEPS = 4
SGD = ["SOLVER.OPTIMIZING_METHOD", "sgd", "SOLVER.BASE_LR", "0.01", "SOLVER.MOMENTUM", "0.9", "SOLVER.DAMPENING", "0.0",
       "SOLVER.NESTEROV", "True"]


def _run_net(out_dir, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_net.py"), "--cfg", YAML,
           "NUM_GPUS", "1", "TRAIN.BATCH_SIZE", "4", "MODEL.LOSS_FUNC", "kldiv+egonce", "MODEL.LOSS_ALPHA", "0.05",
           "TRAIN.MIXED_PRECISION", "True", "CSTS_AMD.STEPS_PER_EPOCH", str(STEPS), "CSTS_AMD.SAVE_CHECKPOINTS", "True",
           "TRAIN.CHECKPOINT_PERIOD", "1", "TRAIN.EVAL_PERIOD", "100", "CSTS_AMD.EPOCHS_THIS_RUN", "1", "LOG_PERIOD", "1",
           "TEST.ENABLE", "False", "OUTPUT_DIR", str(out_dir)] + SGD + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert recs, p.stdout[-2000:]
    return recs


def _of(recs, kind):
    return [r for r in recs if r["_type"] == kind]


def test_run_net_sgd_checkpoint_holds_torch_sgd_state_and_resumes(tmp_path):
    recs = _run_net(tmp_path)
    start = _of(recs, "train_start")[0]
    assert start["resumed"] is False and start["optimizer_steps"] == 0
    iters = _of(recs, "train_iter")
    assert len(iters) == STEPS and all(np.isfinite(r["loss"]) for r in iters)
    assert all(abs(r["lr_device"] - r["lr"]) <= 2e-6 * r["lr"] for r in iters)       # the captured kernels read the schedule
    ck = _of(recs, "checkpoint")
    assert len(ck) == 1 and ck[0]["optimizer_steps"] == STEPS
    path = os.path.join(str(tmp_path), "checkpoints", "checkpoint_epoch_00001.pyth")
    sd = torch.load(path, map_location="cpu", weights_only=False)
    ost = sd["optimizer_state"]
    g0 = ost["param_groups"][0]
    assert g0["momentum"] == 0.9 and g0["dampening"] == 0.0 and g0["nesterov"] is True
    # the state loads into torch.optim.SGD over the same parameters (the reference's construct_optimizer + load_checkpoint); its
    # indices are positions in the parameter groups; a parameter that has had a gradient holds a momentum buffer of its shape
    from csts_amd.config import load_yaml
    from csts_amd.build import build_model
    from csts_amd.train import construct_optimizer
    cfg = load_yaml(YAML, ["NUM_GPUS", 0, "MODEL.LOSS_FUNC", "kldiv+egonce"] + SGD)
    m = build_model(cfg)
    m.load_state_dict(sd["model_state"], strict=True)
    opt = construct_optimizer(m, cfg, device_fused=False)
    assert type(opt) is torch.optim.SGD
    params = [p for g in opt.param_groups for p in g["params"]]
    assert len(ost["state"]) == len(params) == len(sd["model_state"])
    bufs = [ost["state"][i]["momentum_buffer"] for i in range(len(params))]
    assert all("exp_avg" not in ost["state"][i] for i in range(len(params)))
    assert all(b is None or tuple(b.shape) == tuple(p.shape) for b, p in zip(bufs, params))
    assert sum(b is not None for b in bufs) >= 0.95 * len(params)
    assert float(sum(float(b.abs().sum()) for b in bufs if b is not None)) > 0.0
    opt.load_state_dict(ost)
    w = m.blocks[3].mlp.fc1.weight
    assert torch.equal(opt.state[w]["momentum_buffer"], ost["state"][[id(p) for p in params].index(id(w))]["momentum_buffer"])
    first_w = sd["model_state"]["blocks.3.mlp.fc1.weight"].clone()
    del sd, ost, opt, m

    recs2 = _run_net(tmp_path)
    start2 = _of(recs2, "train_start")[0]
    assert start2["resumed"] is True and start2["start_epoch"] == 2 and start2["optimizer_steps"] == STEPS
    iters2 = _of(recs2, "train_iter")
    assert len(iters2) == STEPS and all(np.isfinite(r["loss"]) and r["epoch"] == 2 for r in iters2)
    ck2 = _of(recs2, "checkpoint")
    assert len(ck2) == 1 and ck2[0]["optimizer_steps"] == 2 * STEPS
    sd2 = torch.load(os.path.join(str(tmp_path), "checkpoints", "checkpoint_epoch_00002.pyth"), map_location="cpu", weights_only=False)
    assert not torch.equal(sd2["model_state"]["blocks.3.mlp.fc1.weight"], first_w)
    del sd2
    for f in os.listdir(os.path.join(str(tmp_path), "checkpoints")):
        os.remove(os.path.join(str(tmp_path), "checkpoints", f))
