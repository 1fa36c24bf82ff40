"""Whole-model training with SOLVER.OPTIMIZING_METHOD sgd / adam (slowfast/models/optimizer.py:82-108) through the device-fused
optimizers: the HIP-graph replay of the iteration equals eager execution, and the fp16 compute mode (dynamic loss scaling inside
the optimizer kernels) trains with sgd + SOLVER.CLIP_GRAD_VAL, which the stock torch optimizers cannot do."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd.config import load_yaml              # noqa: E402
from csts_amd.build import build_model             # noqa: E402
from csts_amd import optim as OPT, train as T      # noqa: E402
from oracle import csts_oracle as O                # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")


def test_graphed_sgd_train_step_matches_eager():
    """T8 B2, bf16 mode, sgd (momentum 0.9, nesterov) with the YAML's L2 clip: three HIP-graph replays == three eager steps --
    losses, weights, momentum buffers and their first-step flags (the graph's warm-up steps are undone, so the first replay
    initialises the buffers like the first eager step)."""
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", "bf16",
                           "SOLVER.OPTIMIZING_METHOD", "sgd", "SOLVER.BASE_LR", 0.01, "SOLVER.MOMENTUM", 0.9, "SOLVER.NESTEROV", True])
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(8, 256), strict=True)
    m.eval()
    m2 = copy.deepcopy(m)
    batch = T.synthetic_batch(2, 8, 256, 99, DEV)
    opt_e = T.construct_optimizer(m, cfg)
    opt_g = T.construct_optimizer(m2, cfg, capturable=True)
    assert type(opt_e) is OPT.FusedSGD and opt_e.momentum == 0.9 and opt_e.nesterov and opt_e.max_grad_norm == 1.0
    g = T.GraphedTrainStep(cfg, m2, opt_g, batch, warmup=1)
    assert float(opt_g.buf_step_t.abs().sum()) == 0.0 and opt_g.step_count() == 0       # warm-up undone
    le = [float(T.train_step(cfg, m, batch, opt_e, lr=0.01)[0]) for _ in range(3)]
    lg = [float(g.run(batch, lr=0.01)[0]) for _ in range(3)]
    assert abs(le[0] - lg[0]) < 1e-4 and abs(le[1] - lg[1]) < 5e-3 and abs(le[2] - lg[2]) < 5e-3, (le, lg)
    assert le[2] != le[0]
    w_e, w_g = m.blocks[5].mlp.fc1.weight, m2.blocks[5].mlp.fc1.weight
    assert rel_l2(w_g, w_e) < 1e-3
    assert rel_l2(opt_g.momentum_buffer, opt_e.momentum_buffer) < 5e-2
    assert torch.equal(opt_g.buf_step_t, opt_e.buf_step_t) and float(opt_e.buf_step_t.min()) == 1.0     # every buffer set by step 1
    assert opt_e.step_count() == opt_g.step_count() == 3
    fac = getattr(opt_e, "last_factored_params", [])
    assert len(fac) == 3                                 # the fusion-conv weights took the factored sgd update


def test_fp16_mode_trains_with_sgd_value_clip_and_adam(tmp_path):
    out = tmp_path / "fp16_optim.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CSTS_HALF")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fp16_optim_worker.py"), str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    r = json.load(open(out))
    s = r["sgd_value_clip"]
    assert s["type"] == "FusedSGD" and s["fused"] and s["clip_value"] == 0.5 and s["max_grad_norm"] == 0.0
    a = r["adam"]
    assert a["type"] == "FusedAdam" and a["fused"]
    for c in (s, a):
        assert all(np.isfinite(c["losses"])) and c["params_finite"] and c["moved"] > 0.0, c
        assert c["loss_scale"] >= 1.0 and 1 <= c["steps"] <= 6 and len(c["losses"]) == 6, c
