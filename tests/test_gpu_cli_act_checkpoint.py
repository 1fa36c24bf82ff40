"""`tools/run_net.py ... MODEL.ACT_CHECKPOINT True` in a fresh child process: two epochs of three steps from the captured step,
a checkpoint per epoch, then a resume of the same output directory with the key OFF (checkpoints do not depend on the key)."""
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
STEPS = 3


def _run_net(out_dir, key, epochs):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_net.py"), "--cfg", os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
           "NUM_GPUS", "1", "TRAIN.BATCH_SIZE", "2", "MODEL.LOSS_FUNC", "kldiv+egonce", "MODEL.LOSS_ALPHA", "0.05",
           "MODEL.ACT_CHECKPOINT", str(key), "CSTS_AMD.STEPS_PER_EPOCH", str(STEPS), "CSTS_AMD.SAVE_CHECKPOINTS", "True",
           "TRAIN.CHECKPOINT_PERIOD", "1", "TRAIN.EVAL_PERIOD", "100", "TEST.ENABLE", "False", "CSTS_AMD.EPOCHS_THIS_RUN", str(epochs),
           "LOG_PERIOD", "1", "OUTPUT_DIR", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)       # a failed child ends the test
    assert p.returncode == 0, p.stderr[-4000:]
    recs = [json.loads(ln[len("json_stats: "):]) for ln in p.stdout.splitlines() if ln.startswith("json_stats: ")]
    assert recs, p.stdout[-2000:]
    return recs, p.stdout + p.stderr


def _of(recs, kind):
    return [r for r in recs if r["_type"] == kind]


def test_run_net_trains_with_the_key_on_and_resumes_with_it_off(tmp_path):
    recs, text = _run_net(tmp_path, True, 2)
    assert "not applied" not in text
    start = _of(recs, "train_start")[0]
    assert start["start_epoch"] == 1 and start["resumed"] is False and start["optimizer_steps"] == 0
    iters = _of(recs, "train_iter")
    assert [(r["epoch"], r["iter"]) for r in iters] == [(e, i) for e in (1, 2) for i in range(1, STEPS + 1)]
    for r in iters:
        assert np.isfinite(r["loss"]) and np.isfinite(r["kldiv_loss"]) and np.isfinite(r["nce_loss"])
    ck = _of(recs, "checkpoint")
    assert [c["optimizer_steps"] for c in ck] == [STEPS, 2 * STEPS]
    recs2, text2 = _run_net(tmp_path, False, 1)
    assert "not applied" not in text2
    start2 = _of(recs2, "train_start")[0]
    assert start2["start_epoch"] == 3 and start2["resumed"] is True and start2["optimizer_steps"] == 2 * STEPS
    iters2 = _of(recs2, "train_iter")
    assert len(iters2) == STEPS and all(r["epoch"] == 3 and np.isfinite(r["loss"]) for r in iters2)


def test_two_ranks_with_the_key_on_equal_the_reference_fixture(tmp_path):
    """Two fresh processes on one GPU over gloo, the data-parallel graph chain (TRUNK_CUT 3) with the key on, one clip each: the
    averaged gradients the optimizer reads equal the reference's single-process B = 2 fixture at the bars of
    tests/test_gpu_dist.py; the replicas stay bit-identical after one real update."""
    import socket
    from conftest import GOLDEN
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    here = os.path.dirname(os.path.abspath(__file__))
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "act_checkpoint_dp_worker.py"), str(r), "2", port, "3", "fp32", outs[r]],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=900)
            logs.append(out)
    finally:
        for p in procs:                      # exactly the children started above
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed (code {p.returncode}):\n{logs[r][-4000:]}"
    r0, r1 = [np.load(o, allow_pickle=False) for o in outs]
    g = np.load(os.path.join(GOLDEN, "model_T8_B2.npz"), allow_pickle=False)
    assert int(r0["n_buckets"]) == 3
    assert abs(float(r0["nce"]) - float(r1["nce"])) < 1e-6 and abs(float(r0["nce"]) - float(g["nce"])) < 1e-3
    assert abs(0.5 * (float(r0["kld"]) + float(r1["kld"])) - float(g["kld"])) < 1e-4
    assert abs(0.5 * (float(r0["loss"]) + float(r1["loss"])) - float(g["loss"])) < 1e-4
    assert np.array_equal(r0["grad_norms"], r1["grad_norms"])
    norm_of = dict(zip([str(n) for n in r0["grad_names"]], r0["grad_norms"]))
    for n, ref_norm in zip([str(x) for x in g["grad_names"]], g["grad_norms"]):
        if n == "classifier.bias":
            continue
        assert abs(norm_of[n] - ref_norm) / ref_norm <= 2e-3, (n, norm_of[n], ref_norm)
        ref_slice = g[n.replace(".", "_") + "_g"]
        sl = r0["g__" + n][:ref_slice.size]
        assert np.array_equal(sl, r1["g__" + n][:ref_slice.size]), n
        e = np.linalg.norm(sl.astype(np.float64) - ref_slice) / np.linalg.norm(ref_slice.astype(np.float64))
        assert e < 5e-3, (n, e)
    tot, ref_tot = float(r0["grad_total_norm"]), float(g["grad_total_norm"])
    assert abs(tot - ref_tot) < 1e-3 * ref_tot
    assert abs(float(r0["clip_norm_seen"]) - ref_tot) < 1e-3 * ref_tot
    for k in ("param_sum", "param_heads"):
        assert np.array_equal(r0[k], r1[k]), k
    assert np.isfinite(float(r0["loss_b"])) and abs(float(r0["loss_b"]) - float(r0["loss"])) < 1e-5
