"""Data-parallel training with SOLVER.OPTIMIZING_METHOD sgd: two fresh processes share cuda:0 over gloo and run the
SegmentedTrainStep chain with FusedSGD (averaged flat buckets, factor exchange of the fusion-conv gradients, momentum buffers);
after two steps both replicas are bit-identical and equal ONE process running the same chain on the concatenated B = 2 batch
(tools/train_avgaze_net.py:70-109 under DDP)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _run(tmp_path, world, timeout=900):
    port = _free_port()
    outs = [str(tmp_path / f"w{world}_rank{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_sgd_worker.py"), str(r), str(world), port, outs[r]],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            logs.append(out)
    finally:
        for p in procs:                      # exactly the children started above
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"world {world} rank {r} failed (code {p.returncode}):\n{logs[r][-4000:]}"
    return [np.load(o, allow_pickle=False) for o in outs]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_two_process_sgd_equals_single_process(tmp_path):
    (ref,) = _run(tmp_path, 1)
    r0, r1 = _run(tmp_path, 2)
    for k in ("delta_heads", "buf_heads", "param_sum", "buf_set"):
        assert np.array_equal(r0[k], r1[k]), k                                    # replicas bit-identical
    assert int(r0["steps"]) == int(ref["steps"]) == 2
    assert np.array_equal(r0["buf_set"], ref["buf_set"]) and float(ref["buf_set"].min()) == 1.0
    # EgoNCE over the gathered embeddings is the global value; KLDiv is per rank, its mean is the batch mean
    for s in range(2):
        assert abs(float(r0["losses"][s, 2]) - float(ref["losses"][s, 2])) < 1e-3
        assert abs(0.5 * (float(r0["losses"][s, 1]) + float(r1["losses"][s, 1])) - float(ref["losses"][s, 1])) < 1e-4
    assert abs(float(r0["clip_norm"]) - float(ref["clip_norm"])) < 1e-3 * float(ref["clip_norm"])
    e_delta, e_buf = _rel(r0["delta_heads"], ref["delta_heads"]), _rel(r0["buf_heads"], ref["buf_heads"])
    print(f"\n[sgd, 2 processes vs 1] update rel-L2 {e_delta:.2e}, momentum buffer rel-L2 {e_buf:.2e}")
    assert e_delta < 5e-3 and e_buf < 5e-3
