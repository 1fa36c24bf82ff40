"""Gaze meters between ranks: two fresh child processes share cuda:0 over gloo (as tests/test_gpu_dist.py does), each feeds
its half of every fixture batch to a metrics.GazeMeter, which all-gathers the per-frame counts and labels; both ranks' meter
states must equal a single-process meter fed the whole (concatenated) batches -- what the reference gets from gathering the
predictions (tools/train_avgaze_net.py:114,194)."""
import json
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


@pytest.mark.parametrize("mode", ["train", "val"])
def test_two_rank_meters_equal_the_single_process_meter(tmp_path, mode):
    from csts_amd import metrics
    world, port = 2, _free_port()
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "gaze_meter_worker.py"), str(r), str(world), port, outs[r], mode],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=300)
            logs.append(out)
    finally:
        for p in procs:                      # exactly the children started above
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed (code {p.returncode}):\n{logs[r][-4000:]}"
    z = np.load(os.path.join(ROOT, "tests", "golden", "gaze_meters.npz"))
    meta = json.loads(str(z["meta"]))
    dev = torch.device("cuda:0")
    single = metrics.GazeMeter(meta["datasets"][0], meta["window"], dev, mode)
    for i in range(z["preds"].shape[0]):
        single.update(*(torch.from_numpy(z[k][i]).to(dev) for k in ("preds", "labels_hm", "labels")), world=1)
    want = single.state.cpu().numpy()
    assert single.iterations() == z["preds"].shape[0]
    for o in outs:
        assert np.array_equal(np.load(o)["state"], want)
