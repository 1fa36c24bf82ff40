"""One rank of tests/test_gpu_gaze_meters_dist.py: feeds its half of every fixture batch to a metrics.GazeMeter over a gloo
process group on cuda:0 and saves the meter state.   argv: rank world port out.npz mode"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csts_amd import metrics           # noqa: E402


def main():
    rank, world, port, out, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    try:
        dev = torch.device("cuda:0")
        z = np.load(os.path.join(ROOT, "tests", "golden", "gaze_meters.npz"))
        import json
        meta = json.loads(str(z["meta"]))
        m = metrics.GazeMeter(meta["datasets"][0], meta["window"], dev, mode)
        per = z["preds"].shape[1] // world
        for i in range(z["preds"].shape[0]):
            p, q, lab = (torch.from_numpy(z[k][i][rank * per:(rank + 1) * per]).to(dev) for k in ("preds", "labels_hm", "labels"))
            m.update(p, q, lab)
        torch.cuda.synchronize()
        np.savez(out, state=m.state.cpu().numpy())
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
