"""Gaze meters on the device: metrics.GazeMeter (csts_f1_counts + csts_gaze_meter_update) against the values the reference's
TrainGazeMeter / ValGazeMeter / TestGazeMeter logged (tests/golden/gaze_meters.npz, tools/gen_golden_meters.py) and against
the host twin of the same rule; the update inside a HIP graph; the meter inside the captured training step.

Tolerance against the reference: 2e-6 absolute on f1 / recall / precision (the bound of test_adaptive_f1_on_device), thresholds
to 1e-12.  Device state against the host twin: integers and the fp32 ring bit for bit, fp64 sums to 1e-12 relative (the kernel
and the host function are one function: same operations, same order, one owner per word)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from test_gaze_meters_host import FIXTURE, TOL, TOL_THR, counts_of, load_fixture

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import metrics           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def dev_batches(z):
    return [tuple(torch.from_numpy(z[k][i]).to(DEV) for k in ("preds", "labels_hm", "labels")) for i in range(z["preds"].shape[0])]


def same_state(dev_meter, host_meter):
    a, b = dev_meter._fields(), host_meter._fields()
    assert a[0] == b[0] and a[1] == b[1]                                    # iterations, tracked frames
    assert np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))       # the ring, bit for bit
    for x, y in ((a[2], b[2]), (a[3], b[3])):                               # fp64 totals and per-threshold sums
        assert np.all(np.abs(x - y) <= 1e-12 * np.abs(y)), (x, y)


@pytest.mark.parametrize("mode", ["train", "val", "test"])
@pytest.mark.parametrize("di", [0, 1, 2])
def test_device_meter_equals_reference_and_host_twin(di, mode):
    z, meta = load_fixture()
    dataset = meta["datasets"][di]
    logged = json.loads(str(z[f"d{di}_logged"]))
    m = metrics.GazeMeter(dataset, meta["window"], DEV, mode)
    h = metrics.HostGazeMeter(dataset, meta["window"], mode)
    med = z[f"d{di}_median_train" if mode == "train" else f"d{di}_median_val"]
    per_batch = z[f"d{di}_per_batch"]
    thr = metrics.thresholds_for(dataset)
    for i, (p, q, lab) in enumerate(dev_batches(z)):
        m.update(p, q, lab)
        want = counts_of(z["preds"][i], z["labels_hm"][i], thr)
        assert np.array_equal(m._counts[("local", want.shape[0])].cpu().numpy(), want)       # the count launch alone
        h.update_counts(want, z["labels"][i], batch_size=p.shape[0])
        got = m.window_median()
        assert np.abs(np.array([got["f1"], got["recall"], got["precision"]]) - med[i, :3]).max() <= TOL
        assert abs(got["threshold"] - med[i, 3]) <= TOL_THR
        last = m.last_batch()
        assert np.abs(np.array(last[:3]) - per_batch[i, :3]).max() <= TOL and abs(last[3] - per_batch[i, 3]) <= TOL_THR
        same_state(m, h)
    if mode in ("train", "val"):
        ep, want = m.epoch_stats(), [r for r in logged if r.get("_type") == f"{mode}_epoch"][0]
    else:
        ep, want = m.dataset_stats(), [r for r in logged if r.get("split") == "test_final"][0]
        assert abs(ep["threshold"] - want["threshold"]) <= TOL_THR
    for k in ("f1", "recall", "precision"):
        assert abs(ep[k] - want[k]) <= TOL, (k, ep[k], want[k])
    m.reset()
    assert m.iterations() == 0 and not m.state.any()


def test_nan_rule_and_adaptive_f1_agree_on_the_device():
    z, meta = load_fixture()
    dataset = meta["datasets"][0]
    m = metrics.GazeMeter(dataset, meta["window"], DEV, "val")
    p, q, lab = (torch.from_numpy(z[k]).to(DEV) for k in ("nan_preds", "nan_labels_hm", "nan_labels"))
    m.update(p, q, lab)
    assert all(np.isnan(v) for v in m.last_batch()[:3])
    for p, q, lab in dev_batches(z)[:3]:
        m.update(p, q, lab)
        a, b = m.last_batch(), metrics.adaptive_f1(p, q, lab, dataset, rescale=True)
        assert a[:3] == b[:3] and a[3] == b[3]            # the same fp32 arithmetic in both finish rules


def test_update_captured_in_a_graph_and_replayed_equals_eager_updates():
    z, meta = load_fixture()
    dataset = meta["datasets"][0]
    batches = dev_batches(z)[:7]
    eager = metrics.GazeMeter(dataset, meta["window"], DEV, "val")
    for p, q, lab in batches:
        eager.update(p, q, lab)
    m = metrics.GazeMeter(dataset, meta["window"], DEV, "val")
    static = [t.clone() for t in batches[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(*static)                                  # warm-up: the count buffer is allocated outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.update(*static)
    torch.cuda.synchronize()
    assert m.iterations() == 0                             # a capture executes nothing
    for b in batches:
        for s, t in zip(static, b):
            s.copy_(t)
        g.replay()                                         # no argument changes: the iteration counter lives in the state buffer
    torch.cuda.synchronize()
    assert m.iterations() == 7 > meta["window"]
    assert torch.equal(m.state, eager.state)


def test_graphed_train_step_with_a_meter():
    """T = 8, b = 2, three replays: the losses equal those of a meter-less captured step on the same seed exactly, and the
    meter's per-batch values equal adaptive_f1 on the predictions of the same replay."""
    from conftest import GOLDEN  # noqa: F401
    from oracle import csts_oracle as O
    from csts_amd.build import build_model
    from csts_amd.config import load_yaml
    from csts_amd import train as T
    cfg = load_yaml(os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml"),
                    ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", 8, "CSTS_AMD.COMPUTE", "bf16"])
    m1 = build_model(cfg)
    m1.load_state_dict(O.seeded_params(8, 256), strict=True)
    m1.eval()
    m2 = copy.deepcopy(m1)
    batch = T.synthetic_batch(2, 8, 256, 99, DEV)
    batch["labels"][:, ::3, 2] = 1.0                       # a mix of gaze types: frames 0, 3, 6 of each clip are not fixations
    meter = metrics.GazeMeter(cfg.TRAIN.DATASET, 2, DEV, "train")
    lr = 1e-4
    torch.manual_seed(5)
    plain = T.GraphedTrainStep(cfg, m1, T.construct_optimizer(m1, cfg, capturable=True), batch, warmup=1)
    l1 = [[float(v) for v in plain.run(batch, lr)] for _ in range(3)]
    torch.manual_seed(5)
    step = T.GraphedTrainStep(cfg, m2, T.construct_optimizer(m2, cfg, capturable=True), batch, warmup=1, meter=meter)
    assert meter.iterations() == 0                         # the warm-up iteration was undone
    l2 = []
    for i in range(3):
        l2.append([float(v) for v in step.run(batch, lr)])
        got = meter.last_batch()
        want = metrics.adaptive_f1(step.preds, batch["labels_hm"], batch["labels"], cfg.TRAIN.DATASET, rescale=True)
        print(f"replay {i}: loss {l2[-1][0]:.6f} f1 {got[0]:.6f} recall {got[1]:.6f} precision {got[2]:.6f} threshold {got[3]:.4f}")
        assert got[:3] == want[:3] and got[3] == want[3]
        assert 0.0 <= got[0] <= 1.0
    assert l1 == l2, (l1, l2)
    assert meter.iterations() == 3 and meter.epoch_stats()["samples"] == 6.0
    assert "labels" in step.static and "labels" not in plain.static
