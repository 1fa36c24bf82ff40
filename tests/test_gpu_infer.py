"""The inference path on the model (csts_amd/infer.py): the captured forward-only step replays exactly what the eager eval
forward computes, GazePredictor gives the same answer with and without the graph and from raw uint8 frames, and a saved
checkpoint reproduces the saving model's predictions in a predictor built under another seed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, GraphedEvalStep  # noqa: E402
from csts_amd import checkpoint as ck, inputs, ops, train as T  # noqa: E402
from csts_amd.build import build_model  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.infer import eval_forward  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
FRAMES = 8
KEYS = ("points", "peak", "heatmaps", "rescaled")


def _cfg(*extra):
    return load_yaml(YAML, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", FRAMES, "CSTS_AMD.COMPUTE", "bf16"] + list(extra))


class _NoOptimizer:
    """save_checkpoint writes optimizer.state_dict(); inference needs none of it (and AdamW moments would triple the file)."""

    def state_dict(self):
        return {}


def _eager(model, batch):
    was = model.training
    model.eval()
    with torch.no_grad():
        out = eval_forward(model, batch["video"], batch["audio"])
    model.train(was)
    return {k: v.clone() for k, v in out.items()}


def _raw_clip(B, seed, hw=(256, 256)):
    g = torch.Generator(device=DEV).manual_seed(seed)
    frames = torch.randint(0, 256, (B, FRAMES, hw[0], hw[1], 3), generator=g, device=DEV, dtype=torch.uint8)
    wav = 0.1 * torch.randn(B, 24000 * 5, generator=g, device=DEV)
    idx = (torch.arange(FRAMES, device=DEV, dtype=torch.float32) + 0.5)[None].expand(B, FRAMES).contiguous()
    labels = torch.cat([torch.rand(B, FRAMES, 2, generator=g, device=DEV), torch.zeros(B, FRAMES, 1, device=DEV)], dim=-1)
    return frames, wav, idx, labels


def test_graphed_eval_step_replays_the_eager_forward():
    cfg = _cfg()
    torch.manual_seed(3)
    model = build_model(cfg)
    model.train()                                              # the capture must put the flag back
    before = [p.detach().clone() for p in model.parameters()]
    b1 = T.synthetic_batch(2, FRAMES, 256, 41, DEV)
    b2 = T.synthetic_batch(2, FRAMES, 256, 42, DEV)
    step = GraphedEvalStep(cfg, model, b1)
    assert model.training
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    for b in (b1, b2, b1):                                     # a second run with a different batch, and back
        got = step.run(b["video"], b["audio"])
        want = _eager(model, b)
        assert set(got) == {"logits", "preds", "rescaled", "points", "peak"}
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert got["logits"].shape == (2, 1, FRAMES, 64, 64) and got["points"].shape == (2, FRAMES, 2)
        assert model.training
    assert not torch.equal(_eager(model, b1)["logits"], _eager(model, b2)["logits"])
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    # the head of the graph is the head of the drivers: frame_softmax at temperature 2, then the metric's rescale
    p = ops.frame_softmax(got["logits"], 2.0)
    assert float((got["preds"].double() - p.double()).norm() / p.double().norm()) < 1e-5
    with pytest.raises(ValueError):
        step.run(b1["video"][:1], b1["audio"][:1])
    # an out-of-band weight change reaches the replay (the 16-bit shadows follow the masters)
    with torch.no_grad():
        for prm in model.parameters():
            prm.mul_(1.01)
    got = step.run(b1["video"], b1["audio"])
    want = _eager(model, b1)
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_predictor_graph_equals_eager_and_raw_frames_equal_the_assembled_batch():
    cfg = _cfg()
    torch.manual_seed(4)
    graphed = GazePredictor(cfg, device=DEV, graph=True)
    eager = GazePredictor(cfg, device=DEV, graph=False)
    eager.model.load_state_dict(graphed.model.state_dict())
    assert not graphed.model.training and graphed.checkpoint_path is None
    batch = T.synthetic_batch(2, FRAMES, 256, 43, DEV)
    a, b = graphed.predict_batch(batch), eager.predict_batch(batch)
    assert set(a) == set(b) == set(KEYS)
    assert a["points"].shape == (2, FRAMES, 2) and a["peak"].shape == (2, FRAMES) and a["heatmaps"].shape == a["rescaled"].shape == (2, FRAMES, 64, 64)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    # results are the caller's: another call (other batch size: another graph) does not overwrite them
    keep = {k: v.clone() for k, v in a.items()}
    one = graphed.predict_batch(T.synthetic_batch(1, FRAMES, 256, 44, DEV))
    assert one["points"].shape == (1, FRAMES, 2) and sorted(graphed._steps) == [(1, FRAMES, 256), (2, FRAMES, 256)]
    assert all(torch.equal(a[k], keep[k]) for k in KEYS)
    # points are the arg-max cells of the heat maps, peak their value
    hm = a["heatmaps"].reshape(2 * FRAMES, -1)
    idx = hm.argmax(dim=-1)
    assert torch.equal(hm.max(dim=-1).values, a["peak"].reshape(-1))
    assert torch.equal(a["points"].reshape(-1, 2), torch.stack([(idx % 64).float() / 64, (idx // 64).float() / 64], dim=-1))
    # from uint8 frames + waveform
    frames, wav, fidx, labels = _raw_clip(2, 45)
    for pred in (graphed, eager):
        got = pred.predict(frames, wav, fidx, float(FRAMES))
        want = pred.predict_batch(inputs.assemble_batch(frames, wav, fidx, float(FRAMES), labels))
        assert set(got) == set(KEYS) and all(torch.equal(got[k], want[k]) for k in KEYS)
    # a larger source goes through the test-mode centre crop, labels carried along
    frames, wav, fidx, labels = _raw_clip(2, 46, hw=(300, 400))
    got = graphed.predict(frames, wav, fidx, float(FRAMES), labels=labels)
    ref = inputs.assemble_batch(frames, wav, fidx, float(FRAMES), labels, spatial=dict(crop_size=256, train=False, spatial_idx=1))
    want = graphed.predict_batch(ref)
    assert all(torch.equal(got[k], want[k]) for k in KEYS) and torch.equal(got["labels"], ref["labels"])


def test_checkpoint_reproduces_the_saving_model_under_another_seed(tmp_path):
    cfg = _cfg()
    torch.manual_seed(5)
    model = build_model(cfg)
    batch = T.synthetic_batch(2, FRAMES, 256, 47, DEV)
    want = _eager(model, batch)
    path = ck.save_checkpoint(str(tmp_path), model, _NoOptimizer(), 0, cfg)
    try:
        del model
        torch.manual_seed(77)
        fresh = GazePredictor(cfg, device=DEV, graph=False).predict_batch(batch)
        assert not torch.equal(fresh["heatmaps"], want["preds"].squeeze(1))           # another seed: other weights
        torch.manual_seed(78)
        pred = GazePredictor(cfg, path, device=DEV)
        assert pred.checkpoint_path == path
        got = pred.predict_batch(batch)
        assert torch.equal(got["points"], want["points"]) and torch.equal(got["heatmaps"], want["preds"].squeeze(1))
        assert torch.equal(got["rescaled"], want["rescaled"].squeeze(1)) and torch.equal(got["peak"], want["peak"])
        # TEST.CHECKPOINT_FILE_PATH is the fallback when no path is given
        torch.manual_seed(79)
        pred2 = GazePredictor(_cfg("TEST.CHECKPOINT_FILE_PATH", path), device=DEV, graph=False)
        assert pred2.checkpoint_path == path and torch.equal(pred2.predict_batch(batch)["points"], want["points"])
    finally:
        os.remove(path)                                                              # 0.75 GB
