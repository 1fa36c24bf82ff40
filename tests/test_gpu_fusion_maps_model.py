"""The fusion attention maps at model level: CSTS.forward(return_fusion_maps=True) on the seeded fp32 model against the fixture
captured from the reference (tests/golden/model_T8_B1_attn.npz), GazePredictor.predict_batch(attention=True) with and without
the graph, and GazePredictor.render_attention against ops.gaze_overlay."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2, GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import attention_reference as A  # noqa: E402
from csts_amd import GazePredictor, ops, train as T  # noqa: E402
from csts_amd.build import build_model  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402
from csts_amd.infer import ATTENTION_OUTPUTS, marker_centers, points_to_source  # noqa: E402
from oracle import csts_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
FRAMES = 8
KEYS = ("points", "peak", "heatmaps", "rescaled")
SHAPES = {"audio_attention": (8, 4, 8, 8), "audio_attention_mean": (4, 8, 8), "attention_maps": (9, FRAMES, 8, 8),
          "attention_range": (9, FRAMES, 2), "temporal_attention": (8, 8)}


def test_forward_flag_against_the_reference_fixture():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", FRAMES, "CSTS_AMD.COMPUTE", "fp32"])
    m = build_model(cfg)
    m.load_state_dict(O.seeded_params(FRAMES, 256), strict=True)
    m.eval()
    b1 = {k: v.to(DEV) for k, v in O.synthetic_batch(1, FRAMES, 256, seed=1001).items()}
    g = np.load(os.path.join(GOLDEN, "model_T8_B1_attn.npz"), allow_pickle=False)
    with torch.no_grad():
        plain = m([b1["video"]], b1["audio"])
        out = m([b1["video"]], b1["audio"], return_fusion_maps=True)
        full = m([b1["video"]], b1["audio"], return_spatial_attn=True, return_temporal_attn=True, return_fusion_maps=True)
    assert isinstance(out, list) and len(out) == 2 and torch.is_tensor(out[0]) and isinstance(out[1], dict)
    assert torch.equal(out[0], plain)                                             # the flag does not touch the logits
    fusion = out[1]
    assert set(fusion) == {"column", "column_mean", "maps", "range", "temporal"}
    for k, name in ATTENTION_OUTPUTS.items():
        assert tuple(fusion[name].shape) == (1,) + SHAPES[k] and fusion[name].dtype == torch.float32, k
    want = A.fixture_column()                                                     # (1, 8, 4, 8, 8), stored as fp16
    e_col = rel_l2(fusion["column"], want)
    e_tmp = rel_l2(fusion["temporal"], g["temporal_attn"].mean(axis=1))
    print(f"fusion maps: column against the fixture's slices rel-L2 {e_col:.3e}, temporal {e_tmp:.3e}")
    assert e_col < 3e-3
    assert e_tmp < 1e-4
    # the reference's flags keep their places and shapes beside the new one
    assert len(full) == 4 and torch.equal(full[0], plain)
    assert tuple(full[1].shape) == (1, 8, 260, 260) and tuple(full[2].shape) == (1, 8, 8, 8)
    assert all(torch.equal(full[3][k], fusion[k]) for k in fusion)
    cut = A.cut_column(full[1].cpu().numpy(), 4, 64).reshape(1, 8, 4, 8, 8)
    assert rel_l2(fusion["column"], cut) < 1e-5
    assert torch.equal(fusion["temporal"], full[2].mean(dim=1))


_PRED = {}


def _predictors():
    if not _PRED:
        cfg = load_yaml(YAML, ["NUM_GPUS", 1, "MODEL.LOSS_FUNC", "kldiv+egonce", "DATA.NUM_FRAMES", FRAMES, "CSTS_AMD.COMPUTE", "bf16"])
        torch.manual_seed(4)
        _PRED["graph"] = GazePredictor(cfg, device=DEV, graph=True)
        _PRED["eager"] = GazePredictor(cfg, device=DEV, graph=False)
        _PRED["eager"].model.load_state_dict(_PRED["graph"].model.state_dict())
        _PRED["batch"] = T.synthetic_batch(2, FRAMES, 256, 43, DEV)
        _PRED["result"] = _PRED["graph"].predict_batch(_PRED["batch"], attention=True)
    return _PRED


def test_predictor_attention_graph_equals_eager_and_leaves_the_gaze_alone():
    p = _predictors()
    graphed, eager, batch, a = p["graph"], p["eager"], p["batch"], p["result"]
    b = eager.predict_batch(batch, attention=True)
    assert set(a) == set(b) == set(KEYS) | set(ATTENTION_OUTPUTS)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k, shape in SHAPES.items():
        assert tuple(a[k].shape) == (2,) + shape and a[k].dtype == torch.float32, k
    plain = graphed.predict_batch(batch)
    assert set(plain) == set(KEYS)
    for k in KEYS:
        assert torch.equal(plain[k], a[k]), k
    assert sorted(graphed._steps, key=len) == [(2, FRAMES, 256), (2, FRAMES, 256, "attention")]
    # the results are the caller's: the next replay writes the graph's static buffers, not these
    keep = {k: v.clone() for k, v in a.items()}
    other = T.synthetic_batch(2, FRAMES, 256, 44, DEV)
    c = graphed.predict_batch(other, attention=True)
    want = eager.predict_batch(other, attention=True)
    assert all(torch.equal(a[k], keep[k]) for k in keep)
    assert all(torch.equal(c[k], want[k]) for k in want)
    assert not torch.equal(c["audio_attention"], a["audio_attention"]) and not torch.equal(c["temporal_attention"], a["temporal_attention"])
    # what the arrays are: probabilities, their head mean, maps rescaled by the range
    col = a["audio_attention"]
    assert bool((col > 0).all()) and bool((col < 1).all())
    assert float((a["temporal_attention"].sum(dim=-1) - 1).abs().max()) < 1e-4
    assert bool((a["attention_range"][..., 0] < a["attention_range"][..., 1]).all())


@pytest.mark.parametrize("hw", [(256, 256), (270, 360)])
def test_render_attention_is_one_gaze_overlay(hw):
    p = _predictors()
    pred, res = p["eager"], p["result"]
    H, W = hw
    frames = torch.randint(0, 256, (2, FRAMES, H, W, 3), generator=torch.Generator(device=DEV).manual_seed(7), device=DEV,
                           dtype=torch.uint8)
    row = pred._video_params_row(H, W)
    assert (row == [256, 256, 0, 0, 0]) == (hw == (256, 256))
    flat = frames.view(2 * FRAMES, H, W, 3)
    for head, g in ((None, 8), (3, 3)):
        got = pred.render_attention(frames, res, head=head)
        want = ops.gaze_overlay(flat, res["attention_maps"][:, g].reshape(2 * FRAMES, 8, 8), row, 256)
        assert got.shape == frames.shape and got.dtype == torch.uint8
        assert torch.equal(got.view_as(want), want)
        assert not torch.equal(got, frames)
    if hw != (256, 256):                                                         # outside the centre crop the frame stays
        assert torch.equal(got[:, :, :, :20], frames[:, :, :, :20]) and not torch.equal(got[:, :, :, 60:300], frames[:, :, :, 60:300])
    # a marker at the predicted gaze point, through the crop's geometry
    got = pred.render_attention(frames, res, head=None, points=res["points"], radius=4)
    centers = marker_centers(points_to_source(res["points"].reshape(-1, 2), row, 256), H, W)
    want = ops.gaze_overlay(flat, res["attention_maps"][:, 8].reshape(2 * FRAMES, 8, 8), row, 256, centers=centers, radius=4)
    assert torch.equal(got.view_as(want), want)
    assert bool((got.view_as(want)[0, int(centers[0, 1]), int(centers[0, 0])] == torch.tensor([0, 255, 0], device=DEV, dtype=torch.uint8)).all())
    # in place
    work = frames.clone()
    back = pred.render_attention(work, res, head=3, out=work)
    assert back.data_ptr() == work.data_ptr()
    assert torch.equal(work, pred.render_attention(frames, res, head=3))
    with pytest.raises(ValueError):
        pred.render_attention(frames, res, head=8)
    with pytest.raises(ValueError):
        pred.render_attention(frames, {k: res[k] for k in KEYS})
