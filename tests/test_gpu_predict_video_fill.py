"""GazePredictor.predict_video(fill=...) on the recording of tests/test_gpu_predict_video.py: 200 frames of 64 x 80, stride 16,
batch 3, fp32 compute, random weights, one predictor for the module.  fill=None is the sparse track as before; a fill mode is
csts_amd.fill_track of that track bit for bit, covers every frame between the first and the last prediction, leaves count as it
was, agrees between graph and eager runs, works without the maps and is what overlay=True draws."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, default_max_gap, fill_plan, fill_track, inputs, plan_video  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 200, 64, 80, 16, 3
SPARSE_KEYS = {"points", "peak", "count", "heatmaps", "rescaled", "windows"}
MAPS = ("heatmaps", "rescaled", "points", "peak")


def same(a, b):
    return torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).to(DEV)
    kw = {"stride": STRIDE, "batch": BATCH}
    sparse = predictor.predict_video(frames, wav, **kw)
    linear = predictor.predict_video(frames, wav, fill="linear", **kw)
    plan = plan_video(cfg, N, stride=STRIDE, cols=inputs.stft_logpower(wav[None]).shape[2])
    return {"predictor": predictor, "frames": frames, "wav": wav, "kw": kw, "sparse": sparse, "linear": linear, "plan": plan}


def test_without_a_mode_the_track_is_the_sparse_one(run):
    predictor, sparse = run["predictor"], run["sparse"]
    assert set(sparse) == SPARSE_KEYS
    again = predictor.predict_video(run["frames"], run["wav"], fill=None, **run["kw"])
    assert set(again) == SPARSE_KEYS and again["windows"] == sparse["windows"] == 8
    for k in MAPS + ("count",):
        assert same(again[k], sparse[k]), k
    count = sparse["count"].cpu()
    assert 0 < int((count > 0).sum()) < N and bool(torch.isnan(sparse["points"].cpu()[count == 0]).all())


def test_linear_equals_fill_track_of_the_sparse_track(run):
    sparse, linear, plan = run["sparse"], run["linear"], run["plan"]
    assert set(linear) == SPARSE_KEYS | {"neighbours", "filled", "max_gap"} and linear["max_gap"] == 9
    before = {k: sparse[k].clone() for k in MAPS + ("count",)}
    assert default_max_gap(plan) == 9
    for want in (fill_track(sparse, mode="linear", plan=plan), fill_track(sparse, mode="linear", max_gap=9)):
        assert set(want) == set(linear) and want["windows"] == linear["windows"] and want["max_gap"] == 9
        for k in MAPS + ("count", "neighbours", "filled"):
            assert same(want[k], linear[k]), k
    for k, v in before.items():                                        # the input is not modified
        assert same(sparse[k], v), k
    with pytest.raises(ValueError, match="max_gap"):
        fill_track(sparse)
    with pytest.raises(ValueError, match="heatmaps"):
        fill_track({"count": sparse["count"]}, max_gap=9)
    # a track read back from arrays and moved to the device
    loaded = {k: torch.from_numpy(sparse[k].cpu().numpy()).to(DEV) for k in ("heatmaps", "count")}
    again = fill_track(loaded, mode="linear", max_gap=9)
    assert set(again) == {"heatmaps", "rescaled", "points", "peak", "count", "neighbours", "filled", "max_gap"}
    assert all(same(again[k], linear[k]) for k in MAPS + ("neighbours", "filled"))


def test_count_stays_and_the_predicted_span_is_covered(run):
    sparse, linear = run["sparse"], run["linear"]
    count = sparse["count"].cpu()
    assert torch.equal(linear["count"].cpu(), count) and linear["count"].dtype == torch.int32
    nb = linear["neighbours"].cpu()
    assert nb.dtype == torch.int32 and tuple(nb.shape) == (N, 2)
    assert np.array_equal(nb.numpy().astype(np.int64), fill_plan(count.numpy(), 9))
    filled = linear["filled"].cpu()
    assert filled.dtype == torch.bool and torch.equal(filled, (count == 0) & (nb[:, 0] >= 0))
    predicted = (count > 0).nonzero().flatten()
    first, last = int(predicted[0]), int(predicted[-1])
    covered = (count > 0) | filled
    assert covered.nonzero().flatten().tolist() == list(range(first, last + 1))
    assert int(filled.sum()) == last + 1 - first - predicted.numel() > 0
    points = linear["points"].cpu()
    assert bool(torch.isfinite(points[covered]).all()) and bool(torch.isnan(points[~covered]).all())
    assert float(linear["heatmaps"].cpu()[~covered].abs().max()) == 0.0 and float(linear["peak"].cpu()[~covered].abs().max()) == 0.0
    sums = linear["heatmaps"].double().sum(dim=(1, 2)).cpu()[covered]
    assert float((sums - 1.0).abs().max()) <= 1e-5
    for k in MAPS:                                                     # predicted frames pass through
        assert same(linear[k].cpu()[count > 0], sparse[k].cpu()[count > 0]), k
    hold = run["predictor"].predict_video(run["frames"], run["wav"], fill="hold", **run["kw"])
    assert torch.equal(hold["neighbours"].cpu(), nb) and torch.equal(hold["filled"].cpu(), filled)
    a = nb[:, 0].long().clamp(min=0)
    for k in MAPS:
        assert same(hold[k].cpu()[covered], sparse[k].cpu()[a][covered]), k


def test_graph_and_eager_agree_and_the_maps_can_be_left_out(run):
    predictor, frames, wav, linear = run["predictor"], run["frames"], run["wav"], run["linear"]
    predictor.graph = False
    try:
        eager = predictor.predict_video(frames, wav, fill="linear", **run["kw"])
        small = predictor.predict_video(frames, wav, fill="linear", return_heatmaps=False, **run["kw"])
    finally:
        predictor.graph = True
    assert set(eager) == set(linear)
    for k in MAPS + ("count", "neighbours", "filled"):
        assert same(eager[k], linear[k]), k
    assert set(small) == {"points", "peak", "count", "windows", "neighbours", "filled", "max_gap"}
    assert same(small["points"], linear["points"]) and same(small["peak"], linear["peak"])
    assert bool(torch.isfinite(small["points"].cpu()[linear["filled"].cpu()]).all())
    with pytest.raises(ValueError):
        predictor.predict_video(frames, wav, fill="nearest", **run["kw"])
    with pytest.raises(ValueError):
        predictor.predict_video(frames, wav, max_gap=9, **run["kw"])
    narrow = predictor.predict_video(frames, wav, fill="linear", max_gap=1, return_heatmaps=False, **run["kw"])
    assert int(narrow["filled"].sum()) == 0 and narrow["max_gap"] == 1


def test_the_overlay_draws_the_filled_track(run):
    predictor, frames, wav, linear = run["predictor"], run["frames"], run["wav"], run["linear"]
    drawn = predictor.predict_video(frames, wav, fill="linear", overlay=True, **run["kw"])
    plain = predictor.predict_video(frames, wav, overlay=True, return_heatmaps=False, **run["kw"])
    assert set(drawn) == set(linear) | {"points_source", "overlay"}
    assert drawn["overlay"].shape == frames.shape and drawn["overlay"].dtype == torch.uint8
    n = int(linear["filled"].cpu().nonzero().flatten()[0])
    row = predictor._video_params_row(H, W)                              # (new h, new w, y0, x0, flip): the crop in source pixels
    S = int(predictor.cfg.DATA.TEST_CROP_SIZE)
    x0, x1 = -(-row[3] * W // row[1]) + 1, (row[3] + S) * W // row[1] - 1
    assert 0 < x0 < x1 < W
    inside = (slice(1, H - 1), slice(x0, x1))
    assert bool((drawn["overlay"][n][inside] != frames[n][inside]).any())
    assert torch.equal(plain["overlay"][n], frames[n])                   # the same frame of the sparse track: untouched
    assert torch.equal(drawn["overlay"], predictor.render_track(frames, linear))
    first = int((linear["count"] > 0).cpu().nonzero().flatten()[0])
    assert torch.equal(drawn["overlay"][:first], frames[:first])         # nothing is drawn before the first prediction
