"""GazePredictor.render_track and predict_video(overlay=True) on the small recording of tests/test_gpu_predict_video.py (200
frames of 64 x 80, stride 16, batch 3, random weights, fp32): the overlay of predict_video is render_track of its own track bit
for bit, chunking changes nothing, frames no window predicts come back untouched, points_source is the float64 formula."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from csts_amd import GazePredictor, inputs, marker_centers, ops, points_to_source  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 200, 64, 80, 16, 3
TODAY = {"points", "peak", "count", "heatmaps", "rescaled", "windows"}


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    g = torch.Generator().manual_seed(21)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    wav = (0.1 * torch.randn(N * 24000 // 30, generator=g)).to(DEV)
    track = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, overlay=True)
    return {"cfg": cfg, "predictor": predictor, "frames": frames, "wav": wav, "track": track}


def test_overlay_adds_two_keys_and_equals_render_track(run):
    predictor, frames, track = run["predictor"], run["frames"], run["track"]
    assert set(track) == TODAY | {"points_source", "overlay"}
    assert track["overlay"].dtype == torch.uint8 and track["overlay"].shape == frames.shape
    again = predictor.render_track(frames, track)
    assert torch.equal(again, track["overlay"])
    covered = track["count"] > 0
    assert 0 < int(covered.sum()) < N
    assert torch.equal(track["overlay"][~covered], frames[~covered])                  # nobody predicts them: untouched
    assert bool((track["overlay"][covered] != frames[covered]).flatten(1).any(dim=1).all())
    # the same pixels as the op itself under the row predict_video sampled with, and a green disc centre on every covered frame
    S = int(run["cfg"].DATA.TEST_CROP_SIZE)
    row = predictor._video_params_row(H, W)
    centers = marker_centers(track["points_source"], H, W)
    direct = ops.gaze_overlay(frames, track["rescaled"], row, S, centers=centers)
    assert torch.equal(direct, track["overlay"])
    idx = covered.nonzero().flatten()
    px = track["overlay"][idx, centers[idx, 1].long(), centers[idx, 0].long()]
    assert bool((px == torch.tensor([0, 255, 0], dtype=torch.uint8, device=DEV)).all())


def test_chunked_and_in_place_equal_the_whole(run):
    predictor, frames, track = run["predictor"], run["frames"], run["track"]
    for chunk in (1, 7, 64, 500):
        assert torch.equal(predictor.render_track(frames, track, chunk=chunk), track["overlay"]), chunk
    work = frames.clone()
    assert predictor.render_track(work, track, out=work, chunk=33) is work and torch.equal(work, track["overlay"])
    other = predictor.render_track(frames, track, alpha=0.25, radius=2)
    assert not torch.equal(other, track["overlay"])


def test_points_source_is_the_float64_formula(run):
    cfg, track = run["cfg"], run["track"]
    S = int(cfg.DATA.TEST_CROP_SIZE)
    import numpy as np
    nh, nw, y0, x0, flip = inputs.spatial_rule_host(np.zeros((1, 1, 2)), H, W, S, train=False, spatial_idx=1)[0][0].tolist()
    assert (nh, flip) == (S, 0) and nw > S
    p = track["points"].cpu().double()
    want = torch.stack([(p[:, 0] * S + x0) / nw, (p[:, 1] * S + y0) / nh], dim=-1)
    got = track["points_source"].cpu()
    assert got.dtype == torch.float64 and got.shape == (N, 2)
    covered = (track["count"] > 0).cpu()
    assert torch.equal(got[covered], want[covered]) and bool(torch.isnan(got[~covered]).all())
    assert torch.equal(points_to_source(track["points"], [nh, nw, y0, x0, flip], S).cpu().nan_to_num(-1.0), got.nan_to_num(-1.0))
    assert bool(((got[covered] >= 0) & (got[covered] < 1)).all())


def test_without_overlay_the_keys_are_todays_and_a_track_without_maps_is_refused(run):
    predictor, frames, wav, track = run["predictor"], run["frames"], run["wav"], run["track"]
    plain = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH)
    assert set(plain) == TODAY
    for k in ("points", "peak", "count", "heatmaps", "rescaled"):
        assert torch.equal(plain[k].nan_to_num(-1.0), track[k].nan_to_num(-1.0)), k
    small = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, return_heatmaps=False, overlay=True)
    assert set(small) == {"points", "peak", "count", "windows", "points_source", "overlay"}
    assert torch.equal(small["overlay"], track["overlay"])
    with pytest.raises(ValueError, match="rescaled"):
        predictor.render_track(frames, {k: v for k, v in plain.items() if k != "rescaled"})
    with pytest.raises(ValueError):
        predictor.render_track(frames[:50], plain)
    from csts_amd import lib
    with pytest.raises(lib.CstsError):
        predictor.render_track(frames.cpu(), plain)
