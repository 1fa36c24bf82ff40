"""GazePredictor.predict_video on a small synthetic recording against the composition of the existing pieces: per window,
predict() on the gathered frames with the plan's audio centres, then the float64 mean per target frame.  Random weights, the
Ego4D forecast YAML, fp32 compute.  200 frames of 64 x 80 with a matching 24 kHz waveform; stride 16 gives 8 windows and
batch=3 leaves a padded last batch.

Bounds (those of tests/test_gpu_gaze_track.py): heatmaps rel-L2 <= 1e-6 per covered frame, rescaled 1e-5 absolute, peak 1e-6
relative, count exact, points equal on every frame whose float64 top-two values differ by more than 1e-5 relative (closer
frames may be left out, at most 1 % of them)."""
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

from csts_amd import GazePredictor, plan_video  # noqa: E402
from csts_amd import inputs  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 200, 64, 80, 16, 3


def make_video(seed=21):
    """Seeded uint8 noise frames and a Gaussian waveform of the matching length (800 samples a frame at 24 kHz, 30 fps)."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 24000 // 30, generator=g)
    return frames, wav


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    frames, wav = make_video()
    frames, wav = frames.to(DEV), wav.to(DEV)
    graphed = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH)
    return {"cfg": cfg, "predictor": predictor, "frames": frames, "wav": wav, "graphed": graphed}


def test_equals_the_composition_of_existing_pieces(run):
    cfg, predictor, frames, wav, got = run["cfg"], run["predictor"], run["frames"], run["wav"], run["graphed"]
    T = cfg.DATA.NUM_FRAMES
    cols = inputs.stft_logpower(wav[None]).shape[2]
    plan = plan_video(cfg, N, stride=STRIDE, cols=cols)
    assert plan["windows"] == 8 == got["windows"] and plan["windows"] % BATCH != 0
    # per window: predict() on the gathered frames; frames_idx = the plan's centres on a time axis of `cols` positions, so
    # that predict()'s round(idx / frame_length * cols) is the centre itself (centres are inside its clip range)
    heat = torch.zeros(N, 64 * 64, dtype=torch.float64)
    count = torch.zeros(N, dtype=torch.int64)
    for w in range(plan["windows"]):
        clip = frames[torch.from_numpy(plan["frames_idx"][w]).long().to(DEV)][None]
        cen = torch.from_numpy(plan["audio_centers"][w]).float().to(DEV)[None]
        out = predictor.predict(clip, wav[None], cen, float(cols))
        maps = out["heatmaps"][0].cpu().double().reshape(T, -1)
        for t, f in enumerate(plan["target_idx"][w].tolist()):
            if f < N:
                heat[f] += maps[t]
                count[f] += 1
    hist = np.bincount(plan["target_idx"].reshape(-1)[plan["target_idx"].reshape(-1) < N], minlength=N)
    assert np.array_equal(count.numpy(), hist) and torch.equal(got["count"].cpu().long(), count)
    assert got["count"].dtype == torch.int32
    covered = count > 0
    assert 0 < int(covered.sum()) < N
    heat = heat / count.clamp(min=1)[:, None]
    mn, mx = heat.min(dim=-1, keepdim=True).values, heat.max(dim=-1, keepdim=True).values
    resc = (heat - mn) / (mx - mn + 1e-6)
    top = heat.topk(2, dim=-1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5 * top[:, 0]
    idx = heat.argmax(dim=-1)
    points = torch.stack([(idx % 64).float() / 64, torch.div(idx, 64, rounding_mode="floor").float() / 64], dim=-1)
    assert got["heatmaps"].shape == (N, 64, 64) and got["rescaled"].shape == (N, 64, 64)
    assert got["points"].shape == (N, 2) and got["peak"].shape == (N,)
    got_h = got["heatmaps"].cpu().double().reshape(N, -1)
    rel = ((got_h - heat).norm(dim=-1) / heat.norm(dim=-1).clamp(min=1e-300))[covered]
    e_resc = float((got["rescaled"].cpu().double().reshape(N, -1) - resc)[covered].abs().max())
    e_peak = float(((got["peak"].cpu().double() - mx[:, 0]).abs() / mx[:, 0].clamp(min=1e-300))[covered].max())
    judged = covered & clear
    left_out = int((covered & ~clear).sum())
    off = int((got["points"].cpu()[judged] != points[judged]).any(dim=-1).sum())
    print(f"predict_video: {int(covered.sum())} covered frames, heatmaps rel-L2 max {float(rel.max()):.3e}, rescaled abs "
          f"{e_resc:.3e}, peak rel {e_peak:.3e}, points off {off}, left out {left_out}")
    assert float(rel.max()) <= 1e-6
    assert e_resc <= 1e-5
    assert e_peak <= 1e-6
    assert left_out <= 0.01 * int(covered.sum())
    assert off == 0
    # frames no window predicts
    assert bool(torch.isnan(got["points"].cpu()[~covered]).all()) and bool(torch.isfinite(got["points"].cpu()[covered]).all())
    assert float(got["heatmaps"].cpu()[~covered].abs().max()) == 0.0 and float(got["peak"].cpu()[~covered].abs().max()) == 0.0


def test_graph_and_eager_agree_bit_for_bit_and_maps_can_be_left_out(run):
    predictor, frames, wav, graphed = run["predictor"], run["frames"], run["wav"], run["graphed"]
    assert predictor.graph and len(predictor._steps) >= 1
    predictor.graph = False
    try:
        eager = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH)
        small = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, return_heatmaps=False)
    finally:
        predictor.graph = True
    assert set(eager) == set(graphed) == {"points", "peak", "count", "heatmaps", "rescaled", "windows"}
    for k in ("points", "peak", "count", "heatmaps", "rescaled"):
        assert torch.equal(eager[k].nan_to_num(-1.0), graphed[k].nan_to_num(-1.0)), k
    assert set(small) == {"points", "peak", "count", "windows"}
    assert torch.equal(small["points"].nan_to_num(-1.0), eager["points"].nan_to_num(-1.0)) and torch.equal(small["peak"], eager["peak"])


def test_inputs_are_validated(run):
    predictor, frames, wav = run["predictor"], run["frames"], run["wav"]
    with pytest.raises(ValueError, match="observes 86"):
        predictor.predict_video(frames[:80], wav, stride=STRIDE)
    with pytest.raises(ValueError):
        predictor.predict_video(frames[None], wav)
    with pytest.raises(ValueError):
        predictor.predict_video(frames, wav[None])
    with pytest.raises(ValueError, match="257"):
        predictor.predict_video(frames, wav[:40000], stride=STRIDE)       # too little audio for a window's slice
    from csts_amd import lib
    with pytest.raises(lib.CstsError):
        predictor.predict_video(frames.cpu(), wav)
