"""GazePredictor.predict_video(attention_track=True) on a small synthetic recording: the gaze track keeps its bits, a frame one
(window, input frame) pair shows carries predict(attention=True)'s maps of that pair, graph and eager agree, the fill runs on the
mixed maps and rescales afterwards, and render_attention_track draws what it says.  Random weights, the Ego4D forecast YAML, fp32
compute.  200 frames of 64 x 80 with a matching 24 kHz waveform; stride 16 gives 8 windows, batch=3 a padded last batch."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import overlay_reference as OR  # noqa: E402
from csts_amd import GazePredictor, default_attention_gap, fill_attention_track, fill_plan, plan_video  # noqa: E402
from csts_amd import inputs, ops  # noqa: E402
from csts_amd.config import load_yaml  # noqa: E402

DEV = torch.device("cuda:0")
YAML = os.path.join(ROOT, "configs/Ego4D/CSTS_Ego4D_Gaze_Forecast.yaml")
N, H, W, STRIDE, BATCH = 200, 64, 80, 16, 3
GAZE = ("points", "peak", "count", "heatmaps", "rescaled")
ATT = ("attention_maps", "attention_range", "attention_mixed", "attention_count", "temporal_attention_windows")
SYNTHETIC_SEED = 0        # chosen on the CPU: the close set of the float64 picture stays under overlay_reference's 1 % cap


def make_video(seed=21):
    """Seeded uint8 noise frames and a Gaussian waveform of the matching length (800 samples a frame at 24 kHz, 30 fps)."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    wav = 0.1 * torch.randn(N * 24000 // 30, generator=g)
    return frames, wav


def _same(a, b):
    if a.is_floating_point():
        return a.shape == b.shape and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0)) and torch.equal(a.isnan(), b.isnan())
    return a.shape == b.shape and torch.equal(a, b)


@pytest.fixture(scope="module")
def run():
    cfg = load_yaml(YAML, ["NUM_GPUS", 1, "CSTS_AMD.COMPUTE", "fp32"])
    torch.manual_seed(5)
    predictor = GazePredictor(cfg, device=DEV, graph=True)
    frames, wav = make_video()
    frames, wav = frames.to(DEV), wav.to(DEV)
    plain = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH)
    track = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, attention_track=True)
    cols = inputs.stft_logpower(wav[None]).shape[2]
    plan = plan_video(cfg, N, stride=STRIDE, cols=cols)
    return {"cfg": cfg, "predictor": predictor, "frames": frames, "wav": wav, "plain": plain, "track": track, "plan": plan,
            "cols": cols}


def test_the_gaze_track_keeps_its_bits_and_the_count_is_the_plans(run):
    plain, track, plan = run["plain"], run["track"], run["plan"]
    assert set(track) == set(plain) | set(ATT) | {"attention_crop_size"}
    for k in GAZE:
        assert _same(track[k], plain[k]), k
    flat = plan["frames_idx"].reshape(-1).astype(np.int64)
    want = np.bincount(flat[(flat >= 0) & (flat < N)], minlength=N)
    count = track["attention_count"]
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), want)
    # the inputs of a window lie 9 frames apart and the windows 16: no frame is shown twice here (frames several pairs land on
    # are the kernel test's, tests/test_gpu_attention_track.py), so every hit frame must carry the one-clip maps
    assert set(want.tolist()) == {0, 1}
    G, h, w = track["attention_maps"].shape[1:]
    assert track["attention_maps"].shape == track["attention_mixed"].shape == (N, G, h, w)
    assert track["attention_range"].shape == (N, G, 2)
    nwin = plan["windows"]
    tw = track["temporal_attention_windows"]
    assert nwin == 8 and nwin % BATCH != 0 and tw.dim() == 3 and tw.shape[0] == nwin and tw.shape[1] == tw.shape[2]
    hit = count > 0
    assert bool(torch.isnan(track["attention_range"][~hit]).all()) and bool(torch.isfinite(track["attention_range"][hit]).all())
    assert float(track["attention_maps"][~hit].abs().max()) == 0.0 and float(track["attention_mixed"][~hit].abs().max()) == 0.0


def test_a_frame_one_pair_shows_carries_the_one_clip_maps(run):
    """predict(attention=True) on each batch of windows as predict_video cut it (the last one padded by its last window):
    frames_idx = the plan's audio centres on a time axis of `cols` positions, so predict()'s round(idx / frame_length * cols)
    is the centre itself."""
    predictor, frames, wav, track, plan, cols = (run[k] for k in ("predictor", "frames", "wav", "track", "plan", "cols"))
    count = track["attention_count"].cpu().numpy()
    nwin, seen = plan["windows"], 0
    for w0 in range(0, nwin, BATCH):
        ws = [min(w0 + i, nwin - 1) for i in range(BATCH)]
        clip = frames[torch.from_numpy(plan["frames_idx"][ws].astype(np.int64)).to(DEV)]
        cen = torch.from_numpy(plan["audio_centers"][ws]).float().to(DEV)
        out = predictor.predict(clip, wav[None].expand(BATCH, -1).contiguous(), cen, float(cols), attention=True)
        assert torch.equal(out["temporal_attention"][:min(BATCH, nwin - w0)],
                           track["temporal_attention_windows"][w0:w0 + BATCH])
        for i, w in enumerate(ws[:min(BATCH, nwin - w0)]):
            for j, f in enumerate(plan["frames_idx"][w].tolist()):
                if 0 <= f < N and count[f] == 1:
                    assert torch.equal(track["attention_maps"][f], out["attention_maps"][i, :, j]), (w, j, f)
                    assert torch.equal(track["attention_range"][f], out["attention_range"][i, :, j]), (w, j, f)
                    seen += 1
    assert seen == int((count == 1).sum()) and seen > 0


def test_graph_and_eager_agree_bit_for_bit(run):
    predictor, frames, wav, track = run["predictor"], run["frames"], run["wav"], run["track"]
    assert predictor.graph and any(len(k) == 4 for k in predictor._steps)
    predictor.graph = False
    try:
        eager = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, attention_track=True)
    finally:
        predictor.graph = True
    assert set(eager) == set(track)
    for k in GAZE + ATT:
        assert _same(eager[k], track[k]), k


def test_linear_fill_blends_the_mixed_maps_and_rescales_afterwards(run):
    predictor, frames, wav, track, plan, plain = (run[k] for k in ("predictor", "frames", "wav", "track", "plan", "plain"))
    S = int(run["cfg"].DATA.TEST_CROP_SIZE)
    gap = default_attention_gap(plan)
    assert gap == 9
    filled = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, fill="linear", attention_track=True)
    gaze_only = predictor.predict_video(frames, wav, stride=STRIDE, batch=BATCH, fill="linear")
    assert set(filled) == set(gaze_only) | set(ATT) | {"attention_crop_size", "attention_neighbours", "attention_filled",
                                                         "attention_max_gap"}
    for k in GAZE + ("neighbours", "filled"):
        assert _same(filled[k], gaze_only[k]), k
    assert filled["attention_max_gap"] == gap and filled["max_gap"] == gaze_only["max_gap"]
    count = track["attention_count"]
    assert torch.equal(filled["attention_count"], count)
    hit = count > 0
    for k in ("attention_maps", "attention_range", "attention_mixed"):          # predicted frames keep their bits
        assert torch.equal(filled[k][hit], track[k][hit]), k
    nb = fill_plan(count.cpu().numpy(), gap)
    assert filled["attention_neighbours"].dtype == torch.int32
    assert np.array_equal(filled["attention_neighbours"].cpu().numpy().astype(np.int64), nb)
    is_filled = (count.cpu().numpy() == 0) & (nb[:, 0] >= 0)
    assert np.array_equal(filled["attention_filled"].cpu().numpy(), is_filled) and 0 < int(is_filled.sum())
    empty = (count.cpu().numpy() == 0) & ~is_filled
    assert int(empty.sum()) > 0
    empty_t = torch.from_numpy(empty).to(DEV)
    assert float(filled["attention_maps"][empty_t].abs().max()) == 0.0 and bool(torch.isnan(filled["attention_range"][empty_t]).all())
    # a filled frame: the fp32 blend of its neighbours' mixed maps (two products, one sum), then its own extrema
    mixed = track["attention_mixed"].cpu().numpy()
    n = np.flatnonzero(is_filled)
    a, b = nb[n, 0], nb[n, 1]
    wa = ((b - n).astype(np.float32) / (b - a).astype(np.float32))[:, None, None, None]
    wb = ((n - a).astype(np.float32) / (b - a).astype(np.float32))[:, None, None, None]
    blend = wa * mixed[a] + wb * mixed[b]
    assert blend.dtype == np.float32
    n_t = torch.from_numpy(n).to(DEV)
    assert np.array_equal(filled["attention_mixed"][n_t].cpu().numpy(), blend)
    want = ops.attention_rescale(torch.from_numpy(blend).to(DEV), S)
    assert torch.equal(filled["attention_maps"][n_t], want["maps"]) and torch.equal(filled["attention_range"][n_t], want["range"])
    # the same through the public function on the sparse track; the caller's gap overrides the default
    again = fill_attention_track(track, "linear", plan=plan)
    for k in ("attention_maps", "attention_range", "attention_mixed", "attention_neighbours", "attention_filled"):
        assert _same(again[k], filled[k]), k
    narrow = fill_attention_track(track, "hold", max_gap=1)
    assert not bool(narrow["attention_filled"].any()) and _same(narrow["attention_maps"], track["attention_maps"])
    with pytest.raises(ValueError):
        fill_attention_track(track, "linear")                         # neither max_gap nor plan
    with pytest.raises(ValueError):
        fill_attention_track(plain, "linear", plan=plan)              # no attention track in it
    big = {"attention_mixed": torch.ones(2, 3, 64, 64, device=DEV), "attention_count": torch.ones(2, dtype=torch.int32, device=DEV)}
    with pytest.raises(ValueError, match="CSTS_GAZE_DECODE_MAX_HW"):
        fill_attention_track(big, "linear", max_gap=2, crop_size=S)


def _centres(points, drawn, row, S, radius):
    """The marker centres render_attention_track states, on the host in float64."""
    nh, nw, y0, x0 = row[:4]
    cen = np.full((points.shape[0], 2), -1, dtype=np.int64)
    for n in range(points.shape[0]):
        if not drawn[n]:
            continue
        if np.isfinite(points[n]).all():
            cen[n] = [int(np.floor((points[n, 0] * S + x0) / nw * W)), int(np.floor((points[n, 1] * S + y0) / nh * H))]
        else:
            cen[n] = [W + radius + 1, 0]
    return cen


def synthetic_track(seed):
    """Six frames, two heads on an 8 x 8 grid: min-max rescaled softmax(randn / 2) maps as overlay_reference.make_case draws
    them.  Frame 1 is filled, frames 4 is neither hit nor filled (and has a point all the same), frames 2 and 5 are drawn
    without a point."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8)
    p = torch.softmax(torch.randn(6, 3, 64, generator=g) / 2, dim=-1)
    mn, mx = p.min(dim=-1, keepdim=True).values, p.max(dim=-1, keepdim=True).values
    maps = ((p - mn) / (mx - mn + 1e-6)).reshape(6, 3, 8, 8).contiguous()
    nan = float("nan")
    return {"frames": frames, "attention_maps": maps, "attention_count": torch.tensor([1, 0, 2, 1, 0, 1], dtype=torch.int32),
            "attention_filled": torch.tensor([False, True, False, False, False, False]),
            "points": torch.tensor([[0.5, 0.5], [0.25, 0.75], [nan, nan], [0.2, 0.7], [0.3, 0.3], [nan, nan]], dtype=torch.float32)}


@pytest.mark.parametrize("head", [None, 1])
def test_render_against_the_float64_picture(run, head):
    predictor = run["predictor"]
    S, radius = int(run["cfg"].DATA.TEST_CROP_SIZE), 5
    t = synthetic_track(SYNTHETIC_SEED)
    row = predictor._video_params_row(H, W)
    drawn = ((t["attention_count"] > 0) | t["attention_filled"]).numpy()
    g = 2 if head is None else head
    on_dev = {k: t[k].to(DEV) for k in ("attention_maps", "attention_count", "attention_filled")}
    frames = t["frames"].to(DEV)
    for points in (t["points"], None):
        pts = t["points"].numpy().astype(np.float64) if points is not None else np.full((6, 2), np.nan)
        cen = _centres(pts, drawn, row, S, radius)
        ref = OR.reference(t["frames"], t["attention_maps"][:, g], cen, row, S, radius=radius)
        got = predictor.render_attention_track(frames, on_dev, head=head, radius=radius,
                                               points=None if points is None else points.to(DEV), chunk=4)
        OR.compare(got, ref, f"attention track head {head} points {points is not None}")
        got = got.cpu().numpy()
        assert np.array_equal(got[~drawn], t["frames"].numpy()[~drawn])              # byte for byte, point or not
        green = (got == np.array([0, 255, 0], dtype=np.uint8)).all(axis=-1)
        ref_green = (ref["out"] == np.array([0, 255, 0], dtype=np.uint8)).all(axis=-1)
        no_point = drawn & ~np.isfinite(pts).all(axis=-1)
        assert int(no_point.sum()) >= 2 and not ref["marker"][no_point].any()
        assert not (green & ~ref_green & ~ref["close"])[no_point].any()            # no green the blend did not produce
        with_point = drawn & np.isfinite(pts).all(axis=-1)
        assert all(green[n, cen[n, 1], cen[n, 0]] for n in np.flatnonzero(with_point))
    whole = predictor.render_attention_track(frames, on_dev, head=head, radius=radius, points=t["points"].to(DEV))
    by_chunk = predictor.render_attention_track(frames, on_dev, head=head, radius=radius, points=t["points"].to(DEV), chunk=1)
    assert torch.equal(whole, by_chunk)


def test_render_on_the_recording_and_its_argument_checks(run):
    predictor, frames, track = run["predictor"], run["frames"], run["track"]
    hit = track["attention_count"] > 0
    out = predictor.render_attention_track(frames, track, points=track["points"], chunk=64)
    assert out.shape == frames.shape and out.dtype == torch.uint8
    assert torch.equal(out[~hit], frames[~hit])
    assert bool((out[hit] != frames[hit]).flatten(1).any(dim=1).all())
    with pytest.raises(ValueError):
        predictor.render_attention_track(frames, run["plain"])
    with pytest.raises(ValueError):
        predictor.render_attention_track(frames, track, head=track["attention_maps"].shape[1] - 1)
    with pytest.raises(ValueError):
        predictor.render_attention_track(frames[:10], track)
    with pytest.raises(ValueError):
        predictor.render_attention_track(frames, track, points=track["points"][:10])
    with pytest.raises(ValueError):
        predictor.render_attention_track(frames, track, chunk=0)
